"""Harness for tests/test_gpu_views_of_buffers.py: an entry point run on sample-aligned views of larger allocations, between guard bands.

The library's callers do not hand it whole allocations: a capture resident on the device is cut into frames at an arbitrary sample
(d_capture + 8 * k), one float32 row lies inside a larger grid, a PCM ring is written at a running offset.  include/pss.h ("pointer
alignment") promises such callers that a pointer aligned to one RECORD of its buffer is either served with the bytes a 256-byte-aligned
pointer gets, or refused with PSS_E_ARG before anything is launched; and that no call touches a byte outside its documented buffers or
writes its inputs.  This module checks exactly that, for any callable:

  arena of one pointer argument   [GUARD guard bytes][pad p][payload][GUARD guard bytes], the arena itself 256-byte aligned, p = 0 or one
                                  record.  GUARD = 4096: one stray 16-byte access by every lane of a 256-thread workgroup.
  inputs                          guards (and pad) are quiet-NaN words for float buffers, 0x7f bytes for integer codes
  outputs                         guards, pad AND payload start as 0x7f bytes (test_gpu_grid_caps.sentinel)
  calls                           A: every p = 0 (run twice: is the aligned call reproducible?)   B: inputs padded   C: outputs padded   D: both
  after every call                every input arena unchanged in every byte; every output guard unchanged;
                                  a SERVED call's payloads equal A's in every byte (an entry point that is not reproducible at A is held to
                                  the case's oracle criterion instead, and the report says so);
                                  a REFUSED call raised the case's `refusal` exception, passed `is_refusal`, and left the output arenas alone
  call A                          is also held to the case's oracle (Case.check), so B, C and D cannot be equal to A and wrong together

NumPy only; the device backend (DeviceArenas) uses torch for the allocation and the two copies, nothing else.  The host backend (HostArenas)
runs the same checks over NumPy "entry points": tests/test_view_harness.py seeds every fault the harness exists to find.
"""
import numpy as np

GUARD = 4096
ALIGN = 256
FILL = 0x7F
VARIANTS = (("A", False, False), ("B", True, False), ("C", False, True), ("D", True, True))

# record of each documented layout: bytes a valid pointer is aligned to (include/pss.h, "pointer alignment")
RECORDS = {"complex64": 8, "float32": 4, "float64": 8, "complex128": 8, "pcm16": 4, "int32": 4, "int8": 1, "uint8": 1, "int64": 8}
_NP = {"complex64": np.float32, "float32": np.float32, "float64": np.float64, "complex128": np.float64, "pcm16": np.int16, "int32": np.int32,
       "int8": np.int8, "uint8": np.uint8, "int64": np.int64}


# layouts in which an element of 0x7f bytes is a value a kernel may legitimately write (an int16 sample of 32 639, a byte of 127): the "never
# written" check cannot tell it from the fill and leaves these buffers to the case's oracle
NO_SENTINEL_CHECK = ("pcm16", "int8", "uint8")


class Arg:
    """One pointer argument.  layout: a key of RECORDS.  data: the input's values (an array of the layout's element type, complex arrays
    interleaved on the way in); shape: an output's element count or shape (complex128 outputs: give the interleaved shape [..., 2]).
    serve = False: the entry point refuses this argument at record alignment (the case then tests the refusal).
    sparse = True: an output the call documents as partly written (compacted lists, nullable rows); the 0x7f check is then left to the oracle."""

    def __init__(self, name, layout, data=None, shape=None, serve=True, sparse=False):
        assert layout in RECORDS, layout
        assert (data is None) != (shape is None), f"{name}: an input has data, an output has a shape"
        self.name, self.layout, self.serve, self.sparse = name, layout, serve, sparse
        self.record, self.dtype = RECORDS[layout], np.dtype(_NP[layout])
        self.is_input = data is not None
        if self.is_input:
            a = np.ascontiguousarray(data)
            if a.dtype.kind == "c":
                a = a.view(np.float32 if a.dtype == np.complex64 else np.float64)
            assert a.dtype == self.dtype, f"{name}: {a.dtype} data for a {layout} buffer"
            self.bytes = a.reshape(-1).view(np.uint8).copy()
            self.shape = a.shape
        else:
            self.shape = tuple(np.atleast_1d(shape).tolist())
            self.bytes = None
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        assert self.nbytes > 0 and self.nbytes % self.record == 0, f"{name}: {self.nbytes} bytes are no whole number of {self.record}-byte records"

    def image(self, pad):
        """The arena's bytes before the call."""
        total = GUARD + pad + self.nbytes + GUARD
        img = np.full(total, FILL, np.uint8)
        if self.is_input:
            if self.dtype.kind == "f":     # quiet NaNs: a guard word that reaches a result poisons it
                word = np.array([np.nan], self.dtype).view(np.uint8)
                for lo, hi in ((0, GUARD + pad), (GUARD + pad + self.nbytes, total)):
                    assert lo % len(word) == 0 and (hi - lo) % len(word) == 0
                    img[lo:hi] = np.tile(word, (hi - lo) // len(word))
            img[GUARD + pad:GUARD + pad + self.nbytes] = self.bytes
        return img


class View:
    """What a call receives for one argument: `ptr` (device backend: the payload's address), `array` (host backend: the payload as a NumPy
    view of the element type), and the arena around it (host backend: `arena`, uint8, the payload at arena[off:off + nbytes])."""

    def __init__(self, arg, pad, ptr=None, arena=None):
        self.arg, self.pad, self.off, self.nbytes, self.ptr, self.arena = arg, pad, GUARD + pad, arg.nbytes, ptr, arena
        self.array = None if arena is None else arena[self.off:self.off + self.nbytes].view(arg.dtype).reshape(arg.shape)


class HostArenas:
    """Arenas in host memory (the harness's own tests)."""

    def place(self, arg, pad, img):
        raw = np.empty(len(img) + ALIGN, np.uint8)
        s = (-raw.ctypes.data) % ALIGN
        arena = raw[s:s + len(img)]
        arena[:] = img
        assert arena.ctypes.data % ALIGN == 0
        return View(arg, pad, ptr=arena.ctypes.data + GUARD + pad, arena=arena), arena

    def fetch(self, handle):
        return handle.copy()

    def sync(self):
        pass


class DeviceArenas:
    """Arenas in device memory: one torch allocation each (torch hands out 512-byte-aligned blocks; checked)."""

    def __init__(self, sync):
        import torch
        self.torch, self._sync = torch, sync

    def place(self, arg, pad, img):
        t = self.torch.from_numpy(img).cuda()
        assert t.data_ptr() % ALIGN == 0, f"an allocation at {t.data_ptr():#x} is not {ALIGN}-byte aligned"
        return View(arg, pad, ptr=t.data_ptr() + GUARD + pad), t

    def fetch(self, handle):
        return handle.cpu().numpy()

    def sync(self):
        self._sync()


class Case:
    """One (entry point, kernel family) row.
    call(views): runs the entry point; views maps argument names to View.  check(outputs): the oracle criterion of call A (outputs maps the
    output names to arrays of their element type and shape), raising AssertionError.  setup / teardown: options around the four calls.
    refusal / is_refusal: the exception type a refused call raises and a predicate on the exception (PssError with PSS_E_ARG that names the argument)."""

    def __init__(self, entry, family, shape, args, call, check=None, setup=None, teardown=None, refusal=None, is_refusal=None, note=""):
        self.entry, self.family, self.shape, self.args, self.call, self.check = entry, family, shape, list(args), call, check
        self.setup, self.teardown, self.refusal, self.is_refusal, self.note = setup, teardown, refusal, is_refusal, note
        names = [a.name for a in self.args]
        assert len(set(names)) == len(names), f"{entry}: argument names repeat"

    @property
    def id(self):
        return f"{self.entry}-{self.family}-{self.shape}".replace(" ", "")

    def head(self):
        return f"{self.entry} [{self.family}] {self.shape}"

    def refused_args(self, pad_in, pad_out):
        return [a.name for a in self.args if not a.serve and (pad_in if a.is_input else pad_out)]

    def decisions(self):
        return sum(a.serve for a in self.args), sum(not a.serve for a in self.args)


class ViewFailure(AssertionError):
    pass


def _first_diff(got, want):
    d = np.nonzero(got != want)[0]
    return (int(d[0]), int(d.size)) if d.size else (None, 0)


def _where(off, view):
    """A byte of the arena, named relative to the payload."""
    rel = off - view.off
    if rel < 0:
        return f"byte {rel} relative to the payload (in the {'pad' if off >= GUARD else 'guard'} in front of it)"
    if rel >= view.nbytes:
        return f"byte {rel} relative to the payload ({rel - view.nbytes} into the guard behind it)"
    return f"byte {rel} of the payload (element {rel // view.arg.dtype.itemsize})"


class _Run:
    def __init__(self, which, views, before, after, raised):
        self.which, self.views, self.before, self.after, self.raised = which, views, before, after, raised

    def payload(self, name):
        v = self.views[name]
        return self.after[name][v.off:v.off + v.nbytes]

    def outputs(self):
        return {n: self.payload(n).view(v.arg.dtype).reshape(v.arg.shape) for n, v in self.views.items() if not v.arg.is_input}


def _run(case, backend, which, pad_in, pad_out):
    views, handles, before = {}, {}, {}
    for a in case.args:
        pad = a.record if (pad_in if a.is_input else pad_out) else 0
        img = a.image(pad)
        views[a.name], handles[a.name] = backend.place(a, pad, img)
        before[a.name] = img
    raised = None
    try:
        case.call(views)
    except Exception as ex:   # judged below: a refusal is an exception too
        raised = ex
    backend.sync()
    after = {n: backend.fetch(h) for n, h in handles.items()}
    return _Run(which, views, before, after, raised)


def _check_run(case, run, base, fails, by_oracle):
    """The four assertions on one call.  base: call A's run (None for A itself)."""
    tag = f"{case.head()}, call {run.which}"
    expect_refusal = case.refused_args(*[(pi, po) for w, pi, po in VARIANTS if w == run.which[0]][0])
    for name, v in run.views.items():
        b, a = run.before[name], run.after[name]
        if v.arg.is_input:
            off, cnt = _first_diff(a, b)
            if cnt:
                fails.append(f"{tag}: input {name} was WRITTEN: {cnt} bytes changed, first {_where(off, v)}: {b[off]:#04x} -> {a[off]:#04x}")
            continue
        guard = np.ones(len(a), bool)
        guard[v.off:v.off + v.nbytes] = False
        off, cnt = _first_diff(a[guard], b[guard])
        if cnt:
            off = int(np.nonzero(guard)[0][off])
            fails.append(f"{tag}: output {name}: {cnt} bytes OUTSIDE the buffer were written, first {_where(off, v)}: {a[off]:#04x}")
    if expect_refusal:
        ok = run.raised is not None and (case.refusal is None or isinstance(run.raised, case.refusal)) and \
            (case.is_refusal is None or case.is_refusal(run.raised, expect_refusal))
        if not ok:
            fails.append(f"{tag}: a refusal of {', '.join(expect_refusal)} was expected, got " +
                         ("a served call" if run.raised is None else f"{type(run.raised).__name__}: {run.raised}"))
        for name, v in run.views.items():
            if not v.arg.is_input:
                off, cnt = _first_diff(run.after[name], run.before[name])
                if cnt:
                    fails.append(f"{tag}: refused, yet output {name} was written: {cnt} bytes, first {_where(off, v)}")
        return
    if run.raised is not None:
        fails.append(f"{tag}: raised {type(run.raised).__name__}: {run.raised}")
        return
    for name, v in run.views.items():
        if v.arg.is_input or v.arg.sparse or v.arg.layout in NO_SENTINEL_CHECK:
            continue
        el = run.payload(name).reshape(-1, v.arg.dtype.itemsize)
        un = np.nonzero((el == FILL).all(axis=1))[0]
        if un.size:
            fails.append(f"{tag}: output {name}: {un.size} elements were never written (still 0x7f bytes), first {_where(v.off + int(un[0]) * el.shape[1], v)}")
    if base is None or by_oracle:
        if case.check is not None:
            try:
                case.check(run.outputs())
            except AssertionError as ex:
                fails.append(f"{tag}: the oracle criterion fails: {ex}")
        return
    for name, v in run.views.items():
        if v.arg.is_input:
            continue
        off, cnt = _first_diff(run.payload(name), base.payload(name))
        if cnt:
            fails.append(f"{tag}: output {name} differs from the aligned call's in {cnt} bytes, first {_where(v.off + off, v)}: "
                         f"{run.payload(name)[off]:#04x}, aligned {base.payload(name)[off]:#04x}")


def run_case(case, backend, log=print):
    """The whole protocol for one case; raises ViewFailure naming every finding."""
    fails = []
    if case.setup:
        case.setup()
    try:
        a1 = _run(case, backend, "A", False, False)
        _check_run(case, a1, None, fails, False)
        a2 = _run(case, backend, "A (repeated)", False, False)
        by_oracle = False
        if a1.raised is None and a2.raised is None:
            for name, v in a1.views.items():
                if not v.arg.is_input and _first_diff(a1.payload(name), a2.payload(name))[1]:
                    by_oracle = True
                    log(f"{case.head()}: the aligned call is NOT reproducible byte for byte (output {name}); B, C and D are held to the oracle criterion")
        _check_run(case, a2, a1, fails, by_oracle)
        for which, pad_in, pad_out in VARIANTS[1:]:
            if not any(a.is_input for a in case.args) and pad_in and not pad_out:
                continue
            _check_run(case, _run(case, backend, which, pad_in, pad_out), a1, fails, by_oracle)
    finally:
        if case.teardown:
            case.teardown()
    if fails:
        raise ViewFailure("\n  ".join([f"{case.head()}: {len(fails)} findings"] + fails))

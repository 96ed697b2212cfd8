"""The rows of tests/test_gpu_views_of_buffers.py: one per (core device entry point, kernel family behind it), at the smallest shape that has
two work items of the family plus a partial one (the constants are those tests/launch_caps.py and the per-path tests restate: FPW + 1
frames for the radix-16 spectra, 65 frames for the 64-frame demodulator tiles, 17 for the small-batch arrays, 13 for k_am_grp, 257
elements for element-wise kernels, display widths 111 and 112).

A row is built without a GPU (`Row.make()` -> view_util.Case: the arguments with their layouts and decisions, the inputs from
tests/length_cases.py, no two frames alike); the engine is only touched by `call`, `setup`, `teardown` and `check`.  `check` holds call A to
the oracle (tests/oracle_lib.py) or the NumPy statement under the criterion of the path's existing test, imported from that test where it
is a named constant or function.  Every row has one.  A row that is a composition (the pipelines, the sweep report, the decoder
batches, the `_rows_db` pair) is held, besides, byte for byte to the separate entry points on whole allocations (`_separate`), which
have rows of their own, or to the host twins (pss_h_scan_gate, pss_h_squelch_gate, pss_h_morse_decode, pss_h_ax25_frame).

Decisions (PARITY.md, "Views of buffers"): every argument of every row is SERVED at record alignment — no kernel masks address bits, rounds
a base down or runs a head / tail loop that assumes one, and no atomic touches a caller buffer (the atomicMax sites work on context
scratch) — and every pointer below its record's alignment is refused by the entry point's PSS_ALIGNED line before the first launch.
ALREADY_OFFSET names the units whose own suites run them at offset pointers.
"""
import ctypes as C

import numpy as np

import length_cases as LC
import spectrum_bounds as SB
import view_util as V
from pyspecsdr_amd import _lib as L

FS = 2.4e6
DEFAULT_OPTIONS = {"small_batch": 1, "nfm_fused": 1, "wfm_fused": 1, "ssb_hilbert": 1, "hilbert_exact": 0, "f64_plain": 0, "db_exact": 0,
                   "scan_exact": 1, "fuse_post": 1}

# units that state their own alignment contract in include/pss.h and whose GPU suites already run them at pointers offset into larger,
# guarded allocations: entry point -> that suite
ALREADY_OFFSET = {
    "pss_ddc": "test_gpu_ddc.py", "pss_pfb": "test_gpu_pfb.py", "pss_bank": "test_gpu_bank.py", "pss_resample": "test_gpu_resample.py",
    "pss_welch": "test_gpu_welch.py", "pss_rds_front": "test_gpu_rds.py", "pss_rds_bits": "test_gpu_rds.py", "pss_rds_groups": "test_gpu_rds.py",
    "pss_adsb_frames": "test_gpu_adsb.py", "pss_ais_front": "test_gpu_ais.py", "pss_ais_frames": "test_gpu_ais.py",
    "pss_pocsag_batches": "test_gpu_pocsag.py", "pss_apt_front": "test_gpu_apt.py", "pss_apt_syncs": "test_gpu_apt.py",
    "pss_apt_lines": "test_gpu_apt.py", "pss_unpack_iq": "test_gpu_iq_codes.py", "pss_live_frames": "test_gpu_stream_frames.py",
    "pss_demod_gated": "test_gpu_squelch.py", "pss_decode_mono": "test_gpu_fm_mono.py",
}
# device pointers that are not buffers of samples: the multi-GPU exchange moves opaque bytes (tests/test_multi_gpu.py)
OPAQUE_BYTES = {"pss_gather_packed": "test_multi_gpu.py", "pss_halo_from_left": "test_multi_gpu.py"}


class Row:
    def __init__(self, entry, family, shape, make):
        self.entry, self.family, self.shape, self.make = entry, family, shape, make

    @property
    def id(self):
        return f"{self.entry[4:]}-{self.family}-{self.shape}".replace(" ", "").replace(",", "_")


ROWS = []


def row(entry, family, shape):
    def deco(make):
        ROWS.append(Row(entry, family, shape, make))
        return make
    return deco


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def _engine():
    import gpu_util as G
    return G.engine()


def _options(opts):
    """(setup, teardown) that set the case's options and put the defaults back."""
    if not opts:
        return None, None

    def setup():
        for k, v in opts.items():
            _engine().set_option(k, v)

    def teardown():
        for k in opts:
            _engine().set_option(k, DEFAULT_OPTIONS[k])
    return setup, teardown


def _is_refusal(ex, names):
    return getattr(ex, "code", None) == L.PSS_E_ARG and all(f" {n} must be" in str(ex) for n in names)


def case(entry, family, shape, args, call, check=None, opts=None, note="", target_rate=None):
    """target_rate: demodulate_nfm / _wfm's target_rate for the four calls (pss_set_target_rate), 22 050 again behind them."""
    from pyspecsdr_amd.engine import PssError
    setup, teardown = _options(opts)
    if target_rate is not None:
        opt_setup, opt_teardown = setup, teardown

        def setup():
            if opt_setup:
                opt_setup()
            _engine().set_target_rate(float(target_rate))

        def teardown():
            _engine().set_target_rate(22050.0)
            if opt_teardown:
                opt_teardown()
    return V.Case(entry, family, shape, args, call, check=check, setup=setup, teardown=teardown, refusal=PssError, is_refusal=_is_refusal, note=note)


def _separate(inputs, outputs, fn):
    """The separate entry points on whole allocations, for the rows that are compositions (test_frame_pipeline_modes_equal_separate_calls'
    criterion: byte for byte).  inputs: name -> array (complex arrays interleaved); outputs: name -> (layout, shape), filled with 0x7f bytes;
    fn(p) queues the calls on p[name] pointers and may return a value.  -> (arrays by output name, fn's value)."""
    import torch
    import gpu_util as G
    ins = {k: G.dev(np.ascontiguousarray(v).view(np.float64) if np.asarray(v).dtype == np.complex128 else v) for k, v in inputs.items()}
    outs = {k: torch.full((int(np.prod(shape)) * np.dtype(V._NP[lay]).itemsize,), V.FILL, dtype=torch.uint8, device="cuda") for k, (lay, shape) in outputs.items()}
    torch.cuda.synchronize()
    r = fn({**{k: t.data_ptr() for k, t in ins.items()}, **{k: t.data_ptr() for k, t in outs.items()}})
    G.engine().sync()
    torch.cuda.synchronize()
    return {k: outs[k].cpu().numpy().view(V._NP[lay]).reshape(shape) for k, (lay, shape) in outputs.items()}, r


def _lines_separately(e, p, kind, f64, nf, ln, disp_w, dh, post="d_post"):
    """The display line of every frame from materialised rows: the entry point of `kind` on p[post], p["d_row_lo"], p["d_row_hi"]."""
    if kind == "waterfall":
        e.waterfall_rows(p[post], nf, ln, p["d_row_lo"], p["d_row_hi"], disp_w, p["d_line_a"], p["d_line_b"], f64=f64)
    elif kind == "gradient":
        e.gradient_rows(p[post], nf, ln, p["d_row_lo"], p["d_row_hi"], disp_w, p["d_line_a"], p["d_line_b"], f64=f64)
    else:
        e.persistence_rows(p[post], nf, ln, p["d_row_lo"], p["d_row_hi"], dh, disp_w, p["d_line_a"], f64=f64)


def _same_outputs(what, out, want, names=None):
    for k in (names or want):
        g, w = np.ascontiguousarray(out[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k} is {g.dtype}{g.shape}, the separate calls' {w.dtype}{w.shape}"
        bad = np.nonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))[0]
        assert bad.size == 0, f"{what}: {k} differs from the separate calls' in {bad.size} bytes, first in element {int(bad[0]) // g.dtype.itemsize}"


def A(name, layout, data):
    return V.Arg(name, layout, data=data)


def Out(name, layout, *shape, sparse=False):
    return V.Arg(name, layout, shape=shape, sparse=sparse)


def _distinct(x):
    assert LC.repeats(np.ascontiguousarray(x).reshape(len(x), -1)) == 0, "two input frames are alike"
    return x


def _bits(g, w):
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w, dtype=np.asarray(g).dtype)
    if g.dtype.kind != "f":
        return g == w
    u = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    return (g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))


def _same(what, got, want, ok=None):
    ok = _bits(got, want) if ok is None else ok
    bad = np.argwhere(~np.asarray(ok))
    assert len(bad) == 0, f"{what}: {len(bad)} values fail, first at {tuple(int(i) for i in bad[0])}: got {np.asarray(got)[tuple(bad[0])]!r}, want {np.asarray(want)[tuple(bad[0])]!r}"


def _close(what, got, want, tol):
    with np.errstate(invalid="ignore"):
        _same(what, got, want, np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) <= tol)


def _frames(fn, x):
    import oracle_lib as O
    return O.map_frames(fn, list(x))


def _pcm(audio_rows):
    import oracle_lib as O
    return np.stack([O.pcm16_stereo(a) for a in audio_rows])


def spectrum_family(n):
    """The kernel family of compute_fft at n points (the crossovers test_gpu_spectrum_accuracy.family names)."""
    if SB.bluestein(n):
        return f"bluestein_M{SB.transform_len(n)}"
    return "k_spectrum" if n <= 128 else "k_spectrum_r16" if n <= 4096 else "k_spectrum_xl" if n <= 16384 else "k_spectrum_r16_big" if n <= 65536 else "k_huge"


# ---- compute_fft: pss_spectrum_db and its float64 / complex128 twins ---------------------------------------------------------------------------
SPECTRUM_SHAPES = [(256, 17), (512, 9), (1024, 5), (2048, 3), (4096, 3), (8192, 2), (16384, 2), (64, 3), (32768, 2), (1000, 3), (1 << 17, 1)]


def _spectrum(n, nf, exact):
    def make():
        x = _distinct(LC.fm_frames(nf, n, seed=31))

        def check(out):
            import test_gpu_spectrum_accuracy as SA
            SA.check_rows("exact" if exact else "fast", out["d_db"], x, SA.oracle_rows(x), n, "rows of a view")
        return case("pss_spectrum_db", spectrum_family(n) + ("_db_exact" if exact else ""), f"{nf}x{n}", [A("d_iq", "complex64", x), Out("d_db", "float32", nf, n)],
                    lambda v: _engine().spectrum_db(v["d_iq"].ptr, nf, n, v["d_db"].ptr), check, {"db_exact": 1} if exact else None)
    row("pss_spectrum_db", spectrum_family(n) + ("_db_exact" if exact else ""), f"{nf}x{n}")(make)


for _n, _nf in SPECTRUM_SHAPES:
    for _exact in (0, 1):
        _spectrum(_n, _nf, _exact)


def _spectrum_f64(n, nf, plain, c128=False):
    entry = "pss_spectrum_db_c128" if c128 else "pss_spectrum_db_f64"
    fam = "k_spectrum_c128" if c128 else ("k_spectrum_f64_plain" if plain or n < 256 or n > 4096 else "k_spectrum_r16_f64")

    def make():
        x = _distinct(LC.c128_frames(nf, n, seed=32) if c128 else LC.fm_frames(nf, n, seed=32))

        def check(out):
            import test_gpu_spectrum_accuracy as SA
            SA.check_rows("f64", out["d_db"], x, SA.oracle_rows(x, c128), n, "float64 rows of a view")
        e_call = (lambda v: _engine().spectrum_db_c128(v["d_iq"].ptr, nf, n, v["d_db"].ptr)) if c128 else \
                 (lambda v: _engine().spectrum_db_f64(v["d_iq"].ptr, nf, n, v["d_db"].ptr))
        return case(entry, fam, f"{nf}x{n}", [A("d_iq", "complex128" if c128 else "complex64", x), Out("d_db", "float64", nf, n)], e_call, check,
                    {"f64_plain": 1} if plain else None)
    row(entry, fam, f"{nf}x{n}")(make)


for _n, _nf in [(256, 17), (512, 9), (1024, 5), (2048, 3), (4096, 3), (64, 3), (8192, 2), (32768, 2)]:
    _spectrum_f64(_n, _nf, 0)
_spectrum_f64(1024, 5, 1)
_spectrum_f64(64, 3, 0, c128=True)
_spectrum_f64(4096, 3, 0, c128=True)


# ---- the caller's post-process ------------------------------------------------------------------------------------------------------------------
def db_rows(nf, n, dtype, seed=0):
    """dB rows as compute_fft leaves them for noise with a hump: no two alike, ties in row 1."""
    rng = np.random.default_rng([41, n, seed])
    db = rng.standard_normal((nf, n)) * 6.0 - 35.0
    db[0, n // 4:n // 4 + max(4, n // 10)] += 40.0
    if nf > 1:
        db[1] = np.round(db[1])
    return _distinct(db.astype(dtype))


def numpy_post(db):
    """pyspecsdr.py:2278-2283 on one row in float64 (test_post_process_long_rows' statement)."""
    sm = np.convolve(db.astype(np.float64), np.ones(5) / 5, mode="valid")
    thr = np.median(sm) - 10
    return np.where(sm < thr, thr, sm), thr


def _post_family(n, f64=False, plain=False):
    if f64 and (plain or n - 4 > 16384 or n % 4):
        return "k_post_f64"
    if n % 4 == 0 and n - 4 <= (16384 if f64 else 32768):
        m = n - 4
        return "k_post_sel_" + ("4x1" if m <= 256 else "8x1" if m <= 512 else "16x1" if m <= 1024 else "32x1" if m <= 2048 else "16x4" if m <= 4096 else
                                "32x4" if m <= 8192 else "16x16" if m <= 16384 else "32x16") + ("_f64" if f64 else "")
    return "k_post_select" if n > 8192 else "k_post"


def _check_post(db, out, f64):
    import test_gpu_full_batch as FB
    for f in range(len(db)):
        ref, thr = numpy_post(db[f])
        if f64:
            import oracle_lib as O
            _same(f"post-processed row {f} (bits of the oracle's)", out["d_post"][f], O.postprocess(db[f]))
        elif "d_post" in out:
            _close(f"post-processed row {f} (1e-4 relative)", out["d_post"][f], ref, FB.DB_REL * np.maximum(np.abs(ref), 1.0))
        if "d_row_thr" in out:
            _close(f"clamp threshold of row {f}", out["d_row_thr"][f:f + 1], [thr], FB.DB_REL * max(abs(thr), 1.0))
        if "d_row_lo" in out:
            own = out["d_post"][f] if "d_post" in out else ref.astype(np.float32)
            fin = own[np.isfinite(own)]
            if "d_post" in out:
                assert out["d_row_lo"][f] == fin.min() and out["d_row_hi"][f] == fin.max(), f"row {f}: extremes {out['d_row_lo'][f]!r}, {out['d_row_hi'][f]!r} are not those of its row"
            else:
                _close(f"extremes of row {f}", [out["d_row_lo"][f], out["d_row_hi"][f]], [ref.min(), ref.max()], FB.DB_REL * max(np.abs(ref).max(), 1.0))


def _post(entry, n, nf, f64=False, plain=False):
    fam = _post_family(n, f64, plain)
    el = "float64" if f64 else "float32"

    def make():
        db = db_rows(nf, n, np.float64 if f64 else np.float32)
        args = [A("d_db", el, db)]
        if entry != "pss_spectrum_post_thresholds":
            args.append(Out("d_post", el, nf, n - 4))
        if entry == "pss_spectrum_post_thresholds":
            args.append(Out("d_row_thr", el, nf))
        if entry != "pss_spectrum_post":
            args += [Out("d_row_lo", el, nf), Out("d_row_hi", el, nf)]

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            if entry == "pss_spectrum_post":
                e.spectrum_post(p["d_db"], nf, n, p["d_post"])
            elif entry == "pss_spectrum_post_extremes":
                e.spectrum_post_extremes(p["d_db"], nf, n, p["d_post"], p["d_row_lo"], p["d_row_hi"])
            elif entry == "pss_spectrum_post_thresholds":
                e.spectrum_post_thresholds(p["d_db"], nf, n, p["d_row_thr"], p["d_row_lo"], p["d_row_hi"])
            else:
                e.spectrum_post_f64(p["d_db"], nf, n, p["d_post"], p["d_row_lo"], p["d_row_hi"])
        return case(entry, fam, f"{nf}x{n}", args, call, lambda out: _check_post(db, out, f64), {"f64_plain": 1} if plain else None)
    row(entry, fam, f"{nf}x{n}")(make)


for _n, _nf in [(256, 17), (512, 9), (1024, 5), (2048, 3), (4096, 3), (8192, 2), (16384, 2), (32768, 2), (1002, 3), (65536, 2)]:
    _post("pss_spectrum_post", _n, _nf)
for _n, _nf in [(1024, 5), (1002, 3), (65536, 2)]:
    _post("pss_spectrum_post_extremes", _n, _nf)
for _n, _nf in [(1024, 5), (4096, 3)]:
    _post("pss_spectrum_post_thresholds", _n, _nf)
for _n, _nf in [(1024, 5), (4096, 3), (16384, 2), (32768, 2)]:
    _post("pss_spectrum_post_f64", _n, _nf, f64=True)
_post("pss_spectrum_post_f64", 1024, 5, f64=True, plain=True)


def _db_post(n, nf):
    def make():
        x = _distinct(LC.fm_frames(nf, n, seed=33))
        args = [A("d_iq", "complex64", x), Out("d_db", "float32", nf, n), Out("d_post", "float32", nf, n - 4), Out("d_row_lo", "float32", nf),
                Out("d_row_hi", "float32", nf)]

        def check(out):
            import test_gpu_spectrum_accuracy as SA
            SA.check_rows("fast", out["d_db"], x, SA.oracle_rows(x), n, "rows of a view")
            _check_post(out["d_db"], out, False)     # the post-process of the device's own rows, as test_spectrum_db_post_rows takes it
        return case("pss_spectrum_db_post", spectrum_family(n) + "+" + _post_family(n), f"{nf}x{n}", args,
                    lambda v: _engine().spectrum_db_post(v["d_iq"].ptr, nf, n, v["d_db"].ptr, v["d_post"].ptr, v["d_row_lo"].ptr, v["d_row_hi"].ptr), check)
    row("pss_spectrum_db_post", spectrum_family(n) + "+" + _post_family(n), f"{nf}x{n}")(make)


_db_post(1024, 5)
_db_post(1000, 3)


def _row_extremes(f64):
    entry, el = ("pss_row_extremes_f64", "float64") if f64 else ("pss_row_extremes", "float32")

    def make():
        rows = db_rows(5, 1021, np.float64 if f64 else np.float32, seed=2)
        rows[3, 10:20] = np.inf

        def check(out):
            for f in range(5):
                fin = rows[f][np.isfinite(rows[f])]
                assert out["d_row_lo"][f] == fin.min() and out["d_row_hi"][f] == fin.max(), f"row {f}"
        return case(entry, "k_row_extremes", "5x1021", [A("d_rows", el, rows), Out("d_row_lo", el, 5), Out("d_row_hi", el, 5)],
                    lambda v: _engine().row_extremes(v["d_rows"].ptr, 5, 1021, v["d_row_lo"].ptr, v["d_row_hi"].ptr, f64=f64), check)
    row(entry, "k_row_extremes", "5x1021")(make)


_row_extremes(False)
_row_extremes(True)


# ---- batched display lines ------------------------------------------------------------------------------------------------------------------------
def post_rows(nf, ln, dtype, seed=0):
    rows = np.stack([numpy_post(r)[0] for r in db_rows(nf, ln + 4, np.float64, seed)])
    return _distinct(rows.astype(dtype))


def _display_rows(kind, f64, disp_w):
    entry = f"pss_{kind}_rows" + ("_f64" if f64 else "")
    el, dt = ("float64", np.float64) if f64 else ("float32", np.float32)
    nf, ln, dh = 5, 1020, 36

    def make():
        rows = post_rows(nf, ln, dt, seed=disp_w)
        lo, hi = rows.min(axis=1), rows.max(axis=1)
        args = [A("d_post", el, rows), A("d_row_lo", el, lo), A("d_row_hi", el, hi), Out("d_line_a", "int8", nf, disp_w)]
        if kind != "persistence":
            args.append(Out("d_line_b", "int8", nf, disp_w))

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            if kind == "waterfall":
                e.waterfall_rows(p["d_post"], nf, ln, p["d_row_lo"], p["d_row_hi"], disp_w, p["d_line_a"], p["d_line_b"], f64=f64)
            elif kind == "gradient":
                e.gradient_rows(p["d_post"], nf, ln, p["d_row_lo"], p["d_row_hi"], disp_w, p["d_line_a"], p["d_line_b"], f64=f64)
            else:
                e.persistence_rows(p["d_post"], nf, ln, p["d_row_lo"], p["d_row_hi"], dh, disp_w, p["d_line_a"], f64=f64)

        def check(out):
            import oracle_lib as O
            if kind == "gradient":       # test_gradient_rows_every_frame_of_a_history_against_the_oracle: line i is the oracle grid's newest row
                wide = rows.astype(np.float64)
                for i in range(nf):
                    og, oc = O.gradient_cells(wide[max(0, i - 29):i + 1], 1, disp_w)
                    _same(f"gradient glyphs of frame {i}", out["d_line_a"][i], og[0])
                    _same(f"gradient colours of frame {i}", out["d_line_b"][i], oc[0])
            elif f64:                    # test_gpu_display_geometry's float64 lines
                import test_gpu_display_geometry as DG
                a, b = DG._oracle_lines_f64(rows, lo, hi, 30 if kind == "waterfall" else 10, kind, disp_w, dh)
                _same(f"{kind} line a", out["d_line_a"], a)
                if b is not None:
                    _same("waterfall colours", out["d_line_b"], b)
            elif kind == "waterfall":
                g, c = O.waterfall_rows(rows, 30, disp_w)
                _same("waterfall glyphs", out["d_line_a"], g)
                _same("waterfall colours", out["d_line_b"], c)
            else:
                _same("persistence trace", out["d_line_a"], O.persistence_rows(rows, 10, dh, disp_w))
        return case(entry, "k_slide_extremes+k_disp_rows", f"{nf}x{ln}_w{disp_w}", args, call, check)
    row(entry, "k_slide_extremes+k_disp_rows", f"{nf}x{ln}_w{disp_w}")(make)


for _kind in ("waterfall", "gradient", "persistence"):
    for _f64 in (False, True):
        for _w in (111, 112):
            _display_rows(_kind, _f64, _w)


def _display_rows_db(kind, disp_w):
    entry, nf, n, dh = f"pss_{kind}_rows_db", 5, 1024, 36

    def make():
        db = db_rows(nf, n, np.float32, seed=disp_w)
        post = [numpy_post(r) for r in db]
        # the clamp threshold as the device keeps it (test_display_lines_without_materialised_rows' statement): float32(median of the float32 smoothed row - 10)
        thr = np.array([np.float32(np.median(np.convolve(r.astype(np.float64), np.ones(5) / 5, mode="valid").astype(np.float32)).astype(np.float64) - 10.0)
                        for r in db], np.float32)
        lo = np.array([p.min() for p, _ in post], np.float32)
        hi = np.array([p.max() for p, _ in post], np.float32)
        args = [A("d_db", "float32", db), A("d_row_thr", "float32", thr), A("d_row_lo", "float32", lo), A("d_row_hi", "float32", hi),
                Out("d_line_a", "int8", nf, disp_w)] + ([Out("d_line_b", "int8", nf, disp_w)] if kind == "waterfall" else [])

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            if kind == "waterfall":
                e.waterfall_rows_db(p["d_db"], nf, n, p["d_row_thr"], p["d_row_lo"], p["d_row_hi"], disp_w, p["d_line_a"], p["d_line_b"])
            else:
                e.persistence_rows_db(p["d_db"], nf, n, p["d_row_thr"], p["d_row_lo"], p["d_row_hi"], dh, disp_w, p["d_line_a"])

        def check(out):
            """test_display_lines_without_materialised_rows: the thresholds are the device's own, and the lines are byte for byte those of
            pss_waterfall_rows / pss_persistence_rows on the materialised rows with the same extremes."""
            def separate(p):
                e = _engine()
                e.spectrum_post(p["d_db"], nf, n, p["d_post"])
                e.spectrum_post_thresholds(p["d_db"], nf, n, p["thr"], p["lo"], p["hi"])
                _lines_separately(e, p, kind, False, nf, n - 4, disp_w, dh)
            spec = {"d_post": ("float32", (nf, n - 4)), "thr": ("float32", (nf,)), "lo": ("float32", (nf,)), "hi": ("float32", (nf,)),
                    "d_line_a": ("int8", (nf, disp_w)), "d_line_b": ("int8", (nf, disp_w))}
            want, _ = _separate({"d_db": db, "d_row_lo": lo, "d_row_hi": hi}, spec, separate)
            _same("the thresholds handed in are pss_spectrum_post_thresholds' own", thr, want["thr"])
            _same_outputs("lines from the dB rows", out, want, [k for k in ("d_line_a", "d_line_b") if k in out])
        return case(entry, "k_slide_extremes+k_disp_rows_db", f"{nf}x{n}_w{disp_w}", args, call, check)
    row(entry, "k_slide_extremes+k_disp_rows_db", f"{nf}x{n}_w{disp_w}")(make)


for _kind in ("waterfall", "persistence"):
    for _w in (111, 112):
        _display_rows_db(_kind, _w)


# ---- screen grids ---------------------------------------------------------------------------------------------------------------------------------
CELL_RATE = 1e-3          # test_waterfall_and_persistence_cells: float32 rows differ from the float64 oracle only on quantisation edges


def _cells(kind, f64, disp_w):
    entry = f"pss_{kind}_cells" + ("_f64" if f64 else "")
    el, dt = ("float64", np.float64) if f64 else ("float32", np.float32)
    nr, ln, dh = {"waterfall": 30, "gradient": 30, "persistence": 10}[kind], 1020, 36

    def make():
        rows = post_rows(nr, ln, dt, seed=100 + disp_w)
        args = [A("d_rows", el, rows)] + ([Out("d_glyph", "int8", dh, disp_w)] if kind != "persistence" else []) + [Out("d_colour", "int8", dh, disp_w)]

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            if kind == "waterfall":
                e.waterfall_cells(p["d_rows"], nr, ln, dh, disp_w, p["d_glyph"], p["d_colour"], f64=f64)
            elif kind == "gradient":
                e.gradient_cells(p["d_rows"], nr, ln, dh, disp_w, p["d_glyph"], p["d_colour"], f64=f64)
            else:
                e.persistence_cells(p["d_rows"], nr, ln, dh, disp_w, p["d_colour"], f64=f64)

        def check(out):
            import oracle_lib as O
            r64 = rows.astype(np.float64)
            want = {"waterfall": lambda: dict(zip(("d_glyph", "d_colour"), O.waterfall_cells(r64, dh, disp_w))),
                    "gradient": lambda: dict(zip(("d_glyph", "d_colour"), O.gradient_cells(r64, dh, disp_w))),
                    "persistence": lambda: {"d_colour": O.persistence_cells(r64, dh, disp_w)}}[kind]()
            for k, w in want.items():
                if f64:
                    _same(f"{kind} {k}", out[k], w)
                else:
                    assert np.mean(out[k] != w) < CELL_RATE, f"{kind} {k}: {np.mean(out[k] != w):.2e} of the cells differ from the float64 oracle's"
        return case(entry, "k_cells", f"{nr}x{ln}_{dh}x{disp_w}", args, call, check)
    row(entry, "k_cells", f"{nr}x{ln}_{dh}x{disp_w}")(make)


for _kind in ("waterfall", "gradient", "persistence"):
    for _f64 in (False, True):
        for _w in (111, 112):
            _cells(_kind, _f64, _w)


def _spectrogram(f64, ln, disp_w):
    entry, (el, dt) = "pss_spectrogram_cells" + ("_f64" if f64 else ""), (("float64", np.float64) if f64 else ("float32", np.float32))
    nf, dh, fam = 5, 30, "k_spectrogram_256" if ln <= 4096 else "k_spectrogram_1024"

    def make():
        rows = post_rows(nf, ln, dt, seed=200 + disp_w)
        args = [A("d_rows", el, rows), Out("d_glyph", "int8", nf, dh, disp_w), Out("d_colour", "int8", nf, dh, disp_w), Out("d_range", "float64", nf, 2)]

        def check(out):
            import oracle_lib as O
            for f in range(nf):
                g, c, lo, hi = O.spectrogram_cells(rows[f].astype(np.float64), dh, disp_w)
                _same(f"glyph cells of row {f}", out["d_glyph"][f], g)
                _same(f"colour cells of row {f}", out["d_colour"][f], c)
                assert np.allclose(out["d_range"][f], [lo, hi], rtol=1e-14, atol=0), f"range of row {f}"
        return case(entry, fam, f"{nf}x{ln}_{dh}x{disp_w}", args,
                    lambda v: _engine().spectrogram_cells(v["d_rows"].ptr, nf, ln, dh, disp_w, v["d_glyph"].ptr, v["d_colour"].ptr, v["d_range"].ptr, f64=f64), check)
    row(entry, fam, f"{nf}x{ln}_{dh}x{disp_w}")(make)


for _f64 in (False, True):
    _spectrogram(_f64, 2044, 111)
    _spectrogram(_f64, 2044, 112)
    _spectrogram(_f64, 5000, 112)


def _bars(f64, ln, disp_w):
    entry, (el, dt) = "pss_spectrum_bars" + ("_f64" if f64 else ""), (("float64", np.float64) if f64 else ("float32", np.float32))
    nf, dh = 5, 30
    fam = "k_spectrum_bars_4x1" if ln <= 256 else "k_spectrum_bars_16x1" if ln <= 1024 else "k_spectrum_bars_32x1" if ln <= 2048 else \
        "k_spectrum_bars_16x4" if ln <= 4092 else "k_spectrogram_bars"

    def make():
        rows = post_rows(nf, ln, dt, seed=300 + disp_w)
        args = [A("d_rows", el, rows), Out("d_height", "int8", nf, disp_w), Out("d_level", "int8", nf, disp_w), Out("d_range", "float64", nf, 2)]

        def check(out):
            import oracle_lib as O
            from pyspecsdr_amd import formats
            for f in range(nf):      # the bars ARE the spectrogram's grid, column by column (include/pss.h): expanded on the host and compared
                g, c, lo, hi = O.spectrogram_cells(rows[f].astype(np.float64), dh, disp_w)
                eg, ec = formats.bars_cells(out["d_height"][f:f + 1], out["d_level"][f:f + 1], dh)
                _same(f"glyph cells from the bars of row {f}", np.asarray(eg)[0], g)
                _same(f"colour cells from the bars of row {f}", np.asarray(ec)[0], c)
                assert np.allclose(out["d_range"][f], [lo, hi], rtol=1e-14, atol=0), f"range of row {f}"
        return case(entry, fam, f"{nf}x{ln}_{dh}x{disp_w}", args,
                    lambda v: _engine().spectrum_bars(v["d_rows"].ptr, nf, ln, dh, disp_w, v["d_height"].ptr, v["d_level"].ptr, v["d_range"].ptr, f64=f64), check)
    row(entry, fam, f"{nf}x{ln}_{dh}x{disp_w}")(make)


for _f64 in (False, True):
    for _ln, _w in ((252, 111), (1020, 112), (2044, 111), (4092, 112), (5000, 111)):
        _bars(_f64, _ln, _w)


def _host_twin(fn, *args):
    r = fn(*args)
    assert r == 0, f"the host twin returned {r}"


def _bars_cells(disp_w):
    nf, dh = 5, 30

    def make():
        rng = np.random.default_rng(disp_w)
        height = rng.integers(-1, dh + 1, (nf, disp_w)).astype(np.int8)
        level = np.where(height < 0, -1, rng.integers(0, 4, (nf, disp_w))).astype(np.int8)

        def check(out):
            g, c = np.empty((nf, dh, disp_w), np.int8), np.empty((nf, dh, disp_w), np.int8)
            _host_twin(L.load().pss_h_bars_cells, height.ctypes.data, level.ctypes.data, nf, dh, disp_w, g.ctypes.data, c.ctypes.data)
            _same("glyph cells (pss_h_bars_cells)", out["d_glyph"], g)
            _same("colour cells (pss_h_bars_cells)", out["d_colour"], c)
        return case("pss_bars_cells", "k_bars_cells", f"{nf}x{dh}x{disp_w}",
                    [A("d_height", "int8", height), A("d_level", "int8", level), Out("d_glyph", "int8", nf, dh, disp_w), Out("d_colour", "int8", nf, dh, disp_w)],
                    lambda v: _engine().bars_cells(v["d_height"].ptr, v["d_level"].ptr, nf, dh, disp_w, v["d_glyph"].ptr, v["d_colour"].ptr), check)
    row("pss_bars_cells", "k_bars_cells", f"{nf}x{dh}x{disp_w}")(make)


_bars_cells(111)
_bars_cells(112)


def _surface(f64, max_w):
    entry, (el, dt) = "pss_surface_cells" + ("_f64" if f64 else ""), (("float64", np.float64) if f64 else ("float32", np.float32))
    ln, max_h = 1020, 40

    def make():
        r = post_rows(2, ln, dt, seed=400 + max_w)[0]

        def check(out):
            import oracle_lib as O
            _same("surface colours", out["d_colour"], O.surface_cells(r.astype(np.float64), max_h, max_w))
        return case(entry, "k_cells_surface", f"{ln}_{max_h}x{max_w}", [A("d_row", el, r), Out("d_colour", "int8", max_h, max_w)],
                    lambda v: _engine().surface_cells(v["d_row"].ptr, ln, max_h, max_w, v["d_colour"].ptr, f64=f64), check)
    row(entry, "k_cells_surface", f"{ln}_{max_h}x{max_w}")(make)


for _f64 in (False, True):
    _surface(_f64, 119)
    _surface(_f64, 120)


def _surface_mags(f64, ln, disp_w):
    entry, (el, dt) = "pss_surface_mags" + ("_f64" if f64 else ""), (("float64", np.float64) if f64 else ("float32", np.float32))
    nf, fam = 5, "k_surface_mags_1_staged" if ln <= 1024 else "k_surface_mags_4_staged" if ln <= 4092 else "k_surface_mags_4"

    def make():
        rows = post_rows(nf, ln, dt, seed=500 + disp_w)

        def check(out):
            import oracle_lib as O
            max_h, max_w = 40, disp_w + 8
            co = np.empty((nf, max_h, max_w), np.int8)
            mag = np.ascontiguousarray(out["d_mag"])
            _host_twin(L.load().pss_h_mags_cells, mag.ctypes.data, nf, max_h, max_w, co.ctypes.data)
            for f in range(nf):   # the magnitudes ARE the surface plot's, column by column: expanded on the host and compared with the oracle's grid
                _same(f"surface colours from the magnitudes of row {f}", co[f], O.surface_cells(rows[f].astype(np.float64), max_h, max_w))
                fin = rows[f][np.isfinite(rows[f])].astype(np.float64)
                _same(f"range of row {f}", out["d_range"][f], np.array([fin.min(), fin.max()]))
        return case(entry, fam, f"{nf}x{ln}_w{disp_w}", [A("d_rows", el, rows), Out("d_mag", "int8", nf, disp_w), Out("d_range", "float64", nf, 2)],
                    lambda v: _engine().surface_mags(v["d_rows"].ptr, nf, ln, disp_w, v["d_mag"].ptr, v["d_range"].ptr, f64=f64), check)
    row(entry, fam, f"{nf}x{ln}_w{disp_w}")(make)


for _f64 in (False, True):
    for _ln, _w in ((1020, 111), (4092, 112), (5000, 111)):
        _surface_mags(_f64, _ln, _w)


def _mags_cells(max_w):
    nf, max_h = 5, 40

    def make():
        mag = np.random.default_rng(max_w).integers(-1, 21, (nf, max_w - 8)).astype(np.int8)

        def check(out):
            co = np.empty((nf, max_h, max_w), np.int8)
            _host_twin(L.load().pss_h_mags_cells, mag.ctypes.data, nf, max_h, max_w, co.ctypes.data)
            _same("surface colours (pss_h_mags_cells)", out["d_colour"], co)
        return case("pss_mags_cells", "k_mags_cells", f"{nf}x{max_h}x{max_w}", [A("d_mag", "int8", mag), Out("d_colour", "int8", nf, max_h, max_w)],
                    lambda v: _engine().mags_cells(v["d_mag"].ptr, nf, max_h, max_w, v["d_colour"].ptr), check)
    row("pss_mags_cells", "k_mags_cells", f"{nf}x{max_h}x{max_w}")(make)


_mags_cells(119)
_mags_cells(120)


def _vector_iq(nf, n, seed):
    rng = np.random.default_rng([61, n, seed])
    return _distinct((rng.uniform(-2.1, 2.1, (nf, n)) + 1j * rng.uniform(-2.1, 2.1, (nf, n))).astype(np.complex64))


def _vector_cells(max_w):
    n, max_h = 257, 40

    def make():
        iq = _vector_iq(1, n, max_w)[0]

        def check(out):
            import oracle_lib as O
            _same("constellation grid", out["d_grid"], O.vector_cells(iq, max_h, max_w))
        return case("pss_vector_cells", "k_vector", f"{n}_{max_h}x{max_w}", [A("d_iq", "complex64", iq), Out("d_grid", "int8", max_h, max_w)],
                    lambda v: _engine().vector_cells(v["d_iq"].ptr, n, max_h, max_w, v["d_grid"].ptr), check)
    row("pss_vector_cells", "k_vector", f"{n}_{max_h}x{max_w}")(make)


_vector_cells(119)
_vector_cells(120)


def _vector_masks(n, nf, max_w):
    max_h, words = 40, (max_w + 31) // 32
    fam = "k_vector_masks_1" if n <= 4096 else "k_vector_masks_8"

    def make():
        iq = _vector_iq(nf, n, max_w)

        def check(out):
            import oracle_lib as O
            grid = np.empty((nf, max_h, max_w), np.int8)
            mask = np.ascontiguousarray(out["d_mask"])
            _host_twin(L.load().pss_h_masks_cells, mask.ctypes.data, nf, max_h, max_w, grid.ctypes.data)
            for f in range(nf):
                _same(f"constellation grid from the mask of frame {f}", grid[f], O.vector_cells(iq[f], max_h, max_w))
            spare = ~np.uint32(0) << np.uint32(max_w % 32) if max_w % 32 else np.uint32(0)
            assert not (mask.view(np.uint32)[..., -1] & spare).any(), "bits past the last column are set"
        return case("pss_vector_masks", fam, f"{nf}x{n}_{max_h}x{max_w}", [A("d_iq", "complex64", iq), Out("d_mask", "int32", nf, max_h, words)],
                    lambda v: _engine().vector_masks(v["d_iq"].ptr, nf, n, max_h, max_w, v["d_mask"].ptr), check)
    row("pss_vector_masks", fam, f"{nf}x{n}_{max_h}x{max_w}")(make)


_vector_masks(1024, 5, 119)
_vector_masks(1024, 5, 120)
_vector_masks(5000, 3, 120)


def _masks_cells(max_w):
    nf, max_h, words = 5, 40, (max_w + 31) // 32

    def make():
        mask = np.random.default_rng(max_w).integers(0, 2 ** 32, (nf, max_h, words), dtype=np.uint64).astype(np.uint32).view(np.int32)

        def check(out):
            grid = np.empty((nf, max_h, max_w), np.int8)
            _host_twin(L.load().pss_h_masks_cells, mask.ctypes.data, nf, max_h, max_w, grid.ctypes.data)
            _same("constellation grids (pss_h_masks_cells)", out["d_grid"], grid)
        return case("pss_masks_cells", "k_masks_cells", f"{nf}x{max_h}x{max_w}", [A("d_mask", "int32", mask), Out("d_grid", "int8", nf, max_h, max_w)],
                    lambda v: _engine().masks_cells(v["d_mask"].ptr, nf, max_h, max_w, v["d_grid"].ptr), check)
    row("pss_masks_cells", "k_masks_cells", f"{nf}x{max_h}x{max_w}")(make)


_masks_cells(119)
_masks_cells(120)


def _ring(kind, disp_w, entry=None):
    entry, ln, dh, nr = entry or f"pss_ring_{kind}", 1020, 36, 3

    def make():
        rows = post_rows(nr, ln, np.float32, seed=600 + disp_w)
        args = [A("d_row", "float32", rows)] + ([Out("d_glyph", "int8", dh, disp_w)] if kind == "waterfall" else []) + [Out("d_colour", "int8", dh, disp_w)]

        def call(v):
            e = _engine()
            ring = e.ring_create(30 if kind == "waterfall" else 10, ln)
            try:
                for i in range(nr):          # every pushed row is a view: row i of the padded buffer
                    e.ring_push(ring, v["d_row"].ptr + 4 * ln * i)
                if kind == "waterfall":
                    e.ring_waterfall(ring, dh, disp_w, v["d_glyph"].ptr, v["d_colour"].ptr)
                else:
                    e.ring_persistence(ring, dh, disp_w, v["d_colour"].ptr)
                e.sync()
            finally:
                e.ring_destroy(ring)

        def check(out):
            import oracle_lib as O
            r64 = rows.astype(np.float64)
            want = dict(zip(("d_glyph", "d_colour"), O.waterfall_cells(r64, dh, disp_w))) if kind == "waterfall" else {"d_colour": O.persistence_cells(r64, dh, disp_w)}
            for k, w in want.items():
                assert np.mean(out[k] != w) < CELL_RATE, f"ring {kind} {k}: {np.mean(out[k] != w):.2e} of the cells differ from the float64 oracle's"
        return case(entry, "hipMemcpyAsync+k_cells", f"{nr}x{ln}_{dh}x{disp_w}", args, call, check)
    row(entry, "hipMemcpyAsync+k_cells", f"{nr}x{ln}_{dh}x{disp_w}")(make)


_ring("waterfall", 111)
_ring("persistence", 112)
_ring("waterfall", 112, entry="pss_ring_push")


# ---- Hilbert transform ------------------------------------------------------------------------------------------------------------------------------
def _hilbert_family(n, exact):
    if exact:
        return "k_hilbert_pf" if n <= 16384 else "k_hilbert_pf_long"
    return "k_hilbert_r16" if n <= 4096 else "k_hilbert_xl" if n <= 16384 else "hilbert_long" if n <= 65536 else "k_huge_hilbert"


def _hilbert(n, exact):
    nf, fam = 3, _hilbert_family(n, exact)

    def make():
        rng = np.random.default_rng([71, n])
        x = rng.standard_normal((nf, n)) * 10.0 ** rng.uniform(-2, 1, (nf, 1))
        x[1] = np.cos(2 * np.pi * 37 * np.arange(n) / n)

        def check(out):
            import oracle_lib as O
            got = out["d_analytic"].reshape(nf, 2 * n)
            if exact:
                _same("analytic signal (bits of scipy.signal.hilbert)", got, np.stack(_frames(O.hilbert, x)).view(np.float64))
                return
            import test_gpu_grid_caps as GC
            h = np.zeros(n)
            h[0] = h[n // 2] = 1
            h[1:n // 2] = 2
            ref = np.fft.ifft(np.fft.fft(x, axis=1) * h, axis=1)
            tol = GC.HIL_REL * np.max(np.abs(x), axis=1, keepdims=True)
            g = np.ascontiguousarray(got).view(np.complex128)
            _same("analytic signal (1e-13 of the row's peak)", g, ref, np.abs(g - ref) <= tol)
            _close("real part is the input", g.real, x, tol)
        return case("pss_hilbert", fam, f"{nf}x{n}", [A("d_x", "float64", x), Out("d_analytic", "complex128", nf, n, 2)],
                    lambda v: _engine().hilbert(v["d_x"].ptr, nf, n, v["d_analytic"].ptr), check, {"hilbert_exact": 1} if exact else None)
    row("pss_hilbert", fam, f"{nf}x{n}")(make)


for _n in (256, 8192, 32768, 1 << 17):
    _hilbert(_n, False)
    _hilbert(_n, True)


# ---- demodulators -----------------------------------------------------------------------------------------------------------------------------------
NFM_PATHS = {"small_batch": ({}, 17), "fused": ({"small_batch": 0}, 65), "three_kernel": ({"small_batch": 0, "nfm_fused": 0}, 65)}
WFM_PATHS = {"small_batch": ({}, 17), "fused": ({"small_batch": 0}, 65), "plain": ({"small_batch": 0, "wfm_fused": 0}, 65)}


def _wfm_filt(e, fs):
    lp, pil, lmr, alpha = e.wfm_filters(fs)
    _, sos, zi = e.nfm_filters(fs)
    return dict(lp_sos=lp, pilot_sos=pil, lmr_sos=lmr, alpha=alpha, dec_sos=sos, dec_zi=zi)


def _am_sos(e):
    sos = np.empty((5, 6))
    e.lib.pss_am_bandpass_sos(sos.ctypes.data)
    return sos


def _demod_oracle(mode, x, fs, signal=False, hilbert=True, target_rate=22050):
    """float64 audio rows of the oracle for frames x (WFM: [n_out][2] per frame)."""
    import oracle_lib as O
    e = _engine()
    if mode == L.MODE_NFM:
        taps, sos, zi = e.nfm_filters(fs)
        return np.stack(_frames(lambda r: O.demod_nfm(r, fs, taps, sos, zi), x))
    if mode == L.MODE_AM:
        sos = _am_sos(e)
        return np.stack(_frames(lambda r: O.demod_am(r, sos), x))
    if mode == L.MODE_WFM:
        filt = _wfm_filt(e, fs)
        return np.stack(_frames(lambda r: O.demod_wfm(O.iq_correction(r) if signal else r, fs, filt, target_rate=target_rate), x))
    taps = e.ssb_taps(fs)
    return np.stack(_frames(lambda r: O.demod_ssb(r, taps, hilbert=hilbert), x))


def _pcm_of(mode, audio):
    import test_gpu_length_sweep as LS
    return LS.int16_of(audio) if mode == L.MODE_WFM else LS._pcm_mono(audio)


def _out_len(mode, n, fs, target_rate=22050):
    q = int(fs / target_rate)
    return (n - 1 + q - 1) // q if mode in (L.MODE_NFM, L.MODE_WFM) else n


def _demod(entry, mode, name, fam, nf, n, opts=None, ssb_atol=False, hilbert=True, frames=LC.fm_frames, fs=FS, target_rate=None):
    """ssb_atol: the float64 audio is held to test_gpu_length_sweep.SSB_ATOL (the register Hilbert transform against pocketfft's round trip at
    power-of-two lengths) instead of bit for bit."""
    n_out = _out_len(mode, n, fs, target_rate or 22050)
    stereo = mode == L.MODE_WFM

    def make():
        x = _distinct(frames(nf, n, seed=81 + mode))
        args = [A("d_iq", "complex64", x), Out("d_pcm", "pcm16", nf, n_out, 2), Out("d_audio", "float64", *((nf, n_out, 2) if stereo else (nf, n_out)))]
        if entry == "pss_demod_power":
            args.append(Out("d_power", "float32", nf))

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            if entry == "pss_demod":
                e.demod(mode, p["d_iq"], nf, n, fs, p["d_pcm"], p["d_audio"])
            elif entry == "pss_demod_signal":
                e.demod_signal(mode, p["d_iq"], nf, n, fs, p["d_pcm"], p["d_audio"])
            else:
                e.demod_power(mode, p["d_iq"], nf, n, fs, p["d_pcm"], p["d_audio"], p["d_power"])

        def check(out):
            import oracle_lib as O
            want = _demod_oracle(mode, x, fs, signal=entry == "pss_demod_signal", hilbert=hilbert, target_rate=target_rate or 22050)
            if ssb_atol:
                _close(f"float64 audio ({_ssb_tol():g})", out["d_audio"], want, _ssb_tol())
            else:
                _same("float64 audio bits", out["d_audio"], want)
            _same("int16 PCM", out["d_pcm"], _pcm_of(mode, want))
            if "d_power" in out:
                _same("power bits", out["d_power"], np.array(_frames(O.power_db, x), np.float32))
        return case(entry, fam, f"{name}_{nf}x{n}", args, call, check, opts, target_rate=target_rate)
    row(entry, fam, f"{name}_{nf}x{n}")(make)


for _path, (_opts, _nf) in NFM_PATHS.items():
    for _n in (130, 1024):
        _demod("pss_demod", L.MODE_NFM, "nfm", f"nfm_{_path}", _nf, _n, _opts)
for _path, (_opts, _nf) in WFM_PATHS.items():
    for _n in (130, 1024):
        _demod("pss_demod", L.MODE_WFM, "wfm", f"wfm_{_path}", _nf, _n, _opts)
# decimation factor 1 (launch_caps "wfm_q1": no decimate() stage, n_out = n - 1, an odd count of [L, R] pairs per frame), at test_wfm_factor_one_past_the_cap's
# rates: 250 kS/s, target rate 130 000
_demod("pss_demod", L.MODE_WFM, "wfm", "wfm_q1_small_batch", 17, 512, fs=250000.0, target_rate=130000)
_demod("pss_demod", L.MODE_WFM, "wfm", "wfm_q1", 65, 512, {"small_batch": 0}, fs=250000.0, target_rate=130000)
_demod("pss_demod_signal", L.MODE_WFM, "wfm", "k_iqcorr_scal+wfm_small_batch", 17, 1024, frames=LC.iq_frames)
_demod("pss_demod_signal", L.MODE_WFM, "wfm", "k_iqcorr_scal+wfm_fused", 65, 1024, {"small_batch": 0}, frames=LC.iq_frames)
_demod("pss_demod_signal", L.MODE_NFM, "nfm", "nfm_small_batch", 17, 130)
for _n in (130, 1024):
    _demod("pss_demod", L.MODE_AM, "am", "k_am_grp", 13, _n, frames=LC.iq_frames)
_demod("pss_demod_power", L.MODE_AM, "am", "k_pairwise2+k_am_grp", 13, 1024, frames=LC.iq_frames)
_demod("pss_demod_power", L.MODE_NFM, "nfm", "k_pairwise+nfm_small_batch", 17, 130)


def _ssb_tol():
    import test_gpu_length_sweep as LS
    return LS.SSB_ATOL


for _mode, _name in ((L.MODE_USB, "usb"), (L.MODE_LSB, "lsb")):
    _demod("pss_demod", _mode, _name, "k_ssb_fir+k_finalize", 3, 1000)                                 # no hilbert() round trip: bits
    _demod("pss_demod", _mode, _name, "k_ssb_fir+k_hilbert_r16", 3, 1024, ssb_atol=True)
    _demod("pss_demod", _mode, _name, "k_ssb_rfft", 3, 8192, ssb_atol=True)
    _demod("pss_demod", _mode, _name, "k_ssb_fir+hilbert_long", 3, 32768, ssb_atol=True)
_demod("pss_demod", L.MODE_USB, "usb", "k_ssb_fir+k_finalize_no_hilbert", 3, 1024, {"ssb_hilbert": 0}, hilbert=False)
_demod("pss_demod", L.MODE_USB, "usb", "k_ssb_fir+k_hilbert_pf", 3, 1024, {"hilbert_exact": 1})


def _power_db(nf, n):
    def make():
        x = _distinct(LC.power_frames(nf, n, seed=3))

        def check(out):
            import oracle_lib as O
            _same("power bits", out["d_power"], np.array(_frames(O.power_db, x), np.float32))
        return case("pss_power_db", "k_pairwise", f"{nf}x{n}", [A("d_iq", "complex64", x), Out("d_power", "float32", nf)],
                    lambda v: _engine().power_db(v["d_iq"].ptr, nf, n, v["d_power"].ptr), check)
    row("pss_power_db", "k_pairwise", f"{nf}x{n}")(make)


_power_db(5, 1000)
_power_db(3, 8200)


def _iq_correction(nf, n, fam):
    def make():
        x = _distinct(LC.iq_frames(nf, n, seed=4))

        def check(out):
            import oracle_lib as O
            want = np.stack(_frames(O.iq_correction, x))
            _same("corrected samples (bits)", out["d_out_iq"], want.view(np.float32).reshape(nf, n, 2))
            _same("RAW = real part (bits)", out["d_raw"], want.real)
        return case("pss_iq_correction", fam, f"{nf}x{n}", [A("d_iq", "complex64", x), Out("d_out_iq", "complex64", nf, n, 2), Out("d_raw", "float32", nf, n)],
                    lambda v: _engine().iq_correction(v["d_iq"].ptr, nf, n, v["d_out_iq"].ptr, v["d_raw"].ptr), check)
    row("pss_iq_correction", fam, f"{nf}x{n}")(make)


_iq_correction(5, 1024, "k_iqcorr_staged_wave_tree")
_iq_correction(3, 1000, "k_iqcorr_staged")
_iq_correction(2, 8200, "k_iqcorr")


@row("pss_agc_steps", "k_agc", "257")
def _agc():
    n = 257
    p = (np.random.default_rng(5).uniform(-70, 0, n)).astype(np.float32)

    def check(out):
        import oracle_lib as O
        idx, want = 3, []
        for v in p:
            idx = O.agc_step(v, idx, 8)
            want.append(idx)
        _same("gain indices", out["d_idx_out"], np.array(want, np.int32))
    return case("pss_agc_steps", "k_agc", "257", [A("d_power", "float32", p), Out("d_idx_out", "int32", n)],
                lambda v: _engine().agc_steps(v["d_power"].ptr, n, 3, 8, v["d_idx_out"].ptr), check)


def _c128(entry, nf, n, fam):
    def make():
        x = _distinct(LC.c128_frames(nf, n, seed=6))
        outs = [Out("d_power", "float64", nf)] if entry == "pss_mean_power_c128" else [Out("d_pcm", "pcm16", nf, n, 2), Out("d_audio", "float64", nf, n)]

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            if entry == "pss_mean_power_c128":
                e.mean_power_c128(p["d_iq"], nf, n, p["d_power"])
            elif entry == "pss_demod_am_c128":
                e.demod_am_c128(p["d_iq"], nf, n, p["d_pcm"], p["d_audio"])
            else:
                e.demod_ssb_c128(p["d_iq"], nf, n, 48000.0, p["d_pcm"], p["d_audio"])

        def check(out):
            import oracle_lib as O
            e = _engine()
            if entry == "pss_mean_power_c128":
                _same("mean power bits", out["d_power"], np.array(_frames(O.mean_power_c128, x)))
                return
            if entry == "pss_demod_am_c128":
                sos = _am_sos(e)
                want = np.stack(_frames(lambda r: O.demod_am_c128(r, sos), x))
                _same("float64 audio bits", out["d_audio"], want)
            else:
                taps = e.ssb_taps(48000.0)
                want = np.stack(_frames(lambda r: O.demod_ssb_c128(r, taps), x))
                _close("float64 audio (2e-14)", out["d_audio"], want, _ssb_tol())
            _same("int16 PCM", out["d_pcm"], _pcm(want))
        return case(entry, fam, f"{nf}x{n}", [A("d_iq", "complex128", x)] + outs, call, check)
    row(entry, fam, f"{nf}x{n}")(make)


_c128("pss_mean_power_c128", 3, 1000, "k_power_c128")
_c128("pss_demod_am_c128", 3, 512, "k_am_env_c128+k_sosfilt+k_norm_rows_f64")
_c128("pss_demod_ssb_c128", 3, 1000, "k_ssb_fir_f64+k_finalize")
_c128("pss_demod_ssb_c128", 3, 1024, "k_ssb_fir_f64+k_hilbert_r16")


# ---- element-wise and row kernels -----------------------------------------------------------------------------------------------------------------
def _np_f32(op):
    code = {"arctan2": L.NP_ARCTAN2, "log10": L.NP_LOG10, "abs": L.NP_ABS}[op]

    def make():
        n = 257
        rng = np.random.default_rng(code)
        a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
        b = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
        args = [A("d_a", "float32", a)] + ([A("d_b", "float32", b)] if op != "log10" else []) + [Out("d_out", "float32", n)]

        def check(out):
            import oracle_lib as O
            want = {"arctan2": lambda: O.atan2f(a, b), "log10": lambda: O.log10f(a), "abs": lambda: O.cabsf(a, b)}[op]()
            _same(f"np.{op} bits", out["d_out"], want)
        return case("pss_np_f32", "k_np_f32", f"{op}_{n}", args,
                    lambda v: _engine().np_f32(code, v["d_a"].ptr, v["d_b"].ptr if op != "log10" else None, n, v["d_out"].ptr), check)
    row("pss_np_f32", "k_np_f32", f"{op}_257")(make)


for _op in ("arctan2", "log10", "abs"):
    _np_f32(_op)


def _real_rows(nf, n, seed):
    rng = np.random.default_rng([91, n, seed])
    return _distinct(rng.standard_normal((nf, n)) * 10.0 ** rng.uniform(-3, 3, (nf, 1)))


@row("pss_row_normalise", "k_row_normalise", "3x257")
def _row_normalise():
    nf, n = 3, 257
    x = _real_rows(nf, n, 1)

    def check(out):
        _same("x / max|x| (bits)", out["d_y"], x / np.max(np.abs(x), axis=1, keepdims=True))
    return case("pss_row_normalise", "k_row_normalise", "3x257", [A("d_x", "float64", x), Out("d_y", "float64", nf, n)],
                lambda v: _engine().row_normalise(v["d_x"].ptr, nf, n, v["d_y"].ptr), check)


@row("pss_real_normalise", "k_real_normalise", "3x257")
def _real_normalise():
    nf, n = 3, 257
    x = _distinct(LC.fm_frames(nf, n, seed=7))

    def check(out):
        re = x.real.astype(np.float32)
        _same("real / max|real| in float32, widened (bits)", out["d_audio"], (re / np.max(np.abs(re), axis=1, keepdims=True)).astype(np.float64))
    return case("pss_real_normalise", "k_real_normalise", "3x257", [A("d_iq", "complex64", x), Out("d_audio", "float64", nf, n)],
                lambda v: _engine().real_normalise(v["d_iq"].ptr, nf, n, v["d_audio"].ptr), check)


@row("pss_sosfilt", "k_sosfilt", "65x257")
def _sosfilt():
    nf, n = 65, 257
    x = _real_rows(nf, n, 2)

    def check(out):
        import oracle_lib as O
        sos = _am_sos(_engine())
        _same("sosfilt rows (bits)", out["d_y"], np.stack(_frames(lambda r: O.sosfilt(sos, r), x)))
    return case("pss_sosfilt", "k_sosfilt", "65x257", [A("d_x", "float64", x), Out("d_y", "float64", nf, n)],
                lambda v: _engine().sosfilt(v["d_x"].ptr, nf, n, _am_sos(_engine()), v["d_y"].ptr), check)


@row("pss_lfilter", "k_lfilter", "65x257")
def _lfilter():
    nf, n = 65, 257
    x = _real_rows(nf, n, 3)
    b, a = np.array([0.2, 0.3, 0.1]), np.array([1.0, -0.5, 0.25])

    def check(out):
        from pyspecsdr_amd.engine import Engine
        _same("lfilter rows (bits of pss_h_lfilter)", out["d_y"], np.stack([Engine.h_lfilter(r, b, a) for r in x]))
    return case("pss_lfilter", "k_lfilter", "65x257", [A("d_x", "float64", x), Out("d_y", "float64", nf, n)],
                lambda v: _engine().lfilter(v["d_x"].ptr, nf, n, b, a, v["d_y"].ptr), check)


@row("pss_row_meter_f64", "k_row_meter_64", "5x1020")
def _row_meter_wave():
    return _row_meter(5, 1020)


@row("pss_row_meter_f64", "k_row_meter_256", "3x9000")
def _row_meter_wg():
    return _row_meter(3, 9000)


def _row_meter(nf, ln):
    rows = post_rows(nf, ln, np.float64, seed=700 + ln)

    def check(out):
        _same("np.max", out["d_peak"], rows.max(axis=1))
        _same("np.mean (bits)", out["d_avg"], np.array([np.mean(r) for r in rows]))
    return case("pss_row_meter_f64", "k_row_meter_64" if ln <= 2048 else "k_row_meter_256", f"{nf}x{ln}",
                [A("d_rows", "float64", rows), Out("d_peak", "float64", nf), Out("d_avg", "float64", nf)],
                lambda v: _engine().row_meter(v["d_rows"].ptr, nf, ln, v["d_peak"].ptr, v["d_avg"].ptr), check)


# ---- gates: the device lists against the host twins ------------------------------------------------------------------------------------------------
@row("pss_squelch_gate", "k_gate_flags+k_gate_scan+k_gate_index", "257")
def _squelch_gate():
    n = 257
    peak = np.random.default_rng(8).uniform(-80, -40, n)
    squelch = -60.0
    op, n_open, held = np.empty(n, np.uint8), C.c_long(), C.c_double()
    _host_twin(L.load().pss_h_squelch_gate, peak.ctypes.data, n, squelch, 3, 0, 0.0, op.ctypes.data, C.byref(n_open), C.byref(held))
    k = n_open.value
    assert 0 < k < n
    got = {}

    def call(v):
        got["r"] = _engine().squelch_gate(v["d_peak"].ptr, n, squelch, 3, 0, 0.0, v["d_open"].ptr, v["d_open_idx"].ptr)

    def check(out):
        assert got["r"] == (k, held.value), f"(n_open, held_out) = {got['r']}, the host gate's {(k, held.value)}"
        _same("open flags", out["d_open"], op)
        _same("open indices", out["d_open_idx"][:k], np.nonzero(op)[0].astype(np.int32))
        assert (out["d_open_idx"][k:].view(np.uint8) == V.FILL).all(), "entries behind the n_open-th were written"
    return case("pss_squelch_gate", "k_gate_flags+k_gate_scan+k_gate_index", "257",
                [A("d_peak", "float64", peak), Out("d_open", "uint8", n), Out("d_open_idx", "int32", n, sparse=True)], call, check)


@row("pss_scan_gate", "k_scan_flags+k_gate_scan+k_scan_index", "257")
def _scan_gate():
    n = 257
    rng = np.random.default_rng(9)
    peak, bw = rng.uniform(-60, 0, n).astype(np.float32), rng.uniform(0, 2e5, n)
    hit, idx, n_hit = np.empty(n, np.uint8), np.empty(n, np.int32), C.c_long()
    _host_twin(L.load().pss_h_scan_gate, peak.ctypes.data, bw.ctypes.data, n, -30.0, 50e3, hit.ctypes.data, idx.ctypes.data, C.byref(n_hit))
    k = n_hit.value
    assert 0 < k < n
    got = {}

    def call(v):
        got["r"] = _engine().scan_gate(v["d_peak"].ptr, v["d_bw"].ptr, n, -30.0, 50e3, v["d_hit"].ptr, v["d_hit_idx"].ptr)

    def check(out):
        assert got["r"] == k, f"n_hit = {got['r']}, the host gate's {k}"
        _same("hit flags", out["d_hit"], hit)
        _same("hit indices", out["d_hit_idx"][:k], idx[:k])
        assert (out["d_hit_idx"][k:].view(np.uint8) == V.FILL).all(), "entries behind the n_hit-th were written"
    return case("pss_scan_gate", "k_scan_flags+k_gate_scan+k_scan_index", "257",
                [A("d_peak", "float32", peak), A("d_bw", "float64", bw), Out("d_hit", "uint8", n), Out("d_hit_idx", "int32", n, sparse=True)], call, check)


# ---- scanner, classifier, decoders' front halves --------------------------------------------------------------------------------------------------
def _scan_iq(ns, n, seed):
    rng = np.random.default_rng([101, n, seed])
    return _distinct((0.05 * (rng.standard_normal((ns, n)) + 1j * rng.standard_normal((ns, n))) +
                      0.5 * np.exp(2j * np.pi * rng.uniform(-0.4, 0.4, (ns, 1)) * np.arange(n))).astype(np.complex64))


def _check_scan(out, iq, n, thr, fast=False):
    """fast (option scan_exact = 0: compute_fft's float32 evaluation of the dB value instead of NumPy's float32 chain): the bound grows by
    spectrum_bounds.fast_allowance, the evaluation error of db_of_fast that test_spectrum_db_rows_to_float64_accuracy grants the default rows.
    test_scan_past_the_cap's criteria: dB values within scan_ulp_bound plus the reference transform's allowance; peak, count and bandwidth
    equal to those recomputed from the device's own row."""
    import oracle_lib as O
    ref = (lambda x: O.scan_slice(x, FS)) if thr is None else (lambda x: O.scan_threshold(x, FS, thr))
    want = _frames(ref, iq)
    g, w = out["d_db"], np.stack([v[0] for v in want])
    with np.errstate(invalid="ignore", over="ignore"):
        allow = SB.scan_ulp_bound(w) + SB.db_allowance(w, SB.delta_f32_reference(iq)) + (SB.fast_allowance(w) if fast else 0.0)
    _close("dB values (scan_ulp_bound + the reference transform's allowance)", g, w, allow)
    for k in range(len(iq)):
        p = g[k].max()
        c = int(np.sum(g[k] > (p - np.float32(20) if thr is None else np.float32(thr))))
        assert out["d_peak"][k].tobytes() == p.tobytes() and int(out["d_count"][k]) == c and float(out["d_bw"][k]) == c * (FS / n), f"slice {k}: peak / count / bandwidth"


def _scan(entry, n, ns, fam, opts=None):
    thr = None if entry == "pss_scan" else -30.0

    def make():
        iq = _scan_iq(ns, n, 1)
        args = [A("d_iq", "complex64", iq), Out("d_db", "float32", ns, n), Out("d_peak", "float32", ns), Out("d_bw", "float64", ns), Out("d_count", "int32", ns)]

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            if thr is None:
                e.scan(p["d_iq"], ns, n, FS, p["d_db"], p["d_peak"], p["d_bw"], p["d_count"])
            else:
                e.scan_threshold(p["d_iq"], ns, n, FS, thr, p["d_db"], p["d_peak"], p["d_bw"], p["d_count"])
        return case(entry, fam, f"{ns}x{n}", args, call, lambda out: _check_scan(out, iq, n, thr, fast=bool(opts)), opts)
    row(entry, fam, f"{ns}x{n}")(make)


_scan("pss_scan", 1024, 5, "k_spectrum_r16_scan")
_scan("pss_scan", 64, 3, "k_spectrum_scan")
_scan("pss_scan", 8192, 2, "k_spectrum_xl_scan")
_scan("pss_scan", 1000, 3, "bluestein+k_scan_reduce")
_scan("pss_scan", 1024, 5, "k_spectrum_r16_scan_fast", {"scan_exact": 0})
_scan("pss_scan_threshold", 1000, 3, "bluestein+k_scan_reduce")
_scan("pss_scan_threshold", 2048, 3, "k_spectrum_r16_scan+k_scan_reduce")


def _classify_args(nf):
    return [Out("d_label", "int32", nf), Out("d_bw", "float64", nf), Out("d_mi", "float32", nf), Out("d_flat", "float32", nf), Out("d_psd", "float32", nf, 1024)]


def _check_classify(out, frames, n):
    """test_classify_past_the_cap's criteria."""
    import oracle_lib as O
    want = _frames(lambda x: O.classify(x, FS), frames)
    m = min(n, 1024)
    _same("label", out["d_label"], np.array([O.CLASS_LABELS.index(w[0]) for w in want], np.int32))
    _same("bandwidth", out["d_bw"], np.array([w[1] for w in want]))
    _same("modulation index bits", out["d_mi"], np.array([w[2] for w in want], np.float32))
    wf = np.array([w[3] for w in want], np.float32)
    _close("flatness (1e-5 relative)", out["d_flat"], wf, 1e-5 * np.abs(wf.astype(np.float64)))
    wp = np.stack([w[4] for w in want])
    _close("PSD (1e-6 relative + 1e-10)", out["d_psd"][:, :m], wp, 1e-6 * (wp.astype(np.float64) + 1e-10))


def _classify(n, fam):
    nf = 3

    def make():
        x = _distinct(LC.fm_frames(nf, n, seed=11))
        args = [A("d_iq", "complex64", x)] + _classify_args(nf)
        if n < 1024:
            args[-1] = Out("d_psd", "float32", nf, 1024, sparse=True)     # a short read fills min(n, 1024) values per row
        return case("pss_classify", fam, f"{nf}x{n}", args,
                    lambda v: _engine().classify(v["d_iq"].ptr, nf, n, FS, v["d_label"].ptr, v["d_bw"].ptr, v["d_mi"].ptr, v["d_flat"].ptr, v["d_psd"].ptr),
                    lambda out: _check_classify(out, x, n))
    row("pss_classify", fam, f"{nf}x{n}")(make)


_classify(1024, "k_cls_modidx+k_cls_welch")
_classify(1536, "k_cls_modidx+k_cls_welch")
_classify(600, "k_cls_modidx+k_cls_welch_short")


@row("pss_classify_gated", "k_cls_modidx_gated+k_cls_welch_gated", "2of5x1024")
def _classify_gated():
    nf, n = 5, 1024
    x = _distinct(LC.fm_frames(nf, n, seed=12))
    idx = np.array([1, 3], np.int32)
    args = [A("d_iq", "complex64", x), A("d_idx", "int32", idx)] + _classify_args(2)
    return case("pss_classify_gated", "k_cls_modidx_gated+k_cls_welch_gated", "2of5x1024", args,
                lambda v: _engine().classify_gated(v["d_iq"].ptr, nf, n, FS, v["d_idx"].ptr, 2, v["d_label"].ptr, v["d_bw"].ptr, v["d_mi"].ptr, v["d_flat"].ptr,
                                                   v["d_psd"].ptr),
                lambda out: _check_classify(out, x[idx], n))


def _sweep_iq(ns, n):
    """Slices of a sweep: wideband FM (deviation 300 kHz: tens of bins within 20 dB of the peak, a detection) on the even slices, a carrier over
    noise (a few bins: no detection) on the odd ones."""
    iq = _scan_iq(ns, n, 2)
    t = np.arange(n) / FS
    for k in range(0, ns, 2):
        ph = 2 * np.pi * 3e5 * np.cumsum(np.sin(2 * np.pi * (7e3 + 3e3 * k) * t)) / FS
        iq[k] = (0.5 * np.exp(1j * ph)).astype(np.complex64) + 0.1 * iq[k]
    return _distinct(iq)


@row("pss_sweep_report", "scan+gate+classify_gated", "inline_5x1024")
def _sweep_report():
    ns, n, thr, min_bw = 5, 1024, -30.0, 50e3
    iq = _sweep_iq(ns, n)
    args = [A("d_iq", "complex64", iq), Out("d_db", "float32", ns, n), Out("d_peak", "float32", ns), Out("d_bw", "float64", ns), Out("d_count", "int32", ns),
            Out("d_hit", "uint8", ns), Out("d_hit_idx", "int32", ns, sparse=True), Out("d_label", "int32", ns, sparse=True),
            Out("d_cls_bw", "float64", ns, sparse=True), Out("d_mi", "float32", ns, sparse=True), Out("d_flat", "float32", ns, sparse=True)]
    got = {}

    def call(v):
        p = {k: a.ptr for k, a in v.items()}
        got["n_hit"] = _engine().sweep_report("inline", p["d_iq"], ns, n, FS, thr, p["d_peak"], p["d_bw"], p["d_hit_idx"], min_bw, p["d_db"], p["d_count"],
                                              p["d_hit"], p["d_label"], p["d_cls_bw"], p["d_mi"], p["d_flat"])

    def check(out):
        """The scan's rows and numbers under its own criterion; the gate is pss_h_scan_gate's on those numbers; the classifier's results of the
        detections, in slice order, under test_classify_past_the_cap's criteria; entries behind the n_hit-th untouched."""
        import oracle_lib as O
        _check_scan(out, iq, n, None)
        peak, bw = np.ascontiguousarray(out["d_peak"]), np.ascontiguousarray(out["d_bw"])
        hit, idx, n_hit = np.empty(ns, np.uint8), np.empty(ns, np.int32), C.c_long()
        _host_twin(L.load().pss_h_scan_gate, peak.ctypes.data, bw.ctypes.data, ns, thr, min_bw, hit.ctypes.data, idx.ctypes.data, C.byref(n_hit))
        k = n_hit.value
        assert 0 < k < ns, f"{k} of {ns} slices are detections: the row needs both kinds"
        assert got["n_hit"] == k, f"n_hit = {got['n_hit']}, the host gate's {k}"
        _same("hit flags", out["d_hit"], hit)
        _same("hit indices", out["d_hit_idx"][:k], idx[:k])
        want = _frames(lambda x: O.classify(x, FS), iq[idx[:k]])
        _same("label", out["d_label"][:k], np.array([O.CLASS_LABELS.index(w[0]) for w in want], np.int32))
        _same("classifier bandwidth", out["d_cls_bw"][:k], np.array([w[1] for w in want]))
        _same("modulation index bits", out["d_mi"][:k], np.array([w[2] for w in want], np.float32))
        wf = np.array([w[3] for w in want], np.float32)
        _close("flatness (1e-5 relative)", out["d_flat"][:k], wf, 1e-5 * np.abs(wf.astype(np.float64)))
        for name in ("d_hit_idx", "d_label", "d_cls_bw", "d_mi", "d_flat"):
            assert (np.ascontiguousarray(out[name][k:]).view(np.uint8) == V.FILL).all(), f"{name}: entries behind the n_hit-th were written"
    return case("pss_sweep_report", "scan+gate+classify_gated", "inline_5x1024", args, call, check)


@row("pss_morse_edges", "k_morse_edges", "3x300")
def _morse_edges():
    nf, n, cap = 3, 300, 151
    rng = np.random.default_rng(13)
    key = np.repeat(rng.integers(0, 2, (nf, n // 20 + 1)), 20, axis=1)[:, :n] * rng.uniform(0.05, 1.0, (nf, 1))
    iq = _distinct((key * np.exp(0.2j * np.arange(n)) + 1e-3 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64))

    def check(out):
        import oracle_lib as O
        for f, (r, fl) in enumerate(_frames(O.morse_edges, iq)):
            assert tuple(out["d_counts"][f]) == (len(r), len(fl)), f"frame {f}: counts {tuple(out['d_counts'][f])}, want {(len(r), len(fl))}"
            _same(f"rise indices of frame {f}", out["d_rise"][f, :len(r)], r)
            _same(f"fall indices of frame {f}", out["d_fall"][f, :len(fl)], fl)
    return case("pss_morse_edges", "k_morse_edges", "3x300",
                [A("d_iq", "complex64", iq), Out("d_rise", "int32", nf, cap, sparse=True), Out("d_fall", "int32", nf, cap, sparse=True), Out("d_counts", "int32", nf, 2)],
                lambda v: _engine().morse_edges(v["d_iq"].ptr, nf, n, cap, v["d_rise"].ptr, v["d_fall"].ptr, v["d_counts"].ptr), check)


def _afsk_sos():
    """The band-pass tables of the AFSK fixture (tests/golden/afsk.npz), as test_afsk_bits_past_the_cap hands them to both sides."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "afsk.npz"))
    return np.ascontiguousarray(g["sos1200_a"]), np.ascontiguousarray(g["sos2200_a"])


@row("pss_afsk_bits", "k_sosfilt+k_afsk_bits", "3x5000")
def _afsk_bits():
    nf, n, fs = 3, 5000, 22050.0
    x = _real_rows(nf, n, 4)
    nb = int(L.load().pss_afsk_n_bits(n, fs))
    s1, s2 = _afsk_sos()

    def check(out):
        import oracle_lib as O
        _same("bits (the oracle's)", out["d_bits"], np.stack(_frames(lambda r: O.afsk_bits(r, fs, s1, s2), x)))
    return case("pss_afsk_bits", "k_sosfilt+k_afsk_bits", "3x5000", [A("d_audio", "float64", x), Out("d_bits", "uint8", nf, nb)],
                lambda v: _engine().afsk_bits(v["d_audio"].ptr, nf, n, fs, v["d_bits"].ptr, s1, s2), check)


# ---- one loop iteration per read buffer: compositions of the rows above (pinned byte for byte to the separate calls by test_gpu_parity) ---------------
def _pipeline(entry, mode, name, nf, n, display="waterfall", opts=None, f64=False, fam=None):
    disp_w, dh = 112 if nf % 2 else 111, 36
    el = "float64" if f64 else "float32"
    n_out = _out_len(mode, n, FS)

    def make():
        x = _distinct((LC.iq_frames if mode == L.MODE_WFM else LC.fm_frames)(nf, n, seed=120 + mode))
        args = [A("d_iq", "complex64", x), Out("d_db", el, nf, n), Out("d_post", el, nf, n - 4), Out("d_row_lo", el, nf), Out("d_row_hi", el, nf),
                Out("d_line_a", "int8", nf, disp_w)] + ([Out("d_line_b", "int8", nf, disp_w)] if display != "persistence" else []) + [Out("d_pcm", "pcm16", nf, n_out, 2)]

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            common = (p["d_iq"], nf, n, FS, p["d_db"], p["d_post"], p["d_row_lo"], p["d_row_hi"], disp_w, p["d_line_a"], p.get("d_line_b"), p["d_pcm"])
            if entry == "pss_frame_pipeline_nfm":
                e.frame_pipeline_nfm(*common)
            elif entry == "pss_frame_pipeline_nfm_f64":
                e.frame_pipeline_nfm_f64(*common)
            elif entry == "pss_frame_pipeline":
                e.frame_pipeline(mode, *common, display=display, disp_h=dh)
            else:
                e.frame_pipeline_f64(mode, *common, display=display, disp_h=dh)

        def check(out):
            import test_gpu_spectrum_accuracy as SA
            _same("int16 PCM", out["d_pcm"], _pcm_of(mode, _demod_oracle(mode, x, FS, signal=True)))
            SA.check_rows("f64" if f64 else "fast", out["d_db"], x, SA.oracle_rows(x), n, "dB rows of a view")

            def separate(p):       # test_frame_pipeline_modes_equal_separate_calls: every output byte for byte
                e = _engine()
                e.demod_signal(mode, p["d_iq"], nf, n, FS, p["d_pcm"], None)
                if f64:
                    e.spectrum_db_f64(p["d_iq"], nf, n, p["d_db"])
                    e.spectrum_post_f64(p["d_db"], nf, n, p["d_post"], p["d_row_lo"], p["d_row_hi"])
                else:
                    e.spectrum_db(p["d_iq"], nf, n, p["d_db"])
                    e.spectrum_post_extremes(p["d_db"], nf, n, p["d_post"], p["d_row_lo"], p["d_row_hi"])
                _lines_separately(e, p, display, f64, nf, n - 4, disp_w, dh)
            want, _ = _separate({"d_iq": x}, {a.name: (a.layout, a.shape) for a in args if not a.is_input}, separate)
            _same_outputs("one call against the separate calls", out, want)
        return case(entry, fam or f"{name}+spectrum+post+{display}", f"{nf}x{n}", args, call, check, opts)
    row(entry, fam or f"{name}+spectrum+post+{display}", f"{nf}x{n}")(make)


_pipeline("pss_frame_pipeline_nfm", L.MODE_NFM, "nfm_small_batch", 17, 1024)
_pipeline("pss_frame_pipeline_nfm", L.MODE_NFM, "nfm_fused", 65, 1024, opts={"small_batch": 0})
_pipeline("pss_frame_pipeline", L.MODE_WFM, "wfm_small_batch", 17, 1024, "persistence")
_pipeline("pss_frame_pipeline", L.MODE_WFM, "wfm_fused", 65, 1024, "gradient", opts={"small_batch": 0})
_pipeline("pss_frame_pipeline", L.MODE_AM, "am", 13, 1024, "waterfall")
_pipeline("pss_frame_pipeline", L.MODE_USB, "usb", 3, 8192, "persistence")
_pipeline("pss_frame_pipeline_nfm_f64", L.MODE_NFM, "nfm_small_batch", 17, 1024, f64=True)
_pipeline("pss_frame_pipeline_nfm_f64", L.MODE_NFM, "nfm_fused_f64_plain", 65, 1024, opts={"small_batch": 0, "f64_plain": 1}, f64=True)
_pipeline("pss_frame_pipeline_f64", L.MODE_AM, "am", 13, 2048, "gradient", f64=True)
_pipeline("pss_frame_pipeline_f64", L.MODE_WFM, "wfm_fused", 65, 1024, "persistence", opts={"small_batch": 0}, f64=True)


# the squelch rows: the gate starts open (held_in above the squelch) and closes at the first metered frame, whose peak is far below it:
# frames 0 .. 2 are open, the others closed, whatever the spectra are -- so the open frames are gathered and the PCM is compacted
SQUELCH_DB, HELD_IN = 1000.0, 2000.0


def _cells_pipeline(entry, mode, name, nf, n, display="waterfall", opts=None, db64=True):
    got = {}
    disp_w, dh = 112 if nf % 2 else 111, 36
    n_out = _out_len(mode, n, FS)
    demod = entry != "pss_spectrum_cells"
    squelch = entry == "pss_frame_pipeline_squelch"
    fam = f"{name}+" + ("k_spectrum_post" if n == 1024 and not (opts or {}).get("fuse_post") == 0 else "spectrum_f64+post_sel") + f"+{display}" + ("" if db64 else "_db32")

    def make():
        x = _distinct((LC.iq_frames if mode == L.MODE_WFM else LC.fm_frames)(nf, n, seed=140 + mode))
        args = [A("d_iq", "complex64", x), Out("d_db32", "float32", nf, n)] + ([Out("d_db64", "float64", nf, n)] if db64 else []) + \
               [Out("d_row_lo", "float64", nf), Out("d_row_hi", "float64", nf), Out("d_line_a", "int8", nf, disp_w)] + \
               ([Out("d_line_b", "int8", nf, disp_w)] if display != "persistence" else []) + \
               ([Out("d_pcm", "pcm16", nf, n_out, 2, sparse=squelch)] if demod else []) + \
               ([Out("d_peak", "float64", nf), Out("d_avg", "float64", nf), Out("d_open", "uint8", nf)] if squelch else [])

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            rows = (p["d_db32"], p.get("d_db64"), p["d_row_lo"], p["d_row_hi"], disp_w, p["d_line_a"], p.get("d_line_b"))
            if entry == "pss_spectrum_cells":
                e.spectrum_cells(p["d_iq"], nf, n, *rows, display=display, disp_h=dh)
            elif entry == "pss_frame_pipeline_cells":
                e.frame_pipeline_cells(mode, p["d_iq"], nf, n, FS, *rows, p["d_pcm"], display=display, disp_h=dh)
            else:
                got["gate"] = e.frame_pipeline_squelch(mode, p["d_iq"], nf, n, FS, *rows, p["d_pcm"], SQUELCH_DB, p["d_peak"], p["d_avg"], p["d_open"],
                                                       held_in=HELD_IN, display=display, disp_h=dh)

        def check(out):
            import test_gpu_spectrum_accuracy as SA
            ref = SA.oracle_rows(x)
            if db64:
                SA.check_rows("f64", out["d_db64"], x, ref, n, "float64 dB rows of a view")
                _same("float32 rows are the float64 rows rounded once", out["d_db32"], out["d_db64"].astype(np.float32))
            else:
                SA.check_rows("exact", out["d_db32"], x, ref, n, "float32 dB rows of a view")
            if demod and not squelch and mode in (L.MODE_NFM, L.MODE_AM, L.MODE_WFM):
                _same("int16 PCM", out["d_pcm"], _pcm_of(mode, _demod_oracle(mode, x, FS, signal=True)))

            def separate(p):       # the float64 chain and the demodulator as separate calls: every output byte for byte
                e = _engine()
                e.spectrum_db_f64(p["d_iq"], nf, n, p["d_db64"])
                e.spectrum_post_f64(p["d_db64"], nf, n, p["d_post"], p["d_row_lo"], p["d_row_hi"])
                _lines_separately(e, p, display, True, nf, n - 4, disp_w, dh)
                e.row_meter(p["d_post"], nf, n - 4, p["d_peak"], p["d_avg"])
                e.demod_signal(mode, p["d_iq"], nf, n, FS, p["d_pcm"], None)
            spec = {"d_db64": ("float64", (nf, n)), "d_post": ("float64", (nf, n - 4)), "d_row_lo": ("float64", (nf,)), "d_row_hi": ("float64", (nf,)),
                    "d_line_a": ("int8", (nf, disp_w)), "d_line_b": ("int8", (nf, disp_w)), "d_peak": ("float64", (nf,)), "d_avg": ("float64", (nf,)),
                    "d_pcm": ("pcm16", (nf, n_out, 2))}
            want, _ = _separate({"d_iq": x}, spec, separate)
            _same_outputs("one call against the separate calls", out, want,
                          [k for k in out if k in want and not (k == "d_pcm" and squelch)])
            if squelch:            # the gate is the host twin's on the meter's peaks; the PCM is that of the open frames, compacted
                peak = np.ascontiguousarray(out["d_peak"])
                op, n_open, held = np.empty(nf, np.uint8), C.c_long(), C.c_double()
                _host_twin(L.load().pss_h_squelch_gate, peak.ctypes.data, nf, SQUELCH_DB, 3, 0, HELD_IN, op.ctypes.data, C.byref(n_open), C.byref(held))
                k = n_open.value
                assert k == 3, f"{k} open frames"
                assert got["gate"] == (k, held.value), f"(n_open, held_out) = {got['gate']}, the host gate's {(k, held.value)}"
                _same("open flags", out["d_open"], op)
                _same("int16 PCM of the open frames, compacted", out["d_pcm"][:k], want["d_pcm"][op.astype(bool)])
                assert (np.ascontiguousarray(out["d_pcm"][k:]).view(np.uint8) == V.FILL).all(), "PCM rows behind the n_open-th were written"
        return case(entry, fam, f"{nf}x{n}", args, call, check, opts)
    row(entry, fam, f"{nf}x{n}")(make)


_cells_pipeline("pss_frame_pipeline_cells", L.MODE_NFM, "nfm_small_batch", 17, 1024)
_cells_pipeline("pss_frame_pipeline_cells", L.MODE_NFM, "nfm_fused", 65, 1024, opts={"small_batch": 0}, db64=False)
_cells_pipeline("pss_frame_pipeline_cells", L.MODE_NFM, "nfm_fused", 65, 1024, "persistence", opts={"small_batch": 0, "fuse_post": 0})
_cells_pipeline("pss_frame_pipeline_cells", L.MODE_WFM, "wfm_fused", 65, 1024, "gradient", opts={"small_batch": 0}, db64=False)
_cells_pipeline("pss_frame_pipeline_cells", L.MODE_AM, "am", 13, 2048)
_cells_pipeline("pss_spectrum_cells", L.MODE_NFM, "display", 5, 1024)
_cells_pipeline("pss_spectrum_cells", L.MODE_NFM, "display", 5, 1024, "persistence", db64=False)
_cells_pipeline("pss_spectrum_cells", L.MODE_NFM, "display", 3, 4096, "gradient")
_cells_pipeline("pss_frame_pipeline_squelch", L.MODE_NFM, "squelch_nfm", 17, 1024)
_cells_pipeline("pss_frame_pipeline_squelch", L.MODE_AM, "squelch_am", 13, 1024, "persistence", db64=False)


def _view_pipeline(view, mode, name, nf, n):
    entry = f"pss_frame_pipeline_{view}"
    disp_w, dh, max_h, max_w = 111, 30, 40, 119
    n_out = _out_len(mode, n, FS)
    words = (max_w + 31) // 32

    def make():
        x = _distinct((LC.iq_frames if mode == L.MODE_WFM else LC.fm_frames)(nf, n, seed=160 + mode))
        outs = {"bars": [Out("d_height", "int8", nf, disp_w), Out("d_level", "int8", nf, disp_w), Out("d_range", "float64", nf, 2)],
                "surface": [Out("d_mag", "int8", nf, disp_w), Out("d_range", "float64", nf, 2)],
                "vector": [Out("d_mask", "int32", nf, max_h, words)]}[view]
        args = [A("d_iq", "complex64", x), Out("d_db32", "float32", nf, n), Out("d_db64", "float64", nf, n), Out("d_post", "float64", nf, n - 4)] + outs + \
               [Out("d_pcm", "pcm16", nf, n_out, 2)]

        def call(v):
            e, p = _engine(), {k: a.ptr for k, a in v.items()}
            head = (mode, p["d_iq"], nf, n, FS, p["d_db32"], p["d_db64"], p["d_post"])
            if view == "bars":
                e.frame_pipeline_bars(*head, dh, disp_w, p["d_height"], p["d_level"], p["d_range"], p["d_pcm"])
            elif view == "surface":
                e.frame_pipeline_surface(*head, disp_w, p["d_mag"], p["d_range"], p["d_pcm"])
            else:
                e.frame_pipeline_vector(*head, max_h, max_w, p["d_mask"], p["d_pcm"])

        def check(out):
            import oracle_lib as O
            import test_gpu_spectrum_accuracy as SA
            SA.check_rows("f64", out["d_db64"], x, SA.oracle_rows(x), n, "float64 dB rows of a view")
            _same("float32 rows are the float64 rows rounded once", out["d_db32"], out["d_db64"].astype(np.float32))
            _same("post-processed rows (bits of the oracle's, from the device's dB rows)", out["d_post"], np.stack(_frames(O.postprocess, out["d_db64"])))
            _same("int16 PCM", out["d_pcm"], _pcm_of(mode, _demod_oracle(mode, x, FS, signal=True)))

            def separate(p):       # the view's own entry point on the post-processed rows (the masks: on the read buffers)
                e = _engine()
                e.spectrum_db_f64(p["d_iq"], nf, n, p["d_db64"])
                e.spectrum_post_f64(p["d_db64"], nf, n, p["d_post"])
                if view == "bars":
                    e.spectrum_bars(p["d_post"], nf, n - 4, dh, disp_w, p["d_height"], p["d_level"], p["d_range"], f64=True)
                elif view == "surface":
                    e.surface_mags(p["d_post"], nf, n - 4, disp_w, p["d_mag"], p["d_range"], f64=True)
                else:
                    e.vector_masks(p["d_iq"], nf, n, max_h, max_w, p["d_mask"])
            want, _ = _separate({"d_iq": x}, {a.name: (a.layout, a.shape) for a in args if not a.is_input and a.name not in ("d_db32", "d_pcm")}, separate)
            _same_outputs("one call against the separate calls", out, want)
        return case(entry, f"{name}+spectrum_f64+post_f64+{view}", f"{nf}x{n}", args, call, check)
    row(entry, f"{name}+spectrum_f64+post_f64+{view}", f"{nf}x{n}")(make)


_view_pipeline("bars", L.MODE_NFM, "nfm_small_batch", 17, 1024)
_view_pipeline("surface", L.MODE_AM, "am", 13, 1024)
_view_pipeline("vector", L.MODE_WFM, "wfm_small_batch", 17, 1024)


@row("pss_spectrum_nfm", "nfm_fused+k_spectrum_r16", "65x1024")
def _spectrum_nfm():
    return _make_spectrum_nfm(65, 1024, {"small_batch": 0}, "nfm_fused+k_spectrum_r16")


@row("pss_spectrum_nfm", "nfm_small_batch+k_spectrum_r16", "17x1024")
def _spectrum_nfm_small():
    return _make_spectrum_nfm(17, 1024, None, "nfm_small_batch+k_spectrum_r16")


def _make_spectrum_nfm(nf, n, opts, fam):
    x = _distinct(LC.fm_frames(nf, n, seed=180))
    n_out = _out_len(L.MODE_NFM, n, FS)

    def check(out):
        import test_gpu_spectrum_accuracy as SA
        SA.check_rows("fast", out["d_db"], x, SA.oracle_rows(x), n, "rows of a view")
        _same("int16 PCM", out["d_pcm"], _pcm_of(L.MODE_NFM, _demod_oracle(L.MODE_NFM, x, FS)))
    return case("pss_spectrum_nfm", fam, f"{nf}x{n}", [A("d_iq", "complex64", x), Out("d_db", "float32", nf, n), Out("d_pcm", "pcm16", nf, n_out, 2)],
                lambda v: _engine().spectrum_nfm(v["d_iq"].ptr, nf, n, FS, v["d_db"].ptr, v["d_pcm"].ptr), check, opts)


# ---- the decoders' device halves ----------------------------------------------------------------------------------------------------------------------
def _morse_iq(nf, n):
    rng = np.random.default_rng(14)
    key = np.repeat(rng.integers(0, 2, (nf, n // 40 + 1)), 40, axis=1)[:, :n] * rng.uniform(0.2, 1.0, (nf, 1))
    return _distinct((key * np.exp(0.2j * np.arange(n)) + 1e-3 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64))


def _check_morse_text(out, frames, fs):
    """test_gpu_decode_batch.same_as_host: pulses, text, its length and the timing bits of the host twin pss_h_morse_decode."""
    import test_gpu_decode_batch as DB
    DB.same_as_host([(np.ascontiguousarray(r), np.ascontiguousarray(f)) for r, f in frames], fs,
                    (out["d_text"], out["d_text_len"], out["d_timing"], out["d_pulses"]))


@row("pss_decode_morse_batch", "k_morse_edges+k_morse_text", "3x2000")
def _decode_morse_batch():
    nf, n, cap = 3, 2000, 1001
    iq = _morse_iq(nf, n)
    args = [A("d_iq", "complex64", iq), Out("d_rise", "int32", nf, cap, sparse=True), Out("d_fall", "int32", nf, cap, sparse=True), Out("d_counts", "int32", nf, 2),
            Out("d_text", "uint8", nf, 2 * cap, sparse=True), Out("d_text_len", "int32", nf), Out("d_timing", "float64", nf, 3), Out("d_pulses", "int32", nf)]

    def call(v):
        p = {k: a.ptr for k, a in v.items()}
        _engine().decode_morse_batch(p["d_iq"], nf, n, 8000.0, p["d_rise"], p["d_fall"], p["d_counts"], p["d_text"], p["d_text_len"], p["d_timing"], p["d_pulses"])

    def check(out):
        import oracle_lib as O
        for f, (r, fl) in enumerate(_frames(O.morse_edges, iq)):
            assert tuple(out["d_counts"][f]) == (len(r), len(fl)), f"frame {f}: counts"
            _same(f"rise indices of frame {f}", out["d_rise"][f, :len(r)], r)
            _same(f"fall indices of frame {f}", out["d_fall"][f, :len(fl)], fl)
        _check_morse_text(out, [(out["d_rise"][f, :out["d_counts"][f, 0]], out["d_fall"][f, :out["d_counts"][f, 1]]) for f in range(nf)], 8000.0)
    return case("pss_decode_morse_batch", "k_morse_edges+k_morse_text", "3x2000", args, call, check)


@row("pss_morse_text", "k_morse_text", "3x2000")
def _morse_text():
    import oracle_lib as O
    nf, n, cap = 3, 2000, 1001
    iq = _morse_iq(nf, n)
    rise, fall, counts = np.zeros((nf, cap), np.int32), np.zeros((nf, cap), np.int32), np.zeros((nf, 2), np.int32)

    for f in range(nf):           # the edge lists pss_morse_edges leaves for these frames, from the oracle
        r, fl = O.morse_edges(iq[f])
        rise[f, :len(r)], fall[f, :len(fl)], counts[f] = r, fl, (len(r), len(fl))
    assert counts.min() > 2, "a frame without keying"
    args = [A("d_rise", "int32", rise), A("d_fall", "int32", fall), A("d_counts", "int32", counts), Out("d_text", "uint8", nf, 2 * cap, sparse=True),
            Out("d_text_len", "int32", nf), Out("d_timing", "float64", nf, 3), Out("d_pulses", "int32", nf)]

    def call(v):
        p = {k: a.ptr for k, a in v.items()}
        _engine().morse_text(p["d_rise"], p["d_fall"], p["d_counts"], nf, cap, 8000.0, p["d_text"], p["d_text_len"], p["d_timing"], p["d_pulses"])
    frames = [(rise[f, :counts[f, 0]], fall[f, :counts[f, 1]]) for f in range(nf)]
    return case("pss_morse_text", "k_morse_text", "3x2000", args, call, lambda out: _check_morse_text(out, frames, 8000.0))


@row("pss_ax25_frames", "k_ax25_frames", "5x2000")
def _ax25_frames():
    nf, nb, cap = 5, 2000, 330
    rng = np.random.default_rng(15)
    flag = np.array([0, 1, 1, 1, 1, 1, 1, 0], np.uint8)
    bits = np.zeros((nf, nb), np.uint8)
    for f in range(nf):           # rows 0 .. 2: a flag, a bit-stuffed payload of 20 + f bytes, a flag, in front of noise; rows 3, 4: random bits with two flags
        if f >= 3:
            bits[f] = rng.integers(0, 2, nb)
            bits[f, 40 + f:48 + f] = flag
            bits[f, 1200 + 8 * f:1208 + 8 * f] = flag
            continue
        payload, ones, stuffed = np.unpackbits(rng.integers(0, 256, 20 + f).astype(np.uint8), bitorder="little"), 0, []
        for b in payload:
            stuffed.append(b)
            ones = ones + 1 if b else 0
            if ones == 5:
                stuffed.append(0)
                ones = 0
        frame = np.concatenate([flag, np.array(stuffed, np.uint8), flag])
        bits[f, 40 + f:40 + f + len(frame)] = frame
        bits[f, 1000:] = rng.integers(0, 2, nb - 1000)
    _distinct(bits)
    args = [A("d_bits", "uint8", bits), Out("d_out", "uint8", nf, cap, sparse=True), Out("d_out_len", "int32", nf)]
    return case("pss_ax25_frames", "k_ax25_frames", "5x2000", args,
                lambda v: _engine().ax25_frames(v["d_bits"].ptr, nf, nb, cap, v["d_out"].ptr, v["d_out_len"].ptr),
                lambda out: _check_ax25(out, bits, at_least=1))


def _check_ax25(out, rows, at_least=0):
    """test_gpu_decode_batch.ax_same_as_host's criterion with this harness's fill: the packet of the host twin pss_h_ax25_frame and its true
    length, -1 and nothing written for a row without one, nothing written behind a packet."""
    import test_gpu_decode_batch as DB
    n_packets = 0
    for k, r in enumerate(rows):
        h = DB.host_ax25(r)
        if h is None:
            assert out["d_out_len"][k] == -1 and (out["d_out"][k] == V.FILL).all(), f"row {k}: no packet on the host, length {out['d_out_len'][k]}"
            continue
        n_packets += 1
        keep = min(len(h), out["d_out"].shape[1])
        assert out["d_out_len"][k] == len(h) and out["d_out"][k, :keep].tobytes() == h[:keep], f"row {k}: packet of {out['d_out_len'][k]} bytes, the host's {len(h)}"
        assert (out["d_out"][k, keep:] == V.FILL).all(), f"row {k}: bytes behind the packet were written"
    assert n_packets >= at_least, f"{n_packets} rows hold a packet"


@row("pss_decode_aprs_batch", "k_real_normalise+k_sosfilt+k_afsk_bits+k_ax25_frames", "3x5000")
def _decode_aprs_batch():
    nf, n, fs, cap = 3, 5000, 22050.0, 330
    x = _distinct(LC.fm_frames(nf, n, seed=16))
    nb = int(L.load().pss_afsk_n_bits(n, fs))
    args = [A("d_iq", "complex64", x), Out("d_audio", "float64", nf, n), Out("d_bits", "uint8", nf, nb), Out("d_out", "uint8", nf, cap, sparse=True),
            Out("d_out_len", "int32", nf)]

    def check(out):
        re = x.real.astype(np.float32)
        _same("normalised audio (bits)", out["d_audio"], (re / np.max(np.abs(re), axis=1, keepdims=True)).astype(np.float64))

        def separate(p):           # test_decode_aprs_batch_call_equals_normalise_bits_frames: work buffers included, byte for byte
            e = _engine()
            e.real_normalise(p["d_iq"], nf, n, p["d_audio"])
            e.afsk_bits(p["d_audio"], nf, n, fs, p["d_bits"])
            e.ax25_frames(p["d_bits"], nf, nb, cap, p["d_out"], p["d_out_len"])
        want, _ = _separate({"d_iq": x}, {a.name: (a.layout, a.shape) for a in args if not a.is_input}, separate)
        _same_outputs("one call against the separate calls", out, want)
        _check_ax25(out, out["d_bits"])
    return case("pss_decode_aprs_batch", "k_real_normalise+k_sosfilt+k_afsk_bits+k_ax25_frames", "3x5000", args,
                lambda v: _engine().decode_aprs_batch(v["d_iq"].ptr, nf, n, fs, v["d_audio"].ptr, v["d_bits"].ptr, cap, v["d_out"].ptr, v["d_out_len"].ptr), check)


ENTRIES = sorted({r.entry for r in ROWS})

# every capped launch grid of launch_caps.CAPS -> (entry point, text in the family name) of the rows that run its kernels
CAPS_ROWS = {
    "classify": ("pss_classify", "k_cls_welch"), "classify_short": ("pss_classify", "k_cls_welch_short"), "morse": ("pss_morse_edges", "k_morse_edges"),
    "afsk": ("pss_afsk_bits", "k_afsk_bits"), "row_normalise": ("pss_row_normalise", "k_row_normalise"), "am_c128": ("pss_demod_am_c128", "k_am_env_c128"),
    "power_c128": ("pss_mean_power_c128", "k_power_c128"), "ssb_c128": ("pss_demod_ssb_c128", "k_ssb_fir_f64+k_finalize"), "np_f32": ("pss_np_f32", "k_np_f32"),
    "spectrogram": ("pss_spectrogram_cells", "k_spectrogram"), "vector": ("pss_vector_cells", "k_vector"), "scan": ("pss_scan", "k_scan_reduce"),
    "hilbert_long": ("pss_hilbert", "hilbert_long"), "hilbert_exact_long": ("pss_hilbert", "k_hilbert_pf_long"), "hilbert_exact": ("pss_hilbert", "k_hilbert_pf"),
    "hilbert_xl": ("pss_hilbert", "k_hilbert_xl"), "spectrum_f64_r16": ("pss_spectrum_db_f64", "k_spectrum_r16_f64"),
    "spectrum_f64_plain": ("pss_spectrum_db_f64", "k_spectrum_f64_plain"), "spectrum_c128": ("pss_spectrum_db_c128", "k_spectrum_c128"),
    "post_f64": ("pss_spectrum_post_f64", "k_post_f64"), "hilbert_r16": ("pss_hilbert", "k_hilbert_r16"), "hilbert_huge": ("pss_hilbert", "k_huge_hilbert"),
    "wfm_q1": ("pss_demod", "wfm_q1"),
}

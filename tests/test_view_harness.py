"""tests/view_util.py held to its own purpose: NumPy "entry points" on host arenas, one clean and one per fault the harness exists to find.
Each seeded fault must fail, and the report must name the entry point, the family, the shape, the call (A .. D), the buffer, the byte
relative to the payload and whether it lies in a guard."""
import numpy as np
import pytest

import view_util as V

N = 257


class Refused(Exception):
    def __init__(self, arg):
        super().__init__(f"fake_scale: {arg} must be 8-byte aligned")


def _x():
    return np.random.default_rng(5).standard_normal(N).astype(np.float32)


def _clean(v):
    v["y"].array[:] = v["x"].array.astype(np.float64) * 3.0


def _case(call, serve_y=True, x=None):
    x = _x() if x is None else x
    want = x.astype(np.float64) * 3.0

    def check(out):
        bad = np.nonzero(out["y"].view(np.uint64) != want.view(np.uint64))[0]
        assert bad.size == 0, f"y[{bad[0]}] = {out['y'][bad[0]]!r}, want {want[bad[0]]!r}"

    return V.Case("fake_scale", "k_fake", f"n={N}", [V.Arg("x", "float32", data=x), V.Arg("y", "float64", shape=(N,), serve=serve_y)], call,
                  check=check, refusal=Refused, is_refusal=lambda ex, names: all(f" {n} must" in str(ex) for n in names))


def _fails(call, *needles, **kw):
    with pytest.raises(V.ViewFailure) as info:
        V.run_case(_case(call, **kw), V.HostArenas(), log=lambda s: None)
    text = str(info.value)
    for needle in ("fake_scale [k_fake] n=257",) + needles:
        assert needle in text, f"the report does not say {needle!r}:\n{text}"
    return text


def test_a_clean_entry_point_passes():
    V.run_case(_case(_clean), V.HostArenas())


def test_arena_layout():
    """256-byte-aligned arenas, the payload one record in when padded, NaN words around float inputs, 0x7f everywhere in an output."""
    a = V.Arg("x", "float32", data=_x())
    for pad in (0, 4):
        view, arena = V.HostArenas().place(a, pad, a.image(pad))
        assert arena.ctypes.data % 256 == 0 and view.ptr == arena.ctypes.data + 4096 + pad and view.ptr % 4 == 0
        assert (view.ptr % 16 == 0) == (pad == 0)
        assert np.isnan(arena[:4096 + pad].view(np.float32)).all() and np.isnan(arena[4096 + pad + 4 * N:].view(np.float32)).all()
        assert len(arena) == 4096 + pad + 4 * N + 4096 and (view.array == _x()).all()
    o = V.Arg("pcm", "pcm16", shape=(N, 2))
    assert o.record == 4 and (o.image(4) == 0x7F).all() and len(o.image(4)) == 8192 + 4 + 4 * N
    codes = V.Arg("c", "uint8", data=np.arange(N, dtype=np.uint8))
    assert (codes.image(1)[:4097] == 0x7F).all() and (codes.image(1)[4097 + N:] == 0x7F).all()
    with pytest.raises(AssertionError):
        V.Arg("pcm", "pcm16", shape=(N,))     # half a record


def test_a_byte_written_into_the_guard_behind_the_output():
    def call(v):
        _clean(v)
        v["y"].arena[v["y"].off + v["y"].nbytes + 3] = 0

    _fails(call, "call A", "output y", "OUTSIDE the buffer", "3 into the guard behind it")


def test_a_byte_written_into_the_pad_in_front_of_the_output():
    def call(v):
        _clean(v)
        if v["y"].pad:
            v["y"].arena[v["y"].off - 2] = 0

    text = _fails(call, "call C", "call D", "byte -2 relative to the payload (in the pad in front of it)")
    assert "call A" not in text and "call B" not in text


def test_an_input_written():
    def call(v):
        _clean(v)
        v["x"].array[7] = 0.0

    _fails(call, "call A", "input x was WRITTEN", "byte 28 of the payload (element 7)")


def test_an_input_guard_written():
    def call(v):
        _clean(v)
        v["x"].arena[7] = 0

    _fails(call, "input x was WRITTEN", "byte -4089 relative to the payload (in the guard in front of it)")


def test_a_payload_byte_left_unwritten():
    def call(v):
        keep = v["y"].arena[v["y"].off + 100]
        _clean(v)
        v["y"].arena[v["y"].off + 100] = keep

    _fails(call, "call A", "the oracle criterion fails", "y[12]")


def test_an_element_left_unwritten():
    def call(v):
        keep = v["y"].array[N - 1]
        _clean(v)
        v["y"].array[N - 1] = keep

    _fails(call, "output y", "1 elements were never written", f"byte {8 * (N - 1)} of the payload (element {N - 1})")


def test_a_guard_nan_read_into_a_result():
    def call(v):
        _clean(v)
        x = v["x"]
        past = x.arena[x.off + x.nbytes:x.off + x.nbytes + 4].view(np.float32)[0]      # the load past the last element
        v["y"].array[N - 1] += 0.0 * float(past)

    _fails(call, "call A", "the oracle criterion fails", f"y[{N - 1}] = np.float64(nan)")


def test_a_result_that_depends_on_the_input_pointer():
    def call(v):
        _clean(v)
        if v["x"].ptr % 16:                       # a head loop that assumes the base
            v["y"].array[0] = 0.0

    text = _fails(call, "call B", "call D", "output y differs from the aligned call's", "of the payload (element 0)")
    assert "call C" not in text


def test_a_result_that_depends_on_the_output_pointer():
    def call(v):
        _clean(v)
        if v["y"].ptr % 16:
            v["y"].array[1:] = v["y"].array[:-1].copy()      # addresses rounded down to 16 bytes

    text = _fails(call, "call C", "call D", "of the payload (element 1)")
    assert "call B" not in text


def test_refusals():
    """A refused argument: the call must raise the refusal naming it and leave the outputs alone, in the calls that pad it and in no other."""
    def refusing(v):
        if v["y"].ptr % 16:
            raise Refused("y")
        _clean(v)

    V.run_case(_case(refusing, serve_y=False), V.HostArenas())
    _fails(_clean, "call C", "call D", "a refusal of y was expected, got a served call", serve_y=False)

    def late(v):                                   # refuses after it has written
        _clean(v)
        if v["y"].ptr % 16:
            raise Refused("y")

    _fails(late, "call C", "refused, yet output y was written", serve_y=False)

    def wrong_name(v):
        if v["y"].ptr % 16:
            raise Refused("x")
        _clean(v)

    _fails(wrong_name, "call C", "a refusal of y was expected, got Refused", serve_y=False)

    def everywhere(v):
        raise Refused("y")

    _fails(everywhere, "call A: raised Refused", serve_y=False)


def test_an_entry_point_that_is_not_reproducible_is_named_and_held_to_its_oracle():
    calls, said = [0], []

    def call(v):
        _clean(v)
        calls[0] += 1
        v["y"].array[3] = np.nextafter(v["y"].array[3], np.inf) if calls[0] % 2 else v["y"].array[3]

    x = _x()
    want = x.astype(np.float64) * 3.0
    c = _case(call, x=x)
    c.check = lambda out: np.testing.assert_allclose(out["y"], want, rtol=1e-12)
    V.run_case(c, V.HostArenas(), log=said.append)
    assert len(said) == 1 and "fake_scale [k_fake]" in said[0] and "NOT reproducible" in said[0] and "output y" in said[0]
    c.check = lambda out: np.testing.assert_array_equal(out["y"], want)
    with pytest.raises(V.ViewFailure, match="the oracle criterion fails"):
        V.run_case(c, V.HostArenas(), log=said.append)


def test_decision_counts():
    assert _case(_clean, serve_y=False).decisions() == (1, 1) and _case(_clean).decisions() == (2, 0)

"""The core device entry points on sample-aligned views of larger allocations, between guard bands (tests/view_util.py has the protocol,
tests/view_cases.py the rows: one per entry point and kernel family, at the smallest shape with two work items plus a partial one).

Every other core suite hands the library whole torch allocations, whose bases are 512-byte aligned and whose slack hides a stray access.
Here every buffer starts one RECORD off a 256-byte boundary (a complex64 sample, a float32 value, an int16 [L, R] pair ...: include/pss.h,
"pointer alignment") and lies between 4096-byte guards: quiet NaNs around float inputs, 0x7f bytes around everything else.  Per row:
the aligned call twice (reproducible?), then inputs padded, outputs padded, both; after each call the inputs and all guards must be
untouched and the payloads equal to the aligned call's byte for byte, and the aligned call itself is held to the oracle under the
criterion of the path's own test.  test_pointers_below_their_record are the refusals: PSS_E_ARG naming the argument, nothing written.

Measured on one MI355X: see NOTEBOOK.md, "Views of buffers".
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_util as G
import view_cases as VC
import view_util as V
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import PssError


@pytest.fixture(scope="module")
def arenas():
    return V.DeviceArenas(lambda: (G.engine().sync(), torch.cuda.synchronize()))


@pytest.mark.parametrize("row", VC.ROWS, ids=[r.id for r in VC.ROWS])
def test_views(row, arenas):
    case = row.make()
    assert case.check is not None, f"{case.head()}: call A of every row is held to an oracle"
    V.run_case(case, arenas)


def test_the_harness_sees_a_kernel_that_runs_past_its_buffers(arenas):
    """The device side of tests/test_view_harness.py: pss_np_f32 asked for three elements more than the payloads hold (inside the arenas'
    own guards: allocated memory of this test) reads NaN guard words and writes three values behind d_out; the harness must name the
    entry point, the call, the buffer and the first byte behind the payload."""
    n = 257
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    case = VC.case("pss_np_f32", "k_np_f32", f"abs_{n}+3", [VC.A("d_a", "float32", a), VC.A("d_b", "float32", b), VC.Out("d_out", "float32", n)],
                   lambda v: G.engine().np_f32(L.NP_ABS, v["d_a"].ptr, v["d_b"].ptr, n + 3, v["d_out"].ptr))
    with pytest.raises(V.ViewFailure) as info:
        V.run_case(case, arenas, log=lambda s: None)
    text = str(info.value)
    for which in "ABCD":
        line = [ln for ln in text.splitlines() if f"pss_np_f32 [k_np_f32] abs_{n}+3, call {which}: output d_out" in ln]
        assert len(line) == 1 and "bytes OUTSIDE the buffer were written" in line[0] and \
            f"first byte {4 * n} relative to the payload (0 into the guard behind it)" in line[0], text     # (a NaN's top byte is 0x7f, the fill)
    assert "input" not in text


def _first_of_each_entry():
    seen, rows = set(), []
    for r in VC.ROWS:
        if r.entry not in seen:
            seen.add(r.entry)
            rows.append(r)
    return rows


@pytest.mark.parametrize("row", _first_of_each_entry(), ids=[r.entry for r in _first_of_each_entry()])
def test_pointers_below_their_record(row, arenas):
    """Every argument whose record is wider than a byte, moved half a record off (a d_pcm at 2 bytes, a float32 row at 2, a float64 or
    complex64 buffer at 4): the entry point refuses with PSS_E_ARG and a message that names the argument, before anything is launched —
    no output byte changes, no input byte either."""
    case = row.make()
    wide = [a for a in case.args if a.record > 1]
    refuser = "pss_ring_push" if row.entry.startswith("pss_ring_") else row.entry       # the ring's rows come in through pss_ring_push
    if case.setup:
        case.setup()
    try:
        for target in wide:
            views, handles, before = {}, {}, {}
            for a in case.args:
                img = a.image(a.record)
                views[a.name], handles[a.name] = arenas.place(a, a.record, img)
                before[a.name] = img
            views[target.name].ptr -= target.record // 2
            head = f"{case.head()}, {target.name} {target.record // 2} bytes off its {target.record}-byte record"
            with pytest.raises(PssError) as info:
                case.call(views)
            arenas.sync()
            assert info.value.code == L.PSS_E_ARG and f" {target.name} must be {target.record}-byte aligned" in str(info.value) and \
                refuser + ":" in str(info.value), f"{head}: refused with {info.value}"
            for name, h in handles.items():
                assert np.array_equal(arenas.fetch(h), before[name]), f"{head}: refused, yet {name} was written"
    finally:
        if case.teardown:
            case.teardown()


def test_the_rows_reach_every_family_of_the_per_path_tests():
    """The option sets of test_gpu_length_sweep's NFM_PATHS / WFM_PATHS and the families of launch_caps.CAPS and
    test_gpu_spectrum_accuracy.family are all among the rows; the SSB tolerance the rows use is that test's."""
    import test_gpu_length_sweep as LS
    import test_gpu_spectrum_accuracy as SA
    assert {k: v[0] for k, v in VC.NFM_PATHS.items()} == LS.NFM_PATHS and {k: v[0] for k, v in VC.WFM_PATHS.items()} == LS.WFM_PATHS
    assert VC.NFM_PATHS["fused"][1] == 65 and 1024 in LS.FULL_TILE and 130 in LS.FULL_TILE
    assert VC.NFM_PATHS["small_batch"][1] == LS.IS_G1 and LS.AM_G1 == 13
    fams = {SA.family(n).split("<")[0].split("(")[0] for n, _ in VC.SPECTRUM_SHAPES}
    assert fams == {"k_spectrum", "k_spectrum_r16", "k_spectrum_xl", "k_spectrum_r16_big", "k_huge_p1/p2", "bluestein"}, fams
    for n, nf in VC.SPECTRUM_SHAPES[:5]:
        from launch_caps import r16_cfg
        assert nf == max(3, r16_cfg(n)[1] + 1), f"{n} points: FPW + 1 = {r16_cfg(n)[1] + 1} frames (at least 3), the row has {nf}"
    from launch_caps import CAPS
    assert set(VC.CAPS_ROWS) == set(CAPS), f"launch_caps.CAPS and view_cases.CAPS_ROWS differ: {sorted(set(CAPS) ^ set(VC.CAPS_ROWS))}"
    for key, (entry, text) in VC.CAPS_ROWS.items():
        assert CAPS[key].entry.split()[0].rstrip(",") == entry, f"CAPS[{key!r}] is {CAPS[key].entry}, CAPS_ROWS names {entry}"
        assert any(r.entry == entry and text in r.family for r in VC.ROWS), f"CAPS[{key!r}] ({CAPS[key].kernels}): no row of {entry} has {text!r} in its family"
    served = sum(r.make().decisions()[0] for r in VC.ROWS)
    print(f"{len(VC.ROWS)} rows over {len(VC.ENTRIES)} entry points, {served} arguments served at record alignment, 0 refused")

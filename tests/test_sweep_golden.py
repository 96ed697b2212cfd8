"""The scanner sweep report against tests/golden/sweep.npz (CPU only): the host gate pss_h_scan_gate and the duplicate removal
pss_h_scan_dedupe against what the reference's own sweeps did, formats.sweep_frequencies / scan_signals / scan_result_lines against its
records and the lines display_scan_results drew, and the argument checks.  Every comparison is equality of bits, bytes or strings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sweep_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats
from pyspecsdr_amd.engine import PssError, h_scan_dedupe, h_scan_gate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pss_scan_gate", "pss_h_scan_gate", "pss_classify_gated", "pss_sweep_report", "pss_h_scan_dedupe")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "sweep.npz"))


def golden_records(gold, prefix):
    return [{'frequency': float(f), 'power': p, 'bandwidth': b, 'type': str(t)}
            for f, p, b, t in zip(gold[prefix + "_freq"], gold[prefix + "_power"], gold[prefix + "_bw"], gold[prefix + "_type"])]


def golden_lines(gold, key):
    return [(int(y), int(x), str(t), int(p), bool(b)) for y, x, t, p, b in
            zip(gold[key + "_y"], gold[key + "_x"], gold[key + "_text"], gold[key + "_pair"], gold[key + "_bold"])]


def same_records(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == {'frequency', 'power', 'bandwidth', 'type'}
        assert type(g['frequency']) is float and type(g['power']) is np.float32 and type(g['bandwidth']) is np.float64 and type(g['type']) is str
        assert g['frequency'] == w['frequency'] and g['type'] == w['type']
        assert np.float32(g['power']).tobytes() == np.float32(w['power']).tobytes()
        assert np.float64(g['bandwidth']).tobytes() == np.float64(w['bandwidth']).tobytes()


def test_every_new_symbol_is_declared_exported_and_in_the_ctypes_table():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} is not declared in include/pss.h"
        assert hasattr(lib, name) and name in L._SIGS
    assert "PSS_SWEEP_INLINE = 0" in txt and "PSS_SWEEP_DRIVER = 1" in txt and (L.SWEEP_INLINE, L.SWEEP_DRIVER) == (0, 1)


def test_fixture_has_what_the_issue_lists(gold):
    assert [str(c) for c in gold["cases"]] == [c.name for c in S.CASES]
    assert {(c.kind, c.n) for c in S.CASES} == {("inline", 2048), ("inline", 4096), ("driver", 2048), ("driver", 5000), ("driver", 24000)}
    assert any(float(np.float32(c.threshold)) != c.threshold for c in S.CASES)          # a threshold that is not a float32 value
    for c in S.CASES:
        x = S.slices(c)
        assert 12 <= len(x) <= 16 and x.shape[1] == c.n and S.crc(x) == int(gold[f"crc_{c.name}"]), "the regenerated slices are the generator's"
        peak, bw, hit = gold[f"peak_{c.name}"], gold[f"bw_{c.name}"], gold[f"hit_{c.name}"]
        assert peak.dtype == np.float32 and bw.dtype == np.float64
        thr = np.float32(c.threshold)
        assert (~(peak > thr)).any(), "a slice below the threshold"
        assert ((peak > thr) & ~(bw > S.MIN_BW)).any(), "a slice above it but under 50 kHz"
        assert hit.any() and not hit.all()
        assert len(gold[f"labels_{c.name}"]) == int(hit.sum()) == len(gold[f"rec_{c.name}_freq"])
    assert {"FM_BROADCAST", "DIGITAL", "UNKNOWN"} <= {str(t) for c in S.CASES for t in gold[f"labels_{c.name}"]}


def test_host_gate_reproduces_every_golden_hit_list(gold):
    for c in S.CASES:
        hit, idx = h_scan_gate(gold[f"peak_{c.name}"], gold[f"bw_{c.name}"], c.threshold, S.MIN_BW)
        assert hit.dtype == np.uint8 and idx.dtype == np.int32
        assert np.array_equal(hit, gold[f"hit_{c.name}"]), c.name
        assert np.array_equal(idx, gold[f"hit_idx_{c.name}"]), c.name


def test_host_gate_compares_the_peak_in_float32(gold):
    c = S.case("inline_4096")
    assert c.threshold == -30.05
    peak, bw = gold[f"peak_{c.name}"].copy(), gold[f"bw_{c.name}"]
    i = int(gold[f"hit_idx_{c.name}"][0])
    cast = np.float32(c.threshold)
    assert float(cast) > c.threshold and not (cast > c.threshold)        # the larger real number, and still not above it: NEP 50
    peak[i] = cast
    assert h_scan_gate(peak, bw, c.threshold)[0][i] == 0
    peak[i] = np.nextafter(cast, np.float32(np.inf))
    assert h_scan_gate(peak, bw, c.threshold)[0][i] == 1
    peak[i] = np.nextafter(cast, np.float32(-np.inf))
    assert h_scan_gate(peak, bw, c.threshold)[0][i] == 0


def test_host_gate_edge_values():
    nan, inf = np.nan, np.inf
    peak = np.array([nan, 5, inf, -inf, 5, 5, 5, 5, inf], np.float32)
    bw = np.array([1e6, nan, 1e6, 1e6, 50e3, np.nextafter(50e3, inf), inf, -inf, nan], np.float64)
    hit, idx = h_scan_gate(peak, bw, 0.0, 50e3)
    assert hit.tolist() == [0, 0, 1, 0, 0, 1, 1, 0, 0] and idx.tolist() == [2, 5, 6]          # bw == min_bw: not a hit; a NaN never hits
    assert h_scan_gate(peak, bw, nan, 50e3)[0].sum() == 0 and h_scan_gate(peak, bw, 0.0, nan)[0].sum() == 0
    assert h_scan_gate(peak, bw, inf, 50e3)[0].sum() == 0
    assert h_scan_gate(peak, bw, -inf, -inf)[0].tolist() == [0, 0, 1, 0, 1, 1, 1, 0, 0]       # -inf > -inf is false on either side
    hit, idx = h_scan_gate(np.empty(0, np.float32), np.empty(0), 0.0)
    assert len(hit) == 0 and len(idx) == 0


def test_host_gate_and_dedupe_argument_errors():
    lib = L.load()
    peak, bw, n = np.zeros(4, np.float32), np.zeros(4), C.c_long(-7)
    assert lib.pss_h_scan_gate(None, bw.ctypes.data, 4, 0.0, 0.0, None, None, None) == L.PSS_E_ARG
    assert lib.pss_h_scan_gate(peak.ctypes.data, None, 4, 0.0, 0.0, None, None, None) == L.PSS_E_ARG
    assert lib.pss_h_scan_gate(peak.ctypes.data, bw.ctypes.data, -1, 0.0, 0.0, None, None, None) == L.PSS_E_ARG
    assert lib.pss_h_scan_gate(peak.ctypes.data, bw.ctypes.data, 1 << 31, 0.0, 0.0, None, None, None) == L.PSS_E_ARG
    assert lib.pss_h_scan_gate(None, None, 0, 0.0, 0.0, None, None, C.byref(n)) == 0 and n.value == 0
    assert lib.pss_h_scan_gate(peak.ctypes.data, bw.ctypes.data, 4, -1.0, -1.0, None, None, C.byref(n)) == 0 and n.value == 4   # outputs are optional
    f, keep = np.array([1e5, 2e5]), np.empty(2, np.int32)
    assert lib.pss_h_scan_dedupe(None, 2, 100e3, keep.ctypes.data, C.byref(n)) == L.PSS_E_ARG
    assert lib.pss_h_scan_dedupe(f.ctypes.data, 2, 100e3, None, C.byref(n)) == L.PSS_E_ARG
    assert lib.pss_h_scan_dedupe(f.ctypes.data, -1, 100e3, keep.ctypes.data, C.byref(n)) == L.PSS_E_ARG
    for grid in (0.0, -100e3, np.nan):
        assert lib.pss_h_scan_dedupe(f.ctypes.data, 2, grid, keep.ctypes.data, C.byref(n)) == L.PSS_E_ARG
    for bad in (np.nan, np.inf):
        with pytest.raises(PssError):
            h_scan_dedupe([1e5, bad])
    assert lib.pss_h_scan_dedupe(None, 0, 100e3, None, C.byref(n)) == 0 and n.value == 0
    assert len(h_scan_dedupe([])) == 0


def test_dedupe_equals_the_golden_kept_lists(gold):
    drivers = [c for c in S.CASES if c.kind == "driver"]
    assert drivers
    for c in drivers:
        keep = h_scan_dedupe(gold[f"rec_{c.name}_freq"], S.GRID_HZ)
        assert keep.dtype == np.int32 and np.array_equal(keep, gold[f"keep_{c.name}"]), c.name
    k = gold["keep_driver_2048"]
    assert len(k) < len(gold["rec_driver_2048_freq"]), "the 50 kHz sweep has duplicates to drop"


def python_dedupe(freqs, grid=100e3):
    """pyspecsdr.py:1084-1091 on bare frequencies, returning input indices."""
    unique, seen = [], set()
    for i in sorted(range(len(freqs)), key=lambda j: freqs[j]):
        rounded = round(freqs[i] / grid) * grid
        if rounded not in seen:
            seen.add(rounded)
            unique.append(i)
    return unique


def test_dedupe_rounds_half_to_even_and_sorts_stably():
    assert 88.05e6 / 100e3 == 880.5 and round(880.5) == 880                           # the tie goes to the even key, which 88.00 MHz holds
    quad = [88.00e6, 88.05e6, 88.10e6, 88.15e6]
    assert h_scan_dedupe(quad).tolist() == python_dedupe(quad) == [0, 2, 3]
    assert h_scan_dedupe([88.00e6, 88.05e6, 88.15e6]).tolist() == [0, 2]              # 88.05 shares 880 with 88.00; 88.15 goes to 882
    assert h_scan_dedupe([88.15e6, 88.25e6]).tolist() == python_dedupe([88.15e6, 88.25e6])
    freqs = [3.0e5, 1.0e5, 3.0e5, 1.4e5, 0.0, -1.0e5, 1.0e5, 2.5e5, 3.5e5, 1.5e5, -0.4e5]   # unsorted, with ties: the first of a tie wins
    assert h_scan_dedupe(freqs).tolist() == python_dedupe(freqs)
    assert h_scan_dedupe(freqs, 50e3).tolist() == python_dedupe(freqs, 50e3)
    rng = np.random.default_rng(3)
    freqs = (rng.integers(0, 400, 3000) * 25e3 + 88e6).tolist()
    assert h_scan_dedupe(freqs).tolist() == python_dedupe(freqs)


@pytest.mark.parametrize("start,end,step", [(88e6, 108e6, 100e3), (88e6, 89e6, 1e5 / 3), (108e6, 88e6, 100e3), (88e6, 88e6, 100e3)])
def test_sweep_frequencies_is_the_reference_loop(start, end, step):
    want, current_freq = [], start
    while current_freq <= end:
        want.append(current_freq)
        current_freq += step
    got = formats.sweep_frequencies(start, end, step)
    assert got.dtype == np.float64 and got.tolist() == want
    if (start, end, step) == (88e6, 108e6, 100e3):
        assert len(got) == 201
    if end < start:
        assert got.shape == (0,)


def test_sweep_frequencies_of_the_cases_and_accumulated_rounding(gold):
    for c in S.CASES:
        assert formats.sweep_frequencies(c.start, S.sweep_end(c), c.step).tobytes() == gold[f"freqs_{c.name}"].tobytes()
    step = 1e5 / 3
    got = formats.sweep_frequencies(88e6, 89e6, step)
    assert (got != 88e6 + np.arange(len(got)) * step).any(), "repeated addition, not start + i * step"


def test_scan_signals_equals_the_golden_records(gold):
    for c in S.CASES:
        args = (gold[f"freqs_{c.name}"], gold[f"peak_{c.name}"], gold[f"bw_{c.name}"], gold[f"hit_idx_{c.name}"])
        names = [str(t) for t in gold[f"labels_{c.name}"]]
        numbers = [formats._CLASS_NAMES.index(t) for t in names]
        for labels in (names, numbers, np.array(numbers, np.int32)):
            same_records(formats.scan_signals(*args, labels), golden_records(gold, f"rec_{c.name}"))
        if c.kind == "driver":
            same_records(formats.scan_signals(*args, names, dedupe=True), golden_records(gold, f"ded_{c.name}"))
    lib = L.load()
    assert [lib.pss_class_name(i).decode() for i in range(6)] == list(formats._CLASS_NAMES)
    assert formats.scan_signals([1.0], [0.0], [0.0], [], []) == []
    with pytest.raises(ValueError):
        formats.scan_signals([1.0], [0.0], [0.0], [0], [])


def test_scan_result_lines_equal_every_golden_line(gold):
    two_pages = 0
    for c in S.CASES:
        signals = golden_records(gold, f"ded_{c.name}" if c.kind == "driver" else f"rec_{c.name}")
        for hw in S.SCREENS:
            pages = (len(signals) + hw[0] - 8) // (hw[0] - 7)
            assert f"{S.lines_key(c, hw, pages)}_y" not in gold.files and pages >= 1
            two_pages += pages == 2
            for page in range(pages):
                want = golden_lines(gold, S.lines_key(c, hw, page))
                assert formats.scan_result_lines(signals, hw[0], hw[1], page) == want, (c.name, hw, page)
            with pytest.raises(ValueError):
                formats.scan_result_lines(signals, hw[0], hw[1], pages)
    assert two_pages >= 3
    want = [(int(y), int(x), str(t), int(p), False) for y, x, t, p in
            zip(gold["lines_empty_y"], gold["lines_empty_x"], gold["lines_empty_text"], gold["lines_empty_pair"])]
    assert formats.scan_result_lines([], 40, 120) == want and len(want) == 2


def test_scan_result_lines_colour_and_cut():
    sig = [{'frequency': 145.5e6, 'power': np.float32(-12.34), 'bandwidth': np.float64(12.5e3), 'type': t}
           for t in ("FM_BROADCAST", "DIGITAL", "UNKNOWN", "NARROW_FM", "SSB", "AM_BROADCAST")]
    lines = formats.scan_result_lines(sig, 40, 60)
    assert [l[3] for l in lines[2:8]] == [4, 5, 2, 1, 1, 1]                       # pyspecsdr.py:1245-1252
    assert all(len(l[2]) == 59 for l in lines[2:8]) and [l[0] for l in lines[2:8]] == list(range(2, 8))
    assert lines[2][2] == "  1.  145.500 MHz  Power:  -12.3 dB  BW:   12.5 kHz  Type: FM_BROADCAST   "[:59]
    assert lines[-2][0] == 39 and lines[-1] == (38, 0, "Enter choice: ", 1, True)

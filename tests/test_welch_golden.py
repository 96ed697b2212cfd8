"""The capture survey without a GPU: pss_h_welch (the host twin of k_welch / k_welch_fold: the statements of pyspecsdr_amd/csrc/pss_welch.h
with a radix-2 transform) against SciPy's own welch and spectrogram(mode='psd').max(-1) in float64 — the goldens of tests/golden/welch.npz
and, where SciPy is importable, a live call — inside the derived per-bin bound of tests/welch_bounds.py on every bin; the segment count,
every refusal by name, the default window, survey_signals and survey_freqs on hand-made rows, the header alone under the sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import welch_bounds as WB
import welch_cases as WC
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
NAMES = [c[0] for c in WC.CASES]


def h_call(x, n_rows, n, row_stride, nperseg, step, win, detrend, scale, mean, mx):
    """pss_h_welch as it is declared -> (code, reason)."""
    lib = L.load()
    p = lambda a: None if a is None else a.ctypes.data
    r = lib.pss_h_welch(p(x), n_rows, n, row_stride, nperseg, step, p(win), detrend, scale, p(mean), p(mx))
    return r, lib.pss_last_error(None).decode()


def host_rows(name):
    """pss_h_welch on a case's strided buffer -> (mean, max) [K][N]."""
    _, (_, N, S, _, _, detrend, scaling, _, kinds, _) = WC.case(name)
    buf, n = WC.case_rows(name)
    w = WC.case_window(name)
    mean, mx = np.full((len(kinds), N), -7.25), np.full((len(kinds), N), -7.25)
    r, why = h_call(buf, len(kinds), n, buf.shape[1], N, S, w, detrend, WC.scale_of(w, scaling), mean, mx)
    assert r == 0, why
    return mean, mx


def worst_fractions(name, mean, mx, ref_mean, ref_max, kappa=WB.KAPPA):
    """The worst fraction of the bound over every bin of every row of a case, for the mean and the max row."""
    _, (_, N, S, _, _, detrend, scaling, _, kinds, _) = WC.case(name)
    buf, n = WC.case_rows(name)
    w = WC.case_window(name)
    scale = WC.scale_of(w, scaling)
    fm = fx = 0.0
    for r in range(len(kinds)):
        R = WB.restate(buf[r, :n], N, S, w, detrend, scale)
        b_mean, b_max = WB.bounds(R, N, scale, kappa)
        fm = max(fm, WB.fraction(mean[r], ref_mean[r], b_mean))
        fx = max(fx, WB.fraction(mx[r], ref_max[r], b_max))
    return fm, fx


def test_cases_cover_what_they_are_meant_to():
    assert len(WC.CASES) == 16 and {c[1] for c in WC.CASES} == {256, 512, 1024, 2048, 4096} and {c[3] for c in WC.CASES} == {1, 2, 37}
    assert {c[5] for c in WC.CASES} == {0, 1} and {c[6] for c in WC.CASES} == {"density", "spectrum"} and {c[7] for c in WC.CASES} == {"hann", "hamming", "asym"}
    for _, N, S, *_ in WC.CASES:
        assert S in (N, N // 2, 3 * N // 8, N - 1, 1)
    w = WC.window("asym", 512)
    assert np.all(w > 0) and not np.allclose(w, w[::-1])
    src = open(os.path.join(CSRC, "pss_welch.h")).read()
    assert f"constexpr int BLOCK = {WC.BLOCK};" in src and f"constexpr int FOLD_Q = {WC.FOLD_Q};" in src
    assert f"constexpr long WELCH_GRID_CAP = {WC.GRID_CAP};" in open(os.path.join(CSRC, "pss_welch.hip")).read()
    # nan_max is pss_squelch.h's, restated for the host compiler: the two statements are held together here
    body = lambda txt: re.search(r"double nan_max\(double a, double b\)[^{]*\{\s*(.*?)\s*\}", txt, flags=re.S).group(1)
    assert body(src) == body(open(os.path.join(CSRC, "pss_squelch.h")).read()) == "return (b > a || b != b) ? b : a;"


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_is_inside_the_bound_of_every_golden(golden, name):
    g = golden["welch"]
    assert "stamp" in g.files
    _, (_, N, S, Lw, left, *_rest) = WC.case(name)
    buf, n = WC.case_rows(name)
    assert WC.crc(buf) == g["crc_" + name] and WC.crc(WC.case_window(name)) == g["wcrc_" + name], \
        f"{name}: welch_cases no longer regenerates what the golden was taken on"
    assert Engine.welch_segments(n, N, S) == Lw == int(g["L_" + name])
    mean, mx = host_rows(name)
    fm, fx = worst_fractions(name, mean, mx, g["mean_" + name], g["max_" + name])
    print(f"{name}: worst fraction of the bound: mean {fm:.4f} max {fx:.4f}")
    assert fm <= 1.0 and fx <= 1.0, (name, fm, fx)
    # the gaps between the rows are NaN: they were not read
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(mx))


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_is_inside_the_bound_of_a_live_scipy(name):
    ss = pytest.importorskip("scipy.signal")
    _, (_, N, S, Lw, _, detrend, scaling, _, kinds, _) = WC.case(name)
    buf, n = WC.case_rows(name)
    w = WC.case_window(name)
    kw = dict(fs=WC.FS, window=w, nperseg=N, noverlap=N - S, nfft=N, detrend="constant" if detrend else False, return_onesided=False, scaling=scaling)
    ref_mean = np.array([ss.welch(buf[r, :n].astype(np.complex128), average="mean", **kw)[1] for r in range(len(kinds))])
    ref_max = np.array([ss.spectrogram(buf[r, :n].astype(np.complex128), mode="psd", **kw)[2].max(-1) for r in range(len(kinds))])
    # through the Engine's defaults: the scale computed in NumPy, as SciPy does
    mean, mx = Engine.h_welch(np.ascontiguousarray(buf[:, :n]), N, S, window=w, detrend=bool(detrend), scaling=scaling, fs=WC.FS)
    fm, fx = worst_fractions(name, mean, mx, ref_mean, ref_max)
    assert fm <= 1.0 and fx <= 1.0, (name, fm, fx)
    hm, hx = host_rows(name)
    assert hm.tobytes() == mean.tobytes() and hx.tobytes() == mx.tobytes()      # the strided call gives the packed call's bytes


def test_the_numpy_restatement_of_the_bounds_is_scipys(golden):
    """welch_bounds.restate — where |X_k| and the norms of the bound come from — within 8 units of 2^-53 of the row's maximum."""
    g = golden["welch"]
    for name in NAMES:
        _, (_, N, S, _, _, detrend, scaling, _, kinds, _) = WC.case(name)
        buf, n = WC.case_rows(name)
        w = WC.case_window(name)
        for r in range(len(kinds)):
            R = WB.restate(buf[r, :n], N, S, w, detrend, WC.scale_of(w, scaling))
            for got, ref in ((R["mean"], g["mean_" + name][r]), (R["max"], g["max_" + name][r])):
                assert np.max(np.abs(got - ref)) <= 8 * WB.U * ref.max(), name


def test_max_row_is_optional_and_a_nan_takes_its_row_only():
    name = "rows3"
    _, (_, N, S, _, _, detrend, scaling, _, kinds, _) = WC.case(name)
    buf, n = WC.case_rows(name)
    w = WC.case_window(name)
    scale = WC.scale_of(w, scaling)
    mean, mx = host_rows(name)
    only = np.full_like(mean, -7.25)
    assert h_call(buf, 3, n, buf.shape[1], N, S, w, detrend, scale, only, None)[0] == 0 and only.tobytes() == mean.tobytes()
    for where in (0, n // 2, N + 36 * S - 1):          # the first sample, one in the middle, the last used one
        b = buf.copy()
        b[1, where] = np.nan
        m2, x2 = np.empty_like(mean), np.empty_like(mx)
        assert h_call(b, 3, n, b.shape[1], N, S, w, detrend, scale, m2, x2)[0] == 0
        assert not np.any(np.isfinite(m2[1])) and not np.any(np.isfinite(x2[1])), where
        assert m2[[0, 2]].tobytes() == mean[[0, 2]].tobytes() and x2[[0, 2]].tobytes() == mx[[0, 2]].tobytes()
    b = buf.copy()
    b[1, n - 1] = np.nan                               # behind the last segment: not used
    m2, x2 = np.empty_like(mean), np.empty_like(mx)
    assert h_call(b, 3, n, b.shape[1], N, S, w, detrend, scale, m2, x2)[0] == 0 and m2.tobytes() == mean.tobytes() and x2.tobytes() == mx.tobytes()


REFUSALS = [("nperseg not in", dict(nperseg=300)), ("nperseg not in", dict(nperseg=128)), ("nperseg not in", dict(nperseg=8192)),
            ("step outside", dict(step=0)), ("step outside", dict(step=257)), ("n < nperseg", dict(n=255, row_stride=255)), ("n_rows < 1", dict(n_rows=0)),
            ("n_rows < 1", dict(n_rows=-1)), ("row_stride < n", dict(row_stride=299)), ("null window", dict(win=None)), ("null mean", dict(mean=None)),
            ("null iq", dict(x=None)), ("detrend outside", dict(detrend=2)), ("detrend outside", dict(detrend=-1)), ("scale not finite", dict(scale=0.0)),
            ("scale not finite", dict(scale=-1.0)), ("scale not finite", dict(scale=np.inf)), ("scale not finite", dict(scale=np.nan))]


def test_segment_counts_and_every_refusal_by_name():
    lib = L.load()
    assert lib.pss_welch_segments(4096 + 36 * 2048 + 5, 4096, 2048) == 37 and lib.pss_welch_segments(255, 256, 1) == 0
    assert lib.pss_welch_segments(256, 256, 256) == 1 and lib.pss_welch_segments(511, 256, 256) == 1 and lib.pss_welch_segments(512, 256, 256) == 2
    assert lib.pss_welch_segments(99999744, 4096, 2048) == (99999744 - 4096) // 2048 + 1 and lib.pss_welch_segments(-5, 256, 1) == 0
    for bad in ((1000, 300, 1), (1000, 128, 1), (10000, 8192, 1), (1000, 256, 0), (1000, 256, 257)):
        assert lib.pss_welch_segments(*bad) == L.PSS_E_ARG, bad
    with pytest.raises(ValueError):
        Engine.welch_segments(1000, 300, 1)
    x = np.zeros((2, 300), np.complex64)
    w = np.ones(256)
    mean, mx = np.full((2, 256), -7.25), np.full((2, 256), -7.25)
    for what, change in REFUSALS:
        a = dict(x=x, n_rows=2, n=300, row_stride=300, nperseg=256, step=100, win=w, detrend=1, scale=1.0, mean=mean, mx=mx)
        a.update(change)
        r, why = h_call(a["x"], a["n_rows"], a["n"], a["row_stride"], a["nperseg"], a["step"], a["win"], a["detrend"], a["scale"], a["mean"], a["mx"])
        assert r == L.PSS_E_ARG and why.startswith("pss_h_welch: ") and what in why, (what, change, r, why)
        assert np.all(mean == -7.25) and np.all(mx == -7.25), what
    assert lib.pss_welch_default_window(300, w.ctypes.data) == L.PSS_E_ARG and lib.pss_welch_default_window(256, None) == L.PSS_E_ARG
    with pytest.raises(ValueError, match="window"):
        Engine.h_welch(x, 256, 100, window=np.ones(255))
    with pytest.raises(ValueError, match="scaling"):
        Engine.h_welch(x, 256, 100, scaling="psd")


def test_default_window_is_scipys_periodic_hann():
    ss = pytest.importorskip("scipy.signal")
    for N in (256, 512, 1024, 2048, 4096):
        want = ss.get_window("hann", N)
        assert np.max(np.abs(Engine.welch_c_window(N) - want)) <= 2.0 ** -53, N
        assert Engine.welch_default_window(N).tobytes() == want.tobytes()
        i = np.arange(N)
        assert np.max(np.abs(Engine.welch_c_window(N) - (0.5 - 0.5 * np.cos(2 * np.pi * i / N)))) <= 4 * 2.0 ** -53


def test_header_table_and_library_agree_on_the_new_entry_points():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    want = {"pss_welch_segments": (3, "long"), "pss_welch_default_window": (2, "int"), "pss_welch": (12, "int"), "pss_h_welch": (11, "int")}
    for name, (n_args, res) in want.items():
        m = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, f"{name} is not declared in include/pss.h"
        assert len(m.group(1).split(",")) == n_args == len(L._SIGS[name][1]), name
        assert L._SIGS[name][0] is (C.c_long if res == "long" else C.c_int) and hasattr(lib, name)
    assert ("pss_welch.hip", ["-ffp-contract=off"]) in __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS
    for name in ("welch", "h_welch", "welch_segments", "welch_default_window"):
        assert callable(getattr(Engine, name))
    for name in ("survey_freqs", "survey_recording", "survey_signals"):
        assert callable(getattr(F, name))


def test_survey_freqs():
    f = F.survey_freqs(2.4e6, 4096)
    assert f.shape == (4096,) and f[0] == -1.2e6 and f[2048] == 0.0 and np.all(np.diff(f) > 0) and f[-1] == 1.2e6 - 2.4e6 / 4096
    assert np.array_equal(f, np.fft.fftshift(np.fft.fftfreq(4096, 1 / 2.4e6)))


def test_survey_signals_on_hand_made_rows():
    fs, n = 1000.0, 100          # 10 Hz bins, bin k centred at (k - 50) * 10 Hz
    base = np.full(n, -80.0)

    def runs(row, **kw):
        return [s["bins"] for s in F.survey_signals(row, fs, **kw)]

    row = base.copy()
    row[0:3] = -50           # a run at the lower edge
    row[97:100] = -40        # and at the upper edge: no wrap-around joins them
    row[40:45] = -30
    row[42] = -20
    got = F.survey_signals(row, fs)
    assert [s["bins"] for s in got] == [(0, 2), (40, 44), (97, 99)]
    s = got[1]
    assert s["lo_hz"] == -105.0 and s["hi_hz"] == -55.0 and s["center_hz"] == -80.0 and s["bandwidth_hz"] == 50.0
    assert s["peak_hz"] == -80.0 and s["peak_db"] == -20.0
    assert got[0]["lo_hz"] == -505.0 and got[2]["hi_hz"] == 495.0 and got[0]["bandwidth_hz"] == 30.0
    assert [s["center_hz"] for s in got] == sorted(s["center_hz"] for s in got)
    # two runs one bin apart stay two
    row = base.copy()
    row[10:13] = -40
    row[14:17] = -40
    assert runs(row) == [(10, 12), (14, 16)]
    # a run shorter than min_bins is dropped
    row = base.copy()
    row[20] = -40
    row[30:32] = -40
    assert runs(row) == [(30, 31)] and runs(row, min_bins=1) == [(20, 20), (30, 31)] and runs(row, min_bins=3) == []
    # a NaN compares false: it splits the run it lies in, and is not part of the floor
    row = base.copy()
    row[60:67] = -40
    row[63] = np.nan
    assert runs(row) == [(60, 62), (64, 66)]
    # the threshold is strict, an all-equal row has no signal
    assert runs(base) == [] and runs(np.full(n, np.nan)) == []
    row = base.copy()
    row[5:8] = -70.0         # exactly floor + margin: not above it
    assert runs(row) == [] and runs(row, margin_db=9.5) == [(5, 7)]
    # an explicit floor
    row = base.copy()
    row[50:60] = -40
    assert runs(row, floor_db=-45.0, margin_db=10.0) == [] and runs(row, floor_db=-51.0) == [(50, 59)]
    assert runs(row, floor_db=-100.0) == [(0, 99)]
    with pytest.raises(ValueError):
        F.survey_signals(np.zeros((2, 4)), fs)


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/welch_host.cpp: pss_welch.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "welch_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "welch_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "welch_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

"""The capture survey on the MI355X (-m gpu): k_welch / k_welch_fold against SciPy's goldens and against the host twin inside the derived
bounds of tests/welch_bounds.py on every bin; equal bytes for equal calls and for a row alone or in a batch; a batch one work item past
the grid cap; guard words; the NaN rule; survey_recording and the signal list; every refusal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import welch_bounds as WB
import welch_cases as WC
from gpu_util import engine
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine, PssError

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard words in front of and behind every device buffer
G32, G64 = np.float32(-7.25), -7.25
NAMES = [c[0] for c in WC.CASES]


def run(buf, n, N, S, w, detrend, scale_kw, want_max=True, n_rows=None):
    """Engine.welch on the host buffer [K][row_stride] (complex64) with guard words around the input and both outputs ->
    (mean [K][N], max [K][N] or None); asserts that every guard word is untouched."""
    e = engine()
    K, stride = buf.shape if n_rows is None else (n_rows, buf.shape[1])
    flat = np.full(2 * GUARD + 2 * buf.size, G32, np.float32)
    flat[GUARD:GUARD + 2 * buf.size] = np.ascontiguousarray(buf).view(np.float32).ravel()
    d_in = torch.from_numpy(flat).cuda()
    d_mean = torch.full((2 * GUARD + K * N,), G64, dtype=torch.float64, device="cuda")
    d_max = torch.full((2 * GUARD + K * N,), G64, dtype=torch.float64, device="cuda")
    e.welch(d_in.data_ptr() + 4 * GUARD, K, n, N, S, d_mean.data_ptr() + 8 * GUARD, d_max.data_ptr() + 8 * GUARD if want_max else None, window=w,
            detrend=detrend, row_stride=stride, **scale_kw)
    e.sync()
    h_in, h_mean, h_max = d_in.cpu().numpy(), d_mean.cpu().numpy(), d_max.cpu().numpy()
    assert h_in.tobytes() == flat.tobytes(), "the input was written to"
    for h in (h_mean, h_max):
        assert np.all(h[:GUARD] == G64) and np.all(h[GUARD + K * N:] == G64), "a guard word of an output row was written to"
    if not want_max:
        assert np.all(h_max == G64), "the max row was written although it was not asked for"
    return h_mean[GUARD:GUARD + K * N].reshape(K, N), (h_max[GUARD:GUARD + K * N].reshape(K, N) if want_max else None)


def case_args(name):
    _, (_, N, S, _, _, detrend, scaling, _, kinds, _) = WC.case(name)
    buf, n = WC.case_rows(name)
    return buf, n, N, S, WC.case_window(name), bool(detrend), dict(scaling=scaling, fs=WC.FS)


@pytest.mark.parametrize("name", NAMES)
def test_device_is_inside_the_bound_of_every_golden(golden, name):
    g = golden["welch"]
    buf, n, N, S, w, detrend, kw = case_args(name)
    mean, mx = run(buf, n, N, S, w, detrend, kw)
    scale = WC.scale_of(w, kw["scaling"])
    fm = fx = 0.0
    for r in range(len(buf)):
        R = WB.restate(buf[r, :n], N, S, w, detrend, scale)
        b_mean, b_max = WB.bounds(R, N, scale)
        fm = max(fm, WB.fraction(mean[r], g["mean_" + name][r], b_mean))
        fx = max(fx, WB.fraction(mx[r], g["max_" + name][r], b_max))
    print(f"{name}: worst fraction of the bound: mean {fm:.4f} max {fx:.4f}")
    assert fm <= 1.0 and fx <= 1.0, (name, fm, fx)
    only, none = run(buf, n, N, S, w, detrend, kw, want_max=False)
    assert none is None and only.tobytes() == mean.tobytes()


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096])
def test_device_is_inside_the_bound_of_the_host_twin_over_a_grid_of_shapes(N):
    """Every (S, L) of the grid at this N; the rows of a batch (1 or 3), samples left over behind the last segment (0 or some), detrend and
    the max row (asked for or not) take turns so that every value of each meets every S and every L."""
    B = WC.BLOCK
    steps, counts = [1, N // 2 - 1, N // 2, N - 1, N], [1, 2, B - 1, B, B + 1, 2 * B + 3]
    worst, turn = 0.0, 0
    for si, S in enumerate(steps):
        for li, Lw in enumerate(counts):
            K = (1, 3)[(si + li) % 2]
            left = 0 if S == 1 or (si + li // 2) % 2 == 0 else min(5, S - 1)      # a step of 1 leaves nothing over
            detrend = bool((si + li // 3 + turn) % 2)
            want_max = bool((si // 2 + li + turn) % 2) or Lw == 2 * B + 3
            turn += 1
            n = WC.n_of(N, S, Lw, left)
            gap = 3 if K > 1 else 0
            buf = np.full((K, n + gap), np.nan + 1j * np.nan, np.complex64)
            for r in range(K):
                buf[r, :n] = WC.signal(("noise", "tone", "dc")[(r + li) % 3], n, 7000 + 10 * turn + r)
            w = WC.window(("hann", "asym", "hamming")[turn % 3], N)
            kw = dict(scaling=("density", "spectrum")[turn % 2], fs=WC.FS)
            scale = WC.scale_of(w, kw["scaling"])
            assert Engine.welch_segments(n, N, S) == Lw
            mean, mx = run(buf, n, N, S, w, detrend, kw, want_max=want_max)
            h_mean, h_max = Engine.h_welch(np.ascontiguousarray(buf[:, :n]), N, S, window=w, detrend=detrend, want_max=want_max, **kw)
            for r in range(K):
                R = WB.restate(buf[r, :n], N, S, w, detrend, scale)
                b_mean, b_max = WB.bounds(R, N, scale, WB.KAPPA_TWIN)
                f = WB.fraction(mean[r], h_mean[r], b_mean)
                if want_max:
                    f = max(f, WB.fraction(mx[r], h_max[r], b_max))
                assert f <= 1.0, (N, S, Lw, K, left, detrend, want_max, r, f)
                worst = max(worst, f)
    print(f"N = {N}: worst fraction of the twin bound {worst:.4f}")


@pytest.mark.parametrize("Lw", [WC.BLOCK * WC.FOLD_Q + 1, WC.BLOCK * (7 * WC.FOLD_Q + 2) + 5])
def test_more_blocks_than_chunks_are_inside_the_bound_of_the_host_twin(Lw):
    """The fold's chunks hold more than one block partial from L = BLOCK FOLD_Q + 1 on (chunks of two, the last ones empty) and eight
    from L = 7 BLOCK FOLD_Q + 1 on, where k_welch_fold reads eight partials at a time (here: 56 chunks of eight, one of two)."""
    N, S = 256, 16
    n = WC.n_of(N, S, Lw, 3)
    nb = -(-Lw // WC.BLOCK)
    assert -(-nb // WC.FOLD_Q) == (2 if Lw < 4000 else 8)
    buf = np.stack([WC.signal("noise", n, 81), WC.signal("dc", n, 82)])
    w = WC.window("asym", N)
    kw = dict(scaling="density", fs=WC.FS)
    scale = WC.scale_of(w, "density")
    mean, mx = run(buf, n, N, S, w, True, kw)
    h_mean, h_max = Engine.h_welch(buf, N, S, window=w, detrend=True, **kw)
    for r in range(2):
        R = WB.restate(buf[r], N, S, w, True, scale)
        b_mean, b_max = WB.bounds(R, N, scale, WB.KAPPA_TWIN)
        assert WB.fraction(mean[r], h_mean[r], b_mean) <= 1.0 and WB.fraction(mx[r], h_max[r], b_max) <= 1.0, r
    one, _ = run(buf[1:2], n, N, S, w, True, kw, want_max=False)
    assert one[0].tobytes() == mean[1].tobytes()


@pytest.mark.parametrize("name", ["rows3", "n4096_half", "n256_half"])
def test_equal_calls_give_equal_bytes_and_a_row_is_the_same_alone_or_in_a_batch(name):
    buf, n, N, S, w, detrend, kw = case_args(name)
    if len(buf) == 1:      # three rows of it, the second and third shifted
        buf = np.stack([buf[0], np.roll(buf[0], 17), buf[0][::-1]])
    a_mean, a_max = run(buf, n, N, S, w, detrend, kw)
    b_mean, b_max = run(buf, n, N, S, w, detrend, kw)
    assert a_mean.tobytes() == b_mean.tobytes() and a_max.tobytes() == b_max.tobytes()
    for r in range(len(buf)):
        m1, x1 = run(buf[r:r + 1], n, N, S, w, detrend, kw)
        assert m1[0].tobytes() == a_mean[r].tobytes() and x1[0].tobytes() == a_max[r].tobytes(), r


def test_a_batch_one_work_item_past_the_grid_cap_equals_its_rows_one_by_one():
    """N = 256 puts 16 work items into a workgroup and L = 1 one work item into a row: GRID_CAP * 16 + 1 rows of 256 samples are the
    smallest batch whose last item is walked by the grid-stride loop."""
    e = engine()
    N, K = 256, WC.GRID_CAP * 16 + 1
    rng = np.random.default_rng(11)
    buf = (rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))).astype(np.complex64)
    buf[:, 0] += np.arange(K)          # no two rows alike
    w = WC.window("asym", N)
    d_in = torch.from_numpy(buf.view(np.float32)).cuda()
    d_all = torch.full((2, K, N), G64, dtype=torch.float64, device="cuda")
    d_one = torch.full((2, K, N), G64, dtype=torch.float64, device="cuda")
    e.welch(d_in, K, N, N, N, d_all[0], d_all[1], window=w, detrend=True)
    for r in range(K):
        e.welch(d_in.data_ptr() + 8 * N * r, 1, N, N, N, d_one.data_ptr() + 8 * N * r, d_one.data_ptr() + 8 * N * (K + r), window=w, detrend=True)
    e.sync()
    a, b = d_all.cpu().numpy(), d_one.cpu().numpy()
    assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes()
    h_mean, h_max = Engine.h_welch(buf[-2:], N, N, window=w, detrend=True)
    assert np.allclose(a[0, -2:], h_mean, rtol=0, atol=1e-9 * h_mean.max()) and np.allclose(a[1, -2:], h_max, rtol=0, atol=1e-9 * h_max.max())


def test_a_nan_in_a_used_segment_takes_every_bin_of_its_row_and_no_other_row():
    buf, n, N, S, w, detrend, kw = case_args("rows3")
    mean, mx = run(buf, n, N, S, w, detrend, kw)
    for where in (0, n // 2, N + 36 * S - 1):
        b = buf.copy()
        b[1, where] = np.nan
        for det in (True, False):
            m0, x0 = (mean, mx) if det == detrend else run(buf, n, N, S, w, det, kw)
            m2, x2 = run(b, n, N, S, w, det, kw)
            assert not np.any(np.isfinite(m2[1])) and not np.any(np.isfinite(x2[1])), (where, det)
            assert m2[[0, 2]].tobytes() == m0[[0, 2]].tobytes() and x2[[0, 2]].tobytes() == x0[[0, 2]].tobytes(), (where, det)
    b = buf.copy()
    b[1, n - 1] = np.nan               # behind the last segment: not used
    m2, x2 = run(b, n, N, S, w, detrend, kw)
    assert m2.tobytes() == mean.tobytes() and x2.tobytes() == mx.tobytes()


def _welch_of(x, N, step, **kw):
    """Engine.welch on an uploaded capture -> (mean, max) in FFT order, through the engine survey_recording uses."""
    from pyspecsdr_amd.signal_processing import get_engine
    e = get_engine()
    d_iq = torch.from_numpy(np.ascontiguousarray(x, np.complex64).view(np.float32)).cuda()
    d_rows = torch.empty((2, N), dtype=torch.float64, device="cuda")
    e.welch(d_iq, 1, len(x), N, step, d_rows[0], d_rows[1], **kw)
    e.sync()
    return d_rows.cpu().numpy()


def test_survey_recording_is_one_welch_call_on_the_uploaded_capture():
    n, N, fs = 50000, 1024, 2.4e6
    x = WC.signal("noise", n, 31)
    want = _welch_of(x, N, 512, fs=fs)
    for chunk in (1 << 22, 7777):
        s = F.survey_recording(x, fs, nperseg=N, chunk_samples=chunk)
        assert s["n_segments"] == Engine.welch_segments(n, N, 512) == 96 and s["nperseg"] == N and s["step"] == 512
        assert s["mean"].tobytes() == np.fft.fftshift(want[0]).tobytes() and s["max"].tobytes() == np.fft.fftshift(want[1]).tobytes(), chunk
        assert np.array_equal(s["freqs_hz"], F.survey_freqs(fs, N))
        assert s["mean_db"].tobytes() == (10 * np.log10(s["mean"] + 1e-10)).tobytes() and s["max_db"].tobytes() == (10 * np.log10(s["max"] + 1e-10)).tobytes()
    # other arguments reach the call: a window, no detrend, 'spectrum', an overlap of 3 / 4
    w = WC.window("asym", N)
    want = _welch_of(x, N, 256, window=w, detrend=False, scaling="spectrum", fs=fs)
    s = F.survey_recording(x, fs, nperseg=N, overlap=0.75, window=w, detrend=False, scaling="spectrum", chunk_samples=10001)
    assert s["step"] == 256 and s["mean"].tobytes() == np.fft.fftshift(want[0]).tobytes() and s["max"].tobytes() == np.fft.fftshift(want[1]).tobytes()
    # cu8 codes: unpacked on the device, chunk by chunk
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
    want = _welch_of(F.unpack_iq(codes, "cu8"), N, 512, fs=fs)
    for chunk in (1 << 22, 7777):
        s = F.survey_recording(codes, fs, nperseg=N, chunk_samples=chunk, codes_format="cu8")
        assert s["mean"].tobytes() == np.fft.fftshift(want[0]).tobytes() and s["max"].tobytes() == np.fft.fftshift(want[1]).tobytes(), chunk
    with pytest.raises(ValueError, match="shorter"):
        F.survey_recording(x[:1000], fs, nperseg=N)


def test_survey_finds_three_carriers_of_known_offsets_and_widths():
    fs, N, n = 2.4e6, 4096, 4096 * 64
    carriers = ((-600e3, 50e3, 0.3), (150e3, 25e3, 0.2), (700e3, 100e3, 0.3))
    x = WC.carriers_capture(n, fs, carriers)
    s = F.survey_recording(x, fs, nperseg=N)
    assert s["n_segments"] == 127
    bin_hz = fs / N
    for row in (s["mean_db"], s["max_db"]):
        found = F.survey_signals(row, fs)
        assert len(found) == 3, [(f["center_hz"], f["bandwidth_hz"]) for f in found]
        for f, (off, width, _) in zip(found, carriers):
            assert abs(f["center_hz"] - off) <= bin_hz, (f, off)
            assert abs(f["bandwidth_hz"] - width) <= 6 * bin_hz, (f, width)       # the Hann main lobe widens an edge by up to two bins, the max row by more
            assert f["lo_hz"] < f["peak_hz"] < f["hi_hz"]


def test_every_refusal_comes_back_as_an_argument_error():
    e = engine()
    d_in = torch.zeros(2 * 2 * 300 + 2, dtype=torch.float32, device="cuda")
    d_mean = torch.full((2 * 256 + 1,), G64, dtype=torch.float64, device="cuda")
    d_max = torch.full((2 * 256 + 1,), G64, dtype=torch.float64, device="cuda")
    w = np.ones(256)
    base = dict(iq=d_in.data_ptr(), n_rows=2, n=300, row_stride=300, nperseg=256, step=100, win=w.ctypes.data, detrend=1, scale=1.0,
                mean=d_mean.data_ptr(), mx=d_max.data_ptr())
    changes = [("nperseg not in", dict(nperseg=300)), ("nperseg not in", dict(nperseg=128)), ("nperseg not in", dict(nperseg=8192)),
               ("step outside", dict(step=0)), ("step outside", dict(step=257)), ("n < nperseg", dict(n=255, row_stride=255)), ("n_rows < 1", dict(n_rows=0)),
               ("row_stride < n", dict(row_stride=299)), ("null window", dict(win=None)), ("null mean", dict(mean=None)), ("null iq", dict(iq=None)),
               ("detrend outside", dict(detrend=2)), ("scale not finite", dict(scale=0.0)), ("scale not finite", dict(scale=float("inf"))),
               ("scale not finite", dict(scale=float("nan"))), ("not aligned", dict(iq=d_in.data_ptr() + 4)), ("not aligned", dict(mx=d_max.data_ptr() + 4))]
    for what, change in changes:
        a = dict(base)
        a.update(change)
        r = e.lib.pss_welch(e.h, a["iq"], a["n_rows"], a["n"], a["row_stride"], a["nperseg"], a["step"], a["win"], a["detrend"], a["scale"], a["mean"], a["mx"])
        why = e.lib.pss_last_error(e.h).decode()
        assert r == L.PSS_E_ARG and why.startswith("pss_welch: ") and what in why, (what, r, why)
    e.sync()
    assert np.all(d_mean.cpu().numpy() == G64) and np.all(d_max.cpu().numpy() == G64)
    with pytest.raises(PssError):
        e.welch(d_in, 2, 300, 256, 0, d_mean)
    # the call itself is fine
    assert e.lib.pss_welch(e.h, *[base[k] for k in ("iq", "n_rows", "n", "row_stride", "nperseg", "step", "win", "detrend", "scale", "mean", "mx")]) == 0
    e.sync()
    assert np.all(d_mean.cpu().numpy()[:512] == 0.0)

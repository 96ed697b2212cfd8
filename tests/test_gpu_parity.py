"""GPU parity tests (run with -m gpu on an MI355X): HIP path through the C ABI vs
  (1) the golden vectors captured from the reference (tests/golden, tools/make_goldens.py) and
  (2) the CPU oracle (oracle/pss_oracle.c) on seeded inputs,
plus size-independent properties at larger batch sizes.

Bars: int16 PCM bit-exact; float64 audio bit-exact for NFM/AM (SSB: 2e-14, the reference's Hilbert FFT
round trip); float32 dB within 1e-4 RELATIVE of the reference's float64 value.
"""
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle_lib as O
import gpu_util as G
from pyspecsdr_amd import _lib as L


def rel_err(a, ref):
    return np.abs(a.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-300)


@pytest.mark.parametrize("n", [256, 1024, 2048, 4096, 8192, 16384])
def test_spectrum_vs_golden(golden, n):
    g = golden["spectrum"]
    iq, ref = g[f"iq_{n}"], g[f"db_{n}"]
    db = G.spectrum(iq)
    assert db.dtype == np.float32 and db.shape == ref.shape
    # north-star tolerance: 1e-4 relative on float32 dB, applied as a pure relative bound wherever |ref| > 1e-2 dB
    # and as 1e-6 dB absolute below that (relative error is ill-posed at a zero crossing of the dB scale)
    big = np.abs(ref) > 1e-2
    assert np.all(rel_err(db, ref)[big] <= 1e-4)
    assert np.all(np.abs(db - ref)[~big] <= 1e-6)
    assert np.max(np.abs(db - ref)) < 2e-5  # in practice: float32 rounding of the output only


def test_spectrum_db_exact_is_the_float32_rounding_of_the_reference_rows(golden):
    """Option "db_exact": compute_fft's dB rows evaluated to float64 accuracy and rounded once — the float32 row then IS the float32
    rounding of the reference's float64 row, every golden value of every kernel family (register FFT 256 .. 4096, four-stage
    8192 / 16384, Bluestein lengths).  The default float32 evaluation is 1-2 ulp from that, inside the 1e-4 contract."""
    g = golden["spectrum"]
    e = G.engine()
    sizes = [256, 1024, 2048, 4096, 8192, 16384] + [f"np2_{n}" for n in g["np2_sizes"]]
    for tag in sizes:
        iq, ref = g[f"iq_{tag}"], g[f"db_{tag}"]
        iq, ref = (iq[None], ref[None]) if iq.ndim == 1 else (iq, ref)
        want = ref.astype(np.float32)
        e.set_option("db_exact", 1)
        try:
            got = G.spectrum(iq)
        finally:
            e.set_option("db_exact", 0)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        fast = G.spectrum(iq)
        ulp = np.abs(fast.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 64 and np.all(np.abs(fast - want) <= 1e-6 * np.maximum(np.abs(want), 1.0)), (tag, int(ulp.max()))


def test_spectrum_zero_and_large(golden):
    z = np.zeros((3, 1024), np.complex64)
    assert np.all(np.abs(G.spectrum(z) + 100.0) <= 1e-4 * 100.0)   # reference: exactly -100.0
    rng = np.random.default_rng(5)
    for n in (32768, 65536):
        iq = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))).astype(np.complex64)
        db = G.spectrum(iq)
        ref = np.stack([O.compute_fft(f) for f in iq])
        assert np.all(np.abs(db - ref) <= 1e-4 * np.maximum(np.abs(ref), 1e-2))


@pytest.mark.parametrize("n", [131072, 262144, 524288, 1048576])
def test_spectrum_huge_frames(n):
    """The reference's largest read buffers (pyspecsdr.py:2236, SAMPLES = 9..12 -> 2^17..2^20 samples): two-pass
    256 x NS transform through a float64 scratch."""
    rng = np.random.default_rng(n)
    t = np.arange(n)
    iq = (0.3 * np.exp(2j * np.pi * 0.0371 * t) + 0.05 * (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n)))).astype(np.complex64)
    db = G.spectrum(iq)
    for f in (0, 2):
        ref = O.compute_fft(iq[f])
        assert np.all(np.abs(db[f] - ref) <= 1e-4 * np.maximum(np.abs(ref), 1e-2)), f
        assert np.max(np.abs(db[f] - ref)) < 1e-4


def test_spectrum_linearity_property():
    # Parseval at full batch width: sum |X|^2 = N * sum |w x|^2 for every frame (size-independent check)
    rng = np.random.default_rng(6)
    nf, n = 4096, 1024
    iq = (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))).astype(np.complex64) * np.float32(0.1)
    db = G.spectrum(iq).astype(np.float64)
    w = np.hamming(n)
    lhs = np.sum(10 ** (db / 10) - 1e-10, axis=1)
    rhs = n * np.sum(np.abs(iq.astype(np.complex128) * w) ** 2, axis=1)
    assert np.allclose(lhs, rhs, rtol=2e-6)


@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_post_process(golden, n):
    g = golden["spectrum"]
    e = G.engine()
    db64, ref = g[f"db_{n}"], g[f"post_{n}"]
    d_db = G.dev(db64.astype(np.float32))
    d_post = G.empty((db64.shape[0], n - 4), torch.float32)
    e.spectrum_post(d_db, db64.shape[0], n, d_post)
    e.sync()
    post = G.host(d_post)
    assert np.all(np.abs(post - ref) <= 1e-4 * np.maximum(np.abs(ref), 1.0))


@pytest.mark.parametrize("n", [8192, 16384, 32768, 65536, 1 << 20])
def test_post_process_long_rows(n):
    """pyspecsdr.py:2278-2283 on full read buffers (N = 32768 is the reference's default; up to 2^20): LDS sort up to
    8192, radix select above — against the NumPy formula on the float32 dB rows."""
    rng = np.random.default_rng(n)
    db = (rng.standard_normal((2, n)) * 6.0 - 35.0).astype(np.float32)
    db[0, 1000:1100] += 40.0                                  # a signal hump well above the noise floor
    db[1, :] = np.round(db[1, :])                             # heavy ties
    e = G.engine()
    d_post = G.empty((2, n - 4), torch.float32)
    e.spectrum_post(G.dev(db), 2, n, d_post)
    e.sync()
    post = G.host(d_post)
    for f in range(2):
        sm = np.convolve(db[f].astype(np.float64), np.ones(5) / 5, mode="valid")
        thr = np.median(sm) - 10
        ref = np.where(sm < thr, thr, sm)
        assert np.all(np.abs(post[f] - ref) <= 1e-4 * np.maximum(np.abs(ref), 1.0)), (n, f, np.abs(post[f] - ref).max())


@pytest.mark.parametrize("n", [8, 12, 256, 512, 1000, 1024, 2048, 4096, 8192, 16384, 20000, 32768, 32772])
def test_post_process_select_kernel_equals_sort_kernel(n):
    """The register-resident binary-search select: the smoothed rows, their two middle order statistics and the clamp of the
    reference (rows of many ties, a constant row, a burst of outliers)."""
    rng = np.random.default_rng(n)
    nf = 37 if n <= 4096 else 5
    db = (rng.standard_normal((nf, n)) * 6.0 - 35.0).astype(np.float32)
    db[0, : n // 2] = np.round(db[0, : n // 2])           # heavy ties around the median
    db[1] = -42.5                                          # a constant row
    if n >= 256:
        db[2, 100:140] += 50.0
    e = G.engine()
    d_db = G.dev(db)
    d_post = G.empty((nf, n - 4), torch.float32)
    d_post.fill_(float("nan"))
    e.spectrum_post(d_db, nf, n, d_post)
    e.sync()
    post = G.host(d_post)
    for f in (0, 1, nf - 1):
        sm = np.convolve(db[f].astype(np.float64), np.ones(5) / 5, mode="valid")
        thr = np.median(sm) - 10
        ref = np.where(sm < thr, thr, sm)
        assert np.all(np.abs(post[f] - ref) <= 1e-4 * np.maximum(np.abs(ref), 1.0)), (n, f)


def test_post_process_row_extremes():
    rng = np.random.default_rng(77)
    e = G.engine()
    for n in (1024, 2048, 4096, 16384, 1002):
        nf = 50
        db = (rng.standard_normal((nf, n)) * 5.0 - 60.0).astype(np.float32)
        db[3, 10:20] = np.inf                              # non-finite values are not extremes (np.isfinite mask)
        d_post, d_lo, d_hi = G.empty((nf, n - 4), torch.float32), G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
        e.spectrum_post_extremes(G.dev(db), nf, n, d_post, d_lo, d_hi)
        e.sync()
        post, lo, hi = G.host(d_post), G.host(d_lo), G.host(d_hi)
        for f in range(nf):
            fin = post[f][np.isfinite(post[f])]
            assert lo[f] == fin.min() and hi[f] == fin.max(), (n, f)
        d_lo2, d_hi2 = G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
        e.row_extremes(d_post, nf, n - 4, d_lo2, d_hi2)
        e.sync()
        assert np.array_equal(G.host(d_lo2), lo) and np.array_equal(G.host(d_hi2), hi)


def test_batched_accumulators_vs_reference_histories(golden):
    """pss_waterfall_rows / pss_persistence_rows: one display line per frame for a whole batch, against the grids the
    reference drew frame by frame (tests/golden/caller.npz: draw_waterfall / draw_persistence with a fake stdscr)."""
    g = golden["caller"]
    e = G.engine()
    rows = np.ascontiguousarray(g["rows"])                 # float64 [34][1020], the caller's post-processed rows
    nf, ln = rows.shape
    H, W = [int(v) for v in g["hw"]]
    dh, dw = H - 4, W - 8
    d_rows = G.dev(rows)
    d_lo, d_hi = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
    e.row_extremes(d_rows, nf, ln, d_lo, d_hi, f64=True)
    d_g, d_c = G.empty((nf, dw), torch.int8), G.empty((nf, dw), torch.int8)
    e.waterfall_rows(d_rows, nf, ln, d_lo, d_hi, dw, d_g, d_c, window=30, f64=True)
    e.sync()
    gl, co = G.host(d_g), G.host(d_c)
    for i in range(nf):                                    # line y = 0 of the reference's grid at frame i is the newest row
        assert np.array_equal(gl[i], g["wf_glyph"][i][0]) and np.array_equal(co[i], g["wf_colour"][i][0]), i
    # persistence: the newest trace's '*' row per column; the reference grid holds that trace's colour there
    nps = g["ps_colour"].shape[0]
    d_y = G.empty((nps, dw), torch.int8)
    e.persistence_rows(d_rows, nps, ln, d_lo, d_hi, dh, dw, d_y, window=10, f64=True)
    e.sync()
    ys = G.host(d_y)
    for i in range(nps):
        n_hist = min(i + 1, 10)
        cp_new = int(1 + 5 * (1 - 0.7 ** (10 - (n_hist - 1))))
        win = rows[max(0, i + 1 - 10):i + 1]
        lo, hi = win.min(), win.max()
        rs = np.interp(np.linspace(0, ln - 1, dw), np.arange(ln), rows[i])
        want = ((1 - (rs - lo) / ((hi - lo) or 1.0)) * (dh - 1)).astype(int)
        assert np.array_equal(ys[i], want), i
        assert np.all(g["ps_colour"][i][ys[i], np.arange(dw)] == cp_new), i
    # a history that continues across a block boundary: extremes of the preceding rows as a halo
    cut = 13
    d_g2, d_c2 = G.empty((nf - cut, dw), torch.int8), G.empty((nf - cut, dw), torch.int8)
    e.waterfall_rows(d_rows[cut:], nf - cut, ln, d_lo, d_hi, dw, d_g2, d_c2, n_halo=cut, window=30, f64=True)
    e.sync()
    assert np.array_equal(G.host(d_g2), gl[cut:]) and np.array_equal(G.host(d_c2), co[cut:])
    # float32 rows (what the GPU pipeline produces itself): cells differ only where a value sits on a quantisation edge
    r32 = G.dev(rows.astype(np.float32))
    l32, h32 = G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
    e.row_extremes(r32, nf, ln, l32, h32)
    e.waterfall_rows(r32, nf, ln, l32, h32, dw, d_g, d_c, window=30)
    e.sync()
    assert np.mean(G.host(d_g) != gl) < 2e-3 and np.mean(G.host(d_c) != co) < 2e-3


def test_float64_rows_pipeline_draws_the_reference_cells(golden):
    """pss_frame_pipeline_nfm_f64: float64 dB rows, float64 post-processed rows, and the waterfall lines the REFERENCE drew from the same
    read buffers (tests/golden/caller_iq.npz -> caller.npz, draw_waterfall through a fake screen) — every cell, from IQ.  The float32
    pipeline on the same buffers may differ in a cell where a value sits on a quantisation edge."""
    g, q = golden["caller"], golden["caller_iq"]
    iq = np.ascontiguousarray(q["iq"])
    nf, n = iq.shape
    H, W = [int(v) for v in g["hw"]]
    dw, fs = W - 8, 2.4e6
    e = G.engine()
    q_out = e.demod_out_len(0, n, fs)
    d_iq = G.dev(iq)
    d_db, d_post = G.empty((nf, n), torch.float64), G.empty((nf, n - 4), torch.float64)
    d_lo, d_hi = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
    d_g, d_c = G.empty((nf, dw), torch.int8), G.empty((nf, dw), torch.int8)
    d_pcm = G.empty((nf, q_out, 2), torch.int16)
    e.frame_pipeline_nfm_f64(d_iq, nf, n, fs, d_db, d_post, d_lo, d_hi, dw, d_g, d_c, d_pcm)
    e.sync()
    db, post = G.host(d_db), G.host(d_post)
    assert np.allclose(db, q["db"], rtol=1e-9, atol=1e-9)                    # compute_fft's float64 rows
    assert np.allclose(post, g["rows"], rtol=1e-9, atol=1e-9)                # the caller's post-processed rows ...
    assert np.array_equal(post, np.stack([O.postprocess(r) for r in db]))    # ... and bit for bit np.convolve / np.median / the clamp on the dB rows
    assert np.array_equal(G.host(d_lo), post.min(axis=1)) and np.array_equal(G.host(d_hi), post.max(axis=1))
    gl, co = G.host(d_g), G.host(d_c)
    for i in range(nf):                                                      # line y = 0 of the reference's grid at frame i is the newest row
        assert np.array_equal(gl[i], g["wf_glyph"][i][0]) and np.array_equal(co[i], g["wf_colour"][i][0]), i
    # the PCM is the float32 pipeline's (same demodulator)
    d_db32, d_lo32, d_hi32 = G.empty((nf, n), torch.float32), G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
    d_g2, d_c2, d_pcm2 = G.empty((nf, dw), torch.int8), G.empty((nf, dw), torch.int8), G.empty((nf, q_out, 2), torch.int16)
    e.frame_pipeline_nfm(d_iq, nf, n, fs, d_db32, None, d_lo32, d_hi32, dw, d_g2, d_c2, d_pcm2)
    e.sync()
    assert np.array_equal(G.host(d_pcm), G.host(d_pcm2))
    assert np.allclose(G.host(d_db32), db, rtol=1e-4, atol=1e-4)
    assert np.mean(G.host(d_g2) != gl) < 2e-3 and np.mean(G.host(d_c2) != co) < 2e-3
    # the two halves separately, other lengths, a row with a NaN (np.median -> NaN: nothing is clamped)
    rng = np.random.default_rng(5)
    for n2 in (16, 64, 4096, 16384):
        x = (rng.standard_normal((3, n2)) + 1j * rng.standard_normal((3, n2))).astype(np.complex64)
        d_b, d_p = G.empty((3, n2), torch.float64), G.empty((3, n2 - 4), torch.float64)
        e.spectrum_db_f64(G.dev(x), 3, n2, d_b)
        e.spectrum_post_f64(d_b, 3, n2, d_p)
        e.sync()
        want = np.stack([O.compute_fft(f) for f in x])
        assert np.allclose(G.host(d_b), want, rtol=1e-9, atol=1e-9), n2
        assert np.array_equal(G.host(d_p), np.stack([O.postprocess(r) for r in G.host(d_b)])), n2
    rows = rng.standard_normal((2, 1024)) * 10 - 40
    rows[1, 500] = np.nan
    d_p = G.empty((2, 1020), torch.float64)
    e.spectrum_post_f64(G.dev(rows), 2, 1024, d_p)
    e.sync()
    sm = np.stack([np.convolve(r, np.ones(5) / 5, mode="valid") for r in rows])
    assert np.array_equal(G.host(d_p)[0], O.postprocess(rows[0]))
    assert np.array_equal(G.host(d_p)[1], sm[1], equal_nan=True)


@pytest.mark.parametrize("mode", [L.MODE_AM, L.MODE_NFM, L.MODE_USB])
def test_demod_power_equals_the_two_calls(mode):
    """pss_demod_power: measure_signal_power + demodulate of the same frames (pyspecsdr.py:2251, :2262); for AM both float32 means come out
    of one pass over the IQ (two pairwise trees walked together) — the power bits and the PCM / audio must be those of the separate calls."""
    e = G.engine()
    gen = torch.Generator(device="cuda").manual_seed(31 + mode)
    for nf, n in ((700, 1024), (5, 7), (40, 5000), (9, 16384), (3, 40001), (2, 262144)):
        if mode != L.MODE_AM and n < 64:
            continue
        fs = 2.4e6
        iq = torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3 + 0.1
        torch.cuda.synchronize()
        n_out = e.demod_out_len(mode, n, fs)
        pa, pb = G.empty((nf, n_out, 2), torch.int16), G.empty((nf, n_out, 2), torch.int16)
        aa, ab = G.empty((nf, n_out), torch.float64), G.empty((nf, n_out), torch.float64)
        wa, wb = G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
        e.demod_power(mode, iq, nf, n, fs, pa, aa, wa)
        e.power_db(iq, nf, n, wb)
        e.demod(mode, iq, nf, n, fs, pb, ab)
        e.sync()
        assert torch.equal(wa.view(torch.int32), wb.view(torch.int32)), (mode, nf, n)
        assert torch.equal(pa, pb) and torch.equal(aa.view(torch.int64), ab.view(torch.int64)), (mode, nf, n)
    for k in range(3):   # power bits against the oracle (NumPy's float32 pairwise mean + SVML log10)
        x = iq[k % nf].cpu().numpy().view(np.complex64).reshape(-1)
        assert wa[k % nf].cpu().numpy().tobytes() == np.float32(O.power_db(x)).tobytes()


def test_wfm_correction_in_the_forward_kernel_equals_the_corrected_copy():
    """demodulate_signal(WFM) = iq_correction + demodulate_wfm (signal_processing.py:222-228).  Large batches: a pre-pass leaves the five
    correction scalars per frame and the fused forward kernel corrects every sample as it loads it — against the path that writes the
    corrected copy of the batch first (option "wfm_corr_copy"), and against iq_correction + demod as separate calls: the same PCM and audio bits."""
    e = G.engine()
    gen = torch.Generator(device="cuda").manual_seed(8)
    for nf, n, fs in ((7000, 1024, 2.4e6), (6100, 2048, 1.024e6), (3, 4096, 2.4e6)):
        iq = torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3 + torch.tensor([0.05, -0.02], device="cuda")
        iq[..., 1] *= 0.8                                     # an amplitude imbalance for the correction to act on
        torch.cuda.synchronize()
        n_out = e.demod_out_len(L.MODE_WFM, n, fs)
        outs = []
        for copy in (0, 1):
            e.set_option("wfm_corr_copy", copy)
            pcm, au = G.empty((nf, n_out, 2), torch.int16), G.empty((nf, n_out, 2), torch.float64)
            e.demod_signal(L.MODE_WFM, iq, nf, n, fs, pcm, au)
            e.sync()
            outs.append((pcm, au))
        e.set_option("wfm_corr_copy", 0)
        corr = G.empty((nf, n, 2), torch.float32)
        pcm, au = G.empty((nf, n_out, 2), torch.int16), G.empty((nf, n_out, 2), torch.float64)
        e.iq_correction(iq, nf, n, corr, None)
        e.demod(L.MODE_WFM, corr, nf, n, fs, pcm, au)
        e.sync()
        for p2, a2 in outs:
            assert torch.equal(p2, pcm) and torch.equal(a2.view(torch.int64), au.view(torch.int64)), (nf, n)


def test_float64_pipeline_register_kernels_equal_plain_kernels_and_numpy():
    """The float64-row entry points on the register kernels (k_spectrum_r16<..., D64>, k_post_sel<..., double>, the lines from the rows
    resampled in the same pass) against the plain round-3 kernels (option "f64_plain") and NumPy: dB rows within 1e-11 of each other
    (np.log10 against the table evaluation), the post-process bit for bit np.convolve / np.median / the clamp of the SAME dB rows at
    every length the register select serves, rows with a NaN / infinities, materialised and not materialised rows giving the same lines."""
    e = G.engine()
    rng = np.random.default_rng(11)
    for n in (256, 512, 1024, 2048, 4096):
        x = ((rng.standard_normal((37, n)) + 1j * rng.standard_normal((37, n))) * 0.2).astype(np.complex64)
        d_a, d_b = G.empty((37, n), torch.float64), G.empty((37, n), torch.float64)
        e.spectrum_db_f64(G.dev(x), 37, n, d_a)
        e.set_option("f64_plain", 1)
        e.spectrum_db_f64(G.dev(x), 37, n, d_b)
        e.set_option("f64_plain", 0)
        e.sync()
        want = np.stack([O.compute_fft(f) for f in x])
        assert np.allclose(G.host(d_a), want, rtol=1e-11, atol=1e-11), n
        assert np.allclose(G.host(d_a), G.host(d_b), rtol=1e-11, atol=1e-11), n
    for n in (8, 12, 64, 260, 516, 1000, 1024, 1028, 2048, 3000, 4096, 5000, 8192, 16384, 16388):
        nf = 9
        rows = rng.standard_normal((nf, n)) * 6.0 - 50.0
        rows[1] = np.round(rows[1])                         # many equal values: ties at the median
        rows[2, :] = -47.25                                 # a constant row
        rows[7] = -50.0 + rng.standard_normal(n) * 1e-7     # values that differ in the LOW word of their keys only (the two-level select's second search)
        rows[8, : n // 2] = np.round(rows[8, : n // 2] * 4e4) / 4e4 + rng.integers(0, 3, n // 2) * 1e-12   # many small groups sharing a high word
        if n >= 64:
            rows[3, 5:9] = np.inf
            rows[4, 7] = -np.inf
            rows[5, n // 2] = np.nan                        # np.median -> NaN: nothing is clamped
            rows[6, 3] = np.inf; rows[6, 30] = -np.inf      # inf - inf inside a window never meets here; both kinds of infinity in one row
        d_rows = G.dev(rows)
        outs = []
        for plain in (0, 1):
            e.set_option("f64_plain", plain)
            d_p, d_lo, d_hi = G.empty((nf, n - 4), torch.float64), G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
            e.spectrum_post_f64(d_rows, nf, n, d_p, d_lo, d_hi)
            e.sync()
            outs.append((G.host(d_p), G.host(d_lo), G.host(d_hi)))
        e.set_option("f64_plain", 0)
        m = n - 4
        for k in range(nf):
            sm = rows[k, 0:m] * 0.2
            for j in range(1, 5):
                sm = sm + rows[k, j:j + m] * 0.2
            with np.errstate(invalid="ignore"):
                med = np.median(sm)
                want = sm.copy()
                want[want < med - 10] = med - 10
            assert np.array_equal(outs[0][0][k], want, equal_nan=True), (n, k)
            fin = want[np.isfinite(want)]
            if fin.size:
                assert outs[0][1][k] == fin.min() and outs[0][2][k] == fin.max(), (n, k)
            else:
                assert outs[0][1][k] == np.inf and outs[0][2][k] == -np.inf, (n, k)
        assert np.array_equal(outs[0][0], outs[1][0], equal_nan=True), n
        assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2]), n
    # the pipeline: rows not materialised (one pass leaves extremes + the rows resampled to the display width) == rows materialised
    gen = torch.Generator(device="cuda").manual_seed(99)
    for nf, n, fs, W in ((3000, 1024, 2.4e6, 112), (100, 4096, 2.4e6, 200), (64, 256, 2.4e6, 300), (20, 8192, 2.4e6, 112)):
        iq = torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3
        n_out = e.demod_out_len(0, n, fs)
        def bufs():
            return dict(db=G.empty((nf, n), torch.float64), lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64),
                        g=G.empty((nf, W), torch.int8), c=G.empty((nf, W), torch.int8), pcm=G.empty((nf, n_out, 2), torch.int16))
        a, b = bufs(), bufs()
        d_post = G.empty((nf, n - 4), torch.float64)
        torch.cuda.synchronize()
        e.frame_pipeline_nfm_f64(iq, nf, n, fs, a["db"], d_post, a["lo"], a["hi"], W, a["g"], a["c"], a["pcm"])
        e.frame_pipeline_nfm_f64(iq, nf, n, fs, b["db"], None, b["lo"], b["hi"], W, b["g"], b["c"], b["pcm"])
        e.sync()
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (nf, n, k)
        # and the float32 pipeline's lines without materialised rows == with them (the resampled-row path against k_disp_rows)
        def bufs32():
            return dict(db=G.empty((nf, n), torch.float32), lo=G.empty((nf,), torch.float32), hi=G.empty((nf,), torch.float32),
                        g=G.empty((nf, W), torch.int8), c=G.empty((nf, W), torch.int8), pcm=G.empty((nf, n_out, 2), torch.int16))
        a, b = bufs32(), bufs32()
        d_post32 = G.empty((nf, n - 4), torch.float32)
        e.frame_pipeline_nfm(iq, nf, n, fs, a["db"], d_post32, a["lo"], a["hi"], W, a["g"], a["c"], a["pcm"])
        e.frame_pipeline_nfm(iq, nf, n, fs, b["db"], None, b["lo"], b["hi"], W, b["g"], b["c"], b["pcm"])
        e.sync()
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (nf, n, k, "float32 rows")


def _select_branch_rows(n, rng):
    """dB rows that drive the compaction select of one-wavefront rows (pss_post.h select_kth64_compact / select_kth32_compact) through each of
    its branches; the second value classifies them with a host emulation of the bracket logic (counts on the keys' high words)."""
    fam = [-50.0 + 0.25 * rng.standard_normal((6, n)),                      # everything inside the first bracket: more candidates than the cap
           -50.0 - 3.0 * np.log(rng.random((6, n)))]                        # skewed: the median ~0.9 dB below the mean (second bracket)
    for _ in range(3):                                                      # long runs on a 0.6 dB grid: ties among the candidates
        rows = np.empty((16, n))
        for k in range(16):
            pos = 0
            while pos < n:
                ln = int(rng.integers(5, 40))
                rows[k, pos:pos + ln] = -50.0 + 0.6 * rng.integers(-3, 4)
                pos += ln
        fam.append(rows)
    rows = np.empty((6, n))                                                 # two far-apart modes in long runs: the median outside both brackets
    for k in range(6):
        pos = 0
        while pos < n:
            ln = min(int(rng.integers(20, 60)), n - pos)
            rows[k, pos:pos + ln] = (-40.0 + rng.standard_normal(ln)) if rng.random() < 0.55 else (-75.0 + 0.1 * rng.standard_normal(ln))
            pos += ln
    fam.append(rows)
    r = -45.0 + 5.6 * rng.standard_normal((6, n))                           # a third of the row inside one high word around the median
    idx = rng.permutation(n)[: n // 3]
    r[:, idx] = -45.0 + 1e-9 * rng.standard_normal((6, idx.size))
    fam.append(r)
    fam.append(-45.0 + 5.6 * rng.standard_normal((300, n)))                 # noise rows: rank k is the last key of its bracket in ~1 % of them
    return np.concatenate(fam)


def _select_branch_classes(rows, cap=128):
    def d2ord(v):
        u = np.asarray(v, dtype=np.float64).view(np.uint64)
        return np.where((u >> np.uint64(63)).astype(bool), ~u, u | np.uint64(1 << 63))
    out = []
    for row in rows:
        m = row.size - 4
        sm = row[0:m] * 0.2
        for j in range(1, 5):
            sm = sm + row[j:j + m] * 0.2
        g = np.float32(sm.astype(np.float32).sum(dtype=np.float32) / np.float32(m))
        k = (m - 1) >> 1
        kh = (d2ord(sm) >> np.uint64(32)).astype(np.int64)
        srt = np.sort(sm)
        cls = "general"
        for d in (np.float32(0.5), np.float32(2.0)):
            lo, hi = (int(d2ord(np.float64(np.float32(x))) >> np.uint64(32)) for x in (g - d, g + d))
            nlo, M = int((kh < lo).sum()), int(((kh >= lo) & (kh <= hi)).sum())
            if not (nlo <= k < nlo + M):
                continue
            cls, nhi = ("first" if d < 1 else "second"), nlo + M
            if M > cap:
                cls += ":narrowed"
                while nhi - nlo > cap and lo < hi:
                    t = lo + ((hi - lo + 1) >> 1)
                    c = int((kh < t).sum())
                    if c <= k:
                        lo, nlo = t, c
                    else:
                        hi, nhi = t - 1, c
                if nhi - nlo > cap:
                    cls += ":fallback"
                    break
            cls += ":tie" if srt[k] == srt[k + 1] else ":last" if k + 1 == nhi else ""
            break
        out.append(cls)
    return out


def test_compaction_select_branches_equal_numpy():
    """The order statistics of rows owned by one wavefront (round 6: candidates of the bracket compacted through LDS, the search continued on whole
    keys with ballot counts): rows built to take every branch — more candidates than the cap (sweeps + second compaction), the second bracket,
    neither bracket (the general search), ties among the candidates, rank k + 1 equal to rank k, rank k the LAST key of its bracket (rank k + 1
    then comes from a sweep over all elements), too many keys sharing a high word (falls back) — against np.convolve / np.median / the clamp
    bit for bit, float64 rows and float32 rows (the float32 rounding of the float64 sums), row extremes included."""
    e = G.engine()
    import collections
    for n in (260, 516, 1024, 1028, 2048):
        rng = np.random.default_rng(5 + n)
        rows = _select_branch_rows(n, rng)
        nf, m = rows.shape[0], n - 4
        seen = collections.Counter(c2 for c in _select_branch_classes(rows) for c2 in c.split(":"))
        for need in ("first", "general", "narrowed", "tie") + (("fallback", "last") if n >= 1024 else ()) + (("second",) if n <= 1028 else ()):
            assert seen[need] > 0, (n, need, dict(seen))          # (the host classification of THESE seeded rows; no GPU involved)
        sm = rows[:, 0:m] * 0.2
        for j in range(1, 5):
            sm = sm + rows[:, j:j + m] * 0.2
        # float64 rows
        d_p, d_lo, d_hi = G.empty((nf, m), torch.float64), G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
        e.spectrum_post_f64(G.dev(rows), nf, n, d_p, d_lo, d_hi)
        e.sync()
        med = np.median(sm, axis=1)
        want = np.maximum(sm, (med - 10)[:, None])
        assert np.array_equal(G.host(d_p), want), n
        assert np.array_equal(G.host(d_lo), want.min(axis=1)) and np.array_equal(G.host(d_hi), want.max(axis=1)), n
        # float32 rows: the smoothed row is the float32 rounding of the float64 sums; the median of THOSE values; the threshold rounded to float32
        rows32 = rows.astype(np.float32)
        s32 = rows32[:, 0:m].astype(np.float64) * 0.2
        for j in range(1, 5):
            s32 = s32 + rows32[:, j:j + m].astype(np.float64) * 0.2
        s32 = s32.astype(np.float32)
        srt = np.sort(s32, axis=1)
        k = (m - 1) >> 1
        med32 = srt[:, k].astype(np.float64) if m & 1 else 0.5 * (srt[:, k].astype(np.float64) + srt[:, k + 1].astype(np.float64))
        want32 = np.maximum(s32, (med32 - 10.0).astype(np.float32)[:, None])
        d_p, d_lo, d_hi = G.empty((nf, m), torch.float32), G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
        e.spectrum_post_extremes(G.dev(rows32), nf, n, d_p, d_lo, d_hi)
        e.sync()
        assert np.array_equal(G.host(d_p), want32), n
        assert np.array_equal(G.host(d_lo), want32.min(axis=1)) and np.array_equal(G.host(d_hi), want32.max(axis=1)), n


def test_full_size_float64_pipeline_cells_equal_the_oracle_from_iq():
    """BASELINE.json cfg 2 size (65 536 x 1024) through pss_frame_pipeline_nfm_f64 without materialised rows — the cell-exact step bench.py
    times: EVERY waterfall cell (glyph and colour, 2 x 7.3 million) and every int16 PCM sample against the oracle's own step from IQ in the
    reference's row type (float64 compute_fft rows -> np.convolve / np.median / clamp -> draw_waterfall's min / max over the last 30 rows,
    np.interp, quantisation), and the row extremes to 1e-11."""
    e = G.engine()
    nf, n, fs, W, win = 65536, 1024, 2.4e6, 112, 30
    import bench
    iq = bench.synth_fm_iq(nf, n, fs, torch.device("cuda", 0), seed=777)
    torch.cuda.synchronize()
    d_db = G.empty((nf, n), torch.float64)
    d_lo, d_hi = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
    d_g, d_c = G.empty((nf, W), torch.int8), G.empty((nf, W), torch.int8)
    d_pcm = G.empty((nf, 10, 2), torch.int16)
    e.frame_pipeline_nfm_f64(iq, nf, n, fs, d_db, None, d_lo, d_hi, W, d_g, d_c, d_pcm, window=win)
    e.sync()
    taps, sos, zi = e.nfm_filters(fs)
    import os
    o = O.headline_f64(iq.cpu().numpy().view(np.complex64).reshape(nf, n), fs, taps, sos, zi, win, W, len(os.sched_getaffinity(0)))
    assert np.array_equal(G.host(d_pcm), o["pcm"])
    assert np.allclose(G.host(d_lo), o["lo"], rtol=0, atol=1e-10) and np.allclose(G.host(d_hi), o["hi"], rtol=0, atol=1e-10)
    g, c = G.host(d_g), G.host(d_c)
    bad = int(np.count_nonzero(g != o["glyph"])) + int(np.count_nonzero(c != o["colour"]))
    assert bad == 0, f"{bad} of {2 * g.size} cells differ from the oracle's cells computed from IQ"
    # the step bench.py times since round 6 — pss_frame_pipeline_cells: the same arithmetic, the dB row written as float32 — leaves the same bytes
    d_db32 = G.empty((nf, n), torch.float32)
    d_lo2, d_hi2 = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
    d_g2, d_c2, d_pcm2 = G.empty((nf, W), torch.int8), G.empty((nf, W), torch.int8), G.empty((nf, 10, 2), torch.int16)
    e.frame_pipeline_cells(L.MODE_NFM, iq, nf, n, fs, d_db32, None, d_lo2, d_hi2, W, d_g2, d_c2, d_pcm2, window=win)
    e.sync()
    assert torch.equal(d_g2, d_g) and torch.equal(d_c2, d_c) and torch.equal(d_pcm2, d_pcm)
    assert torch.equal(d_lo2.view(torch.int64), d_lo.view(torch.int64)) and torch.equal(d_hi2.view(torch.int64), d_hi.view(torch.int64))
    assert torch.equal(d_db32.view(torch.int32), d_db.float().view(torch.int32))


def test_fused_transform_post_kernel_equals_the_two_kernels():
    """k_spectrum_post (pss_spec_post.h: compute_fft and the caller's post-process of a 1024-point frame in ONE kernel, the float64 dB values
    handed from the transform's registers through LDS to the select) against the two kernels it replaces (option "fuse_post" = 0:
    k_spectrum_r16<D64> -> k_post_sel<double>): dB rows, row extremes and display lines bit for bit, on batches that end inside a workgroup,
    frames of zeros (a constant row), with a NaN / an infinity among the samples, a pure tone, and amplitudes so small that the rows differ in
    the low words of their values only; every entry point that reaches the kernel (pss_frame_pipeline_f64 in every mode, both displays, with a
    halo; pss_frame_pipeline_cells, whose float32 row must be the float64 row rounded once; pss_spectrum_cells), and the lengths the fused
    kernel does not serve through pss_frame_pipeline_cells' conversion pass."""
    e = G.engine()
    fs, W, H = 2.4e6, 112, 36
    gen = torch.Generator(device="cuda").manual_seed(606)
    try:
        for nf in (1, 3, 4, 5, 1027, 3001):
            n = 1024
            iq = torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3
            if nf >= 5:
                iq[1] = 0.0                                           # every bin -100 dB exactly: a constant row
                iq[2] *= 1e-19                                        # |X|^2 far below the 1e-10 floor: values that differ in their low words only
                t = torch.arange(n, device="cuda", dtype=torch.float64)
                iq[3, :, 0] = torch.cos(2 * np.pi * 100.25 * t / n).float(); iq[3, :, 1] = torch.sin(2 * np.pi * 100.25 * t / n).float()
                iq[4, 17, 0] = float("nan")                           # every bin NaN: np.median -> NaN, nothing clamped, no finite extreme
            if nf >= 1027:
                iq[1000, 5, 1] = float("inf")                         # inf * window -> inf / NaN bins
                iq[nf - 1] *= 30.0
            torch.cuda.synchronize()
            for mode in ((L.MODE_NFM, L.MODE_AM, L.MODE_USB, L.MODE_WFM) if nf == 1027 else (L.MODE_NFM,)):
                for display in ("waterfall", "persistence"):
                    n_out = e.demod_out_len(mode, n, fs)
                    outs = []
                    for fuse in (0, 1):
                        e.set_option("fuse_post", fuse)
                        o = dict(db=G.empty((nf, n), torch.float64), lo=torch.zeros((7 + nf,), dtype=torch.float64, device="cuda") - 55.0,
                                 hi=torch.zeros((7 + nf,), dtype=torch.float64, device="cuda") - 20.0,
                                 a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"),
                                 pcm=G.empty((nf, n_out, 2), torch.int16))
                        e.frame_pipeline_f64(mode, iq, nf, n, fs, o["db"], None, o["lo"], o["hi"], W, o["a"], o["b"], o["pcm"], n_halo=7, display=display,
                                             disp_h=H)
                        e.sync()
                        outs.append(o)
                    for k in outs[0]:
                        assert torch.equal(outs[0][k].view(torch.uint8), outs[1][k].view(torch.uint8)), (nf, mode, display, k)
                    # the cells entry: the same lines / extremes / PCM, the float32 row = the float64 row rounded once; with and without the float64 row
                    e.set_option("fuse_post", 1)
                    for want64 in (False, True):
                        c = dict(db32=G.empty((nf, n), torch.float32), db64=G.empty((nf, n), torch.float64) if want64 else None,
                                 lo=torch.zeros((7 + nf,), dtype=torch.float64, device="cuda") - 55.0, hi=torch.zeros((7 + nf,), dtype=torch.float64, device="cuda") - 20.0,
                                 a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"),
                                 pcm=G.empty((nf, n_out, 2), torch.int16))
                        e.frame_pipeline_cells(mode, iq, nf, n, fs, c["db32"], c["db64"], c["lo"], c["hi"], W, c["a"], c["b"], c["pcm"], n_halo=7,
                                               display=display, disp_h=H)
                        e.sync()
                        for k in ("lo", "hi", "a", "b", "pcm"):
                            assert torch.equal(outs[0][k].view(torch.uint8), c[k].view(torch.uint8)), (nf, mode, display, k, "cells")
                        assert torch.equal(c["db32"].view(torch.int32), outs[0]["db"].float().view(torch.int32)), (nf, mode, "db32")
                        if want64:
                            assert torch.equal(c["db64"].view(torch.int64), outs[0]["db"].view(torch.int64)), (nf, mode, "db64")
            # the display half alone
            s = dict(db32=G.empty((nf, n), torch.float32), lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64),
                     a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"))
            r = dict(db=G.empty((nf, n), torch.float64), lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64),
                     a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"),
                     pcm=G.empty((nf, e.demod_out_len(L.MODE_NFM, n, fs), 2), torch.int16))
            e.spectrum_cells(iq, nf, n, s["db32"], None, s["lo"], s["hi"], W, s["a"], s["b"])
            e.set_option("fuse_post", 0)
            e.frame_pipeline_f64(L.MODE_NFM, iq, nf, n, fs, r["db"], None, r["lo"], r["hi"], W, r["a"], r["b"], r["pcm"])
            e.sync()
            for k in ("lo", "hi", "a", "b"):
                assert torch.equal(s[k].view(torch.uint8), r[k].view(torch.uint8)), (nf, k, "spectrum_cells")
            assert torch.equal(s["db32"].view(torch.int32), r["db"].float().view(torch.int32))
        # display widths around the wavefront size and beyond the row length, an empty batch
        nf, n = 257, 1024
        iq = torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3
        torch.cuda.synchronize()
        for Wd in (1, 2, 63, 64, 65, 300, 1020, 1500):
            outs = []
            for fuse in (0, 1):
                e.set_option("fuse_post", fuse)
                o = dict(db=G.empty((nf, n), torch.float64), lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64),
                         a=torch.zeros((nf, Wd), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, Wd), dtype=torch.int8, device="cuda"))
                e.spectrum_cells(iq, nf, n, None, o["db"], o["lo"], o["hi"], Wd, o["a"], o["b"])
                e.sync()
                outs.append(o)
            for k in outs[0]:
                assert torch.equal(outs[0][k].view(torch.uint8), outs[1][k].view(torch.uint8)), (Wd, k)
        e.set_option("fuse_post", 1)
        e.spectrum_cells(iq, 0, n, None, None, None, None, 112, None, None)        # nothing to do, nothing dereferenced
        e.frame_pipeline_cells(L.MODE_NFM, iq, 0, n, fs, None, None, None, None, 112, None, None, None)
        e.sync()
        # other lengths through the cells entry (float64 rows in the context's scratch + the conversion pass)
        e.set_option("fuse_post", 1)
        for nf, n in ((300, 512), (100, 2048), (9, 8192)):
            iq = torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3
            torch.cuda.synchronize()
            n_out = e.demod_out_len(L.MODE_NFM, n, fs)
            r = dict(db=G.empty((nf, n), torch.float64), lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64),
                     a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), pcm=G.empty((nf, n_out, 2), torch.int16))
            c = dict(db32=G.empty((nf, n), torch.float32), lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64),
                     a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), pcm=G.empty((nf, n_out, 2), torch.int16))
            e.frame_pipeline_f64(L.MODE_NFM, iq, nf, n, fs, r["db"], None, r["lo"], r["hi"], W, r["a"], r["b"], r["pcm"])
            e.frame_pipeline_cells(L.MODE_NFM, iq, nf, n, fs, c["db32"], None, c["lo"], c["hi"], W, c["a"], c["b"], c["pcm"])
            e.sync()
            for k in ("lo", "hi", "a", "b", "pcm"):
                assert torch.equal(r[k].view(torch.uint8), c[k].view(torch.uint8)), (nf, n, k)
            assert torch.equal(c["db32"].view(torch.int32), r["db"].float().view(torch.int32)), (nf, n)
    finally:
        e.set_option("fuse_post", 1)


@pytest.mark.parametrize("display", ["waterfall", "persistence"])
def test_float64_pipeline_every_mode_and_display_cells_equal_the_oracle_from_iq(display):
    """pss_frame_pipeline_f64: the cell-exact step for both batched accumulators (draw_waterfall's line, draw_persistence's newest trace,
    pyspecsdr.py:1342-1406 / :1512-1564) and every demodulation mode — cells against the oracle's own step from the IQ (float64 rows), PCM
    against the float32-row call of the same mode (same demodulator); a capture cut in two blocks with the extremes halo gives the same lines."""
    e = G.engine()
    import bench
    nf, n, fs, W, H = 3000, 2048, 10e6, 112, 36
    win = 30 if display == "waterfall" else 10
    iq = bench.synth_fm_iq(nf, n, fs, torch.device("cuda", 0), seed=4242)
    torch.cuda.synchronize()
    taps, sos, zi = e.nfm_filters(fs)
    o = O.headline_f64(iq.cpu().numpy().view(np.complex64).reshape(nf, n), fs, taps, sos, zi, win, W, O.threads_available(), pcm=True,
                       display=display, disp_h=H)
    want = (o["glyph"], o["colour"]) if display == "waterfall" else (o["glyph"],)
    for mode in (L.MODE_NFM, L.MODE_AM, L.MODE_USB, L.MODE_WFM):
        n_out = e.demod_out_len(mode, n, fs)
        d_db = G.empty((nf, n), torch.float64)
        d_lo, d_hi = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
        d_a, d_b = G.empty((nf, W), torch.int8), torch.zeros((nf, W), dtype=torch.int8, device="cuda")
        d_pcm = G.empty((nf, n_out, 2), torch.int16)
        e.frame_pipeline_f64(mode, iq, nf, n, fs, d_db, None, d_lo, d_hi, W, d_a, d_b, d_pcm, display=display, disp_h=H)
        e.sync()
        got = (G.host(d_a), G.host(d_b)) if display == "waterfall" else (G.host(d_a),)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (mode, display, int(np.count_nonzero(g != w)))
        if mode == L.MODE_NFM:
            assert np.array_equal(G.host(d_pcm), o["pcm"])
        d_db32, d_lo32, d_hi32 = G.empty((nf, n), torch.float32), G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
        d_a2, d_b2, d_pcm2 = G.empty((nf, W), torch.int8), G.empty((nf, W), torch.int8), G.empty((nf, n_out, 2), torch.int16)
        e.frame_pipeline(mode, iq, nf, n, fs, d_db32, None, d_lo32, d_hi32, W, d_a2, d_b2, d_pcm2, display=display, disp_h=H)
        e.sync()
        assert torch.equal(d_pcm, d_pcm2), mode
    # two blocks, the second continuing the first's history through the halo of row extremes
    cut = 1777
    d_db = G.empty((nf, n), torch.float64)
    lo, hi = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
    a, b = G.empty((nf, W), torch.int8), torch.zeros((nf, W), dtype=torch.int8, device="cuda")
    pcm = G.empty((nf, e.demod_out_len(L.MODE_NFM, n, fs), 2), torch.int16)
    e.frame_pipeline_f64(L.MODE_NFM, iq[:cut], cut, n, fs, d_db[:cut], None, lo, hi, W, a[:cut], b[:cut], pcm[:cut], display=display, disp_h=H)
    e.frame_pipeline_f64(L.MODE_NFM, iq[cut:], nf - cut, n, fs, d_db[cut:], None, lo, hi, W, a[cut:], b[cut:], pcm[cut:], n_halo=cut,
                         display=display, disp_h=H)
    e.sync()
    got = (G.host(a), G.host(b)) if display == "waterfall" else (G.host(a),)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), display


@pytest.mark.parametrize("mode", ["waterfall", "persistence"])
def test_streamed_capture_float64_rows_draws_the_oracle_cells(mode):
    """pss_h_stream_display_nfm_f64 (BASELINE configs[4] with the reference's own row type): a host capture streamed in chunks — lines, PCM and
    row extremes against the oracle's own step from the IQ, the full screen after every chunk against the oracle's grid of the last `window`
    rows, and a capture cut in two with the float64 halo."""
    e = G.engine()
    import bench
    nf, n, fs, W, H = 1100, 2048, 10e6, 112, 36
    window = 30 if mode == "waterfall" else 10
    iq = bench.synth_fm_iq(nf, n, fs, torch.device("cuda", 0), seed=99).cpu().numpy().view(np.complex64).reshape(nf, n)
    taps, sos, zi = e.nfm_filters(fs)
    o = O.headline_f64(iq, fs, taps, sos, zi, window, W, O.threads_available(), display=mode, disp_h=H)
    want = (o["glyph"], o["colour"]) if mode == "waterfall" else (o["glyph"],)
    for chunk in (256, 1100, 97):
        got = e.stream_display_nfm_f64(iq, fs, chunk, mode=mode, disp_h=H, disp_w=W, grids=True, want_db=(chunk == 256))
        for g, w in zip(got["lines"], want):
            assert np.array_equal(g, w), (mode, chunk, int(np.count_nonzero(g != w)))
        assert np.array_equal(got["pcm"], o["pcm"])
        assert np.allclose(got["row_lo"], o["lo"], rtol=0, atol=1e-10) and np.allclose(got["row_hi"], o["hi"], rtol=0, atol=1e-10)
        n_chunks = (nf + chunk - 1) // chunk
        for k in range(n_chunks):
            last = min(nf, (k + 1) * chunk) - 1
            rows = o["post"][max(0, last + 1 - window):last + 1]
            if mode == "waterfall":
                wg, wc = O.waterfall_cells(rows, H, W)
                assert np.array_equal(got["grids"][0][k], wg) and np.array_equal(got["grids"][1][k], wc), (chunk, k)
            else:
                assert np.array_equal(got["grids"][0][k], O.persistence_cells(rows, H, W)), (chunk, k)
    cut = 613
    a = e.stream_display_nfm_f64(np.ascontiguousarray(iq[:cut]), fs, 200, mode=mode, disp_h=H, disp_w=W)
    b = e.stream_display_nfm_f64(np.ascontiguousarray(iq[cut:]), fs, 200, mode=mode, disp_h=H, disp_w=W,
                                 halo=(a["row_lo"][cut - (window - 1):], a["row_hi"][cut - (window - 1):]))
    for i, w in enumerate(want):
        assert np.array_equal(np.concatenate([a["lines"][i], b["lines"][i]]), w)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e", "f", "g"])
def test_nfm_vs_golden_bit_exact(golden, tag):
    g = golden["nfm"]
    fs = float(g[f"fs_{tag}"])
    e = G.engine()
    e.set_nfm_filters(fs, g[f"taps_{tag}"], g[f"sos_{tag}"], g[f"zi_{tag}"])  # SciPy's own coefficients
    for small_batch in (1, 0):   # systolic small-batch path (default for <= 8192 frames) and the fused large-batch kernels
        e.set_option("small_batch", small_batch)
        try:
            pcm, audio = G.demod(L.MODE_NFM, g[f"iq_{tag}"], fs)
        finally:
            e.set_option("small_batch", 1)
        assert np.array_equal(pcm, g[f"pcm_{tag}"])            # int16 bit-exact
        assert np.array_equal(audio, g[f"audio_{tag}"])        # float64 bit-exact


def test_nfm_designed_filters_pcm_exact(golden):
    # library-designed coefficients (a few ulp from SciPy's): int16 output still identical on the goldens
    g = golden["nfm"]
    from pyspecsdr_amd.engine import Engine
    e2 = Engine(0)
    for tag in ("a", "b", "c"):
        fs = float(g[f"fs_{tag}"])
        iq = g[f"iq_{tag}"]
        n_out = e2.demod_out_len(L.MODE_NFM, iq.shape[1], fs)
        d_pcm = G.empty((iq.shape[0], n_out, 2), torch.int16)
        e2.demod(L.MODE_NFM, G.dev(iq), iq.shape[0], iq.shape[1], fs, d_pcm, None)
        e2.sync()
        assert np.array_equal(G.host(d_pcm), g[f"pcm_{tag}"])
    e2.close()


def test_nfm_fused_and_three_kernel_paths_agree(golden):
    # the fused forward kernel and the front/edge/iir fallback must produce identical bits
    rng = np.random.default_rng(79)
    e = G.engine()
    for nf, n, fs in ((70, 1024, 2.4e6), (5, 2048, 10e6), (3, 300, 1.024e6), (2, 129, 2.4e6), (2, 4097, 2.4e6)):
        iq = (0.4 * np.exp(2j * np.pi * np.cumsum(rng.standard_normal((nf, n)) * 0.05, axis=1)) +
              0.05 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
        pcm0, a0 = G.demod(L.MODE_NFM, iq, fs)               # small-batch systolic decimator
        e.set_option("small_batch", 0)
        try:
            pcm1, a1 = G.demod(L.MODE_NFM, iq, fs)           # fused forward kernel + backward kernel
            e.set_option("nfm_fused", 0)
            pcm2, a2 = G.demod(L.MODE_NFM, iq, fs)           # front / edge / lane-per-frame IIR
        finally:
            e.set_option("nfm_fused", 1)
            e.set_option("small_batch", 1)
        assert np.array_equal(pcm1, pcm2) and np.array_equal(a1, a2), (nf, n, fs)
        assert np.array_equal(pcm0, pcm1) and np.array_equal(a0, a1), (nf, n, fs)
        taps, sos, zi = e.nfm_filters(fs)
        for k in range(min(nf, 3)):
            assert np.array_equal(a1[k], O.demod_nfm(iq[k], fs, taps, sos, zi)), (n, k)


def test_nfm_edges(golden):
    g = golden["nfm"]
    e = G.engine()
    with pytest.raises(ValueError):   # N-1 <= 27: scipy sosfiltfilt padlen ValueError
        G.demod(L.MODE_NFM, np.ones((1, 28), np.complex64), 2.4e6)
    with pytest.raises(ValueError):   # fs < 30 kHz: firwin cutoff >= Nyquist ValueError
        G.demod(L.MODE_NFM, np.ones((1, 1024), np.complex64), 25000.0)
    e.set_nfm_filters(2.4e6, g["taps_a"], g["sos_a"], g["zi_a"])
    pcm, audio = G.demod(L.MODE_NFM, np.zeros((2, 1024), np.complex64), 2.4e6)  # silence: 0/0 -> NaN -> int16 0
    assert np.isnan(audio).all() and np.array_equal(pcm[0], g["pcm_silence"])
    # ragged batch: 70 frames = one full tile + 6 (masked lanes), every frame must equal its single-frame result
    iq = np.tile(g["iq_a"], (12, 1))[:70]
    for small_batch in (1, 0):
        e.set_option("small_batch", small_batch)
        try:
            pcm, audio = G.demod(L.MODE_NFM, iq, 2.4e6)
        finally:
            e.set_option("small_batch", 1)
        for k in range(70):
            assert np.array_equal(pcm[k], g["pcm_a"][k % 6])
            assert np.array_equal(audio[k], g["audio_a"][k % 6])


def test_nfm_vs_oracle_random():
    # seeded noise-like IQ (worst case for the atan2 path: every octant, wide dynamic range)
    rng = np.random.default_rng(77)
    nf, n, fs = 130, 1024, 2.4e6
    iq = ((rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))) *
          np.exp2(rng.integers(-20, 4, (nf, 1)))).astype(np.complex64)
    e = G.engine()
    taps, sos, zi = e.nfm_filters(fs)
    pcm, audio = G.demod(L.MODE_NFM, iq, fs)
    for k in range(nf):
        a = O.demod_nfm(iq[k], fs, taps, sos, zi)
        assert np.array_equal(audio[k], a), k
        assert np.array_equal(pcm[k], O.pcm16_stereo(a)), k


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_am_vs_golden_bit_exact(golden, tag):
    g = golden["am_ssb"]
    pcm, audio = G.demod(L.MODE_AM, g[f"am_iq_{tag}"], 2.4e6)
    assert np.array_equal(pcm, g[f"am_pcm_{tag}"])
    assert np.array_equal(audio, g[f"am_audio_{tag}"])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
@pytest.mark.parametrize("mode", [L.MODE_USB, L.MODE_LSB])
def test_ssb_vs_golden(golden, tag, mode):
    g = golden["am_ssb"]
    fs = float(g[f"ssb_fs_{tag}"])
    e = G.engine()
    e.set_ssb_taps(fs, g[f"ssb_taps_{tag}"])
    taps = g[f"ssb_taps_{tag}"]
    res = {}
    for hil in (1, 0):     # 1 (default): the reference's hilbert() FFT round trip is executed; 0: skipped (identity on the real part)
        e.set_option("ssb_hilbert", hil)
        try:
            pcm, audio = G.demod(mode, g[f"ssb_iq_{tag}"], fs)
        finally:
            e.set_option("ssb_hilbert", 1)
        res[hil] = audio
        assert np.array_equal(pcm, g[f"ssb_pcm_{tag}"]), hil
        # float64: the reference's own round trip is pocketfft, ours the register transform — both leave ~1e-16 of rounding
        assert np.allclose(audio, g[f"ssb_audio_{tag}"], rtol=0, atol=2e-14), hil
    if True:
        # option "hilbert_exact": pocketfft's own butterfly order — the float64 audio of the reference, every bit
        e.set_option("hilbert_exact", 1)
        try:
            pcm, audio = G.demod(mode, g[f"ssb_iq_{tag}"], fs)
        finally:
            e.set_option("hilbert_exact", 0)
        assert np.array_equal(pcm, g[f"ssb_pcm_{tag}"])
        assert np.array_equal(audio, g[f"ssb_audio_{tag}"])
        for k, iq in enumerate(g[f"ssb_iq_{tag}"]):
            assert np.array_equal(audio[k], O.demod_ssb(iq, taps))
    for k, iq in enumerate(g[f"ssb_iq_{tag}"]):
        assert np.array_equal(res[0][k], O.demod_ssb(iq, taps, hilbert=False))   # without the round trip: the zdot-order FIR, bit-exact
    assert np.max(np.abs(res[1] - res[0])) < 1e-14


@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 1048576])
def test_hilbert_exact_is_scipy_bit_for_bit(n):
    """Option "hilbert_exact": pss_hilbert replays pocketfft (real radix-4 / 2 forward passes, complex radix-8 / 4 / 2 inverse passes,
    its twiddle products): the analytic signal equals scipy.signal.hilbert — through the oracle's restatement, which is pinned to SciPy
    bit for bit on the CPU side — on every bit; the default register transform stays within 2e-14."""
    rng = np.random.default_rng(n)
    rows = 5 if n < 16384 else (3 if n <= 131072 else 2)      # above 16 384 samples: the same passes through global memory
    x = rng.standard_normal((rows, n)) * 10.0 ** rng.integers(-2, 3, size=(rows, 1))
    x[0, ::7] = 0.0
    e = G.engine()
    d_x, d_out = G.dev(x), G.empty((rows, n), torch.complex128)
    e.set_option("hilbert_exact", 1)
    try:
        e.hilbert(d_x, rows, n, d_out)
        e.sync()
    finally:
        e.set_option("hilbert_exact", 0)
    got = G.host(d_out)
    want = np.stack([O.hilbert(r) for r in x])
    assert np.array_equal(got.view(np.float64).view(np.uint64), want.view(np.float64).view(np.uint64))
    e.hilbert(d_x, rows, n, d_out)
    e.sync()
    assert np.max(np.abs(G.host(d_out) - want)) < 2e-14 * np.max(np.abs(x))


def test_ssb_on_the_reference_read_buffer_sizes():
    """demodulate_ssb on the main loop's read buffers ((2 ** SAMPLES) * 256 samples, pyspecsdr.py:2236; 32768 by default): the
    Hilbert round trip runs through a spectrum in HBM there.  int16 equal with and without it, float64 within the transforms'
    rounding, and the path without it bit-exact against the oracle."""
    rng = np.random.default_rng(85)
    e = G.engine()
    fs = 2.4e6
    for n in (32768, 65536, 262144):
        t = np.arange(n) / fs
        iq = (0.4 * np.exp(2j * np.pi * 1.5e3 * t)[None, :] * (1 + 0.3 * np.sin(2 * np.pi * 300 * t))[None, :] +
              0.05 * (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n)))).astype(np.complex64)
        res = {}
        for hil in (1, 0):
            e.set_option("ssb_hilbert", hil)
            try:
                res[hil] = G.demod(L.MODE_USB, iq, fs)
            finally:
                e.set_option("ssb_hilbert", 1)
        assert np.array_equal(res[1][0], res[0][0]), n
        assert np.max(np.abs(res[1][1] - res[0][1])) < 1e-13, n
        taps = e.ssb_taps(fs)
        assert np.array_equal(res[0][1][0], O.demod_ssb(iq[0], taps, hilbert=False)), n
        if n <= 65536:
            e.set_option("hilbert_exact", 1)     # the reference's float64 audio at its own read-buffer sizes, every bit
            try:
                pcm_x, au_x = G.demod(L.MODE_USB, iq, fs)
            finally:
                e.set_option("hilbert_exact", 0)
            assert np.array_equal(pcm_x, res[1][0]), n
            for k in range(len(iq)):
                assert np.array_equal(au_x[k], O.demod_ssb(iq[k], taps)), (n, k)


_COLD = r"""
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np, torch
import gpu_util as G
e = G.engine()
n, nf = int(sys.argv[1]), 9
x = np.random.default_rng(n).standard_normal((nf, n))
d_x = G.dev(x)
outs = []
for rep in range(3):
    d_out = G.empty((nf, n, 2), torch.float64)
    e.hilbert(d_x, nf, n, d_out); e.sync()
    outs.append(G.host(d_out).view(np.uint64).copy())
print("COLD_DIFF", int((outs[0] != outs[2]).sum()), int((outs[1] != outs[2]).sum()))
"""


@pytest.mark.parametrize("n", [8192, 16384])
def test_hilbert_first_launch_in_a_process_equals_later_ones(n):
    """A kernel's very first launch in a process (cold instruction cache) stretches the window of the store-data hazard that
    k_hilbert_xl's 128-bit buffer stores had (round 3: 16-48 samples with a wrong low word, first launch only; the CPU-side guard is
    test_no_unprotected_wide_buffer_store_hazard).  Fresh interpreter, the transform as its first GPU work, three launches bit-equal."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _ in range(3):
        out = subprocess.run([sys.executable, "-c", _COLD, str(n)], cwd=root, check=True, capture_output=True, text=True, timeout=300).stdout
        assert "COLD_DIFF 0 0" in out, out


_COLD_ALL = r"""
import os, sys, zlib
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np, torch
import gpu_util as G
from pyspecsdr_amd import _lib as L
e = G.engine()
rng = np.random.default_rng(7)
def iq(nf, n):
    t = np.arange(n)
    return (0.1 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))) + 0.5 * np.exp(2j * np.pi * rng.uniform(-0.3, 0.3, (nf, 1)) * t)).astype(np.complex64)
cases = []
for n in (256, 1024, 2048, 4096, 8192, 16384, 3000):
    cases.append(("spectrum", n, G.dev(iq(40, n)), 40))
for n in (1024, 4096):
    cases.append(("scan", n, G.dev(iq(40, n)), 40))
for mode, n, nf in ((L.MODE_NFM, 1024, 300), (L.MODE_NFM, 32768, 2), (L.MODE_AM, 16384, 9), (L.MODE_USB, 16384, 9), (L.MODE_USB, 2048, 40), (L.MODE_WFM, 2048, 130), (L.MODE_WFM, 32768, 1)):
    cases.append(("demod%d" % mode, n, G.dev(iq(nf, n)), nf))
cases.append(("power", 16384, G.dev(iq(9, 16384)), 9))
cases.append(("iqcorr", 4096, G.dev(iq(9, 4096)), 9))
def run(kind, n, d, nf):
    fs = 2.4e6 if n <= 4096 else 250e3
    if kind == "spectrum":
        o = G.empty((nf, n), torch.float32); e.spectrum_db(d, nf, n, o); e.sync(); return [G.host(o)]
    if kind == "scan":
        o, pk, bw, c = G.empty((nf, n), torch.float32), G.empty((nf,), torch.float32), G.empty((nf,), torch.float64), G.empty((nf,), torch.int32)
        e.scan(d, nf, n, fs, o, pk, bw, c); e.sync(); return [G.host(o), G.host(pk), G.host(c)]
    if kind.startswith("demod"):
        mode = int(kind[5:]); n_out = e.demod_out_len(mode, n, fs)
        pcm, au = G.empty((nf, n_out, 2), torch.int16), G.empty((nf, n_out * (2 if mode == L.MODE_WFM else 1)), torch.float64)
        e.demod(mode, d, nf, n, fs, pcm, au); e.sync(); return [G.host(pcm), G.host(au)]
    if kind == "power":
        o = G.empty((nf,), torch.float32); e.power_db(d, nf, n, o); e.sync(); return [G.host(o)]
    o = G.empty((nf, n, 2), torch.float32); e.iq_correction(d, nf, n, o); e.sync(); return [G.host(o)]
bad = []
first = [[zlib.crc32(a.tobytes()) for a in run(*c)] for c in cases]     # every kernel family's first launch in this process
for rep in range(2):
    for c, f in zip(cases, first):
        if [zlib.crc32(a.tobytes()) for a in run(*c)] != f: bad.append((c[0], c[1], rep))
print("COLD_ALL", len(cases), bad)
"""


def test_first_launches_in_a_process_equal_later_ones():
    """Every kernel family's first launch in a fresh interpreter against its second and third on the same input, byte for byte
    (spectra 256 ... 16384 and a Bluestein length, scanner slices, NFM / AM / SSB / WFM on both batch shapes, power, iq_correction):
    the generic form of the Hilbert check below — a hazard that only a cold instruction cache exposes shows up here."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _ in range(2):
        out = subprocess.run([sys.executable, "-c", _COLD_ALL], cwd=root, check=True, capture_output=True, text=True, timeout=600).stdout
        assert "COLD_ALL 18 []" in out, out[-2000:]


@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 1048576])
def test_hilbert_rows(n):
    """pss_hilbert = scipy.signal.hilbert along rows (fft, one-sided mask, ifft; _signaltools.py:2318), both transforms in one
    kernel; against the same statements in NumPy float64."""
    rng = np.random.default_rng(n)
    nf = 77 if n <= 4096 else (9 if n <= 65536 else 3)      # above 16384 (the reference's read buffers): spectrum through HBM
    x = rng.standard_normal((nf, n)) * rng.uniform(0.01, 10.0, (nf, 1))
    x[1] = np.cos(2 * np.pi * 37 * np.arange(n) / n)          # analytic signal of a cosine: exp(i w t)
    e = G.engine()
    d_out = G.empty((nf, n, 2), torch.float64)
    e.hilbert(G.dev(x), nf, n, d_out)
    e.sync()
    got = G.host(d_out).view(np.complex128).reshape(nf, n)
    X = np.fft.fft(x, axis=1)
    h = np.zeros(n); h[0] = h[n // 2] = 1; h[1:n // 2] = 2
    ref = np.fft.ifft(X * h, axis=1)
    scale = np.max(np.abs(x), axis=1, keepdims=True)
    assert np.max(np.abs(got - ref) / scale) < 1e-13
    assert np.max(np.abs(got[1] - np.exp(2j * np.pi * 37 * np.arange(n) / n))) < 1e-12
    assert np.max(np.abs(got.real - x) / scale) < 1e-13      # the real part is the input (what demodulate_ssb keeps)
    with pytest.raises(Exception):
        e.hilbert(G.dev(x[:, :100].copy()), nf, 100, d_out)


def test_am_ssb_ragged_vs_oracle():
    rng = np.random.default_rng(78)
    nf, n = 67, 1500   # not a multiple of the 64-frame tile nor of the 64/1024-sample chunks
    iq = (0.3 + 0.2 * rng.standard_normal((nf, n)) + 0.2j * rng.standard_normal((nf, n))).astype(np.complex64)
    e = G.engine()
    sos = np.empty((5, 6))
    e.lib.pss_am_bandpass_sos(sos.ctypes.data)
    pcm, audio = G.demod(L.MODE_AM, iq, 2.4e6)
    for k in range(nf):
        a = O.demod_am(iq[k], sos)
        assert np.array_equal(audio[k], a), k
        assert np.array_equal(pcm[k], O.pcm16_stereo(a)), k
    taps = e.ssb_taps(1.024e6)
    pcm, audio = G.demod(L.MODE_USB, iq, 1.024e6)
    for k in range(nf):
        a = O.demod_ssb(iq[k], taps)
        assert np.array_equal(audio[k], a), k
        assert np.array_equal(pcm[k], O.pcm16_stereo(a)), k


@pytest.mark.parametrize("n", [7, 100, 1024, 16384, 20000, 32768, 40001])
def test_power(golden, n):
    g = golden["power"]
    e = G.engine()
    iq = g[f"iq_{n}"]
    d_p = G.empty((1,), torch.float32)
    e.power_db(G.dev(iq), 1, n, d_p)
    e.sync()
    p = G.host(d_p)[0]
    assert p.tobytes() == np.float32(g[f"p_{n}"]).tobytes()     # bit-exact: NumPy's mean tree + its (SVML) float32 log10
    assert p.tobytes() == np.float32(O.power_db(iq)).tobytes()


def test_numpy_float32_primitives(golden):
    """The device models of NumPy's float32 arctan2 / log10 (SVML under AVX512_SKX) and abs(complex64), element by element
    against NumPy's own outputs (fixtures) and, on random bit patterns, against the oracle; NaNs compared as NaNs."""
    e = G.engine()

    def run(op, a, b=None):
        d_out = G.empty((len(a),), torch.float32)
        e.np_f32(op, G.dev(np.ascontiguousarray(a)), None if b is None else G.dev(np.ascontiguousarray(b)), len(a), d_out)
        e.sync()
        return G.host(d_out)

    def same(got, want):
        nan = np.isnan(want)
        return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))

    for name in ("atan2f", "atan2f_bits"):
        g = golden[name]
        assert same(run(L.NP_ARCTAN2, g["y"], g["x"]), g["theta"]), name
    g = golden["log10f"]
    assert same(run(L.NP_LOG10, g["x"]), g["y"])
    rng = np.random.default_rng(92)
    a = rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    b = rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert same(run(L.NP_ARCTAN2, a, b), O.atan2f(a, b))
    assert same(run(L.NP_LOG10, a), O.log10f(a))
    assert same(run(L.NP_ABS, a, b), O.cabsf(a, b))
    with pytest.raises(Exception):
        run(7, a, b)


def test_power_bits_over_the_float_range():
    # tiny frames with magnitudes all over the float32 range (down to denormal powers, up to overflow): the float32 log10
    # model must agree with the oracle's (which is pinned to NumPy's outputs) in every bit, -inf / inf / NaN included
    rng = np.random.default_rng(91)
    e = G.engine()
    nf, n = 20000, 7
    mag = np.exp2(rng.uniform(-74, 64, (nf, 1))).astype(np.float32)
    iq = ((rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))) * mag).astype(np.complex64)
    iq[0] = 0
    iq[1, 3] = np.inf
    iq[2, 2] = np.nan
    d_p = G.empty((nf,), torch.float32)
    e.power_db(G.dev(iq), nf, n, d_p)
    e.sync()
    p = G.host(d_p)
    want = np.array([O.power_db(iq[f]) for f in range(nf)], np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(p), nan) and np.array_equal(p[~nan].view(np.uint32), want[~nan].view(np.uint32))


def test_iq_correction_and_raw_bit_exact(golden):
    """signal_processing.py:46-80 and the RAW mode of demodulate_signal (:222-238): every float32 bit."""
    g = golden["iqcorr"]
    e = G.engine()
    for n in [int(v) for v in g["sizes"]] + ["u8"]:
        iq, want = g[f"iq_{n}"], g[f"corr_{n}"]
        m = len(iq)
        d_out, d_raw = G.empty((m, 2), torch.float32), G.empty((m,), torch.float32)
        e.iq_correction(G.dev(iq), 1, m, d_out, d_raw)
        e.sync()
        got = G.host(d_out).reshape(-1).view(np.complex64)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
        assert np.array_equal(G.host(d_raw).view(np.uint32), want.real.copy().view(np.uint32)), n
    fz = g["iq_fuzz"]
    d_out = G.empty(fz.shape + (2,), torch.float32)
    e.iq_correction(G.dev(fz), fz.shape[0], fz.shape[1], d_out, None)
    e.sync()
    got = G.host(d_out).reshape(fz.shape[0], -1).view(np.complex64)
    assert np.array_equal(got.view(np.uint32), g["corr_fuzz"].view(np.uint32))
    import pyspecsdr_amd.signal_processing as sp
    raw = sp.demodulate_signal(g["iq_1000"], 2.4e6, "RAW")
    assert raw.dtype == np.float32 and np.array_equal(raw.view(np.uint32), g["raw_1000"].view(np.uint32))
    c = sp.iq_correction(g["iq_4096"])
    assert c.dtype == np.complex64 and np.array_equal(c.view(np.uint32), g["corr_4096"].view(np.uint32))


def test_iq_correction_batch_vs_oracle():
    rng = np.random.default_rng(808)
    e = G.engine()
    # (20 000 x 1024: more frames than workgroups — every workgroup of the one-wavefront-per-frame kernel walks two or three frames, the next
    # one prefetched while the current one is reduced)
    for nf, n in [(300, 1024), (20000, 1024), (5, 9000), (40000, 256), (3, 77)]:
        iq = ((rng.standard_normal((nf, n)) * 0.3 + 0.04) + 1j * (rng.standard_normal((nf, n)) * 0.2 - 0.03)).astype(np.complex64)
        d_out = G.empty((nf, n, 2), torch.float32)
        e.iq_correction(G.dev(iq), nf, n, d_out, None)
        e.sync()
        got = G.host(d_out).reshape(nf, -1).view(np.complex64)
        want = np.stack(O.map_frames(O.iq_correction, iq))         # every frame
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(nf, -1).any(axis=1))[0]
        assert bad.size == 0, (nf, n, bad[:16].tolist())
        # property at batch size: the output power equals the (DC-removed) input power, and the I/Q imbalance is gone
        c = got.astype(np.complex128)
        assert np.allclose(np.var(c, axis=1), np.var(iq.astype(np.complex128), axis=1), rtol=2e-5)
        assert np.all(np.abs(np.mean(c.real * c.imag, axis=1)) < 1e-6 * n ** 0.5 + 2e-7)


def _wfm(e, iq2d, fs, dispatcher=True):
    nf, n = iq2d.shape
    n_out = e.demod_out_len(L.MODE_WFM, n, fs)
    d_pcm, d_au = G.empty((nf, n_out, 2), torch.int16), G.empty((nf, n_out, 2), torch.float64)
    (e.demod_signal if dispatcher else e.demod)(L.MODE_WFM, G.dev(iq2d), nf, n, fs, d_pcm, d_au)
    e.sync()
    return G.host(d_pcm), G.host(d_au)


def _wfm_filters(g, fs):
    key = str(int(fs))
    return {k: g[f"{k}_{key}"] for k in ("lp_sos", "pilot_sos", "lmr_sos", "alpha", "dec_sos", "dec_zi")}


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e", "f", "g"])
def test_wfm_vs_golden_bit_exact(golden, tag):
    """demodulate_signal(..., 'WFM') (signal_processing.py:220-228 -> :46-80 -> :119-176) with SciPy's coefficient
    tables injected: float64 (n_out, 2) audio and its int16 image, bit for bit."""
    g = golden["wfm"]
    fs = float(g[f"fs_{tag}"])
    e = G.engine()
    f = _wfm_filters(g, fs)
    e.set_wfm_filters(fs, f["lp_sos"], f["pilot_sos"], f["lmr_sos"], float(f["alpha"]))
    taps, _, _ = e.nfm_filters(fs)
    e.set_nfm_filters(fs, taps, f["dec_sos"], f["dec_zi"])
    want = g[f"audio_{tag}"]
    for small_batch in (1, 0):   # systolic small-batch kernels (default for a few frames) and the fused large-batch kernels
        e.set_option("small_batch", small_batch)
        try:
            pcm, audio = _wfm(e, g[f"iq_{tag}"], fs)
        finally:
            e.set_option("small_batch", 1)
        assert audio.shape == want.shape
        assert np.array_equal(audio.view(np.uint64), want.view(np.uint64)), (small_batch, np.abs(audio - want).max())
        assert np.array_equal(pcm, g[f"pcm_{tag}"])


def test_wfm_designed_filters_and_shim(golden):
    # library-designed tables: SciPy's bits since round 3 (the designers restate SciPy's / NumPy's arithmetic incl. NumPy's SVML tan / exp),
    # so a context that never saw a SciPy table produces the reference's float64 audio and int16 PCM bit for bit
    g = golden["wfm"]
    from pyspecsdr_amd.engine import Engine
    e2 = Engine(0)
    for tag in ("a", "c", "d", "e"):
        fs = float(g[f"fs_{tag}"])
        lp, pil, lmr, alpha = e2.wfm_filters(fs)
        key = str(int(fs))
        assert np.array_equal(lp, g[f"lp_sos_{key}"]) and np.array_equal(pil, g[f"pilot_sos_{key}"]) and np.array_equal(lmr, g[f"lmr_sos_{key}"])
        assert alpha == float(g[f"alpha_{key}"]) if f"alpha_{key}" in g.files else True
        pcm, audio = _wfm(e2, g[f"iq_{tag}"], fs)
        assert np.array_equal(audio, g[f"audio_{tag}"]), tag
        assert np.array_equal(pcm, g[f"pcm_{tag}"]), tag
    # the de-emphasis coefficient and the pre-warped tables at sample rates where NumPy's SVML exp / tan are NOT libm's (live NumPy: only
    # where it runs the AVX512_SKX dispatch the models restate — the goldens above cover the tables elsewhere)
    import scipy.signal as ss
    from numpy._core._multiarray_umath import __cpu_features__ as cpu
    n_svml = 0
    for fs in (np.linspace(300e3, 12e6, 400) if cpu.get("AVX512_SKX") else []):
        lp, pil, lmr, alpha = e2.wfm_filters(float(fs))
        n_svml += float(np.exp(-1 / (75e-6 * fs))) != math.exp(-1 / (75e-6 * fs))
        assert alpha == float(np.exp(-1 / (75e-6 * fs))), fs
        assert np.array_equal(lmr, ss.butter(5, [23000 / (fs / 2), 53000 / (fs / 2)], btype="band", output="sos")), fs
    assert n_svml > 5 or not cpu.get("AVX512_SKX")
    e2.close()
    import pyspecsdr_amd.signal_processing as sp
    x = g["iq_a"][0]
    a = sp.demodulate_signal(x, 2.4e6, "WFM")
    assert a.dtype == np.float64 and a.shape == (10, 2)
    assert np.array_equal(a.view(np.uint64), g["audio_a"][0].view(np.uint64))  # the shim injects SciPy's tables
    assert np.array_equal(sp.demodulate_pcm(x, 2.4e6, "WFM"), g["pcm_a"][0])
    with pytest.raises(ValueError):
        sp.demodulate_signal(x[:28], 2.4e6, "WFM")      # sosfiltfilt padlen
    with pytest.raises(ValueError):
        sp.demodulate_signal(x, 100e3, "WFM")           # butter: 53 kHz >= fs/2


def test_wfm_batch_vs_oracle():
    rng = np.random.default_rng(4242)
    e = G.engine()
    for nf, n, fs in ((130, 1024, 2.4e6), (3, 5000, 1.024e6), (2, 40, 250e3), (67, 333, 2.048e6)):
        ph = np.cumsum(rng.standard_normal((nf, n)) * 0.15, axis=1)
        iq = (0.5 * np.exp(1j * ph) + 0.02 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
        lp, pil, lmr, alpha = e.wfm_filters(fs)
        _, sos, zi = e.nfm_filters(fs)
        filt = dict(lp_sos=lp, pilot_sos=pil, lmr_sos=lmr, alpha=alpha, dec_sos=sos, dec_zi=zi)
        pcm, audio = _wfm(e, iq, fs, dispatcher=False)      # demodulate_wfm proper (no IQ correction)
        pcm2, audio2 = _wfm(e, iq, fs, dispatcher=True)
        for f in list(range(min(nf, 6))) + [nf - 1]:
            a = O.demod_wfm(iq[f], fs, filt)
            assert np.array_equal(audio[f].view(np.uint64), a.view(np.uint64)), (nf, n, fs, f)
            assert np.array_equal(pcm[f], np.int16(a * 32767))
            a2 = O.demod_wfm(O.iq_correction(iq[f]), fs, filt)
            assert np.array_equal(audio2[f].view(np.uint64), a2.view(np.uint64)), (nf, n, fs, f)
        # property at batch size: both channels peak-normalised jointly -> max |audio| over the frame is exactly 1
        assert np.all(np.abs(audio).max(axis=(1, 2)) == 1.0)


def test_wfm_small_batch_array_at_block_edges():
    """The small-batch WFM path is ONE block-systolic array since round 3 (k_wfm_mrg: both filter passes and the forward decimator, 64-sample
    blocks, the odd-extended sequence 27 samples out of step with them): frame lengths around every block boundary of the audio row
    (M = n - 1) and of its extension (M + 54), one to five frames (two frames per workgroup), against the oracle bit for bit."""
    rng = np.random.default_rng(77)
    e = G.engine()
    fs = 250e3
    lp, pil, lmr, alpha = e.wfm_filters(fs)
    _, sos, zi = e.nfm_filters(fs)
    filt = dict(lp_sos=lp, pilot_sos=pil, lmr_sos=lmr, alpha=alpha, dec_sos=sos, dec_zi=zi)
    for n in (29, 30, 37, 38, 64, 65, 66, 74, 75, 76, 92, 128, 129, 130, 139, 193, 1000, 4097):
        for nf in (1, 2, 3, 5):
            ph = np.cumsum(rng.standard_normal((nf, n)) * 0.2, axis=1)
            iq = (0.5 * np.exp(1j * ph) + 0.02 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
            pcm, audio = _wfm(e, iq, fs, dispatcher=False)
            for f in range(nf):
                a = O.demod_wfm(iq[f], fs, filt)
                assert np.array_equal(audio[f].view(np.uint64), a.view(np.uint64)), (n, nf, f)


def test_wfm_fused_and_unfused_paths_agree():
    # the fused forward kernel (k_wfm_fwd + k_nfm_bwd) and the k_wfm_front + k_nfm_iir path must produce identical bits
    rng = np.random.default_rng(99)
    e = G.engine()
    for nf, n, fs in ((70, 1024, 2.4e6), (3, 29, 2.4e6), (5, 30, 250e3), (2, 45, 1.024e6), (65, 61, 2.4e6), (2, 4097, 2.048e6)):
        ph = np.cumsum(rng.standard_normal((nf, n)) * 0.2, axis=1)
        iq = (0.5 * np.exp(1j * ph) + 0.03 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
        pcm0, a0 = _wfm(e, iq, fs, dispatcher=False)        # small-batch: one lane per filter section
        e.set_option("small_batch", 0)
        try:
            pcm1, a1 = _wfm(e, iq, fs, dispatcher=False)    # fused forward kernel + backward kernel
            e.set_option("wfm_fused", 0)
            pcm2, a2 = _wfm(e, iq, fs, dispatcher=False)    # k_wfm_front + lane-per-frame decimator
        finally:
            e.set_option("wfm_fused", 1)
            e.set_option("small_batch", 1)
        assert np.array_equal(a1.view(np.uint64), a2.view(np.uint64)) and np.array_equal(pcm1, pcm2), (nf, n, fs)
        assert np.array_equal(a0.view(np.uint64), a1.view(np.uint64)) and np.array_equal(pcm0, pcm1), (nf, n, fs)


def test_bandpass_filter_and_sosfilt_rows(golden):
    """bandpass_filter (signal_processing.py:34-42) through the shim, and the batched sosfilt entry behind it."""
    import pyspecsdr_amd.signal_processing as sp
    g = golden["bandpass"]
    for tag in g["tags"]:
        lo, hi, fs = g[f"args_{tag}"]
        y = sp.bandpass_filter(g[f"x_{tag}"], lo, hi, fs)
        assert y.dtype == np.float64 and np.array_equal(y.view(np.uint64), g[f"y_{tag}"].view(np.uint64)), tag
    assert sp.CLASSIFY_RAISES_NAMEERROR is True          # the drop-in default is the reference's present behaviour
    with pytest.raises(NameError):
        sp.classify_signal(np.zeros(2048, np.complex64), 2.4e6, 1e4)   # the reference's own behaviour (App. C2)
    rng = np.random.default_rng(17)
    e = G.engine()
    x = rng.standard_normal((200, 777))
    sos = g["sos_afsk1200"]
    d_y = G.empty(x.shape, torch.float64)
    e.sosfilt(G.dev(x), x.shape[0], x.shape[1], sos, d_y)
    e.sync()
    y = G.host(d_y)
    for r in (0, 63, 64, 199):
        assert np.array_equal(y[r], O.sosfilt(sos, x[r]))


def test_recording_to_wav_roundtrip(tmp_path, golden):
    """Formats either side of the path: an np.save'd IQ recording (pyspecsdr.py:814-824) cut into read
    buffers, demodulated on the GPU, written as the WAV file audio_processing.py:25-43 would produce."""
    import wave
    from pyspecsdr_amd import formats
    g = golden["nfm"]
    frames = g["iq_a"]                                   # 6 buffers of 1024 samples
    rec = np.concatenate([frames.reshape(-1), frames[0][:100]])   # plus an incomplete tail buffer
    npy, wav = str(tmp_path / "rec.npy"), str(tmp_path / "rec.wav")
    np.save(npy, rec)
    pcm = formats.recording_to_wav(npy, wav, 2.4e6, "NFM", frame_len=1024)
    assert np.array_equal(pcm, g["pcm_a"])
    with wave.open(wav, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, 22050)
        assert w.readframes(w.getnframes()) == g["pcm_a"].tobytes() == formats.pipe_bytes(pcm)
    wf = golden["wfm"]
    pcm = formats.demodulate_recording(wf["iq_a"].reshape(-1), 2.4e6, "WFM", frame_len=1024, chunk_frames=3)
    assert np.array_equal(pcm, wf["pcm_a"])


@pytest.mark.parametrize("n", [65536, 70001, 131072, 1 << 20])
def test_long_frames_grouped_reductions(n):
    """Frames longer than one reduction group (8 ufunc chunks = 65536 samples), up to the reference's largest read
    buffer (pyspecsdr.py:2236, SAMPLES = 12): power, IQ correction and the AM mean against the oracle, bit for bit."""
    rng = np.random.default_rng(n)
    iq = ((rng.standard_normal((2, n)) * 0.3 + 0.05) + 1j * (rng.standard_normal((2, n)) * 0.25 - 0.02)).astype(np.complex64)
    e = G.engine()
    d_p = G.empty((2,), torch.float32)
    e.power_db(G.dev(iq), 2, n, d_p)
    d_out = G.empty((2, n, 2), torch.float32)
    e.iq_correction(G.dev(iq), 2, n, d_out, None)
    e.sync()
    p = G.host(d_p)
    got = G.host(d_out).reshape(2, -1).view(np.complex64)
    for f in range(2):
        assert p[f].tobytes() == np.float32(O.power_db(iq[f])).tobytes(), (n, f)
        assert np.array_equal(got[f].view(np.uint32), O.iq_correction(iq[f]).view(np.uint32)), (n, f)
    sos = np.empty((5, 6)); e.lib.pss_am_bandpass_sos(sos.ctypes.data)
    pcm, audio = G.demod(L.MODE_AM, iq[:1], 2.4e6)
    assert np.array_equal(audio[0], O.demod_am(iq[0], sos))


def test_spectrogram_cells(golden):
    """draw_spectrogram (pyspecsdr.py:398-498): float64 rows against the reference's own cell grids (incl. a full
    32768-sample buffer), float32 rows in a batch against the oracle."""
    g = golden["caller"]
    e = G.engine()
    for tag in g["sg_tags"]:
        hh, ww = [int(v) for v in g[f"sg_hw_{tag}"]]
        row = g[f"sg_row_{tag}"]
        dh, dw = hh - 4, ww - 7
        d_gl, d_co = G.empty((dh, dw), torch.int8), G.empty((dh, dw), torch.int8)
        d_rg = G.empty((1, 2), torch.float64)
        e.spectrogram_cells(G.dev(row), 1, len(row), dh, dw, d_gl, d_co, d_rg, f64=True)
        e.sync()
        assert np.array_equal(G.host(d_gl), g[f"sg_glyph_{tag}"]), tag
        assert np.array_equal(G.host(d_co), g[f"sg_colour_{tag}"]), tag
        _, _, dmin, dmax = O.spectrogram_cells(row, dh, dw)
        assert np.allclose(G.host(d_rg)[0], [dmin, dmax], rtol=1e-14, atol=0)
    rng = np.random.default_rng(12)
    rows = (rng.standard_normal((37, 2044)) * 5 - 40).astype(np.float32)
    rows[:, 700:760] += 35
    rows[3, 10] = np.nan                                        # excluded from the statistics; its columns stay undrawn
    d_gl, d_co = G.empty((37, 30, 100), torch.int8), G.empty((37, 30, 100), torch.int8)
    e.spectrogram_cells(G.dev(rows), 37, 2044, 30, 100, d_gl, d_co, None)
    e.sync()
    gl, co = G.host(d_gl), G.host(d_co)
    for f in (0, 3, 36):
        ogl, oco, _, _ = O.spectrogram_cells(rows[f].astype(np.float64), 30, 100)
        assert np.array_equal(gl[f], ogl) and np.array_equal(co[f], oco), f


def test_gradient_waterfall_and_surface_cells(golden):
    """draw_gradient_waterfall (pyspecsdr.py:1640-1716) and draw_surface_plot (:1567-1616) against the reference's grids."""
    g = golden["caller"]
    rows = g["rows"]
    H, W = [int(v) for v in g["hw"]]
    e = G.engine()
    d_gl, d_co = G.empty((H - 4, W - 10), torch.int8), G.empty((H - 4, W - 10), torch.int8)
    for i in (0, 7, 29, 32):
        ring = np.ascontiguousarray(rows[max(0, i + 1 - 30):i + 1])
        e.gradient_cells(G.dev(ring), ring.shape[0], ring.shape[1], H - 4, W - 10, d_gl, d_co, f64=True)
        e.sync()
        assert np.array_equal(G.host(d_gl), g["gw_glyph"][i]) and np.array_equal(G.host(d_co), g["gw_colour"][i]), i
    for i, (row, hh, ww) in enumerate(((rows[0], 40, 120), (rows[5], 40, 120), (g["sg_row_big"], 50, 200))):
        d_c = G.empty((hh, ww), torch.int8)
        e.surface_cells(G.dev(np.ascontiguousarray(row)), len(row), hh, ww, d_c, f64=True)
        e.sync()
        assert np.array_equal(G.host(d_c), g[f"sf_colour_{i}"]), i
    r32 = rows[3].astype(np.float32)
    d_c = G.empty((40, 120), torch.int8)
    e.surface_cells(G.dev(r32), len(r32), 40, 120, d_c)
    e.sync()
    assert np.array_equal(G.host(d_c), O.surface_cells(r32.astype(np.float64), 40, 120))


def test_vector_display_cells(golden):
    g = golden["caller"]
    e = G.engine()
    for tag, hh, ww in (("a", 40, 120), ("b", 25, 81)):
        d_g = G.empty((hh, ww), torch.int8)
        e.vector_cells(G.dev(g["vec_iq"]), len(g["vec_iq"]), hh, ww, d_g)
        e.sync()
        assert np.array_equal(G.host(d_g), g[f"vec_grid_{tag}"]), tag


def test_empty_batches_and_non_finite_samples(golden):
    """Edge cases: zero frames through every batched entry point; NaN / Inf samples behave as in the reference's
    arithmetic (they poison the frame they are in — and only that frame)."""
    e = G.engine()
    z = G.empty((0, 1024, 2), torch.float32)
    e.spectrum_db(z, 0, 1024, G.empty((0, 1024), torch.float32))
    e.power_db(z, 0, 1024, G.empty((0,), torch.float32))
    e.iq_correction(z, 0, 1024, G.empty((0, 1024, 2), torch.float32), None)
    for mode in (L.MODE_NFM, L.MODE_AM, L.MODE_USB, L.MODE_WFM):
        e.demod_signal(mode, z, 0, 1024, 2.4e6, G.empty((0, 10, 2), torch.int16), None)
    e.spectrum_nfm(z, 0, 1024, 2.4e6, G.empty((0, 1024), torch.float32), G.empty((0, 10, 2), torch.int16))
    e.sync()
    rng = np.random.default_rng(31)
    iq = (0.4 * np.exp(2j * np.pi * np.cumsum(rng.standard_normal((5, 1024)) * 0.05, axis=1))).astype(np.complex64)
    iq[1, 500] = complex(np.nan, 0.1)
    iq[3, 17] = complex(np.inf, -0.2)
    taps, sos, zi = e.nfm_filters(2.4e6)
    with np.errstate(all="ignore"):
        pcm, audio = G.demod(L.MODE_NFM, iq, 2.4e6)
        for f in range(5):
            ref = O.demod_nfm(iq[f], 2.4e6, taps, sos, zi)
            assert np.array_equal(audio[f], ref, equal_nan=True), f
            assert np.array_equal(pcm[f, :, 0], np.int16(np.nan_to_num(ref * 32767, nan=0.0))), f
        assert np.isnan(audio[1]).all() and np.isfinite(audio[[0, 2, 4]]).all()   # (an Inf sample only bends the angle)
        am = np.empty((5, 6)); e.lib.pss_am_bandpass_sos(am.ctypes.data)
        pcm, audio = G.demod(L.MODE_AM, iq, 2.4e6)
        for f in range(5):
            assert np.array_equal(audio[f], O.demod_am(iq[f], am), equal_nan=True), f
        d_p = G.empty((5,), torch.float32)
        e.power_db(G.dev(iq), 5, 1024, d_p)
        e.sync()
        p = G.host(d_p)
        assert np.isnan(p[1]) and np.isinf(p[3]) and np.isfinite(p[[0, 2, 4]]).all()
        db = G.spectrum(iq)
        assert np.isnan(db[1]).all() and np.isfinite(db[[0, 2, 4]]).all()


def test_round2_entry_points_edge_cases():
    """Zero frames through the batched accumulators / pipeline / Hilbert; infinities inside a dB row (np.median and the
    np.isfinite masks of the accumulators); argument checks."""
    from pyspecsdr_amd.engine import PssError
    e = G.engine()
    z1 = G.empty((0,), torch.float32)
    e.spectrum_post_extremes(G.empty((0, 1024), torch.float32), 0, 1024, G.empty((0, 1020), torch.float32), z1, z1)
    e.row_extremes(G.empty((0, 1020), torch.float32), 0, 1020, z1, z1)
    e.waterfall_rows(G.empty((0, 1020), torch.float32), 0, 1020, z1, z1, 112, G.empty((0, 112), torch.int8), G.empty((0, 112), torch.int8))
    e.persistence_rows(G.empty((0, 1020), torch.float32), 0, 1020, z1, z1, 36, 112, G.empty((0, 112), torch.int8))
    e.spectrum_db_post(G.empty((0, 1024, 2), torch.float32), 0, 1024, G.empty((0, 1024), torch.float32), G.empty((0, 1020), torch.float32), z1, z1)
    e.frame_pipeline_nfm(G.empty((0, 1024, 2), torch.float32), 0, 1024, 2.4e6, G.empty((0, 1024), torch.float32),
                         G.empty((0, 1020), torch.float32), z1, z1, 112, G.empty((0, 112), torch.int8), G.empty((0, 112), torch.int8),
                         G.empty((0, 10, 2), torch.int16))
    e.hilbert(G.empty((0, 1024), torch.float64), 0, 1024, G.empty((0, 1024, 2), torch.float64))
    got = e.stream_display_nfm(np.zeros((0, 2048), np.complex64), 10e6, 16)
    assert got["pcm"].shape[0] == 0 and got["lines"][0].shape == (0, 112)
    e.sync()
    with pytest.raises(PssError):
        e.persistence_rows(G.empty((1, 1020), torch.float32), 1, 1020, G.empty((1,), torch.float32), G.empty((1,), torch.float32), 128, 112,
                           G.empty((1, 112), torch.int8))                         # row indices are int8
    with pytest.raises(PssError):
        e.spectrum_post_extremes(G.empty((1, 1024), torch.float32), 1, 1024, G.empty((1, 1020), torch.float32), None, None)
    # infinities: +inf / -inf stretches in otherwise ordinary rows (np.median is well defined; the extremes skip them)
    rng = np.random.default_rng(8)
    for n in (1024, 4096):
        db = (rng.standard_normal((6, n)) * 5.0 - 50.0).astype(np.float32)
        db[1, 100:160] = np.inf
        db[2, 300:310] = -np.inf
        db[3, : n // 2 + 50] = np.inf                                                  # the median itself is +inf
        db[4, 7] = -np.inf
        db[4, 900:960] = np.inf
        d_post, d_lo, d_hi = G.empty((6, n - 4), torch.float32), G.empty((6,), torch.float32), G.empty((6,), torch.float32)
        e.spectrum_post_extremes(G.dev(db), 6, n, d_post, d_lo, d_hi)
        e.sync()
        post, lo, hi = G.host(d_post), G.host(d_lo), G.host(d_hi)
        with np.errstate(all="ignore"):
            for f in range(6):
                sm = np.convolve(db[f].astype(np.float64), np.ones(5) / 5, mode="valid")
                sm32 = sm.astype(np.float32)
                thr = np.float32(np.median(sm32.astype(np.float64)) - 10)
                ref = np.where(sm32 < thr, thr, sm32)
                ok = (post[f] == ref) | (np.abs(post[f] - ref) <= 1e-4 * np.maximum(np.abs(ref), 1.0))
                assert ok.all(), (n, f, np.nonzero(~ok)[0][:5], post[f][~ok][:5], ref[~ok][:5])
                fin = post[f][np.isfinite(post[f])]
                if len(fin):
                    assert lo[f] == fin.min() and hi[f] == fin.max(), (n, f)
                else:
                    assert lo[f] == np.inf and hi[f] == -np.inf, (n, f)


def test_afsk_bits(golden):
    """decode_afsk (decoders.py:94-112): the reference's bit lists, and a batch of rows against the oracle."""
    g = golden["afsk"]
    e = G.engine()
    for tag in g["tags"]:
        x, fs = g[f"x_{tag}"], float(g[f"fs_{tag}"])
        nb = e.afsk_n_bits(len(x), fs)
        assert nb == len(g[f"bits_{tag}"])
        if nb == 0:
            continue
        d_bits = G.empty((1, nb), torch.uint8)
        e.afsk_bits(G.dev(x), 1, len(x), fs, d_bits, g[f"sos1200_{tag}"], g[f"sos2200_{tag}"])
        e.sync()
        assert np.array_equal(G.host(d_bits)[0], g[f"bits_{tag}"]), tag
    rng = np.random.default_rng(8)
    x = rng.standard_normal((70, 5000))
    nb = e.afsk_n_bits(5000, 22050.0)
    d_bits = G.empty((70, nb), torch.uint8)
    e.afsk_bits(G.dev(x), 70, 5000, 22050.0, d_bits, g["sos1200_a"], g["sos2200_a"])
    e.sync()
    bits = G.host(d_bits)
    for r in (0, 63, 64, 69):
        assert np.array_equal(bits[r], O.afsk_bits(x[r], 22050.0, g["sos1200_a"], g["sos2200_a"])), r


def test_classify_signal(golden):
    """classify_signal with `welch` bound vs the reference's goldens and vs the oracle: label and bandwidth
    equal, modulation index bit-exact, PSD within 1e-4 relative above the 1e-10 floor, flatness within 1e-5."""
    import pyspecsdr_amd.signal_processing as sp
    g = golden["classify"]
    fs = float(g["fs"])
    e = G.engine()
    sp.CLASSIFY_RAISES_NAMEERROR = False      # the function as written (what `run.py --fix-classify` selects)
    for tag in g["tags"]:
        iq = g[f"iq_{tag}"]
        lab, bw, mi, fl = sp.classify_signal_features(iq, fs)
        rmi, rfl = g[f"mi_{tag}"], float(g[f"flat_{tag}"])
        assert lab == str(g[f"label_{tag}"]) == sp.classify_signal(iq, fs, 0.0), tag
        assert bw == float(g[f"bw_{tag}"]), tag
        assert mi.tobytes() == rmi.tobytes() or (np.isnan(mi) and np.isnan(rmi)), (tag, mi, rmi)
        assert float(fl) == rfl or abs(float(fl) - rfl) <= 1e-5 * abs(rfl), (tag, fl, rfl)
        # device-resident entry with the PSD, against the reference's and (tightly) against the oracle's
        n = len(iq)
        d_psd, d_lab = G.empty((1, 1024), torch.float32), G.empty((1,), torch.int32)
        e.classify(G.dev(iq.view(np.float32).reshape(1, n, 2)), 1, n, fs, d_label=d_lab, d_psd=d_psd)
        e.sync()
        psd, ref = d_psd.cpu().numpy()[0], g[f"psd_{tag}"]
        assert np.all(np.abs(psd - ref) <= 1e-5 * (ref + 1e-10) + 1e-6 * np.sqrt(ref * np.max(ref))), tag   # float32-FFT noise of the reference: ~1e-7 sqrt(p P_peak)
        olab, obw, omi, ofl, opsd = O.classify(iq, fs)
        assert e.class_name(int(d_lab.cpu()[0])) == olab == lab and obw == bw, tag
        assert omi.tobytes() == mi.tobytes() or (np.isnan(omi) and np.isnan(mi)), tag
        assert np.all(np.abs(psd - opsd) <= 1e-6 * (opsd + 1e-10)), tag
    try:
        with pytest.raises(ValueError):
            sp.classify_signal(np.zeros(0, np.complex64), fs, 0.0)
    finally:
        sp.CLASSIFY_RAISES_NAMEERROR = True


def test_classify_signal_short_reads(golden):
    """Reads shorter than Welch's 1024-sample segment (signal_processing.py:299; SciPy then takes ONE segment of len(x) samples):
    same bars as test_classify_signal, n = 1023 .. 1, against the reference's goldens and the oracle; then a batch."""
    import pyspecsdr_amd.signal_processing as sp
    g = golden["classify_short"]
    e = G.engine()
    for tag in g["tags"]:
        iq, fs = g[f"iq_{tag}"], float(g[f"fs_{tag}"])
        n = len(iq)
        lab, bw, mi, fl = sp.classify_signal_features(iq, fs)
        rmi, rfl = g[f"mi_{tag}"], float(g[f"flat_{tag}"])
        assert lab == str(g[f"label_{tag}"]), tag
        assert bw == float(g[f"bw_{tag}"]), tag
        assert mi.tobytes() == rmi.tobytes() or (np.isnan(mi) and np.isnan(rmi)), (tag, mi, rmi)
        assert float(fl) == rfl or abs(float(fl) - rfl) <= 1e-5 * abs(rfl), (tag, fl, rfl)
        d_psd, d_lab = G.empty((1, 1024), torch.float32), G.empty((1,), torch.int32)
        e.classify(G.dev(iq.view(np.float32).reshape(1, n, 2)), 1, n, fs, d_label=d_lab, d_psd=d_psd)
        e.sync()
        psd, ref = d_psd.cpu().numpy()[0, :n], g[f"psd_{tag}"]
        assert np.all(np.abs(psd - ref) <= 1e-5 * (ref + 1e-10) + 1e-6 * np.sqrt(ref * np.max(ref))), tag
        olab, obw, omi, ofl, opsd = O.classify(iq, fs)
        assert e.class_name(int(d_lab.cpu()[0])) == olab == lab and obw == bw, tag
        assert np.all(np.abs(psd - opsd) <= 1e-6 * (opsd + 1e-10)), tag
    rng = np.random.default_rng(78)
    for nf, n, fs in ((300, 1000, 2.4e6), (41, 333, 250e3), (7, 6, 2.4e6)):
        iq = ((rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))) * 0.05 +
              0.5 * np.exp(2j * np.pi * np.cumsum(rng.uniform(-0.2, 0.2, (nf, 1)) + 0.01 * rng.standard_normal((nf, n)), axis=1))).astype(np.complex64)
        d_lab, d_bw = G.empty((nf,), torch.int32), G.empty((nf,), torch.float64)
        d_mi, d_fl, d_psd = G.empty((nf,), torch.float32), G.empty((nf,), torch.float32), G.empty((nf, 1024), torch.float32)
        e.classify(G.dev(iq.view(np.float32).reshape(nf, n, 2)), nf, n, fs, d_lab, d_bw, d_mi, d_fl, d_psd)
        e.sync()
        lab, bw, mi, fl, psd = (a.cpu().numpy() for a in (d_lab, d_bw, d_mi, d_fl, d_psd))
        for f in range(nf):
            olab, obw, omi, ofl, opsd = O.classify(iq[f], fs)
            assert O.CLASS_LABELS[lab[f]] == olab and bw[f] == obw, (n, f)
            assert mi[f].tobytes() == omi.tobytes(), (n, f, mi[f], omi)
            assert abs(float(fl[f]) - float(ofl)) <= 1e-5 * abs(float(ofl)), (n, f)
            assert np.all(np.abs(psd[f, :n] - opsd) <= 1e-6 * (opsd + 1e-10)), (n, f)


def test_classify_batch_vs_oracle():
    """A scanner sweep's worth of reads in one call (cfg-4-like slices and a long dwell), every output against the oracle."""
    rng = np.random.default_rng(77)
    e = G.engine()
    fs = 2.4e6
    for nf, n in ((37, 4096), (5, 2048), (3, 70001), (2, 1 << 20)):   # up to the reference's largest read buffer
        t = np.arange(n) / fs
        iq = np.empty((nf, n), np.complex64)
        for f in range(nf):
            kind = f % 4
            off, dev, noise = rng.uniform(-6e5, 6e5), (0.0, 5e3, 75e3, 3e5)[kind], 10.0 ** rng.uniform(-3, -1)
            ph = 2 * np.pi * dev * np.cumsum(np.sin(2 * np.pi * rng.uniform(300, 15e3) * t)) / fs + 2 * np.pi * off * t
            amp = 0.0 if f % 7 == 6 else 0.5
            iq[f] = (amp * np.exp(1j * ph) + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
        d_lab, d_bw = G.empty((nf,), torch.int32), G.empty((nf,), torch.float64)
        d_mi, d_fl, d_psd = G.empty((nf,), torch.float32), G.empty((nf,), torch.float32), G.empty((nf, 1024), torch.float32)
        e.classify(G.dev(iq.view(np.float32).reshape(nf, n, 2)), nf, n, fs, d_lab, d_bw, d_mi, d_fl, d_psd)
        e.sync()
        lab, bw, mi, fl, psd = (a.cpu().numpy() for a in (d_lab, d_bw, d_mi, d_fl, d_psd))
        for f in range(nf):
            olab, obw, omi, ofl, opsd = O.classify(iq[f], fs)
            assert O.CLASS_LABELS[lab[f]] == olab and bw[f] == obw, (n, f)
            assert mi[f].tobytes() == omi.tobytes(), (n, f, mi[f], omi)
            assert abs(float(fl[f]) - float(ofl)) <= 1e-5 * abs(float(ofl)), (n, f)
            assert np.all(np.abs(psd[f] - opsd) <= 1e-6 * (opsd + 1e-10)), (n, f)


def test_decoder_front_halves(golden):
    """The GPU front halves of the reference's decoders against what the reference computes at the same points:
    decode_morse's rise / fall indices (decoders.py:149-161) and the bit stream decode_aprs hands to its AX.25 framing
    (decoders.py:122-129: real part, / max|x| — on the device here —, decode_afsk); batched pss_morse_edges against the oracle.
    The bookkeeping behind these numbers is the reference's own code and is not mirrored."""
    import pyspecsdr_amd.decoders as D
    g = golden["decoders"]
    e = G.engine()
    for tag in g["mtags"]:
        x = g[f"m_iq_{tag}"]
        rise, fall = D.morse_edges(x)
        assert np.array_equal(rise, g[f"m_rise_{tag}"]) and np.array_equal(fall, g[f"m_fall_{tag}"]), tag
    for tag in g["atags"]:
        x, fs = g[f"a_x_{tag}"], float(g[f"a_fs_{tag}"])
        assert np.array_equal(D.afsk_bits(x, fs, normalise=True), g[f"a_bits_{tag}"]), tag
        xr = np.real(x) if np.iscomplexobj(x) else x
        bits = e.h_afsk_bits(xr / np.max(np.abs(xr)), fs, g[f"a_sos1200_{tag}"], g[f"a_sos2200_{tag}"])   # host-normalised
        assert np.array_equal(bits, g[f"a_bits_{tag}"]), tag
    # the normalisation kernel alone: IEEE division by the row maximum, NaN for a row of zeros
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((9, 4097)) * rng.uniform(1e-3, 1e3, (9, 1))
    rows[4] = 0.0
    d_y = G.empty(rows.shape, torch.float64)
    e.row_normalise(G.dev(rows), rows.shape[0], rows.shape[1], d_y)
    e.sync()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(G.host(d_y), rows / np.max(np.abs(rows), axis=1, keepdims=True), equal_nan=True)
    for thr in (-15.0, -33.3, -1.5):                             # any threshold (the reference's -20 is one precomputed cut): against the oracle
        r, f = e.h_morse_edges(g["m_iq_cq"], threshold_db=thr)
        wr, wf = O.morse_edges(g["m_iq_cq"], thr)
        assert np.array_equal(r, wr) and np.array_equal(f, wf), thr
    rng = np.random.default_rng(9)
    for nf, n in ((33, 5000), (7, 2), (4, 70001), (300, 777)):
        key = np.repeat(rng.integers(0, 2, (nf, n // 40 + 1)), 40, axis=1)[:, :n] * rng.uniform(0.05, 1.0, (nf, 1))
        iq = (key * np.exp(0.2j * np.arange(n)) + 10.0 ** rng.uniform(-4, -1, (nf, 1)) * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
        iq[nf // 2] = 0
        cap = n // 2 + 1
        d_r, d_f, d_c = G.empty((nf, cap), torch.int32), G.empty((nf, cap), torch.int32), G.empty((nf, 2), torch.int32)
        e.morse_edges(G.dev(iq.view(np.float32).reshape(nf, n, 2)), nf, n, cap, d_r, d_f, d_c)
        e.sync()
        r, f, c = G.host(d_r), G.host(d_f), G.host(d_c)
        for k in range(nf):
            orr, off = O.morse_edges(iq[k])
            assert c[k, 0] == len(orr) and c[k, 1] == len(off), (n, k)
            assert np.array_equal(r[k, :len(orr)], orr) and np.array_equal(f[k, :len(off)], off), (n, k)


def test_decoders_end_to_end_vs_reference(golden):
    """The reference's decoders from samples to message: decode_morse(IQ) -> (text, timing) — envelope mask and edges on
    the GPU (pss_morse_edges), timing / classes / table in the library's host code (pss_h_morse_decode) — and decode_aprs(audio) -> packets
    — normalisation + Bell-202 bit slicer on the GPU, AX.25 framing on the host (pss_h_ax25_frame) — against what the reference returned
    for the same buffers (decoders.npz).  'noise': the reference's own answer depends on its random kmeans start; checked for being a
    decode at all."""
    import json
    from pyspecsdr_amd import decoders as D
    import pyspecsdr_amd.signal_processing as sp
    g = golden["decoders"]
    for tag in g["mtags"]:
        text, tm = D.decode_morse(g[f"m_iq_{tag}"], float(g[f"m_fs_{tag}"]))
        got = np.array([float(tm["dot"]), float(tm["dash"]), float(tm["gap"])])
        if tag == "noise":
            assert len(text) >= 1 and 0 < got[0] < got[1]
            continue
        assert text == str(g[f"m_text_{tag}"]), tag
        assert np.array_equal(got.view(np.uint64), g[f"m_timing_{tag}"].view(np.uint64)), (tag, got)
    keep = sp.USE_SCIPY_DESIGNS
    try:
        for scipy_tables in (True, False):         # the host's SciPy tables injected / the library's own designers
            sp.USE_SCIPY_DESIGNS = scipy_tables
            for tag in g["atags"]:
                want = json.loads(str(g[f"a_packets_{tag}"]))
                assert D.decode_aprs(g[f"a_x_{tag}"], float(g[f"a_fs_{tag}"])) == want, (tag, scipy_tables)
                assert D.decode_afsk(np.real(g[f"a_x_{tag}"]) / np.max(np.abs(np.real(g[f"a_x_{tag}"]))), float(g[f"a_fs_{tag}"])) == [int(b) for b in g[f"a_bits_{tag}"]]
    finally:
        sp.USE_SCIPY_DESIGNS = keep


def test_round6_complex128_buffers_vs_reference_goldens(golden):
    """complex128 read buffers (tests/golden/c128.npz: what the reference returns for them — float64 from the first statement): the drop-in's
    compute_fft (float64 rows, 1e-9) and demodulate_am (float64 audio and int16 PCM bit for bit) through pyspecsdr_amd.signal_processing, the
    batched device entry points (pss_spectrum_db_c128 / pss_demod_am_c128) against the same vectors and the oracle, and no narrowing warning."""
    import warnings
    import pyspecsdr_amd.signal_processing as sp
    g = golden["c128"]
    e = G.engine()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # a narrowing warning would be an error here
        for t in g["tags"]:
            for k, x in enumerate(g[f"iq_{t}"]):
                n = len(x)
                a = sp.demodulate_am(x)
                assert a.shape == (n, 2) and a.dtype == np.float64
                assert np.array_equal(a[:, 0], g[f"audio_{t}"][k]) and np.array_equal(a[:, 1], a[:, 0]), (t, k)
                assert np.array_equal(np.int16(a * 32767)[:, 0], g[f"pcm_{t}"][k]), (t, k)
                if n >= 16 and (n & (n - 1)) == 0:
                    db = sp.compute_fft(x)
                    assert db.dtype == np.float64 and np.allclose(db, g[f"db_{t}"][k], rtol=1e-9, atol=1e-9), (t, k)
                # demodulate_ssb: int16 equal, float64 audio to 2e-14 (the register transforms of the hilbert() round trip; option "hilbert_exact": bit for bit)
                for lower in (True, False):
                    a = sp.demodulate_ssb(x, 48000.0, lower=lower)
                    assert a.shape == (n, 2) and a.dtype == np.float64 and np.array_equal(a[:, 0], a[:, 1])
                    assert np.allclose(a[:, 0], g[f"ssb_{t}"][k], rtol=0, atol=2e-14), (t, k)
                    assert np.array_equal(np.int16(a * 32767)[:, 0], g[f"ssbpcm_{t}"][k]), (t, k)
                if (n & (n - 1)) == 0 and n >= 256:
                    sp.get_engine().set_option("hilbert_exact", 1)        # (the drop-in module's own engine)
                    try:
                        assert np.array_equal(sp.demodulate_ssb(x, 48000.0)[:, 0], g[f"ssb_{t}"][k]), (t, k, "hilbert_exact")
                    finally:
                        sp.get_engine().set_option("hilbert_exact", 0)
                # measure_signal_power: the mean power from the device in float64, the scalar log10 by NumPy on the host — the reference's bits
                pw = sp.measure_signal_power(x)
                assert isinstance(pw, np.float64) and pw == g[f"pw_{t}"][k], (t, k)
                assert e.h_mean_power_c128(x) == g[f"mp_{t}"][k], (t, k)
        with np.errstate(all="ignore"):
            z = g["iq_z"][0]
            assert np.array_equal(sp.compute_fft(z), g["db_z"][0])
            assert np.all(np.isnan(sp.demodulate_am(z)))
    # batched device entry points: frames of a batch are independent; PCM = np.int16(audio * 32767), L = R
    t = "a"
    iq = g[f"iq_{t}"]
    nf, n = iq.shape
    big = np.tile(iq, (70, 1))
    d_iq = G.dev(big.view(np.float64).reshape(len(big), n, 2))
    d_db, d_au, d_pcm = G.empty((len(big), n), torch.float64), G.empty((len(big), n), torch.float64), G.empty((len(big), n, 2), torch.int16)
    e.spectrum_db_c128(d_iq, len(big), n, d_db)
    e.demod_am_c128(d_iq, len(big), n, d_pcm, d_au)
    e.sync()
    assert np.allclose(G.host(d_db)[-nf:], g[f"db_{t}"], rtol=1e-9, atol=1e-9)
    assert np.array_equal(G.host(d_au)[:nf], g[f"audio_{t}"]) and np.array_equal(G.host(d_au)[-nf:], g[f"audio_{t}"])
    assert np.array_equal(G.host(d_pcm)[-nf:, :, 0], g[f"pcm_{t}"]) and np.array_equal(G.host(d_pcm)[..., 0], G.host(d_pcm)[..., 1])
    d_pw = G.empty((len(big),), torch.float64)
    e.mean_power_c128(d_iq, len(big), n, d_pw)
    d_sau, d_spcm = G.empty((len(big), n), torch.float64), G.empty((len(big), n, 2), torch.int16)
    e.set_ssb_taps(48000.0, g["ssb_taps"])
    e.demod_ssb_c128(d_iq, len(big), n, 48000.0, d_spcm, d_sau)
    e.sync()
    assert np.allclose(G.host(d_sau)[-nf:], g[f"ssb_{t}"], rtol=0, atol=2e-14) and np.array_equal(G.host(d_spcm)[-nf:, :, 0], g[f"ssbpcm_{t}"])
    assert np.array_equal(G.host(d_spcm)[:nf], G.host(d_spcm)[-nf:]) and np.array_equal(G.host(d_spcm)[..., 0], G.host(d_spcm)[..., 1])
    assert np.array_equal(G.host(d_pw)[:nf], g[f"mp_{t}"]) and np.array_equal(G.host(d_pw)[-nf:], g[f"mp_{t}"])
    # random buffers of awkward lengths against the oracle (the pairwise tree's uneven splits, chunks of 8192)
    rng = np.random.default_rng(66)
    sos = g["am_sos"]
    for n in (1, 7, 8, 9, 127, 129, 1000, 8191, 8193, 20000):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (1.0 + 1e-9 * rng.standard_normal(n))
        with np.errstate(all="ignore"):
            want = O.demod_am_c128(x, sos)
            got = sp.demodulate_am(x)[:, 0]
        assert np.array_equal(got, want, equal_nan=True), n
        assert e.h_mean_power_c128(x) == O.mean_power_c128(x), n
        with np.errstate(all="ignore"):
            got = sp.demodulate_ssb(x, 48000.0)[:, 0]
            want = O.demod_ssb_c128(x, g["ssb_taps"])
        assert np.allclose(got, want, rtol=0, atol=2e-14, equal_nan=True) and np.array_equal(np.int16(np.nan_to_num(got) * 32767), np.int16(np.nan_to_num(want) * 32767)), n
    # demodulate_nfm at a decimation factor of ONE (target_rate above half the sample rate: nothing is dropped, n - 1 output samples)
    keep = sp.USE_SCIPY_DESIGNS
    try:
        for scipy_tables in (True, False):
            sp.USE_SCIPY_DESIGNS = scipy_tables
            sp._designed.clear()
            for t in g["q1_tags"]:
                fs, tr = float(g[f"n_fs_{t}"]), int(g[f"n_tr_{t}"])
                for k, x in enumerate(g[f"n_iq_{t}"]):
                    a = sp.demodulate_nfm(x, fs, tr)
                    assert a.shape == (len(x) - 1, 2) and np.array_equal(a[:, 0], g[f"n_audio_{t}"][k]), (t, k, scipy_tables)
                    assert np.array_equal(np.int16(a[:, 0] * 32767), g[f"n_pcm_{t}"][k]), (t, k)
            # demodulate_wfm at factor one: the decimate() stage is skipped (:152-155), the de-emphasised channels normalised as they are;
            # one buffer through the drop-in function, and a batch through the device entry point (the large-batch branch takes the plain kernels too)
            for t in g["wq1_tags"]:
                fs, tr = float(g[f"w_fs_{t}"]), int(g[f"w_tr_{t}"])
                for k, x in enumerate(g[f"w_iq_{t}"]):
                    a = sp.demodulate_wfm(x, fs, tr)
                    assert a.shape == (len(x) - 1, 2) and np.array_equal(a, g[f"w_audio_{t}"][k]), (t, k, scipy_tables)
                    assert np.array_equal(np.int16(a * 32767), g[f"w_pcm_{t}"][k]), (t, k)
                iq = g[f"w_iq_{t}"]
                big = np.tile(iq, (1500, 1))
                n = iq.shape[1]
                try:
                    e.set_target_rate(float(tr))
                    if scipy_tables:
                        e.set_wfm_filters(fs, g[f"w_lp_{t}"], g[f"w_pil_{t}"], g[f"w_lmr_{t}"], float(g[f"w_alpha_{t}"]))
                    d_pcm, d_au = G.empty((len(big), n - 1, 2), torch.int16), G.empty((len(big), n - 1, 2), torch.float64)
                    e.demod(L.MODE_WFM, G.dev(big), len(big), n, fs, d_pcm, d_au)
                    e.sync()
                    assert np.array_equal(G.host(d_au)[-2:], g[f"w_audio_{t}"]) and np.array_equal(G.host(d_pcm)[:2], g[f"w_pcm_{t}"]), (t, scipy_tables)
                finally:
                    e.set_target_rate(22050)
    finally:
        sp.USE_SCIPY_DESIGNS = keep
        sp._designed.clear()
    # the other functions still narrow a complex128 buffer (with the one-time warning)
    sp._warned_narrowing = False
    with pytest.warns(RuntimeWarning):
        sp.demodulate_nfm(g["iq_a"][0], 2.4e6)


def test_round5_arguments_vs_reference_goldens(golden):
    """The arguments the drop-in module used to refuse (tests/golden/args.npz, tools/make_goldens_round5.py): demodulate_nfm / demodulate_wfm
    with target_rate != 22050 (any decimation factor int(fs / target_rate)), decode_morse with threshold != -20, bandpass_filter on complex
    and 2-D input — through the reference-named functions of pyspecsdr_amd.signal_processing / .decoders, against what the reference returned."""
    import pyspecsdr_amd.signal_processing as sp
    from pyspecsdr_amd import decoders as D
    g = golden["args"]
    keep = sp.USE_SCIPY_DESIGNS
    try:
        for scipy_tables in (True, False):             # SciPy's own tables injected / the library's designers
            sp.USE_SCIPY_DESIGNS = scipy_tables
            sp._designed.clear()
            for t in g["rate_tags"]:
                fs, tr = float(g[f"fs_{t}"]), int(g[f"tr_{t}"])
                fn = sp.demodulate_nfm if str(t).startswith("n") else sp.demodulate_wfm
                for k, x in enumerate(g[f"iq_{t}"]):
                    a = fn(x, fs, tr)
                    assert a.shape == g[f"audio_{t}"][k].shape, (t, a.shape)
                    assert np.array_equal(a, g[f"audio_{t}"][k]), (t, scipy_tables)
                    assert np.array_equal(np.int16(a * 32767), g[f"pcm_{t}"][k]), t
            # a non-default rate never outlives the call that asked for it: straight after one, the int16 path that has no target_rate
            # argument (demodulate_pcm = demodulate_signal + write_to_pipe) and the batched host call give the default-rate goldens
            n = golden["nfm"]
            sp.demodulate_nfm(n["iq_a"][0], float(n["fs_a"]), 11025)
            assert sp._target_rate == float(sp.DEFAULT_SAMPLE_RATE)
            assert np.array_equal(sp.demodulate_pcm(n["iq_a"][0], float(n["fs_a"]), "NFM"), n["pcm_a"][0])
            assert np.array_equal(sp.demodulate_nfm(n["iq_a"][0], float(n["fs_a"]))[:, 0], n["audio_a"][0])
    finally:
        sp.USE_SCIPY_DESIGNS = keep
        sp._designed.clear()
        sp._set_target_rate(sp.DEFAULT_SAMPLE_RATE)
    # batched device entry point with the target rate set on the engine
    e = G.engine()
    t = "n2"
    fs, tr, iq = float(g[f"fs_{t}"]), float(g[f"tr_{t}"]), g[f"iq_{t}"]
    try:
        e.set_target_rate(tr)
        e.set_nfm_filters(fs, g[f"taps_{t}"], g[f"sos_{t}"], g[f"zi_{t}"])
        nf, n = iq.shape
        n_out = e.demod_out_len(L.MODE_NFM, n, fs)
        assert n_out == g[f"audio_{t}"].shape[1]
        big = np.tile(iq, (5000, 1))                    # 10 000 frames: the fused large-batch kernels
        for batch in (iq, big):
            d_pcm, d_au = G.empty((len(batch), n_out, 2), torch.int16), G.empty((len(batch), n_out), torch.float64)
            e.demod(L.MODE_NFM, G.dev(batch), len(batch), n, fs, d_pcm, d_au)
            e.sync()
            assert np.array_equal(G.host(d_au)[:nf], g[f"audio_{t}"][..., 0]) and np.array_equal(G.host(d_pcm)[:nf], g[f"pcm_{t}"])
            assert np.array_equal(G.host(d_pcm)[-nf:], g[f"pcm_{t}"])
    finally:
        e.set_target_rate(22050)
    for t in g["morse_tags"]:
        x, fs, thr = g[f"m_iq_{t}"], float(g[f"m_fs_{t}"]), float(g[f"m_thr_{t}"])
        r, f = D.morse_edges(x, thr)
        assert np.array_equal(r, g[f"m_rise_{t}"]) and np.array_equal(f, g[f"m_fall_{t}"]), t
        text, tm = D.decode_morse(x, fs, thr)
        got = np.array([float(tm["dot"]), float(tm["dash"]), float(tm["gap"])])
        if len(g[f"m_rise_{t}"]) < 40:                  # (the noisy cases: the reference's own answer hangs on its random kmeans start)
            assert text == str(g[f"m_text_{t}"]), (t, text)
            assert np.array_equal(got.view(np.uint64), g[f"m_timing_{t}"].view(np.uint64)), (t, got)
    for t in g["bandpass_tags"]:
        lo, hi, fs = [float(v) for v in g[f"b_args_{t}"]]
        y = sp.bandpass_filter(g[f"b_x_{t}"], lo, hi, fs)
        want = g[f"b_y_{t}"]
        assert y.dtype == want.dtype and y.shape == want.shape, (t, y.dtype, y.shape)
        assert np.array_equal(y, want), t


def test_kernel_timing_and_filter():
    """pss_kernel_times lists every launch; pss_timing_filter keeps one kernel's events only; results do not change."""
    eng = G.engine()
    nf, n, fs = 128, 1024, 2.4e6
    rng = np.random.default_rng(5)
    iq = torch.from_numpy((rng.standard_normal((nf, n, 2)) * 0.3).astype(np.float32)).cuda()
    db = torch.empty((nf, n), dtype=torch.float32, device="cuda")
    pcm = torch.empty((nf, eng.demod_out_len(L.MODE_NFM, n, fs), 2), dtype=torch.int16, device="cuda")
    eng.set_option("small_batch", 0)
    try:
        eng.spectrum_nfm(iq, nf, n, fs, db, pcm); eng.sync()
        want = (db.clone(), pcm.clone())
        eng.enable_timing(True)
        eng.spectrum_nfm(iq, nf, n, fs, db, pcm); eng.sync()
        every = eng.kernel_times()
        assert {"k_nfm_fwd", "k_nfm_bwd", "k_spectrum"} <= set(every) and all(v[0] > 0 for v in every.values())
        assert eng.last_kernel_ms() > 0
        eng.timing_filter("k_nfm_fwd")
        for _ in range(3):
            eng.spectrum_nfm(iq, nf, n, fs, db, pcm)
        eng.sync()
        only = eng.kernel_times()
        assert list(only) == ["k_nfm_fwd"] and len(only["k_nfm_fwd"]) == 3 and min(only["k_nfm_fwd"]) > 0
        assert eng.last_kernel_ms() < 0
        eng.timing_filter(None)
        eng.spectrum_nfm(iq, nf, n, fs, db, pcm); eng.sync()
        assert set(eng.kernel_times()) == set(every)
        assert torch.equal(db, want[0]) and torch.equal(pcm, want[1])
    finally:
        eng.timing_filter(None)
        eng.enable_timing(False)
        eng.set_option("small_batch", 1)


def test_c_abi_from_plain_c(tmp_path):
    """examples/pss_example.c: the library used from C alone (no Python / torch in the process) gives what the shim gives."""
    import math, os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pss_example")
    subprocess.run(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "pss_example.c"),
                    "-L" + os.path.join(root, "pyspecsdr_amd"), "-lpss", "-lm", "-o", exe], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(root, "pyspecsdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, "1024", "2400000"], check=True, capture_output=True, text=True, env=env, timeout=120).stdout.split("\n")
    head = out[0].split()
    n, fs = 1024, 2.4e6
    ph = 0.0
    iq = np.empty(n, np.complex64)
    for i in range(n):
        ph += 2.0 * math.pi * 5e3 * math.sin(2.0 * math.pi * 1000.0 * i / fs) / fs
        iq[i] = np.float32(0.5 * math.cos(ph)) + 1j * np.float32(0.5 * math.sin(ph))
    import pyspecsdr_amd.signal_processing as sp
    db = sp.compute_fft(iq)
    assert int(head[3]) == 10 and int(head[7]) == int(np.argmax(db))
    assert abs(float(head[9]) - float(db.max())) < 1e-5 and abs(float(head[5]) - float(sp.measure_signal_power(iq))) < 1e-5
    sp.USE_SCIPY_DESIGNS, keep = False, sp.USE_SCIPY_DESIGNS     # the C program uses the library's native designers
    try:
        from pyspecsdr_amd.engine import Engine
        e2 = Engine(0)
        _, pcm = e2.h_demodulate(L.MODE_NFM, iq, fs)
        e2.close()
    finally:
        sp.USE_SCIPY_DESIGNS = keep
    assert [int(v) for v in out[1].split()[1:]] == [int(v) for v in pcm[:, 0]]


def _sweep_slices(start, count, n):
    """examples/pss_sweep_ranks.c's synthetic slices [start, start + count) as complex64 rows."""
    i = np.arange(n)
    rows = np.empty((count, n), np.complex64)
    for k in range(count):
        g = start + k
        f1, f2, a1 = (16 + (29 * g) % (n - 32)) / n, ((7 * g) % n) / n, 0.1 + 0.01 * (g % 50)
        rows[k] = ((a1 * np.cos(2 * np.pi * f1 * i) + 0.003 * np.cos(2 * np.pi * f2 * i)).astype(np.float32)
                   + 1j * (a1 * np.sin(2 * np.pi * f1 * i) + 0.003 * np.sin(2 * np.pi * f2 * i)).astype(np.float32))
    return rows


def _build_sweep_example(tmp_path):
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pss_sweep_ranks")
    subprocess.run(["gcc", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include"), "-I/opt/rocm/include",
                    os.path.join(root, "examples", "pss_sweep_ranks.c"), "-L" + os.path.join(root, "pyspecsdr_amd"), "-lpss",
                    "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-o", exe], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(root, "pyspecsdr_amd") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return exe, env


def _check_sweep_output(lines, n_slices, n):
    e = G.engine()
    d_iq = G.dev(_sweep_slices(0, n_slices, n))
    pk, bw, cnt = G.empty((n_slices,), torch.float32), G.empty((n_slices,), torch.float64), G.empty((n_slices,), torch.int32)
    e.scan(d_iq, n_slices, n, 2.4e6, None, pk, bw, cnt)
    e.sync()
    pk, bw, cnt = G.host(pk), G.host(bw), G.host(cnt)
    got = [ln.split() for ln in lines if ln.startswith("slice ")]
    assert [int(g[1]) for g in got] == list(range(n_slices)), "every slice once, in sweep order"
    for g in got:
        k = int(g[1])
        # (libm's and NumPy's cos / sin may round a sample differently: the peaks agree to 1e-4 dB, the counts exactly)
        assert abs(float(g[3]) - float(pk[k])) < 1e-4 and int(g[5]) == int(cnt[k]) and abs(float(g[7]) - float(bw[k])) < 1e-3
    return pk


def test_exchange_steps_behind_the_c_abi_one_rank():
    """pss_comm_* / pss_gather_packed / pss_halo_from_left through a REAL RCCL communicator of one rank (what one GPU can run), and the
    lone-rank mode that never opens librccl; EngineGroup routes shard.py's helpers through them."""
    from pyspecsdr_amd.engine import Engine
    from pyspecsdr_amd.shard import EngineGroup, ShardBuffer, gather_packed, halo_from_left
    e = Engine(0)
    try:
        assert e.comm_size() == (0, 1)
        src = torch.arange(5000, dtype=torch.int32, device="cuda").view(torch.uint8)
        for real in (False, True):
            e.comm_init(e.comm_id() if real else None, 0, 1)
            assert e.comm_size() == (0, 1)
            for dst in (0, None):
                out = torch.zeros_like(src)
                e.gather_packed(src, src.numel(), out, dst)
                e.sync()
                assert torch.equal(out, src)
            halo = torch.empty((4,), dtype=torch.float32, device="cuda")
            assert e.halo_from_left(src, [1250], 16, 4, halo) == 0
            with pytest.raises(Exception):
                e.gather_packed(src, src.numel(), out, 1)             # dst outside the communicator
            if real:
                with pytest.raises(Exception):
                    e.comm_init(e.comm_id(), 0, 1)                    # already joined
            grp = EngineGroup(e)
            assert (grp.rank, grp.world) == (0, 1)
            buf = ShardBuffer([("x", (3,), torch.float32)], 7, "cuda")
            buf.view("x")[:] = torch.arange(21, dtype=torch.float32, device="cuda").view(7, 3)
            assert torch.equal(gather_packed(buf, 7, dst=0, group=grp)["x"], buf.view("x"))
            assert halo_from_left(buf.view("x"), 3, group=grp).shape == (0, 3)
            e.comm_free()
        if torch.cuda.device_count() < 2:
            import warnings
            msg = ("NOT RUN: a communicator of more than one rank (EngineGroup's multi-rank branches, pss_comm.cpp's grouped send / recv): this box "
                   f"shows {torch.cuda.device_count()} GPU; test_exchange_steps_behind_the_c_abi_one_rank covered rank 0 of 1 only.")
            warnings.warn(msg)
            print("\n" + msg, flush=True)
    finally:
        e.close()


def test_sharded_sweep_from_plain_c(tmp_path):
    """examples/pss_sweep_ranks.c (no Python, no torch in the process): a one-rank RCCL communicator and the lone-rank mode give the
    single-GPU sweep; with two GPUs visible, two processes do (each on its own device, the gather and the halo over RCCL)."""
    import subprocess
    exe, env = _build_sweep_example(tmp_path)
    n_slices, n = 37, 4096
    outs = []
    for idf in ("-", str(tmp_path / "id1")):
        r = subprocess.run([exe, "0", "1", idf, str(n_slices), str(n)], check=True, capture_output=True, text=True, env=env, timeout=300)
        lines = [ln for ln in r.stdout.split("\n") if ln.startswith(("rank ", "slice "))]     # (RCCL prints a version banner of its own)
        assert lines[0].split()[:6] == ["rank", "0", "block", "0", str(n_slices), "halo"] and len(lines[0].split()) == 6
        _check_sweep_output(lines, n_slices, n)
        outs.append(lines)
    assert outs[0] == outs[1]
    if torch.cuda.device_count() < 2:
        import warnings
        msg = ("NOT RUN: the two-process branch of test_sharded_sweep_from_plain_c (pss_gather_packed's grouped send / recv and pss_halo_from_left "
               f"with a peer) needs 2 GPUs; this box shows {torch.cuda.device_count()}.  Only the one-rank communicator was exercised.")
        warnings.warn(msg)
        print("\n" + msg, flush=True)
        return
    idf = str(tmp_path / "id2")
    procs = [subprocess.Popen([exe, str(r), "2", idf, str(n_slices), str(n)], stdout=subprocess.PIPE, text=True, env=env) for r in (0, 1)]
    texts = [[ln for ln in p.communicate(timeout=600)[0].split("\n") if ln.startswith(("rank ", "slice "))] for p in procs]
    assert all(p.returncode == 0 for p in procs)
    pk = _check_sweep_output(texts[0], n_slices, n)
    head1 = texts[1][0].split()
    assert head1[:5] == ["rank", "1", "block", "19", "18"]
    assert np.allclose([float(v) for v in head1[6:]], pk[16:19], atol=1e-4)       # the three peaks before rank 1's block


def test_exchange_steps_with_real_peers_over_a_transport_double(tmp_path):
    """pss_gather_packed's grouped send / receive, its all-gather form, and pss_halo_from_left with one and with SEVERAL left neighbours, run by
    two / three / four real processes of examples/pss_sweep_ranks.c (plain C, no torch) on this box's one GPU.  RCCL itself refuses two ranks
    on one device, so the processes load tests/rccl_double/rccl_double.c in its place (PSS_RCCL_LIB; test infrastructure: RCCL's signatures and
    group / ordering semantics, messages as files + hipMemcpy).  What this covers that one rank cannot: pss_comm.cpp's per-peer offsets, which
    rows go to which neighbour, the order of posts inside a group.  What it does not: RCCL's own transport (xGMI) — no N > 1 timing."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, env = _build_sweep_example(tmp_path)
    dbl = str(tmp_path / "librccl_double.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(root, "tests", "rccl_double", "rccl_double.c"),
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", dbl], check=True)
    box = tmp_path / "mail"
    box.mkdir()
    env = dict(env, PSS_RCCL_LIB=dbl, PSS_RCCL_DOUBLE_DIR=str(box))
    n = 4096
    for world, n_slices in ((2, 37), (3, 37), (3, 5), (4, 6)):        # (3, 5): blocks 2 / 2 / 1, (4, 6): 2 / 2 / 1 / 1 — a halo of 3 spans two left neighbours
        idf = str(tmp_path / f"id_{world}_{n_slices}")
        procs = [subprocess.Popen([exe, str(r), str(world), idf, str(n_slices), str(n), "all"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
                 for r in range(world)]
        outs = [p.communicate(timeout=600) for p in procs]
        assert all(p.returncode == 0 for p in procs), [o[1][-500:] for o in outs]
        texts = [[ln for ln in o[0].split("\n") if ln.startswith(("rank ", "slice "))] for o in outs]
        pk = _check_sweep_output(texts[0], n_slices, n)              # rank 0's gathered sweep == the single-GPU sweep, slice for slice
        starts = [sum(((n_slices // world) + (1 if q < n_slices % world else 0)) for q in range(r)) for r in range(world + 1)]
        sums = []
        for r in range(world):
            head = [ln for ln in texts[r] if ln.startswith(f"rank {r} block")][0].split()
            assert head[:5] == ["rank", str(r), "block", str(starts[r]), str(starts[r + 1] - starts[r])], head
            want = pk[max(0, starts[r] - 3):starts[r]]                # the (at most three) peaks before this rank's block, whoever held them
            got = [float(v) for v in head[6:]]
            assert len(got) == len(want) and np.allclose(got, want, atol=1e-4), (world, n_slices, r, got, want)
            sums.append(float([ln for ln in texts[r] if "allgather" in ln][0].split()[3]))
        assert np.allclose(sums, float(np.sum(pk.astype(np.float64))), rtol=0, atol=2e-3) and len(set(sums)) == 1, (world, n_slices, sums)


def test_agc(golden):
    g = golden["caller"]
    e = G.engine()
    n = int(g["agc_ngains"])
    d_p = G.dev(g["agc_powers"])
    for start in (20, 0, n - 1):
        d_idx = G.empty((len(g["agc_powers"]),), torch.int32)
        e.agc_steps(d_p, len(g["agc_powers"]), start, n, d_idx)
        e.sync()
        assert list(G.host(d_idx)) == list(g[f"agc_traj_{start}"])
    # long series (the stepper composes chunk maps and scans them): random walks that hit both rails, dead-band readings, NaN / inf readings,
    # starting indices outside the table — against the oracle's sequential adjust_gain, for lengths around the kernel's chunking
    rng = np.random.default_rng(11)
    for length in (1, 2, 1023, 1024, 1025, 8192, 65536, 100003):
        for ng, start in ((29, 20), (3, 1), (1, 0), (29, 40), (29, -5)):
            p = (-30.0 + rng.choice([-40.0, -3.0, -1.5, 0.0, 1.5, 3.0, 40.0], size=length) + rng.standard_normal(length) * 0.4).astype(np.float32)
            p[rng.integers(0, length, size=max(1, length // 500))] = rng.choice([np.nan, np.inf, -np.inf])
            if length > 4000:
                p[length // 3:length // 3 + 700] = -80.0          # a long climb to the top rail, then a long fall to the bottom one
                p[length // 2:length // 2 + 900] = 20.0
            d_idx = G.empty((length,), torch.int32)
            e.agc_steps(G.dev(p), length, start, ng, d_idx)
            e.sync()
            idx, want = start, np.empty(length, np.int32)
            for i, v in enumerate(p):
                idx = O.agc_step(v, idx, ng)
                want[i] = idx
            assert np.array_equal(G.host(d_idx), want), (length, ng, start)


@pytest.mark.parametrize("n", [2048, 4096])
def test_scanner(golden, n):
    g = golden["scanner"]
    e = G.engine()
    iq = g[f"iq_{n}"]
    ns = iq.shape[0]
    d_db, d_pk = G.empty((ns, n), torch.float32), G.empty((ns,), torch.float32)
    d_bw, d_cnt = G.empty((ns,), torch.float64), G.empty((ns,), torch.int32)
    e.scan(G.dev(iq), ns, n, 2.4e6, d_db, d_pk, d_bw, d_cnt)
    e.sync()
    db, pk, bw, cnt = G.host(d_db), G.host(d_pk), G.host(d_bw), G.host(d_cnt)
    ref = g[f"db_{n}"]
    # every bit of the reference's float32 rows: np.fft.fft(complex64) is a double transform rounded to complex64 (NumPy 2.2), the
    # rest float32 arithmetic modelled exactly (scan_db_np) — so peak, 20-dB-down count and bandwidth are the reference's too
    assert np.array_equal(db.view(np.uint32), ref.view(np.uint32)), int((db.view(np.uint32) != ref.view(np.uint32)).sum())
    assert np.array_equal(pk.view(np.uint32), g[f"peak_{n}"].astype(np.float32).view(np.uint32))
    assert np.array_equal(cnt, g[f"count_{n}"].astype(cnt.dtype)) and np.array_equal(bw, g[f"bw_{n}"])
    for k in range(ns):
        assert pk[k] == db[k].max() and cnt[k] == int(np.sum(db[k] > pk[k] - np.float32(20)))  # self-consistent


def test_scanner_rows_equal_the_oracle_on_every_kernel_family():
    """The scanner's float32 dB rows on the other transform kernels (tiny frames and 8192 / 16384 on the generic kernel, 256 .. 1024
    on the register kernel, a Bluestein length): device == oracle bit for bit — the oracle's rows are the reference's (goldens,
    503 744 fuzzed values)."""
    rng = np.random.default_rng(88)
    e = G.engine()
    diff = total = 0
    for ns, n in ((40, 64), (33, 256), (33, 1024), (5, 8192), (3, 16384), (4, 3000)):
        t = np.arange(n)
        iq = (0.05 * (rng.standard_normal((ns, n)) + 1j * rng.standard_normal((ns, n))) +
              0.5 * np.exp(2j * np.pi * rng.uniform(-0.4, 0.4, (ns, 1)) * t)).astype(np.complex64)
        d_db, d_pk = G.empty((ns, n), torch.float32), G.empty((ns,), torch.float32)
        d_bw, d_cnt = G.empty((ns,), torch.float64), G.empty((ns,), torch.int32)
        e.scan(G.dev(iq), ns, n, 2.4e6, d_db, d_pk, d_bw, d_cnt)
        e.sync()
        db, pk, cnt = G.host(d_db), G.host(d_pk), G.host(d_cnt)
        for k in range(ns):
            odb, opk, obw, ocnt = O.scan_slice(iq[k], 2.4e6)
            ulp = np.abs(db[k].view(np.int32).astype(np.int64) - odb.view(np.int32).astype(np.int64))
            # two float64 transforms (this kernel's, the oracle's) agree to ~1e-16 of the LARGEST bin: a weak bin next to a strong
            # carrier can land on the other side of a float32 rounding boundary (measured here: 1 value of 130 000)
            diff += int((ulp != 0).sum())
            total += n
            assert ulp.max() <= 2, (n, k)       # one float32 ulp in a component moves the dB value by up to two
            assert pk[k].tobytes() == np.float32(opk).tobytes() and int(cnt[k]) == ocnt, (n, k)
    assert diff <= 3, (diff, total)


def test_lengths_that_are_not_a_power_of_two(golden):
    """Bluestein path: compute_fft (shim and batched entry), pss_scan and the sweep driver's pss_scan_threshold on lengths
    that are not a power of two, against the reference's goldens and against the oracle on random batches."""
    import pyspecsdr_amd.signal_processing as sp
    e = G.engine()
    g = golden["spectrum"]
    for n in g["np2_sizes"]:
        iq, ref = g[f"iq_np2_{n}"], g[f"db_np2_{n}"]
        db = G.spectrum(iq)
        big = np.abs(ref) > 1e-2
        assert np.all(rel_err(db, ref)[big] <= 1e-4) and np.all(np.abs(db - ref)[~big] <= 1e-6), n
        one = sp.compute_fft(iq[0])
        assert one.dtype == np.float64 and one.flags.writeable and np.array_equal(one.astype(np.float32), db[0])
    g = golden["scanner"]
    for n in g["sw_sizes"]:
        fs, thr = (float(v) for v in g[f"sw_args_{n}"])
        iq = g[f"sw_iq_{n}"]
        ns = iq.shape[0]
        d_db, d_pk = G.empty((ns, n), torch.float32), G.empty((ns,), torch.float32)
        d_bw, d_cnt = G.empty((ns,), torch.float64), G.empty((ns,), torch.int32)
        e.scan_threshold(G.dev(iq), ns, n, fs, thr, d_db, d_pk, d_bw, d_cnt)
        e.sync()
        db, pk, bw, cnt = G.host(d_db), G.host(d_pk), G.host(d_bw), G.host(d_cnt)
        ref = g[f"sw_db_{n}"]
        assert np.array_equal(db.view(np.uint32), ref.view(np.uint32)), (n, int((db.view(np.uint32) != ref.view(np.uint32)).sum()))
        assert np.array_equal(pk.view(np.uint32), g[f"sw_peak_{n}"].astype(np.float32).view(np.uint32)), n
        assert np.array_equal(cnt, g[f"sw_count_{n}"].astype(cnt.dtype)) and np.array_equal(bw, g[f"sw_bw_{n}"]), n
        for k in range(ns):
            assert bw[k] == cnt[k] * (fs / n) and pk[k] == db[k].max() and cnt[k] == int(np.sum(db[k] > np.float32(thr)))
        # the per-read numbers alone (no dB rows handed back) are the same numbers
        d_pk2, d_cnt2 = G.empty((ns,), torch.float32), G.empty((ns,), torch.int32)
        e.scan_threshold(G.dev(iq), ns, n, fs, thr, None, d_pk2, None, d_cnt2)
        e.sync()
        assert np.array_equal(G.host(d_pk2), pk) and np.array_equal(G.host(d_cnt2), cnt)
    rng = np.random.default_rng(23)
    for nf, n in ((5, 240000), (9, 1000), (3, 65537), (2, 524288), (4, 3)):
        iq = (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))).astype(np.complex64) * 0.2
        iq[:, : n // 2] += (0.4 * np.exp(2j * np.pi * 0.123 * np.arange(n // 2))).astype(np.complex64)
        db = G.spectrum(iq)
        d_db, d_pk = G.empty((nf, n), torch.float32), G.empty((nf,), torch.float32)
        d_bw, d_cnt = G.empty((nf,), torch.float64), G.empty((nf,), torch.int32)
        e.scan(G.dev(iq), nf, n, 2.4e6, d_db, d_pk, d_bw, d_cnt)
        e.sync()
        sdb, pk, cnt = G.host(d_db), G.host(d_pk), G.host(d_cnt)
        for k in (0, nf - 1):
            o = O.compute_fft(iq[k])
            assert np.all(np.abs(db[k] - o) <= 1e-4 * np.maximum(np.abs(o), 1e-2)), (n, k)
            odb, opk, obw, ocnt = O.scan_slice(iq[k], 2.4e6)
            assert np.all(np.abs(sdb[k] - odb) <= 1e-4 * np.maximum(np.abs(odb), 1.0)), (n, k)
            near = int(np.sum(np.abs(odb - (opk - 20)) < 2e-3))
            assert abs(float(pk[k]) - float(opk)) <= 1e-4 * abs(float(opk)) and abs(int(cnt[k]) - ocnt) <= near, (n, k)


def test_waterfall_and_persistence_cells(golden):
    g = golden["caller"]
    e = G.engine()
    rows = g["rows"]
    H, W = [int(v) for v in g["hw"]]
    dh, dw = H - 4, W - 8
    for i in (0, 1, 5, 29, 30, 33):
        ring = np.ascontiguousarray(rows[max(0, i + 1 - 30):i + 1])
        d_g, d_c = G.empty((dh, dw), torch.int8), G.empty((dh, dw), torch.int8)
        e.waterfall_cells(G.dev(ring), ring.shape[0], ring.shape[1], dh, dw, d_g, d_c, f64=True)
        e.sync()
        assert np.array_equal(G.host(d_g), g["wf_glyph"][i]) and np.array_equal(G.host(d_c), g["wf_colour"][i])
    for i in (0, 3, 9, 10, 13):
        ring = np.ascontiguousarray(rows[max(0, i + 1 - 10):i + 1])
        d_c = G.empty((dh, dw), torch.int8)
        e.persistence_cells(G.dev(ring), ring.shape[0], ring.shape[1], dh, dw, d_c, f64=True)
        e.sync()
        assert np.array_equal(G.host(d_c), g["ps_colour"][i])
    # float32 rows (what the GPU pipeline itself produces): cells may differ only where a value sits on a
    # quantisation edge
    ring = np.ascontiguousarray(rows[:30])
    d_g, d_c = G.empty((dh, dw), torch.int8), G.empty((dh, dw), torch.int8)
    e.waterfall_cells(G.dev(ring.astype(np.float32)), 30, ring.shape[1], dh, dw, d_g, d_c)
    e.sync()
    assert np.mean(G.host(d_g) != g["wf_glyph"][29]) < 1e-3


def test_ring_accumulators_follow_the_reference_history(golden):
    # push the caller's rows one by one into 30- and 10-deep device rings; after every push the cells must equal the
    # stateless quantiser on the same window (which test_waterfall_and_persistence_cells pins to the reference)
    g = golden["caller"]
    e = G.engine()
    rows = g["rows"].astype(np.float32)
    H, W = [int(v) for v in g["hw"]]
    dh, dw = H - 4, W - 8
    wf, ps = e.ring_create(30, rows.shape[1]), e.ring_create(10, rows.shape[1])
    d_rows = G.dev(rows)
    for i in range(len(rows)):
        e.ring_push(wf, d_rows[i]); e.ring_push(ps, d_rows[i])
        if i in (0, 4, 9, 10, 11, 29, 30, 33):
            a_g, a_c, b_c = (G.empty((dh, dw), torch.int8) for _ in range(3))
            e.ring_waterfall(wf, dh, dw, a_g, a_c)
            e.ring_persistence(ps, dh, dw, b_c)
            w0, p0 = max(0, i + 1 - 30), max(0, i + 1 - 10)
            r_g, r_c, q_c = (G.empty((dh, dw), torch.int8) for _ in range(3))
            e.waterfall_cells(d_rows[w0:i + 1].contiguous(), i + 1 - w0, rows.shape[1], dh, dw, r_g, r_c)
            e.persistence_cells(d_rows[p0:i + 1].contiguous(), i + 1 - p0, rows.shape[1], dh, dw, q_c)
            e.sync()
            assert torch.equal(a_g, r_g) and torch.equal(a_c, r_c) and torch.equal(b_c, q_c), i
    e.ring_destroy(wf); e.ring_destroy(ps)


def test_dropin_module_matches_reference_signatures(golden):
    import pyspecsdr_amd.signal_processing as sp
    g = golden["nfm"]
    x = g["iq_a"][0]
    a = sp.demodulate_signal(x, 2.4e6, "NFM")
    assert a.dtype == np.float64 and a.shape == (10, 2) and np.array_equal(a[:, 0], a[:, 1])
    assert np.allclose(a[:, 0], g["audio_a"][0], rtol=0, atol=1e-9)
    assert np.array_equal(sp.demodulate_pcm(x, 2.4e6, "NFM"), g["pcm_a"][0])
    db = sp.compute_fft(x)
    assert db.dtype == np.float64 and db.shape == (1024,) and db.flags.writeable
    s = golden["spectrum"]
    db = sp.compute_fft(s["iq_1024"][0])
    assert np.all(np.abs(db - s["db_1024"][0]) <= 1e-4 * np.abs(s["db_1024"][0]))
    p = sp.measure_signal_power(x)
    assert isinstance(p, np.float32)
    am = golden["am_ssb"]
    assert np.array_equal(sp.demodulate_signal(am["am_iq_a"][0], 2.4e6, "AM")[:, 0], am["am_audio_a"][0])
    assert sp.demodulate_signal(x, 2.4e6, "DIGITAL").shape == (1024, 2)
    with pytest.raises(ValueError):
        sp.demodulate_nfm(x[:28], 2.4e6)


def test_spectrum_nfm_large_frames_two_streams():
    # N >= 8192: the spectrum kernel uses its own scratch while the demodulator's backward pass runs beside it
    e = G.engine()
    rng = np.random.default_rng(81)
    nf, n, fs = 130, 8192, 2.4e6
    iq = (0.4 * np.exp(2j * np.pi * np.cumsum(rng.standard_normal((nf, n)) * 0.03, axis=1)) +
          0.05 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
    d_iq = G.dev(iq)
    n_out = e.demod_out_len(L.MODE_NFM, n, fs)
    d_db, d_pcm = G.empty((nf, n), torch.float32), G.empty((nf, n_out, 2), torch.int16)
    for _ in range(3):
        e.spectrum_nfm(d_iq, nf, n, fs, d_db, d_pcm)
    e.sync()
    d_db2, d_pcm2 = G.empty((nf, n), torch.float32), G.empty((nf, n_out, 2), torch.int16)
    e.spectrum_db(d_iq, nf, n, d_db2); e.sync()
    e.demod(L.MODE_NFM, d_iq, nf, n, fs, d_pcm2, None); e.sync()
    assert torch.equal(d_db, d_db2) and torch.equal(d_pcm, d_pcm2)
    taps, sos, zi = e.nfm_filters(fs)
    assert np.array_equal(G.host(d_pcm[7]), O.pcm16_stereo(O.demod_nfm(iq[7], fs, taps, sos, zi)))
    ref = O.compute_fft(iq[7])
    assert np.all(np.abs(G.host(d_db[7]) - ref) <= 1e-4 * np.maximum(np.abs(ref), 1e-2))


def test_streamed_capture_equals_resident_batch():
    # BASELINE.json configs[4] shape in miniature: a host capture cut into 2048-pt frames @10 MS/s, streamed in
    # ragged chunks (pinned buffers, double-buffered) must equal the device-resident batched call bit for bit
    e = G.engine()
    rng = np.random.default_rng(80)
    nf, n, fs = 333, 2048, 10e6
    h_iq = e.pinned_empty((nf, n), np.complex64)
    h_iq[:] = (0.4 * np.exp(2j * np.pi * np.cumsum(rng.standard_normal((nf, n)) * 0.03, axis=1)) +
               0.05 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
    h_db = e.pinned_empty((nf, n), np.float32)
    n_out = e.demod_out_len(L.MODE_NFM, n, fs)
    h_pcm = e.pinned_empty((nf, n_out, 2), np.int16)
    e.stream_spectrum_nfm(h_iq, fs, 100, h_db, h_pcm)       # 100 + 100 + 100 + 33 frames
    d_db, d_pcm = G.empty((nf, n), torch.float32), G.empty((nf, n_out, 2), torch.int16)
    e.spectrum_nfm(G.dev(np.array(h_iq)), nf, n, fs, d_db, d_pcm)
    e.sync()
    assert np.array_equal(h_db, G.host(d_db)) and np.array_equal(h_pcm, G.host(d_pcm))
    _, pcm2 = e.stream_spectrum_nfm(np.array(h_iq), fs, 1000)  # pageable memory, single chunk, no dB rows
    assert np.array_equal(pcm2, h_pcm)
    for a in (h_iq, h_db, h_pcm):
        e.pinned_free(a)


def test_streamed_display_equals_resident_pipeline():
    """pss_h_stream_display_nfm (BASELINE configs[4]: pinned host capture in, display lines + PCM out, chunked, three
    streams) against the device-resident calls on the same frames; the display history crosses chunk boundaries, and a
    capture continued with a halo of row extremes equals the tail of the uninterrupted one."""
    e = G.engine()
    nf, n, fs = 1500, 2048, 10e6
    rng = np.random.default_rng(21)
    t = np.arange(n) / fs
    iq = (0.4 * np.exp(2j * np.pi * (2e5 * t[None, :] + rng.random((nf, 1)))) * (1 + 0.5 * rng.random((nf, 1)))
          + 0.03 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
    iq[700:760] *= 30.0                                     # a burst: the window extremes change across chunk boundaries
    h_iq = e.pinned_empty((nf, n), np.complex64)
    h_iq[:] = iq
    n_out = e.demod_out_len(0, n, fs)
    d_iq = G.dev(iq)
    d_db, d_pcm = G.empty((nf, n), torch.float32), G.empty((nf, n_out, 2), torch.int16)
    d_post, d_lo, d_hi = G.empty((nf, n - 4), torch.float32), G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
    e.set_option("small_batch", 0)
    try:
        e.spectrum_nfm(d_iq, nf, n, fs, d_db, d_pcm)
    finally:
        e.set_option("small_batch", 1)
    e.spectrum_post_extremes(d_db, nf, n, d_post, d_lo, d_hi)
    for mode, window in (("waterfall", 30), ("persistence", 10)):
        if mode == "waterfall":
            a, b = G.empty((nf, 112), torch.int8), G.empty((nf, 112), torch.int8)
            e.waterfall_rows(d_post, nf, n - 4, d_lo, d_hi, 112, a, b, window=window)
            e.sync()
            want = (G.host(a), G.host(b))
        else:
            a = G.empty((nf, 112), torch.int8)
            e.persistence_rows(d_post, nf, n - 4, d_lo, d_hi, 36, 112, a, window=window)
            e.sync()
            want = (G.host(a),)
        for chunk in (256, 7, 1500):
            if chunk == 7 and mode == "persistence":
                continue
            got = e.stream_display_nfm(h_iq, fs, chunk, mode=mode, want_db=(chunk == 256))
            assert all(np.array_equal(x, y) for x, y in zip(got["lines"], want)), \
                (mode, chunk, [(int((x != y).sum()), np.nonzero((x != y).any(axis=1))[0][:8].tolist()) for x, y in zip(got["lines"], want)])
            assert np.array_equal(got["pcm"], G.host(d_pcm)), (mode, chunk)
            assert np.array_equal(got["row_lo"], G.host(d_lo)) and np.array_equal(got["row_hi"], G.host(d_hi))
            if chunk == 256:
                assert np.array_equal(got["db"].view(np.uint32), G.host(d_db).view(np.uint32))
        # continuation: frames 900.. with the extremes of the window-1 rows before them as halo
        cut = 900
        h2 = e.pinned_empty((nf - cut, n), np.complex64)
        h2[:] = iq[cut:]
        lo, hi = G.host(d_lo), G.host(d_hi)
        got = e.stream_display_nfm(h2, fs, 200, mode=mode, halo=(lo[cut - (window - 1):cut], hi[cut - (window - 1):cut]))
        assert all(np.array_equal(x, y[cut:]) for x, y in zip(got["lines"], want)), mode
        e.pinned_free(h2)
    e.pinned_free(h_iq)


@pytest.mark.parametrize("mode,window", [("waterfall", 30), ("persistence", 10)])
def test_streamed_capture_full_display_grids(mode, window):
    """pss_h_stream_display_nfm_grids: besides the per-frame lines, the FULL screen after the last frame of every chunk — every line / trace
    of the history redrawn with the history's current extremes, as draw_waterfall / draw_persistence do on every frame (pyspecsdr.py:1342-1406,
    :1512-1564).  Chunks shorter and longer than the history, a ragged last chunk; against the oracle's grid functions (pinned to the
    reference's own draws by tests/test_oracle_golden.py) on the device's post-processed rows, and against the resident call
    pss_waterfall_cells / pss_persistence_cells on materialised rows."""
    e = G.engine()
    nf, n, fs = 230, 2048, 10e6
    H, W = 36, 112
    rng = np.random.default_rng(33)
    t = np.arange(n) / fs
    iq = (0.4 * np.exp(2j * np.pi * (3e5 * t[None, :] + rng.random((nf, 1)))) * (1 + 0.8 * rng.random((nf, 1)))
          + 0.03 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
    iq[100:105] *= 25.0
    d_iq = G.dev(iq)
    d_db, d_post = G.empty((nf, n), torch.float32), G.empty((nf, n - 4), torch.float32)
    e.spectrum_db(d_iq, nf, n, d_db)
    e.spectrum_post(d_db, nf, n, d_post)
    e.sync()
    post = G.host(d_post)
    for chunk in (7, 64, 100):
        got = e.stream_display_nfm_grids(iq, fs, chunk, mode=mode, window=window, disp_h=H, disp_w=W)
        plain = e.stream_display_nfm(iq, fs, chunk, mode=mode, window=window, disp_h=H, disp_w=W)
        assert all(np.array_equal(a, b) for a, b in zip(got["lines"], plain["lines"])) and np.array_equal(got["pcm"], plain["pcm"])
        n_chunks = (nf + chunk - 1) // chunk
        assert got["grids"][0].shape == (n_chunks, H, W)
        for k in range(n_chunks):
            last = min(nf, (k + 1) * chunk) - 1
            rows = post[max(0, last + 1 - window):last + 1]
            if mode == "waterfall":
                wg, wc = O.waterfall_cells(rows.astype(np.float64), H, W)
                assert np.array_equal(got["grids"][0][k], wg) and np.array_equal(got["grids"][1][k], wc), (chunk, k)
                d_g, d_c = G.empty((H, W), torch.int8), G.empty((H, W), torch.int8)
                e.waterfall_cells(d_post[max(0, last + 1 - window):last + 1], len(rows), n - 4, H, W, d_g, d_c)
                e.sync()
                assert np.array_equal(G.host(d_g), got["grids"][0][k]) and np.array_equal(G.host(d_c), got["grids"][1][k])
            else:
                assert np.array_equal(got["grids"][0][k], O.persistence_cells(rows.astype(np.float64), H, W)), (chunk, k)


def test_frame_pipeline_equals_separate_calls():
    """pss_frame_pipeline_nfm (what bench.py times: one main-loop iteration per frame of the batch, display chain on a side
    stream beside the demodulator's backward pass) against the separate entry points, byte for byte."""
    e = G.engine()
    gen = torch.Generator(device="cuda").manual_seed(77)
    for nf, n, fs in ((9000, 1024, 2.4e6), (300, 2048, 10e6)):
        iq = torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3
        torch.cuda.synchronize()
        n_out = e.demod_out_len(0, n, fs)
        def bufs():
            return dict(db=G.empty((nf, n), torch.float32), post=G.empty((nf, n - 4), torch.float32), lo=G.empty((nf,), torch.float32),
                        hi=G.empty((nf,), torch.float32), g=G.empty((nf, 112), torch.int8), c=G.empty((nf, 112), torch.int8),
                        pcm=G.empty((nf, n_out, 2), torch.int16))
        a, b = bufs(), bufs()
        e.frame_pipeline_nfm(iq, nf, n, fs, a["db"], a["post"], a["lo"], a["hi"], 112, a["g"], a["c"], a["pcm"])
        e.spectrum_nfm(iq, nf, n, fs, b["db"], b["pcm"])
        e.spectrum_post_extremes(b["db"], nf, n, b["post"], b["lo"], b["hi"])
        e.waterfall_rows(b["post"], nf, n - 4, b["lo"], b["hi"], 112, b["g"], b["c"])
        e.sync()
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (nf, k)
        # compute_fft + post-process in one call against the separate entry points
        c = bufs()
        e.spectrum_db_post(iq, nf, n, c["db"], c["post"], c["lo"], c["hi"])
        e.sync()
        for k in ("db", "post", "lo", "hi"):
            assert torch.equal(c[k].view(torch.uint8), b[k].view(torch.uint8)), (nf, k)


@pytest.mark.parametrize("mode", [L.MODE_NFM, L.MODE_WFM, L.MODE_AM, L.MODE_USB, L.MODE_LSB])
@pytest.mark.parametrize("display", ["waterfall", "persistence"])
def test_frame_pipeline_modes_equal_separate_calls(mode, display):
    """pss_frame_pipeline: the main-loop iteration (pyspecsdr.py:2262-2283 + the draw) in every mode demodulate_signal serves — WFM, the
    reference's default (:2855), through the dispatcher's iq_correction — and for both batched accumulators, against the separate entry
    points byte for byte; with materialised post-processed rows and without; small batches (systolic kernels) and large ones."""
    e = G.engine()
    gen = torch.Generator(device="cuda").manual_seed(123 + mode)
    # 32 768 (the reference's default read, pyspecsdr.py:2236) and 65 536 samples: hilbert() of USB / LSB frames and the side stream's
    # spectrum both take their scratch-based kernels there — each has its own scratch buffer (they once shared ctx->scratch_fft)
    shapes = ((7000, 1024, 2.4e6), (40, 8192, 2.4e6)) if mode in (L.MODE_NFM, L.MODE_WFM) else ((600, 1024, 2.4e6), (33, 8192, 2.4e6), (9, 16384, 2.4e6),
                                                                                                  (5, 32768, 2.4e6), (3, 65536, 2.4e6), (2, 131072, 2.4e6))
    for nf, n, fs in shapes:
        iq = torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3 + 0.05
        torch.cuda.synchronize()
        n_out = e.demod_out_len(mode, n, fs)
        H, W = 36, 112

        def bufs():
            return dict(db=G.empty((nf, n), torch.float32), post=G.empty((nf, n - 4), torch.float32), lo=G.empty((nf,), torch.float32),
                        hi=G.empty((nf,), torch.float32), a=G.empty((nf, W), torch.int8), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"),
                        pcm=G.empty((nf, n_out, 2), torch.int16))
        x, y, z = bufs(), bufs(), bufs()
        torch.cuda.synchronize()
        e.frame_pipeline(mode, iq, nf, n, fs, x["db"], x["post"], x["lo"], x["hi"], W, x["a"], x["b"], x["pcm"], display=display, disp_h=H)
        e.frame_pipeline(mode, iq, nf, n, fs, z["db"], None, z["lo"], z["hi"], W, z["a"], z["b"], z["pcm"], display=display, disp_h=H)
        e.demod_signal(mode, iq, nf, n, fs, y["pcm"], None)
        e.spectrum_db(iq, nf, n, y["db"])
        e.spectrum_post_extremes(y["db"], nf, n, y["post"], y["lo"], y["hi"])
        if display == "waterfall":
            e.waterfall_rows(y["post"], nf, n - 4, y["lo"], y["hi"], W, y["a"], y["b"])
        else:
            e.persistence_rows(y["post"], nf, n - 4, y["lo"], y["hi"], H, W, y["a"])
        e.sync()
        for k in x:
            assert torch.equal(x[k].view(torch.uint8), y[k].view(torch.uint8)), (mode, display, nf, n, k)
            if k != "post":
                assert torch.equal(z[k].view(torch.uint8), y[k].view(torch.uint8)), (mode, display, nf, n, k, "rows not materialised")
    # argument errors come back as errors, before any allocation or launch (n_halo < 0, frames too short for a post-processed row)
    from pyspecsdr_amd.engine import PssError
    with pytest.raises(PssError):
        e.frame_pipeline(mode, iq, 1, 1024, 2.4e6, x["db"], None, x["lo"], x["hi"], W, x["a"], x["b"], x["pcm"], n_halo=-1)
    with pytest.raises(PssError):
        e.frame_pipeline(mode, iq, 1, 3, 2.4e6, x["db"], None, x["lo"], x["hi"], W, x["a"], x["b"], x["pcm"])


def test_calls_are_ordered_against_the_callers_stream_without_a_synchronize():
    """The single-threaded call order of the reference's loop (pyspecsdr.py:2250-2283): fill a buffer, call, read the result — with the fills and
    the reads on torch's stream and NO synchronize anywhere.  The library runs on its own non-blocking stream; Engine (order = "torch", the
    default) brackets every device entry point with pss_order_after / pss_order_before, so each call sees the input written just before it and
    torch sees the outputs right after it.  Two alternating inputs, 200 iterations, ten entry points; outputs pre-filled with a sentinel."""
    e = G.engine()
    assert e.order == "torch"
    nf, n, fs = 768, 1024, 2.4e6
    gen = torch.Generator(device="cuda").manual_seed(5)
    src = [torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32) * s + 0.01 for s in (0.3, 0.05)]
    n_out = e.demod_out_len(L.MODE_NFM, n, fs)
    W = 112

    def outputs():
        return dict(db=G.empty((nf, n), torch.float32), post=G.empty((nf, n - 4), torch.float32), thr=G.empty((nf,), torch.float32),
                    lo=G.empty((nf,), torch.float32), hi=G.empty((nf,), torch.float32), g=G.empty((nf, W), torch.int8), c=G.empty((nf, W), torch.int8),
                    pcm=G.empty((nf, n_out, 2), torch.int16), pcm_am=G.empty((nf, n, 2), torch.int16), pw=G.empty((nf,), torch.float32),
                    sdb=G.empty((nf, n), torch.float32), spk=G.empty((nf,), torch.float32), sbw=G.empty((nf,), torch.float64),
                    scnt=G.empty((nf,), torch.int32), corr=G.empty((nf, n, 2), torch.float32), g2=G.empty((nf, W), torch.int8),
                    c2=G.empty((nf, W), torch.int8), pdb=G.empty((nf, n), torch.float32), plo=G.empty((nf,), torch.float32),
                    phi=G.empty((nf,), torch.float32), ppcm=G.empty((nf, n_out, 2), torch.int16))

    def run(iq, o):
        e.spectrum_db(iq, nf, n, o["db"])
        e.spectrum_post_extremes(o["db"], nf, n, o["post"], o["lo"], o["hi"])
        e.spectrum_post_thresholds(o["db"], nf, n, o["thr"], o["lo"], o["hi"])
        e.waterfall_rows(o["post"], nf, n - 4, o["lo"], o["hi"], W, o["g"], o["c"])
        e.demod(L.MODE_NFM, iq, nf, n, fs, o["pcm"], None)
        e.demod(L.MODE_AM, iq, nf, n, fs, o["pcm_am"], None)
        e.power_db(iq, nf, n, o["pw"])
        e.scan(iq, nf, n, fs, o["sdb"], o["spk"], o["sbw"], o["scnt"])
        e.iq_correction(iq, nf, n, o["corr"], None)
        e.frame_pipeline_nfm(iq, nf, n, fs, o["pdb"], None, o["plo"], o["phi"], W, o["g2"], o["c2"], o["ppcm"])

    want = []
    for k in range(2):                       # expected outputs, produced with full synchronisation
        o = outputs()
        torch.cuda.synchronize()
        run(src[k], o)
        e.sync()
        torch.cuda.synchronize()
        want.append({key: v.clone() for key, v in o.items()})
    torch.cuda.synchronize()
    iq, o = torch.empty_like(src[0]), outputs()
    keys = list(o)
    mism = torch.zeros((200, len(keys)), dtype=torch.int32, device="cuda")     # filled on the device: no host round trip inside the loop
    for it in range(200):
        k = it & 1
        iq.copy_(src[k])                     # torch's stream, straight before the calls
        for v in o.values():
            v.fill_(0x55 if v.dtype in (torch.int8, torch.int16, torch.int32) else 1.0e30)
        run(iq, o)
        for j, key in enumerate(keys):       # torch's stream again, no e.sync(): the comparison kernels must see the results
            mism[it, j] = (o[key].view(torch.uint8) != want[k][key].view(torch.uint8)).any()
    bad = [(int(a), keys[int(b)]) for a, b in mism.nonzero().cpu().numpy()]
    assert not bad, bad[:10]


def test_full_size_headline_properties():
    """BASELINE.json cfg 2 size (65 536 x 1024) through pss_frame_pipeline_nfm — the call bench.py times: size-independent properties
    of every output (dB rows, post-processed rows, waterfall lines, PCM), an oracle spot check, and the variant that does not
    materialise the post-processed rows (d_post = NULL) byte for byte."""
    e = G.engine()
    nf, n, fs, W, win = 65536, 1024, 2.4e6, 112, 30
    gen = torch.Generator(device="cuda").manual_seed(1234)
    base = torch.randn((512, n, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.3
    iq = base.repeat(nf // 512, 1, 1).contiguous()            # every block of 512 frames repeats
    d_db, d_post = G.empty((nf, n), torch.float32), G.empty((nf, n - 4), torch.float32)
    d_lo, d_hi = G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
    d_g, d_c = G.empty((nf, W), torch.int8), G.empty((nf, W), torch.int8)
    d_pcm = G.empty((nf, 10, 2), torch.int16)
    e.frame_pipeline_nfm(iq, nf, n, fs, d_db, d_post, d_lo, d_hi, W, d_g, d_c, d_pcm, window=win)
    e.sync()
    R = nf // 512
    db, post, pcm = d_db.view(R, 512, n), d_post.view(R, 512, n - 4), d_pcm.view(R, 512, 10, 2)
    assert bool((db == db[0:1]).all()) and bool((pcm == pcm[0:1]).all()) and bool((post == post[0:1]).all())   # batch-position independence
    assert bool((d_lo.view(R, 512) == d_lo[:512]).all()) and bool((d_hi.view(R, 512) == d_hi[:512]).all())
    # a waterfall line depends on the 29 rows before it: from the second repeat on every line's history is periodic too
    g, c = d_g.view(R, 512, W), d_c.view(R, 512, W)
    assert bool((g[1:] == g[1:2]).all()) and bool((c[1:] == c[1:2]).all())
    assert bool((g[0, win - 1:] == g[1, win - 1:]).all()) and bool((c[0, win - 1:] == c[1, win - 1:]).all())   # first repeat: once its history is full
    assert bool((d_pcm[..., 0] == d_pcm[..., 1]).all())                       # L == R
    assert int(d_pcm.abs().max()) == 31128                                    # peak sample -> trunc(0.95*32767)
    assert bool((d_pcm.abs().amax(dim=(1, 2)) == 31128).all())                # in every frame
    # spot-check 64 frames of the big batch against the oracle: PCM, dB rows, post-processed rows, lines
    taps, sos, zi = e.nfm_filters(fs)
    h = base[:64].cpu().numpy().view(np.complex64).reshape(64, n)
    hp, hdb, hpost = d_pcm[:64].cpu().numpy(), d_db[:64].cpu().numpy(), np.ascontiguousarray(d_post[:64].cpu().numpy())
    for k in range(64):
        assert np.array_equal(hp[k], O.pcm16_stereo(O.demod_nfm(h[k], fs, taps, sos, zi)))
        ref = O.compute_fft(h[k])
        assert np.all(np.abs(hdb[k] - ref) <= 1e-4 * np.maximum(np.abs(ref), 1.0))
        rp = O.postprocess(hdb[k].astype(np.float64))
        assert np.all(np.abs(hpost[k] - rp) <= 1e-4 * np.maximum(np.abs(rp), 1.0))
    buf = O.HeadlineBuffers(64, n, fs, W)
    O.lib().pss_o_waterfall_rows(hpost.reshape(-1), 64, n - 4, win, W, buf.glyph.reshape(-1), buf.colour.reshape(-1), 1)
    assert np.array_equal(d_g[:64].cpu().numpy(), buf.glyph) and np.array_equal(d_c[:64].cpu().numpy(), buf.colour)
    # the same step without materialised post-processed rows
    d_g2, d_c2, d_lo2, d_hi2 = G.empty((nf, W), torch.int8), G.empty((nf, W), torch.int8), G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
    d_pcm2 = G.empty((nf, 10, 2), torch.int16)
    d_db2 = G.empty((nf, n), torch.float32)
    e.frame_pipeline_nfm(iq, nf, n, fs, d_db2, None, d_lo2, d_hi2, W, d_g2, d_c2, d_pcm2, window=win)
    e.sync()
    for a, b in ((d_g, d_g2), (d_c, d_c2), (d_lo, d_lo2), (d_hi, d_hi2), (d_pcm, d_pcm2), (d_db, d_db2)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("nf,n,fs", [(96, 32768, 1.024e6), (12, 32768, 2.4e6), (300, 8192, 2.4e6)])
def test_frame_pipeline_at_the_reference_read_buffer_size(nf, n, fs):
    """The main loop reads 32 768 samples per iteration by default (pyspecsdr.py:2236; 8 192 .. 1 048 576): the pipeline call at that
    frame length against the separate entry points byte for byte, against the oracle on a few frames, with and without
    materialised post-processed rows (small and large batches: both NFM kernel families)."""
    e = G.engine()
    W = 112
    gen = torch.Generator(device="cuda").manual_seed(n + nf)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / fs
    ph = 2 * np.pi * 4e3 * torch.cumsum(torch.sin(2 * np.pi * 700 * t).unsqueeze(0) * torch.linspace(0.2, 1.0, nf, device="cuda", dtype=torch.float64).unsqueeze(1), dim=1) / fs
    iq = torch.stack([0.4 * torch.cos(ph), 0.4 * torch.sin(ph)], dim=-1).float() + 0.03 * torch.randn((nf, n, 2), generator=gen, device="cuda")
    iq = iq.contiguous()
    torch.cuda.synchronize()
    n_out = e.demod_out_len(0, n, fs)
    def bufs():
        return dict(db=G.empty((nf, n), torch.float32), post=G.empty((nf, n - 4), torch.float32), lo=G.empty((nf,), torch.float32),
                    hi=G.empty((nf,), torch.float32), g=G.empty((nf, W), torch.int8), c=G.empty((nf, W), torch.int8),
                    pcm=G.empty((nf, n_out, 2), torch.int16))
    a, b, c = bufs(), bufs(), bufs()
    e.frame_pipeline_nfm(iq, nf, n, fs, a["db"], a["post"], a["lo"], a["hi"], W, a["g"], a["c"], a["pcm"])
    e.spectrum_nfm(iq, nf, n, fs, b["db"], b["pcm"])
    e.spectrum_post_extremes(b["db"], nf, n, b["post"], b["lo"], b["hi"])
    e.waterfall_rows(b["post"], nf, n - 4, b["lo"], b["hi"], W, b["g"], b["c"])
    e.frame_pipeline_nfm(iq, nf, n, fs, c["db"], None, c["lo"], c["hi"], W, c["g"], c["c"], c["pcm"])
    e.sync()
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (nf, n, k)
        if k != "post":
            assert torch.equal(a[k].view(torch.uint8), c[k].view(torch.uint8)), (nf, n, k, "no materialised rows")
    taps, sos, zi = e.nfm_filters(fs)
    h = iq.cpu().numpy().view(np.complex64).reshape(nf, n)
    want = O.map_frames(lambda x: (O.pcm16_stereo(O.demod_nfm(x, fs, taps, sos, zi)), O.compute_fft(x)), h)     # every frame
    pcm, db = a["pcm"].cpu().numpy(), a["db"].cpu().numpy()
    bad = [k for k in range(nf) if not np.array_equal(pcm[k], want[k][0])]
    assert not bad, (n, bad[:16])
    bad = [k for k in range(nf) if not np.all(np.abs(db[k] - want[k][1]) <= 1e-4 * np.maximum(np.abs(want[k][1]), 1.0))]
    assert not bad, (n, bad[:16])


@pytest.mark.parametrize("n", [256, 1024, 2048, 4096, 16384])
def test_display_lines_without_materialised_rows(n):
    """pss_spectrum_post_thresholds + pss_waterfall_rows_db / pss_persistence_rows_db (the post-processed rows are never written: 12 bytes
    per row instead of 4 (n - 4)) against the materialised path, byte for byte — ties, a constant row, non-finite values, a halo."""
    rng = np.random.default_rng(n)
    nf, W, H = 75, 112, 36
    db = (rng.standard_normal((nf, n)) * 6.0 - 35.0).astype(np.float32)
    db[0, : n // 2] = np.round(db[0, : n // 2])
    db[1] = -42.5
    db[2, 100:140] += 50.0
    db[3, 10:20] = np.inf
    db[4, 30] = np.nan
    e = G.engine()
    d_db = G.dev(db)
    halo = 7
    lo, hi = G.empty((halo + nf,), torch.float32), G.empty((halo + nf,), torch.float32)
    lo[:halo] = torch.tensor(rng.uniform(-60, -50, halo).astype(np.float32)); hi[:halo] = torch.tensor(rng.uniform(-20, -5, halo).astype(np.float32))
    lo2, hi2 = lo.clone(), hi.clone()
    d_post, d_thr = G.empty((nf, n - 4), torch.float32), G.empty((nf,), torch.float32)
    e.spectrum_post_extremes(d_db, nf, n, d_post, lo[halo:], hi[halo:])
    e.spectrum_post_thresholds(d_db, nf, n, d_thr, lo2[halo:], hi2[halo:])
    e.sync()
    assert torch.equal(lo.view(torch.int32), lo2.view(torch.int32)) and torch.equal(hi.view(torch.int32), hi2.view(torch.int32))
    post, thr = G.host(d_post), G.host(d_thr)
    for f in (0, 2, nf - 1):
        sm = np.convolve(db[f].astype(np.float64), np.ones(5) / 5, mode="valid").astype(np.float32)
        assert thr[f] == np.float32(np.median(sm).astype(np.float64) - 10.0) and thr[f] <= post[f].min(), (n, f)
    out = [[G.empty((nf, W), torch.int8) for _ in range(3)] for _ in range(2)]
    e.waterfall_rows(d_post, nf, n - 4, lo, hi, W, out[0][0], out[0][1], n_halo=halo, window=30)
    e.persistence_rows(d_post, nf, n - 4, lo, hi, H, W, out[0][2], n_halo=halo, window=10)
    e.waterfall_rows_db(d_db, nf, n, d_thr, lo2, hi2, W, out[1][0], out[1][1], n_halo=halo, window=30)
    e.persistence_rows_db(d_db, nf, n, d_thr, lo2, hi2, H, W, out[1][2], n_halo=halo, window=10)
    e.sync()
    for k in range(3):
        assert torch.equal(out[0][k], out[1][k]), (n, k)


@pytest.mark.gpu
def test_am_small_batch_array_at_group_and_block_edges():
    """k_am_grp (round 4): the AM band-pass as a group-systolic array — five section lanes per frame handing groups of eight samples on in
    registers, 64-sample blocks staged by two load wavefronts, a 128-sample output ring drained by a store wavefront 32 samples out of step
    with the blocks.  Frame lengths around every group / block / ring boundary, batches around the 12 frames of a wavefront and the lanes of
    its DPP rows, a silent frame (0 / 0 -> NaN audio, PCM 0) and leading zeros, against the oracle: float64 audio bits and int16 PCM."""
    rng = np.random.default_rng(404)
    e = G.engine()
    sos = np.empty((5, 6))
    e.lib.pss_am_bandpass_sos(sos.ctypes.data)
    for n in (1, 2, 7, 8, 9, 31, 32, 33, 39, 40, 41, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 1000, 4097):
        for nf in (1, 2, 3, 4, 11, 12, 13, 25):
            iq = (0.3 + 0.2 * rng.standard_normal((nf, n)) + 0.2j * rng.standard_normal((nf, n))).astype(np.complex64)
            if nf >= 3:
                iq[1] = 0                       # silence
                iq[2, : n // 2] = 0             # leading zeros, then signal
            pcm, audio = G.demod(L.MODE_AM, iq, 2.4e6)
            for f in range(nf):
                a = O.demod_am(iq[f], sos)
                fin = ~np.isnan(a)
                assert np.array_equal(np.isnan(audio[f]), ~fin), (n, nf, f)
                assert np.array_equal(audio[f][fin].view(np.uint64), a[fin].view(np.uint64)), (n, nf, f)    # bits: -0.0 is not +0.0 here
                assert np.array_equal(pcm[f], O.pcm16_stereo(a)), (n, nf, f)
    # a batch far beyond the CUs' capacity for resident workgroups (rounds 1-3 switched to a lane-per-frame kernel at 32 768 frames)
    nf, n = 70000, 300
    iq = (0.3 + 0.2 * rng.standard_normal((nf, n)) + 0.2j * rng.standard_normal((nf, n))).astype(np.complex64)
    pcm, audio = G.demod(L.MODE_AM, iq, 2.4e6)
    want = np.stack(O.map_frames(lambda x: O.demod_am(x, sos), iq))      # every frame
    bad = np.nonzero((audio.view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, bad[:16].tolist()
    bad = np.nonzero((pcm != np.stack([O.pcm16_stereo(a) for a in want])).reshape(nf, -1).any(axis=1))[0]
    assert bad.size == 0, bad[:16].tolist()



@pytest.mark.gpu
@pytest.mark.parametrize("small", [True, False])
def test_bench_other_configs_verify(small):
    """tools/bench_configs.py — what bench.py's `other_configs` runs after the headline — at a fraction of every batch and at the FULL
    BASELINE batches (cfg 3: 8192 x 16 384, cfg 4: 8192 x 4096, cfg 5: 48 828 x 2048 resident and streamed, WFM step: 65 536 x 1024): each
    config must time, carry its fields and pass its own oracle / resident-pipeline verification (cfg 3 on two contexts)."""
    import os as _os
    import sys as _sys
    root = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    _sys.path.insert(0, _os.path.join(root, "tools"))
    import bench_configs as BC
    from pyspecsdr_amd.engine import Engine
    eng = Engine(0, order="none")
    try:
        oc = BC.other_configs(eng, torch.device("cuda", 0), verify=True, small=small)
    finally:
        eng.close()
    assert set(oc) == {"cfg2_f32_rows", "cfg2_exact_cells", "cfg3", "cfg4", "cfg5_resident", "cfg5_streamed", "wfm_step"}
    assert oc["cfg2_exact_cells"]["verified"]["cells_differing"] == 0 and oc["cfg2_exact_cells"]["verified"]["rows"] == "float64"
    for name, e in oc.items():
        assert "error" not in e, (name, e.get("error"))
        assert e["verified"]["ok"], (name, e["verified"])
        assert e["ms"] > 0 and e["algo_bytes"] > 0 and 0 < e["frac"] < 1, name
    assert oc["cfg3"]["contexts"] == 2 and oc["cfg3"]["ms_one_stream"] > 0
    assert oc["cfg5_streamed"]["h2d_GBs"] > 1 and oc["cfg5_streamed"]["bound"] == "pcie"

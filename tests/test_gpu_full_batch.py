"""Every frame of the large-batch paths against the CPU oracle (oracle/pss_oracle.c), at the batch sizes bench.py runs and one step past
the grid caps and dispatcher crossovers: the WFM step (65 536 x 1024 and the counts around wfm_small_batch_max = 6000), the NFM crossover
at small_batch_max = 8192, cfg 3 (8192 / 8200 x 16 384: AM, USB / LSB in all three Hilbert modes, power, AGC, dB rows), cfg 4 (8192 / 8200
scanner slices x 4096) and the reference's read-buffer length (732 x 32 768), plus 131 072-point spectra with more than 8192 workgroups in
k_huge_p1.

The per-path tests of test_gpu_parity.py pin each kernel family on small batches; these walk the grid-stride loops of the capped grids
(8192 workgroups that each own several frames), the last partial 64-frame tile and the crossovers, where only spot checks looked before.
Criteria are those of the per-path tests, unchanged.  Every batch is made of frames that differ from each other (checked on the host), with
edge frames planted deep in it (_plant); outputs come to the host in chunks of CHUNK frames, the oracle runs over oracle_lib.map_frames'
thread pool, and a failing assertion names the failing frame indices.

Measured on one MI355X: 44.5 s for the whole file (the 65 536-frame WFM step 6.4 s, each cfg-3 leg 4.1-4.7 s, every other test under
1 s).  The largest leg (cfg-3 SSB at 8200 frames) holds about 6 GB of buffers, freed before the next.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle_lib as O
import gpu_util as G
from spectrum_bounds import exact_rows_bad, scan_ulp_bound
from pyspecsdr_amd import _lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bench_configs as BC  # noqa: E402

CHUNK = 2048
SSB_ATOL = 2e-14          # test_ssb_vs_golden: the register Hilbert transform against pocketfft's round trip
DB_REL = 1e-4             # the spectrum contract: |db - ref| <= 1e-4 * max(|ref|, 1)


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def _dev():
    G.engine()
    return torch.device("cuda", 0)


def _plant(iq):
    """Edge frames deep in the batch (device tensor [nf][n][2], in place): a silent frame (0 / 0: NaN audio, PCM 0), one NaN sample,
    a 1e-19-amplitude frame (values that differ in their low words only; float32 |x|^2 below the normal range) and a near-full-scale
    frame.  Positions 5000, 8191, 8192 and the last frame where the batch has them.  -> {kind: frame}."""
    nf = iq.shape[0]
    pos = {"silent": min(5000, nf // 2), "nan": min(8191, nf - 4), "tiny": min(8192, nf - 3), "full": nf - 1}
    assert len(set(pos.values())) == 4
    iq[pos["silent"]] = 0.0
    iq[pos["nan"], iq.shape[1] // 3, 0] = float("nan")
    iq[pos["tiny"]] *= 1e-19
    iq[pos["full"]] *= 0.999 / float(iq[pos["full"]].abs().max())
    torch.cuda.synchronize()
    return pos


class Frames:
    """Failing frame indices per criterion, gathered over the chunks of a batch, and the check that no two input frames are identical."""

    def __init__(self, label):
        self.label, self.bad, self.digests, self.nf = label, {}, set(), 0

    def add(self, what, frames, f0=0):
        frames = np.asarray(frames, dtype=np.int64)
        if frames.size:
            self.bad.setdefault(what, []).append(frames + f0)

    def inputs(self, x):
        for row in x:
            self.digests.add(hashlib.blake2b(row.tobytes(), digest_size=16).digest())
        self.nf += len(x)

    def check(self):
        assert len(self.digests) == self.nf, f"{self.label}: {self.nf - len(self.digests)} input frames repeat another frame"
        msg = []
        for what, parts in self.bad.items():
            f = np.concatenate(parts)
            msg.append(f"{what}: {f.size} frames, first {f[:16].tolist()}")
        assert not msg, f"{self.label}: " + "; ".join(msg)


def _chunks(nf, size=CHUNK):
    for f0 in range(0, nf, size):
        yield f0, min(nf, f0 + size)


def _host_iq(d_iq, f0, f1):
    return d_iq[f0:f1].cpu().numpy().view(np.complex64).reshape(f1 - f0, -1)


def _h(t, f0, f1):
    return t[f0:f1].cpu().numpy()


def _rows(a, k):
    return np.ascontiguousarray(a).reshape(k, -1)


def bits_bad(got, want):
    """Frames (first axis) whose values differ in any bit; NaN matches NaN whatever its payload."""
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want, dtype=g.dtype)
    u = np.uint64 if g.dtype == np.float64 else np.uint32
    same = (g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))
    return np.nonzero(~_rows(same, len(g)).all(axis=1))[0]


def close_bad(got, want, atol=None, rel=None):
    """Frames with a value off by more than atol (or rel * max(|want|, 1)), or with NaN where the other has none."""
    g = np.asarray(got, np.float64)
    w = np.asarray(want, np.float64)
    tol = atol if atol is not None else rel * np.maximum(np.abs(w), 1.0)
    gn, wn = np.isnan(g), np.isnan(w)
    with np.errstate(invalid="ignore"):
        ok = np.where(gn | wn, gn & wn, np.abs(g - w) <= tol)
    return np.nonzero(~_rows(ok, len(g)).all(axis=1))[0]


def eq_bad(got, want):
    return np.nonzero(_rows(np.asarray(got) != np.asarray(want), len(got)).any(axis=1))[0]


def dev_bad(a, b):
    """Frames where two device tensors of the same shape differ in any byte."""
    d = (a.view(torch.uint8) != b.view(torch.uint8)).reshape(a.shape[0], -1).any(dim=1)
    return torch.nonzero(d).flatten().cpu().numpy()


def int16_of(a):
    """np.int16(a * 32767) as the reference evaluates it on x86: truncation toward zero, NaN -> 0 (oracle pss_o_pcm16_stereo)."""
    v = np.asarray(a, np.float64) * 32767.0
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), 0.0, np.trunc(v)).astype(np.int32).astype(np.int16)


def _free(*_):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _am_sos(e):
    sos = np.empty((5, 6))
    e.lib.pss_am_bandpass_sos(sos.ctypes.data)
    return sos


def _wfm_filt(e, fs):
    lp, pil, lmr, alpha = e.wfm_filters(fs)
    _, sos, zi = e.nfm_filters(fs)
    return dict(lp_sos=lp, pilot_sos=pil, lmr_sos=lmr, alpha=alpha, dec_sos=sos, dec_zi=zi)


# ---- a. the WFM step ------------------------------------------------------------------------------------------------------------------
def _wfm_batch(e, nf, n, fs, seed, filt, cells=True):
    """demodulate_signal(WFM) = iq_correction + demodulate_wfm on every frame: float64 audio bits and np.int16(a * 32767) against the
    oracle; pss_frame_pipeline_cells(WFM) on the same IQ must leave the same PCM bytes."""
    dev = _dev()
    iq = BC.synth("fm", nf, n, fs, dev, seed)
    _plant(iq)
    n_out = e.demod_out_len(L.MODE_WFM, n, fs)
    pcm, au = G.empty((nf, n_out, 2), torch.int16), G.empty((nf, n_out, 2), torch.float64)
    e.demod_signal(L.MODE_WFM, iq, nf, n, fs, pcm, au)
    F = Frames(f"WFM {nf} x {n} @ {fs:g}")
    if cells:
        W = BC.DISP_W
        db32 = G.empty((nf, n), torch.float32)
        lo, hi = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
        gl, co = G.empty((nf, W), torch.int8), G.empty((nf, W), torch.int8)
        pcm_c = G.empty((nf, n_out, 2), torch.int16)
        e.frame_pipeline_cells(L.MODE_WFM, iq, nf, n, fs, db32, None, lo, hi, W, gl, co, pcm_c, window=30)
        e.sync()
        F.add("pss_frame_pipeline_cells PCM != demod_signal PCM", dev_bad(pcm_c, pcm))
        del db32, lo, hi, gl, co, pcm_c
    e.sync()

    def ref(x):
        return O.demod_wfm(O.iq_correction(x), fs, filt)
    with np.errstate(all="ignore"):
        for f0, f1 in _chunks(nf):
            x = _host_iq(iq, f0, f1)
            F.inputs(x)
            want = np.stack(O.map_frames(ref, x))
            F.add("float64 audio bits", bits_bad(_h(au, f0, f1), want), f0)
            F.add("int16 PCM", eq_bad(_h(pcm, f0, f1), int16_of(want)), f0)
    del iq, pcm, au
    _free()
    F.check()


@pytest.mark.parametrize("nf,n,fs", [
    (65536, 1024, 2.4e6),     # the WFM step bench.py times (fused forward kernel, k_wfm_rows_q1 normalisation, capped grids)
    (6000, 1024, 2.4e6),      # the last count on the small-batch array (wfm_small_batch_max)
    (6001, 1024, 2.4e6),      # the first on the fused kernels
    (8192, 1024, 2.4e6),
    (8193, 1024, 2.4e6),      # one frame past a capped grid of 8192 workgroups
    (8255, 1024, 2.4e6),      # neither a multiple of 64 (the fused kernels' TILE) nor of 8192
    (8255, 2048, 1.024e6),    # another rate and length (bench_configs cfg 5's rate), large batch
])
def test_wfm_every_frame_vs_oracle(nf, n, fs):
    """The WFM step on every frame.  The dispatcher's generic path for a decimator that is not [1, 2, 1]-shaped (b121 in pss_demod.hip)
    is covered by test_wfm_generic_decimator_every_frame: no designed rate reaches it — the decimator is scipy's cheby1(8, 0.05, 0.8 / q)
    as second-order sections, whose sections 1..3 have the numerator [1, 2, 1] for every q from 2 to 1999 (checked against SciPy), and
    q = 1 skips decimation altogether."""
    e = G.engine()
    _wfm_batch(e, nf, n, fs, 20261015 + nf + n, _wfm_filt(e, fs))


def test_wfm_generic_decimator_every_frame():
    """A decimator table with the same response but scaled section numerators (section 1 x 2, section 2 x 0.5, exact in binary): not
    [1, 2, 1]-shaped, so a large batch leaves the fused forward kernel for the corrected-copy path with the generic decimator steps —
    every frame against the oracle run with the same table."""
    e = G.engine()
    nf, n, fs = 8193, 1024, 2.4e6
    taps, sos, zi = e.nfm_filters(fs)
    sos2 = sos.copy()
    assert all(np.array_equal(sos[s, :3], [1.0, 2.0, 1.0]) for s in (1, 2, 3))
    sos2[1, :3] *= 2.0
    sos2[2, :3] *= 0.5
    filt = _wfm_filt(e, fs)
    filt["dec_sos"] = sos2
    e.set_nfm_filters(fs, taps, sos2, zi)
    try:
        _wfm_batch(e, nf, n, fs, 4711, filt, cells=False)
    finally:
        e.set_nfm_filters(fs, taps, sos, zi)


@pytest.mark.parametrize("nf", [8192, 8193])
def test_nfm_crossover_every_frame_vs_oracle(nf):
    """NFM at small_batch_max = 8192 (the last count on the small-batch array) and one past it (the fused kernels): float64 audio bits and
    int16 PCM of every frame."""
    e = G.engine()
    n, fs = 1024, 2.4e6
    iq = BC.synth("fm", nf, n, fs, _dev(), 99 + nf)
    _plant(iq)
    n_out = e.demod_out_len(L.MODE_NFM, n, fs)
    pcm, au = G.empty((nf, n_out, 2), torch.int16), G.empty((nf, n_out), torch.float64)
    e.demod(L.MODE_NFM, iq, nf, n, fs, pcm, au)
    e.sync()
    taps, sos, zi = e.nfm_filters(fs)
    F = Frames(f"NFM {nf} x {n}")
    with np.errstate(all="ignore"):
        for f0, f1 in _chunks(nf):
            x = _host_iq(iq, f0, f1)
            F.inputs(x)
            want = np.stack(O.map_frames(lambda r: O.demod_nfm(r, fs, taps, sos, zi), x))
            F.add("float64 audio bits", bits_bad(_h(au, f0, f1), want), f0)
            F.add("int16 PCM", eq_bad(_h(pcm, f0, f1), np.stack([O.pcm16_stereo(a) for a in want])), f0)
    del iq, pcm, au
    _free()
    F.check()


# ---- b. cfg 3 / d. read-buffer length: AM, power, AGC, dB rows; USB / LSB -------------------------------------------------------------
def _am_power_db(nf, n, fs, seed):
    """AM audio bits and int16, power_db bits, pss_demod_power(AM) == the separate calls, the AGC trajectory over every frame, dB rows
    within 1e-4 and (db_exact = 1) equal to the oracle's float64 rows rounded to float32."""
    e = G.engine()
    iq = BC.synth("am", nf, n, fs, _dev(), seed)
    _plant(iq)
    F = Frames(f"AM / power / dB {nf} x {n}")
    pcm, au = G.empty((nf, n, 2), torch.int16), G.empty((nf, n), torch.float64)
    pw, gi = G.empty((nf,), torch.float32), G.empty((nf,), torch.int32)
    e.demod(L.MODE_AM, iq, nf, n, fs, pcm, au)
    e.power_db(iq, nf, n, pw)
    e.agc_steps(pw, nf, 20, 29, gi)
    pcm2, pw2 = G.empty((nf, n, 2), torch.int16), G.empty((nf,), torch.float32)
    e.demod_power(L.MODE_AM, iq, nf, n, fs, pcm2, None, pw2)
    e.sync()
    F.add("pss_demod_power(AM) PCM != demod", dev_bad(pcm2, pcm))
    F.add("pss_demod_power(AM) power != power_db", dev_bad(pw2, pw))
    del pcm2, pw2
    _free()
    db, dbx = G.empty((nf, n), torch.float32), G.empty((nf, n), torch.float32)
    e.spectrum_db(iq, nf, n, db)
    e.set_option("db_exact", 1)
    try:
        e.spectrum_db(iq, nf, n, dbx)
        e.sync()
    finally:
        e.set_option("db_exact", 0)
    sos = _am_sos(e)
    powers = []
    with np.errstate(all="ignore"):
        for f0, f1 in _chunks(nf):
            x = _host_iq(iq, f0, f1)
            F.inputs(x)
            want = O.map_frames(lambda r: (O.demod_am(r, sos), O.power_db(r), O.compute_fft(r)), x)
            a = np.stack([w[0] for w in want])
            p = np.array([w[1] for w in want], np.float32)
            d = np.stack([w[2] for w in want])
            powers.append(p)
            F.add("AM float64 audio bits", bits_bad(_h(au, f0, f1), a), f0)
            F.add("AM int16 PCM", eq_bad(_h(pcm, f0, f1), np.stack([O.pcm16_stereo(r) for r in a])), f0)
            F.add("power_db bits", bits_bad(_h(pw, f0, f1), p), f0)
            F.add("dB rows beyond 1e-4", close_bad(_h(db, f0, f1), d, rel=DB_REL), f0)
            F.add("db_exact rows not the float32 rounding of the oracle's rows", exact_rows_bad(_h(dbx, f0, f1), d), f0)
    idx, traj = 20, np.empty(nf, np.int32)
    for k, p in enumerate(np.concatenate(powers)):
        idx = O.agc_step(p, idx, 29)
        traj[k] = idx
    F.add("AGC gain index", eq_bad(G.host(gi)[:, None], traj[:, None]))
    del iq, pcm, au, pw, gi, db, dbx
    _free()
    F.check()


def _ssb(nf, n, fs, mode, seed):
    """USB / LSB (the reference demodulates both the same way): default register Hilbert (int16 equal, float64 within 2e-14),
    hilbert_exact = 1 (bit-equal to demod_ssb), ssb_hilbert = 0 (bit-equal to demod_ssb without the round trip); USB: pss_demod_power ==
    the separate calls, power bits against the oracle."""
    e = G.engine()
    iq = BC.synth("ssb", nf, n, fs, _dev(), seed)
    _plant(iq)
    taps = e.ssb_taps(fs)
    F = Frames(f"{'USB' if mode == L.MODE_USB else 'LSB'} {nf} x {n}")
    out = {}
    for name, key, val, default in (("register", None, None, None), ("exact", "hilbert_exact", 1, 0), ("no_hilbert", "ssb_hilbert", 0, 1)):
        out[name] = (G.empty((nf, n, 2), torch.int16), G.empty((nf, n), torch.float64))
        if key:
            e.set_option(key, val)
        try:
            e.demod(mode, iq, nf, n, fs, *out[name])
            e.sync()
        finally:
            if key:
                e.set_option(key, default)
    pw = None
    if mode == L.MODE_USB:
        pw, pw2, pcm2 = G.empty((nf,), torch.float32), G.empty((nf,), torch.float32), G.empty((nf, n, 2), torch.int16)
        e.power_db(iq, nf, n, pw)
        e.demod_power(L.MODE_USB, iq, nf, n, fs, pcm2, None, pw2)
        e.sync()
        F.add("pss_demod_power(USB) PCM != demod", dev_bad(pcm2, out["register"][0]))
        F.add("pss_demod_power(USB) power != power_db", dev_bad(pw2, pw))
        del pw2, pcm2
    with np.errstate(all="ignore"):
        for f0, f1 in _chunks(nf):
            x = _host_iq(iq, f0, f1)
            F.inputs(x)
            want = O.map_frames(lambda r: (O.demod_ssb(r, taps), O.demod_ssb(r, taps, hilbert=False), O.power_db(r)), x)
            a = np.stack([w[0] for w in want])
            b = np.stack([w[1] for w in want])
            pa, pb = np.stack([O.pcm16_stereo(r) for r in a]), np.stack([O.pcm16_stereo(r) for r in b])
            F.add("register Hilbert int16 PCM", eq_bad(_h(out["register"][0], f0, f1), pa), f0)
            F.add("register Hilbert float64 audio beyond 2e-14", close_bad(_h(out["register"][1], f0, f1), a, atol=SSB_ATOL), f0)
            F.add("hilbert_exact int16 PCM", eq_bad(_h(out["exact"][0], f0, f1), pa), f0)
            F.add("hilbert_exact float64 audio bits", bits_bad(_h(out["exact"][1], f0, f1), a), f0)
            F.add("ssb_hilbert=0 int16 PCM", eq_bad(_h(out["no_hilbert"][0], f0, f1), pb), f0)
            F.add("ssb_hilbert=0 float64 audio bits", bits_bad(_h(out["no_hilbert"][1], f0, f1), b), f0)
            if pw is not None:
                F.add("power_db bits", bits_bad(_h(pw, f0, f1), np.array([w[2] for w in want], np.float32)), f0)
    del iq, out, pw
    _free()
    F.check()


@pytest.mark.parametrize("nf", [8192, 8200])
def test_cfg3_am_power_agc_db_rows_every_frame(nf):
    """cfg 3 at its full batch (8192 x 16 384: the capped power / AM-mean grids end exactly on their first step) and 8 frames past it
    (the grid-stride second step of k_pairwise / k_pairwise2, k_am_grp, k_spectrum_xl)."""
    _am_power_db(nf, 16384, 2.4e6, 20260928 + 3)


@pytest.mark.parametrize("mode", [L.MODE_USB, L.MODE_LSB], ids=["usb", "lsb"])
@pytest.mark.parametrize("nf", [8192, 8200])
def test_cfg3_ssb_every_frame(nf, mode):
    _ssb(nf, 16384, 2.4e6, mode, 20260928 + 13)


# ---- c. cfg 4 scanner -----------------------------------------------------------------------------------------------------------------
# test_scanner_rows_equal_the_oracle_on_every_kernel_family allows 3 differing values in its 146 912 (two float64 transforms, this
# kernel's and the oracle's, agree to ~1e-16 of the largest bin: a weak bin beside a strong carrier can round the other way in float32).
# Measured on 8192 x 4096 synth("scan") slices: 5 of 33 554 432 values differ (slices 540, 1950, 2371, 4860, 5550).
SCAN_DIFF_RATE = 3 / 146912


@pytest.mark.parametrize("ns", [8192, 8200])
def test_cfg4_scanner_every_slice(ns):
    """cfg 4 (8192 slices x 4096, synth("scan")) and 8 slices past it: every value within scan_ulp_bound of scan_slice, the share of values that
    differ at all within the rate of the per-family test, peak / count / bandwidth equal to the oracle's on bit-equal rows and to those
    recomputed from the device's own row elsewhere."""
    e = G.engine()
    n, fs = 4096, 2.4e6
    iq = BC.synth("scan", ns, n, fs, _dev(), 20260928 + 4)
    _plant(iq)
    db, pk = G.empty((ns, n), torch.float32), G.empty((ns,), torch.float32)
    bw, cnt = G.empty((ns,), torch.float64), G.empty((ns,), torch.int32)
    e.scan(iq, ns, n, fs, db, pk, bw, cnt)
    e.sync()
    F = Frames(f"scanner {ns} x {n}")
    diff = total = 0
    with np.errstate(all="ignore"):
        for f0, f1 in _chunks(ns):
            x = _host_iq(iq, f0, f1)
            F.inputs(x)
            want = O.map_frames(lambda r: O.scan_slice(r, fs), x)
            g, gp, gb, gc = _h(db, f0, f1), _h(pk, f0, f1), _h(bw, f0, f1), _h(cnt, f0, f1)
            w = np.stack([r[0] for r in want])
            gn, wn = np.isnan(g), np.isnan(w)
            ulp = np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64))
            ulp[gn & wn] = 0
            ulp[gn ^ wn] = 1 << 40
            with np.errstate(invalid="ignore"):
                far = ((np.abs(g.astype(np.float64) - w) > scan_ulp_bound(w)) & ~(gn & wn)) | (gn ^ wn)
            F.add("dB value beyond one component ulp of scan_slice", np.nonzero(far.any(axis=1))[0], f0)
            diff += int((ulp != 0).sum())
            total += ulp.size
            for k in range(f1 - f0):
                if not ulp[k].any():
                    ok = (gp[k].tobytes() == np.float32(want[k][1]).tobytes() and int(gc[k]) == want[k][3] and float(gb[k]) == want[k][2])
                else:
                    p = g[k].max()
                    c = int(np.sum(g[k] > p - np.float32(20)))
                    ok = gp[k].tobytes() == p.tobytes() and int(gc[k]) == c and float(gb[k]) == c * (fs / n)
                if not ok:
                    F.add("peak / count / bandwidth", [k], f0)
    del iq, db, pk, bw, cnt
    _free()
    F.check()
    print(f"scanner {ns} x {n}: {diff} of {total} dB values differ from the oracle")
    assert diff <= SCAN_DIFF_RATE * total, (diff, total)


# ---- d. the reference's read-buffer length; spectra on more than 8192 k_huge_p1 workgroups --------------------------------------------
READ_NF, READ_N = 732, 32768     # 10 s of capture at 2.4 MS/s cut into the main loop's 32 768-sample read buffers


def test_read_buffer_nfm_pipeline_every_frame():
    """pss_frame_pipeline_nfm on 732 x 32 768 @ 2.4 MS/s (k_spectrum_r16_big: a grid of 512 workgroups, each walking two frames): every
    frame's int16 PCM equal and dB row within 1e-4."""
    e = G.engine()
    nf, n, fs, W = READ_NF, READ_N, 2.4e6, BC.DISP_W
    iq = BC.synth("fm", nf, n, fs, _dev(), 732)
    _plant(iq)
    n_out = e.demod_out_len(L.MODE_NFM, n, fs)
    db = G.empty((nf, n), torch.float32)
    lo, hi = G.empty((nf,), torch.float32), G.empty((nf,), torch.float32)
    gl, co, pcm = G.empty((nf, W), torch.int8), G.empty((nf, W), torch.int8), G.empty((nf, n_out, 2), torch.int16)
    e.frame_pipeline_nfm(iq, nf, n, fs, db, None, lo, hi, W, gl, co, pcm)
    e.sync()
    taps, sos, zi = e.nfm_filters(fs)
    F = Frames(f"NFM pipeline {nf} x {n}")
    with np.errstate(all="ignore"):
        for f0, f1 in _chunks(nf, 256):
            x = _host_iq(iq, f0, f1)
            F.inputs(x)
            want = O.map_frames(lambda r: (O.pcm16_stereo(O.demod_nfm(r, fs, taps, sos, zi)), O.compute_fft(r)), x)
            F.add("int16 PCM", eq_bad(_h(pcm, f0, f1), np.stack([w[0] for w in want])), f0)
            F.add("dB rows beyond 1e-4", close_bad(_h(db, f0, f1), np.stack([w[1] for w in want]), rel=DB_REL), f0)
    del iq, db, lo, hi, gl, co, pcm
    _free()
    F.check()


def test_read_buffer_am_power_db_every_frame():
    _am_power_db(READ_NF, READ_N, 2.4e6, 733)


def test_read_buffer_usb_every_frame():
    _ssb(READ_NF, READ_N, 2.4e6, L.MODE_USB, 734)


def test_huge_spectra_past_the_k_huge_p1_grid_cap():
    """131 072-point spectra (the N = 256 x NS path, NS = 512): k_huge_p1 wants n_frames * NS / 16 = 300 * 32 = 9600 workgroups and is
    capped at 8192, so its workgroups walk a second step.  (32 768-point frames never reach k_huge_p1: it serves N >= 131 072.)  Every
    row within 1e-4 of compute_fft."""
    e = G.engine()
    nf, n, fs = 300, 131072, 2.4e6
    assert nf * ((n >> 8) // 16) > 8192
    iq = BC.synth("am", nf, n, fs, _dev(), 131)
    _plant(iq)
    db = G.empty((nf, n), torch.float32)
    e.spectrum_db(iq, nf, n, db)
    e.sync()
    F = Frames(f"spectrum {nf} x {n}")
    with np.errstate(all="ignore"):
        for f0, f1 in _chunks(nf, 64):
            x = _host_iq(iq, f0, f1)
            F.inputs(x)
            F.add("dB rows beyond 1e-4", close_bad(_h(db, f0, f1), np.stack(O.map_frames(O.compute_fft, x)), rel=DB_REL), f0)
    del iq, db
    _free()
    F.check()

"""The float64 dB evaluation (pss_db_exact.h: db64_core and the per-frame +inf / NaN fix-up of k_spectrum_post) at the shapes where it can
go wrong: 1, 4, 5 and 9 frames of 1024 points (the fix-up's ballot is per frame, a workgroup holds four frames) through
pss_frame_pipeline_cells and pss_spectrum_cells (the fused kernel: float32 rows, float64 rows, extremes, cells) and through the float64-row
entry pss_spectrum_db_f64, and two frames each of 256, 2048, 4096 and 8192 points with db_exact (k_spectrum_r16 / k_spectrum_xl share the
evaluation).

Inputs: the benchmark's FM synthesis (NumPy's generator, so the CPU test below sees the same samples); an all-zero frame (every bin
10 log10(1e-10)); a batch of 5 whose frame 2 holds one NaN sample and frame 3 one +inf sample, finite frames in the same workgroup; a
windowed tone whose peak bin's power is within 1e-6 of 1 (the 0 dB crossing); noise scaled by 1e15 and by 1e-8.

Expected values: the oracle's own step from the IQ (oracle_lib.headline_f64 / compute_fft).  float64 rows rtol = atol = 1e-11, extremes to
1e-11, PCM and cells equal, non-finite bins equal as values (the +inf-sample frame: see the test).  float32 rows: every bin equal to np.float32 of the oracle's float64 value;
the issue admits one float32 ulp where the oracle's value lies within 1e-9 relative of the midpoint of two float32 neighbours, and asks
for seeds without such a bin.  No seed has none (the CPU test says why), so the window admitted here is the narrower 1e-11, and the CPU
test asserts that the chosen seeds keep every bin clear of it: as they stand, these tests admit no float32 difference at all.

The host check of the arithmetic (tools/check_db_host.cpp: the evaluation and the one it replaced against log10l) is built and run here
without a GPU.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, W = 2.4e6, 112
OTHER_LENGTHS = (256, 2048, 4096, 8192)


def fm(nf, n, seed):
    """bench.synth_fm_iq's signal: three audio tones, 5 kHz deviation, A = 0.5, sigma = 0.02."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    ph0 = 0.1 * np.arange(nf)[:, None]
    m = 0.5 * np.sin(2 * np.pi * 400 * t + ph0) + 0.3 * np.sin(2 * np.pi * 1000 * t + 2 * ph0) + 0.2 * np.sin(2 * np.pi * 2500 * t + 3 * ph0)
    phase = 2 * np.pi * 5e3 * np.cumsum(m, axis=1) / FS + ph0
    x = 0.5 * np.exp(1j * phase) + 0.02 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))
    return x.astype(np.complex64)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)


def tone_0db(n, k, off):
    """A tone on bin k, scaled so that its (windowed) peak bin has power 1 + off (|off| = 8e-7; the complex64 rounding of the samples moves it
    by another ~1e-7): just above or just below 0 dB."""
    x = np.exp(2j * np.pi * k * np.arange(n) / n)
    peak = O.compute_fft(x.astype(np.complex64)).max()
    return (x * (10.0 ** (-peak / 20) * np.sqrt(1.0 + off))).astype(np.complex64)


# seeds (and tone bins) chosen on the CPU so that no bin of the oracle's rows lies within MIDPOINT_CLEAR of a float32 rounding boundary
SEEDS = {"fm1": 0, "fm4": 1, "fm5": 0, "fm9": 9, "special5": 3, "scaled9": 6, 256: 1, 2048: 4, 4096: 0, 8192: 41}
MIDPOINT_CLEAR = 1e-11
MIDPOINT_CLEAR_DB = 5e-14


def batch(name, seed):
    """complex64 [frames, 1024]"""
    n = 1024
    if name.startswith("fm"):
        return fm(int(name[2:]), n, 1000 * seed + int(name[2:]))
    if name == "special5":
        sp = np.stack([tone_0db(n, 128 + seed, 8e-7), np.zeros(n, np.complex64), noise(n, 100 * seed + 1), noise(n, 100 * seed + 2), noise(n, 100 * seed + 3)])
        sp[2, 300] = np.nan + 0.1j
        sp[3, 517] = np.inf + 0.1j
        return sp
    assert name == "scaled9"
    return np.stack([noise(n, 100 * seed + 10 + k) * np.float32(1e15) for k in range(4)] + [noise(n, 100 * seed + 20 + k) * np.float32(1e-8) for k in range(4)]
                    + [tone_0db(n, 200 + seed, -8e-7)])


BATCHES = ("fm1", "fm4", "fm5", "fm9", "special5", "scaled9")


def batches():
    return {name: batch(name, SEEDS[name]) for name in BATCHES}


def other_length_frames(n, seed=None):
    seed = SEEDS[n] if seed is None else seed
    return np.stack([fm(1, n, 1000 * seed + n)[0], tone_0db(n, n // 8 + seed, 8e-7)])


_ORACLE = {}


def oracle(name, x):
    """The oracle's step from the IQ, computed once per batch."""
    if name not in _ORACLE:
        if x.shape[1] == 1024:
            taps, sos, zi = _filters()
            _ORACLE[name] = O.headline_f64(x, FS, taps, sos, zi, 30, W, 2, keep_db=True)
        else:
            _ORACLE[name] = {"db": np.stack([O.compute_fft(f) for f in x])}
    return _ORACLE[name]


_FILTERS = None


def _filters():
    global _FILTERS
    if _FILTERS is None:
        import gpu_util as G
        _FILTERS = G.engine().nfm_filters(FS)
    return _FILTERS


def near_f32_midpoint(want64, rel=1e-9, floor=0.0):
    """Bins whose float64 value lies within max(rel * |value|, floor) of the midpoint of two neighbouring float32 values."""
    with np.errstate(invalid="ignore", over="ignore"):
        w32 = want64.astype(np.float32)
        w = w32.astype(np.float64)
        other = np.where(want64 >= w, np.nextafter(w32, np.float32(np.inf)), np.nextafter(w32, np.float32(-np.inf))).astype(np.float64)
        mid = 0.5 * (w + other)
        return np.isfinite(want64) & (np.abs(want64 - mid) <= np.maximum(rel * np.abs(mid), floor))


def f32_failures(got32, want64, any_nonfinite=()):
    """Bins of a float32 row that are neither np.float32 of the oracle's value nor one ulp off at a near-midpoint value; non-finite bins by
    value (rows listed in any_nonfinite: non-finite where the oracle's are, of either kind)."""
    with np.errstate(invalid="ignore", over="ignore"):
        w32 = want64.astype(np.float32)
    same = (got32 == w32) | (np.isnan(got32) & np.isnan(w32))
    for f in any_nonfinite:
        same[f] |= ~np.isfinite(got32[f]) & ~np.isfinite(w32[f])
    one_ulp = (got32 == np.nextafter(w32, np.float32(np.inf))) | (got32 == np.nextafter(w32, np.float32(-np.inf)))
    return ~(same | (one_ulp & near_f32_midpoint(want64, MIDPOINT_CLEAR)))


def f64_failures(got, want, any_nonfinite=()):
    fin = np.isfinite(want)
    ok = np.where(fin, np.isclose(got, want, rtol=1e-11, atol=1e-11), (np.isnan(got) & np.isnan(want)) | (got == want))
    for f in any_nonfinite:
        ok[f] |= ~np.isfinite(got[f]) & ~fin[f]
    return ~ok


def test_host_check_of_the_db_evaluation(tmp_path):
    """tools/check_db_host.cpp, built without a sanitizer and run: none of the new evaluation's three figures exceeds the old one's."""
    exe = str(tmp_path / "check_db_host")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", os.path.join(ROOT, "tools", "check_db_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "verdict: ok" in r.stdout, r.stdout + r.stderr


def test_chosen_inputs_have_no_bin_at_a_float32_midpoint():
    """The issue's float32 rule: one ulp is admitted where the oracle's value is within 1e-9 (relative) of a float32 rounding boundary, and the
    seeds are to have no such bin.  A window of +-1e-9 covers 1.7 - 3.4 % of the distance between two float32 neighbours (2^-23 .. 2^-24
    relative), so every 1024-bin row has about 25 bins inside it and no seed is free of them (the count is printed).  What the seeds are chosen
    for instead (SEEDS, searched with this function): no bin lies within MIDPOINT_CLEAR = 1e-11 relative — ten times what the transforms
    differ by — nor within MIDPOINT_CLEAR_DB = 5e-14 dB of a boundary (near 0 dB a relative window means nothing: a relative difference of
    1e-15 in a power of 1 is 4e-15 dB).  f32_failures admits one ulp only inside that 1e-11 window, which is empty: every float32 bin has to
    equal np.float32 of the oracle's value."""
    inside = 0
    for name, x in batches().items():
        rows = np.stack([O.compute_fft(f) for f in x])
        assert int(np.count_nonzero(near_f32_midpoint(rows, MIDPOINT_CLEAR, MIDPOINT_CLEAR_DB))) == 0, name
        inside += int(np.count_nonzero(near_f32_midpoint(rows)))
    for n in OTHER_LENGTHS:
        rows = np.stack([O.compute_fft(f) for f in other_length_frames(n)])
        assert int(np.count_nonzero(near_f32_midpoint(rows, MIDPOINT_CLEAR, MIDPOINT_CLEAR_DB))) == 0, n
        inside += int(np.count_nonzero(near_f32_midpoint(rows)))
    print("bins within 1e-9 of a float32 rounding boundary:", inside)
    # the special inputs are what they claim to be
    sp = np.stack([O.compute_fft(f) for f in batches()["special5"]])
    assert abs(sp[0].max()) < 10 * np.log10(1 + 1e-6) and np.all(sp[1] == 10 * np.log10(1e-10))
    assert np.isnan(sp[2]).any() and not np.isfinite(sp[3]).any() and np.isfinite(sp[[0, 1, 4]]).all()


def _report(fails):
    for f in fails:
        print("MISMATCH", f)
    assert not fails, fails[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("name", BATCHES)
def test_fused_kernel_rows_extremes_cells_equal_the_oracle(name):
    import torch
    import gpu_util as G
    from pyspecsdr_amd import _lib as L
    e = G.engine()
    x = batches()[name]
    nf, n = x.shape
    o = oracle(name, x)
    iq = G.dev(x)
    n_out = e.demod_out_len(L.MODE_NFM, n, FS)
    fails = []
    # The +inf-sample frame: which of its bins are +inf and which NaN is the transform's doing (an infinite operand times a twiddle factor's
    # exact zero is NaN in one factorisation and never formed in another): measured, 76 of the 1024 bins are of the other kind than pocketfft's,
    # through the unfused float64-row kernel (whose evaluation tests every value, as before this change) as through the fused one (NOTEBOOK R7-01).
    # So that frame's bins are held to "non-finite where the oracle's are" and, bin for bin, to the KIND the float64-row entry yields — the
    # per-value rule on the same transform, which the fused kernel's per-frame fix-up has to reproduce.  Every other frame: the oracle's kind.
    any_nf = (3,) if name == "special5" else ()
    d = G.empty((nf, n), torch.float64)
    e.spectrum_db_f64(iq, nf, n, d)
    e.sync()
    rows_f64 = G.host(d)
    bad = f64_failures(rows_f64, o["db"], any_nf)
    if bad.any():
        fails.append(("spectrum_db_f64", int(bad.sum()), np.argwhere(bad)[:3].tolist()))

    def kind(a):
        return np.isnan(a) * 1 + np.isposinf(a) * 2 + np.isneginf(a) * 3

    def check(tag, c, pcm):
        for k in ("db32", "db64"):
            if c.get(k) is not None and not np.array_equal(kind(G.host(c[k])), kind(rows_f64)):
                fails.append((tag, k, "kinds of non-finite bins differ from the float64-row entry's", int(np.count_nonzero(kind(G.host(c[k])) != kind(rows_f64)))))
        if c.get("db32") is not None:
            bad = f32_failures(G.host(c["db32"]), o["db"], any_nf)
            print(tag, "float32 bins differing:", int(bad.sum()))
            if bad.any():
                fails.append((tag, "db32", int(bad.sum()), np.argwhere(bad)[:3].tolist()))
        if c.get("db64") is not None:
            bad = f64_failures(G.host(c["db64"]), o["db"], any_nf)
            fin = np.isfinite(o["db"])
            print(tag, "float64 bins outside 1e-11:", int(bad.sum()), "largest error", float(np.max(np.abs(G.host(c["db64"]) - o["db"])[fin], initial=0.0)))
            if bad.any():
                fails.append((tag, "db64", int(bad.sum()), np.argwhere(bad)[:3].tolist()))
        for k in ("lo", "hi"):
            if not np.allclose(G.host(c[k]), o[k], rtol=1e-11, atol=1e-11, equal_nan=True):
                fails.append((tag, k, G.host(c[k]).tolist(), o[k].tolist()))
        for k, ok in (("a", "glyph"), ("b", "colour")):
            d = int(np.count_nonzero(G.host(c[k]) != o[ok]))
            if d:
                fails.append((tag, ok, d))
        if pcm and not np.array_equal(G.host(c["pcm"]), o["pcm"]):
            fails.append((tag, "pcm", int(np.count_nonzero(G.host(c["pcm"]) != o["pcm"]))))

    def bufs(db32, db64):
        return dict(db32=G.empty((nf, n), torch.float32) if db32 else None, db64=G.empty((nf, n), torch.float64) if db64 else None,
                    lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64), a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"),
                    b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), pcm=G.empty((nf, n_out, 2), torch.int16))

    for db32, db64 in ((True, False), (True, True)):
        c = bufs(db32, db64)
        e.frame_pipeline_cells(L.MODE_NFM, iq, nf, n, FS, c["db32"], c["db64"], c["lo"], c["hi"], W, c["a"], c["b"], c["pcm"])
        e.sync()
        check(f"frame_pipeline_cells(db32={db32}, db64={db64})", c, True)
    for db32, db64 in ((True, False), (False, True)):
        c = bufs(db32, db64)
        e.spectrum_cells(iq, nf, n, c["db32"], c["db64"], c["lo"], c["hi"], W, c["a"], c["b"])
        e.sync()
        check(f"spectrum_cells(db32={db32}, db64={db64})", c, False)
    _report(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("n", OTHER_LENGTHS)
def test_other_lengths_share_the_evaluation(n):
    import torch
    import gpu_util as G
    e = G.engine()
    x = other_length_frames(n)
    nf = x.shape[0]
    o = oracle(f"len{n}", x)
    iq = G.dev(x)
    fails = []
    e.set_option("db_exact", 1)
    try:
        d32 = G.empty((nf, n), torch.float32)
        e.spectrum_db(iq, nf, n, d32)
        e.sync()
    finally:
        e.set_option("db_exact", 0)
    bad = f32_failures(G.host(d32), o["db"])
    print(n, "float32 bins differing:", int(bad.sum()))
    if bad.any():
        fails.append((n, "db_exact float32", int(bad.sum()), np.argwhere(bad)[:3].tolist()))
    d64 = G.empty((nf, n), torch.float64)
    e.spectrum_db_f64(iq, nf, n, d64)
    e.sync()
    bad = f64_failures(G.host(d64), o["db"])
    print(n, "float64 bins outside 1e-11:", int(bad.sum()), "largest error", float(np.max(np.abs(G.host(d64) - o["db"]))))
    if bad.any():
        fails.append((n, "float64", int(bad.sum()), np.argwhere(bad)[:3].tolist()))
    _report(fails)

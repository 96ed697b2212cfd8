"""compute_fft's dB rows from every kernel family held to float64 accuracy (spectrum_bounds.py), not only to the 1e-4 contract.

pss_spectrum_db picks a kernel by length (pss_fft.hip launch_spectrum): the generic k_spectrum (16-128), the register k_spectrum_r16<0..4>
(256-4096; 2048 one frame per workgroup), k_spectrum_xl<1, 2> (8192, 16384), k_spectrum_r16_big<3, 4> (32768, 65536; per-workgroup
scratch), k_huge_p1 / k_huge_p2 (2^17-2^20; float64 scratch) and Bluestein (2-15 and every non-power of two, on M = 256 NS), each with
a db_exact instantiation; one-sample frames have a kernel of their own.  The float64-row entry points have their own kernels
(launch_r16_f64, the f64_plain generic path, pss_spectrum_db_c128, the fused k_spectrum_post behind pss_spectrum_cells).

Every length runs a batch of the same inputs: a NaN-sample and an Inf-sample frame, a tone on a bin with noise ~120 dB down, a tone
off-bin, white noise, an impulse at a non-zero index, constant DC, an all-zero frame and a tone at amplitudes 10^k, k = -8 .. 30 (bins
straddling the 1e-10 floor at the low end, |X|^2 past FLT_MAX at the high end).  The grid-cap tests run one frame past each family's
grid cap, read from the launch code, with the non-finite frames first in the workgroups' grid-stride walks.  Reference: the CPU oracle
(oracle/pss_oracle.c) over oracle_lib.map_frames.  A failure names the family, length, frame (and its input) and first offending bin.

Measured on one MI355X: 33 s for the whole file (148 tests).  Device memory in use (hipMemGetInfo, after each test, this process's
torch cache and the library's grow-only scratch included) peaks at 2.84 GiB, after the 2^20-point compute_fft shim test.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle_lib as O
import gpu_util as G
import spectrum_bounds as SB

POW2 = [1 << k for k in range(4, 21)]
PAST_CROSSOVER = [17, 129, 257, 4097, 8193, 16385, 32769, 131073]     # first length past each crossover of the table above
BLUESTEIN = [2, 3, 4, 5, 7, 8, 15, 1001, 4097, 65537, 240000]
LENGTHS = sorted(set([1] + POW2 + PAST_CROSSOVER + BLUESTEIN))
F64_LENGTHS = [1 << k for k in range(4, 17)]                          # the float64-row entry points: powers of two 16 .. 65536


def family(n):
    if n == 1:
        return "k_spectrum_one"
    if SB.bluestein(n):
        return f"bluestein(M={SB.transform_len(n)})"
    if n <= 128:
        return "k_spectrum"
    if n <= 4096:
        return f"k_spectrum_r16<{int(math.log2(n)) - 8}>"
    if n <= 16384:
        return f"k_spectrum_xl<{int(math.log2(n)) - 12}>"
    if n <= 65536:
        return f"k_spectrum_r16_big<{int(math.log2(n)) - 12}>"
    return "k_huge_p1/p2"


def inputs(n, seed=0):
    """(frames complex64 [47, n], names): the non-finite frames first, then the finite ones."""
    rng = np.random.default_rng(seed + n)
    t = np.arange(n)
    noise = lambda: (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2)  # noqa: E731
    tone = np.exp(2j * np.pi * (n // 8) * t / n)
    fr, names = [], []

    def add(name, x):
        fr.append(np.asarray(x, np.complex128))
        names.append(name)
    x = noise()
    x[n // 2] = np.nan
    add("NaN sample", x)
    x = noise()
    x[n // 2] = np.inf
    add("Inf sample", x)
    add("tone on bin + noise -120 dB", tone + 1e-6 * noise())
    add("tone off bin", np.exp(2j * np.pi * (n // 8 + 0.37) * t / n))
    add("white noise", noise())
    imp = np.zeros(n, np.complex128)
    imp[min(n - 1, max(1, n // 3))] = 1 - 0.5j
    add("impulse", imp)
    add("DC", np.full(n, 0.7 - 0.2j))
    add("zeros", np.zeros(n))
    for k in range(-8, 31):
        add(f"tone x 1e{k}", tone * 10.0 ** k)
    return np.stack(fr).astype(np.complex64), names


N_NONFINITE = 2
I_ZERO = 7


def oracle_rows(x, c128=False):
    return np.stack(O.map_frames(O.compute_fft_c128 if c128 else O.compute_fft, list(x)))


def spectrum(x, exact):
    e = G.engine()
    nf, n = x.shape
    e.set_option("db_exact", int(exact))
    try:
        d_db = G.empty((nf, n), torch.float32)
        e.spectrum_db(G.dev(x), nf, n, d_db)
        e.sync()
    finally:
        e.set_option("db_exact", 0)
    return G.host(d_db)


def fail_msg(what, n, bad, names, frame0=0):
    f, k, cnt = bad
    name = names[f] if names is not None else ""
    return f"{family(n)} n={n} {what}: frame {frame0 + f} ({name}) bin {k} is the first of {cnt} values outside the bound"


def check_nonfinite(got, n, what, nan_rows, inf_rows):
    for f in nan_rows:
        assert np.isnan(got[f]).all(), f"{family(n)} n={n} {what}: the NaN-sample frame {f} is not all NaN"
    for f in inf_rows:
        assert not np.isfinite(got[f]).any(), f"{family(n)} n={n} {what}: the Inf-sample frame {f} has finite values"


def check_rows(kind, got, x, ref, n, what, names=None, window=True):
    e = SB.db_allowance(ref, SB.delta(x, window))
    chk = {"f64": SB.check_f64, "exact": SB.check_exact, "fast": SB.check_fast}[kind]
    bad = chk(got, ref, e)
    assert bad is None, fail_msg(what, n, bad, names)


# ---- pss_spectrum_db: every family, default and db_exact rows ------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_spectrum_db_rows_to_float64_accuracy(n):
    x, names = inputs(n)
    ref = oracle_rows(x)
    fin = slice(N_NONFINITE, None)
    for exact in (0, 1):
        got = spectrum(x, exact)
        what = "db_exact rows" if exact else "default rows"
        check_nonfinite(got, n, what, [0], [1])
        check_rows("exact" if exact else "fast", got[fin], x[fin], ref[fin], n, what, names[fin])
        assert np.all(ref[I_ZERO] == -100.0)
        if exact:
            assert np.all(got[I_ZERO] == np.float32(-100.0)), f"{family(n)} n={n}: db_exact row of an all-zero frame is not exactly -100.0f"


def test_large_amplitude_default_rows_are_finite():
    """|X|^2 past FLT_MAX (amplitude 1e20 at 1024 points): the default dB evaluation gave +inf; the reference row is finite (~425 dB)."""
    n = 1024
    x = (np.exp(2j * np.pi * 100 * np.arange(n) / n) * 1e20).astype(np.complex64)[None]
    ref = oracle_rows(x)
    got = spectrum(x, 0)
    assert np.isfinite(ref).all() and ref.max() > 385
    assert np.isfinite(got).all(), f"default rows: {np.count_nonzero(~np.isfinite(got))} of {n} values not finite"
    check_rows("fast", got, x, ref, n, "default rows, amplitude 1e20")


def test_compute_fft_one_sample():
    """compute_fft of a one-sample buffer: np.hamming(1) == [1.0], so the row is [10 log10(|x|^2 + 1e-10)]."""
    from pyspecsdr_amd import signal_processing as sp
    for v in (0.5 - 0.25j, 0.0, 3e20 + 0j, 1e-6j):
        x = np.array([v], np.complex64)
        got = sp.compute_fft(x)
        ref = O.compute_fft(x)
        assert got.shape == (1,)
        check_rows("fast", got[None], x[None], ref[None], 1, f"compute_fft([{v}])")
    x, names = inputs(1)
    got = spectrum(x, 1)
    ref = oracle_rows(x)
    check_nonfinite(got, 1, "db_exact rows", [0], [1])
    check_rows("exact", got[2:], x[2:], ref[2:], 1, "db_exact rows", names[2:])


# ---- one frame past each family's grid cap, the non-finite frames first in the walk ----------------------------------------------------
def _r16_cap(n):
    """Frames one pass of launch_r16's grid covers (pss_fft.hip, product build): the LDS-limited per_cu of the launch, capped by
    vgpr_cap = (split ? 4 : 2) * 256 / wg_threads, times 256 * 2 workgroups of fpw frames.  The LDS sizes are those of pss_r16::Cfg
    (pss_fft_r16.h): split (256 points) FPW * EX doubles, else fpw * EX complex, plus TW2 complex twiddles; 2048 points: one frame per
    128-thread workgroup.  test_grid_caps_are_those_of_the_launch_code pins the source lines this restates."""
    r3 = n // 256
    T = 16 * r3
    FPW = 256 // T
    e1 = T + (4 if r3 == 1 else r3 % 16)
    e2 = 256 + (2 if r3 == 1 else 8 // r3 if r3 <= 8 else 1)
    ex, tw2 = max(16 * e1, r3 * e2), r3 * 17
    split = n == 256
    fpw = 1 if n == 2048 else FPW
    lds = FPW * ex * 8 + tw2 * 16 if split else fpw * ex * 16 + tw2 * 16
    per_cu = max(1, min((160 * 1024) // (lds + 256), (4 if split else 2) * 256 // (fpw * T)))
    return 256 * per_cu * 2 * fpw


# The launch code these caps restate, as it reads in the source: a change to any of them fails test_grid_caps_are_those_of_the_launch_code.
LAUNCH_SOURCE = {
    "pss_fft.hip": [
        "long cap = 256L * per_cu * 4;",                                          # grid_for (generic k_spectrum)
        "if (per_cu > 8) per_cu = 8;",
        "int per_cu = (int)((160 * 1024) / (lds + 256));",                        # launch_r16
        "const int vgpr_cap = (split ? 4 : 2) * 256 / wg_threads;",
        "const long cap = 256L * per_cu * 2;",
        "constexpr bool split = LOG_R3 == 0, prefetch = LOG_R3 >= 1 && !(LOG_R3 == 4 && SCAN), one = LOG_R3 == 3 && !SCAN;",
        "const long cap = 256L * per_cu;",                                        # k_spectrum_xl: go(kern, lds, threads, per_cu)
        "return go(pss_xl::k_spectrum_xl<2, true, false, true>, pss_xl::CfgX<2>::LDS, 1024, 1);",
        "if (n_fft == 8192) return go(pss_xl::k_spectrum_xl<1, true>, pss_xl::CfgX<1>::LDS, 512, 2);",
        "return go(pss_xl::k_spectrum_xl<2, true>, pss_xl::CfgX<2>::LDS, 1024, 1);",
        "const long cap = 512;  // workgroups",                                  # k_spectrum_r16_big
        "dim3((unsigned)(total1 < 8192 ? total1 : 8192))",                        # k_huge_p1, Bluestein's k_huge_p1_g
        "dim3((unsigned)(groups < 8192 ? groups : 8192))",                        # k_huge_p2
        "long chunk = (long)(((size_t)1 << 30) / (M * sizeof(double2)));",       # Bluestein batch chunks (>= the frames below)
    ],
    "pss_fft_r16.h": [
        "static constexpr int E1_STRIDE = T + (R3 == 1 ? 4 : R3 % 16);",
        "static constexpr int E2_STRIDE = 256 + (R3 == 1 ? 2 : R3 <= 8 ? 8 / R3 : 1);",
        "static constexpr int TW2S = 17;",
        "static constexpr int EX = (16 * E1_STRIDE > R3 * E2_STRIDE) ? 16 * E1_STRIDE : R3 * E2_STRIDE;",
    ],
}


def test_grid_caps_are_those_of_the_launch_code():
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyspecsdr_amd", "csrc")
    for fname, lines in LAUNCH_SOURCE.items():
        src = open(os.path.join(csrc, fname)).read()
        for line in lines:
            assert line in src, f"{fname} no longer reads '{line}': update GRID_CAPS / _r16_cap to the new launch grid"
    assert [_r16_cap(n) for n in (256, 512, 1024, 2048, 4096)] == [24576, 8192, 4096, 2048, 1024]


GRID_CAPS = [                      # (n, frames one pass of the grid covers at most, from the launch code)
    (16, 256 * 8 * 4),             # k_spectrum: grid_for(n_frames, per_cu <= 8) = 256 * per_cu * 4 workgroups, one frame each
    (128, 256 * 8 * 4),
    (256, _r16_cap(256)), (512, _r16_cap(512)), (1024, _r16_cap(1024)), (2048, _r16_cap(2048)), (4096, _r16_cap(4096)),
    (8192, 256 * 2),               # k_spectrum_xl<1>: 256 * per_cu(2) workgroups, one frame each
    (16384, 256 * 1),              # k_spectrum_xl<2>
    (32768, 512), (65536, 512),    # k_spectrum_r16_big: 512 workgroups (each owns N float64 of scratch)
    (1 << 20, 8192 * 1 // 256),    # k_huge_p2<4>: 8192 workgroups of one 4096-point row, 256 rows per frame (k_huge_p1: 8192 / 256 too)
    (65537, 8192 * 16 // 1024),    # Bluestein M = 2^18: k_huge_p1_g 8192 workgroups of 16 columns, NS = 1024 columns per frame
    (240000, 8192 * 16 // 2048),   # Bluestein M = 2^19
]


def _cap_batch(n, nf):
    rng = np.random.default_rng(n + nf)
    t = np.arange(n)
    bins = rng.integers(0, n, nf)[:, None]
    x = np.exp(2j * np.pi * (bins + rng.random((nf, 1))) * t / n) + 1e-3 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))
    x[0, n // 2] = np.nan
    x[1, n // 3] = np.inf
    return x.astype(np.complex64)


@pytest.mark.parametrize("n,cap", GRID_CAPS)
def test_spectrum_db_past_the_grid_cap(n, cap):
    nf = cap + 2                               # frames cap and cap + 1 follow the NaN / Inf frames in workgroups 0 and 1
    assert nf > cap
    x = _cap_batch(n, nf)
    ref = oracle_rows(x)
    for exact in (0, 1):
        got = spectrum(x, exact)
        what = f"{'db_exact' if exact else 'default'} rows, {nf} frames"
        check_nonfinite(got, n, what, [0], [1])
        e = SB.db_allowance(ref[2:], SB.delta(x[2:]))
        bad = (SB.check_exact if exact else SB.check_fast)(got[2:], ref[2:], e)
        assert bad is None, fail_msg(what, n, bad, None, frame0=2)


# ---- the float64-row entry points -----------------------------------------------------------------------------------------------------
F64_CASES = [(n, 0) for n in F64_LENGTHS] + [(n, 1) for n in (256, 512, 1024, 2048, 4096)]


@pytest.mark.parametrize("n,plain", F64_CASES)
def test_spectrum_db_f64_rows(n, plain):
    e = G.engine()
    x, names = inputs(n)
    ref = oracle_rows(x)
    e.set_option("f64_plain", plain)
    try:
        d_db = G.empty(x.shape, torch.float64)
        e.spectrum_db_f64(G.dev(x), len(x), n, d_db)
        e.sync()
    finally:
        e.set_option("f64_plain", 0)
    got = G.host(d_db)
    what = f"spectrum_db_f64 (f64_plain {plain})"
    check_nonfinite(got, n, what, [0], [1])
    check_rows("f64", got[2:], x[2:], ref[2:], n, what, names[2:])


@pytest.mark.parametrize("n", F64_LENGTHS)
def test_spectrum_db_c128_rows(n):
    e = G.engine()
    x, names = inputs(n)
    x = x.astype(np.complex128)
    x[2:] += 1e-9 * x[2:]                       # samples that complex64 cannot hold
    ref = oracle_rows(x, c128=True)
    d_db = G.empty(x.shape, torch.float64)
    e.spectrum_db_c128(torch.from_numpy(np.ascontiguousarray(x).view(np.float64)).cuda(), len(x), n, d_db)
    e.sync()
    got = G.host(d_db)
    check_nonfinite(got, n, "spectrum_db_c128", [0], [1])
    check_rows("f64", got[2:], x[2:], ref[2:], n, "spectrum_db_c128", names[2:])


@pytest.mark.parametrize("n", [16, 1024, 4096, 65536, 1001])
def test_spectrum_db_post_rows(n):
    """pss_spectrum_db_post's dB rows (finite frames: the post-process behind it is tested elsewhere)."""
    e = G.engine()
    x, names = inputs(n)
    x, names = x[2:], names[2:]
    ref = oracle_rows(x)
    d_db, d_post = G.empty(x.shape, torch.float32), G.empty((len(x), n - 4), torch.float32)
    e.spectrum_db_post(G.dev(x), len(x), n, d_db, d_post)
    e.sync()
    check_rows("fast", G.host(d_db), x, ref, n, "spectrum_db_post rows", names)


@pytest.mark.parametrize("n", [16, 256, 1024, 2048, 65536])
def test_spectrum_cells_rows(n):
    """pss_spectrum_cells' float64 and float32 rows (1024 points: the fused k_spectrum_post); finite frames, as the display needs."""
    e = G.engine()
    x, names = inputs(n)
    x, names = x[2:], names[2:]
    nf = len(x)
    ref = oracle_rows(x)
    d32, d64 = G.empty((nf, n), torch.float32), G.empty((nf, n), torch.float64)
    lo, hi = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
    la, lb = G.empty((nf, 112), torch.int8), G.empty((nf, 112), torch.int8)
    e.spectrum_cells(G.dev(x), nf, n, d32, d64, lo, hi, 112, la, lb)
    e.sync()
    check_rows("f64", G.host(d64), x, ref, n, "spectrum_cells db64", names)
    check_rows("exact", G.host(d32), x, ref, n, "spectrum_cells db32", names)


# ---- the compute_fft shim and the scanner ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 1000, 1024, 4097, 65536, 1 << 20])
def test_compute_fft_shim_rows(n):
    from pyspecsdr_amd import signal_processing as sp
    x, names = inputs(n)
    for i in (2, 5, I_ZERO, 8, 8 + 8 + 20, len(x) - 1):          # tone, impulse, zeros, 1e-8, 1e20, 1e30
        got = sp.compute_fft(x[i])
        check_rows("fast", got[None], x[i][None], O.compute_fft(x[i])[None], n, f"compute_fft ({names[i]})")


@pytest.mark.parametrize("n", [16, 128, 256, 1024, 2048, 4096, 8192, 16384])
def test_scanner_rows_amplitude_sweep(n):
    """pss_scan / pss_scan_threshold rows (NumPy's float32 chain) against the oracle's, every value, over the amplitude sweep: within
    scan_ulp_bound (the float32 chain) plus the dB allowance of the reference's own complex64 transform (delta_f32_reference), which the
    device's float64 transform does not reproduce: on the bins far below a row's peak that rounding is all the reference row holds.
    Non-finite values (|X|^2 past FLT_MAX in the float32 chain) must match exactly."""
    e = G.engine()
    fs = 2.4e6
    x, names = inputs(n)
    x, names = x[2:], names[2:]
    nf = len(x)
    want = np.stack([r[0] for r in O.map_frames(lambda v: O.scan_slice(v, fs), list(x))]).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        allow = SB.scan_ulp_bound(want) + SB.db_allowance(np.where(np.isfinite(want), want, 0.0), SB.delta_f32_reference(x))
    for thr in (None, -30.0):
        db, pk = G.empty((nf, n), torch.float32), G.empty((nf,), torch.float32)
        bw, cnt = G.empty((nf,), torch.float64), G.empty((nf,), torch.int32)
        if thr is None:
            e.scan(G.dev(x), nf, n, fs, db, pk, bw, cnt)
        else:
            e.scan_threshold(G.dev(x), nf, n, fs, thr, db, pk, bw, cnt)
        e.sync()
        got = G.host(db).astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = np.where(np.isfinite(want), np.abs(got - want) <= allow, (got == want) | (np.isnan(got) & np.isnan(want)))
        bad = np.argwhere(~ok)
        assert len(bad) == 0, (f"{'scan' if thr is None else 'scan_threshold'} n={n}: frame {bad[0][0]} ({names[bad[0][0]]}) bin "
                               f"{bad[0][1]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]} ({len(bad)} values)")


# ---- batches of one and three frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_spectrum_db_one_and_three_frames(n):
    """nf = 1 (a tone with noise) and nf = 3 (a NaN-sample frame first, then that tone and a tone at 1e25) through every family."""
    x, names = inputs(n)
    pick = {1: [2], 3: [0, 2, 8 + 8 + 25]}
    for nf, idx in pick.items():
        xs, nm = x[idx], [names[i] for i in idx]
        ref = oracle_rows(xs)
        fin = [i for i in range(nf) if np.isfinite(xs[i]).all()]
        for exact in (0, 1):
            got = spectrum(xs, exact)
            what = f"{'db_exact' if exact else 'default'} rows, nf = {nf}"
            check_nonfinite(got, n, what, [i for i in range(nf) if i not in fin], [])
            check_rows("exact" if exact else "fast", got[fin], xs[fin], ref[fin], n, what, [nm[i] for i in fin])

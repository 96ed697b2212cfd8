"""Error bounds for compute_fft's dB rows (signal_processing.py:243-264), shared by the spectrum tests.

The reference computes the row in float64: a complex64 frame times np.hamming is complex128, np.fft.fft transforms it, and
10 log10(|X|^2 + 1e-10) is evaluated in float64.  The device rows are held to what float64 arithmetic can promise about that row,
bin by bin, and not to the 1e-4 relative contract alone, which a float32 window or a float32 intermediate in a transform still meets.

Transform allowance (per bin, in the transform's own units): delta = KAPPA * log2(M) * 2^-53 * ||X||_2, where
  - M is the length actually transformed: n for the power-of-two kernels, the Bluestein length 256 * NS for the others;
  - ||X||_2 = sqrt(n * sum |w x|^2) (Parseval; computed from the input in float64);
  - a bin's error is at most the norm of the whole error vector, so delta bounds every bin.

KAPPA comes from the standard norm-wise bound for Cooley-Tukey FFTs (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
Theorem 24.2): with twiddles accurate to mu, the computed transform satisfies ||dX||_2 <= log2(M) * eta * ||X||_2 to first order, with
eta = mu + gamma_4 (sqrt(2) + mu), gamma_4 = 4u / (1 - 4u), u = 2^-53.  A radix-4 or radix-16 stage is two or four radix-2 levels
whose inner twiddles are exactly +-1, +-i, so the same log2(M) levels carry the same eta.  Per side:
  - the device's tables (pss_fft_tables): the angle fl(2 pi) k / n is exact but for the rounding of pi, <= 2.2u absolute; cos / sin
    add 0.5u each: mu_dev = 4u;
  - the oracle's pocketfft tables are correctly rounded: mu_ora = 1u;
  - the window product w x: np.hamming's 0.54 - 0.46 cos(.) is accurate to ~1u absolute, at most 7u relative at its 0.08 ends, and
    the product rounds once: ||d(w x)|| <= 8u ||w x||, which the unitary-scaled DFT carries into ||dX|| <= 8u ||X|| <= 2u log2(M) ||X||
    for M >= 16.
Both rows err, so the allowance on their difference is the sum of the two sides:
  KAPPA = (eta(4u) + 2u) / u + (eta(1u) + 2u) / u = 11.66 + 8.66 -> 21 (rounded up).

Bluestein (lengths 2-15 and every non-power of two): the row is chirp * IFFT_M(FFT_M(x c) * B) / M, three M-point transforms.  An
error eps ||A|| in A = FFT_M(x c) reaches the convolution scaled by max|B| / sqrt(M), and the inverse transform adds the same; B is
computed once from a chirp of unit modulus and is taken to be accurate component-wise to the same eps.  So delta is multiplied by
BETA = 3 max|B| / sqrt(n); max|B| is computed here from the same chirp in float64 (2.0-2.5 sqrt(n) for every n).

In dB the allowance is exact, not linearised: 10 log10 moves by at most
  e_k = 10 / ln 10 * max(ln(((|X_k| + delta)^2 + f) / (|X_k|^2 + f)), ln((|X_k|^2 + f) / (max(|X_k| - delta, 0)^2 + f))),  f = 1e-10,
with |X_k|^2 = 10^(ref_k / 10) - f from the oracle row.  To first order this is 20 / ln 10 * |X_k| delta / (|X_k|^2 + f), finite on the
-100 dB floor; the exact form also holds where delta^2 is not small beside f (large amplitudes beside a near-zero bin).  Added to it is
the evaluation of 10 log10(|X|^2 + 1e-10) on both sides in float64: |X|^2 + f rounds within 3u (both sides), log10 within 1 ulp of its
value (both sides): EVAL(ref) = 10 / ln 10 * 6u + 4u |ref|.

Row types:
  - float64 rows (spectrum_db_f64, spectrum_db_c128, spectrum_cells db64, frame_pipeline_f64):  |got - ref| <= e_k;
  - db_exact rows: got in [f32(ref - e_k), f32(ref + e_k)]: the float32 rounding of a value within float64 accuracy of the row;
  - default rows (db_of_fast, pss_fft_r16.h): |got - ref| <= e_k + fast_allowance(ref), below.
"""
import math

import numpy as np

U = 2.0 ** -53
U24 = 2.0 ** -24
DB_PER_NEPER = 10.0 / math.log(10.0)      # d(10 log10 p) / d(ln p)
FLOOR = 1e-10


def _eta(mu_units):
    g4 = 4 * U / (1 - 4 * U)
    return (mu_units * U + g4 * (math.sqrt(2.0) + mu_units * U)) / U


KAPPA = math.ceil((_eta(4) + 2) + (_eta(1) + 2))   # 21


def is_pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def bluestein(n):
    """True where pss_spectrum_db takes Bluestein's algorithm (lengths 2-15 and every non-power of two)."""
    return n >= 2 and not (is_pow2(n) and n >= 16)


def transform_len(n):
    """The length the device transforms: n, or Bluestein's M = 256 NS >= 2n - 1, at least 2^17 (pss_fft.hip bs_plan)."""
    if not bluestein(n):
        return n
    m = 1 << 17
    while m < 2 * n - 1:
        m <<= 1
    return m


_BETA = {}


def bluestein_beta(n):
    """3 max|B| / sqrt(n), B the M-point transform of the wrapped conjugate chirp (computed in float64)."""
    if n not in _BETA:
        m = transform_len(n)
        k = np.arange(n, dtype=np.float64)
        c = np.exp(-1j * np.pi * ((k * k) % (2 * n)) / n)
        b = np.zeros(m, np.complex128)
        b[:n] = np.conj(c)
        b[m - n + 1:] = np.conj(c[1:][::-1])
        _BETA[n] = 3.0 * float(np.abs(np.fft.fft(b)).max()) / math.sqrt(n)
    return _BETA[n]


def delta(x, window=True):
    """Per-frame transform allowance delta for frames x [nf, n] (any complex type); NaN for frames that are not finite."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    n = x.shape[1]
    w = np.hamming(n) if window else np.ones(n)
    xw = x.astype(np.complex128) * w
    with np.errstate(invalid="ignore", over="ignore"):
        sumsq = np.sum(xw.real ** 2 + xw.imag ** 2, axis=1)
    norm = np.sqrt(n * sumsq)
    m = transform_len(n)
    d = KAPPA * max(math.log2(m), 1.0) * U * norm
    if bluestein(n):
        d = d * bluestein_beta(n)
    return d


KAPPA_F32 = math.ceil(_eta(1) + 1)   # 8: NumPy's complex64 pocketfft (correctly rounded twiddles), in units of 2^-24; + 1 for the other side


def delta_f32_reference(x):
    """Transform allowance of the scanner's reference row, NumPy's complex64 fft of the unwindowed slice: the same norm-wise bound in
    float32 (u = 2^-24; the complex64 samples enter exactly), KAPPA_F32 log2(n) 2^-24 ||X||_2.  The device's float64 transform errs
    2^-29 times less, inside the + 1 of KAPPA_F32."""
    x = np.asarray(x)
    n = x.shape[1]
    xd = x.astype(np.complex128)
    norm = np.sqrt(n * np.sum(xd.real ** 2 + xd.imag ** 2, axis=1))
    return KAPPA_F32 * max(math.log2(n), 1.0) * U24 * norm


def eval_allowance(ref):
    return DB_PER_NEPER * 6 * U + 4 * U * np.abs(ref)


def db_allowance(ref, d):
    """e_k for oracle rows ref [nf, n] (float64) and per-frame transform allowances d [nf]."""
    ref = np.asarray(ref, np.float64)
    d = np.asarray(d, np.float64).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.maximum(np.power(10.0, ref / 10.0) - FLOOR, 0.0)       # |X_k|^2
        a = np.sqrt(p)
        lo = np.maximum(a - d, 0.0)
        up = np.log1p((2 * a * d + d * d) / (p + FLOOR))
        dn = np.log((p + FLOOR) / (lo * lo + FLOOR))
        e = DB_PER_NEPER * np.maximum(up, dn)
    return e + eval_allowance(ref)


def fast_allowance(ref):
    """db_of_fast's float32 evaluation (pss_fft_r16.h), from its operations; u24 = 2^-24.

    Far branch (|pw - 1| >= 0.25): (float)pw rounds by u24 relative, 10 / ln 10 * u24 dB absolute; v_log_f32 (__log2f) is accurate
    to 1 ulp of its result, 2 u24 relative; the constant 3.0102999566398120f is 0.2 u24 off 10 log10 2; the product rounds: 1 u24.
    Relative 3.2 u24 of |ref|.
    Near branch (|t| < 0.25, t = (float)(pw - 1)): s = t / (2 + t) from three roundings and v_rcp_f32 (1 ulp): 5 u24, amplified at
    most 1.16 x through t / (2 + t); the atanh series 2 s (1 + s^2 / 3 + ... + s^8 / 9) truncates at 2 s^11 / 11 (< 3e-10 relative for
    |s| < 1/7) and its outermost fma rounds once (the inner ones are damped by s^2 <= 0.02: 0.1 u24); p = s q rounds; the constant
    4.342944819032518f is 0.76 u24 off 10 / ln 10; the product rounds: 9.7 u24 relative.
    Overflow (pw past the float32 range, amplitudes above ~3e16 at 1024 points): log2 pw = __log2f((float)(pw 2^-200)) + 200: the
    scaling is exact, (float) rounds by u24 relative (u24 / ln 2 absolute in log2), __log2f of a value below 2^96 errs by 1 ulp <= 2^-17
    absolute, the sum (>= 128) rounds by u24 relative, the constant and the product as above: 3.5 u24 relative of |ref|.
    A(ref) = 10 / ln 10 * u24 + 12 u24 |ref|, never looser than the golden test's 1e-6 max(|ref|, 1)."""
    return DB_PER_NEPER * U24 + 12 * U24 * np.abs(np.asarray(ref, np.float64))


def _first_bad(ok):
    """(frame, bin) of the first False in ok [nf, n], or None."""
    bad = np.argwhere(~ok)
    return None if len(bad) == 0 else (int(bad[0][0]), int(bad[0][1]), int(len(bad)))


def _same_nonfinite(got, ref):
    return (np.isnan(got) & np.isnan(ref)) | (np.isinf(got) & (got == ref))


def check_f64(got, ref, e):
    """float64 rows: |got - ref| <= e.  Returns None or (frame, bin, count of offending values)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(got - ref) <= e) | _same_nonfinite(got, ref)
    return _first_bad(ok)


def check_exact(got, ref, e):
    """db_exact rows (float32): got in [f32(ref - e), f32(ref + e)]."""
    g = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = ((g >= (ref - e).astype(np.float32)) & (g <= (ref + e).astype(np.float32))) | _same_nonfinite(g.astype(np.float64), ref)
    return _first_bad(ok)


def check_fast(got, ref, e):
    """Default float32 rows: |got - ref| <= e + fast_allowance(ref)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(got - ref) <= e + fast_allowance(ref)) | _same_nonfinite(got, ref)
    return _first_bad(ok)


def exact_rows_bad(got, ref, rel=1e-12):
    """db_exact rows: frames with a float32 value outside [float32(ref - d), float32(ref + d)], d = rel * max(|row|, 1) — the float32
    rounding of a value within float64 accuracy of the oracle's row.  Bit equality with float32(ref) holds on every golden row
    (test_spectrum_db_exact_is_the_float32_rounding_of_the_reference_rows), but not on every value of 134 million: two float64
    transforms agree to ~1e-16 of the row's LARGEST bin, so a value near 0 dB (a bin of power ~1 beside a 73 dB peak), whose float32
    ulp is far finer than that, can round to the neighbouring float32 value.  Measured on cfg 3's 8192 x 16 384 AM rows: 75 values in
    75 frames (93, 193, 267, ...), each 1 float32 ulp from float32(ref), the oracle's value at most 1.4e-12 dB from the float32
    rounding midpoint (20 ppt of the row's peak) in the 40 inspected; the bound is 1e-12 of the row's peak."""
    g = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        d = rel * np.maximum(np.nanmax(np.abs(ref.reshape(len(ref), -1)), axis=1), 1.0).reshape((-1,) + (1,) * (ref.ndim - 1))
        ok = ((g >= (ref - d).astype(np.float32)) & (g <= (ref + d).astype(np.float32))) | (np.isnan(g) & np.isnan(ref))
    return np.nonzero(~ok.reshape(len(g), -1).all(axis=1))[0]


def scan_ulp_bound(ref):
    """One float32 ulp in a spectrum component moves 10 log10(|X|^2 + 1e-10) by up to 20 / ln 10 * 2^-23 ~ 1.04e-6 dB: two ulp of the
    dB value where |dB| >= 4, more below (a 1-ulp component at -1.83 dB moved the value by 8 ulp, slice 4860 of 8192 x 4096).  The
    bound is two ulp of max(|dB|, 4): the 2-ulp rule of the per-family test wherever its argument holds, the same absolute 9.5e-7 dB
    below."""
    return 2.0 * np.spacing(np.maximum(np.abs(np.asarray(ref, np.float32)), np.float32(4.0))).astype(np.float64)

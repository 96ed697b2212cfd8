"""Error bounds for the capture survey's rows (pss_welch: Welch's mean row and the max-hold row), shared by the survey's tests; written
in the manner of spectrum_bounds.py, whose KAPPA and eta it takes.

The truth is scipy.signal.welch / spectrogram(mode='psd').max(-1) on the capture widened to complex128: float64 throughout.  Both sides
compute, per segment s, v = (x - m_s) w, X = DFT_N(v), p_s[k] = |X_k|^2, then mean[k] = (sum_s p_s[k] / L) scale and
max[k] = max_s p_s[k] scale.  With u = 2^-53:

Per segment, the spectrum.  |dX_k| <= delta_s = KAPPA log2(N) u sqrt(N sum |w (x - m_s)|^2) + delta_mean.  The first term is
spectrum_bounds' norm-wise transform allowance (Higham, Theorem 24.2; Parseval), KAPPA = 21 covering the device's tables (4u) and
pocketfft's (1u) together with 2u a side for the input product: here the window is the caller's float64 table on both sides, the
subtraction and the product round once each, ||dv|| <= 2u ||v||, inside that 2u log2(N) for N >= 16.  delta_mean is the allowance for the
two sides' segment means: a sum of N terms in ANY order errs by at most (N - 1) u sum |x_i| (Higham, section 4.2), the mean by 1 / N of
it, and the division rounds once more (u |m|; exact on the device, where 1 / N is a power of two); real and imaginary parts each, so the
complex mean errs by at most sqrt(2) ((N - 1) / N u sum |x_i| + u |m|) a side.  A mean off by e moves X_k by e W_k, |W_k| <= sum |w|.  Both sides:
  delta_mean = 2 sqrt(2) ((N - 1) / N sum |x_i| + |m|) u sum |w|       (0 without detrend).

Per segment, the power.  p = re^2 + im^2 rounds three times at most (two products and a sum, or a product and a fused multiply-add):
  E_s[k] = 2 |X_k| delta_s + delta_s^2 + 3u |X_k|^2.

The mean of L nonnegative terms.  Any summation order adds at most (L - 1) u relative to the terms' sum (all terms >= 0: sum |p| is the
sum), on either side: 2 (L - 1) u together.  The division by L and the product with scale round once each on either side: 4u.
  B_mean[k] = scale (sum_s E_s[k] / L + (2 (L - 1) + 4) u sum_s p_s[k] / L).
The max.  |max_s a_s - max_s b_s| <= max_s |a_s - b_s|; the product with scale rounds once a side (SciPy scales before it takes the max,
which commutes with a positive scale up to that rounding):
  B_max[k] = scale (max_s E_s[k] + 2u max_s p_s[k]).

Device against host twin: the same with the device's table accuracy (4u) on both sides, KAPPA_TWIN = ceil(2 (eta(4) + 2)) = 24; both
sides add the mean in the same order, the allowance for it is kept (it only loosens the bound by its small term).

|X_k| and the norms are computed here in float64 from the capture (NumPy's fft); their own error moves the bound by a relative 1e-15 and
is ignored, as in spectrum_bounds.  Rows with a NaN are outside the bound (the tests state their rule separately).
"""
import math

import numpy as np

from spectrum_bounds import KAPPA, U, _eta

KAPPA_TWIN = math.ceil(2 * (_eta(4) + 2))   # 24


def segments(x, N, S):
    """The L segments of a row as a view [L][N]."""
    x = np.asarray(x)
    L = (len(x) - N) // S + 1
    return np.lib.stride_tricks.as_strided(x, shape=(L, N), strides=(S * x.strides[0], x.strides[0]), writeable=False)


def restate(x, N, S, w, detrend, scale):
    """A plain NumPy restatement and the bounds' ingredients for one row x (complex64) ->
    dict(mean, max, p [L][N] unscaled powers, delta [L])."""
    seg = segments(np.asarray(x, np.complex64), N, S).astype(np.complex128)
    L = len(seg)
    w = np.asarray(w, np.float64)
    if detrend:
        m = seg.mean(axis=1, keepdims=True)
        v = (seg - m) * w
        d_mean = 2 * math.sqrt(2.0) * ((N - 1) / N * np.abs(seg).sum(axis=1) + np.abs(m[:, 0])) * U * np.abs(w).sum()
    else:
        v = seg * w
        d_mean = np.zeros(L)
    X = np.fft.fft(v, axis=1)
    p = X.real ** 2 + X.imag ** 2
    norm = np.sqrt(N * np.sum(v.real ** 2 + v.imag ** 2, axis=1))
    return dict(mean=p.sum(axis=0) / L * scale, max=p.max(axis=0) * scale, p=p, norm=norm, d_mean=d_mean, L=L)


def bounds(R, N, scale, kappa=KAPPA):
    """(B_mean [N], B_max [N]) from restate()'s result."""
    p, L = R["p"], R["L"]
    delta = (kappa * math.log2(N) * U * R["norm"] + R["d_mean"])[:, None]
    E = 2 * np.sqrt(p) * delta + delta * delta + 3 * U * p
    b_mean = scale * (E.sum(axis=0) / L + (2 * (L - 1) + 4) * U * p.sum(axis=0) / L)
    b_max = scale * (E.max(axis=0) + 2 * U * p.max(axis=0))
    return b_mean, b_max


def fraction(got, ref, bound):
    """The worst |got - ref| / bound over the bins (inf where a value is not finite or a bound is not positive)."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    if got.shape != ref.shape or not (np.all(np.isfinite(got)) and np.all(np.isfinite(ref)) and np.all(bound > 0)):
        return math.inf
    return float(np.max(np.abs(got - ref) / bound))

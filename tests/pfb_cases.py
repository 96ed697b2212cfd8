"""Captures and cases of the polyphase channeliser's fixtures — shared by tools/make_goldens_pfb.py, tests/test_pfb_golden.py and
tests/test_gpu_pfb.py (-m gpu).  NumPy only.

The fixture (tests/golden/pfb.npz) stores results, never captures: every capture and every tap table is regenerated here from its seed
and pinned by a CRC.  The truth in it is the definition, y_c[m] = sum over k of h[k] x[m D + lead - k] exp(-2 pi i c j / M), evaluated
directly in np.longdouble (80-bit) with the phase reduced exactly, (c j) mod M in integers before any float.
"""
import zlib

import numpy as np

VERSION = 1

# (name, M, D, T, n, lead, instants, channels): instants / channels None = all of them.  (8, 3, 50): D does not divide M; (8, 8, 1): one tap;
# (8, 1, 17): no decimation; (1024, 512, 20481): the largest bank with its default tap count, on a subset of instants (first, last, middle)
# and channels (0, 1, the band edge and its neighbours, the last, one in between).
CASES = [
    ("m2", 2, 2, 5, 101, 2, None, None),
    ("m4", 4, 4, 81, 403, 40, None, None),
    ("m8_d4", 8, 4, 161, 801, 80, None, None),
    ("m8_d3", 8, 3, 50, 500, 13, None, None),
    ("m8_t1", 8, 8, 1, 203, 0, None, None),
    ("m8_d1", 8, 1, 17, 150, 16, None, None),
    ("m64", 64, 32, 1281, 2501, 640, None, None),
    ("m1024", 1024, 512, 20481, 40001, 10240, (0, 1, 19, 20, 21, 39, 40, 77, 78), (0, 1, 300, 511, 512, 513, 1023)),
]
TAP_CHANS = [2, 64, 1024]                  # pss_pfb_default_taps against SciPy's firwin(20 M + 1, 1 / M), bit for bit

# the chain test's capture: two NFM stations in one 2.4 MS/s capture, on the grid of the M = 64 bank
CHAIN_FS = 2.4e6
CHAIN_M = 64
CHAIN_D = 32
CHAIN_N = 6144 * 32                      # 6144 samples a row at 75 kS/s: 2048 audio samples at 25 kS/s
CHAIN_SEED = 20261019
CHAIN_STATIONS = ((600e3, 16, 1000.0), (-600e3, 48, 2500.0))   # (offset from the centre, its row, tone), 5 kHz deviation each
CHAIN_DEVIATION = 5e3
CHAIN_SIGMA = 0.01


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


def capture(n, seed):
    """A wideband capture: noise, three carriers and a chirp, amplitude about 1, complex64."""
    rng = np.random.default_rng([51, int(n), int(seed)])
    t = np.arange(n)
    x = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, a in ((0.125, 0.5), (-0.31, 0.4), (0.02, 0.3)):
        x = x + a * np.exp(2j * np.pi * (f * t + rng.uniform()))
    x = x + 0.2 * np.exp(2j * np.pi * (0.1 * t + 0.15 * t * t / max(n, 1)))
    return x.astype(np.complex64)


def case(name):
    for i, c in enumerate(CASES):
        if c[0] == name:
            return i, c
    raise KeyError(name)


def case_capture(name):
    i, c = case(name)
    return capture(c[4], i)


def case_taps(name):
    """A low-pass of the case's length: a Hamming-windowed sinc at 1 / M, scaled to unit sum, with a seeded ripple of 1e-3 so that no two
    taps are equal (a symmetric table would hide a reversed index)."""
    i, (_, M, _, T, _, _, _, _) = case(name)
    rng = np.random.default_rng([52, i])
    k = np.arange(T) - (T - 1) / 2
    w = 0.54 + 0.46 * np.cos(2 * np.pi * k / max(T - 1, 1)) if T > 1 else np.ones(1)
    h = np.sinc(k / M) * w
    h = h / h.sum() + 1e-3 / T * rng.standard_normal(T)
    return np.ascontiguousarray(h, np.float64)


def case_instants(name):
    _, (_, _, D, _, n, _, instants, _) = case(name)
    return list(range(-(-n // D))) if instants is None else list(instants)


def case_channels(name):
    _, (_, M, _, _, _, _, _, channels) = case(name)
    return list(range(M)) if channels is None else list(channels)


def chain_capture():
    """Two NFM stations (1 kHz tone at +600 kHz, 2.5 kHz tone at -600 kHz, 5 kHz deviation) and noise of sigma 0.01 a part."""
    rng = np.random.default_rng(CHAIN_SEED)
    t = np.arange(CHAIN_N) / CHAIN_FS
    x = CHAIN_SIGMA * (rng.standard_normal(CHAIN_N) + 1j * rng.standard_normal(CHAIN_N))
    for off, _, tone in CHAIN_STATIONS:
        x = x + 0.5 * np.exp(1j * (2 * np.pi * off * t + (CHAIN_DEVIATION / tone) * np.sin(2 * np.pi * tone * t)))
    return x.astype(np.complex64)


def half_ulp32(v):
    """Half the spacing of float32 at |v| (float64 array in, float64 out)."""
    return 0.5 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def f64_units(M, T):
    """The float64 term of the output bound in units of 2^-53 sum|h| max(|xr|, |xi|): the chain's ceil(T / M) steps, log2 M butterfly
    stages of four roundings each (a table rounding among them), and 8."""
    return -(-T // M) + 4 * (M.bit_length() - 1) + 8


def bound_excess(y32, ref_hi, ref_lo, M, T, sum_abs_h, xmax):
    """The statement's output bound on each part: |float64(y32) - ref| <= 1/2 ulp_float32(max(|ref|, |y32|)) + f64_units 2^-53 sum|h| xmax,
    ref = ref_hi + ref_lo (the 80-bit truth as a float64 pair).
    -> (the largest error minus its bound over both parts — negative when every output is inside; the largest float64-part error
    |float64(y32) - ref| - 1/2 ulp in units of 2^-53 sum|h| xmax)."""
    y = np.asarray(y32).astype(np.complex128)
    unit = 2.0 ** -53 * sum_abs_h * xmax
    worst, used = -np.inf, -np.inf
    for a, hi, lo in ((y.real, ref_hi.real, ref_lo.real), (y.imag, ref_hi.imag, ref_lo.imag)):
        err = np.abs((a - hi) - lo)
        half = half_ulp32(np.maximum(np.abs(a), np.abs(hi)))
        worst = max(worst, float(np.max(err - (half + f64_units(M, T) * unit))))
        used = max(used, float(np.max(err - half)) / unit)
    return worst, used

"""Captures and cases of the down-converter fixtures — shared by tools/make_goldens_ddc.py, tests/test_ddc_golden.py and
tests/test_gpu_ddc.py (-m gpu).  NumPy only.

The fixture (tests/golden/ddc.npz) stores results, never captures: every capture is regenerated here from its seed and pinned by a CRC.
The truth in it is computed outside the library: exact integer phases, sine and cosine in np.longdouble (80-bit), SciPy's filters.
"""
import zlib

import numpy as np

VERSION = 1

# (name, D, n, zero_phase, offsets as fractions of fs).  D = 5 / n = 1003, D = 3 / n = 400 and D = 50 / n = 5000 are the shapes the
# statement's bound was first checked on; lf_* are the lead = 0 cases (lfilter(h, 1, z)[::D]) with the same SciPy taps.
CASES = [
    ("zp_d5", 5, 1003, True, (0.125, -0.1875)),
    ("zp_d3", 3, 400, True, (0.3, 0.0)),
    ("zp_d50", 50, 5000, True, (0.125, -0.31)),
    ("zp_d2", 2, 257, True, (0.5,)),
    ("zp_d7", 7, 1200, True, (-0.0421,)),
    ("zp_d64", 64, 6500, True, (0.21,)),
    ("lf_d5", 5, 1003, False, (0.125,)),
    ("lf_d50", 50, 5000, False, (-0.31,)),
]
TAP_DECIMS = [2, 3, 5, 7, 50, 64]          # pss_ddc_default_taps against SciPy's firwin, bit for bit

ROTOR_WORDS = [0, 1 << 62, 1 << 63, 1, (1 << 64) - 1]
N_RANDOM_WORDS = 16
N_ROTOR_INDICES = 256                       # per word: 0, 1, 2, 3, 2^62 and random indices below 2^62, 2^44 and 2^20

# the chain test's capture: two NFM stations in one 2.4 MS/s capture
CHAIN_FS = 2.4e6
CHAIN_D = 50
CHAIN_N = 4096 * 50
CHAIN_SEED = 20260131
CHAIN_STATIONS = ((300e3, 1000.0), (-450e3, 2500.0))   # (offset from the centre, tone), 5 kHz deviation each
CHAIN_DEVIATION = 5e3
CHAIN_SIGMA = 0.01


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


def capture(n, seed):
    """A wideband capture: noise, three carriers and a chirp, amplitude about 1, complex64."""
    rng = np.random.default_rng([21, int(n), int(seed)])
    t = np.arange(n)
    x = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, a in ((0.125, 0.5), (-0.31, 0.4), (0.02, 0.3)):
        x = x + a * np.exp(2j * np.pi * (f * t + rng.uniform()))
    x = x + 0.2 * np.exp(2j * np.pi * (0.1 * t + 0.15 * t * t / max(n, 1)))
    return x.astype(np.complex64)


def case_capture(name):
    for i, c in enumerate(CASES):
        if c[0] == name:
            return capture(c[2], i)
    raise KeyError(name)


def rotor_words():
    rng = np.random.default_rng([22, 1])
    return ROTOR_WORDS + [int(w) for w in rng.integers(0, 1 << 64, N_RANDOM_WORDS, dtype=np.uint64)]


def rotor_indices():
    rng = np.random.default_rng([22, 2])
    k = (N_ROTOR_INDICES - 5) // 3
    idx = [0, 1, 2, 3, 1 << 62]
    idx += [int(v) for v in rng.integers(0, 1 << 62, N_ROTOR_INDICES - 5 - 2 * k, dtype=np.int64)]
    idx += [int(v) for v in rng.integers(0, 1 << 44, k, dtype=np.int64)]
    idx += [int(v) for v in rng.integers(0, 1 << 20, k, dtype=np.int64)]
    return idx


def word_of(fraction):
    """The frequency word of offset / fs = fraction as pss_ddc_word defines it, in exact integers: the float64 quotient times 2^64,
    rounded to the nearest integer (ties to even), modulo 2^64."""
    from fractions import Fraction
    return round(Fraction(float(fraction)) * (1 << 64)) % (1 << 64)


def chain_capture():
    """Two NFM stations (1 kHz tone at +300 kHz, 2.5 kHz tone at -450 kHz, 5 kHz deviation) and noise of sigma 0.01 a part."""
    rng = np.random.default_rng(CHAIN_SEED)
    t = np.arange(CHAIN_N) / CHAIN_FS
    x = CHAIN_SIGMA * (rng.standard_normal(CHAIN_N) + 1j * rng.standard_normal(CHAIN_N))
    for off, tone in CHAIN_STATIONS:
        x = x + 0.5 * np.exp(1j * (2 * np.pi * off * t + (CHAIN_DEVIATION / tone) * np.sin(2 * np.pi * tone * t)))
    return x.astype(np.complex64)


def special_identity_input(n=300):
    """Finite float32 inputs for the exact identities: ordinary values, float32 subnormals, the largest and smallest normals, zeros."""
    rng = np.random.default_rng([23, int(n)])
    v = rng.standard_normal(2 * n).astype(np.float32)
    v[::7] = np.float32(1e-41) * rng.integers(1, 1000, len(v[::7])).astype(np.float32)     # subnormals
    v[3::11] = np.finfo(np.float32).max
    v[5::13] = -np.finfo(np.float32).tiny
    v[6::17] = 0.0
    return v.view(np.complex64).copy()


def half_ulp32(v):
    """Half the spacing of float32 at |v| (float64 array in, float64 out)."""
    return 0.5 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def bound_excess(y32, ref, n_taps, sum_abs_h, zmax):
    """The statement's output bound on each part: |float64(y32) - ref| <= 1/2 ulp_float32(max(|ref|, |y32|)) + (T + 8) 2^-53 sum|h| max|z|.
    -> (the largest error minus its bound over both parts — negative when every output is inside; the largest float64-part error
    |float64(y32) - ref| - 1/2 ulp, in units of the float64 term, i.e. the fraction of it that is used)."""
    y = np.asarray(y32).astype(np.complex128)
    f64 = (n_taps + 8) * 2.0 ** -53 * sum_abs_h * zmax
    worst, used = -np.inf, -np.inf
    for a, b in ((y.real, ref.real), (y.imag, ref.imag)):
        err = np.abs(a - b)
        half = half_ulp32(np.maximum(np.abs(a), np.abs(b)))
        worst = max(worst, float(np.max(err - (half + f64))))
        used = max(used, float(np.max(err - half)) / f64)
    return worst, used

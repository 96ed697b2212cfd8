"""Read buffers and rows of the FM-mono fixtures — shared by tools/make_goldens_fm_mono.py, tests/test_fm_mono_golden.py and
tests/test_gpu_fm_mono.py (-m gpu).  NumPy only.

decode_mono (signal_processing.py:331-359) takes n complex64 samples to ceil((n - 1) / 6) int16 samples.  LENGTHS walks the decimator's
edges: fewer samples than one output needs (2 .. 8), n - 1 one short of, at and one past multiples of 6 (13, 14; 61, 67, 68; 133, 134),
the filter's 127-tap span (127, 128), ordinary frames (1000, 1024, 4097) and both sides of the 256 KiB temporary size at which NumPy swaps
the operands of the NFM / WFM product (32 768, 32 769, 40 001) — decode_mono's product is not swapped at any of them.
"""
import hashlib

import numpy as np

LENGTHS = [2, 3, 7, 8, 13, 14, 61, 67, 68, 127, 128, 133, 134, 1000, 1024, 4097, 32768, 32769, 40001]
LONG = 32768                       # from here on the fixture holds digests and the first and last EDGE values instead of the arrays
EDGE = 64
RATES = [250e3, 1.024e6, 2.4e6]
SPECIAL_N = 1600
SPECIALS = ["zeros", "nan", "negzero", "tiny", "wrap"]
LP_LENGTHS = [1, 5, 6, 5000, 40001]
LP_PARAMS = [(3000, 22050, 5), (1800.0, 48000.0, 8)]       # (cutoff, fs, order): lowpass_filter's defaults, and one other
LP_LONG = 40001


def digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).digest(), np.uint8).copy()


def frames(nf, n, seed=0):
    """FM read buffers, every frame different: a random phase walk whose step size is drawn per frame, plus noise."""
    rng = np.random.default_rng([11, int(n), int(seed)])
    ph = np.cumsum(rng.standard_normal((nf, n)) * rng.uniform(0.05, 0.6, (nf, 1)), axis=1)
    noise = rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))
    return (0.5 * np.exp(1j * ph) + 0.02 * noise).astype(np.complex64)


def frame(n):
    """The fixture's frame of n samples."""
    return frames(1, n, seed=1)[0]


def special(name, n=SPECIAL_N):
    x = frames(1, n, seed=2)[0].copy()
    if name == "zeros":
        x[:] = 0
    elif name == "nan":                       # one NaN sample: the mean is NaN, the whole frame comes out 0
        x[n // 3] = np.complex64(complex(np.nan, 0.25))
    elif name == "negzero":                   # -0 components, whole samples of (-0, +0) and (-0, -0): arctan2's zero fix-up, signed zeros in the FIR
        v = x.view(np.float32).reshape(n, 2)
        v[::5, 0] = -0.0
        v[3::7, 1] = -0.0
        v[10::31] = (-0.0, 0.0)
        v[11::31] = (-0.0, -0.0)
    elif name == "tiny":                      # products that underflow to 0 (1e-30) or to denormals (3e-20): arctan2's rare path
        x[: n // 2] *= np.float32(1e-30)
        x[n // 2:] *= np.float32(3e-20)
    elif name == "wrap":                      # full deviation, +3 rad a sample in the first half and -3 in the second: at 2.4 MS/s the
        step = np.where(np.arange(n) < n // 2, 3.0, -3.0)   # scaled audio passes +-32 768 and the int16 cast wraps
        x = (0.5 * np.exp(1j * np.cumsum(step))).astype(np.complex64)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x)


def lp_row(n, dtype):
    """lowpass_filter's input rows: audio-like noise over two tones."""
    rng = np.random.default_rng([12, int(n), np.dtype(dtype).itemsize])
    t = np.arange(n)
    return (0.4 * np.sin(0.05 * t) + 0.3 * np.sin(0.9 * t + 1.0) + 0.1 * rng.standard_normal(n)).astype(dtype)


def lp_rows(nr, n, seed=0):
    rng = np.random.default_rng([13, int(n), int(seed)])
    return np.ascontiguousarray(rng.standard_normal((nr, n)) * np.exp2(rng.integers(-6, 3, (nr, 1))))

"""Captures, windows and cases of the capture survey's fixtures — shared by tools/make_goldens_welch.py, tests/test_welch_golden.py and
tests/test_gpu_welch.py (-m gpu).  NumPy only.

The fixture (tests/golden/welch.npz) stores results, never captures: every capture and every window is regenerated here from its seed
and pinned by a CRC.  The truth in it is SciPy's own, in float64: scipy.signal.welch and spectrogram(mode='psd').max(-1) on the capture
widened to complex128, return_onesided=False.
"""
import zlib

import numpy as np

VERSION = 1
FS = 2.4e6
BLOCK = 32        # pss_welch.h: segments of a block of the summation tree
FOLD_Q = 64       # pss_welch.h: chunks of block partials
GRID_CAP = 1024   # pss_welch.hip: workgroups of a k_welch launch

# (name, N, S, L, left over, detrend, scaling, window, signal kinds of the rows, row_stride - n)
# S covers N, N / 2, 3 N / 8, N - 1 and 1; L covers 1, 2 and 37 (two blocks of the tree, the issue's n = N + 36 S + 5).
CASES = [
    ("n256_full", 256, 256, 37, 5, 1, "density", "hann", ("noise",), 0),
    ("n256_half", 256, 128, 37, 5, 0, "spectrum", "hamming", ("noise",), 0),
    ("n512_38", 512, 192, 37, 0, 1, "density", "asym", ("tone",), 0),
    ("n512_nm1", 512, 511, 2, 3, 0, "density", "hann", ("dc",), 0),
    ("n1024_one", 1024, 1, 37, 0, 1, "spectrum", "hann", ("noise",), 0),
    ("n1024_half", 1024, 512, 37, 5, 1, "density", "hann", ("tone",), 0),
    ("n1024_l1", 1024, 1024, 1, 100, 0, "density", "hamming", ("noise",), 0),
    ("n1024_l2", 1024, 384, 2, 0, 1, "spectrum", "asym", ("dc",), 0),
    ("n2048_full", 2048, 2048, 37, 0, 1, "density", "hamming", ("dc",), 0),
    ("n2048_nm1", 2048, 2047, 37, 5, 0, "spectrum", "hann", ("tone",), 0),
    ("n2048_one", 2048, 1, 2, 0, 1, "density", "asym", ("noise",), 0),
    ("n4096_half", 4096, 2048, 37, 5, 1, "density", "hann", ("noise",), 0),
    ("n4096_38", 4096, 1536, 37, 7, 0, "spectrum", "hamming", ("tone",), 0),
    ("n4096_l1", 4096, 4096, 1, 0, 1, "density", "asym", ("dc",), 0),
    ("n4096_full", 4096, 4096, 2, 0, 0, "density", "hann", ("noise",), 0),
    ("rows3", 1024, 512, 37, 5, 1, "density", "hann", ("noise", "tone", "dc"), 7),
]


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


def case(name):
    for i, c in enumerate(CASES):
        if c[0] == name:
            return i, c
    raise KeyError(name)


def n_of(N, S, L, left):
    return N + (L - 1) * S + left


def signal(kind, n, seed):
    """noise: noise and three carriers; tone: a strong tone (60 dB above the noise) beside noise; dc: noise on a DC offset.  complex64."""
    rng = np.random.default_rng([71, int(n), int(seed)])
    t = np.arange(n)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    if kind == "noise":
        x = 0.3 * z
        for f, a in ((0.125, 0.5), (-0.31, 0.4), (0.02, 0.3)):
            x = x + a * np.exp(2j * np.pi * (f * t + rng.uniform()))
    elif kind == "tone":
        x = 1e-3 * z + np.exp(2j * np.pi * (0.2137 * t + rng.uniform()))
    elif kind == "dc":
        x = 0.05 * z + (0.75 - 0.4j)
    else:
        raise KeyError(kind)
    return x.astype(np.complex64)


def window(kind, N):
    """hann / hamming: the periodic ones (SciPy's get_window default), in plain NumPy; asym: a hand-made window that is not symmetric."""
    i = np.arange(N, dtype=np.float64)
    if kind == "hann":
        return 0.5 - 0.5 * np.cos(2 * np.pi * i / N)
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(2 * np.pi * i / N)
    if kind == "asym":
        rng = np.random.default_rng([72, N])
        return (0.1 + 0.9 * np.sin(np.pi * (i + 0.5) / N) ** 2) * (1.0 + 0.5 * i / N) + 1e-3 * rng.standard_normal(N)
    raise KeyError(kind)


def case_rows(name):
    """-> (buffer complex64 [K][row_stride] with NaN between the rows, n)."""
    i, (_, N, S, L, left, _, _, _, kinds, gap) = case(name)
    n = n_of(N, S, L, left)
    buf = np.full((len(kinds), n + gap), np.nan + 1j * np.nan, np.complex64)
    for r, kind in enumerate(kinds):
        buf[r, :n] = signal(kind, n, 100 * i + r)
    return buf, n


def case_window(name):
    _, c = case(name)
    return np.ascontiguousarray(window(c[7], c[1]), np.float64)


def scale_of(w, scaling, fs=FS):
    return 1.0 / (fs * (w * w).sum()) if scaling == "density" else 1.0 / w.sum() ** 2


def carriers_capture(n, fs, carriers, seed=5, sigma=0.01):
    """A synthetic capture for the signal list: carriers = ((offset_hz, width_hz, amplitude), ...), each a band of flat noise of that width
    around its offset, on a noise floor of sigma a part."""
    rng = np.random.default_rng([73, int(n), int(seed)])
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    f = np.fft.fftfreq(n, 1.0 / fs)
    for off, width, amp in carriers:
        spec = np.where(np.abs(f - off) < width / 2, np.exp(2j * np.pi * rng.uniform(size=n)), 0)
        band = np.fft.ifft(spec)
        x = x + amp * band / np.sqrt(np.mean(np.abs(band) ** 2))
    return x.astype(np.complex64)

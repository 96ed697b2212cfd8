"""Shared by tests/test_sweep_golden.py (CPU), tests/test_gpu_sweep.py and tools/make_goldens_sweep.py: the sweeps of tests/golden/sweep.npz.

A case is one sweep: 16 slices of n samples at 2.4 MS/s — the seven signal kinds of the classify.npz generator, a noise floor, a bare tone,
loud noise and an all-zero slice from one seed, five of the signal kinds again from a second — quantised to 16-bit ADC codes / 32768, as a
radio delivers them.  The slices are NOT stored in the fixture (a driver case alone is 3 MB; a committed file stays under 1 MiB): slices()
regenerates them from integer codes, and `crc_<case>` in the fixture pins their bytes.  Plain seeded NumPy; no GPU import.
"""
import zlib
from collections import namedtuple

import numpy as np

FS = 2.4e6
MIN_BW = 50e3          # MIN_SIGNAL_BANDWIDTH, pyspecsdr.py:127
GRID_HZ = 100e3        # the duplicate grid of scan_frequencies, pyspecsdr.py:1088

# kind: "inline" (pyspecsdr.py:2539-2561, mask = peak - 20 dB) or "driver" (scan_frequencies, :1022-1093, absolute mask)
Case = namedtuple("Case", "name kind n threshold start step seeds")
CASES = (
    Case("inline_2048", "inline", 2048, -10.0, 88.0e6, 100e3, (11, 12)),
    Case("inline_4096", "inline", 4096, -30.05, 144.0e6, 100e3, (21, 22)),     # a threshold that is not a float32 value
    Case("driver_2048", "driver", 2048, 0.0, 88.0e6, 50e3, (31, 32)),          # 88.00 and 88.05 MHz share the key 880 (half to even)
    Case("driver_5000", "driver", 5000, 0.0, 430.0e6, 100e3, (41, 43)),
    Case("driver_24000", "driver", 24000, 20.5, 118.0e6, 100e3, (51, 52)),
)
# slice order: the first, second and fourth slices are wide carriers (the duplicate pair of driver_2048 and the record behind it)
ORDER = (("fm75k", 0), ("wide", 0), ("zero", 0), ("fmoff", 0), ("noise", 0), ("tone", 0), ("nfm5k", 0), ("tone300k", 0), ("am", 0),
         ("floor", 0), ("loud", 0), ("fm75k", 1), ("noise", 1), ("fmoff", 1), ("wide", 1), ("nfm5k", 1))
SCREENS = ((12, 100), (40, 120))   # max_h x max_w: five results per page (two pages), and one page


def case(name):
    return next(c for c in CASES if c.name == name)


def _sig(rng, n, dev, ftone, noise, off=0.0, amp=0.5):
    t = np.arange(n) / FS
    ph = 2 * np.pi * dev * np.cumsum(np.sin(2 * np.pi * ftone * t)) / FS + 2 * np.pi * off * t
    return amp * np.exp(1j * ph) + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def _kind(kind, n, rng):
    t = np.arange(n) / FS
    if kind == "fm75k":
        return _sig(rng, n, 75e3, 1e3, 0.01)
    if kind == "nfm5k":
        return _sig(rng, n, 5e3, 1e3, 0.01)
    if kind == "noise":
        return _sig(rng, n, 0, 1, 0.1, amp=0)
    if kind == "tone300k":
        return _sig(rng, n, 0, 1, 0.001, off=300e3)
    if kind == "fmoff":
        return _sig(rng, n, 75e3, 5e3, 0.02, off=-450e3)
    if kind == "am":
        return (1 + 0.5 * np.sin(2 * np.pi * 1e3 * t)) * 0.5 * np.exp(0.3j) + _sig(rng, n, 0, 1, 0.005, amp=0)
    if kind == "wide":
        return _sig(rng, n, 400e3, 20e3, 0.01)
    if kind == "floor":
        return _sig(rng, n, 0, 1, 0.001, amp=0)
    if kind == "tone":
        return 0.5 * np.exp(2j * np.pi * -600e3 * t)     # on a bin at every case length: one bin wide in either sweep
    if kind == "loud":
        return _sig(rng, n, 0, 1, 0.25, amp=0)
    if kind == "zero":
        return np.zeros(n, np.complex128)
    raise ValueError(kind)


def _quantise(z):
    out = np.empty(len(z), np.complex64)
    v = out.view(np.float32)
    v[0::2] = np.clip(np.rint(z.real * 32768.0), -32768, 32767).astype(np.float32) / np.float32(32768.0)
    v[1::2] = np.clip(np.rint(z.imag * 32768.0), -32768, 32767).astype(np.float32) / np.float32(32768.0)
    return out


_cache = {}


def slices(c):
    """complex64 [16][n]: the case's slices in sweep order (cached: the tests share one copy and leave it unchanged)."""
    if c.name not in _cache:
        rngs = [np.random.default_rng(s) for s in c.seeds]
        x = np.stack([_quantise(_kind(kind, c.n, rngs[which])) for kind, which in ORDER])
        x.setflags(write=False)
        _cache[c.name] = x
    return _cache[c.name]


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


def sweep_end(c):
    """An end frequency for which `while current_freq <= end` visits exactly one frequency per slice."""
    return c.start + (len(ORDER) - 0.5) * c.step


def lines_key(c, hw, page):
    return f"lines_{c.name}_{hw[0]}x{hw[1]}_p{page}"

"""Shared by tests/test_views_golden.py (CPU), tests/test_gpu_views.py and tools/make_goldens_views.py: the constellation buffers of
tests/golden/views.npz and the NumPy statements of the surface view's compact form.  Plain seeded NumPy; no GPU import.

Constellation buffers.  Those built from tests/adc_cases.py are regenerated here (the fixture pins their bytes in `crc_<name>`): integer ADC
codes put samples exactly ON cell edges (centre + code / 128 * scale is an integer for many codes), and the same codes at 3 x full scale
reach coordinates in (-1, 0), which int() truncates ONTO the screen's first line / column.  The unit-circle tone and the Gaussian noise are
stored in the fixture itself (`iq_<name>`): they come from exp / sin, whose last bit may differ between NumPy builds.
Every sample is finite: the reference raises at int(NaN) and abandons the rest of the buffer, the library skips the sample.
"""
import os

import numpy as np

import adc_cases as A

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "views.npz")
SCREENS = ((1, 1), (4, 10), (24, 80), (25, 81), (40, 120), (130, 1100))
LENGTHS = (1, 29, 600, 1024, 32768, 40001)

# name -> (grid, level, signal, n, seed, factor): adc_cases.make(...) * float32(factor)
ADC_BUFFERS = {
    "i8_mid_am_1": ("i8", "mid", "am", 1, 301, 1.0),
    "u8o_clip_mpx_29_x3": ("u8o", "clip", "mpx", 29, 302, 3.0),
    "i8_mid_fm_600": ("i8", "mid", "fm", 600, 303, 1.0),
    "i12_weak_ssb_600_x3": ("i12", "weak", "ssb", 600, 304, 3.0),
    "i8_clip_ssb_1024_x3": ("i8", "clip", "ssb", 1024, 305, 3.0),
    "i16_mid_mpx_32768_x3": ("i16", "mid", "mpx", 32768, 306, 3.0),
    "i8_mid_fm_40001_x3": ("i8", "mid", "fm", 40001, 307, 3.0),
    "i8_clip_mpx_40001": ("i8", "clip", "mpx", 40001, 308, 1.0),
}
STORED_BUFFERS = ("tone_1024", "noise_1024", "noise_32768")


def adc_buffer(name):
    grid, level, kind, n, seed, factor = ADC_BUFFERS[name]
    x = A.make(grid, level, kind, n, seed)
    return (x * np.float32(factor)).astype(np.complex64)


def stored_buffer(name):
    """What tools/make_goldens_views.py stores as iq_<name> (the tests read the stored bytes)."""
    n = int(name.rsplit("_", 1)[1])
    if name.startswith("tone"):
        return np.exp(2j * np.pi * 37 * np.arange(n) / n).astype(np.complex64)
    rng = np.random.default_rng(900 + n)
    return (0.7 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def buffer_names():
    return tuple(ADC_BUFFERS) + STORED_BUFFERS


_G = None


def golden():
    global _G
    if _G is None:
        _G = np.load(PATH)
    return _G


def buffer(name):
    """The read buffer of a fixture case, its bytes checked against the fixture where it is regenerated."""
    g = golden()
    if name in STORED_BUFFERS:
        return np.ascontiguousarray(g[f"iq_{name}"], np.complex64)
    x = adc_buffer(name)
    assert A.crc(x) == int(g[f"crc_{name}"]), f"{name}: the regenerated buffer is not the fixture's"
    return x


def grid(name, H, W):
    """The reference's constellation grid of one case, int8 [H][W], from the fixture's packed bits (np.packbits, little bit order, line by line)."""
    bits = golden()[f"vec_{name}_{H}x{W}"]
    return np.unpackbits(bits, axis=1, count=W, bitorder="little").astype(np.int8)


def masks_of_grid(g):
    """uint32 [..., H, (W + 31) // 32] masks of 0 / 1 grids [..., H, W]: bit x & 31 of word x >> 5 (independent of the library)."""
    g = np.asarray(g)
    W = g.shape[-1]
    words = (W + 31) // 32
    packed = np.packbits(g.astype(bool), axis=-1, bitorder="little")
    pad = words * 4 - packed.shape[-1]
    if pad:
        packed = np.concatenate([packed, np.zeros(packed.shape[:-1] + (pad,), np.uint8)], axis=-1)
    return np.ascontiguousarray(packed).view("<u4").astype(np.uint32).reshape(g.shape[:-1] + (words,))


def surface_mags_numpy(row, disp_w):
    """draw_surface_plot's own NumPy statements (pyspecsdr.py:1575-1593) up to magnitude = int(value * 20) -> (int8 [disp_w], -1 where the
    resampled value is not finite; (min_val, max_val))."""
    row = np.asarray(row, np.float64)
    with np.errstate(all="ignore"):
        fin = row[np.isfinite(row)]
        min_val, max_val = np.min(fin), np.max(fin)
        db_range = max_val - min_val
        if db_range == 0:
            db_range = 1
        normalized = (row - min_val) / db_range
        resampled = np.interp(np.linspace(0, len(normalized) - 1, disp_w), np.arange(len(normalized)), normalized)
    mag = np.full(disp_w, -1, np.int8)
    for x, value in enumerate(resampled):
        if np.isfinite(value):
            mag[x] = int(value * 20)
    return mag, (min_val, max_val)


def surface_cells_numpy(mag, max_h, max_w):
    """The expansion rule of include/pss.h in the reference's loop order (:1591-1601), independent of pss_h_mags_cells."""
    co = np.zeros((max_h, max_w), np.int8)
    c, s = np.cos(np.radians(45)), np.sin(np.radians(45))
    for x, m in enumerate(mag):
        for y in range(int(m)):
            sx = int(x - y * c) + 8
            sy = int(max_h - 2 - y * s)
            if 0 <= sx < max_w and 2 <= sy < max_h - 1:
                co[sy, sx] = 1 + (y % 5)
    return co

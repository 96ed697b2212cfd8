"""The spectrum display in its compact form (include/pss.h, "spectrum bars"), the parts that need no GPU: the new symbols, the host
expansion pss_h_bars_cells against the reference's own grids (tests/golden/display.npz, all `sg` cases), and the dB scale labels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import display_cases as D
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pss_spectrum_bars", "pss_spectrum_bars_f64", "pss_bars_cells", "pss_h_bars_cells", "pss_frame_pipeline_bars", "pss_gradient_rows",
       "pss_gradient_rows_f64")
SG = [c for c in D.cases() if c.kind == "sg"]


def bars_of_grids(glyph, colour):
    """(height, level) of every column of one draw_spectrogram grid pair: height = cells whose colour is not 1 (the cleared pair), -1 for a
    column that was not drawn; level from the column's colours (14 -> 3, 13 -> 2, 12 -> 1, 10 / 11 -> 0; 0 where the height is 0)."""
    disp_h, disp_w = colour.shape
    height = np.count_nonzero(colour != 1, axis=0).astype(np.int8)
    top = colour.max(axis=0)                       # the bar's pair is the largest of the column (cleared = 1, bars 10 .. 14)
    level = np.select([top == 14, top == 13, top == 12], [3, 2, 1], 0).astype(np.int8)
    undrawn = (colour == -1).all(axis=0)
    assert np.array_equal(undrawn, (glyph == -1).all(axis=0)) and np.array_equal(undrawn, (colour == -1).any(axis=0))
    height[undrawn] = -1
    level[undrawn] = -1
    return height, level


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "pss.h")).read()
    for name in NEW:
        assert hasattr(lib, name), f"{name} not exported by libpss.so"
        assert name in L.exported_symbols(), f"{name} missing from the ctypes table"
        assert re.search(r"^int " + name + r"\(", header, re.M), f"{name} not declared in include/pss.h"


def test_sg_cases_are_all_there():
    assert len(SG) == 92
    assert sum(c.raised for c in SG) == 0


@pytest.mark.parametrize("c", SG, ids=lambda c: f"sg{c.i}")
def test_h_bars_cells_reproduces_the_reference_grids(c):
    """Every glyph and every colour of the reference's grid follows from (height, level) of its column."""
    height, level = bars_of_grids(c.a, c.b)
    glyph, colour = F.bars_cells(height, level, c.disp_h)
    assert glyph.shape == c.a.shape and colour.shape == c.b.shape
    assert np.array_equal(glyph, c.a), c.name() + ": glyph " + D.first_diff(glyph, c.a)
    assert np.array_equal(colour, c.b), c.name() + ": colour " + D.first_diff(colour, c.b)


def test_h_bars_cells_batches_and_leading_axes():
    cs = [c for c in SG if (c.disp_h, c.disp_w) == (SG[0].disp_h, SG[0].disp_w)]
    bars = [bars_of_grids(c.a, c.b) for c in cs]
    glyph, colour = F.bars_cells(np.stack([b[0] for b in bars]), np.stack([b[1] for b in bars]), cs[0].disp_h)
    assert np.array_equal(glyph, np.stack([c.a for c in cs])) and np.array_equal(colour, np.stack([c.b for c in cs]))


def test_h_bars_cells_argument_checks():
    lib = L.load()
    h, l = np.zeros(4, np.int8), np.zeros(4, np.int8)
    g, c = np.zeros(4 * 127, np.int8), np.zeros(4 * 127, np.int8)
    call = lambda hh, ll, n, dh, dw, gg, cc: lib.pss_h_bars_cells(hh, ll, n, dh, dw, gg, cc)
    p = lambda a: a.ctypes.data
    assert call(p(h), p(l), 1, 3, 4, p(g), p(c)) == 0
    assert call(p(h), p(l), 1, 127, 4, p(g), p(c)) == 0
    for disp_h in (0, -1, 128):
        assert call(p(h), p(l), 1, disp_h, 4, p(g), p(c)) == L.PSS_E_ARG
    assert call(p(h), p(l), 1, 3, 0, p(g), p(c)) == L.PSS_E_ARG
    assert call(p(h), p(l), -1, 3, 4, p(g), p(c)) == L.PSS_E_ARG
    for bufs in ((None, p(l), p(g), p(c)), (p(h), None, p(g), p(c)), (p(h), p(l), None, p(c)), (p(h), p(l), p(g), None)):
        assert call(bufs[0], bufs[1], 1, 3, 4, bufs[2], bufs[3]) == L.PSS_E_ARG
    assert call(None, None, 0, 3, 4, None, None) == 0          # an empty batch touches nothing
    tall = h.copy()
    tall[2] = 4
    assert call(p(tall), p(l), 1, 3, 4, p(g), p(c)) == L.PSS_E_ARG    # a height above disp_h
    tall[2] = 3
    assert call(p(tall), p(l), 1, 3, 4, p(g), p(c)) == 0
    with pytest.raises(ValueError):
        F.bars_cells(tall, l, 2)


def test_rule_on_hand_made_columns():
    """The expansion rule of include/pss.h spelled out on one column per level (disp_h 10, height 4: rel = 0, .25, .5, .75)."""
    height = np.array([4, 4, 4, 4, 0, -1, 10], np.int8)
    level = np.array([3, 2, 1, 0, 0, -1, 3], np.int8)
    glyph, colour = F.bars_cells(height, level, 10)
    assert glyph[:6, :4].tolist() == [[4] * 4] * 6 and colour[:6, :4].tolist() == [[1] * 4] * 6
    assert glyph[6:, 0].tolist() == [2, 2, 2, 3] and set(colour[6:, 0]) == {14}
    assert glyph[6:, 1].tolist() == [1, 1, 1, 2] and set(colour[6:, 1]) == {13}
    assert glyph[6:, 2].tolist() == [0, 0, 0, 1] and set(colour[6:, 2]) == {12}
    assert glyph[6:, 3].tolist() == [4, 4, 4, 0] and colour[6:, 3].tolist() == [10, 10, 10, 11]
    assert set(glyph[:, 4]) == {4} and set(colour[:, 4]) == {1}
    assert set(glyph[:, 5]) == {-1} and set(colour[:, 5]) == {-1}
    assert glyph[:, 6].tolist() == [2] * 6 + [3] * 4 and set(colour[:, 6]) == {14}


@pytest.mark.parametrize("c", SG[::7], ids=lambda c: f"sg{c.i}")
def test_scale_labels(c):
    """pyspecsdr.py:430-435 on the golden ranges."""
    lo, hi = (float(v) for v in c.sg_range)
    got = F.spectrum_scale_labels(lo, hi, c.disp_h)
    want = []
    for i in range(c.disp_h):
        db_value = hi - (i * (hi - lo) / c.disp_h)
        if i % 3 == 0:
            want.append((i, f"{db_value:4.0f}dB"))
    assert got == want and len(got) == (c.disp_h + 2) // 3
    assert all(len(t) >= 6 and t.endswith("dB") for _, t in got)


def test_scale_labels_of_a_row_without_a_finite_value():
    assert F.spectrum_scale_labels(float("nan"), float("nan"), 4) == [(0, " nandB"), (3, " nandB")]

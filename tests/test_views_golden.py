"""The surface plot and the constellation in their compact forms (include/pss.h, "surface magnitudes" / "constellation masks"), the parts
that need no GPU: the new symbols, the host expansions pss_h_mags_cells / pss_h_masks_cells against the reference's own grids
(tests/golden/display.npz, all `sf` cases; tests/golden/views.npz and caller.npz for the constellation), and the surface's scale labels."""
import os
import re

import numpy as np
import pytest

import display_cases as D
import oracle_lib as O
import views_cases as V
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pss_surface_mags", "pss_surface_mags_f64", "pss_mags_cells", "pss_h_mags_cells", "pss_frame_pipeline_surface", "pss_vector_masks",
       "pss_masks_cells", "pss_h_masks_cells", "pss_frame_pipeline_vector")
SF = [c for c in D.cases() if c.kind == "sf"]
VEC = [(name, H, W) for name in V.buffer_names() for H, W in V.SCREENS]


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "pss.h")).read()
    for name in NEW:
        assert hasattr(lib, name), f"{name} not exported by libpss.so"
        assert name in L.exported_symbols(), f"{name} missing from the ctypes table"
        assert re.search(r"^int " + name + r"\(", header, re.M), f"{name} not declared in include/pss.h"
    assert "16384" in header[header.index("pss_vector_masks"):], "the mask's LDS limit is stated in pss.h"


def test_sf_cases_are_all_there():
    assert len(SF) == 92
    assert sum(c.raised for c in SF) == 0
    assert min(c.length for c in SF) == 2 and max(c.length for c in SF) == 16380
    assert {(4, 10), (130, 1100), (6, 32767)} <= {(c.H, c.W) for c in SF}


def test_fixture_is_what_the_issue_lists():
    g = V.golden()
    assert [str(n) for n in g["vec_cases"]] == list(V.buffer_names())
    assert tuple(map(tuple, g["vec_screens"])) == V.SCREENS
    assert {len(V.buffer(n)) for n in V.buffer_names()} == set(V.LENGTHS)
    assert os.path.getsize(V.PATH) < 300_000
    for n in V.buffer_names():
        assert np.all(np.isfinite(V.buffer(n).view(np.float32))), n
    # samples ON cell edges (an integer coordinate off the centre) and coordinates in (-1, 0), which truncate onto the screen
    x = V.buffer("i8_clip_ssb_1024_x3")
    fx = np.float32(40) + x.real * np.float32(6)
    fy = np.float32(12) - x.imag * np.float32(6)
    assert np.count_nonzero((fx == np.floor(fx)) & (fx != 40)) > 0
    assert np.count_nonzero((fy > -1) & (fy < 0)) + np.count_nonzero((fx > -1) & (fx < 0)) > 0


@pytest.mark.parametrize("c", SF, ids=lambda c: f"sf{c.i}")
def test_surface_cells_reproduces_the_reference_grids(c):
    """Every '#' of the reference's grid follows from the column magnitudes (the reference's own NumPy expressions) and the screen size."""
    mag, _ = V.surface_mags_numpy(c.rows[-1], c.disp_w)
    assert mag.max() <= 20
    colour = F.surface_cells(mag, c.H, c.W)
    assert colour.shape == c.a.shape
    assert np.array_equal(colour, c.a), c.name() + ": " + D.first_diff(colour, c.a)


def test_sf_magnitudes_cover_what_the_issue_counted():
    mags = [V.surface_mags_numpy(c.rows[-1], c.disp_w)[0] for c in SF]
    assert max(int(m.max()) for m in mags) == 20
    assert sum(int(np.count_nonzero(m == -1)) for m in mags) == 186


@pytest.mark.parametrize("H,W", [(4, 10), (14, 19), (24, 80), (25, 81), (40, 120), (50, 200), (130, 1100)])
def test_h_mags_cells_equals_the_oracle_on_seeded_rows(H, W):
    rng = np.random.default_rng(H * 10000 + W)
    w = W - 8
    for k, n in enumerate((2, 3, 7, 60, w, 2 * w + 3)):
        row = rng.standard_normal(n) * 12 - 60
        if k % 3 == 1 and n > 3:
            row[[1, n // 2]] = (np.nan, np.inf)
        if k == 3:
            row[:] = -42.5
        mag, _ = V.surface_mags_numpy(row, w)
        got = F.surface_cells(mag, H, W)
        want = O.surface_cells(row, H, W)
        assert np.array_equal(got, want), f"len {n} screen {H}x{W}: " + D.first_diff(got, want)
        assert np.array_equal(got, V.surface_cells_numpy(mag, H, W))


def test_h_mags_cells_all_magnitudes_and_leading_axes():
    """Every magnitude up to 127 in every column position, against the rule restated in NumPy; leading axes like formats.bars_cells."""
    rng = np.random.default_rng(5)
    mag = rng.integers(-1, 128, (3, 2, 40)).astype(np.int8)
    got = F.surface_cells(mag, 60, 48)
    assert got.shape == (3, 2, 60, 48)
    for i in range(3):
        for j in range(2):
            assert np.array_equal(got[i, j], V.surface_cells_numpy(mag[i, j], 60, 48))
    with pytest.raises(ValueError):
        F.surface_cells(mag, 60, 47)


def test_overwrite_rule_on_hand_made_columns():
    """Screen 12 x 20 (12 columns, base line sy = 10).  Step y of column x lands at (int(10 - y sin45), int(x - y cos45) + 8) and carries
    colour 1 + y % 5; for y = 0 .. 8 the lines are 10 9 8 7 7 6 5 5 4 and the columns x + 8 - (0 1 2 3 3 4 5 5 6) (x >= 1).  The LAST
    (x, y) in the reference's loop order keeps a cell."""
    H, W = 12, 20
    cells = lambda g: {(int(y), int(x)): int(g[y, x]) for y, x in np.argwhere(g)}
    one = np.zeros(12, np.int8)
    one[6] = 4
    assert cells(F.surface_cells(one, H, W)) == {(10, 14): 1, (9, 13): 2, (8, 12): 3, (7, 11): 4}
    # two steps of one column on one cell: y = 3 and y = 4 both land at (7, x + 5), y = 6 and y = 7 at (5, x + 3); the later step stays
    tall = np.zeros(12, np.int8)
    tall[10] = 9
    assert cells(F.surface_cells(tall, H, W)) == {(10, 18): 1, (9, 17): 2, (8, 16): 3, (7, 15): 5, (6, 14): 1, (5, 13): 3, (4, 12): 4}
    # neighbouring columns march side by side without touching
    both = np.zeros(12, np.int8)
    both[6], both[7] = 3, 3
    assert cells(F.surface_cells(both, H, W)) == {(10, 14): 1, (9, 13): 2, (8, 12): 3, (10, 15): 1, (9, 14): 2, (8, 13): 3}
    # ... except where truncation toward zero doubles up: int(0 - cos45) = int(1 - cos45) = 0, so step 1 of columns 0 and 1 share (9, 8)
    # (both writers carry colour 2 here; test_later_column_beats_a_larger_step_of_an_earlier_column tells writers apart)
    left = np.zeros(12, np.int8)
    left[0], left[1] = 2, 2
    assert cells(F.surface_cells(left, H, W)) == {(10, 8): 1, (10, 9): 1, (9, 8): 2}
    left[0], left[1] = 3, 3                              # (0, 2) -> (8, 7); (1, 2) -> (8, 8)
    assert cells(F.surface_cells(left, H, W)) == {(10, 8): 1, (10, 9): 1, (9, 8): 2, (8, 7): 3, (8, 8): 3}
    # columns not drawn draw nothing; lines 0, 1 and max_h - 1 are never drawn however tall the columns
    assert not F.surface_cells(np.full(12, -1, np.int8), H, W).any()
    full = np.full(12, 127, np.int8)
    g = F.surface_cells(full, H, W)
    assert not g[:2].any() and not g[H - 1].any() and g[2:H - 1].any()
    assert np.array_equal(g, V.surface_cells_numpy(full, H, W))


def test_later_column_beats_a_larger_step_of_an_earlier_column():
    """Cell (sy, sx) shared by (x0, y0) and (x1, y1) with x1 > x0 and y1 < y0: the later COLUMN keeps it, whatever the step."""
    H, W = 30, 40
    found = 0
    for x0 in range(4, 20):
        for y0 in range(1, 20):
            for y1 in range(0, y0):
                for x1 in range(x0 + 1, x0 + 3):
                    a = (int(H - 2 - y0 * np.sin(np.radians(45))), int(x0 - y0 * np.cos(np.radians(45))) + 8)
                    b = (int(H - 2 - y1 * np.sin(np.radians(45))), int(x1 - y1 * np.cos(np.radians(45))) + 8)
                    if a != b:
                        continue
                    mag = np.zeros(W - 8, np.int8)
                    mag[x0], mag[x1] = y0 + 1, y1 + 1
                    g = F.surface_cells(mag, H, W)
                    assert g[a] == 1 + y1 % 5 and np.array_equal(g, V.surface_cells_numpy(mag, H, W))
                    found += 1
    assert found > 0, "the geometry has such pairs (two steps on one line whose columns' truncations meet)"


@pytest.mark.parametrize("name,H,W", VEC, ids=lambda v: str(v))
def test_vector_cells_reproduces_the_reference_grids(name, H, W):
    want = V.grid(name, H, W)
    mask = V.masks_of_grid(want)
    assert mask.shape == (H, (W + 31) // 32) and mask.dtype == np.uint32
    got = F.vector_cells(mask, H, W)
    assert np.array_equal(got, want), f"{name} {H}x{W}: " + D.first_diff(got, want)
    assert np.array_equal(want, O.vector_cells(V.buffer(name), H, W)), "the oracle draws the reference's grid"


def test_vector_cells_on_the_caller_fixture_and_leading_axes():
    g = np.load(os.path.join(os.path.dirname(V.PATH), "caller.npz"))
    for tag, H, W in (("a", 40, 120), ("b", 25, 81)):
        want = g[f"vec_grid_{tag}"]
        assert np.array_equal(F.vector_cells(V.masks_of_grid(want), H, W), want), tag
    grids = np.stack([V.grid(n, 25, 81) for n in V.buffer_names()[:6]]).reshape(2, 3, 25, 81)
    got = F.vector_cells(V.masks_of_grid(grids), 25, 81)
    assert got.shape == (2, 3, 25, 81) and np.array_equal(got, grids)
    assert np.array_equal(F.vector_cells(V.masks_of_grid(grids).view(np.int32), 25, 81), grids)     # int32 storage (torch has no uint32 arithmetic)
    with pytest.raises(ValueError):
        F.vector_cells(V.masks_of_grid(grids), 25, 97)


def test_scale_labels_equal_the_stored_strings():
    g = V.golden()
    by_i = {c.i: c for c in SF}
    picked = [int(i) for i in g["sf_label_cases"]]
    assert len(picked) >= 12
    constant = 0
    for i in picked:
        c = by_i[i]
        _, (lo, hi) = V.surface_mags_numpy(c.rows[-1], c.disp_w)
        got = F.surface_scale_labels(lo, hi, c.disp_h)
        want = str(g[f"sf_labels_{i}"]).split("\n") if c.disp_h > 0 else []
        assert [t for _, t in got] == want, c.name()
        assert [k for k, _ in got] == list(range(0, c.disp_h, 3))
        constant += lo == hi
    assert constant >= 1


def test_scale_labels_of_a_constant_row_step_by_one_over_disp_h():
    got = F.surface_scale_labels(-42.5, -42.5, 4)
    assert got == [(0, " -42dB"), (3, f"{-42.5 - 3 / 4:4.0f}dB")]
    assert F.surface_scale_labels(0.4, 0.4, 6) == [(0, "   0dB"), (3, f"{0.4 - 0.5:4.0f}dB")]
    assert F.surface_scale_labels(2.0, 2.0, 1) == [(0, "   2dB")]


def test_h_mags_cells_argument_checks():
    lib = L.load()
    m, c = np.zeros(2 * 12, np.int8), np.zeros(2 * 12 * 20, np.int8)
    p = lambda a: a.ctypes.data
    call = lib.pss_h_mags_cells
    assert call(p(m), 2, 12, 20, p(c)) == 0
    assert call(p(m), 1, 4, 10, p(c)) == 0                      # the smallest screen
    assert call(p(m), 1, 3, 20, p(c)) == L.PSS_E_ARG
    assert call(p(m), 1, 12, 9, p(c)) == L.PSS_E_ARG
    assert call(p(m), -1, 12, 20, p(c)) == L.PSS_E_ARG
    assert call(None, 1, 12, 20, p(c)) == L.PSS_E_ARG
    assert call(p(m), 1, 12, 20, None) == L.PSS_E_ARG
    before = c.copy()
    assert call(None, 0, 12, 20, None) == 0                     # an empty batch touches nothing
    assert np.array_equal(c, before)
    bad = m.copy()
    bad[5] = -2
    assert call(p(bad), 1, 12, 20, p(c)) == L.PSS_E_ARG         # a magnitude outside [-1, 127]
    bad[5] = 127
    assert call(p(bad), 1, 12, 20, p(c)) == 0
    with pytest.raises(ValueError):
        F.surface_cells(np.full(12, -3, np.int8), 12, 20)


def test_h_masks_cells_argument_checks():
    lib = L.load()
    m, g = np.zeros(2 * 5 * 2, np.uint32), np.full(2 * 5 * 40, 7, np.int8)
    p = lambda a: a.ctypes.data
    call = lib.pss_h_masks_cells
    assert call(p(m), 2, 5, 40, p(g)) == 0 and not g.any()
    assert call(p(m), 1, 1, 1, p(g)) == 0
    assert call(p(m), 1, 0, 40, p(g)) == L.PSS_E_ARG
    assert call(p(m), 1, 5, 0, p(g)) == L.PSS_E_ARG
    assert call(p(m), -1, 5, 40, p(g)) == L.PSS_E_ARG
    assert call(None, 1, 5, 40, p(g)) == L.PSS_E_ARG
    assert call(p(m), 1, 5, 40, None) == L.PSS_E_ARG
    g[:] = 7
    assert call(None, 0, 5, 40, None) == 0 and (g == 7).all()   # an empty batch touches nothing
    m[:] = 0xffffffff                                           # the unused bits of a line's last word are not read
    assert call(p(m), 2, 5, 40, p(g)) == 0 and (g == 1).all()


def test_device_entry_points_reject_a_null_context():
    """The PSS_E_ARG rules of the device entry points need a context (tests/test_gpu_views.py); without one every call is refused."""
    lib = L.load()
    assert lib.pss_surface_mags(None, None, 0, 2, 2, None, None) == L.PSS_E_ARG
    assert lib.pss_surface_mags_f64(None, None, 0, 2, 2, None, None) == L.PSS_E_ARG
    assert lib.pss_mags_cells(None, None, 0, 4, 10, None) == L.PSS_E_ARG
    assert lib.pss_vector_masks(None, None, 0, 0, 1, 1, None) == L.PSS_E_ARG
    assert lib.pss_masks_cells(None, None, 0, 1, 1, None) == L.PSS_E_ARG
    assert lib.pss_frame_pipeline_surface(None, 0, None, 0, 1024, 2.4e6, None, None, None, 2, None, None, None) == L.PSS_E_ARG
    assert lib.pss_frame_pipeline_vector(None, 0, None, 0, 1024, 2.4e6, None, None, None, 1, 1, None, None) == L.PSS_E_ARG

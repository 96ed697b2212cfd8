"""Shared by the spectrum-bars and gradient-line tests: the launch caps of the new kernels, the seeded row families that take every path
of pss_spectrum_bars, and the comparison of its bars with pss_spectrogram_cells' grids."""
import numpy as np

# Rows one launch of pss_spectrum_bars covers without its grid-stride loop, per kernel configuration (pss_fft.hip, launch_bars_reg:
# 256 x min(6, 160 KB / (LDS + 512)) workgroups of RPW rows; LDS = RPW x 64 W EPL doubles) — (longest row, rows per launch).
BARS_ROWS_PER_LAUNCH = (
    (256, 256 * 6 * 4),       # EPL 4, one wavefront per row, four rows per workgroup, 8 KB
    (1024, 256 * 4 * 4),      # EPL 16, 32 KB
    (2048, 256 * 2 * 4),      # EPL 32, 64 KB
    (4092, 256 * 4 * 1),      # EPL 16, four wavefronts per row, 32 KB
    (1 << 20, 4096),          # longer rows: k_spectrogram<T, true>, one workgroup per row
)
BARS_CELLS_PER_LAUNCH = 16384 * 256      # k_bars_cells: one thread per cell
BARS_REG_MAX_LEN = 4092


def rows_per_launch(length):
    return next(r for m, r in BARS_ROWS_PER_LAUNCH if length <= m)


def with_count(row, cnt, what=np.nan):
    """`row` with only its first cnt values left finite."""
    row = row.copy()
    row[cnt:] = what
    return row


def row_families(length, seed):
    """A batch [k][length] of float64 rows built to take every path of the percentile: see the names."""
    rng = np.random.default_rng(seed)
    ln = length
    g = lambda: rng.standard_normal(ln) * 6.0 - 50.0
    out = []
    add = lambda name, row: out.append((name, np.asarray(row, np.float64)))
    add("gaussian", g())
    tone = g()
    tone[ln // 3:ln // 3 + max(1, ln // 50)] += 45.0
    add("tone over noise", tone)
    post = g()
    post[rng.random(ln) < 0.35] -= 40.0
    thr = np.median(post) - 10.0
    post[post < thr] = thr
    add("post-processed (a long run equal to median - 10)", post)
    add("coarse grid (ties at both ranks)", np.round(g() / 4.0) * 4.0)
    add("two values", np.where(rng.random(ln) < 0.5, -60.0, -20.0))
    add("constant", np.full(ln, -42.5))
    add("constant zero", np.zeros(ln))
    low = np.float64(-50.0) + np.arange(ln) * 2.0 ** -44
    add("values that differ only in their low words", rng.permutation(low))
    low2 = np.float64(-50.0) + rng.integers(0, 7, ln) * 2.0 ** -46
    add("low words with ties", low2)
    add("low words ending in 32 zero bits among others", np.where(rng.random(ln) < 0.5, -50.0, -50.0 - rng.integers(0, 3, ln) * 2.0 ** -45))
    add("positive and negative values", g() + 50.0)
    add("sorted ascending", np.sort(g()))
    add("sorted descending", np.sort(g())[::-1])
    for what, tag in ((np.nan, "NaN"), (np.inf, "+inf"), (-np.inf, "-inf")):
        r = g()
        r[rng.integers(0, ln)] = what
        add(f"one {tag}", r)
        r = g()
        r[0] = what
        r[ln - 1] = what
        add(f"{tag} at both ends", r)
        add(f"nothing but {tag}", np.full(ln, what))
    mixed = g()
    mixed[::3] = np.nan
    mixed[1::7] = np.inf
    mixed[2::11] = -np.inf
    add("NaN, +inf and -inf among the values", mixed)
    add("nothing finite (mixed)", np.where(np.arange(ln) % 2 == 0, np.nan, np.inf))
    # the number of finite values chosen for np.percentile's weight g = frac(0.2 (cnt - 1)): 0, < 0.5, >= 0.5
    base = [c for c in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11) if c <= ln]
    top = [ln - k for k in range(5) if ln - k >= 1]
    for cnt in sorted(set(base + top)):
        frac = (cnt - 1) % 5
        add(f"cnt = {cnt} (g = {frac / 5})", with_count(np.round(g()), cnt) if cnt % 2 else with_count(g(), cnt, np.inf))
    names = [n for n, _ in out]
    return names, np.ascontiguousarray(np.stack([r for _, r in out]))


def expand_numpy(height, level, disp_h):
    """NumPy statement of the expansion rule of include/pss.h (independent of pss_h_bars_cells)."""
    height, level = np.asarray(height, np.int64), np.asarray(level, np.int64)
    y = np.arange(disp_h).reshape((disp_h, 1))
    h, l = height[..., None, :], level[..., None, :]
    top = disp_h - h
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = (y - top) / h
    hi = rel > 0.5
    glyph = np.select([l == 3, l == 2, l == 1], [np.where(hi, 3, 2), np.where(hi, 2, 1), np.where(hi, 1, 0)], np.where(rel > 0.7, 0, 4))
    colour = np.select([l == 3, l == 2, l == 1], [14, 13, 12], np.where(rel > 0.7, 11, 10))
    above = y < top
    glyph, colour = np.where(above, 4, glyph), np.where(above, 1, colour)
    undrawn = np.broadcast_to(h < 0, glyph.shape)
    return np.where(undrawn, -1, glyph).astype(np.int8), np.where(undrawn, -1, colour).astype(np.int8)

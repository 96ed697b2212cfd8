#!/usr/bin/env python3
"""Golden cell grids of the five display quantisers across screen sizes, row lengths, history depths and non-finite bins
(tests/golden/display.npz) — made like tools/make_goldens.py: the build container imports the reference's caller (pyspecsdr.py) with
make_goldens' stubs, draws seeded rows on make_goldens' fake screen and stores DATA only (the rows, the screen sizes, the cells the
reference drew).

    draw_waterfall          (pyspecsdr.py:1342-1406)  kind "wf": glyph 0..3 / colour 0..5 per [disp_h = H-4][disp_w = W-8] cell, -1 = not drawn
    draw_persistence        (:1512-1564)              kind "ps": colour pair per [H-4][W-8] cell, 0 = empty (last writer wins)
    draw_gradient_waterfall (:1640-1716)              kind "gw": glyph 0..8 / colour 0..5 per [H-4][W-10] cell, -1 = not drawn
    draw_surface_plot       (:1567-1616)              kind "sf": colour pair per cell of the whole [H][W] screen, 0 = empty
    draw_spectrogram        (:398-498)                kind "sg": glyph 0..4 / colour pair per [H-4][W-7] cell, -1 = never written

Rows: the caller's post-processed rows (compute_fft, 5-tap np.convolve 'valid', clamp at median - 10; pyspecsdr.py:2278-2283) of
seeded IQ at n_fft = len + 4 for len in LENS, plus synthetic rows at the short lengths.  pool_<len> [k][len] float64; a case pushes
pool rows 0 .. n_push-1 into a cleared history and records the grid after the last push.  A case may modify the rows first (MODS):
bin `pos` of the last row set to NaN / +inf / -inf, or every row replaced by the constant -42.5.  The rows are stored once per length,
never per case (the file stays small).

Per case i: case_meta[i] = (kind, len, H, W, n_push, mod, pos, raised, a_off, b_off).  The grids are flattened into one int8 array
`cells`: grid a (glyph or colour) at cells[a_off:], grid b (colour, for wf / gw / sg) at cells[b_off:], -1 = no grid b.  raised = 1:
the reference raised ValueError while drawing (draw_waterfall of a zero-range history: int(NaN)); no grid is stored then (offsets -1).
sg_range[i]: (display_min, display_max) of draw_spectrogram (:419-427), evaluated with the same NumPy expressions by this script (the
reference prints them only rounded); NaN for the other kinds.

    python tools/make_goldens_display.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import make_goldens as mg            # stubs (caller_module, Scr), stamp(), save()
import signal_processing as sp      # the reference hot path

P = mg.caller_module()

LENS = (2, 3, 12, 60, 252, 1020, 4092, 16380)
POOL = {2: 45, 3: 45, 12: 45, 60: 45, 252: 7, 1020: 3, 4092: 1, 16380: 1}   # rows of the longer lengths cost the most bytes
MODS = {0: None, 1: np.nan, 2: np.inf, 3: -np.inf, 4: -42.5}           # 4: the constant history
KINDS = ("wf", "ps", "gw", "sf", "sg")
OFF = {"wf": 8, "ps": 8, "gw": 10, "sf": 8, "sg": 7}                        # display_width = max_width - OFF
MIN_HW = {"wf": (5, 9), "ps": (5, 9), "gw": (5, 11), "sf": (4, 10), "sg": (5, 8)}   # one column, one row (surface: the API's smallest)
SIZES = ((24, 80), (40, 120), (50, 200), (130, 1100))
DEPTH = {"wf": (1, 7, 30, 45), "gw": (1, 7, 30, 45), "ps": (1, 7, 10, 14)}
G4 = {".": 0, "-": 1, "=": 2, "#": 3}
G5 = {".": 0, "-": 1, "=": 2, "#": 3, " ": 4}
G9 = " ._-=+*#@"


def post_rows(n_rows, n_fft, seed):
    rng = np.random.default_rng(seed)
    fs = 2.4e6
    t = np.arange(n_fft) / fs
    out = []
    for f in range(n_rows):
        x = (0.5 * np.exp(1j * (2 * np.pi * (150e3 + 9e3 * f) * t + 0.2 * f)) + 0.2 * np.exp(2j * np.pi * -410e3 * t)
             + 0.02 * (rng.standard_normal(n_fft) + 1j * rng.standard_normal(n_fft))) * (1.0 + 0.3 * (f % 5))
        fd = sp.compute_fft(x.astype(np.complex64))
        fd = np.convolve(fd, np.ones(5) / 5, mode="valid")
        thr = np.median(fd) - 10
        fd[fd < thr] = thr
        out.append(fd)
    return np.stack(out)


def pool(n):
    rows = post_rows(POOL[n], n + 4, 700 + n)
    if n <= 12:                                   # synthetic rows: exact knots, a ramp, alternating extremes, a large offset
        rows[1] = np.arange(n, dtype=np.float64) * 3.0 - 40.0
        rows[2] = np.where(np.arange(n) % 2 == 0, -80.0, -20.0)
        rows[3] = -60.0 + np.linspace(0.0, 1.0, n) ** 2 * 37.5
        rows[4] = 1e6 + np.arange(n)[::-1] * 0.125
    return rows


def mod_rows(rows, mod, pos):
    """The rows a case pushes: pool rows, modified as MODS[mod] says (the same function is restated in tests/display_cases.py)."""
    rows = rows.copy()
    if mod == 4:
        rows[:] = MODS[4]
    elif mod:
        rows[-1, pos] = MODS[mod]
    return rows


def draw(kind, rows, H, W):
    """Clear the reference's history, push `rows`, return the grids after the last push: (a, b or None, raised)."""
    fn = {"wf": P.draw_waterfall, "gw": P.draw_gradient_waterfall, "ps": P.draw_persistence, "sf": P.draw_surface_plot,
          "sg": P.draw_spectrogram}[kind]
    P.WATERFALL_HISTORY.clear()
    P.PERSISTENCE_HISTORY.clear()
    scr = None
    try:
        with np.errstate(all="ignore"):
            for r in rows:
                scr = mg.Scr(H, W)
                fn(scr, r.copy(), None, 100e6, 2.4e6, 0, 0, None)
    except ValueError:
        return None, None, 1
    dh, dw = H - 4, W - OFF[kind]
    if kind == "wf":
        a, b = -np.ones((dh, dw), np.int8), -np.ones((dh, dw), np.int8)
        for y, x, s, attr in (c for c in scr.calls if len(c) == 4):
            if s in G4 and len(s) == 1 and x >= 9 and y >= 3 and (attr >> 8) >= 10:
                a[y - 3, x - 9] = G4[s]; b[y - 3, x - 9] = (attr >> 8) - 10
        return a, b, 0
    if kind == "gw":
        a, b = -np.ones((dh, dw), np.int8), -np.ones((dh, dw), np.int8)
        for y, x, s, attr in (c for c in scr.calls if len(c) == 4):
            if len(s) == 1 and s in G9 and 9 <= x < 9 + dw and 2 <= y < 2 + dh and (attr >> 8) >= 10:
                a[y - 2, x - 9] = G9.index(s); b[y - 2, x - 9] = (attr >> 8) - 10
        return a, b, 0
    if kind == "ps":
        a = np.zeros((dh, dw), np.int8)
        for y, x, s, attr in (c for c in scr.calls if len(c) == 4):
            if s == "*":
                a[y - 2, x - 8] = attr >> 8
        return a, None, 0
    if kind == "sf":
        a = np.zeros((H, W), np.int8)
        for y, x, s, attr in (c for c in scr.calls if len(c) == 4):
            if s == "#":
                a[y, x] = attr >> 8
        return a, None, 0
    a, b = -np.ones((dh, dw), np.int8), -np.ones((dh, dw), np.int8)
    for c in scr.calls:
        if len(c) != 4:
            continue
        y, x, s, attr = c
        if len(s) == 1 and s in G5 and x >= 7 and 2 <= y < 2 + dh and x - 7 < dw:
            a[y - 2, x - 7] = G5[s]; b[y - 2, x - 7] = (attr >> 8) & 0xFF
    return a, b, 0


def sg_range(row):
    """draw_spectrogram's display_min / display_max (pyspecsdr.py:419-427), the same NumPy expressions."""
    fin = row[np.isfinite(row)]
    max_db = np.max(fin)
    noise = np.percentile(fin, 20)
    rng_ = max_db - noise
    return np.array([noise - (rng_ * 0.1), max_db + (rng_ * 0.05)])


def main():
    d = {}
    pools = {n: pool(n) for n in LENS}
    for n, rows in pools.items():
        d[f"pool_{n}"] = rows
    meta, cells, ranges = [], [], []
    size = [0]

    def put(grid):
        if grid is None:
            return -1
        cells.append(grid.ravel())
        size[0] += grid.size
        return size[0] - grid.size

    def add(kind, n, H, W, n_push, mod=0, pos=0):
        rows = mod_rows(pools[n][:n_push], mod, pos)
        a, b, raised = draw(kind, rows, H, W)
        meta.append((KINDS.index(kind), n, H, W, n_push, mod, pos, raised, put(a), put(b)))
        ranges.append(sg_range(rows[-1]) if kind == "sg" else np.full(2, np.nan))

    for kind in KINDS:
        push = 1 if kind in ("sf", "sg") else 7
        for n in LENS:
            # screen sizes: the common terminals, the smallest that draws one column and one row (130 x 1100 at three lengths)
            for H, W in SIZES + (MIN_HW[kind],):
                if H * W > 20000 and n not in (12, 1020, 16380):
                    continue
                add(kind, n, H, W, min(push, POOL[n]))
            # widths at the row length: disp_w = len - 1, len, len + 1, 2 len - 1 (every bin read; samples on the knots)
            for dw in sorted({max(1, n - 1), n, n + 1, 2 * n - 1}):
                H = 6 if n >= 1020 else 14
                add(kind, n, max(H, MIN_HW[kind][0]), max(dw + OFF[kind], MIN_HW[kind][1]), min(push, POOL[n]))
    # history depths, disp_h below and above the depth
    for kind, depths in DEPTH.items():
        for n in (12, 60):
            for p in depths:
                for H in (9, 40, 60):
                    add(kind, n, H, 120, p)
    # non-finite bins: NaN / +inf / -inf at bin 1, len // 2, len - 2 (120-column screen), and on a knot of a disp_w = len screen (bin 37), in the
    # newest row of a three-row history (the spectrogram and the surface draw the newest row alone)
    for kind in KINDS:
        for n in (12, 1020):
            for mod in (1, 2, 3):
                for pos, wide in ((1, False), (n // 2, False), (n - 2, False), (min(37, n - 3), True)):
                    W = n + OFF[kind] if wide else 120
                    add(kind, n, 8 if wide else 40, W, 3, mod, pos)
    # zero range: a constant history (draw_waterfall raises; the gradient, persistence and surface guard the range)
    for kind in KINDS:
        for n in (12, 1020):
            add(kind, n, 40, 120, 3, 4)
    d["case_meta"] = np.array(meta, np.int64)
    d["cells"] = np.concatenate(cells).astype(np.int8)
    d["sg_range"] = np.array(ranges)
    d["kinds"] = np.array(KINDS)
    mg.save("display", **d)
    print(len(meta), "cases,", sum(m[7] for m in meta), "raised")


if __name__ == "__main__":
    main()

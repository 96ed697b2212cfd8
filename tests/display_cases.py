"""The cases of tests/golden/display.npz (tools/make_goldens_display.py): the reference's cell grids of the five display quantisers across
screen sizes, row lengths, history depths, non-finite bins and a zero range.  Shared by the oracle test and the GPU test."""
import os
from dataclasses import dataclass

import numpy as np

import oracle_lib as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "display.npz")
OFF = {"wf": 8, "ps": 8, "gw": 10, "sf": 8, "sg": 7}           # display width = screen width - OFF (the reference's layouts)
WINDOW = {"wf": 30, "gw": 30, "ps": 10, "sf": 1, "sg": 1}      # history the reference keeps (WATERFALL_MAX_LINES, PERSISTENCE_LENGTH)


@dataclass
class Case:
    i: int
    kind: str
    length: int
    H: int
    W: int
    rows: np.ndarray        # the history the reference held when it drew: the last WINDOW of the pushed rows, oldest first
    raised: bool
    a: np.ndarray           # glyph (wf / gw / sg) or colour (ps / sf); None if the reference raised
    b: np.ndarray           # colour (wf / gw / sg) or None
    sg_range: np.ndarray    # (display_min, display_max) for sg

    @property
    def disp_h(self):
        return self.H - 4

    @property
    def disp_w(self):
        return self.W - OFF[self.kind]

    def name(self):
        return f"case {self.i} {self.kind} len={self.length} screen {self.H}x{self.W} (disp {self.disp_h}x{self.disp_w}) rows={len(self.rows)}"


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        g = np.load(PATH)
        kinds = [str(k) for k in g["kinds"]]
        out = []
        cells, ranges = g["cells"], g["sg_range"]
        for i, (k, n, H, W, n_push, mod, pos, raised, a_off, b_off) in enumerate(g["case_meta"]):
            kind = kinds[k]
            rows = g[f"pool_{n}"][:n_push].copy()
            if mod == 4:
                rows[:] = -42.5                                   # a constant history
            elif mod:
                rows[-1, pos] = (np.nan, np.inf, -np.inf)[mod - 1]  # a non-finite bin in the newest row
            rows = np.ascontiguousarray(rows[-WINDOW[kind]:])
            shape = (H, W) if kind == "sf" else (H - 4, W - OFF[kind])
            grid = lambda off: None if off < 0 else cells[off:off + shape[0] * shape[1]].reshape(shape)
            out.append(Case(i, kind, int(n), int(H), int(W), rows, bool(raised), grid(a_off), grid(b_off),
                            ranges[i] if kind == "sg" else None))
        _CASES = out
    return _CASES


def oracle(c, rows=None):
    """The oracle's grids for case c (on `rows` if given: e.g. the float32 rounding of the case's rows, widened): (a, b or None, sg_range)."""
    rows = c.rows if rows is None else np.ascontiguousarray(rows, np.float64)
    if c.kind == "wf":
        return (*O.waterfall_cells(rows, c.disp_h, c.disp_w), None)
    if c.kind == "gw":
        return (*O.gradient_cells(rows, c.disp_h, c.disp_w), None)
    if c.kind == "ps":
        return O.persistence_cells(rows, c.disp_h, c.disp_w), None, None
    if c.kind == "sf":
        return O.surface_cells(rows[-1], c.H, c.W), None, None
    gl, co, lo, hi = O.spectrogram_cells(rows[-1], c.disp_h, c.disp_w)
    return gl, co, np.array([lo, hi])


def first_diff(got, want):
    """'(y, x) got g want w' of the first differing cell, and how many differ."""
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return "equal"
    y, x = bad[0]
    return f"{len(bad)} cells differ, first at (y={y}, x={x}): got {got[y, x]} want {want[y, x]}"

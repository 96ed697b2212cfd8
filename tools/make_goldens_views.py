#!/usr/bin/env python3
"""Golden values for the two views without a history (tests/golden/views.npz) — made like tools/make_goldens_adc.py: the build container
imports the reference's caller (pyspecsdr.py) with make_goldens' stubs, draws on make_goldens' fake screen and stores DATA only.

Constellation (draw_vector_display, pyspecsdr.py:1719-1752): every buffer of tests/views_cases.py on every screen of views_cases.SCREENS.
    vec_<buffer>_<H>x<W>   uint8 [H][ceil(W / 8)]: the cells that received a '.', np.packbits(..., bitorder="little") line by line
    crc_<buffer>           CRC-32 of a buffer views_cases regenerates from tests/adc_cases.py (not stored)
    iq_<buffer>            the unit-circle tone and the Gaussian noise themselves, complex64
    vec_cases              the buffer names
Surface scale (draw_surface_plot, :1609-1612): for a dozen `sf` cases of tests/golden/display.npz, the constant row among them,
    sf_label_cases         int64 [k]: the case's index in display.npz
    sf_labels_<index>      the strings the reference wrote in column 0, top to bottom, joined by newlines (line i of them is display line 3 i)

    python tools/make_goldens_views.py
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import numpy as np

import make_goldens as mg            # puts the reference tree on sys.path; stubs (caller_module, Scr), stamp()
from make_goldens_adc import save_deterministic
import adc_cases as A
import display_cases as D
import views_cases as V

N_LABEL_CASES = 12


def constellation(P, d, name, x):
    assert np.all(np.isfinite(x.view(np.float32))), name
    for H, W in V.SCREENS:
        scr = mg.Scr(H, W)
        P.draw_vector_display(scr, x, 100e6, 2.4e6, 0, 0, None)
        g = np.zeros((H, W), np.uint8)
        for call in scr.calls:
            if len(call) == 4 and call[2] == ".":
                g[call[0], call[1]] = 1
        d[f"vec_{name}_{H}x{W}"] = np.packbits(g, axis=1, bitorder="little")


def scale_labels(P, c):
    scr = mg.Scr(c.H, c.W)
    P.draw_surface_plot(scr, c.rows[-1].copy(), None, 100e6, 2.4e6, 0, 0, None)
    rows = [(call[0], call[2]) for call in scr.calls if len(call) == 4 and call[1] == 0 and call[2].endswith("dB")]
    assert [y for y, _ in rows] == [i + 2 for i in range(c.disp_h) if i % 3 == 0], c.name()
    return "\n".join(s for _, s in rows)


def main():
    P = mg.caller_module()
    d = {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for name in V.ADC_BUFFERS:
            x = V.adc_buffer(name)
            d[f"crc_{name}"] = np.array(A.crc(x), np.uint32)
            constellation(P, d, name, x)
        for name in V.STORED_BUFFERS:
            x = V.stored_buffer(name)
            d[f"iq_{name}"] = x
            constellation(P, d, name, x)
        sf = [c for c in D.cases() if c.kind == "sf"]
        constant = [c for c in sf if np.ptp(c.rows[-1][np.isfinite(c.rows[-1])]) == 0]
        step = max(1, len(sf) // (N_LABEL_CASES - len(constant)))
        picked = sorted({c.i for c in constant} | {c.i for c in sf[::step][:N_LABEL_CASES - len(constant)]})
        by_i = {c.i: c for c in sf}
        for i in picked:
            d[f"sf_labels_{i}"] = np.array(scale_labels(P, by_i[i]))
        d["sf_label_cases"] = np.array(picked, np.int64)
    d["vec_cases"] = np.array(V.buffer_names())
    d["vec_screens"] = np.array(V.SCREENS, np.int64)
    d["stamp"] = np.array(mg.stamp())
    save_deterministic("views", d)
    print(len(V.buffer_names()), "buffers x", len(V.SCREENS), "screens;", len(picked), "label cases:", picked)


if __name__ == "__main__":
    main()

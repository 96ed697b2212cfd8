#!/usr/bin/env python3
"""Golden values of the header's Peak / Avg meter and of the squelch gate (tests/golden/squelch.npz) — made like
tools/make_goldens.py: the build container imports the reference's caller (pyspecsdr.py) with make_goldens' stubs, calls its own
draw_header on make_goldens' fake screen and stores DATA only.

    draw_header (pyspecsdr.py:388-392)   PEAK_POWER = np.max(freq_data); "Peak: x dB Avg: y dB" with np.mean(freq_data)
    main loop   (:2261-2263)             if PEAK_POWER >= SQUELCH: demodulate and buffer the audio
                (:2288-2291)             ui_update_counter += 1; draw_header on every third iteration
                (:171-172)               SQUELCH = -60, PEAK_POWER = 0 at start

Rows (not stored again where another fixture holds them): the 34 post-processed rows of caller.npz (`rows`), its `sg_row_big`
(32 764 bins: crosses NumPy's 8192-element summation chunk) and hand-made rows stored here as hand_<i> (a NaN bin; +inf; all -inf;
constant; lengths 1, 4, 12, 124, 128, 132, 8193).  Per row, in that order (34 + 1 + n_hand entries):
    peak   PEAK_POWER as draw_header left it          avg   np.mean(row) (asserted to format to the text the reference printed)
    text   the strength text draw_header wrote
Gate traces over the 34 caller rows as successive loop iterations, PEAK_POWER starting at 0, the counter at 0:
    trace_meta[k] = (squelch, every)     trace_open[k][i] = PEAK_POWER >= SQUELCH tested BEFORE frame i's row is metered
    trace_held[k][i] = PEAK_POWER after iteration i
and the same over the hand-made rows (hand_trace_*), whose peaks include NaN and both infinities.  every = 0: no header is drawn (the
reference's MR mode).  The comparison is made on the reference module's own globals and the metered frames call its draw_header.

    python tools/make_goldens_squelch.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import make_goldens as mg            # puts the reference tree on sys.path; stubs (caller_module, Scr), stamp(), save()

P = mg.caller_module()

SQUELCHES = (-60, 20, 35, 36, 37, 40, 50)
EVERY = (1, 3, 7)


class Sdr:
    ppm = 0
    sample_rate = 2.4e6


def header(row):
    """The reference's draw_header on a fake screen: (PEAK_POWER it left, the strength text it wrote)."""
    scr = mg.Scr(40, 400)
    with np.errstate(all="ignore"):
        P.draw_header(scr, row, None, 100e6, 2.4e6, 0, 0.1e6, Sdr)
    texts = [c[2] for c in scr.calls if isinstance(c[2], str) and c[2].startswith("Peak: ")]
    assert len(texts) == 1
    return P.PEAK_POWER, texts[0]


def hand_rows():
    rng = np.random.default_rng(4242)
    r = lambda n: -40.0 + 25.0 * rng.random(n) ** 3
    nan_row = r(1020); nan_row[333] = np.nan
    inf_row = r(1020); inf_row[7] = np.inf
    ninf_bin = r(1020); ninf_bin[1000] = -np.inf
    return [nan_row, inf_row, np.full(1020, -np.inf), ninf_bin, np.full(1020, -42.5), np.array([-17.25]), r(4), r(12), r(124), r(128), r(132),
            r(8193)]


def trace(rows, squelch, every):
    """The loop's gate over `rows` as successive iterations (pyspecsdr.py:2261, :2288-2291) on the reference module's globals."""
    P.PEAK_POWER = 0
    P.SQUELCH = squelch
    counter = 0
    opened, held = [], []
    for row in rows:
        opened.append(bool(P.PEAK_POWER >= P.SQUELCH))
        counter += 1
        if every and counter % every == 0:
            header(row)
        held.append(float(P.PEAK_POWER))
    return np.array(opened, np.uint8), np.array(held, np.float64)


def main():
    caller = np.load(os.path.join(mg.OUT, "caller.npz"))
    hand = hand_rows()
    rows = list(caller["rows"]) + [caller["sg_row_big"]] + hand
    d = {f"hand_{i}": h for i, h in enumerate(hand)}
    d["n_hand"] = np.array(len(hand))
    peak, avg, text = [], [], []
    for row in rows:
        p, t = header(row.copy())
        with np.errstate(all="ignore"):
            a = np.mean(row)
        assert t == f"Peak: {p:.1f} dB Avg: {a:.1f} dB", (t, p, a)
        peak.append(p); avg.append(a); text.append(t)
    d["peak"], d["avg"], d["text"] = np.array(peak, np.float64), np.array(avg, np.float64), np.array(text)
    # the device's dB values agree with the reference's to ~1e-12 dB (PARITY.md): no golden peak may lie that close to a squelch level,
    # or the open / closed traces from IQ would hinge on the last bits
    for p in peak[:34]:
        assert min(abs(p - s) for s in SQUELCHES) > 1e-6, p
    meta, op, he = [], [], []
    for s in SQUELCHES:
        for ev in EVERY + (0,):
            o, h = trace(rows[:34], s, ev)
            meta.append((s, ev)); op.append(o); he.append(h)
    d["trace_meta"], d["trace_open"], d["trace_held"] = np.array(meta, np.float64), np.stack(op), np.stack(he)
    meta, op, he = [], [], []
    for s in (-60, -45.0, 0, np.inf, -np.inf):
        for ev in (0, 1, 2, 3):
            o, h = trace(hand, s, ev)
            meta.append((s, ev)); op.append(o); he.append(h)
    d["hand_trace_meta"], d["hand_trace_open"], d["hand_trace_held"] = np.array(meta, np.float64), np.stack(op), np.stack(he)
    mg.save("squelch", **d)
    print(len(rows), "rows;", text[33], ";", len(d["trace_meta"]), "+", len(d["hand_trace_meta"]), "traces")


if __name__ == "__main__":
    main()

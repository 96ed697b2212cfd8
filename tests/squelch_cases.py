"""Shared by tests/test_squelch_golden.py (CPU) and tests/test_gpu_squelch.py: the rows of tests/golden/squelch.npz, NumPy models of
the header's meter and of the loop's squelch gate, the oracle's summation tree, bit comparisons.

The fixture (tools/make_goldens_squelch.py) holds, for the 34 post-processed rows of caller.npz, its sg_row_big and hand-made rows, what the
reference's own draw_header left in PEAK_POWER and wrote as text, np.mean of the row, and the gate's open / held traces.
"""
import ctypes as C
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    return np.load(os.path.join(GOLD, "squelch.npz"))


def golden_rows():
    """The fixture's rows in its order: caller.npz rows 0..33, sg_row_big, hand_0 .. hand_{n_hand-1}."""
    g, c = golden(), np.load(os.path.join(GOLD, "caller.npz"))
    return list(c["rows"]) + [c["sg_row_big"]] + [g[f"hand_{i}"] for i in range(int(g["n_hand"]))]


def same_bits(a, b):
    """Equality of float64 bits, NaN compared as NaN (any payload), a zero of either sign equal to a zero (np.max's free choice)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    zero = (a == 0) & (b == 0)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | nan | zero))


def exact_bits(a, b):
    """Equality of every float64 bit, NaN compared as NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | nan))


def meter_model(rows):
    """draw_header's two numbers per row (pyspecsdr.py:388-389): np.max, np.mean."""
    with np.errstate(all="ignore"):
        return np.array([np.max(r) for r in rows]), np.array([np.mean(r) for r in rows])


def oracle_mean(row):
    """The oracle's restatement of NumPy's summation tree, / len (the handle the other tests use, read-only)."""
    import oracle_lib as O
    fn = O.lib().pss_o_pairwise_sum_f64
    fn.restype, fn.argtypes = C.c_double, [np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS"), C.c_long]
    row = np.ascontiguousarray(row, np.float64)
    with np.errstate(all="ignore"):
        return np.float64(fn(row, len(row))) / np.float64(len(row))


def gate_model(peak, squelch, every, phase=0, held_in=0.0):
    """The reference's loop, one iteration per frame (pyspecsdr.py:2261, :2288-2291) -> (open uint8, held after every frame)."""
    held, counter = held_in, phase
    opened, helds = np.empty(len(peak), np.uint8), np.empty(len(peak), np.float64)
    for i, p in enumerate(peak):
        opened[i] = held >= squelch
        counter += 1
        if every and counter % every == 0:
            held = p
        helds[i] = held
    return opened, helds


def random_rows(n_rows, length, seed):
    """Seeded rows of dB-like values with the special rows mixed in: a NaN bin, +inf, -inf bins, all -inf, constant, signed zeros."""
    rng = np.random.default_rng(seed)
    rows = -40.0 + 25.0 * rng.random((n_rows, length)) ** 3
    for r in range(n_rows):
        k = r % 11
        pos = int(rng.integers(0, length))
        if k == 3:
            rows[r, pos] = np.nan
        elif k == 5:
            rows[r, pos] = np.inf
        elif k == 6:
            rows[r, pos] = -np.inf
        elif k == 7:
            rows[r] = -np.inf
        elif k == 8:
            rows[r] = -42.5
        elif k == 9:
            rows[r] *= 1e-3
            rows[r, pos] = np.inf
            rows[r, int(rng.integers(0, length))] = -np.inf     # np.mean: NaN when both infinities meet
    return rows

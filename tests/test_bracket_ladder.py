"""tools/bracket_ladder.py on 256 rows: the table's columns, and the finding the first rung of the compacting selects rests on — the +-0.5 dB
bracket around a benchmark row's mean holds more than CAP = 128 of its 1020 smoothed values on more than half of the rows."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bracket_ladder as B  # noqa: E402

NARROW = 0.35     # pss_post.h: bracket_db(0)


def _tables():
    sm = B.smoothed_rows(B.synth("fm", 256, 11))
    return {mode: B.table(sm, (NARROW, 0.5), mode) for mode in ("sum32", "sum64")}


def test_columns_and_the_half_db_bracket_overflowing():
    t = _tables()
    for mode, recs in t.items():
        assert [r["half_width"] for r in recs] == [NARROW, 0.5]
        for r in recs:
            assert set(r) == set(B.COLUMNS)
            assert 0 < r["M_p50"] <= r["M_p99"] <= r["M_max"] <= B.M_ROW and 0.0 <= r["k_k1_inside"] <= r["k_inside"] <= 1.0
            assert r["sweeps"] >= 2.0
        narrow, half = recs
        assert half["over_cap"] > 0.5, f"+-0.5 dB: M > {B.CAP} on {half['over_cap']:.3f} of the rows"
        assert half["M_mean"] > B.CAP
        assert narrow["over_cap"] < 0.02 and narrow["k_inside"] > 0.95
        assert narrow["sweeps"] < half["sweeps"] - 1.0           # the ladder with the narrow rung in front saves more than a sweep per row
    # the hint summed in float64 and rounded once brackets the same keys as the float32 running sum
    for a, b in zip(t["sum32"], t["sum64"]):
        for c in ("M_mean", "over_cap", "k_inside", "k_k1_inside", "sweeps"):
            assert abs(a[c] - b[c]) <= 0.01 * max(1.0, abs(a[c])), (c, a[c], b[c])


def test_high_word_image_orders_like_the_values():
    v = np.array([-np.inf, -100.0, -1.5, -0.0, 0.0, 1e-300, 2.0, 1e300, np.inf])
    h = B.hi_word(v)
    assert np.all(np.diff(h) >= 0) and h[0] < h[1] and h[-2] < h[-1]
    assert B.hi_word(np.array([-50.0]))[0] == (~np.array([-50.0]).view(np.uint64)[0]) >> np.uint64(32)

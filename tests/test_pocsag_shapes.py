"""The inputs of tests/test_gpu_pocsag.py's shape cases on the CPU — the thousands of one-tile rows, and the sync train whose rank cut falls
past one pass of the wavefront kernels — against the NumPy statement of tests/pocsag_cases.py, so that "device = twin" there and "twin =
statement" here meet on the same arrays.  No GPU."""
import numpy as np
import pytest

import pocsag_cases as P
from bytes_util import same_bytes
from pocsag_caps import DETECT_GRID_CAP, SCAN_STEP, WAVE_PASS
from pyspecsdr_amd.engine import Engine as E

WHAT = ("cw", "fix", "row", "pos", "meta", "score")
R = SCAN_STEP + 1


@pytest.mark.parametrize("dense", [False, True])
def test_one_tile_rows_twin_is_the_statement_on_a_sample_of_rows(dense):
    """The twin runs all 4097 rows.  The statement (a Python loop over every strobe of every survivor) restates a SUBSET: rows 0 and 4096,
    and the first, a middle and the last row of each of the detect grid's five rounds (P.round_sample: 13 rows).  The other rows are held
    to the formula of their positions and to the words that were sent."""
    y = P.short_rows(R, DETECT_GRID_CAP, dense)
    rows = list(range(R)) if dense else P.carrying(R, DETECT_GRID_CAP)
    twin = E.h_pocsag_batches(y, P.SHORT_SPB, max_batches=R + 10)
    assert twin[6] == len(rows) and twin[2].tolist() == rows and twin[3].tolist() == [P.short_start(r) for r in rows]
    assert np.all(twin[0] == np.array(P.WORDS, np.uint32)) and not twin[1].any()
    sample = P.round_sample(R, DETECT_GRID_CAP)
    assert sample[0] == 0 and sample[-1] == R - 1 and {r // DETECT_GRID_CAP for r in sample} == {0, 1, 2, 3, 4}
    stats = {}
    ref = P.numpy_batches(y[sample], P.SHORT_SPB, stats=stats)
    pick = np.isin(twin[2], sample)
    assert ref[6] == int(pick.sum()) and [sample[k] for k in ref[2]] == twin[2][pick].tolist()
    assert stats["survivors"] == (2 if dense else 1) * ref[6]
    for i in (0, 1, 3, 4, 5):
        assert same_bytes(twin[i][pick], ref[i]), WHAT[i]
    for room in (0, len(rows) // 2 + 3):
        cut = E.h_pocsag_batches(y, P.SHORT_SPB, max_batches=room)
        assert cut[6] == len(rows) and all(same_bytes(c, t[:room]) for c, t in zip(cut[:6], twin[:6]))


def test_the_sync_train_cut_past_one_pass_of_the_wave_kernels():
    """Every word of the train is the same, so the statement runs on its first 60 words and on the 60 around the cut; the twin's records in
    between are held to the formula."""
    y, starts = P.sync_train(WAVE_PASS // 2 + 40)
    twin = E.h_pocsag_batches(y, 2, max_batches=len(starts) + 10)
    assert twin[6] == len(starts) and twin[3].tolist() == starts and len({bytes(w) for w in twin[0]}) == 1 and len(set(twin[5].tolist())) == 1
    for w0 in (0, WAVE_PASS // 2 - 20):
        lo, hi = 64 * w0, 64 * (w0 + 60) + 7
        stats = {}
        ref = P.numpy_batches(y[lo:hi], 2, stats=stats)
        assert ref[6] == 60 - 16 and stats["survivors"] == 2 * ref[6] and (ref[3] + lo).tolist() == starts[w0:w0 + 44]
        for i in (0, 1, 4, 5):
            assert same_bytes(ref[i], twin[i][w0:w0 + 44]), WHAT[i]
    for max_batches in (WAVE_PASS // 2 + 9, WAVE_PASS // 2 + 10, WAVE_PASS // 2 + 11):
        assert 2 * max_batches > WAVE_PASS
        cut = E.h_pocsag_batches(y, 2, max_batches=max_batches)
        assert cut[6] == len(starts) and all(same_bytes(c, t[:max_batches]) for c, t in zip(cut[:6], twin[:6]))

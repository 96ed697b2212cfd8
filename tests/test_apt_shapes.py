"""The inputs of tests/test_gpu_apt.py's shape cases on the CPU — the thousands of one-tile rows, the 1709-tile train with its rank cut past
one pass of the lane kernels, and k_apt_front's grid of decimations and tap counts — against the NumPy statement of tests/apt_cases.py, so
that "device = twin" there and "twin = statement" here meet on the same arrays.  No GPU."""
import numpy as np
import pytest

import apt_cases as A
from apt_caps import DETECT_GRID_CAP, LANE_PASS, NEAR, REACH, SCAN_STEP, TILE, front_tile
from bytes_util import same_bytes
from pyspecsdr_amd.engine import Engine as E

WHAT = ("row", "pos", "meta", "score")
R = SCAN_STEP + 1


@pytest.mark.parametrize("dense", [False, True])
def test_one_tile_rows_twin_is_the_statement_on_a_sample_of_rows(dense):
    """The twin runs all 4097 rows.  The statement (a Python loop over every pair of survivors) restates a SUBSET: rows 0 and 4096, and
    the first, a middle and the last row of each of the detect grid's five rounds (A.round_sample: 13 rows).  The other rows are held to
    the formula of their positions, which is all the statement would say of them: every row is a shifted copy of the same 300 samples."""
    env = A.short_rows(R, DETECT_GRID_CAP, dense)
    rows = list(range(R)) if dense else A.carrying(R, DETECT_GRID_CAP)
    se = 4 if dense else 0
    twin = E.h_apt_syncs(env, sync_errors=se, max_syncs=R + 10)
    assert twin[4] == len(rows) and twin[0].tolist() == rows and twin[1].tolist() == [A.short_start(r, dense) for r in rows]
    sample = A.round_sample(R, DETECT_GRID_CAP)
    assert sample[0] == 0 and sample[-1] == R - 1 and {r // DETECT_GRID_CAP for r in sample} == {0, 1, 2, 3, 4}
    ref = A.numpy_syncs(env[sample], se)
    pick = np.isin(twin[0], sample)
    assert ref[4] == int(pick.sum()) and [sample[k] for k in ref[0]] == twin[0][pick].tolist()
    for t, r, what in zip(twin[1:4], ref[1:4], WHAT[1:]):
        assert same_bytes(t[pick], r), what
    for room in (0, len(rows) // 2 + 3):
        cut = E.h_apt_syncs(env, sync_errors=se, max_syncs=room)
        assert cut[4] == len(rows) and all(same_bytes(c, t[:room]) for c, t in zip(cut[:4], twin[:4]))


def test_the_train_with_two_strong_syncs_past_one_pass_of_the_lane_kernels():
    """The statement's pair loop over 538 000 survivors is out of reach, so it runs on the stretches that hold the records (each with NEAR
    samples either side, which is all the one-record rule looks at) and on one stretch of the plain train, where it finds no record."""
    strong = [1500 * TILE + 7, 1680 * TILE + 11, 1700 * TILE + 5]
    env = A.dense_train(1709, strong)
    twin = E.h_apt_syncs(env, sync_errors=4, max_syncs=64)
    assert twin[4] == 5 and twin[1].tolist()[-3:] == strong and twin[1].tolist()[0] == 0
    per_tile = len(A.candidates(env[20 * TILE:21 * TILE + REACH], 4)[0])
    assert per_tile * (1680 - 4) > LANE_PASS
    for pos in twin[1].tolist() + [900 * TILE]:
        lo, hi = max(0, pos - NEAR), pos + NEAR + REACH
        piece = env[lo:hi]
        part = E.h_apt_syncs(piece, sync_errors=4, s_begin=pos - lo, s_end=pos - lo + 1)
        ref = A.numpy_syncs(piece, 4, s_begin=pos - lo, s_end=pos - lo + 1)
        for t, r, what in zip(part[:4], ref[:4], WHAT):
            assert same_bytes(t, r), (pos, what)
        k = twin[1].tolist().index(pos) if pos in twin[1].tolist() else None
        assert part[4] == ref[4] == (k is not None)
        if k is not None:
            assert part[2][0] == twin[2][k] and part[3][0] == twin[3][k]
    for room in (3, 4, 5):
        cut = E.h_apt_syncs(env, sync_errors=4, max_syncs=room)
        assert cut[4] == 5 and cut[1].tolist() == twin[1].tolist()[:room]


@pytest.mark.parametrize("decim", A.GRID_DECIMS)
def test_front_grid_within_one_ulp_of_the_float64_statement(decim):
    """Every grid point of tests/test_gpu_apt.py's front grid, with the bound of tests/test_apt_golden.py: one float32 ulp of the larger of
    the two values."""
    for n_taps in A.GRID_TAPS:
        x, taps = A.grid_case(decim, n_taps, front_tile(decim, n_taps))
        got = E.h_apt_front(x, decim=decim, taps=taps)
        d = E.h_ais_front(x, pulse=np.array([1.0]))
        ref = A.numpy_front(d, taps, decim=decim)
        assert got.dtype == np.float32 and got.shape == ref.shape == (2 * front_tile(decim, n_taps) + 3,)
        ulp = np.spacing(np.maximum(ref, got).astype(np.float32)).astype(np.float64)
        assert np.max(np.abs(got - ref) / ulp) <= 1.0, (decim, n_taps)

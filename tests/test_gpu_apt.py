"""The APT kernels (k_apt_front; k_apt_detect, pss_starts.h's k_starts_scan and k_starts_gather, k_apt_score, k_apt_keep, k_apt_emit;
k_apt_lines) against pss_h_apt_front, pss_h_apt_syncs and pss_h_apt_lines on every byte of every output, and formats.apt_recording end to
end.  Buffers lie between NaNs, rows are strided with NaNs in the gaps, and a sentinel sits behind every output.  The shapes are the smallest
at which each path is taken: 1, 79 and 4097 taps, the lead at both ends, windows with exactly their halo, a row index past 2^40, one (row,
tile) pair past the front's grid cap; syncs on both sides of a tile boundary and across it, more survivors in a tile than a wavefront holds,
more survivors than one pass of the lane kernels and more tiles than the detect grid (one case), rows that must not run into each other,
sync_errors 0 and 4, the row's last candidate, a count above max_syncs, windows with exactly their reach; lines at negative positions and
past the end, 0, 1 and one line past the gather's grid cap, unsorted positions, mixed rows.  Shapes (tests/test_apt_shapes.py runs the
same arrays on the CPU): the front over a grid of ten decimations and nine tap counts and windows on three strided rows; 4097 one-tile rows
(the counts' scan carries, the gather's grid walks twice, detect workgroups alternate tiles with and without survivors); a rank cut past
one pass of the lane kernels.  The caps and tile sizes come from
tests/apt_caps.py, where tests/test_apt_caps.py and, for the start list, tests/test_launch_caps.py pin them to the source lines."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import apt_cases as A
from apt_caps import (BLOCK, DETECT_GRID_CAP, FRONT_GRID_CAP, FRONT_WAVES, GATHER_GRID_CAP, LANE_PASS, LINES_GRID_CAP, NEAR, REACH, SCAN_STEP, TILE, WAVE,
                      front_tile)   # pinned by tests/test_apt_caps.py
from bytes_util import same_bytes
from gpu_util import dev
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine

pytestmark = pytest.mark.gpu

WHAT = ("row", "pos", "meta", "score")
assert A.TILE == TILE
_ENV = {}


@pytest.fixture(scope="module")
def e():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    eng = Engine(0)
    yield eng
    eng.close()


def case_env(name):
    if name not in _ENV:
        env = Engine.h_apt_front(A.case_row(name))
        env.setflags(write=False)
        _ENV[name] = env
    return _ENV[name]


def strided(rows, gap, fill=np.nan):
    """[R][n] -> a flat device tensor holding the rows `n + gap` apart between `fill`s, two elements of fill in front; -> (tensor, offset of
    row 0 in elements, stride)."""
    rows = np.ascontiguousarray(rows)
    r, n = rows.shape
    stride = n + gap
    wide = np.full(2 + r * stride + 2, fill, rows.dtype)
    for k in range(r):
        wide[2 + k * stride:2 + k * stride + n] = rows[k]
    return dev(wide), 2, stride


# ---- front ------------------------------------------------------------------------------------------------------------------------------------
def front_on_device(e, x, fs=62400.0, decim=5, taps=None, lead=None, buf_index0=0, n_row=None, m_begin=0, m_end=None, gap=3):
    x = np.asarray(x, np.complex64)
    rows = x[None, :] if x.ndim == 1 else x
    r, n = rows.shape
    n_row = buf_index0 + n if n_row is None else n_row
    m_end = -(-n_row // decim) if m_end is None else m_end
    m = m_end - m_begin
    d_iq, off, stride = strided(rows, gap)
    d_env = torch.full((r, m + 2), -7.0, dtype=torch.float32, device="cuda")
    e.apt_front(d_iq.data_ptr() + 8 * off, r, n, d_env, fs=fs, decim=decim, taps=taps, x_stride=stride, buf_index0=buf_index0, n_row=n_row, lead=lead,
                m_begin=m_begin, m_end=m_end, env_stride=m + 2)
    e.sync()
    out = d_env.cpu().numpy()
    assert np.all(out[:, m:] == -7.0)
    return out[:, :m] if x.ndim == 2 else out[0, :m]


def front_check(e, x, **kw):
    want = Engine.h_apt_front(x, **kw)
    got = front_on_device(e, x, **kw)
    assert same_bytes(got, want), (kw, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    return want


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_front_fixture_rows(e, name):
    assert same_bytes(front_check(e, A.case_row(name)), case_env(name))


def test_front_tap_counts_leads_and_rates(e):
    from scipy.signal import firwin
    x = A.case_row("noise_10db_3khz_40ppm")[:30011]
    for taps, lead in ((np.array([1.0]), None), (np.array([-2.5]), 0), (None, None), (None, 0), (None, 78), (firwin(4097, 0.01), None),
                       (firwin(4097, 0.01), 0), (firwin(4097, 0.01), 4096), (firwin(130, 0.05), 17)):
        front_check(e, x, taps=taps, lead=lead)
    front_check(e, x, fs=249600.0, decim=7, taps=firwin(201, 0.05))
    front_check(e, x, decim=1)
    front_check(e, x[:6000], decim=4096, taps=firwin(4097, 0.01))
    front_check(e, np.stack([x[:9000], x[9000:18000], x[18000:27000]]))
    bad = x[:9000].copy()
    bad[4000], bad[5000] = np.nan, np.inf
    front_check(e, bad)
    for n in (1, 2, 3, 80):
        front_check(e, x[:n])


def test_front_windows_with_exactly_their_halo_and_a_row_index_past_2_40(e):
    x = A.case_row("smooth_30db")[:30000]
    n = len(x)
    whole = Engine.h_apt_front(x)
    for m0, m1 in ((0, 1), (17, 18), (100, 4000), (895, 897), (5990, 6000)):
        lo, hi = max(0, m0 * 5 + 39 - 78 - 1), min(n, (m1 - 1) * 5 + 39 + 1)
        got = front_on_device(e, x[lo:hi], buf_index0=lo, n_row=n, m_begin=m0, m_end=m1)
        assert same_bytes(got, whole[m0:m1]), (m0, m1)
    big = (1 << 40) + 123456
    index0 = (1 << 40) + 77
    m0, m1 = (index0 + 80) // 5 + 1, (index0 + 20000) // 5 - 40
    want = front_check(e, x[:20080], buf_index0=index0, n_row=big, m_begin=m0, m_end=m1)
    assert len(want) == m1 - m0 and np.isfinite(want).all() and want.max() > 0.1      # (the rotor's phase follows from the index in the ROW)


def test_front_one_pair_past_the_grid_cap(e):
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((FRONT_GRID_CAP + 1, 120)) + 1j * rng.standard_normal((FRONT_GRID_CAP + 1, 120))).astype(np.complex64)
    front_check(e, rows)                                            # one tile a row: 2049 pairs
    m = front_tile(5, 79)
    x = A.case_row("smooth_30db")[:5 * (2 * m + 3)]
    front_check(e, x)                                               # three tiles of one row, the last of three outputs


@pytest.mark.parametrize("decim", A.GRID_DECIMS)
def test_front_grid_of_decimations_and_tap_counts(e, decim):
    """Two whole tiles and one of three outputs at every tap count of the grid: 1, 2 and 3 tap blocks at every decimation, the tile that
    STAGE_CAP shrinks (decim 13 to 1000 with few taps), groups of 64 outputs that are no multiple of the workgroup's wavefronts beside many
    blocks."""
    for n_taps in A.GRID_TAPS:
        m = front_tile(decim, n_taps)
        x, taps = A.grid_case(decim, n_taps, m)
        assert -(-len(x) // decim) == 2 * m + 3
        front_check(e, x, decim=decim, taps=taps)


def test_the_front_grid_reaches_the_shapes_it_is_there_for():
    """(no device work) What the grid's points are, from the tile's own figures: block counts 1, 2, 3 at decimations other than 5; a tile
    cut by STAGE_CAP below its PART_CAP share; a count of 64-output groups that is no multiple of the wavefronts with more than 16 blocks."""
    shapes = {(d, t): (front_tile(d, t), -(-t // BLOCK)) for d in A.GRID_DECIMS for t in A.GRID_TAPS}
    for d in A.GRID_DECIMS:
        assert {shapes[d, t][1] for t in A.GRID_TAPS} >= {1, 2, 3}
    from apt_caps import PART_CAP
    assert all(shapes[d, 1][0] < PART_CAP for d in (13, 64, 100, 1000)) and shapes[1, 1][0] == PART_CAP
    assert any(nb > FRONT_WAVES and -(-m // 64) % FRONT_WAVES for (m, nb) in shapes.values())


@pytest.mark.parametrize("decim,n_taps", [(5, 79), (8, 65)])
def test_front_windows_of_three_rows_with_exactly_their_halo(e, decim, n_taps):
    """The window test again with three different rows 3 NaNs apart: row * x_stride is not 0 where lo > 0."""
    from scipy.signal import firwin
    taps = firwin(n_taps, 1.0 / (3 * decim))
    rows = np.stack([A.case_row(name)[:30000] for name in sorted(A.CASES)])
    n = rows.shape[1]
    whole = Engine.h_apt_front(rows, decim=decim, taps=taps)
    n_m = whole.shape[1]
    assert n_m == -(-n // decim) and not same_bytes(whole[0], whole[1]) and not same_bytes(whole[1], whole[2])
    for m0, m1 in ((0, 1), (17, 18), (100, n_m - 2000), (front_tile(decim, n_taps) - 1, front_tile(decim, n_taps) + 1), (n_m - 10, n_m)):
        lo, hi = A.halo(m0, m1, decim, n_taps, n)
        got = front_on_device(e, rows[:, lo:hi], decim=decim, taps=taps, buf_index0=lo, n_row=n, m_begin=m0, m_end=m1, gap=3)
        assert same_bytes(got, whole[:, m0:m1]), (m0, m1)


# ---- syncs ------------------------------------------------------------------------------------------------------------------------------------
def syncs_on_device(e, env, sync_errors=2, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_syncs=None, gap=3):
    env = np.asarray(env, np.float32)
    rows = env[None, :] if env.ndim == 1 else env
    r, n = rows.shape
    n_row = buf_index0 + n if n_row is None else n_row
    s_end = n_row if s_end is None else s_end
    d_env, off, stride = strided(rows, gap)
    ms = 256 if max_syncs is None else max_syncs
    room = ms + 3
    d_row = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_pos = torch.full((room,), -7, dtype=torch.int64, device="cuda")
    d_meta = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_score = torch.full((room,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    e.apt_syncs(d_env.data_ptr() + 4 * off, r, n, d_row, d_pos, d_meta, d_score, d_count, ms, sync_errors=sync_errors, e_stride=stride,
                buf_index0=buf_index0, n_row=n_row, s_begin=s_begin, s_end=s_end)
    e.sync()
    rw, pos, meta, score, count = (t.cpu().numpy() for t in (d_row, d_pos, d_meta, d_score, d_count))
    assert count[1] == -7
    k = min(int(count[0]), ms)
    assert np.all(rw[k:] == -7) and np.all(pos[k:] == -7) and np.all(meta[k:] == -7) and np.all(score[k:] == -7.0)
    return rw[:k], pos[:k], meta[:k].view(np.uint32), score[:k], int(count[0])


def check(e, env, sync_errors=2, max_syncs=256, gap=3, **kw):
    """Device == twin on every byte -> the twin's result."""
    want = Engine.h_apt_syncs(env, sync_errors=sync_errors, max_syncs=max_syncs, **kw)
    got = syncs_on_device(e, env, sync_errors=sync_errors, max_syncs=max_syncs, gap=gap, **kw)
    for g, w, what in zip(got[:4], want[:4], WHAT):
        assert same_bytes(g, w), (what, g, w)
    assert got[4] == want[4]
    return want


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_syncs_fixture_rows(e, name):
    env = case_env(name)
    for se in range(5):
        r = check(e, env, se)
        assert r[4] == 3 and np.all(np.abs(r[1] - A.case_starts(name)) <= 2)
    noise = np.abs(np.random.default_rng(7).standard_normal(3 * TILE + 50)).astype(np.float32)
    check(e, noise, 4)


def test_syncs_on_both_sides_of_a_tile_boundary_and_across_it(e):
    n = 3 * TILE
    rows = np.stack([A.sync_env(n, [TILE - 1]), A.sync_env(n, [TILE]), A.sync_env(n, [TILE - 60]), A.sync_env(n, [TILE - REACH, 2 * TILE - 1])])
    for se in (0, 4):
        r = check(e, rows, se)
        assert r[0].tolist() == [0, 1, 2, 3, 3] and r[1].tolist() == [TILE - 1, TILE, TILE - 60, TILE - REACH, 2 * TILE - 1]
    both = A.sync_env(n, [TILE - 1, TILE + REACH])                    # neighbours in two tiles: the earlier drops the later
    assert check(e, both, 0)[1].tolist() == [TILE - 1]


def test_more_survivors_in_a_tile_than_a_wavefront_holds(e):
    n = 2 * TILE + 300
    starts = list(range(5, n - REACH, REACH))
    env = A.sync_env(n, starts, full=True)                           # three survivors a sync at sync_errors = 0, nine at 4
    s, _, _ = A.candidates(env, 0)
    assert np.sum(s < TILE) > WAVE and len(s) == 3 * len(starts)
    for se in (0, 4):
        r = check(e, env, se)
        assert r[4] == 1 and r[1].tolist() == [4]                    # equal scores: the earliest of each neighbourhood, and NEAR holds them all
    apart = list(range(5, 4 * TILE - REACH, NEAR + 2))              # the last survivor of one and the first of the next: NEAR apart
    r = check(e, A.sync_env(4 * TILE, apart, full=True), 4)
    assert r[1].tolist() == [s - 1 for s in apart]
    r = check(e, A.sync_env(4 * TILE, list(range(5, 4 * TILE - REACH, NEAR + 1)), full=True), 4)
    assert r[1].tolist() == [4]                                      # one sample closer and each is dropped by the one before it
    # graded scores: every sync stronger than the one before it, so only the last of each neighbourhood stays
    graded = np.full(n, 0.2, np.float32)
    for k, s0 in enumerate(starts):
        graded[s0:s0 + REACH] = A.sync_env(REACH, [0], high=1.0 + 0.01 * k)
    check(e, graded, 0)
    check(e, graded, 4, max_syncs=0)


def test_more_survivors_than_one_pass_and_more_tiles_than_the_detect_grid(e):
    """Sync A every 117 samples, three samples a word, sync_errors = 4: nine survivors a sync.  7.0 M envelope samples (28 MB) hold 1709
    tiles, past the detect grid cap of 1024, and 538 000 survivors, past one pass of the lane kernels (524 288)."""
    n = 1709 * TILE - 1000
    unit = A.sync_env(REACH, [0], full=True)
    env = np.tile(unit, n // REACH + 1)[:n].copy()
    env[5 * TILE:5 * TILE + 3 * NEAR] = 0.2                          # a quiet stretch: the syncs at its edges have one-sided neighbourhoods
    env[1500 * TILE + 7:1500 * TILE + 7 + REACH] = A.sync_env(REACH, [0], high=3.0)   # and one sync that beats its neighbours past the grid cap
    assert n // TILE + 1 > DETECT_GRID_CAP
    want = Engine.h_apt_syncs(env, sync_errors=4, max_syncs=64)
    d_env = dev(env)
    d_row = torch.full((67,), -7, dtype=torch.int32, device="cuda")
    d_pos = torch.full((67,), -7, dtype=torch.int64, device="cuda")
    d_meta = torch.full((67,), -7, dtype=torch.int32, device="cuda")
    d_score = torch.full((67,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    e.apt_syncs(d_env, 1, n, d_row, d_pos, d_meta, d_score, d_count, 64, sync_errors=4)
    e.sync()
    k = min(want[4], 64)
    assert int(d_count.cpu()[0]) == want[4] and want[4] >= 3
    assert same_bytes(d_pos.cpu().numpy()[:k], want[1]) and same_bytes(d_score.cpu().numpy()[:k], want[3]) and bool((d_pos[k:] == -7).all())
    assert 1500 * TILE + 7 in want[1].tolist()
    # the survivors themselves, counted by the detect pass alone: a window whose keep rule has nothing to drop is not at hand, so count them
    # on the host over a stretch and scale
    s, _, _ = A.candidates(env[20 * TILE:21 * TILE + REACH], 4)
    assert len(s) * (n // TILE - 4) > LANE_PASS


@pytest.mark.parametrize("dense", [False, True])
def test_thousands_of_one_tile_rows_the_counts_carry_and_the_gathers_second_pass(e, dense):
    """SCAN_STEP + 1 rows of 300 samples: tpr == 1, one tile past a step of the counts' scan and two passes of the gather's grid.  Plain:
    the rows of every other round of the detect grid carry one sync, so every workgroup meets tiles with, without, with, without survivors
    and workgroup 0 a fifth with them; the carry into the last tile is 2048.  dense: nine survivors in every tile: the carry is 36 000."""
    R = SCAN_STEP + 1
    assert R > GATHER_GRID_CAP and R > 4 * DETECT_GRID_CAP
    env = A.short_rows(R, DETECT_GRID_CAP, dense)
    rows = list(range(R)) if dense else A.carrying(R, DETECT_GRID_CAP)
    se = 4 if dense else 0
    full = check(e, env, se, max_syncs=R + 10)
    assert full[4] == len(rows) == (R if dense else 2 * DETECT_GRID_CAP + 1)
    assert full[0].tolist() == rows and full[1].tolist() == [A.short_start(r, dense) for r in rows]
    assert check(e, env, se, max_syncs=0)[4] == len(rows)
    cut = check(e, env, se, max_syncs=len(rows) // 2 + 3)
    assert cut[4] == len(rows) and cut[0].tolist() == rows[:len(rows) // 2 + 3]


def test_the_rank_cut_falls_past_one_pass_of_the_lane_kernels(e):
    """The 1709-tile train with two strong syncs whose survivor indices lie past LANE_PASS: max_syncs cuts the second of them, then neither,
    then both."""
    n_tiles = 1709
    strong = [1500 * TILE + 7, 1680 * TILE + 11, 1700 * TILE + 5]
    env = A.dense_train(n_tiles, strong)
    s, _, _ = A.candidates(env[20 * TILE:21 * TILE + REACH], 4)
    assert len(s) * (1680 - 4) > LANE_PASS                            # the survivors in front of the last two, counted over a stretch
    d_env = dev(env)
    whole = Engine.h_apt_syncs(env, sync_errors=4, max_syncs=64)
    assert whole[4] == len(whole[1]) and whole[1].tolist()[-3:] == strong
    for room in (whole[4] - 1, whole[4], whole[4] - 2):
        out = [torch.full((room + 3,), -7, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32, torch.float32)]
        d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        e.apt_syncs(d_env, 1, len(env), *out, d_count, room, sync_errors=4)
        e.sync()
        assert int(d_count.cpu()[0]) == whole[4]
        k = min(room, whole[4])
        for t, w, what in zip(out, whole[:4], WHAT):
            got = t.cpu().numpy()
            assert same_bytes(got[:k].view(w.dtype), w[:k]), (room, what)
            assert np.all(got[k:] == -7), (room, what)


def test_rows_do_not_run_into_each_other_the_last_candidate_and_max_syncs(e):
    two = np.stack([A.sync_env(500, [500 - 60]), A.sync_env(500, [])])
    two[1, :57] = A.sync_env(117, [0])[60:]
    assert check(e, two, 4, gap=0)[4] == 0                           # rows back to back in memory
    assert check(e, A.sync_env(300 + 117, [300]), 0)[1].tolist() == [300] and check(e, A.sync_env(300 + 116, [300]), 0)[4] == 0
    for m in (1, 116, 117):
        check(e, np.ones(m, np.float32), 4)
    starts = [500, 500 + NEAR + 7, 20000, 33000]
    env = A.sync_env(40000, starts, full=True)
    for room in (0, 1, 3, 4, 9):
        r = check(e, env, 0, max_syncs=room)
        assert r[4] == 4 and len(r[1]) == min(room, 4)
    for bad in (np.nan, np.inf, -np.inf):
        z = A.sync_env(3000, [700])
        z[700 + 31] = bad
        check(e, z, 4)
        z[:] = bad
        check(e, z, 4)


def test_syncs_windows_with_exactly_their_reach(e):
    env = np.stack([case_env("noise_10db_3khz_40ppm")[:19000], case_env("smooth_30db")[:19000]])
    n = env.shape[1]
    whole = check(e, env, 4)
    assert whole[4] == 6
    parts = []
    cuts = [0, 556, 557, TILE, 6796, 9000, n - 116, n]
    for s0, s1 in zip(cuts[:-1], cuts[1:]):
        lo, hi = max(0, s0 - 3119), min(n, s1 + 3118 + 117)
        parts.append(check(e, env[:, lo:hi], 4, buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
    order = np.lexsort((np.concatenate([q[1] for q in parts]), np.concatenate([q[0] for q in parts])))
    for i in range(4):
        assert same_bytes(np.concatenate([q[i] for q in parts])[order], whole[i]), i
    env2 = A.sync_env(9000, [1000, 1117])
    assert check(e, env2, 0, s_begin=1100, s_end=1200)[4] == 0       # a neighbour outside the window still counts
    assert check(e, env2, 0, s_begin=7, s_end=7)[4] == 0


# ---- lines ------------------------------------------------------------------------------------------------------------------------------------
def lines_check(e, env, line_row, line_pos, gap=5):
    env = np.asarray(env, np.float32)
    rows = env[None, :] if env.ndim == 1 else env
    r, n = rows.shape
    lr, lp = np.asarray(line_row, np.int32), np.asarray(line_pos, np.int64)
    want = Engine.h_apt_lines(rows, lr, lp)
    d_env, off, stride = strided(rows, gap)
    d_words = torch.full((len(lp) + 1, 2083), -7.0, dtype=torch.float32, device="cuda")
    e.apt_lines(d_env.data_ptr() + 4 * off, r, n, dev(lr) if len(lr) else None, dev(lp) if len(lp) else None, len(lp), d_words, e_stride=stride,
                words_stride=2083)
    e.sync()
    got = d_words.cpu().numpy()
    assert np.all(got[:, 2080:] == -7.0) and np.all(got[len(lp):] == -7.0)
    assert same_bytes(got[:len(lp), :2080], want)
    return want


def test_lines_positions_counts_and_rows(e):
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((3, 20000)).astype(np.float32)
    n = rows.shape[1]
    pos = [-100, 0, n - 6240, n - 3000, -6239, -6240, n - 1, n, 5, -2 ** 62, 2 ** 62, 7, 13000, 1, 6241]           # unsorted, hanging over both ends
    row = [0, 1, 2, 1, 0, 2, 0, 1, 2, 0, 1, 2, 7, -1, 0]                                                          # mixed; rows 7 and -1 do not exist
    w = lines_check(e, rows, row, pos)
    assert not w[5].any() and not w[9].any() and not w[12].any() and not w[13].any() and w[0, 33] == rows[0, 0] and w[0, 32] == 0.0
    lines_check(e, rows, [], [])
    lines_check(e, rows, [2], [77])
    many = rng.integers(-7000, n + 1000, LINES_GRID_CAP + 1)
    lines_check(e, rows, rng.integers(0, 3, LINES_GRID_CAP + 1), many)                                            # one line past the grid cap
    lines_check(e, np.ones(1, np.float32), [0, 0], [0, -1])
    env = case_env("smooth_30db")
    r = Engine.h_apt_syncs(env)
    lp, found = F.apt_grid(r[1], r[2], r[3], len(env))
    assert found.all() and len(lp) == 3
    lines_check(e, env, np.zeros(3, np.int32), lp)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_a_refused_device_call_writes_nothing(e):
    from pyspecsdr_amd.engine import PssError
    x = A.case_row("smooth_30db")[:2000]
    d_iq = dev(x)
    d_env = torch.full((400,), -7.0, dtype=torch.float32, device="cuda")
    for why, kw in (("fs must be finite and above 4800 (the 2400 Hz subcarrier below the discriminator's Nyquist)", dict(fs=4800.0)),
                    ("decim outside [1, 4096]", dict(decim=0)), ("n_taps outside [1, 4097]", dict(taps=np.ones(4098))), ("n_rows < 1", dict(n_rows=0)),
                    ("x_stride < n_buf", dict(x_stride=1999)), ("lead outside [0, n_taps - 1]", dict(lead=79)),
                    ("a tap that is not finite", dict(taps=np.array([1.0, np.nan]))), ("[m_begin, m_end) outside [0, ceil(n_capture / decim)]", dict(m_end=401)),
                    ("out_stride < m_end - m_begin", dict(env_stride=399)),
                    ("an output needs a sample of the capture that the buffer does not hold", dict(buf_index0=5, n_row=2005)),
                    ("d_iq must be 8-byte and d_env 4-byte aligned", dict(iq=d_iq.data_ptr() + 4))):
        kw = dict(kw)
        with pytest.raises(PssError, match=re.escape("pss_apt_front: " + why)):
            e.apt_front(kw.pop("iq", d_iq), kw.pop("n_rows", 1), 2000, d_env, **kw)
    e.sync()
    assert bool((d_env == -7.0).all())
    e.apt_front(d_iq, 1, 2000, d_env)
    e.sync()
    assert same_bytes(d_env.cpu().numpy(), Engine.h_apt_front(x))
    # ---- syncs
    env = A.sync_env(9000, [4000])
    n = len(env)
    d_e = dev(env)
    d_row, d_meta = torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int32, device="cuda")
    d_pos, d_score = torch.full((4,), -7, dtype=torch.int64, device="cuda"), torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    reach = "the buffer does not cover the window's reach (3119 starts either side, 117 samples forward)"
    for why, kw in (("n_rows outside [1, 2^20]", dict(n_rows=0)), ("sync_errors outside [0, 4]", dict(sync_errors=5)), ("sync_errors outside [0, 4]", dict(sync_errors=-1)),
                    ("e_stride < n_buf", dict(e_stride=n - 1)), ("s_end < s_begin", dict(s_begin=5, s_end=4)),
                    ("the window does not lie inside the row", dict(s_end=n + 1)), (reach, dict(n_row=100000, s_end=n - 3234)),
                    (reach, dict(buf_index0=50, n_row=n + 50, s_begin=3168, s_end=3169)), ("max_syncs < 0", dict(max_syncs=-1)),
                    ("a misaligned pointer", dict(env=d_e.data_ptr() + 2)), ("null buffer", dict(count=None))):
        kw = dict(kw)
        args = dict(env=kw.pop("env", d_e), n_rows=kw.pop("n_rows", 1), max_syncs=kw.pop("max_syncs", 4), count=kw.pop("count", d_count))
        with pytest.raises(PssError, match=re.escape("pss_apt_syncs: " + why)):
            e.apt_syncs(args["env"], args["n_rows"], n, d_row, d_pos, d_meta, d_score, args["count"], args["max_syncs"], **kw)
    e.sync()
    assert int(d_count.cpu()[0]) == -7 and bool((d_pos == -7).all()) and bool((d_row == -7).all()) and bool((d_score == -7.0).all())
    e.apt_syncs(d_e, 1, n, d_row, d_pos, d_meta, d_score, d_count, 4)      # and the same buffers are taken as they are
    e.sync()
    assert int(d_count.cpu()[0]) == 1 and int(d_pos.cpu()[0]) == 4000
    # ---- lines
    d_lr, d_lp = dev(np.zeros(2, np.int32)), dev(np.zeros(2, np.int64))
    d_words = torch.full((2, 2080), -7.0, dtype=torch.float32, device="cuda")
    for why, kw in (("n_rows outside [1, 2^20]", dict(n_rows=0)), ("e_stride < n_row", dict(e_stride=n - 1)), ("n_lines outside [0, 2^24]", dict(n_lines=-1)),
                    ("words_stride < 2080", dict(words_stride=2079)), ("null buffer", dict(lp=None)), ("a misaligned pointer", dict(lp=d_lp.data_ptr() + 4))):
        kw = dict(kw)
        with pytest.raises(PssError, match=re.escape("pss_apt_lines: " + why)):
            e.apt_lines(d_e, kw.pop("n_rows", 1), n, d_lr, kw.pop("lp", d_lp), kw.pop("n_lines", 2), d_words, **kw)
    e.sync()
    assert bool((d_words == -7.0).all())
    e.apt_lines(d_e, 1, n, d_lr, d_lp, 2, d_words)
    e.sync()
    assert same_bytes(d_words.cpu().numpy(), Engine.h_apt_lines(env, np.zeros(2, np.int32), np.zeros(2, np.int64)))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def capture(fs, up, down, offset_hz, seed):
    """The smooth case's pass at 62 400 S/s, brought to fs = 62 400 up / down and moved to offset_hz, with a little noise -> complex64."""
    from scipy.signal import resample_poly
    seed_, n_lines, start, _, _, _, image = A.CASES["smooth_30db"]
    x = A.modulate(A.pass_words(n_lines, image, seed_), start, 0.0, 0.0, 60.0, seed).astype(np.complex128)
    y = resample_poly(x, up, down)
    t = np.arange(len(y)) / fs
    rng = np.random.default_rng(seed)
    y = y * np.exp(2j * np.pi * offset_hz * t) + 0.02 * (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y)))
    return y.astype(np.complex64)


def test_rows_on_the_device_are_the_twin_route(e):
    """apt_rows against h_apt_rows: three rows with carriers at 0, +3 and -4 kHz, and rows too short for the carrier step."""
    rows = np.stack([A.case_row(name)[:95000] for name in sorted(A.CASES)])
    for kw in ({}, dict(tune=False), dict(sync_errors=4)):
        got, want = F.apt_rows(rows, **kw), F.h_apt_rows(rows, **kw)
        for g, w, name in zip(got, want, sorted(A.CASES)):
            assert g["offset_hz"] == w["offset_hz"] and g["syncs"] == w["syncs"], (name, kw)
            for key in ("words", "image", "pos", "found"):
                assert same_bytes(g[key], w[key]), (name, kw, key)
            if kw.get("tune", True):
                assert abs(g["offset_hz"] - A.CASES[name][3]) < 50.0
    got, want = F.apt_rows(rows[:, :2048]), F.h_apt_rows(rows[:, :2048])
    assert all(g["offset_hz"] == 0.0 == w["offset_hz"] and same_bytes(g["words"], w["words"]) for g, w in zip(got, want))


@pytest.mark.parametrize("fs,up,down,plan,mistuned", [(249600.0, 4, 1, (4, 1, 1), 0.0), (240000.0, 50, 13, (3, 39, 50), 2500.0)])
def test_recording_end_to_end(e, fs, up, down, plan, mistuned):
    assert Engine.apt_plan(fs) == plan
    center, chan = 137.6e6, 137.62e6
    x = capture(fs, up, down, chan - center, 9)
    chan -= mistuned                                                 # the caller's frequency is off: the carrier lands at +mistuned Hz
    out = F.apt_recording(x, fs, center, (chan,))
    assert out["fs"] == 12480 and len(out["rows"]) == 1
    got = out["rows"][0]
    # the twin route: pss_h_ddc, pss_h_resample, the three host twins
    decim = plan[0]
    taps = np.empty(20 * decim + 1, np.float64)
    assert e.lib.pss_design_firwin(len(taps), 40000.0 / fs, taps.ctypes.data) == 0
    bb = Engine.h_ddc(x, [Engine.ddc_word(chan - center, fs)[0]], decim, taps=taps)
    if plan[1:] != (1, 1):
        bb = Engine.h_resample(bb, plan[1], plan[2])
    want = F.h_apt_rows(bb)[0]
    assert same_bytes(got["image"], want["image"]) and same_bytes(got["words"], want["words"]) and same_bytes(got["pos"], want["pos"])
    assert got["syncs"] == want["syncs"] and same_bytes(got["found"], want["found"]) and got["offset_hz"] == want["offset_hz"]
    assert abs(got["offset_hz"] - mistuned) < 50.0
    sent = A.case_starts("smooth_30db")
    assert got["found"].all() and len(got["pos"]) == 3 and np.all(np.abs(got["pos"] - sent) <= 3)
    a = slice(A.IMAGE_A, A.IMAGE_A + 909)
    assert np.corrcoef(got["words"][:, a].ravel(), A.case_words("smooth_30db")[:, a].ravel())[0, 1] > 0.99
    again = F.apt_recording(x, fs, center, (chan,), chunk_samples=77777)["rows"][0]
    assert same_bytes(again["image"], got["image"]) and same_bytes(again["words"], got["words"]) and again["syncs"] == got["syncs"]

"""The arrays of tests/test_gpu_flex.py, each case a function of `check(y, h, **kw)`: the GPU file hands in a check that holds the device to
the host twin on every byte and returns the twin's result, tests/test_flex_shapes.py one that holds the twin to the NumPy statement of
tests/flex_cases.py (numpy=False where the statement would take too long: the case then only restates its expectations).  The result is
Engine.h_flex_frames': (words, fix, fiw, row, pos, meta, score, count)."""
import numpy as np

import flex_cases as F
from flex_caps import DETECT_GRID_CAP, GROUP_PASS, LANE_PASS, SCAN_STEP, TILE

W, FX, FIW, ROW, POS, META, SCORE, COUNT = range(8)


def sent_words(mode, per_phase=None):
    """uint32 [4][88]: what a clean frame of F.MESSAGES reads back as."""
    w = F.frame_words(mode, F.MESSAGES if per_phase is None else per_phase)
    return np.array([w.get(p, [0] * 88) for p in range(4)], np.uint32)


def every_mode_both_polarities_and_the_rows_end(check, h):
    for mode in range(5):
        n = 100 + F.FRAME_H * h
        for inverted in (False, True):
            y = F.frame_row(mode, h, 100, n, hold=h, inverted=inverted)       # it ends exactly with the row
            r = check(y, h, sync_errors=0)
            assert r[POS].tolist() == [100] and np.array_equal(r[W][0], sent_words(mode)) and not r[FX].any(), (mode, inverted)
            assert r[META][0].tolist() == [int(inverted) << 8 | mode << 12, 0] and r[SCORE][0] == 2.0
            assert r[FIW][0] == F.word(F.fiw_data(3, 77))
            assert check(y[:-1], h, sync_errors=0)[COUNT] == 0                # one sample shorter
    if h <= 12:
        noise = np.random.default_rng(h).standard_normal(2 * TILE + F.FRAME_H * h).astype(np.float32)
        check(noise, h, numpy=h <= 2)
        mixed = noise + F.frame_row(3, h, TILE + 5, len(noise), hold=h, amp=8.0)
        pos = check(mixed, h, numpy=h <= 2, max_bad=352)[POS].tolist()
        assert len(pos) == 1 and TILE + 5 <= pos[0] < TILE + 5 + h               # the noise decides among the h alignments


def tile_boundaries(check, h):
    """Sync codes on both sides of a tile boundary and across it; the FIW (160 h .. 223 h) and the first data symbol (304 h) straddling one."""
    for mode, s in ((0, TILE - 1), (1, TILE), (2, TILE + 1), (3, TILE - 64 * h), (0, TILE - 126 * h - 1), (1, TILE - 126 * h), (4, 2 * TILE - 190 * h),
                    (1, 2 * TILE - 304 * h - 1), (3, TILE - 304 * h), (2, 2 * TILE - 305 * h)):
        if s < 0:
            continue
        y = F.frame_row(mode, h, s, s + F.FRAME_H * h + 50)
        r = check(y, h, numpy=h <= 2)
        assert r[POS].tolist() == [s] and np.array_equal(r[W][0], sent_words(mode)), (h, mode, s)


def one_tile_past_the_detect_grid_cap(check):
    n = TILE * DETECT_GRID_CAP + 13000
    starts = [200, TILE * (DETECT_GRID_CAP - 1) + 7, TILE * DETECT_GRID_CAP + 2]   # the last two overlap: one on the odd samples, one on the even
    y = sum(F.frame_row(k, 2, s, n) for k, s in enumerate(starts))
    r = check(y, 2, numpy=False)
    assert r[POS].tolist() == starts and (r[META][:, 0] >> 12).tolist() == [0, 1, 2]


def stub_train(check):
    """Sync + FIW stubs back to back at h = 2, every level held both samples: two survivors a stub, the earlier stays; with max_bad = 352
    each is a frame.  More survivors than one pass of k_flex_head and k_flex_keep (8192) and of k_flex_walk and k_flex_compact (2048) take,
    more than one step of the scan; a count above max_frames, max_frames = 0, and a rank cut inside the second pass of the workgroup
    kernels."""
    n_stubs = LANE_PASS // 2 + 50
    y, starts = F.stub_train(n_stubs, h=2)
    small = F.stub_train(12, h=2)
    stats = {}
    ref = F.numpy_frames(small[0], 2, max_bad=352, stats=stats)
    assert ref[POS].tolist() == small[1] and stats["survivors"] == 2 * len(small[1])
    assert 2 * n_stubs > LANE_PASS and n_stubs > GROUP_PASS and n_stubs > SCAN_STEP
    full = check(y, 2, max_bad=352, max_frames=n_stubs + 10, numpy=False)
    assert full[COUNT] == n_stubs and full[POS].tolist() == starts
    assert ((full[FIW] >> 8) & 127).tolist() == [k & 127 for k in range(n_stubs)]
    for max_frames in (GROUP_PASS // 2 + 9, GROUP_PASS // 2 + 10, 100, 0):
        cut = check(y, 2, max_bad=352, max_frames=max_frames, numpy=False)
        assert cut[COUNT] == n_stubs and cut[POS].tolist() == starts[:max_frames]


def sync_errors_boundaries(check):
    h = 2
    n = 50 + F.FRAME_H * h + 20

    def run(sync_word, mode=0, **kw):
        return check(F.frame_row(mode, h, 50, n, sync_word=sync_word), h, **kw)
    code = F.MODES[0][0]
    clean = code << 48 | F.MARKER << 16 | (~code & 0xFFFF)
    flips_m = [1 << 20, 1 << 33, 1 << 47, 1 << 16]          # marker bits
    for se in range(4):
        hurt = clean
        for f in flips_m[:se]:
            hurt ^= f
        assert run(hurt, sync_errors=se)[META][:, 0].tolist() == [se]
        assert run(hurt ^ 1 << 25, sync_errors=se)[COUNT] == 0
    # the outer code: flips in C alone count against A ^ ~C and not against the mode
    for se in range(4):
        hurt = clean
        for k in range(se):
            hurt ^= 1 << k
        assert run(hurt, sync_errors=se)[META][:, 0].tolist() == [se]
        assert run(hurt ^ 1 << 9, sync_errors=se)[COUNT] == 0
    # the mode code: the same flips in A and in C leave A ^ ~C alone
    for se in range(4):
        hurt = clean
        for k in range(se):
            hurt ^= (1 << 48 + k) | (1 << k)
        assert run(hurt, sync_errors=se)[META][:, 0].tolist() == [se | 0 << 12]
        assert run(hurt ^ (1 << 60 | 1 << 12), sync_errors=se)[COUNT] == 0


def fix_fiw_and_max_bad_boundaries(check):
    h = 1
    n = 50 + F.FRAME_H * h + 20
    good = F.word(F.fiw_data(3, 77))

    def run(mode=1, **kw):
        fr = {k: kw.pop(k) for k in ("fiw", "per_phase") if k in kw}
        flips = kw.pop("flips", ())
        y = F.frame_row(mode, h, 50, n, **fr)
        for slot in flips:                                     # a two-level slot of the row reads the other way
            y[50 + slot * h] = -y[50 + slot * h]
        return check(y, h, **kw)
    # the FIW: 1, 2, 3 wrong bits against fix; the fixed bits count towards the record's errors
    for wrong in (1, 2, 3):
        hurt = good ^ [1 << 3, 1 << 3 | 1 << 17, 1 << 3 | 1 << 17 | 1 << 29][wrong - 1]
        for fix in (0, 1, 2):
            r = run(fiw=hurt, fix=fix)
            if wrong <= fix:
                assert r[COUNT] == 1 and r[FIW][0] == good and r[META][0, 0] == 1 << 12 | wrong << 16
            else:
                assert r[COUNT] == 0 or r[FIW][0] != good
    # the FIW's sum: a valid word whose nibbles do not add up
    assert run(fiw=F.word(F.fiw_data(3, 77) ^ 1))[COUNT] == 0
    assert run(fiw=F.word(F.fiw_data(15, 127)))[COUNT] == 1
    # a phase word: mode 0, symbol i of stream 0 is bit (i & 255) >> 3 of word 8 (i >> 8) + (i & 7); its slots are 304 + 2 i and + 1
    sym = lambda word, bit: (word >> 3) * 256 + bit * 8 + (word & 7)
    for wrong in (1, 2, 3):
        flips = [304 + 2 * sym(13, b) + u for b in (4, 19, 27)[:wrong] for u in (0, 1)]
        for fix in (0, 1, 2):
            r = run(mode=0, flips=flips, fix=fix, max_bad=1)
            if wrong <= fix:
                assert r[FX][0, 0, 13] == wrong and r[W][0, 0, 13] == sent_words(0)[0, 13] and r[META][0, 1] == wrong << 16
            else:
                assert r[FX][0, 0, 13] == 255 and r[W][0, 0, 13] == 0 and r[META][0, 1] == 1
            assert run(mode=0, flips=flips, fix=fix, max_bad=0)[COUNT] == (1 if wrong <= fix else 0)
    # n_bad at max_bad and one either side: five wrong bits in a row in `bad` words of every active phase
    for mode, bad in ((0, 1), (0, 3), (3, 88)):
        per = len(F.active(mode))
        flips = []
        for word in range(bad):
            for b in range(5):
                i = sym(word, b)
                flips += [304 + 2 * i, 304 + 2 * i + 1]        # 3200 baud: the symbols 2 i and 2 i + 1, phases A / B and C / D
        y = F.frame_row(mode, h, 50, n)
        for slot in flips:
            v = y[50 + slot * h]
            y[50 + slot * h] = -v if abs(v) > 0.5 else -3 * v   # outer <-> outer, inner -> the far outer level: bit_a and bit_b both change
        r = check(y, h, max_bad=352)
        n_bad = int(r[META][0, 1] & 0xFFFF)
        assert r[COUNT] == 1 and n_bad >= bad and n_bad == int((r[FX][0] == 255).sum()) and n_bad <= bad * per
        assert check(y, h, max_bad=n_bad)[COUNT] == 1 and check(y, h, max_bad=n_bad - 1)[COUNT] == 0
        if n_bad < 352:
            assert check(y, h, max_bad=n_bad + 1)[COUNT] == 1
    # random levels behind the sync of a four-phase frame: most of the 352 words are bad
    y = F.frame_row(3, h, 50, n)
    y[50 + 304 * h:50 + F.FRAME_H * h] = np.random.default_rng(9).choice(np.array([-1, -1 / 3, 1 / 3, 1], np.float32), 5632 * h)
    r = check(y, h, max_bad=352)
    n_bad = int(r[META][0, 1] & 0xFFFF)
    assert r[COUNT] == 1 and n_bad > 176 and check(y, h, max_bad=n_bad)[COUNT] == 1 and check(y, h, max_bad=n_bad - 1)[COUNT] == 0


def four_level_thresholds(check):
    """amp 1 on an offset of 0.25: at 1600 baud c = 0.5 and a = 2 exactly; mode 3 halves them.  A data symbol exactly on a threshold and one
    ulp either side; its words have one bit to fix where the symbol reads differently from what was sent."""
    f32 = np.float32
    for mode, h in ((1, 2), (3, 2), (3, 1)):
        fast = mode == 3
        n = 30 + F.FRAME_H * h + 10
        base = F.frame_row(mode, h, 30, n, base=0.0) + f32(0.25) * (F.direct_y(n, [(np.ones(F.FRAME_H), 30)], h) != 0)
        base = base.astype(f32)
        centre = f32(0.25) if fast else f32(0.5)
        T = F.TWO_THIRDS * (f32(1.0) if fast else f32(2.0))
        lo, hi = f32(centre - T), f32(centre + T)
        words = sent_words(mode)
        i = 700                                                  # stream 0: word 8 * 2 + 4, bit (700 & 255) >> 3
        at, bit = 8 * (i >> 8) + (i & 7), (i & 255) >> 3
        sent = (int(words[0, at] >> bit) & 1, int(words[1, at] >> bit) & 1)
        t = 30 + F.DATA_H * h + 2 * h * i
        for thr, below, above in ((lo, (0, 0), (0, 1)), (centre, (0, 1), (1, 1)), (hi, (1, 1), (1, 0))):
            for val, want in ((thr, below), (np.nextafter(thr, f32(-np.inf)), below), (np.nextafter(thr, f32(np.inf)), above)):
                y = base.copy()
                y[t] = val
                if not fast:
                    y[t + h] = 0.0
                r = check(y, h)
                assert r[COUNT] == 1 and r[SCORE][0] == 2.0
                assert (int(r[FX][0, 0, at]), int(r[FX][0, 1, at])) == (int(want[0] != sent[0]), int(want[1] != sent[1])), (mode, h, thr, val, want, sent)


def equal_scores_and_neighbours(check):
    h = 12
    s = TILE - 5                                                  # the alignments lie on both sides of a tile boundary
    y = F.frame_row(0, h, s, s + F.FRAME_H * h + 50, hold=h)
    assert check(y, h, numpy=False)[POS].tolist() == [s]          # h equal starts: the earliest stays
    for k in (1, h - 1):
        assert check(y, h, numpy=False, s_begin=s + k)[COUNT] == 0    # the earliest lies outside the window and still drops the others
    z = y.copy()
    z[s + 9 + 2 * h * np.arange(64)] *= 1.5                        # a larger mean distance at one alignment
    z[s + 9 + h + 2 * h * np.arange(64)] *= 1.5
    assert check(z, h, numpy=False)[POS].tolist() == [s + 9]
    assert check(z, h, numpy=False, s_begin=s, s_end=s + 9)[COUNT] == 0   # the stronger neighbour outside the window drops those inside


def rows_do_not_run_into_each_other(check):
    h = 1
    n = 9000
    flat = F.frame_row(0, h, n - 3000, 2 * n)
    assert check(flat, h)[POS].tolist() == [n - 3000]
    assert check(flat.reshape(2, n), h)[COUNT] == 0
    assert check(flat.reshape(2, n), h, gap=0)[COUNT] == 0          # the rows back to back in memory
    rows5 = np.stack([F.frame_row(k % 5, h, 60 + 7 * k, 20000, inverted=bool(k & 1)) + F.frame_row((k + 2) % 5, h, 10000 - 11 * k, 20000) for k in range(5)])
    r = check(rows5, h)
    assert r[ROW].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and r[COUNT] == 10


def windows_with_exactly_their_reach(check, same_bytes):
    h = 2
    n = 3 * TILE + F.FRAME_H * h + 24
    # frames are longer than a tile, so they overlap: the second lies on the odd samples (its strobes never meet the first's), the third is
    # four times as strong as the first, whose data it runs over
    y = np.stack([F.frame_row(1, h, 200, n) + F.frame_row(0, h, TILE - 1, n) + F.frame_row(2, h, 2 * TILE + 1000, n, amp=4.0),
                  F.frame_row(3, h, 900, n, hold=2, inverted=True)])
    whole = check(y, h, max_bad=352)
    assert whole[COUNT] >= 4 and {200, TILE - 1, 2 * TILE + 1000, 900} <= set(whole[POS].tolist())
    for cuts in ([100, 150, 203, TILE - 1, TILE, TILE + 10], [TILE + 7, 2 * TILE + 7 + 9], [1]):
        edges = [0] + cuts + [n]
        parts = []
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = F.reach(s0, s1, n, h)
            parts.append(check(y[:, lo:hi], h, max_bad=352, buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
        order = np.lexsort((np.concatenate([q[POS] for q in parts]), np.concatenate([q[ROW] for q in parts])))
        for i in range(7):
            assert same_bytes(np.concatenate([q[i] for q in parts])[order], whole[i]), (cuts, i)


def non_finite_samples(check):
    h = 2
    n = 50 + F.FRAME_H * h + 20
    y = F.frame_row(3, h, 50, n)
    for at, v in ((50 + 2 * h * 5, np.nan), (50 + 2 * h * 5 + h, np.inf), (50 + 2 * h * 63, -np.inf), (50 + 2 * h * 90, np.nan), (50 + 2 * h * 100 + h, np.inf),
                  (50 + 304 * h + 77 * h, np.nan), (50 + 304 * h + 1000 * h, np.inf), (50 + 304 * h + 5631 * h, -np.inf), (3, np.nan)):
        z = y.copy()
        z[at] = v
        r = check(z, h, max_bad=352)
        assert r[COUNT] == (0 if at < 50 + 128 * h and at >= 50 else 1), (at, v)
    check(np.full(3 * F.FRAME_H, np.nan, np.float32), h)
    check(np.zeros(10, np.float32), h)
    check(np.zeros(F.FRAME_H * h - 1, np.float32), h)
    check(np.zeros(F.FRAME_H * h, np.float32), h)

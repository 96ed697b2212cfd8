"""The POCSAG kernels (k_pocsag_detect, pss_starts.h's k_starts_scan and k_starts_gather, k_pocsag_walk, k_pocsag_keep, k_pocsag_emit) against
pss_h_pocsag_batches on every byte of every output, and formats.pocsag_recording end to end.  Buffers lie between NaNs, rows are strided
with NaNs in the gaps, and a sentinel sits behind max_batches.  The shapes are the smallest at which each path is taken: every rate from 2 to
128 samples a bit, sync words on both sides of a tile boundary and across it, one tile past the detect grid cap, more survivors in a tile
than a wavefront holds and more than one pass of each list kernel takes, more accepted batches than one step of the scan, a count above
max_batches, equal scores, rows that must not run into each other, both polarities, every fix / sync_errors / max_bad boundary, windows
with exactly their reach; 4097 one-tile rows (the counts' scan carries, the gather's grid walks twice, detect workgroups alternate tiles
with and without survivors) and a rank cut past one pass of the wavefront kernels (tests/test_pocsag_shapes.py runs the same arrays on
the CPU).  The caps and tile sizes come from tests/pocsag_caps.py, where tests/test_pocsag_caps.py and, for the start list,
tests/test_launch_caps.py pin them to the source lines."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pocsag_cases as P
from bytes_util import same_bytes
from gpu_util import dev
from pocsag_caps import DETECT_GRID_CAP, GATHER_GRID_CAP, LANE_PASS, SCAN_STEP, TILE, WAVE, WAVE_PASS   # pinned by tests/test_pocsag_caps.py
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
WHAT = ("cw", "fix", "row", "pos", "meta", "score")
assert P.TILE == TILE


@pytest.fixture(scope="module")
def e():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    eng = Engine(0)
    yield eng
    eng.close()


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


def on_device(e, y, spb, sync_errors=2, fix=2, max_bad=0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_batches=None, gap=3):
    """h_pocsag_batches' result from the device."""
    y = np.asarray(y, np.float32)
    rows = y[None, :] if y.ndim == 1 else y
    r, n = rows.shape
    n_row = buf_index0 + n if n_row is None else n_row
    s_end = n_row if s_end is None else s_end
    d_y, off, stride = strided(rows, gap)
    mb = 256 if max_batches is None else max_batches
    room = mb + 3
    d_cw = torch.full((room, 16), -7, dtype=torch.int32, device="cuda")
    d_fix = torch.full((room, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    d_row = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_pos = torch.full((room,), -7, dtype=torch.int64, device="cuda")
    d_meta = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_score = torch.full((room,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    e.pocsag_batches(d_y.data_ptr() + 4 * off, r, n, spb, d_cw, d_fix, d_row, d_pos, d_meta, d_score, d_count, mb, sync_errors=sync_errors, fix=fix,
                     max_bad=max_bad, y_stride=stride, buf_index0=buf_index0, n_row=n_row, s_begin=s_begin, s_end=s_end)
    e.sync()
    cw, fx, rw, pos, meta, score, count = (t.cpu().numpy() for t in (d_cw, d_fix, d_row, d_pos, d_meta, d_score, d_count))
    assert count[1] == -7
    k = min(int(count[0]), mb)
    assert np.all(cw[k:] == -7) and np.all(fx[k:] == SENTINEL) and np.all(rw[k:] == -7) and np.all(pos[k:] == -7) and np.all(meta[k:] == -7)
    assert np.all(score[k:] == -7.0)
    return cw[:k].view(np.uint32), fx[:k], rw[:k], pos[:k], meta[:k].view(np.uint32), score[:k], int(count[0])


def check(e, y, spb, max_batches=256, gap=3, **kw):
    """Device == twin on every byte -> the twin's result."""
    want = Engine.h_pocsag_batches(y, spb, max_batches=max_batches, **kw)
    got = on_device(e, y, spb, max_batches=max_batches, gap=gap, **kw)
    for g, w, what in zip(got[:6], want[:6], WHAT):
        assert same_bytes(g, w), (what, g, w)
    assert got[6] == want[6]
    return want


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_fixture_rows(e, name):
    baud, _, inverted, messages = P.CASES[name]
    r = check(e, P.case_row(name), P.SPB[baud])
    assert r[6] == P.case_batches(name)[0] and P.reported(F.pocsag_messages(F.pocsag_records(*r[:6]), P.SPB[baud])) == P.expected(messages, baud)
    for spb in (16, 32, 75):
        if spb != P.SPB[baud]:
            assert check(e, P.case_row(name), spb)[6] == 0


@pytest.mark.parametrize("spb", [2, 16, 32, 75, 128])
def test_every_rate_both_polarities_and_the_rows_end(e, spb):
    n = 100 + P.LAST_K * spb + 1
    for inverted in (False, True):
        y = P.batch_row(spb, 100, n, inverted=inverted, hold=spb)            # it ends exactly with the row: one start exists of the spb
        r = check(e, y, spb)
        assert r[3].tolist() == [100] and r[0][0].tolist() == P.WORDS and r[4][0] == int(inverted) << 8
        assert check(e, y[:-1], spb)[6] == 0                                  # one sample shorter
        y = P.batch_row(spb, 100, n + 2 * spb, inverted=inverted, hold=spb)  # all spb alignments survive the sync test; the earliest stays
        stats = {}
        assert P.numpy_batches(y, spb, stats=stats)[3].tolist() == [100] and stats["survivors"] == spb
        assert check(e, y, spb)[3].tolist() == [100]
    noise = np.random.default_rng(spb).standard_normal(3 * TILE + 544 * spb).astype(np.float32)
    check(e, noise, spb)
    mixed = noise + P.batch_row(spb, TILE + 5, len(noise), hold=spb, amp=4.0)
    assert check(e, mixed, spb)[6] == 1


def test_sync_words_on_both_sides_of_a_tile_boundary_and_across_it(e):
    for spb in (2, 16, 128):
        for s in (TILE - 1, TILE, TILE + 1, TILE - 15 * spb, 2 * TILE - 31 * spb - 1, TILE - 31 * spb, TILE - 31 * spb + 1):
            y = P.batch_row(spb, s, s + 544 * spb + 50)
            assert check(e, y, spb)[3].tolist() == [s], (spb, s)


sync_train = P.sync_train       # (the CPU tests of tests/test_pocsag_shapes.py use the same rows)


def test_more_survivors_in_a_tile_than_a_wavefront_holds_and_more_than_a_wave_pass(e):
    y, starts = sync_train(WAVE_PASS // 2 + 40)
    assert 2 * len(starts) > WAVE_PASS and 2 * len(starts) / (len(y) / TILE) > WAVE
    stats = {}
    ref = P.numpy_batches(y[:64 * 40], 2, stats=stats)
    assert stats["survivors"] == 2 * ref[6] == 2 * 23
    full = check(e, y, 2, max_batches=len(starts) + 10)
    assert full[6] == len(starts) > SCAN_STEP and full[3].tolist() == starts and not full[1].any()
    cut = check(e, y, 2, max_batches=100)
    assert cut[6] == len(starts) and len(cut[3]) == 100
    assert check(e, y, 2, max_batches=0)[6] == len(starts)
    one = check(e, sync_train(200, hold=1)[0], 2)                 # one survivor per word: nothing to drop
    assert one[6] == 200 - 16


def test_more_survivors_than_one_pass_of_the_lane_kernel_and_one_tile_past_the_detect_grid_cap(e):
    y, starts = sync_train(LANE_PASS // 2 + 60)
    assert 2 * len(starts) > LANE_PASS and len(y) > TILE * (DETECT_GRID_CAP + 1)
    r = check(e, y, 2, max_batches=50)
    assert r[6] == len(starts) and r[3].tolist() == starts[:50]


def test_the_rank_cut_falls_past_one_pass_of_the_wave_kernels(e):
    """The sync train of the test above: survivors come two a kept start, so record k is survivor 2 k, and max_batches just past
    WAVE_PASS / 2 cuts in the second pass of k_pocsag_emit's loop."""
    y, starts = sync_train(WAVE_PASS // 2 + 40)
    for max_batches in (WAVE_PASS // 2 + 10, WAVE_PASS // 2 + 11, WAVE_PASS // 2 + 9):
        assert 2 * (max_batches - 1) > WAVE_PASS and 2 * max_batches > WAVE_PASS and max_batches < len(starts)
        cut = check(e, y, 2, max_batches=max_batches)
        assert cut[6] == len(starts) and cut[3].tolist() == starts[:max_batches]


@pytest.mark.parametrize("dense", [False, True])
def test_thousands_of_one_tile_rows_the_counts_carry_and_the_gathers_second_pass(e, dense):
    """SCAN_STEP + 1 rows of 1147 samples at 2 samples a bit: tpr == 1, one tile past a step of the counts' scan and two passes of the
    gather's grid.  Plain: the rows of every other round of the detect grid carry one batch, so every workgroup meets tiles with, without,
    with, without survivors and workgroup 0 a fifth with them; the carry into the last tile is 2048.  dense: two survivors in every tile:
    the carry is 8192."""
    R = SCAN_STEP + 1
    assert R > GATHER_GRID_CAP and R > 4 * DETECT_GRID_CAP
    y = P.short_rows(R, DETECT_GRID_CAP, dense)
    rows = list(range(R)) if dense else P.carrying(R, DETECT_GRID_CAP)
    full = check(e, y, P.SHORT_SPB, max_batches=R + 10)
    assert full[6] == len(rows) == (R if dense else 2 * DETECT_GRID_CAP + 1)
    assert full[2].tolist() == rows and full[3].tolist() == [P.short_start(r) for r in rows]
    assert all(w.tolist() == P.WORDS for w in full[0][[0, len(rows) // 2, -1]]) and not full[1].any()
    assert check(e, y, P.SHORT_SPB, max_batches=0)[6] == len(rows)
    cut = check(e, y, P.SHORT_SPB, max_batches=len(rows) // 2 + 3)
    assert cut[6] == len(rows) and cut[2].tolist() == rows[:len(rows) // 2 + 3]


def test_one_tile_past_the_detect_grid_cap(e):
    n = TILE * DETECT_GRID_CAP + 3000
    starts = [200, TILE * (DETECT_GRID_CAP - 1) + 7, TILE * DETECT_GRID_CAP + 1]
    y = sum(P.batch_row(2, s, n) for s in starts)
    assert check(e, y, 2)[3].tolist() == starts


def test_equal_scores_keep_the_earlier_start_and_a_stronger_one_wins(e):
    spb = 16
    s = TILE - 5                                                  # the alignments lie on both sides of a tile boundary
    y = P.batch_row(spb, s, s + 544 * spb + 50, hold=spb)
    assert check(e, y, spb)[3].tolist() == [s]
    for k in range(1, spb):
        assert check(e, y, spb, s_begin=s + k)[6] == 0            # the earliest lies outside the window and still drops the others
    z = y.copy()
    z[s + 9 + spb * np.arange(32)] *= 1.5
    assert check(e, z, spb)[3].tolist() == [s + 9]


def test_rows_do_not_run_into_each_other(e):
    spb = 16
    n = 6000
    flat = P.batch_row(spb, n - 3000, 2 * n)
    assert check(e, flat, spb)[3].tolist() == [n - 3000]
    assert check(e, flat.reshape(2, n), spb)[6] == 0
    assert check(e, flat.reshape(2, n), spb, gap=0)[6] == 0       # the rows back to back in memory
    rows5 = np.stack([P.batch_row(spb, 60 + 7 * k, 20000, hold=1 + k, inverted=bool(k & 1)) + P.batch_row(spb, 10000 - 11 * k, 20000, words=P.WORDS[::-1])
                      for k in range(5)])
    r = check(e, rows5, spb)
    assert r[2].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and r[6] == 10


def test_fix_sync_errors_and_max_bad_boundaries(e):
    spb = 16
    n = 50 + 544 * spb + 20

    def run(flips, **kw):
        return check(e, P.batch_row(spb, 50, n, flips=flips), spb, **kw)
    # exactly sync_errors mismatches and one more
    for se in (0, 1, 2):
        flips = [3, 17, 30][:se]
        assert run(flips, sync_errors=se)[4].tolist() == [se]
        assert run(flips + [8], sync_errors=se)[6] == 0
    # 1, 2 and 3 wrong bits in data codeword 5 against fix 0 / 1 / 2
    at = 32 + 32 * 5
    for wrong in (1, 2, 3):
        flips = [at + 4, at + 19, at + 27][:wrong]
        hurt = P.WORDS[5] ^ sum(1 << (31 - (k - at)) for k in flips)
        for fix in (0, 1, 2):
            nf, cw = P.check(hurt, fix)
            assert (nf, cw) == (wrong, P.WORDS[5]) if wrong <= fix else cw != P.WORDS[5]
            r = run(flips, fix=fix, max_bad=1)
            if nf >= 0:
                assert r[1][0, 5] == nf and r[0][0, 5] == cw and r[4][0] == nf << 24
            else:
                assert r[1][0, 5] == 255 and r[0][0, 5] == 0 and r[4][0] == 1 << 16, (wrong, fix)
            assert run(flips, fix=fix, max_bad=0)[6] == (1 if nf >= 0 else 0)
    # the parity bit alone, parity + 1, parity + 2 (refused at fix 2)
    assert run([at + 31], fix=1)[1][0, 5] == 1 and run([at + 31], fix=0)[6] == 0
    assert run([at + 31, at + 2], fix=2)[1][0, 5] == 2 and run([at + 31, at + 2], fix=1)[6] == 0
    assert run([at + 31, at + 2, at + 11], fix=2)[6] == 0
    # n_bad at max_bad and one above
    burst = 0xF8000000                                             # five wrong bits in a row: uncorrectable in every word here
    assert all(P.check(w ^ burst, 2) == (-1, 0) for w in P.WORDS)
    for bad in (1, 3, 16):
        flips = [32 + 32 * j + k for j in range(bad) for k in range(5)]
        r = run(flips, max_bad=bad)
        assert r[6] == 1 and r[4][0] == bad << 16 and r[1][0].tolist() == [255] * bad + [0] * (16 - bad)
        assert run(flips, max_bad=bad - 1)[6] == 0
        if bad < 16:
            assert run(flips, max_bad=bad + 1)[6] == 1


def test_non_finite_samples(e):
    spb = 16
    n = 50 + 544 * spb + 20
    y = P.batch_row(spb, 50, n)
    for at, v in ((50 + spb * 5, np.nan), (50 + spb * 5, np.inf), (50 + spb * 31, -np.inf), (50 + spb * 100, np.nan), (50 + spb * 543, np.inf), (3, np.nan)):
        z = y.copy()
        z[at] = v
        check(e, z, spb, max_bad=16)
    check(e, np.full(9000, np.nan, np.float32), spb)
    check(e, np.zeros(10, np.float32), spb)
    check(e, np.zeros(544 * spb, np.float32), spb)


def test_windows_with_exactly_their_reach(e):
    spb = 4
    n = 3 * TILE + 544 * spb + 24
    starts = [200, TILE - 1, TILE + 2500, 2 * TILE + 1000]          # more than a batch apart
    y = np.stack([sum(P.batch_row(spb, s, n, hold=3, words=P.WORDS if k & 1 else P.WORDS[::-1]) for k, s in enumerate(starts)),
                  P.batch_row(spb, 900, n, hold=2, inverted=True)])
    whole = check(e, y, spb)
    assert whole[6] == 5
    for cuts in ([100, 150, 203, TILE - 1, TILE, TILE + 10], [TILE + 7, 2 * TILE + 7 + 9], [1]):
        edges = [0] + cuts + [n]
        parts = []
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = P.reach(s0, s1, n, spb)
            parts.append(check(e, y[:, lo:hi], spb, buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
        order = np.lexsort((np.concatenate([q[3] for q in parts]), np.concatenate([q[2] for q in parts])))
        for i in range(6):
            assert same_bytes(np.concatenate([q[i] for q in parts])[order], whole[i]), (cuts, i)


def test_a_refused_device_call_writes_nothing(e):
    from pyspecsdr_amd.engine import PssError
    spb = 16
    n = 50 + 544 * spb + 20
    d_y = dev(P.batch_row(spb, 50, n))
    d_cw = torch.full((4, 16), -7, dtype=torch.int32, device="cuda")
    d_fix = torch.full((4, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    d_row, d_meta = torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int32, device="cuda")
    d_pos, d_score = torch.full((4,), -7, dtype=torch.int64, device="cuda"), torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    reach = "the buffer does not cover the window's reach (spb - 1 starts either side, 543 spb + 1 samples forward)"
    for why, kw in (("n_rows outside [1, 2^20]", dict(n_rows=0)), ("spb outside [2, 128]", dict(spb=1)), ("spb outside [2, 128]", dict(spb=129)),
                    ("sync_errors outside [0, 2]", dict(sync_errors=3)), ("fix outside [0, 2]", dict(fix=-1)), ("max_bad outside [0, 16]", dict(max_bad=17)),
                    ("y_stride < n_buf", dict(y_stride=n - 1)), ("s_end < s_begin", dict(s_begin=5, s_end=4)),
                    ("the window does not lie inside the row", dict(s_end=n + 1)), (reach, dict(n_row=100000, s_end=900)),
                    (reach, dict(buf_index0=50, n_row=n + 50, s_begin=60, s_end=61)), ("max_batches < 0", dict(max_batches=-1)),
                    ("a misaligned pointer", dict(y=d_y.data_ptr() + 2)), ("null buffer", dict(count=None))):
        kw = dict(kw)
        args = dict(y=kw.pop("y", d_y), n_rows=kw.pop("n_rows", 1), max_batches=kw.pop("max_batches", 4), count=kw.pop("count", d_count),
                    spb=kw.pop("spb", spb))
        with pytest.raises(PssError, match=re.escape("pss_pocsag_batches: " + why)):
            e.pocsag_batches(args["y"], args["n_rows"], n, args["spb"], d_cw, d_fix, d_row, d_pos, d_meta, d_score, args["count"], args["max_batches"], **kw)
    e.sync()
    assert int(d_count.cpu()[0]) == -7 and bool((d_cw == -7).all()) and bool((d_pos == -7).all()) and bool((d_fix == SENTINEL).all())
    e.pocsag_batches(d_y, 1, n, spb, d_cw, d_fix, d_row, d_pos, d_meta, d_score, d_count, 4)      # and the same buffers are taken as they are
    e.sync()
    assert int(d_count.cpu()[0]) == 1 and int(d_pos.cpu()[0]) == 50


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
CHANNELS = ((-50e3, 1200, False, [(1234567, 3, "Hello from the first channel"), (2000, 0, "0123456789")]),
            (50e3, 2400, True, [(77001, 2, "the second channel is inverted and twice as fast"), (5, 1, None), (654321, 0, "42")]))


def capture(fs, seed):
    """Two channels at -50 and +50 kHz, 20 dB in the 38.4 kHz band -> complex64 at fs centred between them."""
    n38 = 400 + max(P.SPB[baud] * len(P.transmission_bits(messages)) for _, baud, _, messages in CHANNELS) + 1200
    n38 += -n38 % 4
    n = n38 * int(fs) // P.RATE
    assert n * P.RATE == n38 * int(fs)
    t = np.arange(n) / fs
    x = np.zeros(n, np.complex128)
    for off, baud, inverted, messages in CHANNELS:
        b = P.fsk_iq(n38, P.SPB[baud], P.transmission_bits(messages), 400, offset_hz=300.0, inverted=inverted)
        spec = np.fft.fft(b)
        wide = np.zeros(n, np.complex128)
        wide[:n38 // 2], wide[-(n38 // 2):] = spec[:n38 // 2], spec[-(n38 // 2):]
        x += np.fft.ifft(wide) * (n / n38) * np.exp(2j * np.pi * off * t)
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(10.0 ** (-20.0 / 10.0) / 2 * fs / P.RATE)
    x += sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def test_recording_end_to_end(e):
    fs = 240e3
    assert Engine.pocsag_plan(fs) == (6, 24, 25)
    x = capture(fs, 5)
    out = F.pocsag_recording(x, fs, 150.0e6, [150.0e6 + c[0] for c in CHANNELS])
    assert out["fs"] == 38400
    for row, (_, baud, inverted, messages) in enumerate(CHANNELS):
        got = [m for m in out["messages"] if m["row"] == row]
        assert P.reported(got) == P.expected(messages, baud) and all(m["baud"] == baud and not m["damaged"] for m in got), (row, got)
        assert all(b["inverted"] == inverted and b["baud"] == baud and b["n_bad"] == 0 for b in out["batches"] if b["row"] == row)
    assert len(out["messages"]) == 5 and len(out["lines"]) == 5 and len(out["batches"]) == sum(len(P.batches_of(c[3])) for c in CHANNELS)
    assert "POCSAG1200: Address: 1234567  Function: 3  Alpha:   Hello from the first channel" in out["lines"]
    again = F.pocsag_recording(x, fs, 150.0e6, [150.0e6 + c[0] for c in CHANNELS], chunk_samples=77777)
    assert again["messages"] == out["messages"] and again["batches"] == out["batches"] and again["lines"] == out["lines"]

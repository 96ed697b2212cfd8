"""The AIS kernels (k_ais_front; k_ais_detect, pss_starts.h's k_starts_scan and k_starts_gather, k_ais_walk, k_ais_keep, k_ais_emit) against pss_h_ais_front and
pss_h_ais_frames on every byte of every output, and formats.ais_recording end to end.  Buffers lie between NaNs, rows are strided with NaNs
in the gaps, and a sentinel sits behind max_frames and behind each row's window.  The shapes are the smallest at which each path is taken:
row lengths around the pulse's half-width and the front's tile, one tile past each grid cap, flags on both sides of a tile boundary, a
1024-bit frame across two of them, more survivors in a tile than a wavefront holds and more than one pass of the list kernels takes, more
accepted frames than one step of the scan, more tiles than one step of the scan, a count above max_frames, equal scores, rows that must
not run into each other, windows with exactly their reach, 4097 one-tile rows whose detect workgroups alternate tiles with and without
survivors.  The caps and tile sizes come from tests/ais_caps.py, where
tests/test_ais_caps.py and, for the start list shared with ADS-B, tests/test_launch_caps.py pin them to the source lines."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_cases as A
from ais_caps import DETECT_GRID_CAP, FRONT_GRID_CAP, FRONT_TILE, GATHER_GRID_CAP, LIST_PASS, SCAN_STEP, TILE, WAVE   # pinned to csrc/pss_ais.hip and pss_starts.h by tests/test_ais_caps.py
from bytes_util import same_bytes
from gpu_util import dev
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
WHAT = ("msg", "len", "row", "pos", "score")
GOOD = A.with_crc(A.SHIPS[0])
assert A.TILE == TILE and A.FRONT_TILE == FRONT_TILE


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


# ---- front --------------------------------------------------------------------------------------------------------------------------------
def front_on_device(e, x, pulse=None, buf_index0=0, n_row=None, i_begin=0, i_end=None, gap=3):
    x = np.asarray(x, np.complex64)
    rows = x[None, :] if x.ndim == 1 else x
    r, n = rows.shape
    n_row = buf_index0 + n if n_row is None else n_row
    i_end = n_row if i_end is None else i_end
    width = i_end - i_begin
    d_x, off, stride = strided(rows, gap)
    y_stride = width + 2
    d_y = torch.full((r * y_stride + 1,), -7.0, dtype=torch.float32, device="cuda")
    e.ais_front(d_x.data_ptr() + 8 * off, r, n, d_y, pulse=pulse, x_stride=stride, buf_index0=buf_index0, n_row=n_row, i_begin=i_begin, i_end=i_end,
                y_stride=y_stride)
    e.sync()
    y = d_y.cpu().numpy()
    assert y[-1] == -7.0
    out = y[:-1].reshape(r, y_stride)
    assert np.all(out[:, width:] == -7.0)                          # nothing behind a row's window
    return out[:, :width] if x.ndim == 2 else out[0, :width]


def check_front(e, x, gap=3, **kw):
    want = Engine.h_ais_front(x, **kw)
    got = front_on_device(e, x, gap=gap, **kw)
    assert same_bytes(got, want), (np.nonzero(got.view(np.uint32) != want.view(np.uint32)), got, want)
    return want


def noisy(n, seed, rows=None):
    rng = np.random.default_rng(seed)
    shape = (n,) if rows is None else (rows, n)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("P", [1, 11, 65])
def test_front_lengths_around_the_half_width_and_the_tile(e, P):
    g = np.array([1.0]) if P == 1 else (Engine.ais_default_pulse(2) if P == 11 else np.linspace(-1.0, 1.0, 65) ** 3 + 0.01)
    c = (P - 1) // 2
    for n in sorted({1, 2, max(c, 1), c + 1, FRONT_TILE - 1, FRONT_TILE, FRONT_TILE + 1}):
        check_front(e, noisy(n, 100 + n), pulse=g)


def test_front_rows_with_gaps_and_special_samples(e):
    x = noisy(3000, 5, rows=3)
    x[0, 10] = np.nan
    x[1, 500] = np.inf + 0j
    x[1, 2047] = complex(0.0, -np.inf)
    x[2, 100:110] = 0
    x[2, 200] = complex(-0.0, 0.0)
    x[2, 201] = complex(1.0, -0.0)
    x[2, 2999] = np.nan
    y = check_front(e, x, gap=7)
    assert np.isnan(y[0, 5:16]).all() and np.isfinite(y[0, 17:]).all()


def test_front_one_tile_past_the_grid_cap(e):
    n = FRONT_TILE * FRONT_GRID_CAP + 5
    check_front(e, noisy(n, 6), pulse=np.array([0.5, 0.25, -0.125]))
    check_front(e, noisy(FRONT_TILE * 3 + 1, 7, rows=5))            # rows x tiles, walked in pairs


def test_front_windows_with_exactly_their_halo(e):
    n = 3 * FRONT_TILE
    x = noisy(n, 8, rows=2)
    whole = Engine.h_ais_front(x)
    for i0, i1 in ((0, 1), (1, 2), (6, 7), (7, FRONT_TILE + 8), (FRONT_TILE - 1, 2 * FRONT_TILE + 1), (n - 3, n), (0, n)):
        lo, hi = max(0, i0 - 6), min(n, i1 + 5)
        got = check_front(e, x[:, lo:hi], buf_index0=lo, n_row=n, i_begin=i0, i_end=i1)
        assert same_bytes(got, whole[:, i0:i1])


# ---- frames -------------------------------------------------------------------------------------------------------------------------------
def on_device(e, y, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, gap=3):
    """h_ais_frames' result from the device."""
    y = np.asarray(y, np.float32)
    rows = y[None, :] if y.ndim == 1 else y
    r, n = rows.shape
    n_row = buf_index0 + n if n_row is None else n_row
    s_end = n_row if s_end is None else s_end
    d_y, off, stride = strided(rows, gap)
    mf = 256 if max_frames is None else max_frames
    room = mf + 3
    d_msg = torch.full((room, 128), SENTINEL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_row = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_pos = torch.full((room,), -7, dtype=torch.int64, device="cuda")
    d_score = torch.full((room,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    e.ais_frames(d_y.data_ptr() + 4 * off, r, n, d_msg, d_len, d_row, d_pos, d_score, d_count, mf, y_stride=stride, buf_index0=buf_index0, n_row=n_row,
                 s_begin=s_begin, s_end=s_end)
    e.sync()
    msg, ln, rw, pos, score, count = (t.cpu().numpy() for t in (d_msg, d_len, d_row, d_pos, d_score, d_count))
    assert count[1] == -7
    k = min(int(count[0]), mf)
    assert np.all(msg[k:] == SENTINEL) and np.all(ln[k:] == -7) and np.all(rw[k:] == -7) and np.all(pos[k:] == -7) and np.all(score[k:] == -7.0)
    return msg[:k], ln[:k], rw[:k], pos[:k], score[:k], int(count[0])


def check(e, y, max_frames=256, gap=3, **kw):
    """Device == twin on every byte -> the twin's result."""
    want = Engine.h_ais_frames(y, max_frames=max_frames, **kw)
    got = on_device(e, y, max_frames=max_frames, gap=gap, **kw)
    for g, w, what in zip(got[:5], want[:5], WHAT):
        assert same_bytes(g, w), (what, g, w)
    assert got[5] == want[5]
    return want


def frames_of(r):
    return [bytes(m[:n]) for m, n in zip(r[0], r[1])]


def row_with(bursts, n, **kw):
    return A.direct_y(n, bursts, **kw)


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_fixture_captures_front_and_frames(e, name):
    x = A.case_iq(name)
    y = check_front(e, x)
    r = check(e, y)
    assert frames_of(r) == [A.with_crc(m) for m, _, _, _ in A.CASES[name][3]]


def test_flags_on_both_sides_of_a_tile_boundary(e):
    good = A.burst_bits(GOOD)
    for s in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1):
        y = row_with([(good, s - 5 * A.TRAINING)], s + 5 * len(good) + 50)
        assert check(e, y)[3].tolist() == [s]
        assert check(e, row_with([(good, s - 5 * A.TRAINING)], s + 5 * len(good) + 50, hold=5))[3].tolist() == [s]


def test_a_1024_bit_frame_across_two_tile_boundaries(e):
    frame = A.long_frame()
    bits = A.burst_bits(frame)
    s = TILE - 100
    assert s + 5 * (len(bits) - A.TRAINING) > 2 * TILE
    last = s - 5 * A.TRAINING + 5 * (len(bits) - 1)
    r = check(e, row_with([(bits, s - 5 * A.TRAINING)], last + 1))           # it ends exactly with the row
    assert frames_of(r) == [frame] and r[3].tolist() == [s]
    assert check(e, row_with([(bits, s - 5 * A.TRAINING)], last))[5] == 0    # one sample shorter
    assert check(e, row_with([(A.burst_bits(A.with_crc(bytes(127))), 50)], 8000))[5] == 0


def test_one_tile_past_the_detect_grid_cap(e):
    good = A.burst_bits(GOOD)
    n = TILE * DETECT_GRID_CAP + 3000
    starts = [200, TILE * (DETECT_GRID_CAP - 1) + 7, TILE * DETECT_GRID_CAP + 1]
    y = row_with([(good, s - 5 * A.TRAINING) for s in starts], n)
    assert check(e, y)[3].tolist() == starts


def test_more_tiles_than_a_scan_step(e):
    good = A.burst_bits(GOOD)
    n = TILE * (SCAN_STEP + 1) + 2000
    starts = [300, TILE * SCAN_STEP - 1, TILE * SCAN_STEP + 40]
    y = row_with([(good, s - 5 * A.TRAINING) for s in starts], n)
    assert check(e, y)[3].tolist() == starts


@pytest.mark.parametrize("dense", [False, True])
def test_thousands_of_one_tile_rows_and_workgroups_that_alternate_tiles_with_and_without_survivors(e, dense):
    """SCAN_STEP + 1 rows of one short burst's length: tpr == 1, one tile past a step of the counts' scan and two passes of the gather's
    grid.  Plain: the rows of every other round of the detect grid carry the burst, so every workgroup meets tiles with, without, with,
    without survivors and workgroup 0 a fifth with them.  dense: five survivors in every tile."""
    R = SCAN_STEP + 1
    assert R > GATHER_GRID_CAP and R > 4 * DETECT_GRID_CAP and A.SHORT_N <= TILE
    y = A.short_rows(R, DETECT_GRID_CAP, dense)
    rows = list(range(R)) if dense else A.carrying(R, DETECT_GRID_CAP)
    full = check(e, y, max_frames=R + 10)
    assert full[5] == len(rows) == (R if dense else 2 * DETECT_GRID_CAP + 1)
    assert full[2].tolist() == rows and full[3].tolist() == [A.short_start(r) for r in rows]
    assert set(frames_of(full)) == {A.SHORT_FRAME}
    assert check(e, y, max_frames=0)[5] == len(rows)
    cut = check(e, y, max_frames=len(rows) // 2 + 3)
    assert cut[5] == len(rows) and cut[2].tolist() == rows[:len(rows) // 2 + 3]


def interleaved(n_per_phase, frames=None):
    """Five bursts interleaved sample by sample, one per alignment, every `period` samples: with frames=None training + flag only
    (survivors of the flag test, no frame), else alignment ph carries frames[ph] (five different ones: equal bytes a sample apart would
    leave one record of the five)."""
    head = [k & 1 for k in range(8)] + list(A.FLAG)
    per_phase = []
    for ph in range(5):
        bits = head if frames is None else head + A.stuff(A.wire_bits(frames[ph])) + list(A.FLAG) + [1, 1]
        per_phase.append(bits + ([0] if A.nrzi(bits)[-1] != 1.0 else []))       # ends on the level the next burst's training changes from
    width = max(len(b) for b in per_phase)
    per_phase = [b + [1] * (width - len(b)) for b in per_phase]
    period = 5 * width
    n = 10 + period * n_per_phase + 60
    y = np.zeros(n, np.float32)
    y[5:10] = 1.0
    starts = []
    for i in range(n_per_phase):
        for ph in range(5):
            at = 10 + ph + period * i
            y[at + 5 * np.arange(width)] = A.nrzi(per_phase[ph])
            starts.append(at + 40)
    return y, starts


def test_more_survivors_in_a_tile_than_a_wavefront_holds(e):
    y, starts = interleaved(130)
    assert len(starts) / (len(y) / TILE) > 2 * WAVE
    stats = {}
    assert A.numpy_frames(y, stats=stats)[5] == 0 and stats["survivors"] == len(starts)
    assert check(e, y)[5] == 0


def test_more_survivors_than_one_pass_of_the_list_kernels(e):
    y, starts = interleaved(LIST_PASS // 5 + 50)
    assert len(starts) > LIST_PASS
    y2 = np.concatenate([y, row_with([(A.burst_bits(GOOD), 20)], 2000)])
    r = check(e, y2)
    assert r[5] == 1 and r[3].tolist() == [len(y) + 20 + 5 * A.TRAINING]


def test_more_frames_than_a_scan_step_and_than_max_frames(e):
    frames = [A.with_crc(A.SHIPS[0][:4] + bytes([ph])) for ph in range(5)]     # 56 bits: the shortest frame
    y, starts = interleaved(SCAN_STEP // 5 + 7, frames)
    full = check(e, y, max_frames=len(starts) + 10)
    assert full[5] == len(starts) > SCAN_STEP and full[3].tolist() == sorted(starts) and frames_of(full)[:5] == frames
    cut = check(e, y, max_frames=100)
    assert cut[5] == len(starts) and len(cut[3]) == 100
    assert check(e, y, max_frames=0)[5] == len(starts)


def test_equal_scores_keep_the_earlier_start(e):
    good = A.burst_bits(GOOD)
    s = TILE - 2                                                  # the five alignments lie on both sides of a tile boundary
    y = row_with([(good, s - 5 * A.TRAINING)], s + 5 * len(good) + 50, hold=5)
    assert check(e, y)[3].tolist() == [s]
    for k in range(1, 5):
        assert check(e, y, s_begin=s + k)[5] == 0                 # the earliest lies outside the window and still drops the others
    z = y.copy()
    z[s + 3 + 5 * np.arange(-8, 8)] *= 1.5
    assert check(e, z)[3].tolist() == [s + 3]


def test_rows_do_not_run_into_each_other(e):
    good = A.burst_bits(GOOD)
    n = 60 + 5 * (len(good) - 1) - 12
    flat = row_with([(good, 60)], 2 * n)
    assert frames_of(check(e, flat)) == [GOOD]
    assert check(e, flat.reshape(2, n))[5] == 0
    assert check(e, flat.reshape(2, n), gap=0)[5] == 0             # the rows back to back in memory
    rows5 = np.stack([row_with([(good, 60 + 7 * k), (A.burst_bits(A.with_crc(A.SHIPS[1])), 3000 - 11 * k)], 5000, hold=1 + k) for k in range(5)])
    r = check(e, rows5)
    assert r[2].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and r[5] == 10


def test_windows_with_exactly_their_reach(e):
    good, other = A.burst_bits(GOOD), A.burst_bits(A.with_crc(A.SHIPS[1]))
    n = 3 * TILE
    starts = [200, TILE - 1, TILE + 2000, 2 * TILE + 100]
    y = np.stack([row_with([(good if k & 1 else other, s - 5 * A.TRAINING) for k, s in enumerate(starts)], n, hold=5),
                  row_with([(other, 900)], n, hold=2)])
    whole = check(e, y)
    assert whole[5] == 5
    for cuts in ([100, 150, 203, TILE - 1, TILE, TILE + 10], [TILE + 7, 2 * TILE + 7 + 9], [1]):
        edges = [0] + cuts + [n]
        parts = []
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = A.reach(s0, s1, n)
            parts.append(check(e, y[:, lo:hi], buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
        order = np.lexsort((np.concatenate([q[3] for q in parts]), np.concatenate([q[2] for q in parts])))
        for i in range(5):
            assert same_bytes(np.concatenate([q[i] for q in parts])[order], whole[i]), (cuts, i)


def test_non_finite_samples(e):
    y = row_with([(A.burst_bits(GOOD), 60)], 3000)
    s = A.flag_start(60)
    for at, v in ((s - 20, np.nan), (s + 10, np.nan), (s + 300, np.inf), (s - 40, -np.inf), (3, np.nan)):
        z = y.copy()
        z[at] = v
        check(e, z)
    check(e, np.full(500, np.nan, np.float32))
    check(e, np.zeros(10, np.float32))
    check(e, np.zeros(81, np.float32))


def test_a_refused_device_call_writes_nothing(e):
    from pyspecsdr_amd.engine import PssError
    n = 7000
    d_y = dev(row_with([(A.burst_bits(GOOD), 60)], n))
    d_msg = torch.full((4, 128), SENTINEL, dtype=torch.uint8, device="cuda")
    d_len, d_row = torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int32, device="cuda")
    d_pos, d_score = torch.full((4,), -7, dtype=torch.int64, device="cuda"), torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    reach = "the buffer does not cover the window's reach (4 starts either side, 45 samples back, 6221 samples forward)"
    for why, kw in (("n_rows outside [1, 2^20]", dict(n_rows=0)), ("y_stride < n_buf", dict(y_stride=n - 1)), ("s_end < s_begin", dict(s_begin=5, s_end=4)),
                    ("the window does not lie inside the row", dict(s_end=n + 1)), (reach, dict(n_row=100000, s_end=900)),
                    (reach, dict(buf_index0=50, n_row=n + 50, s_begin=98, s_end=99)), ("max_frames < 0", dict(max_frames=-1)),
                    ("a misaligned pointer", dict(y=d_y.data_ptr() + 2)), ("null buffer", dict(count=None))):
        kw = dict(kw)
        args = dict(y=kw.pop("y", d_y), n_rows=kw.pop("n_rows", 1), max_frames=kw.pop("max_frames", 4), count=kw.pop("count", d_count))
        with pytest.raises(PssError, match=re.escape("pss_ais_frames: " + why)):
            e.ais_frames(args["y"], args["n_rows"], n, d_msg, d_len, d_row, d_pos, d_score, args["count"], args["max_frames"], **kw)
    d_x = dev(noisy(100, 3))
    d_out = torch.full((100,), -7.0, dtype=torch.float32, device="cuda")
    halo = r"the buffer does not cover the window's halo \(\(P - 1\) / 2 \+ 1 samples in front, \(P - 1\) / 2 behind\)"
    for why, kw in ((r"n_pulse must be odd and in \[1, 65\]", dict(pulse=np.ones(10))), ("a pulse tap that is not finite", dict(pulse=np.array([1.0, np.nan, 1.0]))),
                    (halo, dict(n_row=200, i_end=96)), ("the window does not lie inside the row", dict(i_end=101)), ("x_stride < n_buf", dict(x_stride=99))):
        with pytest.raises(PssError, match="pss_ais_front: " + why):
            e.ais_front(d_x, 1, 100, d_out, **kw)
    e.sync()
    assert int(d_count.cpu()[0]) == -7 and bool((d_msg == SENTINEL).all()) and bool((d_pos == -7).all()) and bool((d_out == -7.0).all())
    e.ais_frames(d_y, 1, n, d_msg, d_len, d_row, d_pos, d_score, d_count, 4)      # and the same buffers are taken as they are
    e.sync()
    assert int(d_count.cpu()[0]) == 1 and int(d_pos.cpu()[0]) == A.flag_start(60)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def capture(fs, n, seed):
    """Two channels, six bursts each at 20 dB in the 48 kS/s band, some overlapping in time across the channels -> (complex64 [n] at fs
    centred on 162.0 MHz, {channel: [(mmsi, lon, lat)]})."""
    n48 = n * 48000 // int(fs)
    assert n48 * int(fs) == n * 48000
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.complex128)
    t = np.arange(n) / fs
    sent = {}
    for ch, (off, shift) in enumerate(((-25e3, 0), (25e3, 600))):
        ships = [(211000000 + 100 * ch + i, round(8.0 + 0.01 * i + ch, 4), round(53.5 + 0.02 * i, 4)) for i in range(6)]
        bursts = [(A.with_crc(A.type1(m, lon, lat, speed=5 + i, course=10.0 * i, second=i)), 250 + shift + 1850 * i, 1.0, 0.0)
                  for i, (m, lon, lat) in enumerate(ships)]
        b = A.synth(n48, bursts)
        spec = np.fft.fft(b.astype(np.complex128))
        wide = np.zeros(n, np.complex128)
        wide[:n48 // 2], wide[-(n48 // 2):] = spec[:n48 // 2], spec[-(n48 // 2):]
        x += np.fft.ifft(wide) * (n / n48) * np.exp(2j * np.pi * off * t)
        sent["AB"[ch]] = ships
    sigma = np.sqrt(10.0 ** (-20.0 / 10.0) / 2 * fs / 48000.0)
    x += sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), sent


@pytest.mark.parametrize("fs,n", [(2.4e6, 600000), (250e3, 250000)])
def test_recording_end_to_end(e, fs, n):
    x, sent = capture(fs, n, seed=int(fs) % 97)
    assert Engine.ais_plan(fs) == ((50, 1, 1) if fs == 2.4e6 else (5, 24, 25))
    out = F.ais_recording(x, fs)
    assert out["fs"] == 48000
    for ch in "AB":
        got = [(f["mmsi"], round(f["lon"], 4), round(f["lat"], 4)) for f in out["frames"] if f["channel"] == ch]
        assert got == sent[ch], (ch, got)
    assert len(out["frames"]) == 12 and [t["frames"] for t in out["tracks"]] == [1] * 12
    assert len(out["nmea"]) == 12 and all(s.startswith("!AIVDM,1,1,,") for s in out["nmea"])
    assert [F.ais_payload([s]) for s in out["nmea"]] == [f["msg"] for f in out["frames"]]
    again = F.ais_recording(x, fs, chunk_samples=77777)
    assert again["frames"] == out["frames"] and again["nmea"] == out["nmea"]

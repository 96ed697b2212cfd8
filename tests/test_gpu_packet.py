"""The packet-radio kernels (k_packet_front; k_packet_detect, pss_starts.h's k_starts_scan and k_starts_gather, k_packet_walk, k_packet_keep,
k_packet_emit) against pss_h_packet_front and pss_h_packet_frames on every byte of every output, and formats.packet_rows /
packet_recording end to end.  Buffers lie between NaNs, rows are strided with NaNs in the gaps, and a sentinel sits behind max_frames and
behind each row's window.  The shapes are the smallest at which each path is taken: row lengths around the window's halves and the front's
and the detect kernel's tiles, one (row, tile) pair past each grid cap in many short rows, a flag on each side of a detect-tile boundary,
the 330-byte frame across the tiles it spans, more survivors in a tile than a wavefront holds and more than one pass of the list kernels
takes, a count above max_frames, equal scores, rows that must not run into each other, windows with exactly their reach.  The caps and
tile sizes come from tests/packet_caps.py, where tests/test_packet_caps.py and, for the shared start list, tests/test_launch_caps.py pin
them to the source lines."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packet_cases as P
from bytes_util import same_bytes
from gpu_util import dev
from packet_caps import DETECT_GRID_CAP, FRONT_GRID_CAP, FRONT_TILE, GATHER_GRID_CAP, LIST_PASS, SCAN_STEP, TILE, WAVE   # pinned by tests/test_packet_caps.py
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
WHAT = ("msg", "len", "row", "pos", "score")
GOOD = P.with_crc(P.FRAMES["status"])
GOOD_BITS = P.burst_bits(GOOD, lead=1, tail=1)
assert P.TILE == TILE and P.FRONT_TILE == FRONT_TILE


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


def same_z(a, b):
    """Every bit; a NaN for a NaN (the sign and payload of a NaN that arithmetic made are the processor's)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- front --------------------------------------------------------------------------------------------------------------------------------
def front_on_device(e, x, tones=None, space_gain=1.0, buf_index0=0, n_row=None, i_begin=0, i_end=None, gap=3):
    x = np.asarray(x, np.complex64)
    rows = x[None, :] if x.ndim == 1 else x
    r, n = rows.shape
    n_row = buf_index0 + n if n_row is None else n_row
    i_end = n_row if i_end is None else i_end
    width = i_end - i_begin
    d_x, off, stride = strided(rows, gap)
    z_stride = width + 2
    d_z = torch.full((r * z_stride + 1,), -7.0, dtype=torch.float32, device="cuda")
    e.packet_front(d_x.data_ptr() + 8 * off, r, n, d_z, tones=tones, space_gain=space_gain, x_stride=stride, buf_index0=buf_index0, n_row=n_row,
                   i_begin=i_begin, i_end=i_end, z_stride=z_stride)
    e.sync()
    z = d_z.cpu().numpy()
    assert z[-1] == -7.0
    out = z[:-1].reshape(r, z_stride)
    assert np.all(out[:, width:] == -7.0)                          # nothing behind a row's window
    return out[:, :width] if x.ndim == 2 else out[0, :width]


def check_front(e, x, gap=3, **kw):
    want = Engine.h_packet_front(x, **kw)
    got = front_on_device(e, x, gap=gap, **kw)
    assert same_z(got, want), (np.nonzero(got.view(np.uint32) != want.view(np.uint32)), got, want)
    return want


def noisy(n, seed, rows=None):
    rng = np.random.default_rng(seed)
    shape = (n,) if rows is None else (rows, n)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def test_front_lengths_around_the_window_and_the_tiles(e):
    for n in (1, 2, 10, 11, 12, 21, 22, 23, FRONT_TILE - 1, FRONT_TILE, FRONT_TILE + 1, FRONT_TILE + 12, TILE - 1, TILE, TILE + 1):
        check_front(e, noisy(n, 100 + n))
        check_front(e, noisy(n, 200 + n), space_gain=0.35)


def test_front_rows_with_gaps_special_samples_and_another_table(e):
    x = noisy(3000, 5, rows=3)
    x[0, 10] = np.nan
    x[1, 500] = np.inf + 0j
    x[1, 2047] = complex(0.0, -np.inf)
    x[2, 100:160] = 0
    x[2, 200:260] = 1.0                                             # a bare carrier: d = 0 over the whole window, den == 0
    x[2, 300] = complex(-0.0, 0.0)
    x[2, 2999] = np.nan
    z = check_front(e, x, gap=7)
    assert np.isnan(z[0, 0:23]).all() and np.isfinite(z[0, 23:]).all()           # d[10] and d[11] are NaNs
    assert z[2, 212:250].tobytes() == np.zeros(38, np.float32).tobytes()
    rng = np.random.default_rng(9)
    check_front(e, x, tones=rng.standard_normal((4, 22)), space_gain=2.5)
    check_front(e, noisy(500, 6), tones=np.zeros((4, 22)))          # den == 0 everywhere: +0


def test_front_one_pair_past_the_grid_cap(e):
    check_front(e, noisy(30, 6, rows=FRONT_GRID_CAP + 1))           # one tile a row: pair 2048 is the grid-stride loop's second round
    check_front(e, noisy(FRONT_TILE * 3 + 1, 7, rows=5))            # rows x tiles, walked in pairs


def test_front_windows_with_exactly_their_halo(e):
    n = 3 * FRONT_TILE
    x = noisy(n, 8, rows=2)
    whole = Engine.h_packet_front(x)
    for i0, i1 in ((0, 1), (1, 2), (11, 12), (12, FRONT_TILE + 13), (FRONT_TILE - 1, 2 * FRONT_TILE + 1), (n - 3, n), (0, n)):
        lo, hi = P.front_span(i0, i1, n)
        got = check_front(e, x[:, lo:hi], buf_index0=lo, n_row=n, i_begin=i0, i_end=i1)
        assert same_z(got, whole[:, i0:i1])


# ---- frames -------------------------------------------------------------------------------------------------------------------------------
def on_device(e, z, q_min=0.0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, gap=3):
    """h_packet_frames' result from the device."""
    z = np.asarray(z, np.float32)
    rows = z[None, :] if z.ndim == 1 else z
    r, n = rows.shape
    n_row = buf_index0 + n if n_row is None else n_row
    s_end = n_row if s_end is None else s_end
    d_z, off, stride = strided(rows, gap)
    mf = 256 if max_frames is None else max_frames
    room = mf + 3
    d_msg = torch.full((room, P.REC_BYTES), SENTINEL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_row = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_pos = torch.full((room,), -7, dtype=torch.int64, device="cuda")
    d_score = torch.full((room,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    e.packet_frames(d_z.data_ptr() + 4 * off, r, n, d_msg, d_len, d_row, d_pos, d_score, d_count, mf, q_min=q_min, z_stride=stride, buf_index0=buf_index0,
                    n_row=n_row, s_begin=s_begin, s_end=s_end)
    e.sync()
    msg, ln, rw, pos, score, count = (t.cpu().numpy() for t in (d_msg, d_len, d_row, d_pos, d_score, d_count))
    assert count[1] == -7
    k = min(int(count[0]), mf)
    assert np.all(msg[k:] == SENTINEL) and np.all(ln[k:] == -7) and np.all(rw[k:] == -7) and np.all(pos[k:] == -7) and np.all(score[k:] == -7.0)
    return msg[:k], ln[:k], rw[:k], pos[:k], score[:k], int(count[0])


def check(e, z, max_frames=256, gap=3, **kw):
    """Device == twin on every byte -> the twin's result."""
    want = Engine.h_packet_frames(z, max_frames=max_frames, **kw)
    got = on_device(e, z, max_frames=max_frames, gap=gap, **kw)
    for g, w, what in zip(got[:5], want[:5], WHAT):
        assert same_bytes(g, w), (what, g, w)
    assert got[5] == want[5]
    return want


def frames_of(r):
    return [bytes(m[:n]) for m, n in zip(r[0], r[1])]


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_fixture_rows_front_and_frames(e, name):
    c = P.CASES[name]
    z = check_front(e, P.case_iq(name), space_gain=c["gain"])
    r = check(e, z)
    assert frames_of(r) == c["expect"]


def test_row_lengths_around_the_first_start_and_the_tile(e):
    for n in (1, 12, 22, 23, 176, 177, 178):
        check(e, np.ones(n, np.float32))
    z, s, n = P.edge_row()
    assert n < TILE
    for m in (TILE - 1, TILE, TILE + 1, FRONT_TILE, FRONT_TILE + 1):
        y = np.zeros(m, np.float32)
        y[:min(n, m)] = z[:m]
        assert check(e, y, q_min=0.5)[5] == (1 if m >= n else 0)
    assert check(e, z, q_min=0.5)[3].tolist() == [s] and check(e, z[:-1], q_min=0.5)[5] == 0      # the look-ahead on the row's last sample


def test_a_flag_on_each_side_of_a_tile_boundary(e):
    for s in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 10):
        z = P.direct_z(s + P.SPB * len(GOOD_BITS) + 50, [(GOOD_BITS, s, 0.25, 1.0)])
        assert check(e, z, q_min=0.5)[3].tolist() == [s]
        # the 22 starts of the flag's cell lie on both sides of the boundary: equal scores, the earliest stays
        r = check(e, P.direct_z(s + P.SPB * len(GOOD_BITS) + 50, [(GOOD_BITS, s)]))
        assert r[3].tolist() == [s - 11] and frames_of(r) == [GOOD]


def test_the_330_byte_frame_across_the_tiles_it_spans(e):
    frame = P.with_crc(P.FRAMES["long"])
    bits = P.burst_bits(frame, lead=3, tail=1)
    s = TILE - 30                                                    # the frame's flag: the third
    at = s - 16 * P.SPB
    last = at + P.SPB * (len(bits) - 1)
    assert 70000 < last < 80000 and last // TILE - s // TILE >= 16
    z = P.direct_z(last + 1, [(bits, at, 0.25, 1.0)])
    r = check(e, z, q_min=0.5)                                       # it ends exactly with the row
    assert frames_of(r) == [frame] and r[3].tolist() == [s] and r[1].tolist() == [330]
    assert check(e, z[:-1], q_min=0.5)[5] == 0                       # one sample shorter
    # through the front, with noise and a fast clock: the front's 37 tiles and the detect kernel's 19
    x = P.synth(76000, [(P.burst_bits(frame, lead=12), 700, 1.004)], snr_db=15.0, seed=51)
    zz = check_front(e, x)
    assert frames_of(check(e, zz)) == [frame]
    too_long = P.with_crc(P.FRAMES["long"] + b"\x55")
    assert check(e, P.direct_z(76000, [(P.burst_bits(too_long, lead=2), 100)]))[5] == 0


def test_thousands_of_one_tile_rows_past_every_grid_cap(e):
    """SCAN_STEP + 1 rows of one short burst's length: tpr == 1, one tile past a step of the counts' scan, four rounds of the detect grid
    and two passes of the gather's.  The rows of every other round of the detect grid carry the burst, so every workgroup meets tiles with,
    without, with, without survivors and workgroup 0 a fifth with them."""
    R = SCAN_STEP + 1
    assert R > GATHER_GRID_CAP and R > 4 * DETECT_GRID_CAP and P.SHORT_N <= TILE
    z = P.short_rows(R, DETECT_GRID_CAP)
    rows = P.carrying(R, DETECT_GRID_CAP)
    full = check(e, z, max_frames=R + 10)
    assert full[5] == len(rows) == 2 * DETECT_GRID_CAP + 1
    assert full[2].tolist() == rows and full[3].tolist() == [P.short_at(r) - 11 for r in rows]
    assert set(frames_of(full)) == {P.SHORT_FRAME}
    assert check(e, z, max_frames=0)[5] == len(rows)                 # a count above max_frames
    cut = check(e, z, max_frames=len(rows) // 2 + 3)
    assert cut[5] == len(rows) and cut[2].tolist() == rows[:len(rows) // 2 + 3]


def test_more_survivors_in_a_tile_than_a_wavefront_holds(e):
    z, starts = P.dense_row(200)
    assert 22 * len(starts) / (len(z) / TILE) > 2 * WAVE
    assert check(e, z)[5] == 0
    # and with a frame behind the run of flags: every flag but the last ends in the walk as a frame of no bits
    bits = list(P.FLAG) * 60 + P.burst_bits(GOOD, lead=1, tail=1)
    r = check(e, P.direct_z(P.BACK + 11 + P.SPB * len(bits) + 40, [(bits, P.BACK + 11)]))
    assert frames_of(r) == [GOOD] and r[3].tolist() == [P.BACK + 60 * 8 * P.SPB]


def test_more_survivors_than_one_pass_of_the_list_kernels(e):
    z, starts = P.dense_row(LIST_PASS // 22 + 60)
    assert 22 * len(starts) > LIST_PASS
    tail = P.direct_z(P.BACK + 11 + P.SPB * len(GOOD_BITS) + 40, [(GOOD_BITS, P.BACK + 11)])
    r = check(e, np.concatenate([z, tail]))
    assert r[5] == 1 and r[3].tolist() == [len(z) + P.BACK] and frames_of(r) == [GOOD]


def test_equal_scores_keep_the_earlier_start(e):
    s = TILE - 2
    z = P.direct_z(s + P.SPB * len(GOOD_BITS) + 50, [(GOOD_BITS, s)])
    assert check(e, z)[3].tolist() == [s - 11]
    for k in (-10, 0, 10):
        assert check(e, z, s_begin=s + k)[5] == 0                 # the earliest lies outside the window and still drops the others
    assert check(e, z, s_end=s - 11)[5] == 0 and check(e, z, s_end=s - 10)[5] == 1
    y = z.copy()
    y[s + 3 + P.SPB * np.arange(-1, 8)] *= 1.5
    assert check(e, y)[3].tolist() == [s + 3]


def test_rows_do_not_run_into_each_other(e):
    n = P.BACK + 11 + P.SPB * (len(GOOD_BITS) - 1) - 40
    flat = P.direct_z(2 * n, [(GOOD_BITS, P.BACK + 11)])
    assert frames_of(check(e, flat)) == [GOOD]
    assert check(e, flat.reshape(2, n))[5] == 0
    assert check(e, flat.reshape(2, n), gap=0)[5] == 0             # the rows back to back in memory
    other = P.burst_bits(P.with_crc(P.FRAMES["short"]), lead=2, tail=1)
    rows = np.stack([P.direct_z(12000, [(GOOD_BITS, 40 + 7 * k), (other, 7000 - 11 * k)]) for k in range(4)])
    r = check(e, rows)
    assert r[2].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and r[5] == 8


def test_windows_with_exactly_their_reach(e):
    other = P.burst_bits(P.with_crc(P.FRAMES["compressed"]), lead=2, tail=1)
    n = 80000                                                        # longer than a start's reach
    starts = [200, 3 * TILE - 1, 5 * TILE + 2000, n - 12000]
    z = np.stack([P.direct_z(n, [(GOOD_BITS if k & 1 else other, s) for k, s in enumerate(starts)]),
                  P.direct_z(n, [(other, 900, 0.5, 1.0)])])
    whole = check(e, z)
    assert whole[5] == 5
    assert whole[3].tolist()[:2] == [200 + 8 * P.SPB - 11, 3 * TILE - 12]
    for cuts in ([100, 150, 365, 366, 3 * TILE - 12, 3 * TILE, 3 * TILE + 10], [n - P.REACH, 5 * TILE + 7, n - 12000], [1]):
        edges = [0] + cuts + [n]
        parts = []
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = P.reach(s0, s1, n)
            parts.append(check(e, z[:, lo:hi], buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
        order = np.lexsort((np.concatenate([q[3] for q in parts]), np.concatenate([q[2] for q in parts])))
        for i in range(5):
            assert same_bytes(np.concatenate([q[i] for q in parts])[order], whole[i]), (cuts, i)


def test_non_finite_samples(e):
    z = P.direct_z(P.BACK + P.SPB * len(GOOD_BITS) + 50, [(GOOD_BITS, P.BACK, 0.25, 1.0)])
    s = P.BACK
    for at, v in ((s - 22, np.nan), (s + 44, np.nan), (s + 300, np.inf), (s + 301, -np.inf), (s + 500, np.nan), (3, np.nan)):
        y = z.copy()
        y[at] = v
        check(e, y, q_min=0.5)
        check(e, y)
    check(e, np.full(500, np.nan, np.float32))
    check(e, np.zeros(10, np.float32))
    check(e, np.zeros(177, np.float32))


def test_a_refused_device_call_writes_nothing(e):
    from pyspecsdr_amd.engine import PssError
    z = P.direct_z(P.BACK + P.SPB * len(GOOD_BITS) + 50, [(GOOD_BITS, P.BACK, 0.25, 1.0)])
    n = len(z)
    d_z = dev(z)
    d_msg = torch.full((4, P.REC_BYTES), SENTINEL, dtype=torch.uint8, device="cuda")
    d_len, d_row = torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int32, device="cuda")
    d_pos, d_score = torch.full((4,), -7, dtype=torch.int64, device="cuda"), torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    reach = "the buffer does not cover the window's reach (21 starts either side, 22 samples back, 73203 samples forward)"
    for why, kw in (("n_rows outside [1, 2^20]", dict(n_rows=0)), ("z_stride < n_buf", dict(z_stride=n - 1)), ("s_end < s_begin", dict(s_begin=5, s_end=4)),
                    ("the window does not lie inside the row", dict(s_end=n + 1)), (reach, dict(n_row=1000000, s_end=900)),
                    (reach, dict(buf_index0=50, n_row=n + 50, s_begin=92, s_end=93)), ("max_frames < 0", dict(max_frames=-1)),
                    ("q_min must be finite and >= 0", dict(q_min=-1.0)), ("q_min must be finite and >= 0", dict(q_min=float("nan"))),
                    ("a misaligned pointer", dict(z=d_z.data_ptr() + 2)), ("null buffer", dict(count=None))):
        kw = dict(kw)
        args = dict(z=kw.pop("z", d_z), n_rows=kw.pop("n_rows", 1), max_frames=kw.pop("max_frames", 4), count=kw.pop("count", d_count))
        with pytest.raises(PssError, match=re.escape("pss_packet_frames: " + why)):
            e.packet_frames(args["z"], args["n_rows"], n, d_msg, d_len, d_row, d_pos, d_score, args["count"], args["max_frames"], **kw)
    d_x = dev(noisy(100, 3))
    d_out = torch.full((100,), -7.0, dtype=torch.float32, device="cuda")
    bad = P.tones()
    bad[1, 3] = np.nan
    halo = r"the buffer does not cover the window's halo \(12 samples in front, 10 behind\)"
    for why, kw in (("a table entry that is not finite", dict(tones=bad)), ("space_gain must be finite and > 0", dict(space_gain=0.0)),
                    ("space_gain must be finite and > 0", dict(space_gain=float("inf"))), (halo, dict(n_row=200, i_end=96)),
                    ("the window does not lie inside the row", dict(i_end=101)), ("x_stride < n_buf", dict(x_stride=99))):
        with pytest.raises(PssError, match="pss_packet_front: " + why):
            e.packet_front(d_x, 1, 100, d_out, **kw)
    e.sync()
    assert int(d_count.cpu()[0]) == -7 and bool((d_msg == SENTINEL).all()) and bool((d_pos == -7).all()) and bool((d_out == -7.0).all())
    e.packet_frames(d_z, 1, n, d_msg, d_len, d_row, d_pos, d_score, d_count, 4, q_min=0.5)      # and the same buffers are taken as they are
    e.sync()
    assert int(d_count.cpu()[0]) == 1 and int(d_pos.cpu()[0]) == P.BACK


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
CENTER = 144.8e6
CHANNELS = (144.775e6, 144.825e6)


def capture(fs, n, seed):
    """Two channels 25 kHz either side of the centre, three frames each at 20 dB in the 26.4 kS/s band with clock factors 1, 1.003 and 0.997,
    overlapping in time across the channels -> (complex64 [n] at fs, [frames per channel])."""
    n26 = n * 26400 // int(fs)
    assert n26 * int(fs) == n * 26400
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.complex128)
    t = np.arange(n) / fs
    sent = []
    for ch, shift in enumerate((0, 900)):
        frames = [P.with_crc(P.ui_frame(("APRS", 0), ("N%dCALL" % ch, i), [("WIDE2", 1, False)], b"!49%02d.50N/07201.75W>channel %d frame %d" % (i, ch, i)))
                  for i in range(3)]
        b = P.synth(n26, [(P.burst_bits(f, lead=10), 400 + shift + 15000 * i, clock) for i, (f, clock) in enumerate(zip(frames, (1.0, 1.003, 0.997)))])
        spec = np.fft.fft(b.astype(np.complex128))
        wide = np.zeros(n, np.complex128)
        wide[:n26 // 2], wide[-(n26 // 2):] = spec[:n26 // 2], spec[-(n26 // 2):]
        x += np.fft.ifft(wide) * (n / n26) * np.exp(2j * np.pi * (CHANNELS[ch] - CENTER) * t)
        sent.append(frames)
    sigma = np.sqrt(10.0 ** (-20.0 / 10.0) / 2 * fs / 26400.0)
    x += sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), sent


@pytest.mark.parametrize("fs,n", [(264e3, 480000), (240e3, 480000)])
def test_recording_end_to_end_on_two_channels(e, fs, n):
    x, sent = capture(fs, n, seed=int(fs) % 97)
    decim, up, down = Engine.packet_plan(fs)
    assert (decim, up, down) == ((10, 1, 1) if fs == 264e3 else (9, 99, 100))
    out = F.packet_recording(x, fs, CENTER, CHANNELS)
    assert out["fs"] == 26400
    for ch in range(2):
        assert [f["msg"] + P.crc16(f["msg"]).to_bytes(2, "little") for f in out["frames"] if f["row"] == ch] == sent[ch], ch
    assert len(out["frames"]) == 6 and [t["frames"] for t in out["tracks"]] == [1] * 6 and len(out["lines"]) == 6
    assert out["lines"][0].startswith("N0CALL>APRS,WIDE2-1:!4900.50N/07201.75W>channel 0 frame 0")
    # the host twins of the same route give the same records, whatever the chunking
    taps = np.empty(20 * decim + 1, np.float64)
    assert e.lib.pss_design_firwin(len(taps), 16000.0 / fs, taps.ctypes.data) == 0
    words = [Engine.ddc_word(c - CENTER, fs)[0] for c in CHANNELS]
    rows = Engine.h_ddc(x, words, decim, taps=taps)
    if (up, down) != (1, 1):
        rows = Engine.h_resample(rows, up, down)
    want = F.h_packet_rows(rows)
    for chunk in (1 << 22, 77777):
        again = F.packet_recording(x, fs, CENTER, CHANNELS, chunk_samples=chunk)
        assert again["frames"] == want and again["lines"] == [f["tnc2"] for f in want]
    # rows resident on the device go through packet_rows as they are
    assert F.packet_rows(rows) == want

"""The ADS-B kernels (k_adsb_detect, pss_starts.h's k_starts_scan and k_starts_gather, k_adsb_keep, k_adsb_emit) against pss_h_adsb_frames on every
byte — the messages, pos, the meta word, the score bits and the count — and formats.adsb_recording end to end.  The shapes are the smallest
at which each path is taken: frames on both sides of a tile boundary, one tile past the grid cap, more survivors in a tile than a wavefront
holds and more than one pass of the second compaction takes (ratio 0, at every rate that has its own LDS extent), more accepted frames than
one step of the scan and than one pass of the list kernels, a count above max_frames, windows with exactly their reach, of less than a tile
and of a tile and a few starts; 4097 tiles, so that a workgroup of the detect kernel walks five and the tiles' counts carry in the scan;
every downlink format; up to eight starts with one score; frames that end with the capture.  The caps and tile sizes come from
tests/launch_caps.py, where tests/test_launch_caps.py pins them to the source lines.

A frame spans at most 240 * 8 = 1920 samples and a tile of the detect kernel is 4096 starts, so no frame covers three tiles: the spc 8 case
below puts one across a boundary and its reach into the tile after."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adsb_cases as A
from bytes_util import same_bytes
from gpu_util import dev
from launch_caps import DETECT_GRID_CAP, DETECT_TILE, LIST_PASS, LS_GRID_CAP, SCAN_STEP   # pinned to csrc/pss_starts.h and pss_adsb.hip by tests/test_launch_caps.py
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adsb.npz"))
NAMES = [str(n) for n in GOLD["names"]]
SENTINEL = 0xA5
assert A.TILE == DETECT_TILE


@pytest.fixture(scope="module")
def e():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    eng = Engine(0)
    yield eng
    eng.close()


def on_device(e, x, spc, ratio=2.0, icao=(), buf_index0=0, n_capture=None, s_begin=0, s_end=None, max_frames=None):
    """h_adsb_frames' result from the device.  The buffer lies between NaNs, and every output carries a sentinel behind max_frames."""
    x = np.ascontiguousarray(x, np.complex64)
    n_capture = buf_index0 + len(x) if n_capture is None else n_capture
    s_end = n_capture if s_end is None else s_end
    wide = np.full(len(x) + 4, np.nan, np.complex64)
    wide[2:2 + len(x)] = x
    d_wide = dev(wide)
    a = np.ascontiguousarray(icao, np.uint32)
    d_icao = torch.from_numpy(a.view(np.int32)).cuda() if len(a) else None
    mf = 256 if max_frames is None else max_frames
    room = mf + 3
    d_msg = torch.full((room, 14), SENTINEL, dtype=torch.uint8, device="cuda")
    d_pos = torch.full((room,), -7, dtype=torch.int64, device="cuda")
    d_meta = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    d_score = torch.full((room,), -7.0, dtype=torch.float32, device="cuda")
    d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    e.adsb_frames(d_wide.data_ptr() + 16, len(x), spc, d_msg, d_pos, d_meta, d_score, d_count, mf, ratio=ratio, d_icao=d_icao, n_icao=len(a),
                  buf_index0=buf_index0, n_capture=n_capture, s_begin=s_begin, s_end=s_end)
    e.sync()
    msg, pos, meta, score, count = (t.cpu().numpy() for t in (d_msg, d_pos, d_meta, d_score, d_count))
    assert count[1] == -7
    k = min(int(count[0]), mf)
    assert np.all(msg[k:] == SENTINEL) and np.all(pos[k:] == -7) and np.all(meta[k:] == -7) and np.all(score[k:] == -7.0)   # nothing past max_frames
    return msg[:k], pos[:k], meta[:k].view(np.uint32), score[:k], int(count[0])


def check(e, x, spc, max_frames=256, **kw):
    """Device == twin on every byte -> the twin's result."""
    want = Engine.h_adsb_frames(x, spc, max_frames=max_frames, **kw)
    got = on_device(e, x, spc, max_frames=max_frames, **kw)
    for g, w, what in zip(got[:4], want[:4], ("msg", "pos", "meta", "score")):
        assert same_bytes(g, w), (what, g, w)
    assert got[4] == want[4]
    return want


@pytest.mark.parametrize("name", NAMES)
def test_fixture_captures(e, name):
    spc = A.CASES[name][0]
    iq = A.case_iq(name)
    assert A.capture_crc32(iq) == int(GOLD[name + "/crc32"][0])
    msg, pos, meta, score, count = check(e, iq, spc, icao=GOLD[name + "/addresses"])
    assert same_bytes(msg, GOLD[name + "/msg"]) and same_bytes(pos, GOLD[name + "/pos"]) and same_bytes(meta, GOLD[name + "/meta"])
    assert same_bytes(score, GOLD[name + "/score"]) and count == len(pos)
    assert [(bytes(m), int(p)) for m, p in zip(msg, pos)] == A.case_expected(name)


@pytest.mark.parametrize("spc", [3, 8])
def test_frames_at_a_tile_boundary(e, spc):
    S = DETECT_TILE
    for k, p in enumerate((S - 1, S, S + 1, S - 100 * spc)):
        n = p + 240 * spc + 50
        rng_frames = [(A.IDENT, 17, 10.0, 0.4), (A.POS_EVEN, p, 10.0, 1.1)]
        x = A.synth(n, spc, rng_frames, seed=[77, spc, k])
        msg, pos, meta, score, count = check(e, x, spc)
        assert pos.tolist() == [17, p], (p, pos)


def test_twin_starts_on_both_sides_of_a_tile_boundary(e):
    S = DETECT_TILE
    for p in (S - 2, S - 1, S):            # the starts p and p + 1 are both accepted and carry the same score
        x, _ = A.twin_starts(p)
        msg, pos, meta, score, count = check(e, x, 2)
        assert pos.tolist() == [p] and count == 1
        # through a window that holds only the later one: its suppressor lies outside the window and still drops it
        assert check(e, x, 2, s_begin=p + 1)[4] == 0


def test_one_tile_past_the_grid_cap(e):
    S, cap = DETECT_TILE, DETECT_GRID_CAP
    n = (cap + 1) * S + 300                 # tiles 0 .. cap, and a short last one: the first workgroup walks two tiles
    at = [5, cap * S + 7, n - 240 - 3]
    x = np.zeros(n, np.complex64)           # zeros fail the strict preamble test: the twin stays quick
    for p, m in zip(at, (A.IDENT, A.POS_EVEN, A.VELOCITY)):
        x[p:p + 240] = A.chips_of(m)
    msg, pos, meta, score, count = check(e, x, 1)
    assert pos.tolist() == at


def test_more_survivors_in_a_tile_than_a_wavefront_holds(e):
    rng = np.random.default_rng(2024)
    x = np.zeros(6000, np.complex64)
    pre = np.zeros(16)
    pre[list(A.PULSES)] = 1.0
    for k in range(100):                     # a hundred clean preambles 40 samples apart, chip pairs of garbage between and behind them
        x[40 * k:40 * k + 16] = pre
        x[40 * k + 16:40 * k + 40] = rng.integers(0, 2, 24)
    x[4000:4300] = rng.integers(0, 2, 300)
    x[4400:4640] = A.chips_of(A.IDENT)
    msg, pos, meta, score, count = check(e, x, 1)
    assert 4400 in pos.tolist()


def test_more_survivors_in_a_tile_than_one_pass_of_the_second_compaction(e):
    """ratio 0 passes every start whose four pulse chips hold any energy: in noise that is nearly every start of a tile, so the loop that
    compacts the accepted survivors runs past its first 1024 and carries its count.  Frames among the noise give it something to keep."""
    spc, n = 2, DETECT_TILE + 3000
    x = A.synth(n, spc, [(A.IDENT, 700, 10.0, 0.2), (A.ALL_CALL, 2500, 10.0, 0.9), (A.VELOCITY, DETECT_TILE - 5, 10.0, 1.7)], seed=[88, 0])
    want = check(e, x, spc, ratio=0.0, max_frames=512)
    assert {700, 2500, DETECT_TILE - 5} <= set(want[1].tolist())
    # the three frames sit near survivors 700, 2500 and 4091 of the first tile's list: in the first, third and fourth pass of that loop
    assert want[4] >= 3


def test_more_than_64_frames_and_a_count_above_max_frames(e):
    msgs = [A.ALL_CALL, A.IDENT, A.ALT_REPLY]
    frames, p = [], 3
    for k in range(300):
        m = msgs[k % 3]
        frames.append((m, p))
        p += 16 + 8 * len(m) + (k % 5)
    x = A.clean(p + 10, 1, frames)
    want = check(e, x, 1, icao=[A.ADDRESS], max_frames=400)
    assert want[4] == 300 and want[1].tolist() == [q for _, q in frames]
    short = check(e, x, 1, icao=[A.ADDRESS], max_frames=10)
    assert short[4] == 300 and len(short[1]) == 10
    assert check(e, x, 1, icao=[A.ADDRESS], max_frames=0)[4] == 300
    assert check(e, x, 1, max_frames=400)[4] == 200           # without the address the DF 4 replies are not reported


def test_more_kept_frames_than_one_step_of_the_scan(e):
    k = SCAN_STEP + 104                       # short frames back to back: the ranks carry over from one step of k_starts_scan to the next
    x = A.clean(3 + 128 * k + 5, 1, [(A.ALL_CALL, 3 + 128 * i) for i in range(k)])
    want = check(e, x, 1, max_frames=k + 10)
    assert want[4] == k and want[1].tolist() == [3 + 128 * i for i in range(k)]


def test_windows_with_exactly_their_reach_and_a_far_index(e):
    x, cuts = A.windows_capture()
    n, spc = len(x), 2
    whole = check(e, x, spc)
    assert whole[4] == 3
    for base in (0, 2 ** 40 + 777):
        pad = 2 * spc - 1 if base else 0        # the virtual capture holds samples in front of ours: the first window's reach goes there
        xx = np.concatenate([np.zeros(pad, np.complex64), x])
        origin = base - pad
        parts = []
        edges = [0] + cuts + [n]
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = A.reach(base + s0, base + s1, spc, base + n)
            parts.append(check(e, xx[lo - origin:hi - origin], spc, buf_index0=lo, n_capture=base + n, s_begin=base + s0, s_end=base + s1))
        for i in range(4):
            joined = np.concatenate([p[i] for p in parts])
            assert same_bytes(joined, whole[i] + base if i == 1 else whole[i]), (base, i)
        assert sum(p[4] for p in parts) == whole[4]


def test_non_finite_samples_stay_in_their_frame(e):
    name = "spc3"
    spc = A.CASES[name][0]
    x = A.case_iq(name).copy()
    ref = Engine.h_adsb_frames(x, spc)
    p = int(ref[1][1])
    x[p + spc] = np.nan                      # in a gap of the preamble, and so in chip 0 or 1 of every start that could slice this frame
    x[p + spc * 90 + 1] = np.inf
    got = check(e, x, spc)
    assert got[1].tolist() == [q for q in ref[1].tolist() if q != p]


def test_address_list(e):
    x = A.clean(400, 1, [(A.ALT_REPLY, 11), (A.ALL_CALL, 200)])
    first = (A.ADDRESS + 7 * np.arange(1000)).astype(np.uint32)             # the address as the first and as the last of 1000 entries
    last = (A.ADDRESS - 7 * np.arange(999, -1, -1)).astype(np.uint32)
    others = first[1:]
    assert first[0] == A.ADDRESS and last[-1] == A.ADDRESS and len(last) == 1000
    for icao, n_want in (((), 1), ([A.ADDRESS], 2), (first, 2), (last, 2), (others, 1)):
        assert check(e, x, 1, icao=icao)[4] == n_want


def test_recording_end_to_end(e):
    name = "spc2"
    spc, n, seed, amp, addresses, frames = A.CASES[name]
    iq = A.case_iq(name)
    fs = 2e6 * spc
    big = F.adsb_recording(iq, fs, addresses=(), learn=True)
    small = F.adsb_recording(iq, fs, addresses=(), learn=True, chunk_samples=240 * spc)     # shorter than one frame's reach plus one
    assert big["frames"] == small["frames"] and big["fs"] == fs
    want = Engine.h_adsb_frames(iq, spc, icao=[A.ADDRESS])
    assert [f["pos"] for f in big["frames"]] == want[1].tolist()
    assert [f["msg"].ljust(14, b"\0") for f in big["frames"]] == [bytes(m) for m in want[0]]
    assert np.array_equal(np.array([f["score"] for f in big["frames"]], np.float32), want[3])
    # POS_ODD and IDENT teach the pass nothing about 4840D6 ... IDENT does: the DF 4 reply comes with learn, and not without
    assert 4 in [f["df"] for f in big["frames"]]
    plain = F.adsb_recording(iq, fs, learn=False)
    assert 4 not in [f["df"] for f in plain["frames"]] and len(plain["frames"]) == len(big["frames"]) - 1
    # cu8 codes of the same capture: the records of the twin on the widened buffer
    table = F.iq_table("cu8")
    scale = 16.0
    codes = np.clip(np.round(np.stack([iq.real, iq.imag], -1) / scale * 128.0 + 127.4), 0, 255).astype(np.uint8)
    wide = F.unpack_iq(codes, "cu8", table)
    from_codes = F.adsb_recording(codes, fs, codes_format="cu8", table=table, chunk_samples=1000)
    w = Engine.h_adsb_frames(wide, spc, icao=[A.ADDRESS])
    assert [f["pos"] for f in from_codes["frames"]] == w[1].tolist()
    assert np.array_equal(np.array([f["score"] for f in from_codes["frames"]], np.float32), w[3])
    assert [f["msg"] for f in from_codes["frames"]] == [f["msg"] for f in big["frames"]]


def test_recording_resamples_a_dongle_rate(e):
    fs = 2.4e6
    t_us = A.RATE_CASE_US                                      # the frames' first instants, microseconds: on no sample of either rate
    msgs = [A.IDENT, A.POS_EVEN, A.VELOCITY, A.ALL_CALL]
    x = A.synth_rate(24000, fs, [(m, t0, 10.0, 0.3 + i) for i, (m, t0) in enumerate(zip(msgs, t_us))], seed=A.RATE_CASE_SEED)
    out = F.adsb_recording(x, fs)
    assert out["fs"] == 4e6
    # the same through the host twins: the resident row is pss_resample's, and the records are the twin's on it
    want = Engine.h_adsb_frames(Engine.h_resample(x, 5, 3), 2)
    assert [f["pos"] for f in out["frames"]] == want[1].tolist() and len(want[1]) == 4
    got = [(f["msg"].hex().upper(), f["pos"] / out["fs"] * 1e6) for f in out["frames"]]
    assert [g[0] for g in got] == msgs
    assert all(abs(g[1] - t0) <= 0.5 for g, t0 in zip(got, t_us)), got          # within one chip


# ---- the loops, carries and reuses that need more tiles, more accepted starts or another rate than the tests above have
def test_4097_tiles(e):
    """Workgroup 0 of k_adsb_detect walks tiles 0, 1024, 2048, 3072 and 4096: survivors, none, survivors, none, survivors, so the prefetched
    registers, ms / surv, wcount and acc_s are reused after a tile that had work.  k_starts_gather walks tiles 2048 .. a second time, and
    k_starts_scan<int> carries into its second step at tile 4096."""
    S = DETECT_TILE
    tiles = 4 * DETECT_GRID_CAP + 1
    assert tiles == SCAN_STEP + 1 and tiles > 2 * LS_GRID_CAP
    n = (tiles - 1) * S + 600
    at = [5, 2 * DETECT_GRID_CAP * S + 7, (tiles - 1) * S - 300, (tiles - 1) * S + 3, n - 240]
    x = np.zeros(n, np.complex64)           # zeros fail the strict preamble test: the twin stays quick
    for p, m in zip(at, (A.IDENT, A.POS_EVEN, A.VELOCITY, A.POS_ODD, A.IDENT)):
        x[p:p + 240] = A.chips_of(m)
    msg, pos, meta, score, count = check(e, x, 1)
    assert pos.tolist() == at and count == 5


def test_more_accepted_starts_than_one_pass_of_the_list_kernels(e):
    k = LIST_PASS + 5                        # k_adsb_keep and k_adsb_emit: four accepted starts a workgroup, LS_GRID_CAP workgroups
    at = [3 + 128 * i for i in range(k)]
    x = A.clean(3 + 128 * k + 5, 1, [(A.ALL_CALL, p) for p in at])
    want = check(e, x, 1, max_frames=k + 10)
    assert want[4] == k and want[1].tolist() == at
    cut = check(e, x, 1, max_frames=LIST_PASS - 2)      # the rank cut falls inside the second pass of k_adsb_emit
    assert cut[4] == k and cut[1].tolist() == at[:LIST_PASS - 2]


@pytest.mark.parametrize("spc", [1, 2, 4, 6, 7, 8])
def test_dense_survivors_at_every_rate(e, spc):
    """ratio 0 at every rate: the survivor list fills the aliased ms, the second compaction takes four passes, and at spc 8 the LDS images
    are at their full size.  At spc 8 the frame at 700 runs into the one at 2500 and is reported at no start (tests/test_adsb_golden.py)."""
    x = A.dense_capture(spc)
    assert len(x) == DETECT_TILE + 240 * spc + 600
    want = check(e, x, spc, ratio=0.0, max_frames=512)
    ref = A.numpy_frames(x, spc, ratio=0.0, max_frames=512)
    assert all(same_bytes(w, r) for w, r in zip(want[:4], ref[:4])) and want[4] == ref[4]
    for q in (700,) * (spc < 8) + (2500, DETECT_TILE - 5):
        assert np.any(np.abs(want[1] - q) < spc), (q, want[1])


def test_window_of_two_tiles_with_exactly_its_reach(e):
    """A windowed call whose last tile has c starts, from a buffer that ends with the window's reach: the zeros the kernel stages behind
    it enter no sum that a start of the tile reads (the header comment of k_adsb_detect)."""
    x, p, spc = A.two_tile_window_capture(), A.TWO_TILE_P, 8
    n = len(x)
    whole = check(e, x, spc)
    assert whole[1].tolist() == [p, p + 240 * spc + 100]
    for c in A.TWO_TILE_EXTRA:
        s_begin = p - 4066 - c
        for s_end, at in ((p, []), (p + 1, [p])):
            lo, hi = A.reach(s_begin, s_end, spc, n)
            assert hi - lo == DETECT_TILE + c + 1919 + (s_end - p)
            part = check(e, x[lo:hi], spc, buf_index0=lo, n_capture=n, s_begin=s_begin, s_end=s_end)
            assert part[1].tolist() == at and part[4] == len(at), (c, s_end)
            inside = (whole[1] >= s_begin) & (whole[1] < s_end)
            for a, b in zip(part[:4], whole[:4]):
                assert same_bytes(a, b[inside]), (c, s_end)


@pytest.mark.parametrize("spc", [1, 3, 8])
@pytest.mark.parametrize("msg", [A.IDENT, A.ALL_CALL], ids=["long", "short"])
def test_frames_that_end_with_the_capture(e, spc, msg):
    x, p = A.ending_capture(spc, msg)        # the capture ends five samples into the second tile
    assert check(e, x, spc)[1].tolist() == [p]
    short = check(e, x[:-1], spc)
    ref = A.numpy_frames(x[:-1], spc)
    assert all(same_bytes(s, r) for s, r in zip(short[:4], ref[:4])) and short[4] == ref[4]
    assert p not in short[1].tolist() and short[1].tolist() == ([p - 1] if spc == 8 else [])


def test_every_downlink_format(e):
    x, accepted = A.every_format_capture()
    first = (A.ADDRESS + 7 * np.arange(1000)).astype(np.uint32)
    last = (A.ADDRESS - 7 * np.arange(999, -1, -1)).astype(np.uint32)
    for icao in ([A.ADDRESS], first, last):
        msg, pos, meta, score, count = check(e, x, 1, icao=icao)
        assert pos.tolist() == accepted and count == 9 and [int(w) >> 16 for w in meta] == list(A.REPORTED_DF)
    msg, pos, meta, score, count = check(e, x, 1)
    assert count == 3 and [int(w) >> 16 for w in meta] == [11, 17, 18]
    assert check(e, x, 1, icao=first[1:])[4] == 3


@pytest.mark.parametrize("spc", [4, 8])
def test_equal_scores_across_a_tile_boundary(e, spc):
    """spc starts with bit-equal scores on both sides of a tile boundary: k_adsb_keep walks up to spc - 1 neighbours on either side."""
    p = DETECT_TILE - spc // 2
    x, _ = A.same_score_starts(spc, p)
    assert check(e, x, spc)[1].tolist() == [p]
    assert check(e, x, spc, s_begin=p + 1)[4] == 0
    assert check(e, x, spc, s_begin=p + spc - 1)[4] == 0
    assert check(e, x, spc, s_end=p)[4] == 0
    assert check(e, x, spc, ratio=0.0)[1].tolist() == [p]


def test_one_workgroup_walks_dense_tiles_back_to_back(e):
    """ratio 0, spc 2: tiles 0, 1024 and 2048 are the first workgroup's, and each holds noise, so every one of them fills the survivor
    list, acc_s and the wavefront counts behind a tile that filled them too, fuller (4096 survivors, then about 2300, then about 1000):
    what a tile leaves behind its own count must not reach the next one's list.  Everything between is zero and passes no preamble."""
    S, cap, spc = DETECT_TILE, DETECT_GRID_CAP, 2
    n = 2 * cap * S + 1100 + 240 * spc
    x = np.zeros(n, np.complex64)
    at = []
    for k, (lo, hi, p, m) in enumerate(((0, S + 700, 700, A.IDENT), (cap * S - 300, cap * S + 2300, cap * S + 1500, A.ALL_CALL),
                                        (2 * cap * S + 100, n, 2 * cap * S + 300, A.VELOCITY))):
        x[lo:hi] = A.synth(hi - lo, spc, [(m, p - lo, 10.0, 0.5 + k)], seed=[89, k])
        at.append(p)
    stats = {}
    A.numpy_frames(x[:S + 240 * spc], spc, ratio=0.0, s_end=S - 2 * spc + 1, stats=stats)
    assert stats["survivors"] == S                                   # every start of tile 0
    want = check(e, x, spc, ratio=0.0, max_frames=512)
    assert set(at) <= set(want[1].tolist())

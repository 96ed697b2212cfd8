"""The decoders for batches on the GPU (include/pss.h, "decoders for batches"): pss_morse_text and pss_ax25_frames against their host twins
frame by frame, pss_real_normalise against NumPy's float32 expression, the one-call entries against the composition of the separate calls,
and decode_morse_batch / decode_aprs_batch / formats.decode_recording against what the reference returned for the recordings of
tests/golden/decode_batch.npz.  Every comparison is equality of bytes or bit patterns (NaN = NaN)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import decode_cases as S
import gpu_util as G
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import decoders as D
from pyspecsdr_amd import formats as F
from pyspecsdr_amd import signal_processing as SP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097)     # 4096: the most pulses the kernel keeps in LDS (MT_STAGE), 4097: one more
# pss_morse_text: hipLaunchKernelGGL(k_morse_text, dim3(n_frames < MT_GRID_MAX ? n_frames : MT_GRID_MAX), dim3(256), ...), one workgroup per frame
MT_GRID_MAX = 4096
# pss_ax25_frames: groups = (n_rows + 3) / 4; dim3(groups < AX_GRID_MAX ? groups : AX_GRID_MAX), dim3(256): one wavefront per row, four per workgroup
AX_GRID_MAX = 2048
# pss_real_normalise: dim3(n_rows < RN_GRID_MAX ? n_rows : RN_GRID_MAX), dim3(256): one workgroup per row
RN_GRID_MAX = 8192
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "decode_batch.npz"))


@pytest.fixture(scope="module")
def old():
    return np.load(os.path.join(ROOT, "tests", "golden", "decoders.npz"))


# ---- 1. pss_morse_text against pss_h_morse_decode ---------------------------------------------------------------------------------------------

def edges(lengths, gaps, lead_fall=False, trail_rise=False, start=5):
    """rise / fall index lists of pulses with these lengths and the gaps between them; a fall before the first rise / a rise behind the last fall"""
    rise, fall, t = [], [], start
    for i, ln in enumerate(lengths):
        rise.append(t)
        t += int(ln)
        fall.append(t)
        if i < len(gaps):
            t += int(gaps[i])
    if lead_fall:
        fall = [start - 3] + fall
    if trail_rise:
        rise = rise + [t + 4]
    return np.array(rise, np.int32), np.array(fall, np.int32)


def host_morse(rise, fall, fs):
    """-> (pulses, text bytes, timing float64[3]) of the host twin; pulses -2: it returns PSS_E_ARG (edges that do not alternate)"""
    lib = L.load()
    cap = 4 * (len(rise) + 2) + 16
    text, tm = C.create_string_buffer(cap), np.zeros(3)
    r = lib.pss_h_morse_decode(rise.ctypes.data, len(rise), fall.ctypes.data, len(fall), float(fs), text, cap, tm.ctypes.data)
    if r < 0:
        return -2, b"", np.zeros(3)
    return D._n_gaps(rise, fall) + 1, text.raw[:r], tm


def run_morse_text(frames, fs, cap=None, text_cap=None, counts=None):
    """frames: list of (rise, fall).  -> text uint8 [nf][text_cap], len, timing, pulses; sentinel rows either side of every output stay."""
    e = G.engine()
    nf = len(frames)
    cap = max([1] + [max(len(r), len(f)) for r, f in frames]) if cap is None else cap
    rise, fall = np.full((nf, cap), -77, np.int32), np.full((nf, cap), -77, np.int32)
    cnt = np.zeros((nf, 2), np.int32)
    for k, (r, f) in enumerate(frames):
        rise[k, :min(len(r), cap)], fall[k, :min(len(f), cap)] = r[:cap], f[:cap]
        cnt[k] = len(r), len(f)
    if counts is not None:
        cnt = np.asarray(counts, np.int32)
    text_cap = 2 * cap if text_cap is None else text_cap
    d_text = torch.full((nf + 2, text_cap), 0xAB, dtype=torch.uint8, device="cuda")
    d_len, d_np = torch.full((nf + 2,), -99, dtype=torch.int32, device="cuda"), torch.full((nf + 2,), -99, dtype=torch.int32, device="cuda")
    d_tm = torch.full((nf + 2, 3), -99.0, dtype=torch.float64, device="cuda")
    e.morse_text(G.dev(rise), G.dev(fall), G.dev(cnt), nf, cap, fs, d_text[1:], d_len[1:], d_tm[1:], d_np[1:], text_cap=text_cap)
    e.sync()
    text, ln, tm, pulses = G.host(d_text), G.host(d_len), G.host(d_tm), G.host(d_np)
    for a, s in ((text, 0xAB), (ln, -99), (tm, -99.0), (pulses, -99)):
        assert (a[0] == s).all() and (a[-1] == s).all(), "a sentinel either side of the output was overwritten"
    return text[1:-1], ln[1:-1], tm[1:-1], pulses[1:-1]


def same_as_host(frames, fs, got, text_cap=None):
    text, ln, tm, pulses = got
    for k, (r, f) in enumerate(frames):
        hp, ht, htm = host_morse(r, f, fs)
        assert pulses[k] == hp, (k, pulses[k], hp)
        assert ln[k] == len(ht), (k, ln[k], len(ht))
        keep = len(ht) if text_cap is None else min(len(ht), text_cap)
        assert text[k, :keep].tobytes() == ht[:keep], (k, text[k, :keep].tobytes(), ht)
        assert not text[k, keep:].any(), (k, "bytes behind the text are zero")
        assert np.array_equal(tm[k].view(np.uint64), htm.view(np.uint64)), (k, tm[k], htm)


def family(name, n, rng):
    """-> (lengths, gaps) of n pulses"""
    if name == "two":              # two lengths with jitter; letter and word gaps among the element gaps
        ln = rng.choice([40, 120], n) + rng.integers(-3, 4, n)
        gp = rng.choice([40, 130, 300], max(n - 1, 0), p=[0.6, 0.3, 0.1]) + rng.integers(-3, 4, max(n - 1, 0))
    elif name == "equal":
        ln, gp = np.full(n, 57), rng.choice([57, 180, 420], max(n - 1, 0))
    elif name == "small":          # lengths from {1, 2, 3, 4}: ties between splits
        ln, gp = rng.integers(1, 5, n), rng.integers(1, 12, max(n - 1, 0))
    elif name == "geometric":      # noise-like
        ln, gp = rng.geometric(0.3, n), rng.geometric(0.2, max(n - 1, 0))
    elif name == "distinct":       # every length another: the most candidate splits a frame of this many pulses can have
        ln, gp = rng.permutation(n) + 1, rng.integers(1, 9, max(n - 1, 0))
    else:
        raise ValueError(name)
    return ln, gp


FAMILIES = ("two", "equal", "small", "geometric", "distinct")


@pytest.fixture(scope="module")
def morse_frames():
    rng = np.random.default_rng(4242)
    frames = []
    for name in FAMILIES:
        for n in COUNTS:
            ln, gp = family(name, n, rng)
            for lead in (False, True):
                for trail in (False, True):
                    frames.append(edges(ln, gp, lead, trail))
    frames.append(edges(rng.permutation(300) + 1, rng.integers(1, 40, 299)))    # all lengths distinct inside n = 60 000
    assert frames[-1][1][-1] < 60000
    return frames


@pytest.mark.parametrize("fs", [48000.0, 22050.0])
def test_morse_text_equals_the_host_twin_on_every_family_and_count(morse_frames, fs):
    assert len(morse_frames) == len(FAMILIES) * len(COUNTS) * 4 + 1
    same_as_host(morse_frames, fs, run_morse_text(morse_frames, fs))


def keyed(symbols, dot=10, dash=30):
    """letters (strings of . and -) separated by letter gaps; ' ' = a word gap"""
    ln, gp = [], []
    for s in symbols:
        if s == " ":
            gp[-1] = 8 * dot
            continue
        for ch in s:
            ln.append(dot if ch == "." else dash)
            gp.append(dot)
        gp[-1] = 4 * dot
    return ln, gp[:-1]


def test_morse_text_table_prosign_long_letters_and_word_gaps():
    table = [".-", "-...", "-.-.", "-..", ".", "..-.", "--.", "....", "..", ".---", "-.-", ".-..", "--", "-.", "---", ".--.", "--.-", ".-.", "...",
             "-", "..-", "...-", ".--", "-..-", "-.--", "--..", ".----", "..---", "...--", "....-", ".....", "-....", "--...", "---..", "----.",
             "-----", "--..--", ".-.-.-", "..--..", "-..-.", "-....-", "-.--.", "-.--.-", ".-...", "---...", "-.-.-.", "-...-", ".-.-.", ".-..-.",
             "...-..-", ".--.-.", "..--.-", "...---..."]
    texts = 'ABCDEFGHIJKLMNOPQRSTUVWXYZ1234567890,.?/-()&:;=+"$@_'
    frames, want = [], []
    frames.append(edges(*keyed(table)))
    want.append(texts + "SOS")
    frames.append(edges(*keyed(["...---...", " ", "...", "---", "...", " ", "...---..", "...---....", "-" * 9, "." * 10, "-.-" * 4, "...---..."]), True, True))
    want.append("SOS SOS ?????SOS")
    frames.append(edges(*keyed(["-.-.", "--.-", " ", "-.-.", "--.-", " ", "-..", ".", " ", "-.-"])))
    want.append("CQ CQ DE K")
    frames.append(edges(*keyed(["." * 40 + "-"])))                                  # one letter of 41 elements
    want.append("?")
    frames.append(edges(*keyed(["....-.", "......", "-", "--------", "---------"])))   # symbols of table length that are not in the table
    want.append("??T??")
    got = run_morse_text(frames, 48000.0)
    same_as_host(frames, 48000.0, got)
    for k, w in enumerate(want):
        assert got[0][k, :got[1][k]].tobytes().decode("ascii") == w, k


def test_morse_text_truncated_lists_text_cap_and_edges_that_do_not_alternate():
    rng = np.random.default_rng(7)
    frames = [edges(*family("two", 30, rng)) for _ in range(6)] + [edges(*keyed(["...", "---", "..."]))]
    cap = 32
    counts = [[len(r), len(f)] for r, f in frames]
    counts[1], counts[2], counts[3] = [cap + 1, cap], [cap, cap + 1], [40000, 40000]          # truncated edge lists
    text, ln, tm, pulses = run_morse_text(frames, 48000.0, cap=cap, counts=counts)
    assert pulses[1] == pulses[2] == pulses[3] == -1
    for k in (1, 2, 3):
        assert ln[k] == 0 and not text[k].any() and not tm[k].any()
    keep = [0, 4, 5, 6]
    same_as_host([frames[k] for k in keep], 48000.0, (text[keep], ln[keep], tm[keep], pulses[keep]))
    # a text buffer shorter than the text: the true length, a truncated prefix
    for text_cap in (0, 1, 5):
        got = run_morse_text(frames, 48000.0, text_cap=text_cap)
        assert (got[1] > text_cap).any() and (got[1] >= 3).all()
        same_as_host(frames, 48000.0, got, text_cap=text_cap)
    # edges that do not alternate (two rises more than falls): the host twin refuses them, the device marks them
    r, f = frames[0]
    bad = (np.concatenate([r, [r[-1] + 500, r[-1] + 900]]).astype(np.int32), f)
    text, ln, tm, pulses = run_morse_text([frames[4], bad, frames[5]], 48000.0)
    assert host_morse(*bad, 48000.0)[0] == -2 and pulses[1] == -2 and ln[1] == 0 and not text[1].any() and not tm[1].any()
    same_as_host([frames[4], frames[5]], 48000.0, (text[[0, 2]], ln[[0, 2]], tm[[0, 2]], pulses[[0, 2]]))
    # no rise, no fall, one of each in the wrong order: the reference's early returns
    z = np.zeros(0, np.int32)
    empties = [(z, z), (np.array([5], np.int32), z), (z, np.array([5], np.int32)), (np.array([9], np.int32), np.array([5], np.int32))]
    text, ln, tm, pulses = run_morse_text(empties, 48000.0)
    assert not pulses.any() and not ln.any() and not tm.any() and not text.any()
    same_as_host(empties, 48000.0, (text, ln, tm, pulses))


@pytest.mark.parametrize("nf", [1, 3, 70, MT_GRID_MAX + 1])
def test_morse_text_batch_sizes_and_one_frame_past_the_grid_cap(nf):
    rng = np.random.default_rng(nf)
    kinds = [edges(*family(name, n, rng), lead, trail) for name, n, lead, trail in
             (("two", 12, False, True), ("small", 9, True, False), ("equal", 5, False, False), ("geometric", 20, True, True),
              ("distinct", 7, False, False), ("two", 1, False, False), ("two", 0, False, False))]
    frames = [kinds[(k * 5 + k // 7) % len(kinds)] for k in range(nf)]
    text, ln, tm, pulses = run_morse_text(frames, 48000.0)
    ref = [host_morse(r, f, 48000.0) for r, f in kinds]
    for k in range(nf):
        hp, ht, htm = ref[(k * 5 + k // 7) % len(kinds)]
        assert pulses[k] == hp and ln[k] == len(ht) and text[k, :ln[k]].tobytes() == ht and not text[k, ln[k]:].any(), k
        assert np.array_equal(tm[k].view(np.uint64), htm.view(np.uint64)), k


# ---- 2. pss_ax25_frames against pss_h_ax25_frame ----------------------------------------------------------------------------------------------

def host_ax25(row):
    """-> None (no packet) or the packet's bytes"""
    lib = L.load()
    row = np.ascontiguousarray(row, np.uint8)
    cap = len(row) // 8 + 64
    out, n = C.create_string_buffer(cap), C.c_long(0)
    r = lib.pss_h_ax25_frame(row.ctypes.data, len(row), out, cap, C.byref(n))
    assert r in (0, 1)
    return out.raw[:n.value] if r == 1 else None


def run_ax25(rows, out_cap=None):
    e = G.engine()
    rows = np.ascontiguousarray(rows, np.uint8)
    nr, nb = rows.shape
    out_cap = nb // 8 + 64 if out_cap is None else out_cap
    d_out = torch.full((nr + 2, out_cap), 0xAB, dtype=torch.uint8, device="cuda")
    d_len = torch.full((nr + 2,), -99, dtype=torch.int32, device="cuda")
    e.ax25_frames(G.dev(rows) if rows.size else None, nr, nb, out_cap, d_out[1:] if out_cap else None, d_len[1:])
    e.sync()
    out, ln = G.host(d_out), G.host(d_len)
    assert (out[0] == 0xAB).all() and (out[-1] == 0xAB).all() and ln[0] == ln[-1] == -99
    return out[1:-1], ln[1:-1]


def ax_same_as_host(rows, got, out_cap=None):
    out, ln = got
    n_packets = 0
    for k, row in enumerate(rows):
        h = host_ax25(row)
        if h is None:
            assert ln[k] == -1 and (out[k] == 0xAB).all(), (k, ln[k])
            continue
        n_packets += 1
        keep = len(h) if out_cap is None else min(len(h), out_cap)
        assert ln[k] == len(h) and out[k, :keep].tobytes() == h[:keep], (k, ln[k], out[k, :keep].tobytes(), h)
        assert (out[k, keep:] == 0xAB).all(), (k, "bytes behind the packet are not written")
    return n_packets


def test_ax25_frames_on_the_fixture_streams(old):
    lens, outs = old["ax_len"], json.loads(str(old["ax_out"]))
    assert len(lens) == len(outs) == 40
    off = np.concatenate([[0], np.cumsum(lens)])
    for k in range(40):
        row = old["ax_bits"][off[k]:off[k + 1]]
        out, ln = run_ax25(row[None, :])
        if outs[k] == "<None>":
            assert ln[0] == -1, k
        else:
            assert out[0, :ln[0]].tobytes() == outs[k].encode("latin-1"), k
        ax_same_as_host(row[None, :], (out, ln))


@pytest.mark.parametrize("nb", [0, 7, 8, 15, 16, 63, 64, 65, 225, 599, 4097])
def test_ax25_frames_random_rows_and_planted_flags(nb):
    rng = np.random.default_rng(1000 + nb)
    rows = []
    for density in (0.5, 0.8, 0.95):
        for plant in (None, (0,), (nb - 8,), (nb - 9,), (nb // 2,), (0, nb // 2), (3, nb - 9), (0, nb // 3, 2 * nb // 3)):
            for rep in range(3):
                row = (rng.random(nb) < density).astype(np.uint8)
                for p in plant or ():
                    if 0 <= p and p + 8 <= nb:
                        row[p:p + 8] = FLAG
                rows.append(row)
    frame = S.ax25_bits("APRS", "N0CALL", rng.integers(0, 256, 12))              # information bytes of every value, NULs and 0xff included
    for lead in (0, 1, 7, 30):
        if lead + len(frame) + 9 <= nb:
            row = np.zeros(nb, np.uint8)
            row[lead:lead + len(frame)] = frame
            rows.append(row)
    rows = np.array(rows, np.uint8).reshape(len(rows), nb)
    n_packets = ax_same_as_host(rows, run_ax25(rows))
    if nb >= 225:
        assert n_packets >= 10, "rows that decode are among the cases"


def test_ax25_frames_stuffing_at_the_end_kept_stream_flags_and_frame_sizes():
    rng = np.random.default_rng(31)
    rows = []
    body = lambda nbytes: [int(b) for b in np.tile([1, 0, 1, 0, 0, 1, 0, 0], nbytes)]     # no run of five ones: nothing is stuffed
    pad = lambda bits: np.concatenate([np.array(bits, np.uint8), np.zeros(225 - len(bits), np.uint8)])
    for k in range(-3, 12):           # five ones whose last one sits k bits in front of the loop's bound n_bits - 7 ...
        row = pad(FLAG + body(15))
        p = 225 - 7 - k - 5
        row[p:p + 5] = 1
        rows.append(row.copy())       # ... and a zero behind them: the stuffed zero, dropped
        row[p + 6] = 1
        rows.append(row.copy())       # ... with a one behind that zero
        row[p + 5] = 1
        rows.append(row)              # six ones and more: nothing is dropped
    for nbytes in (12, 13, 14, 15, 16, 17):     # 13 bytes: no packet; 14: addresses alone; 15: the PID is dropped; 16: one information byte
        rows.append(pad(FLAG + body(nbytes) + FLAG))
    # an end flag that exists only in the kept stream: 0 11111 [0 dropped] 1 0
    for nbytes in (14, 20):
        rows.append(pad(FLAG + body(nbytes) + [0, 1, 1, 1, 1, 1, 0, 1, 0] + [1, 0, 1, 1, 0, 0, 1, 0] * 3))
    # addresses made of the characters str.strip() removes, and of none of them
    for fill in (0x20, 0x09, 0x1c, 0x41, 0x00, 0x7f):
        by = [fill << 1] * 6 + [0x60] + [(0x41 << 1)] + [fill << 1] * 5 + [0x61, 0x03, 0xF0, 0x00, 0xff, 0x41]
        bits, st, ones = [(v >> j) & 1 for v in by for j in range(8)], [], 0
        for b in bits:
            st.append(b)
            ones = ones + 1 if b else 0
            if ones == 5:
                st.append(0)
                ones = 0
        rows.append(pad(FLAG + st + FLAG))
    # values other than 0 / 1: kept as ones, never part of a raw flag
    row = rows[-1].copy()
    row[row == 1] = rng.integers(1, 256, int((row == 1).sum()))
    row[:8] = FLAG
    rows.append(row)
    rows = np.array(rows)
    assert ax_same_as_host(rows, run_ax25(rows)) >= 20
    lens = {len(h) for h in map(host_ax25, rows) if h is not None}
    assert min(lens) < 14 < max(lens)              # stripped addresses, and packets with an information field


@pytest.mark.parametrize("nbytes", [13, 14, 15, 16])
def test_ax25_frames_without_an_end_flag_the_frame_runs_up_to_the_bound(nbytes):
    """no end flag: the kept bits up to i < n_bits - 7 are the frame — row lengths either side of a whole number of bytes"""
    for extra in range(0, 9):
        nb = 8 + 8 * nbytes + 7 + extra - 4
        row = np.zeros(nb, np.uint8)
        row[:8] = FLAG
        row[8:] = np.tile([1, 0, 1, 0, 0, 1, 0, 0], nbytes + 2)[:nb - 8]
        rows = np.stack([row, row, row])
        got = run_ax25(rows)
        ax_same_as_host(rows, got)
        kept_bytes = (nb - 7 - 8) // 8
        assert (got[1] >= 0).all() == (kept_bytes >= 14), (nb, kept_bytes)


@pytest.mark.parametrize("out_cap", [0, 1, 9, 15])    # the shortest packet below is 16 bytes: every one of them is cut
def test_ax25_frames_out_cap_too_small(out_cap):
    rng = np.random.default_rng(5)
    rows = []
    for k in range(6):
        frame = S.ax25_bits("DST%d" % k, "SRC%d" % k, rng.integers(32, 127, 5 + 3 * k))
        row = np.zeros(400, np.uint8)
        row[k:k + len(frame)] = frame
        rows.append(row)
    rows.append(np.zeros(400, np.uint8))
    rows = np.array(rows)
    got = run_ax25(rows, out_cap=out_cap)
    assert (got[1][:6] > out_cap).all() and got[1][6] == -1
    ax_same_as_host(rows, got, out_cap=out_cap)


@pytest.mark.parametrize("nr", [1, 3, 4 * AX_GRID_MAX + 1])
def test_ax25_frames_row_counts_and_one_row_past_the_grid_cap(nr):
    rng = np.random.default_rng(nr)
    kinds = []
    for k in range(7):
        row = (rng.random(300) < 0.6).astype(np.uint8)         # the longest frame below is 226 bits
        if k % 3 != 2:
            frame = S.ax25_bits("APRS", "N%dCALL" % k, rng.integers(32, 127, 4 + k))
            row[k:k + len(frame)] = frame
        kinds.append(row)
    pick = lambda k: (k * 3 + k // 7) % len(kinds)
    rows = np.array([kinds[pick(k)] for k in range(nr)])
    out, ln = run_ax25(rows)
    ref = [host_ax25(r) for r in kinds]
    assert sum(r is not None for r in ref) >= 4
    for k in range(nr):
        h = ref[pick(k)]
        if h is None:
            assert ln[k] == -1, k
        else:
            assert ln[k] == len(h) and out[k, :ln[k]].tobytes() == h, k


# ---- 3. pss_real_normalise against NumPy's float32 expression ------------------------------------------------------------------------------------

def same_bits_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def run_real_normalise(x):
    e = G.engine()
    nr, n = x.shape
    d_out = torch.full((nr + 2, n), -99.0, dtype=torch.float64, device="cuda")
    e.real_normalise(G.dev(x), nr, n, d_out[1:])
    e.sync()
    out = G.host(d_out)
    assert (out[0] == -99.0).all() and (out[-1] == -99.0).all(), "a sentinel either side of the output was overwritten"
    return out[1:-1]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 24000])
def test_real_normalise_equals_numpys_float32_division(n):
    rng = np.random.default_rng(n)
    x = ((rng.standard_normal((12, n)) + 1j * rng.standard_normal((12, n))) * np.exp2(rng.integers(-30, 20, (12, 1)))).astype(np.complex64)
    v = x.view(np.float32).reshape(12, n, 2)
    v[1] = 0.0                                   # a row of zeros: 0 / 0
    v[2, n // 2, 0] = np.nan                     # NaN in the real part: the maximum, hence the whole row
    v[3, n - 1, 0] = np.inf
    v[4, 0, 0] = -np.inf
    v[5, :, 1] = np.nan                          # NaN in the imaginary parts only: no effect
    v[6, n // 3, 1] = np.inf
    v[7, ::2, 0] = -0.0                          # -0 keeps its sign (behind a non-zero maximum when n > 1)
    v[8, :, 0] = np.float32(1e-39) * rng.integers(1, 9, n).astype(np.float32)      # subnormal reals
    v[9, :, 0] = np.abs(v[9, :, 0])
    v[9, n // 2, 0] = np.float32(3.0e38)         # quotients that underflow
    v[10] = (rng.integers(-32768, 32768, (n, 2)) / 32768.0).astype(np.float32)     # ADC codes
    got, want = run_real_normalise(x), S.real_normalise_np(x)
    for k in range(12):
        assert same_bits_nan(got[k], want[k]), (k, got[k][:4], want[k][:4])
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and not np.isnan(got[5]).any()
    if n > 2:
        assert np.signbit(got[7, 0]) and got[7, 0] == 0.0


def test_real_normalise_one_row_past_the_grid_cap():
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((RN_GRID_MAX + 1, 3)) + 1j * rng.standard_normal((RN_GRID_MAX + 1, 3))).astype(np.complex64)
    assert same_bits_nan(run_real_normalise(x), S.real_normalise_np(x))


# ---- 4. the one-call entries are the composition of the separate calls, work buffers included --------------------------------------------

def test_decode_morse_batch_call_equals_edges_then_text():
    e = G.engine()
    rng = np.random.default_rng(12)
    c = S.case("morse_60")
    x = np.concatenate([S.frames(c)[:5], (0.08 * (rng.standard_normal((2, c.n)) + 1j * rng.standard_normal((2, c.n)))).astype(np.complex64),
                        np.zeros((1, c.n), np.complex64)])
    nf, n, cap = len(x), c.n, c.n // 2 + 1
    d_iq = G.dev(x)
    res = []
    for one_call in (True, False):
        bufs = [torch.full(shape, fill, dtype=dt, device="cuda") for shape, fill, dt in
                (((nf, cap), -5, torch.int32), ((nf, cap), -5, torch.int32), ((nf, 2), -5, torch.int32), ((nf, 2 * cap), 0xAB, torch.uint8),
                 ((nf,), -5, torch.int32), ((nf, 3), -5.0, torch.float64), ((nf,), -5, torch.int32))]
        rise, fall, cnt, text, ln, tm, pulses = bufs
        if one_call:
            e.decode_morse_batch(d_iq, nf, n, c.fs, rise, fall, cnt, text, ln, tm, pulses)
        else:
            e.morse_edges(d_iq, nf, n, cap, rise, fall, cnt)
            e.morse_text(rise, fall, cnt, nf, cap, c.fs, text, ln, tm, pulses)
        e.sync()
        res.append([G.host(b) for b in bufs])
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes()
    rise, fall, cnt, text, ln, tm, pulses = res[0]
    assert (pulses[:5] > 0).any() and pulses[5] > 1000 and pulses[7] == 0, "keyed buffers, noise at the cut, silence"
    frames = [(rise[k, :cnt[k, 0]], fall[k, :cnt[k, 1]]) for k in range(nf)]      # noise: device against the host twin only
    same_as_host(frames, c.fs, (text, ln, tm, pulses))


def test_decode_aprs_batch_call_equals_normalise_bits_frames():
    e = G.engine()
    c = S.case("aprs_9600")
    x = S.frames(c)[:9]
    nr, n, nb = len(x), c.n, e.afsk_n_bits(c.n, c.fs)
    out_cap = nb // 8 + 64
    d_iq = G.dev(x)
    res = []
    for one_call in (True, False):
        bufs = [torch.full(shape, fill, dtype=dt, device="cuda") for shape, fill, dt in
                (((nr, n), -5.0, torch.float64), ((nr, nb), 0xAB, torch.uint8), ((nr, out_cap), 0xAB, torch.uint8), ((nr,), -5, torch.int32))]
        audio, bits, out, ln = bufs
        if one_call:
            e.decode_aprs_batch(d_iq, nr, n, c.fs, audio, bits, out_cap, out, ln)
        else:
            e.real_normalise(d_iq, nr, n, audio)
            e.afsk_bits(audio, nr, n, c.fs, bits)
            e.ax25_frames(bits, nr, nb, out_cap, out, ln)
        e.sync()
        res.append([G.host(b) for b in bufs])
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes()
    assert same_bits_nan(res[0][0], S.real_normalise_np(x)) and (res[0][3] > 0).any()


def test_one_call_entries_refuse_bad_arguments_and_accept_empty_batches():
    e = G.engine()
    lib, t = e.lib, torch.zeros(64, dtype=torch.int32, device="cuda")
    p = t.data_ptr()
    assert lib.pss_decode_morse_batch(e.h, None, 0, 16, 48000.0, -20.0, 9, None, None, None, 18, None, None, None, None) == 0
    assert lib.pss_decode_aprs_batch(e.h, None, 0, 16, 48000.0, None, None, 5, None, None, 8, None, None) == 0
    assert lib.pss_morse_text(e.h, None, None, None, 0, 4, 48000.0, 8, None, None, None, None) == 0
    assert lib.pss_ax25_frames(e.h, None, 0, 8, 8, None, None) == 0 and lib.pss_real_normalise(e.h, None, 0, 8, None) == 0
    for r in (lib.pss_morse_text(e.h, p, p, p, 1, 4, 0.0, 8, p, p, p, p), lib.pss_morse_text(e.h, p, p, p, -1, 4, 48000.0, 8, p, p, p, p),
              lib.pss_morse_text(e.h, p, p, None, 1, 4, 48000.0, 8, p, p, p, p), lib.pss_morse_text(e.h, p, p, p, 1, -1, 48000.0, 8, p, p, p, p),
              lib.pss_ax25_frames(e.h, p, 1, -1, 8, p, p), lib.pss_ax25_frames(e.h, p, 1, 8, 8, p, None), lib.pss_ax25_frames(e.h, None, 1, 8, 8, p, p),
              lib.pss_real_normalise(e.h, p, 1, -1, p), lib.pss_real_normalise(e.h, p, 1, 4, None),
              lib.pss_decode_morse_batch(e.h, p, 1, 0, 48000.0, -20.0, 9, p, p, p, 18, p, p, p, p),
              lib.pss_decode_aprs_batch(e.h, p, 1, 16, 800.0, None, None, 5, p, p, 8, p, p)):
        assert r == L.PSS_E_ARG and lib.pss_last_error(e.h)
    e.sync()


# ---- 5. the fixture recordings, each as one batch ----------------------------------------------------------------------------------------------

def timing_bits(tm):
    return np.array([float(tm["dot"]), float(tm["dash"]), float(tm["gap"])]).view(np.uint64)


@pytest.mark.parametrize("c", S.MORSE, ids=lambda c: c.name)
def test_decode_morse_batch_equals_the_reference_and_the_drop_in(gold, c):
    x = S.frames(c)
    got = D.decode_morse_batch(x, c.fs)
    assert len(got) == len(x)
    for f, (text, tm) in enumerate(got):
        assert text == str(gold[f"text_{c.name}"][f]), (f, text)
        assert np.array_equal(timing_bits(tm), gold[f"timing_{c.name}"][f]), f
        one_text, one_tm = D.decode_morse(x[f], c.fs)
        assert text == one_text and set(tm) == set(one_tm) == {"dot", "dash", "gap"}
        for k in tm:
            assert type(tm[k]) is type(one_tm[k]) and np.float64(tm[k]).tobytes() == np.float64(one_tm[k]).tobytes(), (f, k)


@pytest.mark.parametrize("scipy_tables", [True, False], ids=["scipy_tables", "own_designers"])
@pytest.mark.parametrize("c", S.APRS, ids=lambda c: c.name)
def test_decode_aprs_batch_equals_the_reference(gold, c, scipy_tables, monkeypatch):
    monkeypatch.setattr(SP, "USE_SCIPY_DESIGNS", scipy_tables)
    e = G.engine()
    x = S.frames(c)
    want = json.loads(str(gold[f"packets_{c.name}"]))
    assert D.decode_aprs_batch(x, c.fs) == want
    packets, bits = D._aprs_batch_dev(e, G.dev(x), len(x), c.n, c.fs, want_bits=True)
    assert packets == want and bits.tobytes() == gold[f"bits_{c.name}"].tobytes()
    for f in range(0, len(x), 7):       # the drop-in on the float32 quotients (their maximum is 1: its own float64 division changes nothing)
        assert D.decode_aprs(S.real_normalise_np(x[f]), c.fs) == want[f], f


@pytest.mark.parametrize("name", ["morse_60", "aprs_9600"])
def test_decode_recording_from_npy_and_cs16_files(gold, name, tmp_path):
    c = S.case(name)
    codes = S.codes(c)
    np.save(tmp_path / "rec.npy", S.frames(c).reshape(-1))
    np.concatenate([codes, codes[:c.n // 2]]).astype("<i2").tofile(tmp_path / "rec.cs16")     # half a buffer more: the tail is dropped
    a = F.decode_recording(F.load_iq_recording(str(tmp_path / "rec.npy")), c.fs, c.kind, chunk_frames=5)
    b = F.decode_recording(F.load_iq_codes(str(tmp_path / "rec.cs16"), "cs16"), c.fs, c.kind, chunk_frames=5, codes_format="cs16")
    assert len(a) == len(b) == len(S.frames(c))
    if c.kind == "aprs":
        assert a == b == json.loads(str(gold[f"packets_{name}"]))
        return
    for f, ((ta, ma), (tb, mb)) in enumerate(zip(a, b)):
        assert ta == tb == str(gold[f"text_{name}"][f]), f
        assert np.array_equal(timing_bits(ma), gold[f"timing_{name}"][f]) and np.array_equal(timing_bits(mb), gold[f"timing_{name}"][f]), f
    assert F.decode_recording(np.zeros(c.n - 1, np.complex64), c.fs, c.kind) == []


def test_the_morse_goldens_of_decoders_npz_as_batches_of_three(old):
    for tag in old["mtags"]:
        x, fs = old[f"m_iq_{tag}"], float(old[f"m_fs_{tag}"])
        got = D.decode_morse_batch(np.stack([x, x, x]), fs)
        assert len(got) == 3 and got[0][0] == got[1][0] == got[2][0]
        for text, tm in got:
            bits = timing_bits(tm)
            assert np.array_equal(bits, timing_bits(got[0][1]))
            if tag == "noise":           # the reference's own answer depends on its random draw: the host twin is the statement
                rise, fall = D.morse_edges(x)
                one_text, one_tm = D.morse_from_edges(rise, fall, fs)
                assert text == one_text and len(text) >= 1 and np.array_equal(bits, timing_bits(one_tm))
                continue
            assert text == str(old[f"m_text_{tag}"]), tag
            assert np.array_equal(bits, old[f"m_timing_{tag}"].view(np.uint64)), (tag, tm)

"""The packet-radio receiver's host side — pss_packet_plan, pss_packet_default_tones, pss_h_packet_front, pss_h_packet_frames,
formats.h_packet_rows — against tests/golden/packet.npz and the NumPy statement of the rules in tests/packet_cases.py — no GPU.  The
arithmetic is the project's own (pyspecsdr_amd/csrc/pss_packet.h), so the truth is made outside it: NumPy builds the frames, the audio and
the FM rows and restates the front, the flag test, the walk with its clock tracking, the check and the one-record rule; the twin must agree
with it z for z and record for record, and hand back exactly the frames sent.  tests/test_gpu_packet.py (-m gpu) holds the kernels to the
twins on every byte.  tests/packet_host.cpp runs the header alone under AddressSanitizer and UBSan.

The discriminator in front of the four chains is pss_ais.h's: the project's model of NumPy's float32 arctan2, which the AIS and FM-mono
suites hold to NumPy where NumPy runs the modelled routine.  Here it is held to the float64 angle within float32 rounding, and the statement
of everything behind it starts from the twin's own d (pss_h_ais_front with the one-tap pulse returns it)."""
import os
import re
import subprocess

import numpy as np
import pytest

import packet_cases as P
from bytes_util import same_bytes
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
GOLD = np.load(os.path.join(HERE, "golden", "packet.npz"))
NAMES = [str(n) for n in GOLD["names"]]
SYMBOLS = ("pss_packet_plan", "pss_packet_default_tones", "pss_packet_front", "pss_h_packet_front", "pss_packet_frames", "pss_h_packet_frames")
WHAT = ("msg", "len", "row", "pos", "score")
ONE = np.array([1.0])


def p(a):
    return None if a is None else a.ctypes.data


def both(z, **kw):
    """The twin and the NumPy statement agree on every record -> the twin's result."""
    twin = E.h_packet_frames(z, **kw)
    ref = P.numpy_frames(z, **kw)
    for t, r, what in zip(twin[:5], ref[:5], WHAT):
        assert same_bytes(t, r), (what, t, r)
    assert twin[5] == ref[5]
    return twin


def frames_of(r):
    return [bytes(m[:n]) for m, n in zip(r[0], r[1])]


def same_z(a, b):
    """Every bit, a NaN for a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def front_both(x, space_gain=1.0):
    """The twin's z equals the statement's on every sample -> z."""
    z = E.h_packet_front(x, space_gain=space_gain)
    assert same_z(z, P.numpy_front(x, space_gain=space_gain, d=E.h_ais_front(x, pulse=ONE)))
    return z


def test_symbols_are_declared_exported_and_in_the_table():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    units = __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS
    assert ("pss_packet.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]) in units
    for name in ("packet_plan", "packet_default_tones", "packet_front", "h_packet_front", "packet_frames", "h_packet_frames"):
        assert callable(getattr(E, name))
    for name in ("ax25_decode", "aprs_tnc2", "aprs_decode", "aprs_tracks", "packet_rows", "h_packet_rows", "packet_recording"):
        assert callable(getattr(F, name))
    # the calls the receiver leaves as they are
    for name in ("pss_ax25_frames", "pss_afsk_bits", "pss_decode_aprs_batch"):
        assert name in L._SIGS
    assert callable(E.decode_aprs_batch)


def test_goldens_are_the_synthesisers():
    assert NAMES == sorted(P.CASES)
    for name in NAMES:
        c = P.CASES[name]
        assert P.row_crc32(P.case_iq(name)) == int(GOLD[name + "/crc32"][0]), name
        assert int(GOLD[name + "/seed"][0]) == c["seed"]
        sent = [f for fs, _, _ in c["bursts"] for f in fs]
        assert bytes(GOLD[name + "/sent"]) == b"".join(sent) and GOLD[name + "/sent_len"].tolist() == [len(f) for f in sent]


def test_the_fixtures_cover_what_they_are_there_for():
    c = P.CASES
    assert sorted({c[n]["clock"] for n in ("clock_1000", "clock_1004", "clock_0996")}) == [0.996, 1.0, 1.004]
    assert c["preemph_gain_100"]["preemph"] and c["preemph_gain_035"]["preemph"] and (c["preemph_gain_100"]["gain"], c["preemph_gain_035"]["gain"]) == (1.0, 0.35)
    assert [lead for _, _, lead in c["two_flags"]["bursts"]] == [2, 2] and c["clock_1000"]["bursts"][0][2] == 20
    assert len(c["shared_flag"]["bursts"]) == 1 and len(c["shared_flag"]["bursts"][0][0]) == 3
    assert sorted(len(f) for f in c["short_and_long"]["expect"]) == [17, 330]
    long = c["short_and_long"]["expect"][1]
    assert long[72:328] == bytes([0xFF]) * 256 and F.ax25_decode(long[:-2])["path"][-1]["call"] == "DIGI8"
    assert len(F.ax25_decode(c["ten_addresses"]["expect"][0][:-2])["path"]) == 8
    lower, one, flipped, good = [f for fs, _, _ in c["refused"]["bursts"] for f in fs]
    assert P.crc16(lower[:-2]) == int.from_bytes(lower[-2:], "little") and not P.address_ok(lower) and b"n0call" in bytes(b >> 1 for b in lower[:14])
    assert P.crc16(one[:-2]) == int.from_bytes(one[-2:], "little") and not P.address_ok(one) and one[6] & 1
    assert P.crc16(flipped[:-2]) != int.from_bytes(flipped[-2:], "little") and P.address_ok(flipped)
    assert c["refused"]["expect"] == [good] and c["nan_inside"]["nan_at"] is not None and c["all_zero"]["expect"] == []
    assert all(c[n]["snr"] == 15.0 for n in NAMES if n != "all_zero")


@pytest.mark.parametrize("name", NAMES)
def test_twin_is_the_numpy_statement_and_the_golden_and_recovers_the_frames(name):
    c = P.CASES[name]
    z = front_both(P.case_iq(name), c["gain"])
    r = both(z)
    for got, what in zip(r[:5], WHAT):
        assert same_bytes(got, GOLD[name + "/" + what]), what
    # every frame sent that the fixture expects comes out, and no other record does
    assert frames_of(r) == c["expect"] and r[5] == len(c["expect"])
    if name == "all_zero":
        assert z.tobytes() == np.zeros(len(z), np.float32).tobytes()              # den == 0: +0 everywhere, no candidate
    if name == "nan_inside":
        lo, hi = c["nan_at"]
        assert np.all(np.isnan(z[lo - 10:hi + 12])) and not np.isnan(z[lo - 11]) and not np.isnan(z[hi + 12])      # d[hi] reads x[hi - 1]


def test_discriminator_and_front_against_float64():
    """d = angle(x[i] conj(x[i - 1])) in float64: the twin's float32 discriminator stays within 3 float32 roundings of the product's parts
    and one of the angle (each 2^-24 relative on a signal of about unit amplitude, |d| <= pi: below 1e-5, the AIS suite's bound).  z behind
    it is a ratio in [-1, 1] of sums of 22 such samples: the same statement in float64 throughout stays within 1e-4 wherever the energy is
    not tiny."""
    x = P.case_iq("clock_1000")[:8000]
    z64 = x.astype(np.complex128)
    d64 = np.concatenate([[0.0], np.angle(z64[1:] * np.conj(z64[:-1]))])
    d = E.h_ais_front(x, pulse=ONE)
    assert d.dtype == np.float32 and np.max(np.abs(d - d64)) < 1e-5
    assert np.max(np.abs(P.numpy_disc(x) - d64)) < 1e-5
    t = P.tones()
    pad = np.concatenate([np.zeros(11), d64, np.zeros(10)])
    c = np.stack([np.convolve(pad, t[j][::-1], mode="valid") for j in range(4)])
    em, es = c[0] ** 2 + c[1] ** 2, c[2] ** 2 + c[3] ** 2
    for g in (1.0, 0.35):
        ref = (g * es - em) / (g * es + em)
        z = E.h_packet_front(x, space_gain=g)
        assert z.dtype == np.float32 and z.shape == (8000,) and np.max(np.abs(z - ref)[em + es > 1e-2]) < 1e-4
        assert np.all(np.abs(z) <= 1.0)
    # windows with exactly their halo give the row's bytes; another table is the caller's to hand in
    whole = E.h_packet_front(x)
    for i0, i1 in ((0, 1), (1, 2), (11, 12), (12, 700), (7990, 8000), (0, 8000)):
        lo, hi = P.front_span(i0, i1, 8000)
        assert same_bytes(E.h_packet_front(x[lo:hi], buf_index0=lo, n_row=8000, i_begin=i0, i_end=i1), whole[i0:i1])
    swapped = P.tones()[[2, 3, 0, 1]]
    assert same_bytes(E.h_packet_front(x, tones=swapped), -whole + np.float32(0.0)) or np.max(np.abs(E.h_packet_front(x, tones=swapped) + whole)) < 1e-6


SENSITIVITY = [(1.0, 41), (1.004, 42), (0.996, 43)]


@pytest.mark.parametrize("clock,seed", SENSITIVITY)
def test_eight_of_eight_at_15_db(clock, seed):
    x, frames = P.many_frames(8, 15.0, clock, seed)
    r = E.h_packet_frames(E.h_packet_front(x))
    assert frames_of(r) == frames and r[5] == 8


def test_noise_alone_reports_nothing():
    rng = np.random.default_rng(7)
    n = 1_000_000
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    z = E.h_packet_front(x)
    assert E.h_packet_frames(z)[5] == 0
    stats = {}
    assert P.numpy_frames(z[:200000], stats=stats)[5] == 0
    s = stats["strobes"]
    print(f"noise alone: {stats['survivors']} starts in 200000 pass the flag test; their walks read {np.mean(s):.0f} strobes on average, {max(s)} at most; no frame")


# ---- crafted rows: z given outright ----------------------------------------------------------------------------------------------------------------
GOOD = P.with_crc(P.FRAMES["status"])


def test_the_closing_look_ahead_on_the_last_sample():
    z, s, n = P.edge_row()
    r = both(z, q_min=0.5)
    assert frames_of(r) == [P.SHORT_FRAME] and r[3].tolist() == [s] and r[4].tolist() == [1.0] and r[2].tolist() == [0]
    assert both(z[:-1], q_min=0.5)[5] == 0                                                  # one sample shorter: the look-ahead lies outside
    assert both(z, q_min=1.0)[5] == 1 and both(z, q_min=np.nextafter(np.float32(1), np.float32(2)))[5] == 0
    # without q_min the 22 starts of the flag's cell pass, and those the tracking has pulled to the centre or in front of it close inside
    # the row; the centred one scores highest
    stats = {}
    assert P.numpy_frames(z, stats=stats)[5] == 1 and stats["survivors"] > 22
    r0 = both(z)
    assert frames_of(r0) == [P.SHORT_FRAME] and r0[3].tolist() == [s] and r0[4].tolist() == [1.0]
    # the first start of the row: one sample earlier the level in front would lie outside
    z2, s2, n2 = P.edge_row(at=P.BACK + 5)
    assert both(z2[5:], q_min=0.5)[3].tolist() == [P.BACK] and both(z2[6:], q_min=0.5)[5] == 0


def test_equal_scores_keep_the_earlier_start_and_a_higher_score_wins():
    bits = P.burst_bits(GOOD, lead=1, tail=1)
    z = P.direct_z(P.BACK + 11 + P.SPB * len(bits) + 50, [(bits, P.BACK + 11)])
    r = both(z)
    s = P.BACK + 11
    assert frames_of(r) == [GOOD] and r[3].tolist() == [s - 11] and r[4].tolist() == [1.0]       # 22 starts, equal scores: the earliest
    assert both(z, s_begin=s)[5] == 0 and both(z, s_end=s - 11)[5] == 0 and both(z, s_end=s - 10)[3].tolist() == [s - 11]
    z2 = z.copy()
    z2[s + 3 + P.SPB * np.arange(-1, 8)] *= 1.5
    assert both(z2)[3].tolist() == [s + 3]


def test_max_frames_keeps_the_true_count():
    c = P.CASES["shared_flag"]
    z = E.h_packet_front(P.case_iq("shared_flag"))
    full = both(z)
    assert full[5] == 3
    for mf in (0, 2):
        cut = both(z, max_frames=mf)
        assert cut[5] == 3 and len(cut[3]) == mf and same_bytes(cut[0], full[0][:mf])
    lib = L.load()
    msg, ln, rw = np.full((3, 332), 0xA5, np.uint8), np.full(3, -7, np.int32), np.full(3, -7, np.int32)
    pos, score, count = np.full(3, -7, np.int64), np.full(3, -7, np.float32), np.zeros(1, np.int32)
    assert lib.pss_h_packet_frames(p(z), 1, len(z), len(z), 0, len(z), 0, len(z), 0.0, p(msg), p(ln), p(rw), p(pos), p(score), p(count), 2) == 0
    assert count[0] == 3 and np.all(msg[2:] == 0xA5) and ln[2] == -7 and rw[2] == -7 and pos[2] == -7 and score[2] == -7
    assert same_bytes(msg[:2], full[0][:2]) and c["expect"][0] == bytes(msg[0, :ln[0]])


def test_rows_do_not_run_into_each_other():
    """Two rows back to back in memory: row 0's frame would only close inside row 1's samples."""
    bits = P.burst_bits(GOOD, lead=1, tail=1)
    n = P.BACK + 11 + P.SPB * (len(bits) - 1) - 40                                          # the closing flag's last two bits lie in row 1
    flat = P.direct_z(2 * n, [(bits, P.BACK + 11)])
    assert frames_of(both(flat)) == [GOOD]
    assert both(flat.reshape(2, n))[5] == 0
    rows = np.stack([P.direct_z(n + 200, [(bits, P.BACK + 11 + 7 * k)]) for k in range(4)])
    r = both(rows)
    assert r[2].tolist() == [0, 1, 2, 3] and r[3].tolist() == [P.BACK + 7 * k for k in range(4)]


def windows_row():
    a, b, c = (P.burst_bits(P.with_crc(P.FRAMES[k]), lead=2, tail=1) for k in ("status", "short", "compressed"))
    n = 40000
    z = P.direct_z(n, [(a, 60), (b, 2 * 4096 - 8 * P.SPB + 3), (c, 12500)])       # b's second flag: its cell lies across the boundary of two detect tiles
    return z


def test_windows_do_not_change_a_byte():
    z = windows_row()
    n = len(z)
    whole = both(z)
    starts = whole[3].tolist()
    assert len(starts) == 3 and starts[1] == 2 * 4096 + 3 - 11
    for cuts in ([starts[0] + 1, starts[1] - 3, 8192, starts[1] + 12, 12500], [starts[0], starts[1], starts[2], n - 1], [1, 2, 3]):
        edges = [0] + cuts + [n]
        parts = []
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = P.reach(s0, s1, n)
            parts.append(both(z[lo:hi], buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
        for i in range(5):
            assert same_bytes(np.concatenate([q[i] for q in parts]), whole[i]), (cuts, i)
        assert sum(q[5] for q in parts) == whole[5]


def test_dense_survivors_and_no_frame():
    z, starts = P.dense_row(40)
    stats = {}
    assert P.numpy_frames(z, stats=stats)[5] == 0 and stats["survivors"] == 22 * 40 and E.h_packet_frames(z)[5] == 0


def test_non_finite_samples():
    bits = P.burst_bits(GOOD, lead=1, tail=1)
    z = P.direct_z(P.BACK + P.SPB * len(bits) + 50, [(bits, P.BACK, 0.25, 1.0)])
    s = P.BACK
    assert frames_of(both(z, q_min=0.5)) == [GOOD]
    for at, v in ((s - 22, np.nan), (s + 44, np.nan), (s + 300, np.inf), (s + 301, -np.inf), (s + 500, np.nan)):
        y = z.copy()
        y[at] = v
        both(y, q_min=0.5)
        both(y)
    y = z.copy()
    y[s + 44] = np.nan                                                                       # a strobe of the flag: a NaN is no level and no score
    assert both(y, q_min=0.5)[5] == 0


def test_refusals_by_message():
    lib = L.load()
    bits = P.burst_bits(GOOD, lead=1, tail=1)
    z = P.direct_z(P.BACK + P.SPB * len(bits) + 50, [(bits, P.BACK, 0.25, 1.0)])
    n = len(z)
    msg, ln, rw, pos, score = np.zeros((4, 332), np.uint8), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(4, np.float32)
    count = np.full(1, -7, np.int32)
    ok = dict(z=p(z), n_rows=1, stride=n, n_buf=n, index0=0, n_row=n, s0=0, s1=n, q_min=0.5, msg=p(msg), len=p(ln), row=p(rw), pos=p(pos), score=p(score),
              count=p(count), max_frames=4)
    order = ("z", "n_rows", "stride", "n_buf", "index0", "n_row", "s0", "s1", "q_min", "msg", "len", "row", "pos", "score", "count", "max_frames")

    def refused(why, **kw):
        a = dict(ok, **kw)
        r = lib.pss_h_packet_frames(*[a[k] for k in order])
        assert r == L.PSS_E_ARG and lib.pss_last_error(None).decode() == "pss_packet_frames: " + why, lib.pss_last_error(None).decode()
        assert count[0] == -7 and not msg.any()
    refused("n_rows outside [1, 2^20]", n_rows=0)
    refused("z_stride < n_buf", stride=n - 1)
    refused("s_end < s_begin", s0=10, s1=9)
    refused("the window does not lie inside the row", s1=n + 1)
    refused("the buffer does not lie inside the row", n_row=n - 1)
    refused("the buffer does not lie inside the row", index0=-1)
    reach = "the buffer does not cover the window's reach (21 starts either side, 22 samples back, 73203 samples forward)"
    refused(reach, n_row=1000000, s1=60)                                                  # the window's last start reads 73 203 ahead
    refused(reach, index0=50, n_row=n + 50, s0=92, s1=93)                                 # and 22 + 21 back
    refused("a window of more than 2^30 starts", n_row=1 << 40, s1=(1 << 30) + 1)
    refused("more than 2^31 starts in the rows of one call", n_rows=3, n_row=1 << 40, s1=1 << 30)
    refused("n_row outside [0, 2^60]", n_row=-1)
    refused("n_row outside [0, 2^60]", n_row=(1 << 60) + 1)
    refused("q_min must be finite and >= 0", q_min=-0.5)
    refused("q_min must be finite and >= 0", q_min=float("nan"))
    refused("q_min must be finite and >= 0", q_min=float("inf"))
    refused("max_frames < 0", max_frames=-1)
    refused("null buffer", count=None)
    refused("null buffer", z=None)
    refused("null buffer", msg=None)
    refused("a misaligned pointer", z=p(z) + 2)
    refused("a misaligned pointer", pos=p(pos) + 4)
    refused("a misaligned pointer", count=p(count) + 2)
    assert lib.pss_h_packet_frames(*[ok[k] for k in order]) == 0 and count[0] == 1 and pos[0] == P.BACK
    assert E.h_packet_frames(z, s_begin=7, s_end=7)[5] == 0                                # an empty window is no refusal
    # the front
    x = np.ones(100, np.complex64)
    out = np.full(100, -7, np.float32)
    t = E.packet_default_tones()
    okf = dict(iq=p(x), n_rows=1, stride=100, n_buf=100, index0=0, n_row=100, tones=p(t), gain=1.0, i0=0, i1=100, z=p(out), z_stride=100)
    orderf = ("iq", "n_rows", "stride", "n_buf", "index0", "n_row", "tones", "gain", "i0", "i1", "z", "z_stride")

    def refused_f(why, **kw):
        a = dict(okf, **kw)
        r = lib.pss_h_packet_front(*[a[k] for k in orderf])
        assert r == L.PSS_E_ARG and lib.pss_last_error(None).decode() == "pss_packet_front: " + why, lib.pss_last_error(None).decode()
        assert np.all(out == -7)
    refused_f("n_rows < 1", n_rows=0)
    refused_f("x_stride < n_buf", stride=99)
    refused_f("the buffer does not lie inside the row", n_row=99)
    refused_f("i_end < i_begin", i0=5, i1=4)
    refused_f("the window does not lie inside the row", i1=101)
    refused_f("z_stride < i_end - i_begin", z_stride=99)
    refused_f("a window of more than 2^30 samples", n_row=1 << 40, i1=(1 << 30) + 1, z_stride=1 << 31)
    refused_f("n_row outside [0, 2^60]", n_row=-1)
    refused_f("null tone table", tones=None)
    for v in (np.inf, np.nan):
        bad = t.copy()
        bad[2, 7] = v
        refused_f("a table entry that is not finite", tones=p(bad))
    for g in (0.0, -1.0, float("inf"), float("nan")):
        refused_f("space_gain must be finite and > 0", gain=g)
    halo = "the buffer does not cover the window's halo (12 samples in front, 10 behind)"
    refused_f(halo, n_row=200, i1=96)
    refused_f(halo, index0=10, n_row=110, i0=21, i1=30)
    refused_f("null buffer", iq=None)
    refused_f("null buffer", z=None)
    refused_f("a misaligned pointer", iq=p(x) + 4)
    refused_f("a misaligned pointer", z=p(out) + 2)
    assert lib.pss_h_packet_front(*[okf[k] for k in orderf]) == 0 and out.tobytes() == np.zeros(100, np.float32).tobytes()   # a bare carrier: den == 0
    with pytest.raises(ValueError, match="tones"):
        E.h_packet_front(x, tones=np.zeros((4, 21)))


def test_rows_through_formats_are_the_twins_records():
    """formats.h_packet_rows: front, frames and the decoders in one call; the GPU suite holds formats.packet_rows and packet_recording to it."""
    x = np.stack([P.case_iq("clock_1004"), P.case_iq("clock_0996")])
    recs = F.h_packet_rows(x)
    assert [(r["row"], r["msg"]) for r in sorted(recs, key=lambda r: (r["row"], r["pos"]))] == \
        [(row, f[:-2]) for row, name in enumerate(("clock_1004", "clock_0996")) for f in P.CASES[name]["expect"]]
    assert [r["pos"] for r in recs] == sorted(r["pos"] for r in recs)
    first = next(r for r in recs if r["row"] == 0)
    assert first["tnc2"] == "N0CALL-7>APRS,WIDE1-1*,WIDE2-2:" + P.POSITION.decode() and first["aprs"]["symbol"] == "/-"
    assert F.h_packet_rows(np.zeros((2, 0), np.complex64)) == [] and F.h_packet_rows(np.zeros(5000, np.complex64)) == []
    pre = P.case_iq("preemph_gain_035")
    assert [r["msg"] for r in F.h_packet_rows(pre, space_gain=0.35)] == [f[:-2] for f in P.CASES["preemph_gain_035"]["expect"]]


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/packet_host.cpp: pss_packet.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "packet_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "packet_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "packet_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

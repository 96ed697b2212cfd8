"""The AIS receiver's host side — pss_ais_plan, pss_ais_default_pulse, pss_ais_crc, pss_h_ais_front, pss_h_ais_frames, formats.ais_decode /
ais_nmea / ais_tracks — against the published vector, tests/golden/ais.npz and the NumPy statement of the rules in tests/ais_cases.py — no
GPU.  The arithmetic is the project's own (pyspecsdr_amd/csrc/pss_ais.h), so the truth is made outside it: NumPy builds the bursts from
the message fields and restates the candidate, walk, check and one-record rules; the twin must agree with it record for record, and hand
back exactly the injected frames.  tests/test_gpu_ais.py (-m gpu) holds the kernels to the twins on every byte.  tests/ais_host.cpp runs
the header alone under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest

import ais_cases as A
from bytes_util import same_bytes
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
GOLD = np.load(os.path.join(HERE, "golden", "ais.npz"))
NAMES = [str(n) for n in GOLD["names"]]
SYMBOLS = ("pss_ais_plan", "pss_ais_default_pulse", "pss_ais_crc", "pss_ais_front", "pss_h_ais_front", "pss_ais_frames", "pss_h_ais_frames")
WHAT = ("msg", "len", "row", "pos", "score")


def p(a):
    return None if a is None else a.ctypes.data


def both(y, **kw):
    """The twin and the NumPy statement agree on every record -> the twin's result."""
    twin = E.h_ais_frames(y, **kw)
    ref = A.numpy_frames(y, **kw)
    for t, r, what in zip(twin[:5], ref[:5], WHAT):
        assert same_bytes(t, r), (what, t, r)
    assert twin[5] == ref[5]
    return twin


def frames_of(r):
    return [bytes(m[:n]) for m, n in zip(r[0], r[1])]


def test_symbols_are_declared_exported_and_in_the_table():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    units = __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS
    assert ("pss_ais.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]) in units
    for name in ("ais_plan", "ais_default_pulse", "ais_crc", "ais_front", "h_ais_front", "ais_frames", "h_ais_frames"):
        assert callable(getattr(E, name))
    for name in ("ais_decode", "ais_nmea", "ais_tracks", "ais_recording"):
        assert callable(getattr(F, name))


def test_plan():
    assert E.ais_plan(2.4e6) == (50, 1, 1) and E.ais_plan(250e3) == (5, 24, 25) and E.ais_plan(48000) == (1, 1, 1)
    assert E.ais_plan(2.048e6) == (42, 63, 64) and E.ais_plan(20e6) == (204, 306, 625)
    for fs, why in ((48000.5, "fs must be an integer number of Hz"), (float("nan"), "fs must be an integer number of Hz"),
                    (47999.0, "fs must be at least 48 000"), (-1.0, "fs must be at least 48 000"),
                    (1000003.0, "48 000 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take")):
        with pytest.raises(ValueError, match="^" + re.escape("pss_ais: " + why)):
            E.ais_plan(fs)


def test_crc():
    assert E.ais_crc(b"123456789") == 0x906E == A.crc16(b"123456789")
    assert E.ais_crc(b"123456789" + (0x906E).to_bytes(2, "little")) ^ 0xFFFF == 0xF0B8       # the register's residue
    assert E.ais_crc(b"") == 0 and E.ais_crc(np.frombuffer(A.VECTOR, np.uint8)) == A.crc16(A.VECTOR)
    assert L.load().pss_ais_crc(None, 3) == 0xFFFFFFFF


def test_default_pulse_against_numpy():
    for span in range(1, 13):
        g = E.ais_default_pulse(span)
        assert len(g) == 5 * span + 1
        k = np.arange(len(g)) - (len(g) - 1) / 2
        w = np.exp(-(2 * np.pi ** 2 / np.log(2)) * 0.16 * (k / 5.0) ** 2)
        w = w / w.sum()
        assert np.all(np.abs(g - w) <= 1e-15 * np.abs(w)), span
    with pytest.raises(ValueError):
        E.ais_default_pulse(0)
    with pytest.raises(ValueError):
        E.ais_default_pulse(13)


def test_the_published_vector_both_directions():
    d = F.ais_decode(A.VECTOR)
    assert (d["type"], d["repeat"], d["mmsi"], d["status"], d["heading"], d["second"]) == (1, 0, 477553000, 5, 181, 15)
    assert abs(d["lon"] - -122.345833) < 1e-6 and abs(d["lat"] - 47.582833) < 1e-6 and d["course"] == 51.0 and d["speed"] == 0.0
    assert F.ais_nmea(A.VECTOR, "B") == [A.VECTOR_SENTENCE] and A.VECTOR_SENTENCE.endswith("*5C")
    assert F.ais_payload([A.VECTOR_SENTENCE]) == A.VECTOR
    assert F.ais_decode(A.with_crc(A.VECTOR)) == d                                     # the check bytes behind it change nothing
    with pytest.raises(ValueError):
        F.ais_payload([A.VECTOR_SENTENCE[:-1] + "D"])
    # the same fields built here give the same bits up to the radio status
    assert A.SHIPS[0][:18] == A.VECTOR[:18]
    na = F.ais_decode(A.type1(1, 181.0, 91.0, speed=102.3, course=360.0, turn=-128))
    assert (na["lon"], na["lat"], na["speed"], na["course"], na["heading"], na["turn"]) == (None, None, None, None, None, None)


def test_type_5_from_fields_and_back_in_two_sentences():
    m = A.SHIPS[3]
    d = F.ais_decode(m)
    assert (d["type"], d["mmsi"], d["imo"], d["callsign"], d["name"], d["ship_type"]) == (5, 244660000, 9074729, "PBQR", "NOORDZEE", 70)
    assert (d["to_bow"], d["to_stern"], d["to_port"], d["to_starboard"], d["eta"], d["draught"], d["destination"]) == (100, 20, 8, 7, (5, 17, 6, 30), 6.4,
                                                                                                                      "ROTTERDAM")
    s = F.ais_nmea(m, "A", seq=3)
    assert len(s) == 2 and s[0].startswith("!AIVDM,2,1,3,A,") and s[1].startswith("!AIVDM,2,2,3,A,")
    assert len(s[0].split(",")[5]) == 56 and len(s[1].split(",")[5]) == 15 and s[0].split(",")[6][0] == "0" and s[1].split(",")[6][0] == "2"
    assert F.ais_payload(s) == m
    for sen in s:
        body, cs = sen[1:].split("*")
        x = 0
        for ch in body:
            x ^= ord(ch)
        assert "%02X" % x == cs


def test_other_types():
    d = F.ais_decode(A.SHIPS[2])
    assert (d["type"], d["mmsi"], d["speed"], d["course"], d["heading"], d["second"]) == (18, 338123456, 6.1, 271.0, None, 7)
    assert abs(d["lon"] - 4.2501) < 1e-6 and abs(d["lat"] - 51.9502) < 1e-6
    assert F.ais_decode(A.SHIPS[4]) == {"type": 24, "repeat": 0, "mmsi": 338123456, "part": 0, "name": "SEA BREEZE"}
    t4 = A.pack([(4, 6), (0, 2), (2320001, 30), (2026, 14), (10, 4), (20, 5), (8, 5), (44, 6), (3, 6), (1, 1), (round(-1.5 * 600000), 28),
                 (round(50.25 * 600000), 27), (0, 4), (0, 10), (0, 1), (0, 19)])
    d = F.ais_decode(t4)
    assert (d["year"], d["month"], d["day"], d["hour"], d["minute"], d["second"], d["lon"], d["lat"]) == (2026, 10, 20, 8, 44, 3, -1.5, 50.25)
    t21 = A.pack([(21, 6), (0, 2), (992351000, 30), (14, 5)] + A.sixbit("NORTH CARDINAL", 20) + [(1, 1), (round(2.0 * 600000), 28), (round(51.0 * 600000), 27),
                 (1, 9), (2, 9), (3, 6), (4, 6), (7, 4), (60, 6), (1, 1), (0, 8), (0, 1), (0, 1), (0, 1), (0, 1)])
    d = F.ais_decode(t21)
    assert (d["aid_type"], d["name"], d["lon"], d["lat"], d["to_bow"], d["to_starboard"], d["off_position"]) == (14, "NORTH CARDINAL", 2.0, 51.0, 1, 4, 1)
    assert F.ais_decode(A.pack([(27, 6), (1, 2), (5, 30), (0, 58)])) == {"type": 27, "repeat": 1, "mmsi": 5}
    assert F.ais_decode(A.SHIPS[3][:20]) == {"type": 5, "repeat": 0, "mmsi": 244660000}      # too short for its type


def test_tracks():
    recs = [dict(msg=A.SHIPS[2], pos=48000), dict(msg=A.SHIPS[0], pos=96000), dict(msg=A.SHIPS[4], pos=144000), dict(msg=A.SHIPS[3], pos=150000)]
    tr = F.ais_tracks(recs)
    assert [t["mmsi"] for t in tr] == [338123456, 477553000, 244660000]
    b, a, c = tr
    assert (b["name"], b["frames"], b["first"], b["last"], b["speed"], b["course"]) == ("SEA BREEZE", 2, 1.0, 3.0, 6.1, 271.0)
    assert abs(b["position"][0] - 51.9502) < 1e-6 and abs(a["position"][1] - -122.345833) < 1e-6
    assert (c["name"], c["callsign"], c["ship_type"], c["position"]) == ("NOORDZEE", "PBQR", 70, None)


def test_goldens_are_the_synthesisers():
    assert NAMES == sorted(A.CASES)
    for name in NAMES:
        assert A.capture_crc32(A.case_iq(name)) == int(GOLD[name + "/crc32"][0])


@pytest.mark.parametrize("name", NAMES)
def test_twin_is_the_numpy_statement_and_the_golden_and_recovers_the_frames(name):
    y = E.h_ais_front(A.case_iq(name))
    r = both(y)
    for got, what in zip(r[:5], WHAT):
        assert same_bytes(got, GOLD[name + "/" + what]), what
    sent = [A.with_crc(m) for m, _, _, _ in A.CASES[name][3]]
    assert frames_of(r) == sent and r[5] == len(sent)
    # each within a bit and a half of where it was put (the front's delay is zero: the pulse is centred)
    for q, (_, at, _, _) in zip(r[3].tolist(), A.CASES[name][3]):
        assert abs(q - (at + 5 * A.TRAINING + 2)) <= 7


def test_front_against_numpy_in_float64():
    """d = angle(x[i] conj(x[i - 1])), y = its convolution with the pulse, in float64: the twin's float32 discriminator stays within
    3 float32 roundings of the product's parts (each 2^-24 relative on a unit signal), one of the angle and one of y: below 1e-5."""
    x = A.case_iq("quiet")[:6000]
    for pulse in (None, np.array([1.0]), E.ais_default_pulse(12)):
        g = E.ais_default_pulse(2) if pulse is None else pulse
        z = x.astype(np.complex128)
        d = np.concatenate([[0.0], np.angle(z[1:] * np.conj(z[:-1]))])
        c = (len(g) - 1) // 2
        ref = np.convolve(np.concatenate([np.zeros(c), d, np.zeros(c)]), g[::-1], mode="valid")
        y = E.h_ais_front(x, pulse=pulse)
        assert y.dtype == np.float32 and y.shape == (6000,) and np.max(np.abs(y - ref)) < 1e-5
    # windows with exactly their halo give the row's bytes
    whole = E.h_ais_front(x)
    for i0, i1 in ((0, 1), (1, 2), (5, 6), (6, 700), (5990, 6000), (0, 6000)):
        lo, hi = max(0, i0 - 6), min(6000, i1 + 5)
        assert same_bytes(E.h_ais_front(x[lo:hi], buf_index0=lo, n_row=6000, i_begin=i0, i_end=i1), whole[i0:i1])


SENSITIVITY = [(off, seed) for off, seed in ((0.0, 21), (500.0, 22), (-500.0, 23))]


@pytest.mark.parametrize("off,seed", SENSITIVITY)
def test_twenty_of_twenty_at_15_db(off, seed):
    x, msgs = A.many_bursts(20, 15.0, off, seed)
    r = E.h_ais_frames(E.h_ais_front(x))
    assert frames_of(r) == msgs and r[5] == 20


def test_noise_alone_reports_nothing():
    rng = np.random.default_rng(7)
    n = 2_000_000
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    y = E.h_ais_front(x)
    stats = {}
    assert E.h_ais_frames(y)[5] == 0 and A.numpy_frames(y, stats=stats)[5] == 0
    print(f"noise alone: {stats['survivors']} starts in {n} pass the flag test, no frame")


# ---- crafted rows: levels at the strobes ---------------------------------------------------------------------------------------------------
GOOD = A.with_crc(A.SHIPS[0])
AT = 60


def row_of(bits, n=None, at=AT, **kw):
    n = at + 5 * len(bits) + 40 if n is None else n
    return A.direct_y(n, [(bits, at)], **kw)


def test_a_frame_at_the_strobes_and_its_rejections():
    s = A.flag_start(AT)
    good = A.burst_bits(GOOD)
    r = both(row_of(good))
    assert frames_of(r) == [GOOD] and r[3].tolist() == [s] and r[4].tolist() == [1.0]
    mid = A.stuff(A.wire_bits(GOOD))
    head = good[:A.TRAINING + 8]
    # 127 message bytes: 1032 bits with the check bytes, eight more than a frame holds
    assert both(row_of(A.burst_bits(A.with_crc(bytes(127)))))[5] == 0
    assert frames_of(both(row_of(A.burst_bits(A.long_frame())))) == [A.long_frame()]       # 1024 bits are accepted
    assert both(row_of(A.burst_bits(A.with_crc(A.SHIPS[0][:4]))))[5] == 0                   # 48 bits: below 56
    assert frames_of(both(row_of(A.burst_bits(A.with_crc(A.SHIPS[0][:5]))))) == [A.with_crc(A.SHIPS[0][:5])]   # 56 bits
    assert both(row_of(A.burst_bits(None, stuffed=mid + [0, 1, 0])))[5] == 0               # no multiple of 8
    assert both(row_of(head + mid + [0, 1, 1, 1, 1, 1, 1, 1, 0, 0]))[5] == 0               # seven ones
    for i in (0, 77, len(mid) - 1):
        flipped = A.wire_bits(GOOD)
        flipped[min(i, len(flipped) - 1)] ^= 1
        assert both(row_of(A.burst_bits(None, stuffed=A.stuff(flipped))))[5] == 0          # the check
    # the closing flag's last strobe is the row's last sample: accepted; one sample shorter: not
    last = AT + 5 * (len(good) - 1)
    assert frames_of(both(row_of(good, n=last + 1))) == [GOOD]
    assert both(row_of(good, n=last))[5] == 0


def test_five_ones_directly_before_the_closing_flag():
    for k in range(4096):
        frame = A.with_crc(A.SHIPS[0][:-2] + k.to_bytes(2, "big"))
        if frame[-1] >> 3 == 0x1F:
            break
    mid = A.stuff(A.wire_bits(frame))
    assert mid[-6:] == [1, 1, 1, 1, 1, 0]
    assert frames_of(both(row_of(A.burst_bits(frame)))) == [frame]


def test_threshold_follows_the_carrier_offset():
    good = A.burst_bits(GOOD)
    y = A.direct_y(AT + 5 * len(good) + 40, [(good, AT, 0.25, 0.75)], base=0.75)
    r = both(y)
    assert frames_of(r) == [GOOD] and r[4].tolist() == [0.25]


def test_equal_scores_keep_the_earlier_start():
    good = A.burst_bits(GOOD)
    s = A.flag_start(AT)
    y = row_of(good, hold=5)
    assert both(y)[3].tolist() == [s]
    for k in range(1, 5):
        assert both(y, s_begin=s + k)[5] == 0                                             # the earliest lies outside the window and still drops
        alone = both(row_of(good, at=AT + k, n=len(y)))                                    # every later alignment alone is accepted
        assert alone[3].tolist() == [s + k] and alone[4].tolist() == [1.0]
    assert both(y, s_end=s)[5] == 0 and both(y, s_end=s + 1)[3].tolist() == [s]
    z = y.copy()
    z[s + 2 + 5 * np.arange(-8, 8)] *= 1.5                                                # the third alignment stands farther from the threshold
    assert both(z)[3].tolist() == [s + 2]


def test_max_frames_keeps_the_true_count():
    y = E.h_ais_front(A.case_iq("quiet"))
    full = both(y)
    for mf in (0, full[5] - 1):
        cut = both(y, max_frames=mf)
        assert cut[5] == full[5] and len(cut[3]) == mf and same_bytes(cut[0], full[0][:mf])
    lib = L.load()
    k = full[5]
    msg, ln, rw = np.full((k, 128), 0xA5, np.uint8), np.full(k, -7, np.int32), np.full(k, -7, np.int32)
    pos, score, count = np.full(k, -7, np.int64), np.full(k, -7, np.float32), np.zeros(1, np.int32)
    assert lib.pss_h_ais_frames(p(y), 1, len(y), len(y), 0, len(y), 0, len(y), p(msg), p(ln), p(rw), p(pos), p(score), p(count), 2) == 0
    assert count[0] == k and np.all(msg[2:] == 0xA5) and np.all(ln[2:] == -7) and np.all(rw[2:] == -7) and np.all(pos[2:] == -7) and np.all(score[2:] == -7)
    assert same_bytes(msg[:2], full[0][:2])


def test_rows_do_not_run_into_each_other():
    """Two rows back to back in memory: row 0's last frame would only close inside row 1's samples."""
    good = A.burst_bits(GOOD)
    n = AT + 5 * (len(good) - 1) - 12                                                     # the closing flag's last three strobes lie in row 1
    flat = row_of(good, n=2 * n)
    assert frames_of(both(flat)) == [GOOD]                                                # as one row it closes
    assert both(flat.reshape(2, n))[5] == 0
    rows5 = np.stack([row_of(good, n=n + 100, at=AT + 7 * k) for k in range(5)])
    r = both(rows5)
    assert r[2].tolist() == [0, 1, 2, 3, 4] and r[3].tolist() == [A.flag_start(AT + 7 * k) for k in range(5)]


def windows_row():
    good, other = A.burst_bits(GOOD), A.burst_bits(A.with_crc(A.SHIPS[1]))
    n = 9000
    y = A.direct_y(n, [(good, 50), (other, 2000), (good, 4100 - 5 * A.TRAINING)], hold=5)
    y += A.direct_y(n, [(A.burst_bits(A.with_crc(A.SHIPS[2])), 6000)], hold=1)
    return y, [A.flag_start(50), A.flag_start(2000), 4100, A.flag_start(6000)]


def test_windows_do_not_change_a_byte():
    y, starts = windows_row()
    n = len(y)
    whole = both(y)
    assert whole[3].tolist() == starts
    for cuts in ([starts[0] + 1, starts[1] + 3, 4096, 4101, 6000], [starts[0], 4099, 4100, n - 1], [1, 2, 3]):
        edges = [0] + cuts + [n]
        parts = []
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = A.reach(s0, s1, n)
            parts.append(both(y[lo:hi], buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
        for i in range(5):
            assert same_bytes(np.concatenate([q[i] for q in parts]), whole[i]), (cuts, i)
        assert sum(q[5] for q in parts) == whole[5]


def test_dense_survivors_and_no_frame():
    y, starts = A.dense_row(300)
    stats = {}
    assert A.numpy_frames(y, stats=stats)[5] == 0 and stats["survivors"] == 300 and E.h_ais_frames(y)[5] == 0


def test_non_finite_samples():
    y = row_of(A.burst_bits(GOOD), hold=1)
    s = A.flag_start(AT)
    for at, v in ((s - 20, np.nan), (s + 10, np.nan), (s + 300, np.inf), (s - 40, -np.inf)):
        z = y.copy()
        z[at] = v
        both(z)
    z = y.copy()
    z[3] = np.nan                                                                          # in front of everything the start reads
    assert frames_of(both(z)) == [GOOD]


def test_refusals_by_message():
    lib = L.load()
    y = row_of(A.burst_bits(GOOD))
    n = len(y)
    msg, ln, rw, pos, score = np.zeros((4, 128), np.uint8), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(4, np.float32)
    count = np.full(1, -7, np.int32)
    ok = dict(y=p(y), n_rows=1, stride=n, n_buf=n, index0=0, n_row=n, s0=0, s1=n, msg=p(msg), len=p(ln), row=p(rw), pos=p(pos), score=p(score),
              count=p(count), max_frames=4)
    order = ("y", "n_rows", "stride", "n_buf", "index0", "n_row", "s0", "s1", "msg", "len", "row", "pos", "score", "count", "max_frames")

    def refused(why, **kw):
        a = dict(ok, **kw)
        r = lib.pss_h_ais_frames(*[a[k] for k in order])
        assert r == L.PSS_E_ARG and lib.pss_last_error(None).decode() == "pss_ais_frames: " + why, lib.pss_last_error(None).decode()
        assert count[0] == -7 and not msg.any()
    refused("n_rows outside [1, 2^20]", n_rows=0)
    refused("y_stride < n_buf", stride=n - 1)
    refused("s_end < s_begin", s0=10, s1=9)
    refused("the window does not lie inside the row", s1=n + 1)
    refused("the buffer does not lie inside the row", n_row=n - 1)
    refused("the buffer does not lie inside the row", index0=-1)
    reach = "the buffer does not cover the window's reach (4 starts either side, 45 samples back, 6221 samples forward)"
    refused(reach, n_row=100000, s1=60)                                                   # the window's last start reads 6221 ahead
    refused(reach, index0=50, n_row=n + 50, s0=98, s1=99)                                 # and 45 + 4 back
    refused("a window of more than 2^30 starts", n_row=1 << 40, s1=(1 << 30) + 1)
    refused("more than 2^31 starts in the rows of one call", n_rows=3, n_row=1 << 40, s1=1 << 30)
    refused("n_row outside [0, 2^60]", n_row=-1)
    refused("n_row outside [0, 2^60]", n_row=(1 << 60) + 1)
    refused("max_frames < 0", max_frames=-1)
    refused("null buffer", count=None)
    refused("null buffer", y=None)
    refused("null buffer", msg=None)
    refused("a misaligned pointer", y=p(y) + 2)
    refused("a misaligned pointer", pos=p(pos) + 4)
    refused("a misaligned pointer", count=p(count) + 2)
    assert lib.pss_h_ais_frames(*[ok[k] for k in order]) == 0 and count[0] == 1 and pos[0] == A.flag_start(AT)
    assert E.h_ais_frames(y, s_begin=7, s_end=7)[5] == 0                                   # an empty window is no refusal
    # the front
    x = np.ones(100, np.complex64)
    out = np.full(100, -7, np.float32)
    g = E.ais_default_pulse(2)
    okf = dict(iq=p(x), n_rows=1, stride=100, n_buf=100, index0=0, n_row=100, pulse=p(g), n_pulse=11, i0=0, i1=100, y=p(out), y_stride=100)
    orderf = ("iq", "n_rows", "stride", "n_buf", "index0", "n_row", "pulse", "n_pulse", "i0", "i1", "y", "y_stride")

    def refused_f(why, **kw):
        a = dict(okf, **kw)
        r = lib.pss_h_ais_front(*[a[k] for k in orderf])
        assert r == L.PSS_E_ARG and lib.pss_last_error(None).decode() == "pss_h_ais_front: " + why, lib.pss_last_error(None).decode()
        assert np.all(out == -7)
    refused_f("n_rows < 1", n_rows=0)
    refused_f("x_stride < n_buf", stride=99)
    refused_f("the buffer does not lie inside the row", n_row=99)
    refused_f("i_end < i_begin", i0=5, i1=4)
    refused_f("the window does not lie inside the row", i1=101)
    refused_f("y_stride < i_end - i_begin", y_stride=99)
    refused_f("a window of more than 2^30 samples", n_row=1 << 40, i1=(1 << 30) + 1, y_stride=1 << 31)
    refused_f("n_row outside [0, 2^60]", n_row=-1)
    refused_f("n_pulse must be odd and in [1, 65]", n_pulse=10)
    refused_f("n_pulse must be odd and in [1, 65]", n_pulse=67)
    refused_f("n_pulse must be odd and in [1, 65]", pulse=None)
    bad = g.copy()
    bad[3] = np.inf
    refused_f("a pulse tap that is not finite", pulse=p(bad))
    halo = "the buffer does not cover the window's halo ((P - 1) / 2 + 1 samples in front, (P - 1) / 2 behind)"
    refused_f(halo, n_row=200, i1=96)
    refused_f(halo, index0=10, n_row=110, i0=15, i1=20)
    refused_f("null buffer", iq=None)
    refused_f("null buffer", y=None)
    refused_f("a misaligned pointer", iq=p(x) + 4)
    refused_f("a misaligned pointer", y=p(out) + 2)
    assert lib.pss_h_ais_front(*[okf[k] for k in orderf]) == 0 and np.all(out == 0)


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/ais_host.cpp: pss_ais.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "ais_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "ais_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ais_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

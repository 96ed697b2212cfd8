"""The ADS-B receiver's host side — pss_adsb_plan, pss_adsb_crc, pss_h_adsb_frames, formats.adsb_decode / adsb_tracks — against the published
vectors, tests/golden/adsb.npz and the NumPy statement of the rules in tests/adsb_cases.py — no GPU.  The arithmetic is the project's own
(pyspecsdr_amd/csrc/pss_adsb.h), so the truth is made outside it: NumPy builds the captures from the messages, and restates rules 1-7 with
float32 sums added one term at a time; the twin must agree with it record for record, and hand back exactly the injected frames.
tests/test_gpu_adsb.py (-m gpu) holds the kernels to the twin on every byte.  tests/adsb_host.cpp runs the header alone under
AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adsb_cases as A
from bytes_util import same_bytes
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
GOLD = np.load(os.path.join(HERE, "golden", "adsb.npz"))
NAMES = [str(n) for n in GOLD["names"]]
SYMBOLS = ("pss_adsb_plan", "pss_adsb_crc", "pss_adsb_frames", "pss_h_adsb_frames")


def p(a):
    return None if a is None else a.ctypes.data


def both(x, spc, **kw):
    """The twin and the NumPy statement agree on every record -> the twin's result."""
    twin = E.h_adsb_frames(x, spc, **kw)
    ref = A.numpy_frames(x, spc, **kw)
    for t, r, what in zip(twin[:4], ref[:4], ("msg", "pos", "meta", "score")):
        assert same_bytes(t, r), (what, t, r)
    assert twin[4] == ref[4]
    return twin


def test_symbols_are_declared_exported_and_in_the_table():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    units = __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS
    assert ("pss_adsb.hip", ["-ffp-contract=off"]) in units
    for name in ("adsb_plan", "adsb_crc", "adsb_frames", "h_adsb_frames"):
        assert callable(getattr(E, name))
    for name in ("adsb_decode", "adsb_tracks", "adsb_recording"):
        assert callable(getattr(F, name))


def test_goldens_are_the_synthesisers():
    assert NAMES == sorted(A.CASES)
    assert [str(v) for v in GOLD["vectors"]] == list(A.VECTORS + (A.DF19, A.DF24))
    assert {A.CASES[n][0] for n in NAMES} == {1, 2, 3, 5, 8}
    for name in NAMES:
        spc, n, seed, amp, addresses, frames = A.CASES[name]
        assert GOLD[name + "/params"].tolist() == [spc, n, seed, amp] and amp == 10.0 and 4 <= len(frames) <= 6
        assert GOLD[name + "/tx_msg"].tolist() == [m for m, _, _ in frames] and GOLD[name + "/tx_pos"].tolist() == [q for _, q, _ in frames]
        assert A.capture_crc32(A.case_iq(name)) == int(GOLD[name + "/crc32"][0])
    sent = {m for n in NAMES for m, _, _ in A.CASES[n][5]}
    assert {A.ALL_CALL, A.ALT_REPLY, A.DF19, A.DF24} <= sent


def test_plan():
    assert [E.adsb_plan(2e6 * k) for k in range(1, 9)] == list(range(1, 9))
    for fs in (2.4e6, 2.048e6, 3.2e6, 1e6, 18e6, 0.0, -2e6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^pss_adsb: fs / 2 000 000 must be an integer in \[1, 8\]"):
            E.adsb_plan(fs)


def test_crc_of_the_vectors_and_of_every_single_bit_error():
    for v in A.VECTORS + (A.DF19, A.DF24):
        b = bytes.fromhex(v)
        want = A.ADDRESS if v == A.ALT_REPLY else 0
        assert E.adsb_crc(b) == want == A.crc24(b), v
        for i in range(8 * len(b)):
            flipped = bytearray(b)
            flipped[i >> 3] ^= 0x80 >> (i & 7)
            r = E.adsb_crc(flipped)
            assert r == A.crc24(flipped) and r != want, (v, i)


def test_decode_of_the_published_vectors():
    d = F.adsb_decode(bytes.fromhex(A.IDENT), 112)
    assert (d["df"], d["icao"], d["tc"], d["callsign"]) == (17, 0x4840D6, 4, "KLM1023")
    d = F.adsb_decode(bytes.fromhex(A.POS_EVEN), 112)
    assert (d["df"], d["icao"], d["tc"], d["altitude"], d["odd"], d["cpr_lat"], d["cpr_lon"]) == (17, 0x40621D, 11, 38000, 0, 93000, 51372)
    d = F.adsb_decode(np.frombuffer(bytes.fromhex(A.POS_ODD), np.uint8), 112)
    assert (d["tc"], d["altitude"], d["odd"], d["cpr_lat"], d["cpr_lon"]) == (11, 38000, 1, 74158, 50194)
    d = F.adsb_decode(bytes.fromhex(A.VELOCITY), 112)
    assert (d["df"], d["icao"], d["tc"], d["vertical_rate"]) == (17, 0x485020, 19, -832)
    assert abs(d["speed"] - 159.20) < 0.005 and abs(d["track"] - 182.88) < 0.005
    assert F.adsb_decode(bytes.fromhex(A.ALL_CALL) + bytes(7), 56) == {"df": 11, "icao": 0x4840D6}
    assert F.adsb_decode(bytes.fromhex(A.ALT_REPLY), 56) == {"df": 4, "icao": 0x4840D6}
    # Q bit clear: no altitude
    no_q = bytearray(bytes.fromhex(A.POS_EVEN))
    no_q[5] &= 0xFE
    assert F.adsb_decode(bytes(no_q), 112)["altitude"] is None


def rec(msg, t, fs=2e6):
    b = bytes.fromhex(msg)
    return dict(msg=b, n_bits=8 * len(b), pos=int(round(t * fs)))


def test_tracks_and_the_position_of_the_pair():
    fs = 2e6
    tr = F.adsb_tracks([rec(A.IDENT, 0.5), rec(A.POS_ODD, 1.0), rec(A.VELOCITY, 1.5), rec(A.ALT_REPLY, 2.0), rec(A.POS_EVEN, 3.0)], fs)
    assert [t["icao"] for t in tr] == [0x4840D6, 0x40621D, 0x485020]
    klm, pos, vel = tr
    assert (klm["callsign"], klm["frames"], klm["first"], klm["last"], klm["position"]) == ("KLM1023", 2, 0.5, 2.0, None)
    assert pos["altitude"] == 38000 and pos["frames"] == 2 and (pos["first"], pos["last"]) == (1.0, 3.0)
    lat, lon = pos["position"]
    assert abs(lat - 52.2572021484375) <= 1e-9 and abs(lon - 3.91937255859375) <= 1e-9
    assert F._cpr_nl(lat) == 36
    assert vel["velocity"]["vertical_rate"] == -832 and abs(vel["velocity"]["speed"] - 159.20) < 0.005
    # the odd frame the newer one: its own latitude, the same zone
    lat_o, lon_o = F.adsb_tracks([rec(A.POS_EVEN, 1.0), rec(A.POS_ODD, 3.0)], fs)[0]["position"]
    j = np.floor(59 * 93000 / 131072 - 60 * 74158 / 131072 + 0.5)                  # 8
    m = np.floor(51372 / 131072 * 35 - 50194 / 131072 * 36 + 0.5)                   # 0: zone 36 has 35 odd longitude zones
    assert (j, m) == (8, 0)
    assert abs(lat_o - 360 / 59 * (8 + 74158 / 131072)) <= 1e-9 and abs(lon_o - 360 / 35 * (50194 / 131072)) <= 1e-9


def test_no_position_from_a_stale_pair_or_across_zones():
    fs = 2e6
    assert F.adsb_tracks([rec(A.POS_ODD, 1.0), rec(A.POS_EVEN, 11.5)], fs)[0]["position"] is None
    assert F.adsb_tracks([rec(A.POS_ODD, 1.0), rec(A.POS_EVEN, 11.0)], fs)[0]["position"] is not None
    assert F.adsb_tracks([rec(A.POS_EVEN, 1.0)], fs)[0]["position"] is None
    # latitudes on both sides of a zone boundary: NL(lat_even) != NL(lat_odd)
    found = None
    for lat_o in range(0, 131072, 997):
        if F.adsb_position((93000, 51372), (lat_o, 50194), False) is None:
            found = lat_o
            break
    assert found is not None


@pytest.mark.parametrize("name", NAMES)
def test_twin_is_the_numpy_statement_and_recovers_the_frames(name):
    spc = A.CASES[name][0]
    iq = A.case_iq(name)
    msg, pos, meta, score, count = both(iq, spc, icao=GOLD[name + "/addresses"])
    assert same_bytes(msg, GOLD[name + "/msg"]) and same_bytes(pos, GOLD[name + "/pos"]) and same_bytes(meta, GOLD[name + "/meta"])
    assert same_bytes(score, GOLD[name + "/score"])
    # exactly the injected reportable frames, each once, at its injection sample: no DF 19, no DF 24, the DF 4 only with its address
    assert [(bytes(m), int(q)) for m, q in zip(msg, pos)] == A.case_expected(name) and count == len(pos)
    assert all((int(w) >> 16) in A.REPORTED_DF for w in meta)
    bare = both(iq, spc)
    assert [int(w) >> 16 for w in bare[2]] == [int(w) >> 16 for w in meta if (int(w) >> 16) in (11, 17, 18)]


def test_rule_6_has_work_to_do_at_spc_5():
    """Without the rule the fixture capture reports several starts per frame.  A window of one start still sees its suppressors; a capture
    cut to the start's own 240 spc samples holds none of a long frame's (they do not fit it)."""
    name = "spc5"
    spc, n = A.CASES[name][0], A.CASES[name][1]
    iq = A.case_iq(name)
    addresses = GOLD[name + "/addresses"]
    kept = E.h_adsb_frames(iq, spc, icao=addresses)[1].tolist()
    raw = 0
    for q in kept:
        for s in range(q - 2 * spc + 1, q + 2 * spc):
            if 0 <= s and s + 240 * spc <= n:
                raw += E.h_adsb_frames(iq[s:s + 240 * spc], spc, icao=addresses, s_begin=0, s_end=1, n_capture=240 * spc)[4]
    assert raw > len(kept)


def test_noise_alone_reports_nothing():
    """2 000 000 samples of unit noise at spc 1 and 2: a few preambles pass in a million starts at spc 1 (the count is printed and written
    into PARITY.md), none of them is a frame."""
    rng = np.random.default_rng(7)
    n = 2_000_000
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    for spc in (1, 2):
        stats = {}
        assert A.numpy_frames(x, spc, icao=[A.ADDRESS], stats=stats)[4] == 0
        assert E.h_adsb_frames(x, spc, icao=[A.ADDRESS])[4] == 0
        print(f"noise alone, spc {spc}: {stats['survivors']} preamble survivors in {n} samples, no frame")
        # spc 1: the magnitudes are unit exponentials, so P(min of four > 2 max of twelve) = 12 B(9, 12) = 12 * 8! 11! / 20! = 7.94e-6 a
        # start: 15.9 expected in 2 000 000, Poisson deviation 4.0; six deviations up is 40.  spc 2: sums of two concentrate, so fewer pass.
        assert stats["survivors"] <= 40 and (spc == 2 or stats["survivors"] >= 1)


def test_edges_of_the_capture():
    for spc in (1, 3):
        span, half = 240 * spc, 128 * spc
        for at in (0, 7):
            x = A.clean(at + span, spc, [(A.IDENT, at)])                      # at sample 0; ending on the last sample
            assert both(x, spc)[1].tolist() == [at]
            assert both(x[:-1], spc)[4] == 0                                     # one sample shorter: not reported
        x = A.clean(5 + half, spc, [(A.ALL_CALL, 5)])                         # a short frame fits where a long one would not
        assert both(x, spc)[1].tolist() == [5]
        x = A.clean(3 + span + half + span, spc, [(A.IDENT, 3), (A.ALL_CALL, 3 + span), (A.VELOCITY, 3 + span + half)])   # back to back
        assert both(x, spc)[1].tolist() == [3, 3 + span, 3 + span + half]
        assert both(np.zeros(1000, np.complex64), spc)[4] == 0                   # all zero
        for n in (0, 1, half - 1):
            assert both(np.ones(n, np.complex64), spc)[4] == 0                   # below one short frame


def test_the_preamble_comparison_is_strict():
    c = A.chips_of(A.IDENT)
    x = np.where(c > 0, 2.0, 0.0).astype(np.complex64)
    gaps = [k for k in range(16) if k not in A.PULSES]
    x[gaps] = 1 + 1j                                                              # m = 2 in every gap, 4 in every pulse: hi == 2 lo
    assert both(x, 1)[4] == 0
    x[list(A.PULSES)] = 2.5
    assert both(x, 1)[1].tolist() == [0]
    assert both(x, 1, ratio=6.25 / 2)[4] == 0 and both(x, 1, ratio=3.0)[4] == 1     # 6.25 == 3.125 * 2 exactly; 6.25 > 6


def test_non_finite_samples_take_their_frame_and_no_other():
    name = "spc3"
    spc = A.CASES[name][0]
    x = A.case_iq(name).copy()
    ref = both(x, spc)
    q = int(ref[1][1])
    x[q + spc] = np.nan
    x[q + spc * 90 + 1] = np.inf
    got = both(x, spc)
    keep = [k for k, s in enumerate(ref[1].tolist()) if s != q]
    for a, b in zip(got[:4], ref[:4]):
        assert same_bytes(a, b[keep])


def test_max_frames_keeps_the_true_count():
    name = "spc2"
    spc = A.CASES[name][0]
    iq = A.case_iq(name)
    full = both(iq, spc, icao=[A.ADDRESS])
    for mf in (0, full[4] - 1):
        cut = both(iq, spc, icao=[A.ADDRESS], max_frames=mf)
        assert cut[4] == full[4] and len(cut[1]) == mf and same_bytes(cut[0], full[0][:mf])
    # nothing is written past max_frames
    lib = L.load()
    x = np.ascontiguousarray(iq)
    msg, pos = np.full((full[4], 14), 0xA5, np.uint8), np.full(full[4], -7, np.int64)
    meta, score, count = np.full(full[4], 7, np.uint32), np.full(full[4], -7, np.float32), np.zeros(1, np.int32)
    a = np.array([A.ADDRESS], np.uint32)
    assert lib.pss_h_adsb_frames(p(x), len(x), 0, len(x), spc, 2.0, p(a), 1, 0, len(x), p(msg), p(pos), p(meta), p(score), p(count), 2) == 0
    assert count[0] == full[4] and np.all(msg[2:] == 0xA5) and np.all(pos[2:] == -7) and np.all(meta[2:] == 7) and np.all(score[2:] == -7)
    assert same_bytes(msg[:2], full[0][:2])


def test_equal_scores_keep_the_earlier_start():
    x, q = A.twin_starts()
    assert both(x, 2)[1].tolist() == [q]
    # each of the two alone is accepted: a buffer that ends before the later start's last chip holds only the earlier one, and the
    # later one reported through a window of its own is dropped by the earlier one outside the window
    assert both(x, 2, s_begin=q + 1)[4] == 0 and both(x, 2, s_end=q + 1)[1].tolist() == [q]
    y = x.copy()
    y[q + 1] *= 1.5                           # the first pulse is no longer the weakest: nothing changes
    assert both(y, 2)[1].tolist() == [q]
    y = x.copy()
    y[q + 2 * np.array([1, 3, 8, 10])] = 0.5  # the first samples of the earlier start's gaps 1, 3, 8, 10 lie in the later start's pulses: its score is 1.25
    assert both(y, 2)[1].tolist() == [q + 1]


def test_address_list():
    x = A.clean(400, 1, [(A.ALT_REPLY, 11), (A.ALL_CALL, 200)])
    first = (A.ADDRESS + 7 * np.arange(1000)).astype(np.uint32)
    last = (A.ADDRESS - 7 * np.arange(999, -1, -1)).astype(np.uint32)
    for icao, n_want in (((), 1), ([A.ADDRESS], 2), (first, 2), (last, 2), (first[1:], 1)):
        assert both(x, 1, icao=icao)[4] == n_want


def test_windows_do_not_change_a_byte():
    x, cuts = A.windows_capture()
    n, spc = len(x), 2
    whole = both(x, spc)
    assert whole[4] == 3
    for base in (0, 2 ** 40 + 777):
        pad = 2 * spc - 1 if base else 0
        xx = np.concatenate([np.zeros(pad, np.complex64), x])
        origin = base - pad
        parts = []
        edges = [0] + cuts + [n]
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = A.reach(base + s0, base + s1, spc, base + n)
            parts.append(both(xx[lo - origin:hi - origin], spc, buf_index0=lo, n_capture=base + n, s_begin=base + s0, s_end=base + s1))
        for i in range(4):
            joined = np.concatenate([q[i] for q in parts])
            assert same_bytes(joined, whole[i] + base if i == 1 else whole[i]), (base, i)
        assert sum(q[4] for q in parts) == whole[4]


def test_a_resampled_dongle_capture_gives_its_frames_back():
    msgs = [A.IDENT, A.POS_EVEN, A.VELOCITY, A.ALL_CALL]
    x = A.synth_rate(24000, 2.4e6, [(m, t0, 10.0, 0.3 + i) for i, (m, t0) in enumerate(zip(msgs, A.RATE_CASE_US))], seed=A.RATE_CASE_SEED)
    assert F.plan_resample(2.4e6, 4e6) == (5, 3)
    msg, pos, meta, score, count = both(E.h_resample(x, 5, 3), 2)
    assert [bytes(m[:(int(w) & 0xFFFF) // 8]).hex().upper() for m, w in zip(msg, meta)] == msgs
    assert all(abs(q / 4.0 - t0) <= 0.5 for q, t0 in zip(pos.tolist(), A.RATE_CASE_US))      # within one chip of the injection


def test_refusals_by_message():
    lib = L.load()
    x = A.clean(300, 1, [(A.IDENT, 5)])
    msg, pos, meta, score, count = np.zeros((4, 14), np.uint8), np.zeros(4, np.int64), np.zeros(4, np.uint32), np.zeros(4, np.float32), np.full(1, -7, np.int32)
    ok = dict(iq=p(x), n_buf=300, index0=0, n_capture=300, spc=1, ratio=2.0, icao=None, n_icao=0, s0=0, s1=300, msg=p(msg), pos=p(pos), meta=p(meta),
              score=p(score), count=p(count), max_frames=4)

    def refused(why, **kw):
        a = dict(ok, **kw)
        r = lib.pss_h_adsb_frames(a["iq"], a["n_buf"], a["index0"], a["n_capture"], a["spc"], a["ratio"], a["icao"], a["n_icao"], a["s0"], a["s1"], a["msg"],
                                  a["pos"], a["meta"], a["score"], a["count"], a["max_frames"])
        assert r == L.PSS_E_ARG and lib.pss_last_error(None).decode() == "pss_adsb_frames: " + why, lib.pss_last_error(None).decode()
        assert count[0] == -7 and not msg.any()                                    # a refused call writes nothing
    refused("spc outside [1, 8]", spc=9)
    refused("spc outside [1, 8]", spc=0)
    for ratio in (-1.0, float("nan"), float("inf")):
        refused("ratio must be finite and not negative", ratio=ratio)
    refused("s_end < s_begin", s0=10, s1=9)
    refused("the window does not lie inside the capture", s1=301)
    refused("the buffer does not lie inside the capture", n_capture=299)
    reach = "the buffer does not cover the window's reach (2 spc - 1 starts either side, 240 spc samples forward)"
    refused(reach, n_buf=299, n_capture=1000, s1=60)                               # the window's last start reads to 60 + 239
    refused(reach, index0=1, n_capture=301, s0=1, s1=2)                            # and the start in front of its first
    refused("max_frames < 0", max_frames=-1)
    refused("null buffer", count=None)
    refused("null buffer", iq=None)
    refused("null buffer", msg=None)
    refused("null buffer", icao=None, n_icao=1)
    refused("a misaligned pointer", iq=p(x) + 4)
    refused("a misaligned pointer", pos=p(pos) + 4)
    refused("a misaligned pointer", count=p(count) + 2)
    for bad in ([5, 4], [4, 4], [1 << 24]):
        a = np.array(bad, np.uint32)
        refused("the address list must be ascending, unique and below 2^24", icao=p(a), n_icao=len(a))
    assert lib.pss_h_adsb_frames(*[ok[k] for k in ("iq", "n_buf", "index0", "n_capture", "spc", "ratio", "icao", "n_icao", "s0", "s1", "msg", "pos", "meta",
                                                   "score", "count", "max_frames")]) == 0 and count[0] == 1 and pos[0] == 5
    # an empty window is no refusal: the count is zero
    assert E.h_adsb_frames(x, 1, s_begin=7, s_end=7)[4] == 0


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/adsb_host.cpp: pss_adsb.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "adsb_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "adsb_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "adsb_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- the captures tests/test_gpu_adsb.py sends through the kernels' loops and carries: here the twin is held to the NumPy statement on them
def test_twin_starts_is_same_score_starts_at_spc_2():
    c = A.chips_of(A.IDENT)
    for q, tail in ((41, 9), (4095, 9), (7, 3)):
        x = np.zeros(q + 2 * len(c) + tail, np.complex64)
        x[q + 1:q + 1 + 2 * len(c):2] = c
        for got in (A.twin_starts(q, tail), A.same_score_starts(2, q, tail=tail)):
            assert got[1] == q and got[0].dtype == np.complex64 and same_bytes(got[0], x)


def test_overlaid_has_the_address_as_its_remainder():
    for head in ("20000B38", "A0000B38AB0D0D11223344"):
        m = bytes.fromhex(A.overlaid(head, A.ADDRESS))
        assert A.crc24(m) == A.ADDRESS == E.adsb_crc(m) and m[:-3] == bytes.fromhex(head) and A.crc24(bytes.fromhex(A.with_parity(head))) == 0
    assert A.overlaid("20000B38", A.ADDRESS) == A.ALT_REPLY


def test_every_downlink_format():
    x, accepted = A.every_format_capture()
    assert len(accepted) == 9
    first = (A.ADDRESS + 7 * np.arange(1000)).astype(np.uint32)
    last = (A.ADDRESS - 7 * np.arange(999, -1, -1)).astype(np.uint32)
    for icao in ([A.ADDRESS], first, last):
        msg, pos, meta, score, count = both(x, 1, icao=icao)
        assert pos.tolist() == accepted and count == 9
        assert [int(w) >> 16 for w in meta] == list(A.REPORTED_DF) and [int(w) & 0xFFFF for w in meta] == [56, 56, 56, 56, 112, 112, 112, 112, 112]
        assert [A.crc24(bytes(m[:(int(w) & 0xFFFF) // 8])) for m, w in zip(msg, meta)] == [A.ADDRESS] * 3 + [0, A.ADDRESS, 0, 0, A.ADDRESS, A.ADDRESS]
    msg, pos, meta, score, count = both(x, 1)
    assert count == 3 and [int(w) >> 16 for w in meta] == [11, 17, 18] and pos.tolist() == [accepted[3], accepted[5], accepted[6]]
    assert both(x, 1, icao=first[1:])[4] == 3                       # 999 addresses, none of them the frames'


@pytest.mark.parametrize("spc", [2, 4, 8])
def test_equal_scores_at_every_start_of_a_chip(spc):
    q = A.TILE - spc // 2                                           # the spc starts lie on both sides of a tile boundary of the kernel
    x, _ = A.same_score_starts(spc, q)
    assert both(x, spc)[1].tolist() == [q]
    for k in range(1, spc):                                         # every later start alone is accepted, with the same score bits
        alone = both(x[q + k:], spc, s_begin=0, s_end=1)
        assert alone[4] == 1 and same_bytes(alone[3], both(x, spc)[3])
    assert both(x, spc, s_begin=q + 1)[4] == 0                      # the earliest start lies outside the window and still drops the others
    assert both(x, spc, s_begin=q + spc - 1)[4] == 0
    assert both(x, spc, s_end=q)[4] == 0
    assert both(x, spc, ratio=0.0)[1].tolist() == [q]


@pytest.mark.parametrize("spc", [1, 3, 8])
@pytest.mark.parametrize("msg", [A.IDENT, A.ALL_CALL], ids=["long", "short"])
def test_frames_that_end_with_the_capture(spc, msg):
    x, q = A.ending_capture(spc, msg)
    assert len(x) == A.TILE + 5
    assert both(x, spc)[1].tolist() == [q]
    # one sample shorter: the frame at q no longer fits.  spc 8: the start in front of it slices the same bits out of 7/8 of every chip and fits
    assert both(x[:-1], spc)[1].tolist() == ([q - 1] if spc == 8 else [])


def test_window_of_two_tiles_with_exactly_its_reach():
    x, q, spc = A.two_tile_window_capture(), A.TWO_TILE_P, 8
    n = len(x)
    whole = both(x, spc)
    assert whole[1].tolist() == [q, q + 240 * spc + 100]
    for c in A.TWO_TILE_EXTRA:
        s_begin = q - 4066 - c
        for s_end, want in ((q, []), (q + 1, [q])):                 # start q - 1 is accepted; q, in the right margin, drops it
            lo, hi = A.reach(s_begin, s_end, spc, n)
            assert hi - lo == A.TILE + c + 1919 + (s_end - q)
            part = both(x[lo:hi], spc, buf_index0=lo, n_capture=n, s_begin=s_begin, s_end=s_end)
            assert part[1].tolist() == want and part[4] == len(want)
            inside = (whole[1] >= s_begin) & (whole[1] < s_end)
            for a, b in zip(part[:4], whole[:4]):
                assert same_bytes(a, b[inside])


@pytest.mark.parametrize("spc", [1, 2, 4, 6, 7, 8])
def test_dense_survivors(spc):
    """ratio 0: nearly every start survives its preamble test.  At spc 8 the frame at 700 runs into the one at 2500 (700 + 1920 > 2500) and
    is not reported at any start."""
    stats = {}
    x = A.dense_capture(spc)
    A.numpy_frames(x, spc, ratio=0.0, stats=stats)
    assert stats["survivors"] > A.TILE
    pos = both(x, spc, ratio=0.0)[1]
    for q in (700,) * (spc < 8) + (2500, A.TILE - 5):
        assert np.any(np.abs(pos - q) < spc), (q, pos)

"""Packet radio's host-side shapes — pss_packet_plan over the project's sample rates, the tone table against NumPy, formats.ax25_decode /
aprs_tnc2 / aprs_decode on the published vectors, aprs_tracks — no GPU."""
import math
import re

import numpy as np
import pytest

import packet_cases as P
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine as E


def test_plan():
    assert E.packet_plan(2.4e6) == (90, 99, 100) and E.packet_plan(240e3) == (9, 99, 100)          # the issue's two: 99 / 100 behind pss_ddc
    assert E.packet_plan(26400) == (1, 1, 1) and E.packet_plan(264000) == (10, 1, 1) and E.packet_plan(250e3) == (9, 594, 625)
    for fs in (240000, 250000, 1024000, 2048000, 2400000, 3200000, 10000000, 20000000, 48000, 96000, 200000):
        d = min(fs // 26400, 204)
        g = math.gcd(26400 * d, fs)
        up, down = 26400 * d // g, fs // g
        if up <= 4096 and down <= 4096:
            assert E.packet_plan(fs) == (d, up, down), fs
            assert fs * up == 26400 * d * down                                                      # fs / d up / down is 26 400 exactly
        else:
            with pytest.raises(ValueError, match=r"^pss_packet: 26 400 decim / fs reduces to factors outside \[1, 4096\]"):
                E.packet_plan(fs)
    assert E.packet_plan(10e6) == (204, 1683, 3125) and E.packet_plan(2.048e6) == (77, 2541, 2560) and E.packet_plan(1.024e6) == (38, 627, 640)
    with pytest.raises(ValueError, match="factors outside"):
        E.packet_plan(20e6)                                                                         # 1683 / 6250
    for fs, why in ((26400.5, "fs must be an integer number of Hz"), (float("nan"), "fs must be an integer number of Hz"),
                    (26399.0, "fs must be at least 26 400"), (-1.0, "fs must be at least 26 400"),
                    (1000003.0, "26 400 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take")):
        with pytest.raises(ValueError, match="^" + re.escape("pss_packet: " + why)):
            E.packet_plan(fs)


def test_tone_table_against_numpy():
    t = E.packet_default_tones()
    assert t.shape == (4, 22) and t.dtype == np.float64
    ref = P.tones()
    # libm against NumPy: the last bit may differ, nothing more; the receiver never computes the table on the device, so that bit never
    # enters a comparison between the kernel and its twin
    assert np.max(np.abs(t - ref)) <= 2 ** -52
    assert t[0, 0] == 1.0 and t[1, 0] == 0.0 and t[2, 0] == 1.0 and t[3, 0] == 0.0 and t[2, 6] == -1.0 and t[2, 12] == 1.0
    # one cycle of the mark tone a window: its rows are orthogonal and of energy 11; the space rows hold 11 / 6 cycles
    assert abs(t[0] @ t[1]) < 1e-12 and abs(t[0] @ t[0] - 11) < 1e-12 and abs(t[1] @ t[1] - 11) < 1e-12
    assert abs(t[2] @ t[2] + t[3] @ t[3] - 22) < 1e-12


def test_ax25_decode_and_the_monitor_line():
    body = P.FRAMES["position"]
    d = F.ax25_decode(body)
    assert d["dest"] == dict(call="APRS", ssid=0, repeated=True) and d["source"] == dict(call="N0CALL", ssid=7, repeated=False)
    assert d["path"] == [dict(call="WIDE1", ssid=1, repeated=True), dict(call="WIDE2", ssid=2, repeated=False)]
    assert (d["control"], d["pid"], d["info"]) == (0x03, 0xF0, P.POSITION)
    assert F.aprs_tnc2(body) == "N0CALL-7>APRS,WIDE1-1*,WIDE2-2:" + P.POSITION.decode()
    assert F.aprs_tnc2(P.FRAMES["status"]) == "DL1ABC>APRS:>Net Control Center"
    assert F.aprs_tnc2(P.FRAMES["message"]) == "N0CALL-7>APRS,RELAY*,WIDE2-1::W1AW-9   :Testing 1 2 3{042"
    # the star stands behind the LAST digipeater that has repeated
    two = P.ui_frame(("APRS", 0), ("W1AW", 0), [("A", 1, True), ("B", 2, True), ("C", 3, False)], b">x")
    assert F.aprs_tnc2(two) == "W1AW>APRS,A-1,B-2*,C-3:>x"
    long = F.ax25_decode(P.FRAMES["long"])
    assert len(long["path"]) == 8 and long["source"]["ssid"] == 15 and long["info"] == bytes([0xFF]) * 256
    short = F.ax25_decode(P.FRAMES["short"])
    assert (short["dest"]["call"], short["source"]["call"], short["path"], short["control"], short["pid"], short["info"]) == ("CQ", "N0CALL", [], 3, None, b"")
    sframe = P.address("CQ") + P.address("N0CALL", 1, last=True) + bytes([0x01, 0x55])          # a supervisory frame carries no PID
    assert F.ax25_decode(sframe)["pid"] is None and F.ax25_decode(sframe)["info"] == b"\x55"
    for bad in (b"", bytes(14), P.address("N0CALL", 0, last=True) + b"\x03\xf0", P.FRAMES["status"][:14]):
        with pytest.raises(ValueError, match="malformed address field"):
            F.ax25_decode(bad)


def test_aprs_positions_the_published_vectors():
    d = F.aprs_decode(b"!4903.50N/07201.75W-")
    assert d["type"] == "!" and abs(d["lat"] - 49.05833) < 1e-5 and abs(d["lon"] + 72.02917) < 1e-5 and d["symbol"] == "/-" and not d["compressed"]
    assert d["lat"] == 49 + 3.5 / 60 and d["lon"] == -(72 + 1.75 / 60) and d["comment"] == ""
    c = F.aprs_decode("=/5L!!<*e7>7P[")
    assert c["type"] == "=" and c["compressed"] and c["symbol"] == "/>" and c["course"] == 88 and abs(c["speed"] - 36.2) < 0.05
    assert c["lat"] == 90 - 15427503 / 380926 and c["lon"] == -180 + 20427156 / 190463            # the base-91 arithmetic, by hand
    assert abs(c["lat"] - 49.5) < 1e-4 and abs(c["lon"] + 72.75) < 1e-4
    # with a timestamp, with course and speed in the comment, south and east
    t = F.aprs_decode(b"@092345z4903.50N/07201.75W>088/036 under way")
    assert t["timestamp"] == "092345z" and t["course"] == 88 and t["speed"] == 36.0 and t["comment"] == " under way" and t["symbol"] == "/>"
    s = F.aprs_decode(b"/092345z3356.55S\\15112.72E#")
    assert s["lat"] == -(33 + 56.55 / 60) and s["lon"] == 151 + 12.72 / 60 and s["symbol"] == "\\#"
    tc = F.aprs_decode(b"@092345z/5L!!<*e7>  [")
    assert tc["compressed"] and "course" not in tc and tc["timestamp"] == "092345z"
    # a position that is none: type and raw text
    for raw in (b"!", b"!4903.50X/07201.75W-", b"=short"):
        d = F.aprs_decode(raw)
        assert d["type"] == raw[:1].decode() and d["raw"] == raw[1:].decode() and "lat" not in d


def test_aprs_status_messages_and_the_rest():
    assert F.aprs_decode(b">Net Control Center") == dict(type=">", raw="Net Control Center", status="Net Control Center")
    m = F.aprs_decode(b":W1AW-9   :Testing 1 2 3{042")
    assert (m["type"], m["addressee"], m["text"], m["number"]) == (":", "W1AW-9", "Testing 1 2 3", "042")
    assert F.aprs_decode(b":BLN1     :no number")["number"] is None and F.aprs_decode(b":short")["raw"] == "short"
    for raw in (b"`(_f n\"Oj/", b"'abc", b"T#005,199,000,255,073,123,01101001", b"_10090556c220s004g005t077", b""):
        d = F.aprs_decode(raw)
        assert d == dict(type=raw[:1].decode("latin-1"), raw=raw[1:].decode("latin-1"))             # Mic-E included: out of scope
    assert F.aprs_decode(bytes([0x3E, 0xE9]))["status"] == "é"                                # Latin-1, never an exception


def test_aprs_tracks():
    fs = 26400
    recs = [dict(msg=P.FRAMES["position"], pos=26400), dict(msg=P.FRAMES["status"], pos=3 * 26400), dict(msg=P.FRAMES["compressed"], pos=2 * 26400),
            dict(msg=P.FRAMES["message"], pos=5 * 26400),
            dict(msg=P.ui_frame(("APRS", 0), ("N0CALL", 7), [], b">on the air"), pos=4 * 26400)]
    tr = F.aprs_tracks(recs, fs)
    assert [t["source"] for t in tr] == ["N0CALL-7", "DL1ABC", "W1AW-9"]
    a, b, c = tr
    assert a["frames"] == 3 and (a["first"], a["last"]) == (1.0, 5.0) and a["position"] == (49 + 3.5 / 60, -(72 + 1.75 / 60)) and a["symbol"] == "/-"
    assert a["status"] == "on the air" and a["course"] is None
    assert b["frames"] == 1 and b["position"] is None and b["status"] == "Net Control Center" and b["first"] == b["last"] == 3.0
    assert c["position"] == (90 - 15427503 / 380926, -180 + 20427156 / 190463) and c["course"] == 88 and abs(c["speed"] - 36.2) < 0.05
    assert F.aprs_tracks([]) == []

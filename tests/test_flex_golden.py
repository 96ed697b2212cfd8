"""The FLEX receiver's host side — pss_flex_default_pulse, pss_flex_word, pss_h_flex_frames, formats.flex_messages / flex_lines / h_flex_rows —
against tests/golden/flex.npz and the NumPy statement of the rules in tests/flex_cases.py — no GPU.  The arithmetic is the project's own
(pyspecsdr_amd/csrc/pss_flex.h), the reference holds no FLEX code and no FLEX program or off-air capture was at hand, so the truth is made
outside the library: NumPy builds the frames from the messages with an encoder written from the same published description as the
receiver (not checked against a transmitter), and restates the rules; the twin must agree with the statement record for record, and hand
back exactly the injected messages.  tests/test_gpu_flex.py (-m gpu) holds the kernels to the twin on every byte.  tests/flex_host.cpp runs
the header alone under AddressSanitizer and UBSan."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import flex_cases as F
import pocsag_cases as P
from bytes_util import same_bytes
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as FM
from pyspecsdr_amd.engine import Engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "flex.npz"))


def test_symbols_are_declared_exported_and_in_the_table():
    hdr = open(os.path.join(ROOT, "include", "pss.h")).read()
    lib = L.load()
    for name in ("pss_flex_default_pulse", "pss_flex_word", "pss_flex_frames", "pss_h_flex_frames"):
        assert re.search(rf"\b{name}\(", hdr) and hasattr(lib, name) and name in L.exported_symbols(), name
    assert os.path.getsize(os.path.join(HERE, "golden", "flex.npz")) <= 4096


def test_the_word_is_a_pocsag_codeword_bit_reversed():
    brev21 = lambda d: F.brev32(d) >> 11
    for d in list(range(0, 1 << 21, 9973)) + [0, 1, 0x1FFFFF, 0x100000, 0x0AAAAA]:
        w = E.flex_word(d)
        assert w == F.brev32(E.pocsag_codeword(brev21(d))) == F.word(d) and w & 0x1FFFFF == d and bin(w).count("1") % 2 == 0
        assert P.remainder31(F.brev32(w) >> 1) == 0
    assert E.flex_word(0x3FFFFF) == E.flex_word(0x1FFFFF)        # bits above the 21 are ignored


def test_pulse():
    for h in range(1, 65):
        g = E.flex_default_pulse(h)
        assert len(g) == F.pulse_len(h) == (h if h & 1 else max(h - 1, 1)) and np.all(g == 1.0 / len(g))
    for h in (0, 65, -1):
        with pytest.raises(ValueError):
            E.flex_default_pulse(h)


def test_goldens_are_the_synthesisers(golden):
    assert golden["names"].tolist() == sorted(F.CASES)
    for k, name in enumerate(sorted(F.CASES)):
        assert F.row_crc32(F.case_row(name)) == int(golden["crc32"][k, 0]), name
    assert sorted(c[0] for c in F.CASES.values())[:4] == [0, 1, 1, 2] and any(c[3] for c in F.CASES.values())
    assert any(c[1] == 12 and c[4] is not None for c in F.CASES.values())


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_twin_is_the_numpy_statement_and_the_golden_and_recovers_the_messages(golden, name):
    mode, h, _, inverted, _ = F.CASES[name]
    k = sorted(F.CASES).index(name)
    y = F.case_row(name)
    ref = F.numpy_frames(y, h)
    twin = E.h_flex_frames(y, h)
    for a, b in zip(twin[:7], ref[:7]):
        assert same_bytes(a, b), (name, a, b)
    assert twin[7] == ref[7] == 1
    assert same_bytes(twin[4], golden["pos"][k:k + 1]) and same_bytes(twin[2], golden["fiw"][k:k + 1]) and same_bytes(twin[5], golden["meta"][k:k + 1])
    assert same_bytes(twin[6], golden["score"][k:k + 1])
    assert (zlib.crc32(twin[0].tobytes()), zlib.crc32(twin[1].tobytes())) == tuple(int(v) for v in golden["crc32"][k, 1:])
    recs = FM.flex_records(*twin[:7])
    assert recs[0]["mode"] == mode and recs[0]["inverted"] == inverted and recs[0]["n_bad"] == 0
    assert (recs[0]["baud"], recs[0]["levels"]) == F.MODES[mode][1:] and (recs[0]["cycle"], recs[0]["frame"]) == (F.CASES[name][2] & 15, F.CASES[name][2])
    msgs = FM.flex_messages(recs)
    assert F.reported(msgs) == F.expected(mode, F.MESSAGES) and not any(m["damaged"] for m in msgs)
    for other in (1, 2, 12):
        if other != h:
            assert E.h_flex_frames(y, other)[7] == 0, (name, other)


@pytest.mark.parametrize("mode", range(5))
def test_round_trip_of_alphanumeric_and_numeric_messages_in_every_mode_and_phase(mode):
    per_phase = {p: [(1000 * (p + 1) + mode, "ALN", f"mode {mode} phase {F.PHASES[p]}: ~text~ with 7-bit characters!"), (2 ** 20 + p, "NUM", "0123456789 U-[]"[:15 - p]),
                     (40000 + p, "NUM", "7"), (90 + p, "ALN", "")] for p in range(4)}
    for inverted in (False, True):
        y = F.frame_row(mode, 1, 20, 20 + F.FRAME_H + 5, inverted=inverted, per_phase=per_phase, cycle=mode, frame=120 + mode)
        twin = E.h_flex_frames(y, 1)
        assert twin[7] == 1 and twin[4].tolist() == [20]
        msgs = FM.flex_messages(FM.flex_records(*twin[:7]))
        assert F.reported(msgs) == F.expected(mode, per_phase)
        assert all((m["cycle"], m["frame"], m["baud"], m["levels"]) == (mode, 120 + mode) + F.MODES[mode][1:] and not m["damaged"] for m in msgs)
        assert all(m["fragment"] == 3 and m["cont"] == 0 for m in msgs if m["type"] == "ALN")


def test_lines_and_message_rules():
    y = F.frame_row(3, 1, 20, 20 + F.FRAME_H + 5)
    recs = FM.flex_records(*E.h_flex_frames(y, 1)[:7])
    msgs = FM.flex_messages(recs)
    lines = FM.flex_lines(msgs)
    assert lines[0] == "FLEX: 3200/4/A 03.077 [001234567] ALN Hello, FLEX pager!"
    assert lines[1] == "FLEX: 3200/4/A 03.077 [000000042] NUM 0123456789"
    assert lines[2] == "FLEX: 3200/4/A 03.077 [000000099] T2 00002D"
    assert "FLEX: 3200/4/C 03.077 [long 1F0000 012345] T6 000069 0AAAAA" in lines and len(lines) == len(F.expected(3, F.MESSAGES))
    # a long address takes two address words and two vector words: the message behind it is found where it was put
    assert [m["text"] for m in msgs if m["phase"] == "C" and "text" in m] == ["phase C: the odd symbols at 3200 baud.", "42"]
    # damage: an uncorrectable word in a message's body, in its vector, in the block information word
    body = dict(recs[0], fix=[list(f) for f in recs[0]["fix"]], words=[list(w) for w in recs[0]["words"]])
    d = [w & 0x1FFFFF for w in body["words"][0]]
    first_vec = d[0] >> 10 & 63
    start = d[first_vec] >> 7 & 127
    body["fix"][0][start + 2] = 255
    hurt = FM.flex_messages([body])
    assert [m["damaged"] for m in hurt if m["phase"] == "A"] == [True, False, False] and hurt[0]["type"] == "ALN"
    body["fix"][0][start + 2], body["fix"][0][first_vec + 1] = 0, 255
    hurt = FM.flex_messages([body])
    assert [m["damaged"] for m in hurt if m["phase"] == "A"] == [False, True, False] and hurt[1]["type"] == 3 and "text" not in hurt[1]
    body["fix"][0][first_vec + 1], body["fix"][0][0] = 0, 255
    assert [m for m in FM.flex_messages([body]) if m["phase"] == "A"] == []
    body["fix"][0][0], body["words"][0][0] = 0, body["words"][0][0] ^ 1
    assert [m for m in FM.flex_messages([body]) if m["phase"] == "A"] == []      # the block information word's sum
    assert FM.flex_messages([]) == [] and FM.flex_lines([]) == []


def test_host_rows_from_fsk_in_every_mode():
    """FSK IQ at 12 samples a symbol through the host front (discriminator and boxcar) and the twin: the four-level thresholds come from the
    frame's own sync."""
    n = 300 + F.FRAME_H * 12 + 300
    for mode, inverted, off in ((0, False, 0.0), (1, True, 900.0), (2, False, -1200.0), (3, True, 400.0), (4, False, 0.0)):
        lv = F.frame_levels(mode, F.frame_words(mode, F.MESSAGES))
        x = F.fsk_iq(n, 12, [(lv, 300)], offset_hz=off, inverted=inverted) + 1e-3
        msgs, frames = FM.h_flex_rows(x.astype(np.complex64))
        assert len(frames) == 1 and frames[0]["mode"] == mode and frames[0]["inverted"] == inverted and frames[0]["n_bad"] == 0, (mode, frames)
        assert F.reported(msgs) == F.expected(mode, F.MESSAGES)


def test_the_end_to_end_capture_reads_clean_by_the_numpy_statement_alone():
    """tests/test_gpu_flex.py::test_recording_end_to_end's capture through the host twins of the down-converter, the resampler and the front,
    then the NumPy statement: at 25 dB in the 38.4 kHz band both frames are reported with n_bad = 0 and no fixed bit, and the lines are those
    that were sent.  The low-pass is flex_recording's default: firwin(20 decim + 1, 20 000 / fs)."""
    fs = F.CAPTURE_FS
    x = F.capture()
    decim, up, down = E.pocsag_plan(fs)
    assert (decim, up, down) == (6, 24, 25)
    taps = np.empty(20 * decim + 1, np.float64)
    assert L.load().pss_design_firwin(len(taps), 20000.0 / fs, taps.ctypes.data) == 0
    words = np.array([E.ddc_word(c[0], fs)[0] for c in F.CHANNELS], np.uint64)
    y = E.h_ais_front(E.h_resample(E.h_ddc(x, words, decim, taps=taps), up, down), pulse=E.flex_default_pulse(F.CAPTURE_H))
    ref = F.numpy_frames(y, F.CAPTURE_H)
    assert ref[7] == 2 and ref[3].tolist() == [0, 1] and (ref[5][:, 1] & 0xFFFF).tolist() == [0, 0]
    assert (ref[5][:, 0] >> 12 & 15).tolist() == [c[1] for c in F.CHANNELS] and (ref[5][:, 0] >> 8 & 1).tolist() == [int(c[2]) for c in F.CHANNELS]
    assert FM.flex_lines(FM.flex_messages(FM.flex_records(*ref[:7]))) == F.capture_lines()
    twin = E.h_flex_frames(y, F.CAPTURE_H)
    assert all(same_bytes(a, b) for a, b in zip(twin[:7], ref[:7]))


def test_max_frames_keeps_the_true_count_and_windows_do_not_change_a_byte():
    y, starts = F.stub_train(9, h=1)
    full = E.h_flex_frames(y, 1, max_bad=352)
    assert full[7] == 9 and full[4].tolist() == starts
    cut = E.h_flex_frames(y, 1, max_bad=352, max_frames=4)
    assert cut[7] == 9 and cut[4].tolist() == starts[:4] and E.h_flex_frames(y, 1, max_bad=352, max_frames=0)[7] == 9
    n = len(y)
    parts = []
    for s0, s1 in ((0, 3), (3, 4), (4, 500), (500, n)):
        lo, hi = F.reach(s0, s1, n, 1)
        parts.append(E.h_flex_frames(y[lo:hi], 1, max_bad=352, buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
        ref = F.numpy_frames(y[lo:hi], 1, max_bad=352, buf_index0=lo, n_row=n, s_begin=s0, s_end=s1)
        assert all(same_bytes(a, b) for a, b in zip(parts[-1][:7], ref[:7]))
    for i in range(7):
        assert same_bytes(np.concatenate([q[i] for q in parts]), full[i]), i


def test_refusals_by_message():
    y = F.frame_row(0, 1, 10, 10 + F.FRAME_H)
    n = len(y)
    for why, kw in (("h outside [1, 64]", dict(h=0)), ("h outside [1, 64]", dict(h=65)), ("sync_errors outside [0, 3]", dict(sync_errors=4)),
                    ("fix outside [0, 2]", dict(fix=3)), ("max_bad outside [0, 352]", dict(max_bad=-1)), ("s_end < s_begin", dict(s_begin=5, s_end=4)),
                    ("the window does not lie inside the row", dict(s_end=n + 1)), ("max_frames < 0", dict(max_frames=-1)),
                    ("the buffer does not cover the window's reach (2 h - 1 starts either side, 5936 h samples forward)", dict(n_row=2 * n, s_end=20))):
        kw = dict(kw)
        with pytest.raises(ValueError, match=re.escape("pss_flex_frames: " + why)):
            E.h_flex_frames(y, kw.pop("h", 1), **kw)
    assert E.h_flex_frames(y, 1, s_begin=7, s_end=7)[7] == 0                        # an empty window is no refusal
    assert E.h_flex_frames(y, 1)[4].tolist() == [10]


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/flex_host.cpp: pss_flex.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a program
    of its own, rows in heap buffers of exactly their size."""
    exe = str(tmp_path / "flex_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "flex_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "flex_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

"""The RDS receiver's host twins (pss_h_rds_front, pss_h_resample, pss_h_rds_bits, pss_h_rds_groups), pss_rds_plan, pss_rds_default_pulse and
formats.rds_decode against tests/golden/rds.npz and the synthesiser of tests/rds_cases.py — no GPU.  The arithmetic is the project's own
(pyspecsdr_amd/csrc/pss_rds.h), so the truth is made outside it: NumPy builds the station's signal from the groups (checkwords,
differential coding, the shaping filter inverted numerically), and the receiver must hand the groups and the bits back.

  groups   every transmitted group but possibly the first and the last of the row comes back, in order, and nothing else does
  bits     the bit row equals the transmitted bits from the second one (the first has no symbol before it) to the last, at every clock
           offset and across the wraps of the timing offset, which the test locates with a NumPy restatement of the timing decision
  pulse    within PULSE_BOUND of the numerically inverted table (derived below from the inversion grid)
tests/test_gpu_rds.py (-m gpu) holds the kernels to the twins on every byte.  tests/rds_host.cpp runs the header alone under
AddressSanitizer and UBSan.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import rds_cases as R
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
GOLD = np.load(os.path.join(HERE, "golden", "rds.npz"))
NAMES = [str(n) for n in GOLD["names"]]

# The golden pulse is the trapezoid rule with h = 2 / 4096 on f(v) = cos(pi v / 4) cos(2 pi tau v), v in [0, 2], over the same rule on
# cos(pi v / 4) (= 4 / pi): |error| <= 2 h^2 / 12 max|f''| with |f''| <= (pi / 4 + 2 pi |tau|)^2 and |tau| <= 2.25 for the 65 taps, per
# value of g; a tap is the difference of two.  The table's grid holds the taps' instants exactly, so nothing is interpolated.
_H = 2.0 / 4096
PULSE_BOUND = 2 * (2 * _H ** 2 / 12 * (np.pi / 4 + 2 * np.pi * 2.25) ** 2) / (4 / np.pi) + 1e-7


def p(a):
    return None if a is None else a.ctypes.data


def test_goldens_are_the_synthesisers():
    assert NAMES == sorted(R.CASES)
    for name in NAMES:
        fs, ppm, sub, tune, side, n_groups, seed = R.CASES[name]
        assert GOLD[name + "/params"].tolist() == [fs, ppm, sub, tune, side, n_groups, seed]
        assert np.array_equal(GOLD[name + "/groups"], R.case_groups(name))
        assert np.array_equal(GOLD[name + "/bits"], R.data_bits(R.case_groups(name), seed))
    assert {R.CASES[n][0] for n in NAMES} == {240000, 250000, 400000, 1024000, 2400000}


@functools.lru_cache(maxsize=None)
def chain(name):
    """-> (iq, baseband at 19 kS/s, bit row, groups, pos) of a case through the host twins; made once and never changed."""
    iq, bits = R.case_iq(name)
    assert np.array_equal(bits, GOLD[name + "/bits"])
    fs = R.CASES[name][0]
    D, up, down = E.rds_plan(fs)
    bb = E.h_resample(E.h_rds_front(iq, fs, D), up, down)
    rx = E.h_rds_bits(bb)
    groups, pos, n = E.h_rds_groups(rx)
    assert n <= len(groups)
    for a in (iq, bb, rx, groups, pos):
        a.setflags(write=False)
    return iq, bb, rx, groups[:n], pos[:n]


@pytest.mark.parametrize("name", NAMES)
def test_groups_come_back(name):
    tx = GOLD[name + "/groups"]
    _, _, _, groups, pos = chain(name)
    idx = R.find_groups(tx, groups)
    assert idx is not None, "a group that was not transmitted"
    assert set(range(1, len(tx) - 1)) <= set(idx), (idx, len(tx))
    assert np.all(np.diff(pos) >= 104)


@pytest.mark.parametrize("name", NAMES)
def test_bits_come_back_without_a_slip(name):
    tx = GOLD[name + "/bits"]
    _, _, rx, groups, pos = chain(name)
    idx = R.find_groups(GOLD[name + "/groups"], groups)
    shift = R.PAD_BITS + 104 * idx[0] - int(pos[0])        # tx index = rx index + shift
    assert 1 - shift >= 0 and len(tx) - shift <= len(rx), "the bit row does not cover the transmitted bits"
    assert np.array_equal(rx[1 - shift:len(tx) - shift], tx[1:])


def wraps(offsets):
    """The steps of the timing offset that cross the wrap: +1 for 15 -> 0 (a strobe is dropped), -1 for 0 -> 15 (one is inserted)."""
    d = np.diff(np.asarray(offsets))
    return [int(np.sign(-v)) for v in d if abs(v) > 8]


def test_the_wrap_falls_inside_the_rows():
    pulse = E.rds_default_pulse()
    seen = {name: wraps(R.timing_offsets(chain(name)[1], pulse)) for name in NAMES}
    assert 1 in seen["fs240k_plain"] and -1 in seen["fs240k_plain"]          # noise alone toggles a row that sits on the wrap
    assert seen["fs400k_fast_clock"] == [-1] and seen["fs250k_slow_wrap"] == [1]   # the clock error carries these across, once


def test_rows_without_a_station():
    D, up, down = E.rds_plan(240000)
    for iq in (R.noise_row(60000), np.zeros(60000, np.complex64), R.noise_row(50), np.zeros(1, np.complex64)):
        bb = E.h_resample(E.h_rds_front(iq, 240000, D), up, down)
        rx = E.h_rds_bits(bb)
        assert E.h_rds_groups(rx)[2] == 0
    assert len(E.h_rds_bits(np.zeros(0, np.complex64))) == 0


def test_a_nan_in_the_row():
    name = "fs240k_plain"
    iq = chain(name)[0].copy()
    iq[len(iq) // 2] = np.nan
    D, up, down = E.rds_plan(240000)
    y = E.h_rds_front(iq, 240000, D)
    assert np.isnan(y.real).any() and not np.isnan(y.real[:100]).any()
    rx = E.h_rds_bits(E.h_resample(y, up, down))
    groups, _, n = E.h_rds_groups(rx)
    idx = R.find_groups(GOLD[name + "/groups"], groups[:n])
    assert idx is not None and 0 < len(idx) < 8                             # the groups the NaN does not reach, and no other
    # a row that is NaN from end to end: every comparison is false, the offset stays 0 and every bit reads 0
    rx = E.h_rds_bits(np.full(3000, np.nan, np.complex64))
    assert len(rx) == 3000 // 16 - 1 + (3000 % 16 > 0) and not rx.any()


def test_two_rows_of_one_batch_with_other_strides():
    lib = L.load()
    a, b = chain("fs240k_plain")[0][:30000], chain("fs240k_fast_clock")[0][:30000]
    D = 12
    taps = E.ddc_default_taps(D)
    m = 2500
    want = np.stack([E.h_rds_front(a, 240000, D), E.h_rds_front(b, 240000, D)])
    buf = np.full((2, 30011), np.nan, np.complex64)
    buf[0, :30000], buf[1, :30000] = a, b
    out = np.full((2, m + 3), 7 + 7j, np.complex64)
    assert lib.pss_h_rds_front(p(buf), 2, 30011, 30000, 0, 30000, 240000.0, D, p(taps), len(taps), 120, 0, m, p(out), m + 3) == 0
    assert np.array_equal(out[:, :m].view(np.uint32), want.view(np.uint32)) and np.all(out[:, m:] == 7 + 7j)
    bb = np.ascontiguousarray(out[:, :m])
    pulse = E.rds_default_pulse()
    wide = np.full((2, m + 9), np.nan, np.complex64)
    wide[:, :m] = bb
    bits, n_bits = np.zeros((2, 200), np.uint8), np.zeros(2, np.int32)
    assert lib.pss_h_rds_bits(p(wide), 2, m + 9, m, p(pulse), len(pulse), p(bits), 200, p(n_bits)) == 0
    for r in range(2):
        one = E.h_rds_bits(bb[r])
        assert n_bits[r] == len(one) and np.array_equal(bits[r, :len(one)], one)


def test_decode_names_the_station():
    d = F.rds_decode(chain("fs240k_plain")[3])
    assert d["pi"] == R.PI and d["ps"] == R.PS and d["radiotext"] == R.RADIOTEXT and d["pty"] == 10 and d["tp"] == 1
    assert d["group_counts"] == {"0A": 4, "2B": 1, "2A": 2, "0B": 1}
    d = F.rds_decode(R.station_groups()[:6])
    assert d["ps"] is None and d["radiotext"] == R.RADIOTEXT               # three of four name segments: no name yet
    d = F.rds_decode(R.station_groups()[:2])
    assert d["radiotext"] == "ab"                                           # the 2B text before the flag toggles
    g = R.station_groups()[3:4].copy()
    g[0, 2] = 0x0141                                                        # an unprintable character
    assert F.rds_decode(g)["radiotext"] == "?ADI"
    assert F.rds_decode(np.zeros((0, 4), np.uint16)) == {"pi": None, "pty": None, "tp": None, "group_counts": {}, "ps": None, "radiotext": None}


def test_default_pulse_is_the_inverted_spectrum():
    for span, key in ((4, "pulse"), (8, "pulse_span8")):
        got = E.rds_default_pulse(span)
        assert got.shape == GOLD[key].shape == (16 * span + 1,)
        if span == 4:
            assert np.abs(got - GOLD[key]).max() <= PULSE_BOUND < 2e-5
        assert np.array_equal(got, -got[::-1]) and got[8 * span] == 0.0
    assert np.array_equal(E.rds_default_pulse(8)[64 - 32:64 + 33], E.rds_default_pulse(4))
    lib, n = L.load(), C.c_int()
    for span in (0, 17):
        assert lib.pss_rds_default_pulse(span, None, C.byref(n)) == L.PSS_E_ARG
        assert lib.pss_last_error(None).startswith(b"pss_rds_default_pulse: span_bits outside [1, 16]")


def test_plan():
    want = {240000: (12, 19, 20), 250000: (13, 247, 250), 400000: (21, 399, 400), 1024000: (53, 1007, 1024), 2400000: (126, 399, 400),
            10000000: (204, 969, 2500), 200000: (10, 19, 20)}
    for fs, w in want.items():
        assert E.rds_plan(fs) == w
        D, up, down = w
        assert fs * up == 19000 * D * down                                  # fs / D up / down is 19 000 exactly
    for fs, why in ((240000.5, "fs must be an integer number of Hz"), (float("nan"), "fs must be an integer number of Hz"),
                    (120000, "fs must be above 120 000"), (96000, "fs must be above 120 000"), (1000003, "factors outside [1, 4096]")):
        with pytest.raises(ValueError, match=re.escape(why)) as e:
            E.rds_plan(fs)
        assert str(e.value).startswith("pss_rds: ")


def test_refusals_by_message():
    lib = L.load()
    iq, taps = np.zeros(100, np.complex64), np.ones(5)
    out = np.full(50, 3 + 3j, np.complex64)

    def front(why, n_rows=1, x_stride=100, n_buf=100, index0=0, n_cap=100, fs=240000.0, D=2, n_taps=5, lead=2, m0=0, m1=50, stride=50, t=taps, o=out):
        assert lib.pss_h_rds_front(p(iq), n_rows, x_stride, n_buf, index0, n_cap, fs, D, p(t), n_taps, lead, m0, m1, p(o), stride) == L.PSS_E_ARG
        assert lib.pss_last_error(None).decode() == "pss_h_rds_front: " + why
    front("fs must be finite and above 114 000 (the 57 kHz subcarrier below the discriminator's Nyquist)", fs=114000.0)
    front("decim outside [1, 4096]", D=0)
    front("n_taps outside [1, 4097]", n_taps=4098)
    front("n_rows < 1", n_rows=0)
    front("null taps", t=None)
    front("x_stride < n_buf", x_stride=99)
    front("lead outside [0, n_taps - 1]", lead=5)
    front("a tap that is not finite", t=np.array([1, 2, np.inf, 4, 5.0]))
    front("the buffer [buf_index0, buf_index0 + n_buf) is not inside the capture [0, n_capture)", n_cap=99)
    front("[m_begin, m_end) outside [0, ceil(n_capture / decim)]", m1=51)
    front("out_stride < m_end - m_begin", stride=49)
    front("null output", o=None)
    front("an output needs a sample of the capture that the buffer does not hold", n_cap=200, index0=0, m1=60, stride=60)
    # the discriminator's one sample more: outputs 10 .. need samples 18 ..., sample 18's discriminator reads sample 17
    front("an output needs a sample of the capture that the buffer does not hold", n_cap=200, index0=18, m0=10, m1=50, stride=40)
    assert lib.pss_h_rds_front(p(iq), 1, 100, 100, 17, 200, 240000.0, 2, p(taps), 5, 2, 10, 50, p(out), 40) == 0
    assert np.all(out[40:] == 3 + 3j)
    assert lib.pss_h_rds_front(None, 1, 0, 0, 0, 100, 240000.0, 2, p(taps), 5, 2, 7, 7, None, 0) == 0     # an empty window needs no buffers

    bb, pulse = np.zeros(64, np.complex64), E.rds_default_pulse()
    bits, nb = np.zeros(8, np.uint8), np.zeros(1, np.int32)

    def rbits(why, n_rows=1, stride=64, n=64, pl=pulse, n_pulse=65, b=bits, max_bits=8, cnt=nb, x=bb):
        assert lib.pss_h_rds_bits(p(x), n_rows, stride, n, p(pl), n_pulse, p(b), max_bits, p(cnt)) == L.PSS_E_ARG
        assert lib.pss_last_error(None).decode() == "pss_h_rds_bits: " + why
    rbits("n_rows < 1", n_rows=0)
    rbits("n outside [0, 2^30]", n=-1)
    rbits("n outside [0, 2^30]", n=2 ** 30 + 1, stride=2 ** 30 + 1)
    rbits("row_stride < n", stride=63)
    rbits("max_bits outside [0, 2^30]", max_bits=-1)
    rbits("n_pulse must be odd and in [1, 257]", n_pulse=64)
    rbits("n_pulse must be odd and in [1, 257]", n_pulse=259)
    rbits("n_pulse must be odd and in [1, 257]", pl=None)
    rbits("a pulse tap that is not finite", pl=np.full(65, np.nan))
    rbits("null buffer", cnt=None)
    rbits("null buffer", x=None)
    rbits("null buffer", b=None)

    g, pos, ng = np.zeros((2, 4), np.uint16), np.zeros(2, np.int32), np.zeros(1, np.int32)

    def rgroups(why, b=bits, cnt=nb, n_rows=1, max_bits=8, gg=g, pp=pos, max_groups=2, n=ng):
        assert lib.pss_h_rds_groups(p(b), p(cnt), n_rows, max_bits, p(gg), p(pp), max_groups, p(n)) == L.PSS_E_ARG
        assert lib.pss_last_error(None).decode() == "pss_h_rds_groups: " + why
    rgroups("n_rows < 1", n_rows=0)
    rgroups("max_bits outside [0, 2^30]", max_bits=-1)
    rgroups("max_groups < 0", max_groups=-1)
    for kw in (dict(b=None), dict(cnt=None), dict(gg=None), dict(pp=None), dict(n=None)):
        rgroups("null buffer", **kw)


def test_front_rows_do_not_depend_on_the_cut():
    iq = chain("fs250k_slow_clock")[0][:40000]
    fs, D = 250000, 13
    taps = E.ddc_default_taps(D)
    T, lead = len(taps), (len(taps) - 1) // 2
    whole = E.h_rds_front(iq, fs, D)
    n = len(iq)

    def window(m0, m1):
        lo, hi = max(0, m0 * D + lead - (T - 1) - 1), min(n, (m1 - 1) * D + lead + 1)
        return E.h_rds_front(iq[lo:hi], fs, D, taps=taps, buf_index0=lo, n_capture=n, m_begin=m0, m_end=m1)
    cuts = [0, 1, 9, 10, 11, 1000, 1001, len(whole) - 1, len(whole)]    # 10 D + lead - (T - 1) = 0: windows that start inside the halo
    got = np.concatenate([window(a, b) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    # a row of more than 2^40 samples of which the buffer holds the last 40 000: any cut of it, the same bytes
    big = 2 ** 40 + 12345
    index0 = big - n
    m_lo = -(-(index0 + 1 + (T - 1) - lead) // D)
    m_hi = -(-big // D)
    far = E.h_rds_front(iq, fs, D, taps=taps, buf_index0=index0, n_capture=big, m_begin=m_lo, m_end=m_hi)
    mid = (m_lo + m_hi) // 2

    def far_window(m0, m1):
        lo, hi = max(index0, m0 * D + lead - (T - 1) - 1), min(big, (m1 - 1) * D + lead + 1)
        return E.h_rds_front(iq[lo - index0:hi - index0], fs, D, taps=taps, buf_index0=lo, n_capture=big, m_begin=m0, m_end=m1)
    parts = np.concatenate([far_window(m_lo, mid), far_window(mid, mid + 1), far_window(mid + 1, m_hi)])
    assert np.array_equal(parts.view(np.uint32), far.view(np.uint32))
    k = len(far) // 2
    assert not np.array_equal(far[k:k + 50], whole[k:k + 50])             # the phase follows the index in the row


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/rds_host.cpp: pss_rds.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "rds_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "rds_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rds_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_header_table_and_library_agree_on_the_new_entry_points():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in ("pss_rds_plan", "pss_rds_front", "pss_h_rds_front", "pss_rds_default_pulse", "pss_rds_bits", "pss_h_rds_bits", "pss_rds_groups",
                 "pss_h_rds_groups"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    units = __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS
    assert ("pss_rds.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]) in units
    import pyspecsdr_amd.signal_processing as sp
    assert callable(sp.extract_rds) and callable(sp.demodulate_rds_bpsk)

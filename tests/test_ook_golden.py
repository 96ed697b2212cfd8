"""The OOK receiver's host side — pss_ook_halo, pss_h_ook_envelope, pss_h_ook_levels, pss_h_ook_messages, formats.ook_spec / ook_levels /
ook_records / ook_messages / ook_decode / ook_lines / h_ook_rows — against tests/golden/ook.npz and the NumPy statement of the rules in
tests/ook_cases.py — no GPU.  The arithmetic is the project's own (pyspecsdr_amd/csrc/pss_ook.h) and the reference holds no OOK code, so the
truth is made outside the library: NumPy keys the bursts and restates the envelope, the levels, the state, the edges, the messages and the
slicers with array operations; the twin must agree with it byte for byte, stage by stage, and hand back exactly the copies that were sent.
tests/test_gpu_ook.py (-m gpu) holds the kernels to the twin on every byte.  tests/ook_host.cpp runs the header alone under AddressSanitizer
and UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest

import ook_cases as K
from bytes_util import same_bytes
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
GOLD = np.load(os.path.join(HERE, "golden", "ook.npz"))
SYMBOLS = ("pss_ook_halo", "pss_ook_envelope", "pss_h_ook_envelope", "pss_ook_levels", "pss_h_ook_levels", "pss_ook_messages", "pss_h_ook_messages")
WHAT = ("bits", "n_bits", "row", "pos", "span", "meta")


def p(a):
    return None if a is None else a.ctypes.data


def both(x, hi, lo, spec, P=9, R=64, **kw):
    """The twin and the NumPy statement agree on every record -> the twin's result."""
    twin = E.h_ook_messages(x, hi, lo, spec, P=P, R=R, **kw)
    ref = K.messages(x, hi, lo, spec, P, R, kw.get('s_begin', 0), kw.get('s_end'))
    for t, r, what in zip(twin[:6], ref, WHAT):
        assert same_bytes(t, r), (what, t, r)
    assert twin[6] == len(ref[0])
    return twin


def test_symbols_are_declared_exported_and_in_the_table():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    for name, value in (("PSS_OOK_PWM", "0"), ("PSS_OOK_PPM", "1"), ("PSS_OOK_MC", "2"), ("PSS_OOK_MAX_PULSES", "1024"), ("PSS_OOK_MAX_BITS", "256"),
                        ("PSS_OOK_OPEN", "(1u << 22)"), ("PSS_OOK_LONG", "(1u << 23)"), ("PSS_OOK_MANY", "(1u << 24)"), ("PSS_OOK_FULL", "(1u << 25)")):
        assert f"#define {name} {value}\n" in txt, name
    assert (E.OOK_PWM, E.OOK_PPM, E.OOK_MC, E.OOK_OPEN, E.OOK_LONG, E.OOK_MANY, E.OOK_FULL) == (K.PWM, K.PPM, K.MC, K.OPEN, K.LONG, K.MANY, K.FULL)
    units = __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS
    assert ("pss_ook.hip", ["-ffp-contract=off"]) in units
    for name in ("ook_halo", "ook_envelope", "ook_levels", "ook_messages", "h_ook_envelope", "h_ook_levels", "h_ook_messages"):
        assert callable(getattr(E, name))
    for name in ("ook_spec", "ook_levels", "ook_records", "ook_messages", "ook_decode", "ook_lines", "ook_rows", "h_ook_rows", "ook_recording"):
        assert callable(getattr(F, name))


def test_goldens_are_the_generators():
    rows, _, _ = K.small_rows()
    assert K.crc(rows) == int(GOLD["small_crc"])
    assert [K.crc(c['rows']) for c in K.shape_cases()] == GOLD["cases_crc"].tolist()
    assert [str(n) for n in GOLD["names"]] == [f"{kind}{snr}" for kind, snr, _ in K.FIXTURES]


@pytest.mark.parametrize("P", [1, 2, 9, 64, 65])
def test_envelope_and_levels_stage_by_stage(P):
    rows, _, _ = K.small_rows()
    x = np.concatenate([rows, K.level_row(rows.shape[1], 3)[None, :]])
    env = E.h_ook_envelope(x, P=P)
    means = E.h_ook_levels(x)
    for k in range(len(x)):
        m = K.magnitude(x[k])
        assert same_bytes(env[k], K.envelope(m, P)) and same_bytes(means[k], K.block_means(m))
    # windows of both: any split concatenates to the whole row's bytes, each buffer holding exactly its reach
    n = x.shape[1]
    cuts = sorted({0, 1, P - 1, P, 4095, 4096, 4097, 9000, n})
    parts = [E.h_ook_envelope(x[:, max(0, a - (P - 1)):b], P=P, buf_index0=max(0, a - (P - 1)), n_row=n, i_begin=a, i_end=b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert same_bytes(np.concatenate(parts, axis=1), env)
    parts = [E.h_ook_levels(x[:, b * K.BLOCK:(b + 1) * K.BLOCK], buf_index0=b * K.BLOCK, n_row=n, b_begin=b, b_end=b + 1) for b in range(n // K.BLOCK)]
    assert same_bytes(np.concatenate(parts, axis=1), means)
    if P > 1:
        with pytest.raises(ValueError, match=r"pss_ook_envelope: the buffer does not cover the window's reach \(P - 1 samples back\)"):
            E.h_ook_envelope(x[:, 5001 - (P - 1):6000], P=P, buf_index0=5001 - (P - 1), n_row=n, i_begin=5000, i_end=6000)


def test_levels_are_the_lower_quartile():
    means = np.array([5.0, 1.0, 9.0, 2.0, 7.0, 3.0, 8.0, 4.0])
    hi, lo = F.ook_levels(means)
    assert (hi, lo) == (np.float32(24.0), np.float32(12.0)) and hi.dtype == np.float32      # sorted[8 // 4] = 3
    assert F.ook_levels(means, hi_ratio=2.5, lo_ratio=1.5, quantile=0.5) == (np.float32(12.5), np.float32(7.5))
    assert F.ook_levels(means[:1]) == (np.float32(40.0), np.float32(20.0))
    assert F.ook_levels(means) == K.levels(means)
    with pytest.raises(ValueError, match="no whole block"):
        F.ook_levels([])


@pytest.mark.parametrize("k", range(len(K.SMALL_SPECS)))
def test_small_rows_twin_is_the_statement_and_the_golden(k):
    rows, hi, lo = K.small_rows()
    twin = both(rows, hi, lo, K.SMALL_SPECS[k])
    assert twin[6] > 0
    for t, what in zip(twin[:6], WHAT):
        assert same_bytes(t, GOLD[f"small{k}_{what}"]), what
    # the NaN and inf samples of row 2 are there and change nothing but their own neighbourhood
    assert np.isnan(rows[2]).sum() == 2 and np.isinf(rows[2]).sum() == 1


@pytest.mark.parametrize("kind,snr,seed", K.FIXTURES, ids=[f"{f[0]}{f[1]}" for f in K.FIXTURES])
def test_fixtures_every_copy_and_nothing_else(kind, snr, seed):
    """8 000 000 samples at 250 kS/s, 30 transmissions of 3 copies: every sent copy is reported exactly, and no other record of 16 bits or
    more.  The inputs are pinned by their CRC-32; the thresholds come from the lower quartile of the block means."""
    name = f"{kind}{snr}"
    x, sent, spec = K.burst_fixture(kind, snr, seed)
    assert K.crc(x) == int(GOLD[name + "_crc"]) and np.array_equal(np.array(sent, np.uint8), GOLD[name + "_sent"])
    means = E.h_ook_levels(x)[0]
    assert K.crc(means) == int(GOLD[name + "_means_crc"]) and same_bytes(means, K.block_means(K.magnitude(x)))
    hi, lo = F.ook_levels(means)
    assert same_bytes(np.array([hi, lo]), GOLD[name + "_levels"])
    twin = both(x, hi, lo, spec)
    for t, what in zip(twin[:6], WHAT):
        assert same_bytes(t, GOLD[f"{name}_{what}"]), what
    assert spec['min_bits'] == 16 and twin[6] == 90
    assert [K.bits_of(b, n) for b, n in zip(twin[0], twin[1])] == sent
    assert np.all(twin[5] >> 11 == 0) and np.all((twin[5] & 0x7FF) == (37 if kind == 'ppm' else 24))     # no odd symbol, no flag, every pulse
    # the other slicer finds nothing of 16 bits in it, and the same noise without a carrier gives no record at all
    other = dict(K.PWM_SPEC if kind == 'ppm' else K.PPM_SPEC)
    assert E.h_ook_messages(x, hi, lo, other)[6] == 0
    if snr == 15:
        noise = K.burst_fixture(kind, snr, seed, n=4_000_000, n_tx=0)[0]
        assert E.h_ook_messages(noise, hi, lo, dict(spec, min_bits=0, max_odd=2047))[6] == 0


def test_spec_strings():
    s = F.ook_spec("n=nexus,m=OOK_PPM,s=1000,l=2000,g=3000,r=5000,bits>=36", 250e3)
    assert (s['name'], s['mode'], s['short'], s['long'], s['gap_limit'], s['reset'], s['min_bits'], s['tol'], s['sync'], s['invert'], s['phase']) == \
        ('nexus', K.PPM, 250, 500, 750, 1250, 36, 62, 0, 0, 0)                                # the default tolerance: a quarter of s
    s = F.ook_spec(F.OOK_DEVICES['ev1527'], 250e3)
    assert (s['mode'], s['short'], s['long'], s['gap_limit'], s['tol'], s['reset'], s['min_bits']) == (K.PWM, 88, 264, 600, 40, 3000, 24)
    s = F.ook_spec("m=OOK_MC_ZEROBIT, s=100, t=30, y=777, invert", 1e6)
    assert (s['mode'], s['short'], s['tol'], s['sync'], s['invert'], s['phase'], s['name']) == (K.MC, 100, 30, 777, 1, 1, '')
    assert F.ook_spec("m=OOK_PWM,s=333,l=666", 2.4e6)['short'] == int(round(333 * 2.4e6 / 1e6)) == 799
    for bad, why in (("m=OOK_PWM,s=1,l=2,q=3", "unknown key 'q'"), ("m=FSK_PCM,s=1,l=2", "unknown modulation 'FSK_PCM'"), ("s=1,l=2", "m= and s= are needed"),
                     ("m=OOK_PWM,s=5", "l= is needed"), ("m=OOK_PWM,s=1,l=2,bogus", "unknown key 'bogus'")):
        with pytest.raises(ValueError, match=re.escape("ook_spec: " + why)):
            F.ook_spec(bad, 250e3)
    assert sorted(F.OOK_DEVICES) == ['ev1527', 'nexus']


def nexus_bits(ident, battery, channel, tenths, humidity):
    word = ident << 28 | battery << 27 | (channel - 1) << 24 | (tenths & 0xFFF) << 12 | 0xF << 8 | humidity
    return [(word >> (35 - k)) & 1 for k in range(36)]


def test_decode_on_written_out_bit_patterns():
    bits = [int(c) for c in "10100101" "1" "0" "10" "000011100110" "1111" "00101101"]
    assert F.ook_decode('nexus', bits) == dict(model='nexus', id=0xA5, battery_ok=1, channel=3, temperature_c=23.0, humidity=45)
    for channel in (1, 2, 3, 4):
        for battery in (0, 1):
            for tenths in (-1, -400, -2048, 0, 2047, 215):                                   # negative temperatures: two's complement in 12 bits
                d = F.ook_decode('nexus', nexus_bits(0x3C, battery, channel, tenths, 99))
                assert (d['id'], d['battery_ok'], d['channel'], d['temperature_c'], d['humidity']) == (0x3C, battery, channel, tenths / 10.0, 99)
    broken = list(bits)
    broken[9] = 1
    assert F.ook_decode('nexus', broken) == dict(model='nexus', n_bits=36, hex="a5e0e6f2d0")
    assert F.ook_decode('nexus', bits[:35])['hex'] == "a5a0e6f2c"[:0] + bytes(F._ook_field(bits[:35] + [0] * 5, k, k + 8) for k in range(0, 40, 8)).hex()
    ev = [int(c) for c in "1011" "0000" "1111" "0101" "0011" "0100"]
    assert F.ook_decode('ev1527', ev) == dict(model='ev1527', id=0xB0F53, buttons=0b0100)
    assert F.ook_decode('ev1527', ev[:23])['model'] == 'ev1527' and 'id' not in F.ook_decode('ev1527', ev[:23])
    assert F.ook_decode('other', [1, 0, 1]) == dict(model='other', n_bits=3, hex="a0")


def test_repeats_are_joined_and_lines():
    rec = lambda row, pos, span, bits: dict(bits=list(bits), n_bits=len(bits), row=row, pos=pos, span=span, n_pulses=len(bits), n_odd=0, flags=[], hex="")  # noqa: E731
    a, b = [1, 0, 1, 1], [1, 0, 1, 0]
    # reset 100 us at 1 MS/s = 100 samples from a copy's END to the next copy's start
    records = [rec(0, 1000, 50, a), rec(0, 1151, 50, a), rec(0, 1301, 50, a), rec(0, 1400, 50, b), rec(1, 1460, 50, b), rec(0, 1500, 50, b), rec(0, 900, 10, a)]
    m = F.ook_messages(records, 1e6, 100)
    assert [(x['row'], x['pos'], x['count'], x['span'], x['bits']) for x in m] == \
        [(0, 900, 2, 150, a), (0, 1151, 2, 200, a), (0, 1400, 2, 150, b), (1, 1460, 1, 50, b)]     # 100 samples join, 101 do not
    assert m[0]['time'] == 900 / 1e6
    got = F.h_ook_rows(np.stack(K.small_rows()[0]), K.FS, specs=["n=ppm,m=OOK_PPM,s=1000,l=2000,g=3000,t=240", "n=pwm,m=OOK_PWM,s=352,l=1056,g=2400,t=160"])
    assert [r['name'] for r in got['records']] == sorted([r['name'] for r in got['records']]) and len(got['lines']) == len(got['messages']) > 0
    assert all(re.fullmatch(r" *\d+\.\d{4} s  row \d  (ppm|pwm): \d+ bits [0-9a-f]*  x\d+", ln) for ln in got['lines']), got['lines']
    lines = F.ook_lines([dict(time=1.5, row=0, name='nexus', count=3, fields=F.ook_decode('nexus', nexus_bits(7, 1, 2, -35, 40))),
                         dict(time=2.0, row=1, name='ev1527', count=1, fields=dict(model='ev1527', id=0xB0F53, buttons=4))])
    assert lines == ["    1.5000 s  row 0  nexus: id 7 channel 2 battery ok temperature -3.5 C humidity 40 %  x3",
                     "    2.0000 s  row 1  ev1527: id b0f53 buttons 0100  x1"]


def test_windows_do_not_change_a_byte():
    rows, hi, lo = K.small_rows()
    x = np.concatenate([rows, K.level_row(rows.shape[1], 11, 40)[None, :] * np.float32(0.7)])
    n = x.shape[1]
    for spec, R in ((K.SMALL_SPECS[0], 64), (K.SMALL_SPECS[1], 0), (dict(K.SMALL_SPECS[2], span=700), 300), (dict(K.PWM_S, span=100), 5)):
        whole = both(x, hi, lo, spec, R=R)
        assert whole[6] > 3
        before, after = E.ook_halo(9, R, spec['gap_limit'], spec['span'])
        assert (before, after) == (spec['gap_limit'] + R + 9, spec['span'])
        for cuts in ([100, 150, 3396, K.TILE - 1, K.TILE, K.TILE + 10], [K.TILE + 7, 2 * K.TILE + 16, n - 1], [1], list(range(500, n, 777))):
            ends = [0] + cuts + [n]
            parts = []
            for s0, s1 in zip(ends[:-1], ends[1:]):
                b0, b1 = max(0, s0 - before), min(n, s1 + after)                  # exactly the window's reach
                parts.append(E.h_ook_messages(x[:, b0:b1], hi, lo, spec, R=R, buf_index0=b0, n_row=n, s_begin=s0, s_end=s1))
                if b0 > 0:
                    with pytest.raises(ValueError, match="the buffer does not cover the window's reach"):
                        E.h_ook_messages(x[:, b0 + 1:b1], hi, lo, spec, R=R, buf_index0=b0 + 1, n_row=n, s_begin=s0, s_end=s1)
                if b1 < n:
                    with pytest.raises(ValueError, match="the buffer does not cover the window's reach"):
                        E.h_ook_messages(x[:, b0:b1 - 1], hi, lo, spec, R=R, buf_index0=b0, n_row=n, s_begin=s0, s_end=s1)
            order = np.lexsort((np.concatenate([q[3] for q in parts]), np.concatenate([q[2] for q in parts])))
            for i in range(6):
                assert same_bytes(np.concatenate([q[i] for q in parts])[order], whole[i]), (cuts, i)


def test_refusals_by_message():
    lib = L.load()
    x = K.small_rows()[0][0]
    n = len(x)
    bits, nb, rw, pos = np.zeros((4, 32), np.uint8), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.int64)
    sp, meta, count = np.zeros(4, np.int32), np.zeros(4, np.uint32), np.full(1, -7, np.int32)
    ok = dict(x=p(x), n_rows=1, stride=n, n_buf=n, index0=0, n_row=n, s0=0, s1=n, P=9, hi=2.0, lo=1.0, R=64, gap=750, span=65536, mode=K.PWM, short=88, long=264,
              sync=0, tol=40, phase=0, invert=0, min_bits=0, max_odd=2047, bits=p(bits), nb=p(nb), row=p(rw), pos=p(pos), sp=p(sp), meta=p(meta), count=p(count),
              max_msgs=4)
    order = ("x", "n_rows", "stride", "n_buf", "index0", "n_row", "s0", "s1", "P", "hi", "lo", "R", "gap", "span", "mode", "short", "long", "sync", "tol", "phase",
             "invert", "min_bits", "max_odd", "bits", "nb", "row", "pos", "sp", "meta", "count", "max_msgs")

    def refused(why, **kw):
        a = dict(ok, **kw)
        r = lib.pss_h_ook_messages(*[a[k] for k in order])
        assert r == L.PSS_E_ARG and lib.pss_last_error(None).decode() == "pss_ook_messages: " + why, lib.pss_last_error(None).decode()
        assert count[0] == -7 and not bits.any() and not nb.any()
    refused("n_row outside [0, 2^60]", n_row=-1)
    refused("the buffer does not lie inside the row", n_row=n - 1)
    refused("the buffer does not lie inside the row", index0=-1)
    refused("s_end < s_begin", s0=10, s1=9)
    refused("the window does not lie inside the row", s1=n + 1)
    refused("a window of more than 2^30 starts", n_row=1 << 40, s1=(1 << 30) + 1)
    refused("n_rows outside [1, 2^20]", n_rows=0)
    refused("n_rows outside [1, 2^20]", n_rows=(1 << 20) + 1)
    refused("x_stride < n_buf", stride=n - 1)
    refused("null buffer", x=None)
    refused("a misaligned pointer", x=p(x) + 4)
    refused("P outside [1, 65]", P=0)
    refused("P outside [1, 65]", P=66)
    refused("R outside [0, 4096]", R=-1)
    refused("R outside [0, 4096]", R=4097)
    refused("the thresholds must satisfy hi >= lo > 0", hi=0.5)
    refused("the thresholds must satisfy hi >= lo > 0", lo=0.0)
    refused("the thresholds must satisfy hi >= lo > 0", hi=float("nan"))
    refused("gap_limit outside [1, 2^20]", gap=0)
    refused("gap_limit outside [1, 2^20]", gap=(1 << 20) + 1)
    refused("span outside [1, 2^24]", span=0)
    refused("span outside [1, 2^24]", span=(1 << 24) + 1)
    refused("mode is none of PSS_OOK_PWM, PSS_OOK_PPM, PSS_OOK_MC", mode=3)
    refused("tol outside [0, 2^24]", tol=-1)
    refused("short outside [1, 2^24]", short=0)
    refused("long outside [1, 2^24]", long=0)
    refused("sync outside [0, 2^24]", sync=-1)
    refused("phase outside {0, 1}", phase=2)
    refused("invert outside {0, 1}", invert=2)
    refused("min_bits outside [0, 256]", min_bits=257)
    refused("max_odd outside [0, 2047]", max_odd=2048)
    refused("short, long and sync are not more than 2 tol apart", tol=88)
    refused("short, long and sync are not more than 2 tol apart", sync=300)
    refused("short and 2 short are not more than 2 tol apart", mode=K.MC, tol=44)
    refused("more than 2^31 edge positions in the rows of one call", n_rows=3, n_row=1 << 40, s1=1 << 30)
    refused("max_msgs < 0", max_msgs=-1)
    refused("null buffer", count=None)
    refused("null buffer", bits=None)
    refused("null buffer", sp=None)
    refused("a misaligned pointer", pos=p(pos) + 4)
    refused("a misaligned pointer", count=p(count) + 2)
    reach = "the buffer does not cover the window's reach (gap_limit + R + P samples back, span samples forward)"
    refused(reach, n_row=1 << 20, s1=100)                                                 # the window's last start reads span ahead
    refused(reach, index0=50, n_row=n + 50, s0=60, s1=61)                                 # and gap_limit + R + P back
    assert lib.pss_h_ook_messages(*[ok[k] for k in order]) == 0 and count[0] == 1 and nb[0] == 12 and pos[0] == K.TILE - 700 + 1     # e reaches hi = 2 with the second keyed sample: 2 * 16 / 9
    assert E.h_ook_messages(x, 2.0, 1.0, K.PWM_SPEC, s_begin=7, s_end=7)[6] == 0          # an empty window is no refusal
    assert lib.pss_h_ook_messages(*[dict(ok, mode=K.MC, long=0, tol=43)[k] for k in order]) == 0     # Manchester reads neither long nor sync
    for call, name in ((lambda: E.ook_halo(0, 64, 750, 100), "pss_ook_halo: P outside [1, 65]"), (lambda: E.ook_halo(9, 4097, 750, 100), "pss_ook_halo: R outside [0, 4096]"),
                       (lambda: E.ook_halo(9, 64, 0, 100), "pss_ook_halo: gap_limit outside [1, 2^20]"), (lambda: E.ook_halo(9, 64, 750, 0), "pss_ook_halo: span outside [1, 2^24]"),
                       (lambda: E.h_ook_envelope(x, P=66), "pss_ook_envelope: P outside [1, 65]"),
                       (lambda: E.h_ook_envelope(x, i_begin=5, i_end=4), "pss_ook_envelope: i_end < i_begin"),
                       (lambda: E.h_ook_levels(x, b_end=4), "pss_ook_levels: the window does not lie inside the row's whole blocks"),
                       (lambda: E.h_ook_levels(x, b_begin=2, b_end=1), "pss_ook_levels: b_end < b_begin"),
                       (lambda: E.h_ook_levels(x[:5000], buf_index0=100, n_row=9000, b_begin=0, b_end=1), "pss_ook_levels: the buffer does not cover the window's blocks")):
        with pytest.raises(ValueError, match=re.escape(name)):
            call()
    assert E.ook_halo(65, 4096, 1 << 20, 1 << 24) == ((1 << 20) + 4096 + 65, 1 << 24)


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/ook_host.cpp: pss_ook.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a program
    of its own; rows and windows sit in heap buffers of exactly their stated size."""
    exe = str(tmp_path / "ook_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "ook_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ook_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

"""The POCSAG receiver's host side — pss_pocsag_plan, pss_pocsag_default_pulse, pss_pocsag_codeword, pss_pocsag_check, pss_h_pocsag_batches,
formats.pocsag_messages / pocsag_lines — against published constants, tests/golden/pocsag.npz and the NumPy statement of the rules in
tests/pocsag_cases.py — no GPU.  The arithmetic is the project's own (pyspecsdr_amd/csrc/pss_pocsag.h) and the reference holds no POCSAG
code, so the truth is made outside the library: NumPy builds the transmissions from the messages and restates the candidate, walk, check,
accept and one-record rules; the twin must agree with it record for record, and hand back exactly the injected messages.
tests/test_gpu_pocsag.py (-m gpu) holds the kernels to the twin on every byte.  tests/pocsag_host.cpp runs the header alone under
AddressSanitizer and UBSan."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import pocsag_cases as P
from bytes_util import same_bytes
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
GOLD = np.load(os.path.join(HERE, "golden", "pocsag.npz"))
NAMES = [str(n) for n in GOLD["names"]]
SYMBOLS = ("pss_pocsag_plan", "pss_pocsag_default_pulse", "pss_pocsag_codeword", "pss_pocsag_check", "pss_pocsag_batches", "pss_h_pocsag_batches")
WHAT = ("cw", "fix", "row", "pos", "meta", "score")
SPB = 16
AT = 50
N = AT + 544 * SPB + 20


def p(a):
    return None if a is None else a.ctypes.data


def both(y, spb, **kw):
    """The twin and the NumPy statement agree on every record -> the twin's result."""
    twin = E.h_pocsag_batches(y, spb, **kw)
    ref = P.numpy_batches(y, spb, **kw)
    for t, r, what in zip(twin[:6], ref[:6], WHAT):
        assert same_bytes(t, r), (what, t, r)
    assert twin[6] == ref[6]
    return twin


def run(flips=(), spb=SPB, **kw):
    return both(P.batch_row(spb, AT, AT + 544 * spb + 20, flips=flips), spb, **kw)


def test_symbols_are_declared_exported_and_in_the_table():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    units = __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS
    assert ("pss_pocsag.hip", ["-ffp-contract=off"]) in units
    for name in ("pocsag_plan", "pocsag_default_pulse", "pocsag_codeword", "pocsag_check", "pocsag_batches", "h_pocsag_batches"):
        assert callable(getattr(E, name))
    for name in ("pocsag_messages", "pocsag_lines", "pocsag_rows", "pocsag_recording", "pocsag_records"):
        assert callable(getattr(F, name))


def test_constants_of_the_code():
    assert E.pocsag_codeword(0x7CD215D8 >> 11) == 0x7CD215D8 == P.codeword(0x7CD215D8 >> 11)
    assert E.pocsag_codeword(0x7A89C197 >> 11) == 0x7A89C197 == P.codeword(0x7A89C197 >> 11)
    assert P.address_word(1234567, 3) == 0x4B5A1A25 == E.pocsag_codeword((1234567 >> 3) << 2 | 3) and 1234567 & 7 == 7
    rng = np.random.default_rng(1)
    for d in rng.integers(0, 1 << 21, 500).tolist():
        assert E.pocsag_codeword(d) == P.codeword(d)
    lib = L.load()
    assert lib.pss_pocsag_check(0x7CD215D8, 2, None) == 0 and lib.pss_pocsag_check(0x7CD215D8, 3, None) == -1 and lib.pss_pocsag_check(0x7CD215D8, -1, None) == -1


def test_check_on_every_single_double_and_triple_error():
    for cw in (0x7CD215D8, 0x7A89C197, 0x4B5A1A25):
        assert E.pocsag_check(cw, 0) == (0, cw)
        for i in range(32):
            assert E.pocsag_check(cw ^ 1 << i, 2) == (1, cw) == E.pocsag_check(cw ^ 1 << i, 1) and E.pocsag_check(cw ^ 1 << i, 0) == (-1, 0)
        for i, j in itertools.combinations(range(32), 2):
            hurt = cw ^ 1 << i ^ 1 << j
            assert E.pocsag_check(hurt, 2) == (2, cw) and E.pocsag_check(hurt, 1) == (-1, 0) == E.pocsag_check(hurt, 0)
        refused = 0
        for i, j, k in itertools.combinations(range(32), 3):
            hurt = cw ^ 1 << i ^ 1 << j ^ 1 << k
            n, out = E.pocsag_check(hurt, 2)
            assert (n, out) == P.check(hurt, 2)
            if n < 0:
                refused += 1
                assert out == 0
            else:                                               # another valid codeword, at most two bits from what was received
                assert out != cw and P.remainder31(out >> 1) == 0 and bin(out).count("1") % 2 == 0 and bin(out ^ hurt).count("1") == n
        assert refused == 4960      # the code with its parity bit has distance 6: three wrong bits lie three or more from every codeword


def test_plan_and_pulse():
    assert E.pocsag_plan(2.4e6) == (62, 124, 125) and E.pocsag_plan(250e3) == (6, 576, 625) and E.pocsag_plan(38400) == (1, 1, 1)
    assert E.pocsag_plan(240e3) == (6, 24, 25) and E.pocsag_plan(50e3) == (1, 96, 125)
    for fs, why in ((38400.5, "fs must be an integer number of Hz"), (float("nan"), "fs must be an integer number of Hz"),
                    (38399.0, "fs must be at least 38 400"), (-1.0, "fs must be at least 38 400"),
                    (1000003.0, "38 400 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take")):
        with pytest.raises(ValueError, match="^" + re.escape("pss_pocsag: " + why)):
            E.pocsag_plan(fs)
    for spb, taps in ((75, 65), (32, 31), (16, 15), (2, 1), (3, 3), (128, 65), (65, 65), (66, 65), (64, 63)):
        g = E.pocsag_default_pulse(spb)
        assert len(g) == taps == P.pulse_len(spb) and np.all(g == 1.0 / taps)
    for spb in (1, 0, 129, -3):
        with pytest.raises(ValueError, match=re.escape("pocsag_default_pulse: spb outside [2, 128]")):
            E.pocsag_default_pulse(spb)


def test_goldens_are_the_synthesisers():
    assert NAMES == sorted(P.CASES)
    for name in NAMES:
        assert P.row_crc32(P.case_row(name)) == int(GOLD[name + "/crc32"][0])


@pytest.mark.parametrize("name", NAMES)
def test_twin_is_the_numpy_statement_and_the_golden_and_recovers_the_messages(name):
    baud, _, inverted, messages = P.CASES[name]
    spb = P.SPB[baud]
    y = P.case_row(name)
    r = both(y, spb)
    for got, what in zip((r[0], r[3], r[4], r[5]), ("cw", "pos", "meta", "score")):
        assert same_bytes(got, GOLD[name + "/" + what]), what
    n_batches, first = P.case_batches(name)
    # every injected batch with n_bad = 0 (and nothing to fix), each within half a bit of where it was put, nothing else
    assert r[6] == n_batches and not r[1].any() and not r[2].any() and np.all(r[4] == int(inverted) << 8)
    assert all(2 * abs(q - (first + 544 * spb * k)) <= spb for k, q in enumerate(r[3].tolist()))
    assert r[0].reshape(-1).tolist() == [w for b in P.batches_of(messages) for w in b]
    stats = {}
    msgs = F.pocsag_messages(F.pocsag_records(*r[:6]), spb, stats=stats)
    assert P.reported(msgs) == P.expected(messages, baud) and stats == {"orphans": 0}
    assert all(m["baud"] == baud and m["row"] == 0 and m["fixed"] == 0 and not m["damaged"] for m in msgs)
    assert [m["pos"] for m in msgs] == sorted(m["pos"] for m in msgs)
    for other in (16, 32, 75):                                  # and nothing at the other rates
        if other != spb:
            assert E.h_pocsag_batches(y, other)[6] == 0


def test_lines_and_message_rules():
    assert F.pocsag_lines([dict(baud=1200, ric=1234567, function=3, bits=20, numeric="", alpha="Hi")]) == \
        ["POCSAG1200: Address: 1234567  Function: 3  Alpha:   Hi"]
    assert F.pocsag_lines([dict(baud=512, ric=7, function=0, bits=20, numeric="12345", alpha="?"), dict(baud=2400, ric=8, function=1, bits=0, numeric="", alpha="")]) == \
        ["POCSAG512: Address:       7  Function: 0  Numeric: 12345", "POCSAG2400: Address:       8  Function: 1"]
    # two batches chained, a damaged message, an orphan, two slicings of one batch, a batch of the other polarity that does not continue
    spb = 32
    a = [P.IDLE] * 16
    a[14:16] = P.message_words(1234567, 3, "abcdefghijklmnop")[:2]
    rest = P.message_words(1234567, 3, "abcdefghijklmnop")[2:]
    b = rest + [P.IDLE] * (16 - len(rest))
    b[8:11] = P.message_words(36, 2, "xyz")[:1] + [0] + P.message_words(36, 2, "xyz")[1:2]
    fix_b = [0] * 16
    fix_b[9] = 255
    rec = lambda cw, pos, fix=None, inverted=False, score=1.0, n_bad=0, fixed=0: dict(cw=cw, fix=fix or [0] * 16, row=0, pos=pos, meta=0, score=score,
                                                                                    sync_errors=0, inverted=inverted, n_bad=n_bad, fixed=fixed)
    recs = [rec(a, 1000), rec(a, 1003, score=0.5), rec(b, 1000 + 544 * spb + 16, fix=fix_b, n_bad=1), rec(b, 1000 + 2 * 544 * spb, inverted=True)]
    stats = {}
    msgs = F.pocsag_messages(recs, spb, stats=stats)
    assert [(m["ric"], m["alpha"], m["damaged"]) for m in msgs][:2] == [(1234567, "abcdefghijklmnop", False), (36, "", True)]
    # the third batch stands alone: its leading data words have no open message
    assert stats["orphans"] == len(rest) + 1 and len(msgs) == 4 and msgs[0]["pos"] == 1000 + (32 + 32 * 14) * spb


def test_boundaries_of_sync_errors_fix_and_max_bad():
    for se in (0, 1, 2):
        flips = [3, 17, 30][:se]
        assert run(flips, sync_errors=se)[4].tolist() == [se]
        assert run(flips + [8], sync_errors=se)[6] == 0
    at = 32 + 32 * 5
    for wrong in (1, 2, 3):
        flips = [at + 4, at + 19, at + 27][:wrong]
        hurt = P.WORDS[5] ^ sum(1 << (31 - (k - at)) for k in flips)
        for fix in (0, 1, 2):
            nf, cw = P.check(hurt, fix)
            assert (nf, cw) == (wrong, P.WORDS[5]) if wrong <= fix else cw != P.WORDS[5]
            r = run(flips, fix=fix, max_bad=1)
            if nf >= 0:
                assert r[1][0, 5] == nf and r[0][0, 5] == cw and r[4][0] == nf << 24
            else:
                assert r[1][0, 5] == 255 and r[0][0, 5] == 0 and r[4][0] == 1 << 16
            assert run(flips, fix=fix, max_bad=0)[6] == (1 if nf >= 0 else 0)
    assert run([at + 31], fix=1)[1][0, 5] == 1 and run([at + 31], fix=0)[6] == 0                         # the parity bit alone
    assert run([at + 31, at + 2], fix=2)[1][0, 5] == 2 and run([at + 31, at + 2], fix=1)[6] == 0           # parity + 1
    assert run([at + 31, at + 2, at + 11], fix=2)[6] == 0                                                # parity + 2: refused at fix 2
    assert all(P.check(w ^ 0xF8000000, 2) == (-1, 0) for w in P.WORDS)
    for bad in (1, 3, 16):
        flips = [32 + 32 * j + k for j in range(bad) for k in range(5)]
        r = run(flips, max_bad=bad)
        assert r[6] == 1 and r[4][0] == bad << 16 and r[1][0].tolist() == [255] * bad + [0] * (16 - bad) and not r[0][0, :bad].any()
        assert run(flips, max_bad=bad - 1)[6] == 0


def test_polarity_rates_and_the_rows_end():
    for spb in (2, 16, 32, 75, 128):
        n = 100 + P.LAST_K * spb + 1
        for inverted in (False, True):
            y = P.batch_row(spb, 100, n, inverted=inverted, hold=spb)
            r = both(y, spb)
            assert r[3].tolist() == [100] and r[0][0].tolist() == P.WORDS and r[4][0] == int(inverted) << 8 and r[5][0] == 1.0
            assert both(y[:-1], spb)[6] == 0                       # one sample short of 543 spb + 1
    y = P.batch_row(16, 100, 9000, amp=0.25, base=0.0) + np.float32(3.0)    # the threshold follows the offset
    assert both(y, 16)[3].tolist() == [100] and both(y, 16)[5][0] == 0.25


def test_non_finite_samples():
    y = P.batch_row(SPB, AT, N)
    for k, v in ((5, np.nan), (5, np.inf), (31, -np.inf)):
        z = y.copy()
        z[AT + SPB * k] = v
        assert both(z, SPB, max_bad=16)[6] == 0
    for k, v in ((100, np.nan), (543, np.inf), (200, -np.inf)):
        z = y.copy()
        z[AT + SPB * k] = v
        assert both(z, SPB, max_bad=16)[6] == 1
    assert both(np.full(9000, np.nan, np.float32), SPB)[6] == 0


def test_equal_scores_keep_the_earlier_start_and_max_batches_keeps_the_true_count():
    y = P.batch_row(SPB, AT, N, hold=SPB)
    assert both(y, SPB)[3].tolist() == [AT]
    for k in range(1, SPB):
        assert both(y, SPB, s_begin=AT + k)[6] == 0
    z = y.copy()
    z[AT + 9 + SPB * np.arange(32)] *= 1.5
    assert both(z, SPB)[3].tolist() == [AT + 9]
    many = sum(P.batch_row(2, 10 + 1100 * k, 8000) for k in range(6))
    assert both(many, 2)[6] == 6 and both(many, 2, max_batches=4)[6] == 6 and len(both(many, 2, max_batches=4)[3]) == 4
    assert both(many, 2, max_batches=0)[6] == 6
    rows = np.stack([many, many[::-1].copy(), np.roll(many, 7)])
    assert both(rows, 2)[2].tolist() == [0] * 6 + [2] * 6


def test_windows_do_not_change_a_byte():
    spb = 4
    n = 3 * P.TILE + 544 * spb + 24
    starts = [200, P.TILE - 1, P.TILE + 2500, 2 * P.TILE + 1000]
    y = np.stack([sum(P.batch_row(spb, s, n, hold=3, words=P.WORDS if k & 1 else P.WORDS[::-1]) for k, s in enumerate(starts)),
                  P.batch_row(spb, 900, n, hold=2, inverted=True)])
    whole = both(y, spb)
    assert whole[6] == 5
    for cuts in ([100, 150, 203, P.TILE - 1, P.TILE, P.TILE + 10], [P.TILE + 7, 2 * P.TILE + 16], [1]):
        edges = [0] + cuts + [n]
        parts = []
        for s0, s1 in zip(edges[:-1], edges[1:]):
            lo, hi = P.reach(s0, s1, n, spb)                     # exactly the window's reach
            parts.append(both(y[:, lo:hi], spb, buf_index0=lo, n_row=n, s_begin=s0, s_end=s1))
        order = np.lexsort((np.concatenate([q[3] for q in parts]), np.concatenate([q[2] for q in parts])))
        for i in range(6):
            assert same_bytes(np.concatenate([q[i] for q in parts])[order], whole[i]), (cuts, i)


def test_refusals_by_message():
    lib = L.load()
    y = P.batch_row(SPB, AT, N)
    n = len(y)
    cw, fx, rw, pos = np.zeros((4, 16), np.uint32), np.zeros((4, 16), np.uint8), np.zeros(4, np.int32), np.zeros(4, np.int64)
    meta, score, count = np.zeros(4, np.uint32), np.zeros(4, np.float32), np.full(1, -7, np.int32)
    ok = dict(y=p(y), n_rows=1, stride=n, n_buf=n, index0=0, n_row=n, s0=0, s1=n, spb=SPB, se=2, fix=2, max_bad=0, cw=p(cw), fx=p(fx), row=p(rw), pos=p(pos),
              meta=p(meta), score=p(score), count=p(count), max_batches=4)
    order = ("y", "n_rows", "stride", "n_buf", "index0", "n_row", "s0", "s1", "spb", "se", "fix", "max_bad", "cw", "fx", "row", "pos", "meta", "score", "count",
             "max_batches")

    def refused(why, **kw):
        a = dict(ok, **kw)
        r = lib.pss_h_pocsag_batches(*[a[k] for k in order])
        assert r == L.PSS_E_ARG and lib.pss_last_error(None).decode() == "pss_pocsag_batches: " + why, lib.pss_last_error(None).decode()
        assert count[0] == -7 and not cw.any()
    refused("n_rows outside [1, 2^20]", n_rows=0)
    refused("n_rows outside [1, 2^20]", n_rows=(1 << 20) + 1)
    refused("spb outside [2, 128]", spb=1)
    refused("spb outside [2, 128]", spb=129)
    refused("sync_errors outside [0, 2]", se=3)
    refused("sync_errors outside [0, 2]", se=-1)
    refused("fix outside [0, 2]", fix=3)
    refused("fix outside [0, 2]", fix=-1)
    refused("max_bad outside [0, 16]", max_bad=17)
    refused("max_bad outside [0, 16]", max_bad=-1)
    refused("y_stride < n_buf", stride=n - 1)
    refused("s_end < s_begin", s0=10, s1=9)
    refused("the window does not lie inside the row", s1=n + 1)
    refused("the buffer does not lie inside the row", n_row=n - 1)
    refused("the buffer does not lie inside the row", index0=-1)
    reach = "the buffer does not cover the window's reach (spb - 1 starts either side, 543 spb + 1 samples forward)"
    refused(reach, n_row=100000, s1=100)                                                  # the window's last start reads 543 spb + 1 ahead
    refused(reach, index0=50, n_row=n + 50, s0=60, s1=61)                                 # and spb - 1 starts back
    refused("a window of more than 2^30 starts", n_row=1 << 40, s1=(1 << 30) + 1)
    refused("more than 2^31 starts in the rows of one call", n_rows=3, n_row=1 << 40, s1=1 << 30)
    refused("n_row outside [0, 2^60]", n_row=-1)
    refused("n_row outside [0, 2^60]", n_row=(1 << 60) + 1)
    refused("max_batches < 0", max_batches=-1)
    refused("null buffer", count=None)
    refused("null buffer", y=None)
    refused("null buffer", cw=None)
    refused("null buffer", fx=None)
    refused("a misaligned pointer", y=p(y) + 2)
    refused("a misaligned pointer", pos=p(pos) + 4)
    refused("a misaligned pointer", count=p(count) + 2)
    assert lib.pss_h_pocsag_batches(*[ok[k] for k in order]) == 0 and count[0] == 1 and pos[0] == AT and cw[0].tolist() == P.WORDS
    assert E.h_pocsag_batches(y, SPB, s_begin=7, s_end=7)[6] == 0                         # an empty window is no refusal


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/pocsag_host.cpp: pss_pocsag.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own; it holds the 1024-entry table to a brute-force search."""
    exe = str(tmp_path / "pocsag_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "pocsag_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pocsag_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

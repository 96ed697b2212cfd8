"""The APT receiver's host side — pss_apt_plan, pss_apt_default_taps, pss_h_apt_front, pss_h_apt_syncs, pss_h_apt_lines, formats.apt_grid /
apt_image / apt_channels / apt_telemetry / write_pgm — against tests/golden/apt.npz and the NumPy statement of the rules in
tests/apt_cases.py — no GPU.  The arithmetic is the project's own (pyspecsdr_amd/csrc/pss_apt.h) and the reference holds no APT code, so the
truth is made outside the library: NumPy builds the passes from the words and restates the front, the candidate test, the one-record rule and
the line gather; the twins must agree with it (the front within 1 float32 ulp, the other two record for record and byte for byte) and hand
back the lines that were sent.  tests/test_gpu_apt.py (-m gpu) holds the kernels to the twins on every byte.  tests/apt_host.cpp runs the
header alone under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.signal import firwin

import apt_cases as A
from bytes_util import same_bytes
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
GOLD = np.load(os.path.join(HERE, "golden", "apt.npz"))
NAMES = [str(n) for n in GOLD["names"]]
SYMBOLS = ("pss_apt_plan", "pss_apt_default_taps", "pss_apt_front", "pss_h_apt_front", "pss_apt_syncs", "pss_h_apt_syncs", "pss_apt_lines",
           "pss_h_apt_lines")
WHAT = ("row", "pos", "meta", "score")
RECOVERY = ("smooth_30db", "noise_10db_3khz_40ppm")
_ENV = {}


def p(a):
    return None if a is None else a.ctypes.data


def case_env(name):
    """The twin's envelope of the case's row (made once; read-only)."""
    if name not in _ENV:
        env = E.h_apt_front(A.case_row(name))
        env.setflags(write=False)
        _ENV[name] = env
    return _ENV[name]


def both(env, sync_errors=2, **kw):
    """The twin and the NumPy statement agree on every record -> the twin's result."""
    twin = E.h_apt_syncs(env, sync_errors=sync_errors, **kw)
    ref = A.numpy_syncs(env, sync_errors, **{k: v for k, v in kw.items() if k in ("s_begin", "s_end", "max_syncs")})
    for t, r, what in zip(twin[:4], ref[:4], WHAT):
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
    assert ("pss_apt.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]) in units
    for name in ("apt_plan", "apt_default_taps", "apt_front", "h_apt_front", "apt_syncs", "h_apt_syncs", "apt_lines", "h_apt_lines"):
        assert callable(getattr(E, name))
    for name in ("apt_grid", "apt_image", "apt_channels", "apt_telemetry", "write_pgm", "apt_rows", "h_apt_rows", "apt_offset", "apt_recording"):
        assert callable(getattr(F, name))


def test_plan_and_taps():
    assert E.apt_plan(2.4e6) == (38, 247, 250) and E.apt_plan(2.048e6) == (32, 39, 40) and E.apt_plan(240e3) == (3, 39, 50)
    assert E.apt_plan(10e6) == (160, 624, 625) and E.apt_plan(62400) == (1, 1, 1) and E.apt_plan(249600) == (4, 1, 1)
    for fs, why in ((62400.5, "fs must be an integer number of Hz"), (float("nan"), "fs must be an integer number of Hz"),
                    (float("inf"), "fs must be an integer number of Hz"), (62399.0, "fs must be at least 62 400"), (-1.0, "fs must be at least 62 400"),
                    (1000003.0, "62 400 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take")):
        with pytest.raises(ValueError, match="^" + re.escape("pss_apt: " + why)):
            E.apt_plan(fs)
    taps = E.apt_default_taps()
    assert same_bytes(taps, firwin(79, 1.0 / 15.0))
    n = np.zeros(1, np.int32)
    assert L.load().pss_apt_default_taps(None, n.ctypes.data_as(L.C.POINTER(L.C.c_int))) == 0 and n[0] == 79


def test_goldens_are_the_synthesisers():
    assert NAMES == sorted(A.CASES)
    for name in NAMES:
        assert A.row_crc32(A.case_row(name)) == int(GOLD[name + "/crc32"][0])


@pytest.mark.parametrize("name", NAMES)
def test_front_within_one_ulp_of_the_float64_statement(name):
    """The statement takes the library's float32 discriminator (pss_h_ais_front with the pulse [1.0] hands it out unchanged; NumPy's own
    float32 arctan2 differs from the model in the last bit on some CPUs) and runs the mixer, the filter and the magnitude in float64."""
    x = A.case_row(name)
    env = case_env(name)
    d = E.h_ais_front(x, pulse=np.array([1.0]))
    ref = A.numpy_front(d, E.apt_default_taps())
    assert env.dtype == np.float32 and env.shape == ref.shape == (-(-len(x) // 5),)
    ulp = np.spacing(np.maximum(ref, env).astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(env.astype(np.float64) - ref) / ulp))
    print(name, "largest |twin - float64| in float32 ulps:", worst, "smallest envelope sample:", float(env.min()))
    assert worst <= 1.0


def test_front_windows_strides_and_other_arguments():
    lib = L.load()
    x = A.case_row("smooth_30db")[:30000]
    n = len(x)
    whole = E.h_apt_front(x)
    assert same_bytes(whole[:5900], case_env("smooth_30db")[:5900])
    for m0, m1 in ((0, 1), (1, 2), (17, 18), (100, 4000), (5990, 6000), (0, 6000)):
        lo, hi = max(0, m0 * 5 + 39 - 78 - 1), min(n, (m1 - 1) * 5 + 39 + 1)
        assert same_bytes(E.h_apt_front(x[lo:hi], buf_index0=lo, n_row=n, m_begin=m0, m_end=m1), whole[m0:m1]), (m0, m1)
    # lead at both ends, one tap, other rates and decimations: against the statement
    d = E.h_ais_front(x, pulse=np.array([1.0]))
    for taps, lead, fs, decim in ((np.array([1.0]), 0, 62400.0, 1), (E.apt_default_taps(), 0, 62400.0, 5), (E.apt_default_taps(), 78, 62400.0, 5),
                                  (firwin(201, 0.05), 100, 249600.0, 7)):
        got = E.h_apt_front(x, fs=fs, decim=decim, taps=taps, lead=lead)
        ref = A.numpy_front(d, taps, fs=fs, decim=decim, lead=lead)
        ulp = np.spacing(np.maximum(ref, got).astype(np.float32)).astype(np.float64)
        assert np.max(np.abs(got - ref) / ulp) <= 1.0, (len(taps), lead, fs, decim)
    # two rows of one batch with other strides; nothing is written behind a row's window
    a, b = x[:20000], A.case_row("noise_10db_3khz_40ppm")[:20000]
    buf = np.full((2, 20011), np.nan, np.complex64)
    buf[0, :20000], buf[1, :20000] = a, b
    taps = E.apt_default_taps()
    out = np.full((2, 4003), 7.0, np.float32)
    assert lib.pss_h_apt_front(p(buf), 2, 20011, 20000, 0, 20000, 62400.0, 5, p(taps), 79, 39, 0, 4000, p(out), 4003) == 0
    assert same_bytes(out[:, :4000], np.stack([E.h_apt_front(a), E.h_apt_front(b)])) and np.all(out[:, 4000:] == 7.0)
    assert len(E.h_apt_front(np.zeros(0, np.complex64))) == 0 and E.h_apt_front(np.ones(1, np.complex64)).tolist() == [0.0]


@pytest.mark.parametrize("name", NAMES)
def test_syncs_and_lines_are_the_numpy_statement_and_the_golden(name):
    env = case_env(name)
    for se in range(5):
        r = both(env, se)
        if se == 2:
            assert same_bytes(r[1], GOLD[name + "/pos"]) and same_bytes(r[2], GOLD[name + "/meta"])
            assert np.max(np.abs(r[3] - GOLD[name + "/score"])) < 1e-4
    lp, found = F.apt_grid(r[1], r[2], r[3], len(env))
    pos = np.concatenate([lp, [-100, len(env) - 3000, -6239, len(env) - 1]]).astype(np.int64)
    assert same_bytes(E.h_apt_lines(env, np.zeros(len(pos), np.int32), pos), A.numpy_lines(env, np.zeros(len(pos)), pos))


@pytest.mark.parametrize("name", RECOVERY)
def test_every_sent_line_is_found_and_nothing_else(name):
    r = both(case_env(name), 2)
    want = A.case_starts(name)
    assert r[4] == len(want) and np.all(np.abs(r[1] - want) <= 2) and not r[0].any()


@pytest.mark.parametrize("name", RECOVERY)
def test_image_a_correlates_with_what_was_sent(name):
    """The Pearson correlation of the image-A words the receiver recovers (formats.h_apt_rows: apt_rows through the host twins) with the
    sent ones is at least 0.95.  Measured: smooth_30db 0.99990, noise_10db_3khz_40ppm 0.9697.  The receiver puts the row's carrier at
    0 Hz before the front (apt_rows' `tune`): the three stages alone on the row as it is give 0.9233 at 10 dB with the 3 kHz offset,
    because the offset is a constant in the discriminator's output (0.30 rad) that the mixer moves to 2400 Hz, where firwin(79, 1 / 15)
    still passes 0.29 of it (PARITY.md "APT").  That figure is printed beside the asserted one."""
    sent = A.case_words(name)
    r = F.h_apt_rows(A.case_row(name))[0]
    assert r["words"].shape == sent.shape and r["found"].all()
    a = slice(A.IMAGE_A, A.IMAGE_A + 909)
    c = float(np.corrcoef(r["words"][:, a].ravel(), sent[:, a].ravel())[0, 1])
    env = case_env(name)
    s = E.h_apt_syncs(env)
    bare = float(np.corrcoef(E.h_apt_lines(env, s[0], s[1])[:, a].ravel(), sent[:, a].ravel())[0, 1])
    print(name, "correlation of image A:", c, "the three stages without the carrier step:", bare)
    assert c >= 0.95


def test_the_carrier_step():
    """apt_offset: the median of the inner block means, times 62 400 / 2 pi.  On the fixture rows it lands within 50 Hz of the offset the
    synthesiser put in (50 Hz leave 0.005 rad in the discriminator, a sixtieth of what 3 kHz leave; the clock error moves the carrier
    by 40 ppm of 3 kHz, nothing).  Without the step the receiver is the three stages on the row as it is."""
    assert F.apt_offset([9.0, 0.1, 0.3, 0.2, -9.0]) == 0.2 * 62400 / (2 * np.pi) and F.apt_offset([1.0, 2.0]) == 0.0 == F.apt_offset([])
    assert F.apt_offset([1.0, np.nan, np.nan, np.nan, 1.0]) == 0.0 and F.apt_offset(np.float32([0, 0.5, 0])) == 0.5 * 62400 / (2 * np.pi)
    for name in NAMES:
        r = F.h_apt_rows(A.case_row(name))[0]
        assert abs(r["offset_hz"] - A.CASES[name][3]) < 50.0, (name, r["offset_hz"])
        bare = F.h_apt_rows(A.case_row(name), tune=False)[0]
        env = case_env(name)
        s = E.h_apt_syncs(env)
        lp, _ = F.apt_grid(s[1], s[2], s[3], len(env))
        assert bare["offset_hz"] == 0.0 and same_bytes(bare["words"], E.h_apt_lines(env, np.zeros(len(lp), np.int32), lp))
        assert np.all(np.abs(r["pos"] - bare["pos"]) <= 1)
    # fewer than three blocks of 1024: nothing is estimated and the row is left as it is
    short = A.case_row("noise_10db_3khz_40ppm")[:2048]
    a, b = F.h_apt_rows(short)[0], F.h_apt_rows(short, tune=False)[0]
    assert a["offset_hz"] == 0.0 and same_bytes(a["words"], b["words"])
    assert F.h_apt_rows(np.full(9000, np.nan, np.complex64))[0]["offset_hz"] == 0.0
    # rows of one batch get their own offsets
    two = F.h_apt_rows(np.stack([A.case_row("smooth_30db")[:95000], A.case_row("noise_10db_3khz_40ppm")[:95000]]))
    assert abs(two[0]["offset_hz"]) < 50.0 and abs(two[1]["offset_hz"] - 3000.0) < 50.0


def test_mismatches_come_before_the_score():
    """A full-contrast 1040 Hz texture that ends on a black wedge reads as sync A with two mismatches (its first four words are texture) and
    out-scores the true sync, which has none: the true sync stays."""
    n, at = 9000, 1000
    env = A.sync_env(n, [at], high=0.6, low=0.2)
    tex = at + 2400                                                  # the texture's last seven pulses start four words behind this
    words = np.array(([1, 1, 0, 0] * 40)[:160], bool)                # 160 words of texture whose last word pair is low
    t0 = tex + 3 * 32 - 3 * len(words)                               # ... and ends where sync A's pulse train would
    env[t0:tex + 96] = np.repeat(np.where(words, 1.0, 0.0), 3).astype(np.float32)
    env[tex + 96:tex + 400] = 0.0                                    # the black wedge
    s, mism, q = A.candidates(env, 2)
    i_true, i_tex = np.flatnonzero(s == at)[0], np.flatnonzero(s == tex)[0]
    assert mism[i_true] == 0 and mism[i_tex] == 2 and q[i_tex] > q[i_true] and tex - at < A.NEAR
    r = both(env, 2)
    assert r[4] == 1 and r[1].tolist() == [at] and r[2].tolist() == [0] and abs(float(r[3][0]) - 0.4) < 1e-6
    r = both(env[at + 200:], 2)                                      # without the true sync the texture is reported
    assert r[4] >= 1 and np.all(r[2] == 2)


def test_equal_scores_keep_the_earlier_start_and_max_syncs_keeps_the_true_count():
    n = 40000
    starts = [500, 500 + A.NEAR + 7, 20000, 33000]
    env = A.sync_env(n, starts, full=True)                           # three samples a word: the starts one either side read the same words
    s, mism, q = A.candidates(env, 0)
    assert sorted(s.tolist()) == sorted(a + d for a in starts for d in (-1, 0, 1)) and len(set(q.tolist())) == 1
    r = both(env, 0)
    assert r[1].tolist() == [a - 1 for a in starts] and r[4] == 4
    for room in (0, 1, 3, 4, 9):
        c = both(env, 0, max_syncs=room)
        assert c[4] == 4 and len(c[1]) == min(room, 4) and c[1].tolist() == r[1].tolist()[:room]
    lib = L.load()
    rw, pos, meta, score, count = np.full(2, -1, np.int32), np.full(2, -1, np.int64), np.full(2, 9, np.uint32), np.full(2, -1, np.float32), np.zeros(1, np.int32)
    assert lib.pss_h_apt_syncs(p(env), 1, n, n, 0, n, 0, n, 0, p(rw), p(pos), p(meta), p(score), p(count), 1) == 0
    assert count[0] == 4 and pos.tolist() == [499, -1] and rw.tolist() == [0, -1] and meta.tolist() == [0, 9]   # nothing past max_syncs


def test_windows_do_not_change_a_byte():
    env = case_env("noise_10db_3khz_40ppm")
    n = len(env)
    whole = both(env, 4)
    cuts = [0, 1, 556, 557, 4096, 6796, 6797, 9000, n - 116, n]
    got = [[], [], [], []]
    for s0, s1 in zip(cuts[:-1], cuts[1:]):
        lo, hi = max(0, s0 - 3119), min(n, s1 + 3118 + 117)          # exactly the reach
        r = E.h_apt_syncs(env[lo:hi], sync_errors=4, buf_index0=lo, n_row=n, s_begin=s0, s_end=s1)
        ref = A.numpy_syncs(env, 4, s_begin=s0, s_end=s1)
        for k in range(4):
            assert same_bytes(r[k], ref[k])
            got[k].append(r[k])
    for k in range(4):
        assert same_bytes(np.concatenate(got[k]), whole[k])
    # a neighbour outside the window still counts: of two syncs 117 apart the later one alone in the window is dropped by the earlier
    env2 = A.sync_env(9000, [1000, 1117])
    assert both(env2, 0)[1].tolist() == [1000] and both(env2, 0, s_begin=1100, s_end=1200)[4] == 0
    assert E.h_apt_syncs(env2, s_begin=7, s_end=7)[4] == 0            # an empty window is no refusal


def test_non_finite_samples_sync_b_short_rows_and_the_last_candidate():
    n, at = 3000, 700
    clean = A.sync_env(n, [at])
    assert both(clean, 0)[1].tolist() == [at]
    for bad in (np.nan, np.inf, -np.inf):
        env = clean.copy()
        env[at + 3 * 10 + 1] = bad                                   # a strobe of the pulse train: the threshold is NaN or infinite
        r = both(env, 4)
        assert r[4] == 0 if bad != -np.inf else True
        env = clean.copy()
        env[at + 3 * 36 + 1] = bad                                   # a low word outside the threshold's strobes
        assert both(env, 1)[1].tolist() == [at]
        env = clean.copy()
        env[at + 3 * 10 + 2] = bad                                   # between two strobes of this start
        assert at in both(env, 0)[1].tolist()
    for fill in (np.nan, np.inf, 0.0, 1.0):
        assert both(np.full(500, fill, np.float32), 4)[4] == 0
    # sync B is never taken for sync A, at any shift
    for full in (False, True):
        assert both(A.sync_env(n, [at, 2000], pattern=A.SYNC_B, full=full), 4)[4] == 0
    # rows shorter than 117 samples hold no candidate; the row's last candidate is the start with 116 samples behind it
    for m in (0, 1, 116):
        assert both(np.ones(m, np.float32), 4)[4] == 0
    assert both(A.sync_env(117, [0]), 0)[1].tolist() == [0]
    assert both(A.sync_env(300 + 117, [300]), 0)[1].tolist() == [300] and both(A.sync_env(300 + 116, [300]), 0)[4] == 0
    # (four words earlier sync A reads as itself with four mismatches: the mismatch-first rule is what keeps that start out)
    r = both(A.sync_env(3000, [300]), 4)
    assert r[1].tolist() == [300] and sorted(A.candidates(A.sync_env(3000, [300]), 4)[0].tolist()) == [288, 300, 312]
    # rows do not run into each other
    two = np.stack([A.sync_env(500, [500 - 60]), A.sync_env(500, [])])
    two[1, :57] = A.sync_env(117, [0])[60:]                          # the sync's tail at the head of the next row
    assert both(two, 4)[4] == 0
    two = np.stack([A.sync_env(500, [100]), A.sync_env(500, [300])])
    r = both(two, 0)
    assert r[0].tolist() == [0, 1] and r[1].tolist() == [100, 300]


def test_lines_hang_over_both_ends_and_read_zero_there():
    env = np.arange(1, 20001, dtype=np.float32)
    rows = np.stack([env, -env])
    pos = np.array([-100, 0, 20000 - 6240, 20000 - 3000, -6239, -6240, 19999, 20000, 5, -2 ** 62, 2 ** 62, 7], np.int64)
    row = np.array([0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 1, 0], np.int32)
    got = E.h_apt_lines(rows, row, pos)
    assert same_bytes(got, A.numpy_lines(rows, row, pos))
    assert got[0, 32] == 0.0 and got[0, 33] == 1.0 and got[0, 34] == 4.0 and got[1, 0] == -2.0 and got[2, 2079] == 19999.0 and got[3, 1000] == 0.0
    assert got[4, 2079] == 0.0 and got[4, 2078] == 0.0 and not got[5].any() and not got[6].any() and not got[9].any() and not got[10].any()
    assert not np.signbit(got).any() or np.all(got[np.signbit(got)] < 0)       # the zeros are +0
    assert E.h_apt_lines(rows, np.array([2, -1], np.int32), np.array([0, 0], np.int64)).any() == False   # noqa: E712  (no such row: +0)
    assert E.h_apt_lines(rows, np.zeros(0, np.int32), np.zeros(0, np.int64)).shape == (0, 2080)


def test_refusals_by_message():
    lib = L.load()
    # ---- front
    iq = np.zeros(200, np.complex64)
    taps = np.ones(5)
    out = np.full(40, 7.0, np.float32)
    ok = dict(iq=p(iq), n_rows=1, stride=200, n_buf=200, index0=0, n_row=200, fs=62400.0, decim=5, taps=p(taps), n_taps=5, lead=2, m0=0, m1=40, out=p(out),
              ostride=40)
    order = ("iq", "n_rows", "stride", "n_buf", "index0", "n_row", "fs", "decim", "taps", "n_taps", "lead", "m0", "m1", "out", "ostride")

    def front_refused(why, **kw):
        a = dict(ok, **kw)
        assert lib.pss_h_apt_front(*[a[k] for k in order]) == L.PSS_E_ARG
        assert lib.pss_last_error(None).decode() == "pss_h_apt_front: " + why, lib.pss_last_error(None).decode()
        assert np.all(out == 7.0)
    front_refused("fs must be finite and above 4800 (the 2400 Hz subcarrier below the discriminator's Nyquist)", fs=4800.0)
    front_refused("fs must be finite and above 4800 (the 2400 Hz subcarrier below the discriminator's Nyquist)", fs=float("nan"))
    front_refused("decim outside [1, 4096]", decim=0)
    front_refused("decim outside [1, 4096]", decim=4097)
    front_refused("n_taps outside [1, 4097]", n_taps=0)
    front_refused("n_taps outside [1, 4097]", n_taps=4098)
    front_refused("n_rows < 1", n_rows=0)
    front_refused("null taps", taps=None)
    front_refused("x_stride < n_buf", stride=199)
    front_refused("lead outside [0, n_taps - 1]", lead=5)
    front_refused("lead outside [0, n_taps - 1]", lead=-1)
    front_refused("a tap that is not finite", taps=p(np.array([1.0, np.inf, 1.0, 1.0, 1.0])))
    front_refused("the buffer [buf_index0, buf_index0 + n_buf) is not inside the capture [0, n_capture)", n_row=199)
    front_refused("the buffer [buf_index0, buf_index0 + n_buf) is not inside the capture [0, n_capture)", index0=-1)
    front_refused("[m_begin, m_end) outside [0, ceil(n_capture / decim)]", m1=41)
    front_refused("[m_begin, m_end) outside [0, ceil(n_capture / decim)]", m0=3, m1=2)
    front_refused("out_stride < m_end - m_begin", ostride=39)
    front_refused("null output", out=None)
    front_refused("null input", iq=None)
    front_refused("an output needs a sample of the capture that the buffer does not hold", index0=10, n_row=210, m0=0, m1=1)
    front_refused("an output needs a sample of the capture that the buffer does not hold", n_buf=100, m1=40)
    # the discriminator of the first needed sample reads the one before it: sample 50 * 5 + 2 - 4 = 248 needs 247
    front_refused("an output needs a sample of the capture that the buffer does not hold", index0=248, n_row=1000, n_buf=200, m0=50, m1=60)
    assert lib.pss_h_apt_front(*[dict(ok, index0=247, n_row=1000, n_buf=200, m0=50, m1=60, ostride=10)[k] for k in order]) == 0
    assert lib.pss_h_apt_front(None, 1, 0, 0, 0, 100, 62400.0, 5, p(taps), 5, 2, 7, 7, None, 0) == 0          # an empty window needs no buffers
    # ---- syncs
    env = A.sync_env(9000, [4000])
    n = len(env)
    rw, pos, meta, score, count = np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(4, np.uint32), np.zeros(4, np.float32), np.full(1, -7, np.int32)
    ok2 = dict(env=p(env), n_rows=1, stride=n, n_buf=n, index0=0, n_row=n, s0=0, s1=n, se=2, row=p(rw), pos=p(pos), meta=p(meta), score=p(score),
               count=p(count), room=4)
    order2 = ("env", "n_rows", "stride", "n_buf", "index0", "n_row", "s0", "s1", "se", "row", "pos", "meta", "score", "count", "room")

    def syncs_refused(why, **kw):
        a = dict(ok2, **kw)
        assert lib.pss_h_apt_syncs(*[a[k] for k in order2]) == L.PSS_E_ARG
        assert lib.pss_last_error(None).decode() == "pss_apt_syncs: " + why, lib.pss_last_error(None).decode()
        assert count[0] == -7 and not pos.any()
    syncs_refused("n_rows outside [1, 2^20]", n_rows=0)
    syncs_refused("n_rows outside [1, 2^20]", n_rows=(1 << 20) + 1)
    syncs_refused("sync_errors outside [0, 4]", se=5)
    syncs_refused("sync_errors outside [0, 4]", se=-1)
    syncs_refused("e_stride < n_buf", stride=n - 1)
    syncs_refused("s_end < s_begin", s0=10, s1=9)
    syncs_refused("the window does not lie inside the row", s1=n + 1)
    syncs_refused("the window does not lie inside the row", s0=-1)
    syncs_refused("the buffer does not lie inside the row", n_row=n - 1)
    syncs_refused("the buffer does not lie inside the row", index0=-1)
    reach = "the buffer does not cover the window's reach (3119 starts either side, 117 samples forward)"
    syncs_refused(reach, n_row=100000, s1=n - 3234)                                       # 3118 + 117 samples ahead of the last start
    syncs_refused(reach, index0=50, n_row=n + 50, s0=3168, s1=3169)                       # and 3119 starts back
    assert lib.pss_h_apt_syncs(*[dict(ok2, n_row=100000, s1=n - 3235)[k] for k in order2]) == 0 and count[0] == 1 and pos[0] == 4000
    pos[:], count[0] = 0, -7
    assert lib.pss_h_apt_syncs(*[dict(ok2, index0=50, n_row=n + 50, s0=3169, s1=3170)[k] for k in order2]) == 0 and count[0] == 0
    count[0] = -7
    syncs_refused("a window of more than 2^30 starts", n_row=1 << 40, s1=(1 << 30) + 1)
    syncs_refused("more than 2^31 starts in the rows of one call", n_rows=3, n_row=1 << 40, s1=1 << 30)
    syncs_refused("n_row outside [0, 2^60]", n_row=-1)
    syncs_refused("n_row outside [0, 2^60]", n_row=(1 << 60) + 1)
    syncs_refused("max_syncs < 0", room=-1)
    syncs_refused("null buffer", count=None)
    syncs_refused("null buffer", env=None)
    syncs_refused("null buffer", pos=None)
    syncs_refused("null buffer", score=None)
    syncs_refused("a misaligned pointer", env=p(env) + 2)
    syncs_refused("a misaligned pointer", pos=p(pos) + 4)
    syncs_refused("a misaligned pointer", count=p(count) + 2)
    assert lib.pss_h_apt_syncs(*[ok2[k] for k in order2]) == 0 and count[0] == 1 and pos[0] == 4000
    # ---- lines
    lr, lp, words = np.zeros(2, np.int32), np.zeros(2, np.int64), np.full((2, 2080), 7.0, np.float32)
    ok3 = dict(env=p(env), n_rows=1, stride=n, n_row=n, lr=p(lr), lp=p(lp), n_lines=2, words=p(words), wstride=2080)
    order3 = ("env", "n_rows", "stride", "n_row", "lr", "lp", "n_lines", "words", "wstride")

    def lines_refused(why, **kw):
        a = dict(ok3, **kw)
        assert lib.pss_h_apt_lines(*[a[k] for k in order3]) == L.PSS_E_ARG
        assert lib.pss_last_error(None).decode() == "pss_apt_lines: " + why, lib.pss_last_error(None).decode()
        assert np.all(words == 7.0)
    lines_refused("n_rows outside [1, 2^20]", n_rows=0)
    lines_refused("n_row outside [0, 2^60]", n_row=-1)
    lines_refused("e_stride < n_row", stride=n - 1)
    lines_refused("n_lines outside [0, 2^24]", n_lines=-1)
    lines_refused("n_lines outside [0, 2^24]", n_lines=(1 << 24) + 1)
    lines_refused("words_stride < 2080", wstride=2079)
    lines_refused("null buffer", env=None)
    lines_refused("null buffer", lr=None)
    lines_refused("null buffer", lp=None)
    lines_refused("null buffer", words=None)
    lines_refused("a misaligned pointer", lp=p(lp) + 4)
    lines_refused("a misaligned pointer", words=p(words) + 2)
    assert lib.pss_h_apt_lines(*[ok3[k] for k in order3]) == 0 and same_bytes(words, A.numpy_lines(env, lr, lp))


def test_grid_fills_a_gap_and_ignores_an_outlier():
    true = lambda k: 100.0 + 6240.3 * k                              # noqa: E731  (a clock 48 ppm slow)
    have = [0, 1, 2, 6, 7]
    pos = sorted([int(round(true(k))) for k in have] + [int(true(2)) + 2000])
    meta = np.zeros(len(pos), np.uint32)
    score = np.ones(len(pos), np.float32)
    n_env = int(true(8)) + 50
    lp, found = F.apt_grid(pos, meta, score, n_env)
    assert len(lp) == 8 and found.tolist() == [True, True, True, False, False, False, True, True]
    assert np.all(np.abs(lp - np.array([true(k) for k in range(8)])) <= 1) and lp.dtype == np.int64 and found.dtype == bool
    # lines before the first record and behind the last, as far as their 6240 samples lie in the row
    lp2, found2 = F.apt_grid([20000, 26240], [0, 0], [1.0, 1.0], 40000)
    assert lp2.tolist() == [1280, 7520, 13760, 20000, 26240, 32480] and found2.tolist() == [False, False, False, True, True, False]
    assert F.apt_grid([], [], [], 1000)[0].shape == (0,) and F.apt_grid([5], [1], [0.5], 6245)[0].tolist() == [5] and not len(F.apt_grid([5], [1], [0.5], 6244)[0])
    assert F.apt_grid([5], [1], [0.5], 6245 + 6240)[0].tolist() == [5, 6245]
    # ties: of two chains of one length the fewer mismatches, then the higher score, then the earlier
    a, b = [1000, 7240], [3000, 9240]
    for meta_a, meta_b, q_a, q_b, first in ((0, 1, 1.0, 9.0, 1000), (1, 0, 9.0, 1.0, 3000), (1, 1, 1.0, 2.0, 3000), (1, 1, 2.0, 2.0, 1000)):
        lp, _ = F.apt_grid([a[0], b[0], a[1], b[1]], [meta_a, meta_b, meta_a, meta_b], [q_a, q_b, q_a, q_b], 20000)
        assert first in lp.tolist() and (4000 - first) not in lp.tolist(), (meta_a, meta_b, q_a, q_b)
    with pytest.raises(ValueError, match="pos must ascend"):
        F.apt_grid([5, 5], [0, 0], [1.0, 1.0], 100)


def test_telemetry_image_channels_and_pgm(tmp_path):
    for ids, names in (((2, 4), ("2", "4")), ((3, 6), ("3A", "3B")), ((1, 5), ("1", "5"))):
        words = A.pass_words(130, "smooth", 3, ids=ids, first_line=37)
        tel = F.apt_telemetry(words)
        for c in range(2):
            t = tel[c]
            assert t["channel"] == names[c] and t["phase"] == 128 - 37 and abs(t["gain"] - 255.0) < 1e-6 and abs(t["offset"]) < 1e-6
            assert np.allclose(t["levels"][:9] * 255.0, [31, 63, 95, 127, 159, 191, 224, 255, 0]) and t["levels"].shape == (16,)
        img = F.apt_image(words, telemetry=tel)
        # (a word that lands on a half, 178.5, may round either way behind a gain of 255 - 1e-13: one grey level, a handful of words)
        close = lambda a, b: np.max(np.abs(a.astype(int) - b.astype(int))) <= 1 and np.mean(a != b) < 1e-4   # noqa: E731
        assert img.dtype == np.uint8 and img.shape == (130, 2080) and close(img, np.floor(words * 255.0 + 0.5).astype(np.uint8))
        # another gain and offset on the words: the staircase takes them out again
        assert close(F.apt_image(words * 0.37 + 0.11, telemetry=F.apt_telemetry(words * 0.37 + 0.11)), img)
    assert F.apt_telemetry(words[:127]) == (None, None) and F.apt_telemetry(words[:128])[0]["channel"] == "1"
    pct = F.apt_image(words)
    lo, hi = np.percentile(words, [1, 99])
    assert np.array_equal(pct, np.clip(np.floor((words - lo) * (255.0 / (hi - lo)) + 0.5), 0, 255).astype(np.uint8))
    bad = words.copy()
    bad[3, 7] = np.nan
    assert F.apt_image(bad)[3, 7] == 0 and F.apt_image(np.zeros((0, 2080))).shape == (0, 2080)
    a, b = F.apt_channels(img)
    assert a.shape == b.shape == (130, 909) and np.array_equal(a, img[:, 86:995]) and np.array_equal(b, img[:, 1126:2035])
    path = str(tmp_path / "a.pgm")
    F.write_pgm(path, a)
    raw = open(path, "rb").read()
    head = b"P5\n909 130\n255\n"
    assert raw.startswith(head) and np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(130, 909), a)
    with pytest.raises(ValueError):
        F.write_pgm(path, a.astype(np.float32))


def test_h_apt_rows_end_to_end():
    rows = F.h_apt_rows(np.stack([A.case_row("smooth_30db")[:95000], A.case_row("smooth_10db_minus_4khz_minus_60ppm")[:95000]]))
    assert len(rows) == 2
    for r, name in zip(rows, ("smooth_30db", "smooth_10db_minus_4khz_minus_60ppm")):
        want = A.case_starts(name)
        want = want[want + 6240 <= 19000]
        assert r["words"].shape == (len(want), 2080) == r["image"].shape and r["image"].dtype == np.uint8
        assert np.all(np.abs(r["pos"] - want) <= 2) and r["found"].all() and r["telemetry"] == (None, None)
        assert [s["mismatches"] for s in r["syncs"]] == [0] * len(r["syncs"]) and len(r["syncs"]) >= len(want)
    assert F.h_apt_rows(np.zeros((2, 0), np.complex64))[1]["words"].shape == (0, 2080)


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/apt_host.cpp: pss_apt.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "apt_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "apt_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "apt_host: ok", (r.stdout, r.stderr)

"""The down-converter's host twins (pss_h_ddc, pss_h_ddc_rotor, pss_ddc_word, pss_ddc_default_taps) against tests/golden/ddc.npz — no
GPU.  The arithmetic is the project's own (pyspecsdr_amd/csrc/pss_ddc.h), so the truth is computed outside it: exact integer phases,
sine and cosine in 80-bit long double, SciPy's decimate and lfilter on the capture mixed in float64 (tools/make_goldens_ddc.py).

  rotor    within 4 * 2^-53 absolute of the 80-bit truth: half an ulp for the knot, about one for the two polynomials, two roundings in
           the product pair.  Exact at word 0 and at the quarter turn.
  output   |float64(y32) - ref| <= 1/2 ulp_float32(max(|ref|, |y32|)) + (T + 8) 2^-53 sum|h| max|z| on each part: the float32
           rounding of the result plus the fma chain's bound with the rotor's and the product's errors.
  shape    K channels in one call, any split of [m_begin, m_end), any chunking of the capture with exactly the needed halo: the same bytes.
tests/test_gpu_ddc.py (-m gpu) holds the kernel to the twin bit for bit.  tests/ddc_host.cpp runs the header alone under
AddressSanitizer and UBSan.
"""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bytes_util import same_bytes, zeros_alike
import ddc_cases as DC
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "ddc.npz"))


def test_fixture_inputs_are_what_the_makers_give_today(g):
    assert int(g["version"]) == DC.VERSION
    assert [int(w) for w in g["rotor_words"]] == DC.rotor_words() and [int(i) for i in g["rotor_indices"]] == DC.rotor_indices()
    for name, D, n, _, fractions in DC.CASES:
        x = DC.case_capture(name)
        assert len(x) == n and int(g[f"crc_{name}"]) == DC.crc(x), name
        assert [int(w) for w in g[f"words_{name}"]] == [DC.word_of(f) for f in fractions]
        assert g[f"ref_{name}"].shape == (len(fractions), -(-n // D))
    assert int(g["chain_crc"]) == DC.crc(DC.chain_capture())


def test_rotor_is_within_four_units_of_the_80_bit_truth(g):
    words, idx = DC.rotor_words(), DC.rotor_indices()
    assert max(idx) == 1 << 62 and {0, 1 << 62, 1 << 63, 1, (1 << 64) - 1} <= set(words) and len(words) == 5 + 16
    c_hi, c_lo, s_hi, s_lo = (g[k] for k in ("rotor_c_hi", "rotor_c_lo", "rotor_s_hi", "rotor_s_lo"))
    worst = 0.0
    for k, w in enumerate(words):
        for j, i in enumerate(idx):
            c, s = Engine.h_ddc_rotor(w, i, 1)
            worst = max(worst, abs((c[0] - c_hi[k, j]) - c_lo[k, j]), abs((s[0] - s_hi[k, j]) - s_lo[k, j]))
    print(f"largest rotor error: {worst / 2.0 ** -53:.3f} * 2^-53")
    assert worst <= 4 * 2.0 ** -53


def test_rotor_is_exact_at_word_zero_and_at_the_quarter_turn():
    for index0 in (0, 1, 2, 3, 12345, (1 << 40) + 1, (1 << 62) - 8):
        c, s = Engine.h_ddc_rotor(0, index0, 8)
        assert np.all(c == 1.0) and np.all(s == 0.0)
        c, s = Engine.h_ddc_rotor(1 << 62, index0, 8)
        k = (index0 + np.arange(8)) & 3
        assert np.array_equal(c, np.array([1.0, 0.0, -1.0, 0.0])[k]) and np.array_equal(s, np.array([0.0, -1.0, 0.0, 1.0])[k])
    # consecutive indices of one call are the indices of single calls
    w = DC.rotor_words()[7]
    c, s = Engine.h_ddc_rotor(w, 1000, 50)
    for t in (0, 1, 49):
        c1, s1 = Engine.h_ddc_rotor(w, 1000 + t, 1)
        assert c1[0] == c[t] and s1[0] == s[t]


def test_word_is_pythons_integer_rounding_and_the_effective_offset_follows():
    rng = np.random.default_rng(41)
    cases = [(0.0, 2.4e6), (600e3, 2.4e6), (-600e3, 2.4e6), (1.2e6, 2.4e6), (-1.2e6, 2.4e6), (300e3, 2.4e6), (-450e3, 2.4e6), (1.0, 10e6),
             (2.0 ** -65, 1.0), (1.5 * 2.0 ** -64, 1.0), (2.5 * 2.0 ** -64, 1.0), (-2.0 ** -64, 1.0)]
    cases += [(float(f), float(fs)) for f, fs in zip(rng.uniform(-0.5, 0.5, 200) * 2.4e6, np.full(200, 2.4e6))]
    cases += [(float(f * fs), float(fs)) for f, fs in zip(rng.uniform(-0.5, 0.5, 100), rng.uniform(1e3, 1e8, 100))]
    for off, fs in cases:
        w, eff = Engine.ddc_word(off, fs)
        want = round(Fraction(off / fs) * (1 << 64)) % (1 << 64)          # the float64 quotient, scaled exactly, ties to even
        assert w == want, (off, fs, w, want)
        signed = w - (1 << 64) if w >= 1 << 63 else w
        assert eff == (float(signed) * 2.0 ** -64) * fs
        if abs(off) < fs / 2:
            assert abs(eff - off) <= fs * 2.0 ** -64 + abs(off) * 2.0 ** -52
    assert Engine.ddc_word(1.2e6, 2.4e6) == (1 << 63, -1.2e6)              # +fs / 2 is the same oscillator as -fs / 2
    for off, fs in ((1.2e6 + 1, 2.4e6), (-1.3e6, 2.4e6), (0.0, 0.0), (0.0, -1.0), (np.nan, 1.0), (0.0, np.inf), (np.inf, 1.0)):
        with pytest.raises(ValueError):
            Engine.ddc_word(off, fs)
    assert L.load().pss_last_error(None)


def test_default_taps_equal_scipys_firwin(g):
    for D in DC.TAP_DECIMS:
        assert same_bytes(Engine.ddc_default_taps(D), g[f"taps_{D}"]), D
    assert same_bytes(Engine.ddc_default_taps(1), np.array([1.0]))
    assert len(Engine.ddc_default_taps(204)) == 4081
    for D in (0, -1, 205, 4096):
        with pytest.raises(ValueError):
            Engine.ddc_default_taps(D)
    lib = L.load()
    assert [lib.pss_ddc_out_len(n, 5) for n in (0, 1, 4, 5, 6, 1003)] == [0, 1, 1, 1, 2, 201]
    assert lib.pss_ddc_out_len(-1, 5) < 0 and lib.pss_ddc_out_len(10, 0) < 0 and lib.pss_ddc_out_len(10, 4097) < 0
    assert lib.pss_ddc_out_len(2 ** 62, 4096) == 2 ** 50


def test_golden_cases_are_inside_the_output_bound(g):
    worst = []
    for name, D, n, zero_phase, _ in DC.CASES:
        x, h, ref = DC.case_capture(name), g[f"h_{name}"], g[f"ref_{name}"]
        if zero_phase:
            y = Engine.h_ddc(x, g[f"words_{name}"], D)                    # the default taps and the default lead
            assert same_bytes(y, Engine.h_ddc(x, g[f"words_{name}"], D, taps=h, lead=(len(h) - 1) // 2))
        else:
            y = Engine.h_ddc(x, g[f"words_{name}"], D, taps=h, lead=0)
        assert y.shape == ref.shape and y.dtype == np.complex64
        for c in range(len(ref)):
            excess, used = DC.bound_excess(y[c], ref[c], len(h), np.abs(h).sum(), g[f"zmax_{name}"][c])
            print(f"{name}[{c}]: excess {excess:.3e}, float64 term used {used:.4f}")
            worst.append((excess, name, c))
    assert max(worst)[0] <= 0, max(worst)


def test_identity_and_quarter_turn_are_exact():
    x = DC.special_identity_input()
    n = len(x)
    assert np.isfinite(x.view(np.float32)).all() and np.any((x.real != 0) & (np.abs(x.real) < np.finfo(np.float32).tiny))
    for index0 in (0, 1, 2, 3):
        kw = dict(taps=[1.0], lead=0, buf_index0=index0, n_capture=index0 + n, m_begin=index0, m_end=index0 + n)
        y = Engine.h_ddc(x, [0, 1 << 62], 1, **kw)
        assert np.array_equal(y[0], x)                                     # (== on the values: the sign of a zero is not part of the contract)
        turn = np.array([1, -1j, -1, 1j])[(index0 + np.arange(n)) & 3]
        assert np.array_equal(y[1], (x.astype(np.complex128) * turn).astype(np.complex64)), index0


def test_the_shape_of_the_call_changes_no_byte():
    D, T, n, lead = 7, 141, 3001, 70
    x = DC.capture(n, 77)
    rng = np.random.default_rng(42)
    h = rng.standard_normal(T) / 12
    words = [DC.word_of(f) for f in (0.3, -0.0421, 0.4999)] + [0x0123456789abcdef, (1 << 64) - 12345]
    n_out = -(-n // D)
    whole = Engine.h_ddc(x, words, D, taps=h, lead=lead)
    assert whole.shape == (5, n_out)
    for c, w in enumerate(words):                                          # K channels in one call against K calls
        assert zeros_alike(Engine.h_ddc(x, [w], D, taps=h, lead=lead)[0]) == zeros_alike(whole[c])
    cuts = [0, 1, 2, 57, 58, 200, n_out - 1, n_out]
    for a, b in zip(cuts[:-1], cuts[1:]):                                  # [m_begin, m_end) split at arbitrary points
        assert zeros_alike(Engine.h_ddc(x, words, D, taps=h, lead=lead, m_begin=a, m_end=b)) == zeros_alike(whole[:, a:b]), (a, b)
        lo, hi = max(0, a * D + lead - (T - 1)), min(n, (b - 1) * D + lead + 1)   # buffers of awkward lengths with exactly the needed halo
        assert (hi - lo) % D or b - a < 3
        part = Engine.h_ddc(x[lo:hi], words, D, taps=h, lead=lead, buf_index0=lo, n_capture=n, m_begin=a, m_end=b)
        assert zeros_alike(part) == zeros_alike(whole[:, a:b]), (a, b, lo, hi)
    for lead2 in (0, T - 1):                                               # the other leads, chunked the same way
        w2 = Engine.h_ddc(x, words[:2], D, taps=h, lead=lead2)
        a, b = 100, 233
        lo, hi = max(0, a * D + lead2 - (T - 1)), min(n, (b - 1) * D + lead2 + 1)
        part = Engine.h_ddc(x[lo:hi], words[:2], D, taps=h, lead=lead2, buf_index0=lo, n_capture=n, m_begin=a, m_end=b)
        assert zeros_alike(part) == zeros_alike(w2[:, a:b])


def test_outputs_follow_the_defining_sum():
    """y[m] = sum over k of h[k] z[m D + lead - k] with z = 0 outside the capture, at the first and last outputs, where the zeros enter."""
    D, T, n, lead = 3, 65, 100, 20
    x = DC.capture(n, 78)
    h = np.random.default_rng(43).standard_normal(T) / 8
    w = DC.word_of(0.11)
    c, s = Engine.h_ddc_rotor(w, 0, n)
    z = x.astype(np.complex128) * (c + 1j * s)
    y = Engine.h_ddc(x, [w], D, taps=h, lead=lead)[0]
    for m in range(len(y)):
        acc = sum(h[k] * z[m * D + lead - k] for k in range(T) if 0 <= m * D + lead - k < n)
        assert abs(y[m] - acc) <= 1e-6 * max(1.0, abs(acc)), m


def test_refused_arguments_say_why():
    lib = L.load()
    n, D, T = 1000, 5, 101
    x = np.ascontiguousarray(DC.capture(n, 79))
    h = np.ascontiguousarray(np.random.default_rng(44).standard_normal(T))
    words = np.array([1, 2], np.uint64)
    out = np.full((2, 200), -7.25, np.complex64)
    nan_taps, inf_taps = h.copy(), h.copy()
    nan_taps[7], inf_taps[100] = np.nan, -np.inf
    p = lambda a: None if a is None else a.ctypes.data
    good = dict(iq=x, n_buf=n, buf_index0=0, n_capture=n, words=words, n_chan=2, decim=D, taps=h, n_taps=T, lead=50, m_begin=0, m_end=200, out=out,
                out_stride=200)
    order = ["iq", "n_buf", "buf_index0", "n_capture", "words", "n_chan", "decim", "taps", "n_taps", "lead", "m_begin", "m_end", "out", "out_stride"]

    def call(**change):
        a = dict(good)
        a.update(change)
        return lib.pss_h_ddc(*[p(a[k]) if k in ("iq", "words", "taps", "out") else a[k] for k in order])

    assert call() == 0
    ok = out.copy()
    bad = [dict(decim=0), dict(decim=4097), dict(n_taps=0), dict(n_taps=4098), dict(n_chan=0), dict(n_chan=-1), dict(lead=-1), dict(lead=T),
           dict(taps=nan_taps), dict(taps=inf_taps), dict(iq=None), dict(words=None), dict(taps=None), dict(out=None),
           dict(n_capture=-1), dict(n_buf=-1), dict(buf_index0=-1), dict(n_capture=n - 1), dict(buf_index0=1),
           dict(m_begin=-1), dict(m_begin=3, m_end=2), dict(m_end=201), dict(out_stride=199),
           dict(n_buf=n - 1),                                              # output 199 needs sample 999
           dict(buf_index0=10, n_buf=n - 10)]                              # output 0 needs sample 0
    for b in bad:
        lib.pss_h_ddc_rotor(0, -1, 0, None, None)                          # leaves a message of its own behind
        before = lib.pss_last_error(None)
        assert call(**b) == L.PSS_E_ARG, b
        msg = lib.pss_last_error(None)
        assert msg and msg.startswith(b"pss_h_ddc: ") and msg != before, (b, msg)
    assert same_bytes(out, ok)                                             # a refused call writes nothing
    # an empty range is no error and needs no buffers
    assert call(m_begin=7, m_end=7, out=None, iq=None) == 0
    for args in ((0, -1, 1), (0, 0, -1), (0, 2 ** 63 - 1, 2)):
        assert lib.pss_h_ddc_rotor(*args, p(np.empty(2)), p(np.empty(2))) == L.PSS_E_ARG
    n_taps = C.c_int()
    assert lib.pss_ddc_default_taps(5, None, None) == L.PSS_E_ARG and lib.pss_ddc_default_taps(5, None, C.byref(n_taps)) == 0 and n_taps.value == 101
    assert lib.pss_ddc_word(0.0, 1.0, None, None) == L.PSS_E_ARG


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/ddc_host.cpp: pss_ddc.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "ddc_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "ddc_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ddc_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_header_table_and_library_agree_on_the_new_entry_points():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in ("pss_ddc_word", "pss_ddc_out_len", "pss_ddc_default_taps", "pss_h_ddc_rotor", "pss_ddc", "pss_h_ddc"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    build = open(os.path.join(ROOT, "pyspecsdr_amd", "build.py")).read()
    assert '("pss_ddc.hip", ["-ffp-contract=off"])' in build


def test_python_layers_check_their_arguments_without_a_gpu():
    from pyspecsdr_amd import formats as F
    with pytest.raises(ValueError):
        F.demodulate_channels(np.zeros(10, np.complex64), 2.4e6, [0.0], 50, mode="FM")
    with pytest.raises(ValueError):
        F.demodulate_channels(np.zeros(10, np.complex64), 2.4e6, [0.0], 50, frame_len=0)
    with pytest.raises(ValueError):
        Engine.h_ddc(np.zeros((2, 2), np.complex64), [0], 1)
    with pytest.raises(ValueError):
        Engine.h_ddc(np.zeros(4, np.complex64), [0], 300)                   # no default taps past D = 204
    assert Engine.h_ddc(np.zeros(0, np.complex64), [0, 1], 5).shape == (2, 0)

"""FM mono (decode_mono, signal_processing.py:331-359) and lowpass_filter (:28-31) on the host, against what the reference returned
(tests/golden/fm_mono.npz, tools/make_goldens_fm_mono.py) — no GPU, no reference at test time.

pss_h_decode_mono and pss_h_lfilter are the host twins of the kernels: the same statements of pyspecsdr_amd/csrc/pss_mono.h on one thread.
Here they are pinned to the reference bit for bit (NaN matching NaN) in the int16 result, the float64 value the cast sees and the float32
decimated row, at every length x rate of the fixture and on its special frames; tests/test_gpu_fm_mono.py then compares the device with
the same goldens and with the twins.  tests/mono_host.cpp runs the header alone under AddressSanitizer and UBSan.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_mono_cases as M
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")


@pytest.fixture(scope="module")
def g(golden):
    return golden["fm_mono"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def matches(g, key, got, long):
    """`got` against the fixture's array, or against its digest, head and tail."""
    if not long:
        return same_bits(got, g[key])
    return (np.array_equal(M.digest(got), g[key + "_digest"]) and same_bits(got[:M.EDGE], g[key + "_head"])
            and same_bits(got[-M.EDGE:], g[key + "_tail"]))


def test_fixture_inputs_are_what_the_makers_give_today(g):
    assert list(g["lengths"]) == M.LENGTHS and list(g["rates"]) == M.RATES and list(g["specials"]) == M.SPECIALS
    assert int(g["special_n"]) == M.SPECIAL_N and list(g["lp_lengths"]) == M.LP_LENGTHS
    assert np.array_equal(g["lp_params"], np.array(M.LP_PARAMS, np.float64))
    for n in M.LENGTHS:
        x = M.frame(n)
        if n >= M.LONG:
            assert np.array_equal(M.digest(x), g[f"crc_{n}"]), n
        else:
            assert same_bits(x.view(np.float32), g[f"in_{n}"].view(np.float32)), n
    for name in M.SPECIALS:
        assert same_bits(M.special(name).view(np.float32), g[f"in_sp_{name}"].view(np.float32)), name
    for dt in ("float32", "float64"):
        for n in M.LP_LENGTHS:
            x = M.lp_row(n, dt)
            if n >= M.LP_LONG:
                assert np.array_equal(M.digest(x), g[f"lp_crc_{dt}_{n}"])
            else:
                assert same_bits(x, g[f"lp_in_{dt}_{n}"])
    stamp = str(g["stamp"])
    assert '"numpy": "2.2.6"' in stamp and '"scipy": "1.15.3"' in stamp and "AVX512_SKX" in stamp


@pytest.mark.parametrize("fs", M.RATES)
def test_host_twin_equals_the_reference_at_every_length(g, fs):
    bad = []
    for n in M.LENGTHS:
        pcm, audio, dec = Engine.h_decode_mono(M.frame(n), fs, stages=True)
        k, long = f"{n}_{int(fs)}", n >= M.LONG
        assert len(pcm) == L.load().pss_decode_mono_len(n) == -(-(n - 1) // 6)
        for name, got in (("pcm", pcm), ("audio", audio), ("dec", dec)):
            if not matches(g, f"{name}_{k}", got, long):
                bad.append((n, name))
    assert not bad, bad


@pytest.mark.parametrize("fs", M.RATES)
def test_host_twin_equals_the_reference_on_the_special_frames(g, fs):
    bad = []
    for name in M.SPECIALS:
        pcm, audio, dec = Engine.h_decode_mono(g[f"in_sp_{name}"], fs, stages=True)
        k = f"sp_{name}_{int(fs)}"
        for what, got in (("pcm", pcm), ("audio", audio), ("dec", dec)):
            if not same_bits(got, g[f"{what}_{k}"]):
                bad.append((name, what))
    assert not bad, bad


def test_the_fixture_holds_a_wrap_a_nan_frame_and_zeros(g):
    k = f"sp_wrap_{int(2.4e6)}"
    audio, pcm = g[f"audio_{k}"], g[f"pcm_{k}"]
    over = np.abs(audio) >= 32768
    assert over.sum() >= 1, "no value of the wrap frame passes the int16 range"
    assert np.array_equal(pcm[over].view(np.uint16), (np.trunc(audio[over]).astype(np.int64) & 0xffff).astype(np.uint16))
    assert np.any(pcm[over].astype(np.float64) * audio[over] < 0), "the wrapped values did not change sign: a saturating cast would pass"
    got = Engine.h_decode_mono(g["in_sp_wrap"], 2.4e6)
    assert np.array_equal(got, pcm)
    for fs in M.RATES:
        assert np.isnan(g[f"audio_sp_nan_{int(fs)}"]).all() and not g[f"pcm_sp_nan_{int(fs)}"].any()
        assert not Engine.h_decode_mono(g["in_sp_nan"], fs).any()
        assert not g[f"pcm_sp_zeros_{int(fs)}"].any() and not Engine.h_decode_mono(g["in_sp_zeros"], fs).any()
    # the rare path of arctan2 is in the fixture: products that are zero and products that are denormal
    prod = g["prod_sp_tiny"].view(np.float32)
    assert np.any(prod == 0) and np.any((prod != 0) & (np.abs(prod) < np.finfo(np.float32).tiny))


def test_the_operands_are_not_swapped_on_either_side_of_the_elision_threshold(g):
    """samples[:-1] * samples.conj()[1:] as NumPy's FMA loop multiplies it, a = x[i], b = conj(x[i + 1]), at 32 768, 32 769 and 40 001 samples
    as at 1024: re = fma(a.re, b.re, -(a.im b.im)), im = fma(a.re, b.im, a.im b.re) in float64-emulated single rounding."""
    for n in (1024, 4097, 32768, 32769, 40001):
        x = M.frame(n)
        a, b = x[:-1], np.conj(x[1:])
        ar, ai, br, bi = (v.astype(np.float64) for v in (a.real, a.imag, b.real, b.imag))
        # float32 products are exact in float64; the fused sum rounds once (float64's 53 bits hold the 48-bit product plus the addend's
        # alignment in all but double-rounding cases, which the digest comparison below would expose)
        re = (ar * br + -(ai * bi).astype(np.float32).astype(np.float64)).astype(np.float32)
        im = (ar * bi + (ai * br).astype(np.float32).astype(np.float64)).astype(np.float32)
        sw = (ai * br + (ar * bi).astype(np.float32).astype(np.float64)).astype(np.float32)      # the swapped form NFM / WFM take when long
        key, long = f"prod_{n}", n >= M.LONG
        want_head = g[key + "_head"] if long else g[key][:M.EDGE]
        assert same_bits(re[:M.EDGE], np.ascontiguousarray(want_head.real)) and same_bits(im[:M.EDGE], np.ascontiguousarray(want_head.imag)), n
        assert not same_bits(sw[:M.EDGE], np.ascontiguousarray(want_head.imag)), n


def test_empty_and_one_sample_buffers_give_empty_results():
    lib = L.load()
    assert lib.pss_decode_mono_len(0) == 0 and lib.pss_decode_mono_len(1) == 0 and lib.pss_decode_mono_len(2) == 1
    assert lib.pss_decode_mono_len(7) == 1 and lib.pss_decode_mono_len(8) == 2 and lib.pss_decode_mono_len(-1) == L.PSS_E_ARG
    for n in (0, 1):
        pcm, audio, dec = Engine.h_decode_mono(np.zeros(n, np.complex64), 2.4e6, stages=True)
        assert pcm.shape == audio.shape == dec.shape == (0,) and pcm.dtype == np.int16
    assert lib.pss_h_decode_mono(None, 0, 2.4e6, None, None, None) == 0
    x = np.zeros(8, np.complex64)
    assert lib.pss_h_decode_mono(x.ctypes.data, 8, 0.0, None, None, None) == L.PSS_E_ARG
    assert lib.pss_h_decode_mono(x.ctypes.data, -1, 2.4e6, None, None, None) == L.PSS_E_ARG


def test_deemphasis_design_equals_scipys_bilinear(g):
    import scipy.signal as ss
    lib = L.load()
    b, a = np.empty(2), np.empty(2)
    for fs in M.RATES:
        assert lib.pss_design_deemph(75e-6, fs, b.ctypes.data, a.ctypes.data) == 0
        assert same_bits(b, g[f"bz_{int(fs)}"]) and same_bits(a, g[f"az_{int(fs)}"]), fs
    # the sample-rate sweep of test_designers_equal_scipy_on_sweeps (its `rates`), both time constants
    rates = list(np.linspace(240e3, 20e6, 115)) + [250e3, 1.024e6, 2.048e6, 2.4e6, 10e6]
    for tau in (75e-6, 50e-6):
        for fs in rates:
            assert lib.pss_design_deemph(tau, fs, b.ctypes.data, a.ctypes.data) == 0
            rb, ra = ss.bilinear([1], [tau, 1], fs=fs)
            assert same_bits(b, rb) and same_bits(a, ra), (tau, fs)
    assert lib.pss_design_deemph(75e-6, 0.0, b.ctypes.data, a.ctypes.data) == L.PSS_E_ARG
    assert lib.pss_design_deemph(0.0, 1e6, b.ctypes.data, a.ctypes.data) == L.PSS_E_ARG


def test_decimator_taps_equal_scipys_firwin_as_float32(g):
    import scipy.signal as ss
    t = np.empty(121)
    assert L.load().pss_design_firwin(121, 1.0 / 6, t.ctypes.data) == 0
    assert same_bits(t.astype(np.float32), g["taps"])
    assert same_bits(t.astype(np.float32), ss.firwin(121, 1.0 / 6, window="hamming").astype(np.float32))


def test_host_lfilter_equals_the_reference(g):
    bad = []
    for p in range(len(M.LP_PARAMS)):
        b, a = g[f"lp_b_{p}"], g[f"lp_a_{p}"]
        assert len(b) == len(a) == M.LP_PARAMS[p][2] + 1
        for dt in ("float32", "float64"):
            for n in M.LP_LENGTHS:
                y = Engine.h_lfilter(M.lp_row(n, dt), b, a)
                if y.dtype != np.float64 or not matches(g, f"lp_out_{dt}_{n}_{p}", y, n >= M.LP_LONG):
                    bad.append((p, dt, n))
    assert not bad, bad
    # rows are independent, coefficients are divided by a[0]
    b, a = g["lp_b_0"], g["lp_a_0"]
    rows = M.lp_rows(3, 50)
    y = Engine.h_lfilter(rows, b, a)
    for r in range(3):
        assert same_bits(y[r], Engine.h_lfilter(rows[r], b, a))
    assert same_bits(Engine.h_lfilter(rows, 2.0 * b, 2.0 * a), y)          # a power of two: every quotient exact
    for bb, aa in ((b[:1], a[:1]), (np.ones(10), np.ones(10)), (b, a[:-1])):
        with pytest.raises(ValueError):
            Engine.h_lfilter(rows, bb, aa)
    with pytest.raises(ValueError):
        Engine.h_lfilter(rows, b, np.concatenate([[0.0], a[1:]]))


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/mono_host.cpp: pss_mono.h and pss_npsum.h with the host compiler — the header must not need HIP — under AddressSanitizer
    and UBSan, as a program of its own."""
    exe = str(tmp_path / "mono_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "mono_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mono_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_header_table_and_library_agree_on_the_new_entry_points():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    want = {"pss_decode_mono_len": 1, "pss_decode_mono": 8, "pss_h_decode_mono": 6, "pss_design_deemph": 4, "pss_lfilter": 8, "pss_h_lfilter": 7}
    for name, n_args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, f"{name} is not declared in include/pss.h"
        assert len(m.group(1).split(",")) == n_args == len(L._SIGS[name][1]), name
        assert L._SIGS[name][0] is C.c_int and hasattr(lib, name)
    # the drop-in module exports the reference's four names
    from pyspecsdr_amd import signal_processing as sp
    for name in ("decode_mono", "lowpass_filter", "butter_lowpass", "butter_bandpass"):
        assert name in sp.__all__ and callable(getattr(sp, name))
    assert ("pss_mono.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]) in __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS


def test_shim_designs_and_argument_checks_need_no_gpu():
    import scipy.signal as ss
    from pyspecsdr_amd import signal_processing as sp
    b, a = sp.butter_lowpass(3000, 22050)
    rb, ra = ss.butter(5, 3000 / (0.5 * 22050), btype="low", analog=False)
    assert same_bits(b, rb) and same_bits(a, ra)
    b, a = sp.butter_bandpass(300.0, 3000.0, 22050, order=3)
    rb, ra = ss.butter(3, [300.0 / 11025.0, 3000.0 / 11025.0], btype="band")
    assert same_bits(b, rb) and same_bits(a, ra)
    with pytest.raises(TypeError):
        sp.lowpass_filter(np.zeros(8, np.complex64))
    with pytest.raises(ValueError):
        sp.lowpass_filter(np.zeros((2, 2, 2)))

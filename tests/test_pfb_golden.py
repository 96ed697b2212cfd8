"""The polyphase channeliser's host twin (pss_h_pfb, pss_pfb_default_taps) against tests/golden/pfb.npz — no GPU.  The arithmetic is the
project's own (pyspecsdr_amd/csrc/pss_pfb.h), so the truth is computed outside it: the definition evaluated directly in 80-bit long
double with exactly reduced phases (tools/make_goldens_pfb.py).

  output   |float64(y32) - ref| <= 1/2 ulp_float32(max(|ref|, |y32|)) + (ceil(T / M) + 4 log2 M + 8) 2^-53 sum|h| max(|xr|, |xi|) on each
           part: the float32 rounding of the result, the branch's fma chain, log2 M butterfly stages with one table rounding each.
  ddc      row c is pss_h_ddc's channel of word c 2^64 / M (exact): the two float32 results differ by at most 1 ulp_float32 plus both
           statements' float64 bounds.
  shape    any split of [m_begin, m_end), any chunking of the capture with exactly the needed halo: the same bytes.
tests/test_gpu_pfb.py (-m gpu) holds the kernel to the twin bit for bit.  tests/pfb_host.cpp runs the header alone under
AddressSanitizer and UBSan.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bytes_util import same_bytes, zeros_alike
import pfb_cases as PC
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "pfb.npz"))


def test_fixture_inputs_are_what_the_makers_give_today(g):
    assert int(g["version"]) == PC.VERSION
    assert [c[1:4] for c in PC.CASES] == [(2, 2, 5), (4, 4, 81), (8, 4, 161), (8, 3, 50), (8, 8, 1), (8, 1, 17), (64, 32, 1281), (1024, 512, 20481)]
    for name, M, D, T, n, lead, _, _ in PC.CASES:
        x, h = PC.case_capture(name), PC.case_taps(name)
        assert len(x) == n and int(g[f"crc_{name}"]) == PC.crc(x), name
        assert len(h) == T and int(g[f"hcrc_{name}"]) == PC.crc(h), name
        assert g[f"ref_hi_{name}"].shape == (len(PC.case_channels(name)), len(PC.case_instants(name)))
        assert float(g[f"sumh_{name}"]) == np.abs(h).sum() and float(g[f"xmax_{name}"]) == max(np.abs(x.real).max(), np.abs(x.imag).max())
    assert int(g["chain_crc"]) == PC.crc(PC.chain_capture())


def test_golden_cases_are_inside_the_output_bound(g):
    worst, most = [], -np.inf
    for name, M, D, T, n, lead, _, _ in PC.CASES:
        x, h = PC.case_capture(name), PC.case_taps(name)
        ins, ch = PC.case_instants(name), PC.case_channels(name)
        if len(ins) == -(-n // D):
            y = Engine.h_pfb(x, M, D, taps=h, lead=lead)
            assert y.shape == (M, -(-n // D)) and y.dtype == np.complex64
            y = y[ch]
        else:                                                              # a subset of instants: one call each
            y = np.concatenate([Engine.h_pfb(x, M, D, taps=h, lead=lead, m_begin=m, m_end=m + 1) for m in ins], axis=1)[ch]
        excess, used = PC.bound_excess(y, g[f"ref_hi_{name}"], g[f"ref_lo_{name}"], M, T, float(g[f"sumh_{name}"]), float(g[f"xmax_{name}"]))
        print(f"{name}: excess {excess:.3e}; error beyond the float32 half ulp: {used:.3f} of {PC.f64_units(M, T)} units")
        worst.append((excess, name))
        most = max(most, used)
    print(f"worst case: {most:.3f} units of 2^-53 sum|h| max|x| beyond the float32 half ulp (negative: inside the float32 rounding alone)")
    assert max(worst)[0] <= 0, max(worst)


def test_rows_are_the_down_converters_channels_at_the_grid_words():
    """pss_h_ddc with word c 2^64 / M computes the same quantity by another statement: rotor, mix, one long chain."""
    for name, M, D, T, n, lead, _, _ in PC.CASES:
        if T > 4097:
            continue                                                       # pss_ddc's tap limit
        x, h = PC.case_capture(name), PC.case_taps(name)
        y = Engine.h_pfb(x, M, D, taps=h, lead=lead)
        words = [c * ((1 << 64) // M) for c in range(M)]
        z = Engine.h_ddc(x, words, D, taps=h, lead=lead)
        assert y.shape == z.shape
        unit = 2.0 ** -53 * np.abs(h).sum()
        f64 = PC.f64_units(M, T) * unit * max(np.abs(x.real).max(), np.abs(x.imag).max()) + (T + 8) * unit * np.abs(x.astype(np.complex128)).max() * (1 + 2.0 ** -50)
        for a, b in ((y.real, z.real), (y.imag, z.imag)):
            a, b = a.astype(np.float64), b.astype(np.float64)
            ulp = 2 * PC.half_ulp32(np.maximum(np.abs(a), np.abs(b)))
            assert np.all(np.abs(a - b) <= ulp + f64), (name, float(np.max(np.abs(a - b) - ulp - f64)))


def test_the_shape_of_the_call_changes_no_byte():
    for M, D, T, n, lead in ((8, 3, 50, 3001, 13), (16, 16, 161, 3001, 0), (4, 2, 41, 2001, 40)):
        x = PC.capture(n, 77)
        h = np.random.default_rng([53, M]).standard_normal(T) / 12
        n_out = -(-n // D)
        whole = Engine.h_pfb(x, M, D, taps=h, lead=lead)
        assert whole.shape == (M, n_out)
        cuts = [0, 1, 2, 57, 58, n_out // 2, n_out - 1, n_out]
        for a, b in zip(cuts[:-1], cuts[1:]):                              # [m_begin, m_end) split at arbitrary points
            assert zeros_alike(Engine.h_pfb(x, M, D, taps=h, lead=lead, m_begin=a, m_end=b)) == zeros_alike(whole[:, a:b]), (a, b)
            lo, hi = max(0, a * D + lead - (T - 1)), min(n, (b - 1) * D + lead + 1)   # buffers with exactly the needed halo
            part = Engine.h_pfb(x[lo:hi], M, D, taps=h, lead=lead, buf_index0=lo, n_capture=n, m_begin=a, m_end=b)
            assert zeros_alike(part) == zeros_alike(whole[:, a:b]), (a, b, lo, hi)


def definition_f64(x, index0, n_capture, h, M, D, lead, instants):
    """The definition in float64 with the phase reduced exactly in Python integers -> complex128 [M][len(instants)].  Its own error per part
    is at most (T + 4) 2^-53 sum|h| sqrt(2) max|x part|: a product pair, a rotation and a T-term sum."""
    T = len(h)
    ang = 2 * np.pi * np.arange(M) / M
    out = np.zeros((M, len(instants)), np.complex128)
    for a, m in enumerate(instants):
        for k in range(T):
            j = m * D + lead - k
            if 0 <= j < n_capture:
                q = (np.arange(M) * (j % M)) % M
                out[:, a] += h[k] * complex(x[j - index0]) * (np.cos(ang[q]) - 1j * np.sin(ang[q]))
    return out


def test_a_buffer_past_2_to_the_40_follows_the_definition():
    M, D, T, lead, n_buf = 8, 3, 50, 13, 400
    index0, n_cap = (1 << 40) + 12345, 1 << 41
    x = PC.capture(n_buf, 78)
    h = np.random.default_rng(54).standard_normal(T) / 8
    a = -(-(index0 + (T - 1) - lead) // D)
    b = (index0 + n_buf - 1 - lead) // D + 1
    y = Engine.h_pfb(x, M, D, taps=h, lead=lead, buf_index0=index0, n_capture=n_cap, m_begin=a, m_end=b)
    assert y.shape == (M, b - a) and b - a > 100
    ref = definition_f64(x, index0, n_cap, h, M, D, lead, range(a, b))
    unit = 2.0 ** -53 * np.abs(h).sum() * max(np.abs(x.real).max(), np.abs(x.imag).max())
    tol = (PC.f64_units(M, T) + (T + 4) * np.sqrt(2)) * unit
    for p, r in ((y.real, ref.real), (y.imag, ref.imag)):
        p = p.astype(np.float64)
        assert np.all(np.abs(p - r) <= PC.half_ulp32(np.maximum(np.abs(p), np.abs(r))) + tol)
    # the phase is the capture's: the same buffer D samples later turns row c by exp(-2 pi i c D / M)
    z = Engine.h_pfb(x, M, D, taps=h, lead=lead, buf_index0=index0 + D, n_capture=n_cap, m_begin=a + 1, m_end=b + 1)
    turn = np.exp(-2j * np.pi * np.arange(M) * D / M)[:, None]
    assert np.abs(z - y * turn).max() <= 1e-6 * np.abs(y).max() and np.abs(z[1] - y[1]).max() > 0.1 * np.abs(y[1]).max()


def test_default_taps_equal_scipys_firwin(g):
    for M in PC.TAP_CHANS:
        assert same_bytes(Engine.pfb_default_taps(M), g[f"taps_{M}"]), M
    assert len(Engine.pfb_default_taps(256)) == 5121
    for M in (0, 1, -2, 3, 48, 2048):
        with pytest.raises(ValueError):
            Engine.pfb_default_taps(M)
    x = PC.capture(700, 79)
    assert same_bytes(Engine.h_pfb(x, 8, 4), Engine.h_pfb(x, 8, 4, taps=Engine.pfb_default_taps(8), lead=80))


def test_refused_arguments_say_why():
    lib = L.load()
    n, M, D, T = 1000, 8, 5, 101
    x = np.ascontiguousarray(PC.capture(n, 80))
    h = np.ascontiguousarray(np.random.default_rng(55).standard_normal(T))
    out = np.full((M, 200), -7.25, np.complex64)
    nan_taps, inf_taps = h.copy(), h.copy()
    nan_taps[7], inf_taps[100] = np.nan, -np.inf
    long_taps = np.zeros(32 * M + 1)
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    good = dict(iq=x, n_buf=n, buf_index0=0, n_capture=n, n_chan=M, decim=D, taps=h, n_taps=T, lead=50, m_begin=0, m_end=200, out=out, out_stride=200)
    order = ["iq", "n_buf", "buf_index0", "n_capture", "n_chan", "decim", "taps", "n_taps", "lead", "m_begin", "m_end", "out", "out_stride"]

    def call(**change):
        a = dict(good)
        a.update(change)
        return lib.pss_h_pfb(*[p(a[k]) if k in ("iq", "taps", "out") else a[k] for k in order])

    assert call() == 0
    ok = out.copy()
    bad = [dict(n_chan=0), dict(n_chan=1), dict(n_chan=6), dict(n_chan=2048), dict(n_chan=-8), dict(decim=0), dict(decim=M + 1), dict(n_taps=0),
           dict(taps=long_taps, n_taps=32 * M + 1), dict(lead=-1), dict(lead=T), dict(taps=nan_taps), dict(taps=inf_taps),
           dict(iq=None), dict(taps=None), dict(out=None), dict(iq=x.ctypes.data + 4), dict(out=out.ctypes.data + 4),
           dict(n_capture=-1), dict(n_buf=-1), dict(buf_index0=-1), dict(n_capture=n - 1), dict(buf_index0=1),
           dict(m_begin=-1), dict(m_begin=3, m_end=2), dict(m_end=201), dict(out_stride=199),
           dict(n_buf=n - 1),                                              # output 199 needs sample 999
           dict(buf_index0=10, n_buf=n - 10)]                              # output 0 needs sample 0
    for b in bad:
        lib.pss_h_ddc_rotor(0, -1, 0, None, None)                          # leaves a message of its own behind
        before = lib.pss_last_error(None)
        assert call(**b) == L.PSS_E_ARG, b
        msg = lib.pss_last_error(None)
        assert msg and msg.startswith(b"pss_h_pfb: ") and msg != before, (b, msg)
    assert same_bytes(out, ok)                                             # a refused call writes nothing
    # an empty range is no error and needs no buffers
    assert call(m_begin=7, m_end=7, out=None, iq=None) == 0
    n_taps = C.c_int()
    assert lib.pss_pfb_default_taps(8, None, None) == L.PSS_E_ARG and lib.pss_pfb_default_taps(8, None, C.byref(n_taps)) == 0 and n_taps.value == 161
    assert lib.pss_pfb_default_taps(12, None, C.byref(n_taps)) == L.PSS_E_ARG and lib.pss_last_error(None).startswith(b"pss_pfb_default_taps: ")


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/pfb_host.cpp: pss_pfb.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "pfb_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "pfb_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pfb_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_header_table_and_library_agree_on_the_new_entry_points():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in ("pss_pfb_default_taps", "pss_pfb", "pss_h_pfb"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    build = open(os.path.join(ROOT, "pyspecsdr_amd", "build.py")).read()
    assert '("pss_pfb.hip", ["-ffp-contract=off"])' in build


def test_python_layers_check_their_arguments_without_a_gpu():
    from pyspecsdr_amd import formats as F
    off = F.bank_offsets(2.4e6, 64)
    assert off.dtype == np.float64 and off.shape == (64,) and off[0] == 0 and off[16] == 600e3 and off[48] == -600e3 and off[32] == -1.2e6 and off[31] == 31 * 37500.0
    for m in (0, 1, 3, 2048):
        with pytest.raises(ValueError):
            F.bank_offsets(1.0, m)
    with pytest.raises(ValueError):
        F.demodulate_bank(np.zeros(10, np.complex64), 2.4e6, 64, mode="FM")
    with pytest.raises(ValueError):
        F.demodulate_bank(np.zeros(10, np.complex64), 2.4e6, 64, frame_len=0)
    with pytest.raises(ValueError):
        F.demodulate_bank(np.zeros(10, np.complex64), 2.4e6, 64, decim=65)
    with pytest.raises(ValueError):
        Engine.h_pfb(np.zeros((2, 2), np.complex64), 2, 1)
    with pytest.raises(ValueError):
        Engine.h_pfb(np.zeros(4, np.complex64), 3, 1)
    assert Engine.h_pfb(np.zeros(0, np.complex64), 4, 2).shape == (4, 0)

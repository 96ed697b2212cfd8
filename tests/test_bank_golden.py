"""The band-plan channeliser's host twin (pss_h_bank, pss_bank_default_taps: grids of 2^a 3^b 5^c channels) against
tests/golden/bank.npz — no GPU.  The arithmetic is the project's own (pyspecsdr_amd/csrc/pss_bank.h), so the truth is computed outside
it: the definition evaluated directly in 80-bit long double with exactly reduced phases (tools/make_goldens_bank.py).

  output   |float64(y32) - ref| <= 1/2 ulp_float32(max(|ref|, |y32|)) + (ceil(T / M) + sum of u(r) over the stages + 8) 2^-53 sum|h|
           max(|xr|, |xi|) on each part, u(2) = 4, u(3) = 7, u(5) = 9 (bank_cases.f64_units; the count is pss_bank.h's).
  ddc      row c is pss_h_ddc's channel at the word nearest c 2^64 / M: the two float32 results differ by at most 1 ulp_float32 plus both
           statements' float64 bounds (the margin tests/test_pfb_golden.py applies to its grid words).
  pfb      a power-of-two M is pss_h_pfb's bytes.
  shape    any split of [m_begin, m_end), any chunking of the capture with exactly the needed halo: the same bytes.
tests/test_gpu_bank.py (-m gpu) holds the kernel to the twin bit for bit.  tests/bank_host.cpp runs the header alone under
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
import bank_cases as BC
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "bank.npz"))


def test_fixture_inputs_are_what_the_makers_give_today(g):
    assert int(g["version"]) == BC.VERSION
    assert [c[1:6] for c in BC.CASES] == [(3, 3, 7, 100, 3), (5, 2, 26, 203, 12), (6, 3, 121, 600, 60), (12, 5, 50, 500, 13), (15, 15, 1, 203, 0),
                                          (45, 1, 17, 150, 16), (96, 48, 1921, 4001, 960), (192, 48, 3841, 8001, 1920), (625, 125, 2501, 6001, 1250),
                                          (729, 243, 2917, 7001, 1458), (1000, 500, 20001, 40001, 10000)]
    for name, M, D, T, n, lead, _, _ in BC.CASES:
        x, h = BC.case_capture(name), BC.case_taps(name)
        assert len(x) == n and int(g[f"crc_{name}"]) == BC.crc(x), name
        assert len(h) == T and int(g[f"hcrc_{name}"]) == BC.crc(h), name
        ins, ch = BC.case_instants(name), BC.case_channels(name)
        assert g[f"ref_hi_{name}"].shape == (len(ch), len(ins))
        if M >= 192:                                                       # the kept subset: the ends, the middle, the band edge
            n_out = -(-n // D)
            assert {0, n_out // 2, n_out - 1} <= set(ins) and {0, 1, M // 2 - 1, M // 2, M // 2 + 1, M - 1} <= set(ch) and len(ch) == 7
        assert float(g[f"sumh_{name}"]) == np.abs(h).sum() and float(g[f"xmax_{name}"]) == max(np.abs(x.real).max(), np.abs(x.imag).max())
    assert int(g["chain_crc"]) == BC.crc(BC.chain_capture())
    assert BC.f64_units(96, 1921) == 21 + 4 * 5 + 7 + 8 and BC.f64_units(1000, 20001) == 21 + 4 * 3 + 9 * 3 + 8 and BC.f64_units(729, 1) == 1 + 7 * 6 + 8


def test_golden_cases_are_inside_the_output_bound(g):
    worst, most = [], -np.inf
    for name, M, D, T, n, lead, _, _ in BC.CASES:
        x, h = BC.case_capture(name), BC.case_taps(name)
        ins, ch = BC.case_instants(name), BC.case_channels(name)
        if len(ins) == -(-n // D):
            y = Engine.h_bank(x, M, D, taps=h, lead=lead)
            assert y.shape == (M, -(-n // D)) and y.dtype == np.complex64
            y = y[ch]
        else:                                                              # a subset of instants: one call each
            y = np.concatenate([Engine.h_bank(x, M, D, taps=h, lead=lead, m_begin=m, m_end=m + 1) for m in ins], axis=1)[ch]
        excess, used = BC.bound_excess(y, g[f"ref_hi_{name}"], g[f"ref_lo_{name}"], M, T, float(g[f"sumh_{name}"]), float(g[f"xmax_{name}"]))
        print(f"{name}: excess {excess:.3e}; error beyond the float32 half ulp: {used:.3f} of {BC.f64_units(M, T)} units")
        worst.append((excess, name))
        most = max(most, used)
    print(f"worst case: {most:.3f} units of 2^-53 sum|h| max|x| beyond the float32 half ulp (negative: inside the float32 rounding alone)")
    assert max(worst)[0] < 0, max(worst)


def test_rows_are_the_down_converters_channels_at_the_nearest_words():
    """pss_h_ddc at the word nearest c 2^64 / M computes the same quantity by another statement: rotor, mix, one long chain.  The word is
    off c 2^64 / M by at most 1/2, so sample j turns by at most j 2^-65 of a turn more: at most n 2^-65 of a turn over a capture of n
    samples, below 2^-50 of a turn for the n <= 10^4 here — under one of the down-converter's T + 8 units where n <= 600, under 12 of
    its more than 1900 at the largest n.  The comparison and the margin are test_pfb_golden.py's for its grid words."""
    done = []
    for name, M, D, T, n, lead, _, _ in BC.CASES:
        if T > 4097 or n > 10 ** 4:
            continue                                                       # pss_ddc's tap limit; the small cases
        x, h = BC.case_capture(name), BC.case_taps(name)
        y = Engine.h_bank(x, M, D, taps=h, lead=lead)
        words = [((c << 64) + M // 2) // M for c in range(M)]              # the integer nearest c 2^64 / M (no ties: M is no power of two)
        z = Engine.h_ddc(x, words, D, taps=h, lead=lead)
        assert y.shape == z.shape
        unit = 2.0 ** -53 * np.abs(h).sum()
        f64 = BC.f64_units(M, T) * unit * max(np.abs(x.real).max(), np.abs(x.imag).max()) + (T + 8) * unit * np.abs(x.astype(np.complex128)).max() * (1 + 2.0 ** -50)
        for a, b in ((y.real, z.real), (y.imag, z.imag)):
            a, b = a.astype(np.float64), b.astype(np.float64)
            ulp = 2 * BC.half_ulp32(np.maximum(np.abs(a), np.abs(b)))
            assert np.all(np.abs(a - b) <= ulp + f64), (name, float(np.max(np.abs(a - b) - ulp - f64)))
        done.append(M)
    assert done == [3, 5, 6, 12, 15, 45, 96, 192, 625, 729]


def test_a_power_of_two_is_the_polyphase_channelisers_bytes():
    for M, D, T, n, lead in ((2, 2, 5, 101, 2), (64, 32, 1281, 2501, 640), (64, 24, 300, 2001, 17), (1024, 512, 2049, 3001, 1024)):
        x = BC.capture(n, 81)
        h = np.random.default_rng([58, M]).standard_normal(T) / 12
        assert same_bytes(Engine.h_bank(x, M, D, taps=h, lead=lead), Engine.h_pfb(x, M, D, taps=h, lead=lead)), M
    x = BC.capture(700, 82)
    assert same_bytes(Engine.h_bank(x, 8, 4), Engine.h_pfb(x, 8, 4))
    for M in (2, 64, 1024):
        assert same_bytes(Engine.bank_default_taps(M), Engine.pfb_default_taps(M))


def test_the_shape_of_the_call_changes_no_byte():
    for M, D, T, n, lead in ((12, 5, 50, 3001, 13), (15, 15, 161, 3001, 0), (6, 2, 41, 2001, 40), (45, 9, 100, 2500, 50)):
        x = BC.capture(n, 77)
        h = np.random.default_rng([53, M]).standard_normal(T) / 12
        n_out = -(-n // D)
        whole = Engine.h_bank(x, M, D, taps=h, lead=lead)
        assert whole.shape == (M, n_out)
        cuts = [0, 1, 2, 57, 58, n_out // 2, n_out - 1, n_out]
        for a, b in zip(cuts[:-1], cuts[1:]):                              # [m_begin, m_end) split at arbitrary points
            assert zeros_alike(Engine.h_bank(x, M, D, taps=h, lead=lead, m_begin=a, m_end=b)) == zeros_alike(whole[:, a:b]), (a, b)
            lo, hi = max(0, a * D + lead - (T - 1)), min(n, (b - 1) * D + lead + 1)   # buffers with exactly the needed halo
            part = Engine.h_bank(x[lo:hi], M, D, taps=h, lead=lead, buf_index0=lo, n_capture=n, m_begin=a, m_end=b)
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
    M, D, T, lead, n_buf = 240, 48, 50, 13, 2000
    index0, n_cap = (1 << 40) + 12345, 1 << 41
    x = BC.capture(n_buf, 78)
    h = np.random.default_rng(54).standard_normal(T) / 8
    a = -(-(index0 + (T - 1) - lead) // D)
    b = (index0 + n_buf - 1 - lead) // D + 1
    y = Engine.h_bank(x, M, D, taps=h, lead=lead, buf_index0=index0, n_capture=n_cap, m_begin=a, m_end=b)
    assert y.shape == (M, b - a) and b - a > 30
    ref = definition_f64(x, index0, n_cap, h, M, D, lead, range(a, b))
    unit = 2.0 ** -53 * np.abs(h).sum() * max(np.abs(x.real).max(), np.abs(x.imag).max())
    tol = (BC.f64_units(M, T) + (T + 4) * np.sqrt(2)) * unit
    for p, r in ((y.real, ref.real), (y.imag, ref.imag)):
        p = p.astype(np.float64)
        assert np.all(np.abs(p - r) <= BC.half_ulp32(np.maximum(np.abs(p), np.abs(r))) + tol)
    # the phase is the capture's: the same buffer one sample later turns row c by exp(-2 pi i c / M)
    z = Engine.h_bank(x, M, D, taps=h, lead=lead + 1, buf_index0=index0 + 1, n_capture=n_cap, m_begin=a, m_end=b)
    turn = np.exp(-2j * np.pi * np.arange(M) / M)[:, None]
    assert np.abs(z - y * turn).max() <= 1e-6 * np.abs(y).max() and np.abs(z[60] - y[60]).max() > 0.1 * np.abs(y[60]).max()


def test_default_taps_equal_scipys_firwin(g):
    assert BC.TAP_CHANS == [3, 12, 192, 1000]
    for M in BC.TAP_CHANS:
        assert same_bytes(Engine.bank_default_taps(M), g[f"taps_{M}"]), M
    assert len(Engine.bank_default_taps(240)) == 4801
    for M in (0, 1, -2, 7, 14, 49, 1025, 1080, 2048):
        with pytest.raises(ValueError):
            Engine.bank_default_taps(M)
    x = BC.capture(700, 79)
    assert same_bytes(Engine.h_bank(x, 12, 4), Engine.h_bank(x, 12, 4, taps=Engine.bank_default_taps(12), lead=120))


def test_refused_arguments_say_why():
    lib = L.load()
    n, M, D, T = 1000, 12, 5, 101
    x = np.ascontiguousarray(BC.capture(n, 80))
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
        return lib.pss_h_bank(*[p(a[k]) if k in ("iq", "taps", "out") else a[k] for k in order])

    assert call() == 0
    ok = out.copy()
    bad = [dict(n_chan=0), dict(n_chan=1), dict(n_chan=7), dict(n_chan=14), dict(n_chan=49), dict(n_chan=1025), dict(n_chan=1080), dict(n_chan=-6),
           dict(decim=0), dict(decim=M + 1), dict(n_taps=0),
           dict(taps=long_taps, n_taps=32 * M + 1), dict(lead=-1), dict(lead=T), dict(taps=nan_taps), dict(taps=inf_taps),
           dict(iq=None), dict(taps=None), dict(out=None), dict(iq=x.ctypes.data + 4), dict(out=out.ctypes.data + 4),
           dict(n_capture=-1), dict(n_buf=-1), dict(buf_index0=-1), dict(n_capture=n - 1), dict(buf_index0=1),
           dict(m_begin=-1), dict(m_begin=3, m_end=2), dict(m_end=201), dict(out_stride=199),
           dict(n_buf=n - 1),                                              # output 199 needs sample 999
           dict(buf_index0=10, n_buf=n - 10),                              # output 0 needs sample 0
           dict(n_chan=8, decim=9), dict(n_chan=8, taps=np.zeros(257), n_taps=257)]   # a power of two is refused here too, in this call's name
    for b in bad:
        lib.pss_h_ddc_rotor(0, -1, 0, None, None)                          # leaves a message of its own behind
        before = lib.pss_last_error(None)
        assert call(**b) == L.PSS_E_ARG, b
        msg = lib.pss_last_error(None)
        assert msg and msg.startswith(b"pss_h_bank: ") and msg != before, (b, msg)
    assert same_bytes(out, ok)                                             # a refused call writes nothing
    # an empty range is no error and needs no buffers
    assert call(m_begin=7, m_end=7, out=None, iq=None) == 0
    n_taps = C.c_int()
    assert lib.pss_bank_default_taps(12, None, None) == L.PSS_E_ARG and lib.pss_bank_default_taps(12, None, C.byref(n_taps)) == 0 and n_taps.value == 241
    assert lib.pss_bank_default_taps(14, None, C.byref(n_taps)) == L.PSS_E_ARG and lib.pss_last_error(None).startswith(b"pss_bank_default_taps: ")


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/bank_host.cpp: pss_bank.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as a
    program of its own."""
    exe = str(tmp_path / "bank_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "bank_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bank_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_header_table_and_library_agree_on_the_new_entry_points():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    for name in ("pss_bank_default_taps", "pss_bank", "pss_h_bank"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L._SIGS and getattr(lib, name)
    assert L._SIGS["pss_bank"] == L._SIGS["pss_pfb"] and L._SIGS["pss_h_bank"] == L._SIGS["pss_h_pfb"]
    build = open(os.path.join(ROOT, "pyspecsdr_amd", "build.py")).read()
    assert '("pss_bank.hip", ["-ffp-contract=off"])' in build
    head = open(os.path.join(CSRC, "pss_bank.h")).read()
    for line in ("u(2) = 4", "u(3) = 7", "u(5) = 9", "return (T + M - 1) / M + 4 * n2 + 7 * n3 + 9 * n5 + 8;"):
        assert line in head, line                                          # bank_cases.f64_units restates the header's count
    assert (BC.U3, BC.U5) == (7, 9)


def test_plan_bank_turns_a_spacing_into_a_bank():
    from pyspecsdr_amd import formats as F
    assert F.plan_bank(2.4e6, 12.5e3) == (192, 48)                         # 50 kS/s: the NFM demodulator needs more than 30 kS/s
    assert F.plan_bank(10e6, 25e3) == (400, 200)                           # 50 kS/s
    assert F.plan_bank(2.4e6, 10e3) == (240, 48)
    assert F.plan_bank(2.4e6, 25e3) == (96, 48) and F.plan_bank(10e6, 12.5e3) == (800, 200) and F.plan_bank(10e6, 10e3) == (1000, 200)
    assert F.plan_bank(2.4e6, 25e3, min_rate=25e3) == (96, 96) and F.plan_bank(2.4e6, 12.5e3, min_rate=2.4e6) == (192, 1)
    assert F.plan_bank(2.4e6, 37.5e3) == (64, 32)                          # a power of two is a plan like any other
    with pytest.raises(ValueError, match="not an integer"):
        F.plan_bank(2.4e6, 8333.0)
    with pytest.raises(ValueError) as err:
        F.plan_bank(7e3 * 343, 7e3)
    assert "343" in str(err.value) and "324" in str(err.value) and "360" in str(err.value)
    with pytest.raises(ValueError) as err:
        F.plan_bank(10e6, 6.25e3)                                          # 1600 channels: 5-smooth but above the limit
    assert "1600" in str(err.value) and "1024" in str(err.value)
    for bad in ((0.0, 1.0), (1.0, 0.0), (-2.4e6, 12.5e3)):
        with pytest.raises(ValueError):
            F.plan_bank(*bad)
    with pytest.raises(ValueError):
        F.plan_bank(24e3, 12e3)                                            # the capture's own rate is below the default min_rate


def test_plan_offsets_and_rows():
    from pyspecsdr_amd import formats as F
    assert np.array_equal(F.plan_offsets(5.0, 5), [0.0, 1.0, 2.0, -2.0, -1.0])                 # odd: no band-edge row
    assert np.array_equal(F.plan_offsets(6.0, 6), [0.0, 1.0, 2.0, -3.0, -2.0, -1.0])           # even: row M / 2 reads -fs / 2
    off = F.plan_offsets(2.4e6, 192)
    assert off.dtype == np.float64 and off.shape == (192,) and off[0] == 0 and off[24] == 300e3 and off[159] == -412.5e3 and off[96] == -1.2e6 and off[95] == 95 * 12.5e3
    assert np.array_equal(F.plan_offsets(2.4e6, 64), F.bank_offsets(2.4e6, 64))
    for m in (0, 1, 7, 14, 1080, 2048):
        with pytest.raises(ValueError):
            F.plan_offsets(1.0, m)
    rows = F.plan_rows(2.4e6, 446e6, [446e6 + 300e3, 446e6 - 412.5e3, 446e6, 446e6 - 1.2e6, 446e6 + 1.2e6, 446e6 + 12500.4], 12.5e3)
    assert rows.tolist() == [24, 159, 0, 96, 96, 1]
    with pytest.raises(ValueError) as err:
        F.plan_rows(2.4e6, 446e6, [446e6 + 300e3, 446e6 + 300040.0, 446e6 + 1.3e6, 446e6 - 12.5e3], 12.5e3)
    assert "446300040.0" in str(err.value) and "447300000.0" in str(err.value) and "446300000.0" not in str(err.value) and "445987500.0" not in str(err.value)
    with pytest.raises(ValueError):
        F.monitor_channels(np.zeros(10, np.complex64), 2.4e6, 0.0, [0.0], 12.5e3, mode="FM")
    with pytest.raises(ValueError):
        F.monitor_channels(np.zeros(10, np.complex64), 2.4e6, 0.0, [0.0], 12.5e3, frame_len=0)
    with pytest.raises(TypeError):
        F.monitor_channels(np.zeros(10, np.complex64), 2.4e6, 0.0, [0.0], 12.5e3, nonsense=1)
    with pytest.raises(ValueError):
        Engine.h_bank(np.zeros((2, 2), np.complex64), 6, 1)
    with pytest.raises(ValueError):
        Engine.h_bank(np.zeros(4, np.complex64), 7, 1)
    assert Engine.h_bank(np.zeros(0, np.complex64), 6, 2).shape == (6, 0)

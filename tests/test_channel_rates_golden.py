"""The CPU oracle and the library's filter designers pinned at the channel rates (no GPU, no reference, no SciPy at test time):
tests/golden/channel_rates.npz holds what the reference's demodulate_signal returns for one frame at each of
channel_rate_cases.GOLDEN_LENGTHS and each rate of NFM_RATES / WFM_RATES / SSB_RATES, with SciPy's filter tables
(tools/make_goldens_channel_rates.py).  tests/test_gpu_length_sweep.py compares the device with this oracle at these rates; these tests
are what makes that comparison a measurement of the device.

Criteria, those of tests/test_lengths_golden.py: bit for bit (NaN matching NaN), except the SSB float64 audio at lengths that are no power
of two, where the oracle skips the reference's hilbert() round trip (2e-14, int16 equal).
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import channel_rate_cases as CR
import length_cases as LC
import oracle_lib as O
from pyspecsdr_amd import _lib as L

NFM = [fs for fs, _, _ in CR.NFM_RATES]
WFM = [fs for fs, _, _ in CR.WFM_RATES]
SSB = [fs for fs, _, _ in CR.SSB_RATES]


@pytest.fixture(scope="module")
def g(golden):
    return golden["channel_rates"]


@pytest.fixture(scope="module")
def frames(g):
    """The read buffers, regenerated from their seeds; the fixture holds a digest of each."""
    out = {}
    for n in CR.GOLDEN_LENGTHS:
        x = LC.fm_frames(1, n, seed=1)[0]
        crc = np.frombuffer(hashlib.blake2b(np.ascontiguousarray(x).tobytes(), digest_size=16).digest(), np.uint8)
        assert np.array_equal(crc, g[f"crc_{n}"]), n
        out[n] = x
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def test_lists_and_fixture_agree(g):
    assert list(g["lengths"]) == CR.GOLDEN_LENGTHS and len(CR.GOLDEN_LENGTHS) == 12
    assert list(g["nfm_rates"]) == NFM and list(g["wfm_rates"]) == WFM and list(g["ssb_rates"]) == SSB
    assert list(g["nfm_refused"]) == CR.NFM_REFUSED and list(g["wfm_refused"]) == CR.WFM_REFUSED
    assert set(CR.GOLDEN_LENGTHS) <= set(LC.DEMOD_LENGTHS) and set(CR.GOLDEN_LENGTHS) - set(LC.GOLDEN_DEMOD_LENGTHS) == {61}
    for n in (29, 30, 129, 257, 1024, 1025, 2049):
        assert n in CR.GOLDEN_LENGTHS
    factors = {q for _, q, _ in CR.NFM_RATES + CR.WFM_RATES}
    assert factors == {1, 2, 3, 4, 5, 10}
    assert any(all((n - 1) % q == 0 for q in factors) for n in CR.GOLDEN_LENGTHS)        # n_out = (n - 1) / q exactly, at every rate
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "channel_rates.npz")) < 543304   # bank.npz


def test_every_rate_has_the_factor_stated():
    for fs, q, _ in CR.NFM_RATES + CR.WFM_RATES:
        assert int(fs / 22050) == q == CR.factor(fs), fs
        assert L.load().pss_demod_out_len(L.MODE_NFM, 1025, fs) == -(-1024 // q)
    assert [q for _, q, _ in CR.NFM_RATES] == [1, 2, 2, 2, 3, 5] and [q for _, q, _ in CR.WFM_RATES] == [4, 5, 5, 10]
    assert all(fs / 2 > 15000 for fs in NFM) and all(fs / 2 > 53000 for fs in WFM)          # the designs exist
    assert all(not fs / 2 > 15000 for fs in CR.NFM_REFUSED) and all(not fs / 2 > 53000 for fs in CR.WFM_REFUSED)
    assert L.load().pss_demod_out_len(L.MODE_NFM, 1024, 22049.0) < 0


def test_plan_audio_rates_are_todays():
    from pyspecsdr_amd import formats as F
    assert CR.PLAN_AUDIO == {m: float(r) for m, r in F._AUDIO_MID.items()}
    for mode, rate in CR.PLAN_AUDIO.items():
        for rate_in in (50000.0, 75000.0, 48000.0):
            up, down, mid = F.plan_audio(rate_in, mode)
            assert mid == rate and rate_in * up / down == rate, (mode, rate_in)
    assert CR.PLAN_AUDIO["NFM"] in NFM and CR.PLAN_AUDIO["WFM"] in WFM and CR.PLAN_AUDIO["AM"] in SSB
    assert 2.4e6 / 50 in NFM and 2.4e6 / 48 in NFM and 2.4e6 / 32 in NFM and 2.4e6 / 64 in NFM and 2.4e6 / 20 in WFM and 2.4e6 / 10 in WFM


def _wfm_tables(g, fs):
    k = str(int(fs))
    filt = {name: g[f"{name}_{k}"] for name in ("lp_sos", "pilot_sos", "lmr_sos", "dec_sos", "dec_zi")}
    filt["alpha"] = float(g[f"alpha_{k}"])
    return filt


@pytest.mark.parametrize("fs", NFM, ids=CR.rate_id)
def test_nfm_equals_the_reference(g, frames, fs):
    k = str(int(fs))
    for n in CR.GOLDEN_LENGTHS:
        with np.errstate(all="ignore"):
            a = O.demod_nfm(frames[n], fs, g[f"taps_{k}"], g[f"dec_sos_{k}"], g[f"dec_zi_{k}"])
        assert len(a) == -(-(n - 1) // CR.factor(fs)) and same_bits(a, g[f"nfm_{n}_{k}"]), (fs, n)


@pytest.mark.parametrize("fs", WFM, ids=CR.rate_id)
def test_wfm_equals_the_reference(g, frames, fs):
    filt = _wfm_tables(g, fs)
    for n in CR.GOLDEN_LENGTHS:
        with np.errstate(all="ignore"):
            w = O.demod_wfm(O.iq_correction(frames[n]), fs, filt)
        assert w is not None and w.shape == (-(-(n - 1) // CR.factor(fs)), 2) and same_bits(w, g[f"wfm_{n}_{int(fs)}"]), (fs, n)


@pytest.mark.parametrize("fs", SSB, ids=lambda fs: str(int(fs)))
def test_ssb_equals_the_reference(g, frames, fs):
    taps = g[f"ssb_taps_{int(fs)}"]
    for n in CR.GOLDEN_LENGTHS:
        a, want = O.demod_ssb(frames[n], taps), g[f"ssb_{n}_{int(fs)}"]
        if n & (n - 1) == 0:
            assert same_bits(a, want), (fs, n)        # the real FIR and SciPy's hilbert() round trip, every bit
        else:
            assert np.allclose(a, want, rtol=0, atol=2e-14), (fs, n)
        assert np.array_equal(O.pcm16_stereo(a)[:, 0], np.int16(want * 32767)), (fs, n)


def test_the_librarys_designs_equal_scipys_tables(g):
    """pss_design_firwin / cheby1_sos / sosfilt_zi / butter_sos and the de-emphasis alpha (NumPy's exp restated, pss_h_np_f64) against the
    fixture's SciPy tables at every channel rate, cheby1(8, 0.05, 0.8) at q = 1 and the rates below 240 kS/s included: np.array_equal,
    the criterion of test_abi_and_design (every bit of every value; the sign of a section's structural zero is not compared)."""
    lib = L.load()
    taps, sos, zi = np.empty(65), np.empty((4, 6)), np.empty((4, 2))
    for fs in sorted(set(NFM + WFM)):
        k, q = str(int(fs)), CR.factor(fs)
        assert lib.pss_design_firwin(65, 15000 / (fs / 2), taps.ctypes.data) == 0
        assert lib.pss_design_cheby1_sos(8, 0.05, 0.8 / q, sos.ctypes.data) == 0
        assert lib.pss_design_sosfilt_zi(sos.ctypes.data, 4, zi.ctypes.data) == 0
        assert np.array_equal(taps, g["taps_" + k]) and np.array_equal(sos, g["dec_sos_" + k]) and np.array_equal(zi, g["dec_zi_" + k]), fs
    for fs in WFM:
        k, nyq = str(int(fs)), fs / 2
        for name, lo, hi, ns in (("lp_sos", 0.0, 15000.0, 3), ("pilot_sos", 18800.0, 19200.0, 5), ("lmr_sos", 23000.0, 53000.0, 5)):
            s, n = np.zeros((ns, 6)), C.c_int()
            assert lib.pss_design_butter_sos(5, lo / nyq, hi / nyq, s.ctypes.data, C.addressof(n)) == 0 and n.value == ns
            assert np.array_equal(s, g[f"{name}_{k}"]), (fs, name)
        x, a = np.array([-1 / (75e-6 * fs)]), np.empty(1)
        assert lib.pss_h_np_f64(1, x.ctypes.data, 1, a.ctypes.data) == 0 and np.array_equal(a, g["alpha_" + k].reshape(1)), fs
    for fs in SSB:
        assert lib.pss_design_firwin(65, 3000 / fs, taps.ctypes.data) == 0
        assert np.array_equal(taps, g[f"ssb_taps_{int(fs)}"]), fs


def test_the_designers_refuse_where_scipy_raises(g):
    lib = L.load()
    taps, sos = np.empty(65), np.zeros((5, 6))
    for fs in g["nfm_refused"]:
        assert lib.pss_design_firwin(65, 15000 / (fs / 2), taps.ctypes.data) == L.PSS_E_CUTOFF, fs
    for fs in g["wfm_refused"]:
        assert lib.pss_design_butter_sos(5, 23000 / (fs / 2), 53000 / (fs / 2), sos.ctypes.data, None) == L.PSS_E_CUTOFF, fs

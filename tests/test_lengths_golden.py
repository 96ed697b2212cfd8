"""The CPU oracle pinned at the length sweep's frame lengths (no GPU, no reference at test time): tests/golden/lengths.npz holds what the
reference returns for one frame at each of length_cases.GOLDEN_LENGTHS (tools/make_goldens_lengths.py), and NumPy itself is the
reference of the two summation trees at every length of REDUCE_LENGTHS.  tests/test_gpu_length_sweep.py compares the device with this
oracle at every length of the lists; these tests are what makes that comparison a measurement of the device.

Criteria: bit for bit (NaN matching NaN), except what the existing golden tests except — SSB float64 audio at lengths that are no power
of two, where the oracle skips the reference's hilbert() round trip (2e-14, int16 equal: test_oracle_golden.test_ssb), and the classifier's
PSD and flatness (the bounds of test_oracle_golden's classifier tests).
"""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import length_cases as LC
import oracle_lib as O


@pytest.fixture(scope="module")
def g(golden):
    return golden["lengths"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "c":
        a, b = a.view(a.real.dtype), b.view(b.real.dtype)
    u = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def _digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).digest(), np.uint8)


def test_lists_and_fixture_agree(g):
    assert list(g["lengths"]) == LC.GOLDEN_DEMOD_LENGTHS and list(g["long_lengths"]) == LC.GOLDEN_LONG_LENGTHS
    for n in (29, 129, 152, 255, 419, 1023, 1025, 2047, 2049):
        assert n in LC.GOLDEN_DEMOD_LENGTHS
    for n in (8193, 8199, 65537, 65543):
        assert n in LC.GOLDEN_LONG_LENGTHS
    assert len(LC.GOLDEN_LENGTHS) == 28
    # the stored read buffers are those the makers give today (the GPU sweep draws from the same makers)
    for n in LC.GOLDEN_DEMOD_LENGTHS:
        assert same_bits(LC.fm_frames(1, n, seed=1)[0], g[f"fm_{n}"]) and same_bits(LC.iq_frames(1, n, seed=1)[0], g[f"iq_{n}"]), n
    for n in LC.GOLDEN_LONG_LENGTHS:
        assert np.array_equal(_digest(LC.iq_frames(1, n, seed=1)[0]), g[f"crc_{n}"]), n


def test_every_batch_of_the_makers_is_made_of_different_frames():
    for maker in (LC.fm_frames, LC.iq_frames, LC.power_frames, LC.c128_frames):
        for n in (1, 2, 7, 129, 1024):
            assert LC.repeats(maker(65, n)) == 0, (maker.__name__, n)
        x = maker(3, 8)
        assert LC.repeats(np.concatenate([x, x[:1]])) == 1


@pytest.mark.parametrize("fs", [2.4e6, 250e3])
def test_nfm_and_wfm_equal_the_reference(g, fs):
    k = str(int(fs))
    filt = {name: g[f"{name}_{k}"] for name in ("lp_sos", "pilot_sos", "lmr_sos", "dec_sos", "dec_zi")}
    filt["alpha"] = float(g[f"alpha_{k}"])
    for n in LC.GOLDEN_DEMOD_LENGTHS:
        x = g[f"fm_{n}"]
        with np.errstate(all="ignore"):
            a = O.demod_nfm(x, fs, g[f"taps_{k}"], g[f"dec_sos_{k}"], g[f"dec_zi_{k}"])
            w = O.demod_wfm(O.iq_correction(x), fs, filt)
        assert same_bits(a, g[f"nfm_{n}_{k}"]), ("NFM", fs, n)
        assert w is not None and same_bits(w, g[f"wfm_{n}_{k}"]), ("WFM", fs, n)


def test_am_equals_the_reference(g):
    for n in LC.GOLDEN_DEMOD_LENGTHS:
        with np.errstate(all="ignore"):
            assert same_bits(O.demod_am(g[f"iq_{n}"], g["am_sos"]), g[f"am_{n}"]), n


@pytest.mark.parametrize("fs", [2.4e6, 48e3])
def test_ssb_equals_the_reference(g, fs):
    taps = g[f"ssb_taps_{int(fs)}"]
    for n in LC.GOLDEN_DEMOD_LENGTHS:
        a, want = O.demod_ssb(g[f"fm_{n}"], taps), g[f"ssb_{n}_{int(fs)}"]
        if n & (n - 1) == 0:
            assert same_bits(a, want), (fs, n)        # the real FIR and SciPy's hilbert() round trip, every bit
        else:
            assert np.allclose(a, want, rtol=0, atol=2e-14), (fs, n)
        assert np.array_equal(O.pcm16_stereo(a)[:, 0], np.int16(want * 32767)), (fs, n)


def test_iq_correction_and_power_equal_the_reference(g):
    for n in LC.GOLDEN_DEMOD_LENGTHS:
        x = g[f"iq_{n}"]
        assert same_bits(O.iq_correction(x), g[f"corr_{n}"]), n
        assert same_bits(np.array(O.power_db(x)), g[f"pw_{n}"]), n
    for n in LC.GOLDEN_LONG_LENGTHS:     # a chunk and a group tail of fewer than 8 elements
        x = LC.iq_frames(1, n, seed=1)[0]
        c = O.iq_correction(x)
        assert same_bits(c[:64], g[f"corr_head_{n}"]) and same_bits(c[-64:], g[f"corr_tail_{n}"]), n
        assert np.array_equal(_digest(c), g[f"corr_digest_{n}"]), n
        assert same_bits(np.array(O.power_db(x)), g[f"pw_{n}"]), n


def test_classifier_equals_the_reference(g):
    fs = float(g["classify_fs"])
    for n in LC.GOLDEN_DEMOD_LENGTHS:
        with np.errstate(all="ignore"):
            lab, bw, mi, fl, psd = O.classify(g[f"fm_{n}"], fs)
        ref = g[f"psd_{n}"]
        assert lab == str(g[f"label_{n}"]) and bw == float(g[f"bw_{n}"]), n
        assert same_bits(np.array(mi), g[f"mi_{n}"]), (n, mi, g[f"mi_{n}"])
        rfl = float(g[f"flat_{n}"])
        assert float(fl) == rfl or abs(float(fl) - rfl) <= 1e-5 * abs(rfl), (n, fl, rfl)
        assert psd.shape == ref.shape
        assert np.all(np.abs(psd - ref) <= 1e-5 * (ref + 1e-10) + 1e-6 * np.sqrt(ref * np.max(ref))), n


def test_float32_tree_equals_numpy_at_every_reduce_length():
    bad = []
    for n in LC.REDUCE_LENGTHS:
        a = np.ascontiguousarray(LC.power_frames(1, n)[0].real)
        if O.pairwise_sum_f32(a).tobytes() != np.add.reduce(a).tobytes():
            bad.append(n)
    assert not bad, bad[:20]


def test_complex64_tree_equals_numpy_at_every_reduce_length():
    bad = []
    for n in LC.REDUCE_LENGTHS:
        x = LC.power_frames(1, n)[0]
        if O.csum_f32(x).tobytes() != np.add.reduce(x).tobytes():
            bad.append(n)
    assert not bad, bad[:20]

"""The CPU oracle against tests/golden/adc.npz (tools/make_goldens_adc.py): the reference's outputs on ADC-quantised read buffers —
exact zeros of both signs, ties, samples on the rails, discriminator products that cancel exactly (tests/adc_cases.py).

Comparisons are made on BIT PATTERNS (adc_cases.same_bits: -0 is not +0; NaN equals NaN) wherever the contract is "the reference's bits";
np.array_equal calls a -0 equal to a +0, and iq_correction's output differed from the reference's in exactly that.
"""
import numpy as np
import pytest

import adc_cases as A
import oracle_lib as O
import spectrum_bounds as SB

FS = A.FS
GOLDEN = [c.name for c in A.golden_cases()]


@pytest.fixture(scope="module")
def g(golden):
    return golden["adc"]


@pytest.fixture(scope="module")
def filt(golden):
    nfm, wfm, am = golden["nfm"], golden["wfm"], golden["am_ssb"]
    key = str(int(FS))
    return {"nfm": (nfm["design_taps_" + key], nfm["design_sos_" + key], nfm["design_zi_" + key]),
            "wfm": {k: wfm[f"{k}_{key}"] for k in ("lp_sos", "pilot_sos", "lmr_sos", "alpha", "dec_sos", "dec_zi")},
            "am_sos": am["am_sos"], "ssb_taps": am["ssb_taps_a"]}


def test_cases_hold_what_they_are_there_for():
    """Every case against its FLOORS; the named headline floors of the issue; the variants really carry -0 words."""
    for c in A.cases():
        k = A.counts(c.iq)
        for key, floor in A.FLOORS[c.name].items():
            assert k[key] >= floor, (c.name, key, k[key], floor)
    k = A.counts(A.by_name("i8_floor_fm_32768").iq)
    assert k["disc_pi"] >= 1000 and k["zero_samples"] >= 10000 and k["prod_im_neg0"] >= 1000 and k["prod_re_neg0"] >= 1000
    assert A.counts(A.by_name("dead_zero_1024").iq)["db_m100"] == 1024
    assert A.counts(A.by_name("dead_rails_1024").iq)["max_ties"] == 1024
    for c in A.cases():
        signed = c.name.rsplit("_", 1)[-1] in ("conj", "negre", "neg", "sprinkle")
        nz = A.counts(c.iq)["neg_zero_words"]
        if signed and ("_floor_" in c.name or "_weak_" in c.name):
            assert nz >= 1, c.name
        if not signed:
            assert nz == 0, c.name          # built from integer codes: every zero is +0
    assert sorted({c.n for c in A.cases()}) == sorted(A.LENGTHS)
    assert len({c.name.split("_")[0] for c in A.cases()} & set(A.GRIDS)) == 4


def test_fixture_is_data_of_these_cases(g):
    assert [str(v) for v in g["cases"]] == GOLDEN
    for c in A.golden_cases():
        assert int(g[f"crc_{c.name}"]) == A.crc(c.iq), c.name     # the generator still yields the buffers the fixture was made from
    for k in g.files:
        assert g[k].dtype.kind in "fciuU", k                       # arrays of numbers and tags only


def test_same_bits_tells_zeros_apart():
    a = np.array([0.0, -0.0, np.nan, 1.0], np.float32)
    assert A.same_bits(a, a.copy()) and np.array_equal(a[:2], -a[:2])
    assert not A.same_bits(a, np.array([-0.0, -0.0, np.nan, 1.0], np.float32))
    assert not A.same_bits(a, np.array([0.0, -0.0, 1.0, 1.0], np.float32))
    z = np.array([complex(0.0, -0.0)], np.complex64)
    assert not A.same_bits(z, np.conj(z)) and A.same_bits(z.astype(np.complex128), z.astype(np.complex128))


def _have(g, item, name):
    """True if the reference returned `item` for the case; the oracle's behaviour where it raised is not pinned here."""
    return f"err_{item}_{name}" not in g.files


@pytest.mark.parametrize("name", GOLDEN)
def test_iq_correction_and_raw_bits(g, name):
    x = A.by_name(name).iq
    got = O.iq_correction(x)
    assert A.same_bits(got, g[f"corr_{name}"]), A.diff_bits(got, g[f"corr_{name}"])
    if f"raw_{name}" in g.files:
        assert A.same_bits(got.real.copy(), g[f"raw_{name}"]), A.diff_bits(got.real.copy(), g[f"raw_{name}"])


@pytest.mark.parametrize("name", GOLDEN)
def test_wfm_bits(g, filt, name):
    """demodulate_signal(..., 'WFM') = iq_correction + demodulate_wfm: every float64 bit of both channels, and the int16."""
    x = A.by_name(name).iq
    assert _have(g, "wfm", name)
    with np.errstate(all="ignore"):
        a = O.demod_wfm(O.iq_correction(x), FS, filt["wfm"])
        assert a is not None
        want = g[f"wfm_{name}"]
        assert A.same_bits(a, want), A.diff_bits(a, want)
        assert np.array_equal(np.int16(a * 32767), g[f"wfm_pcm_{name}"])


@pytest.mark.parametrize("name", GOLDEN)
def test_nfm_am_bits(g, filt, name):
    x = A.by_name(name).iq
    with np.errstate(all="ignore"):
        a = O.demod_nfm(x, FS, *filt["nfm"])
        assert A.same_bits(a, g[f"nfm_{name}"]), A.diff_bits(a, g[f"nfm_{name}"])
        assert np.array_equal(O.pcm16_stereo(a), g[f"nfm_pcm_{name}"])
        if f"am_{name}" in g.files:
            a = O.demod_am(x, filt["am_sos"])
            assert A.same_bits(a, g[f"am_{name}"]), A.diff_bits(a, g[f"am_{name}"])
            assert np.array_equal(O.pcm16_stereo(a), g[f"am_pcm_{name}"])


@pytest.mark.parametrize("name", [n for n in GOLDEN if A.by_name(n).n < 32768])
def test_ssb(g, filt, name):
    """USB = LSB in the reference (asserted when the fixture was made).  Frames of 2^k samples: every bit; other lengths: 2e-14."""
    x = A.by_name(name).iq
    n = len(x)
    with np.errstate(all="ignore"):
        a = O.demod_ssb(x, filt["ssb_taps"])
        want = g[f"usb_{name}"]
        if n & (n - 1) == 0:
            assert A.same_bits(a, want), A.diff_bits(a, want)
        else:
            assert np.array_equal(np.isnan(a), np.isnan(want)) and np.allclose(a, want, rtol=0, atol=2e-14, equal_nan=True), A.diff_bits(a, want)
        assert np.array_equal(O.pcm16_stereo(a), g[f"usb_pcm_{name}"])


@pytest.mark.parametrize("name", GOLDEN)
def test_spectrum_power_scanner(g, name):
    x = A.by_name(name).iq
    with np.errstate(all="ignore"):
        db, ref = O.compute_fft(x), g[f"db_{name}"]
        # two float64 transforms of the same row: spectrum_bounds' allowance (its derivation covers a bin that is all rounding noise —
        # a stuck converter's row away from DC — where no relative bound on the dB value holds)
        assert SB.check_f64(db[None], ref[None], SB.db_allowance(ref[None], SB.delta(x))) is None, np.max(np.abs(db - ref))
        if not x.any():
            assert A.same_bits(db, ref)                        # an all-zero buffer: exactly -100
        if f"post_{name}" in g.files:
            post = O.postprocess(ref)
            assert post.shape == g[f"post_{name}"].shape and np.allclose(post, g[f"post_{name}"], rtol=1e-13, atol=1e-12)
        p = O.power_db(x)
        assert A.same_bits(np.array(p), g[f"power_{name}"]), (p, g[f"power_{name}"])
        if f"scan_db_{name}" in g.files:
            sdb, pk, bw, cnt = O.scan_slice(x, FS)
            ref = g[f"scan_db_{name}"]
            assert A.same_bits(sdb, ref), A.diff_bits(sdb, ref)
            assert A.same_bits(np.array(pk), g[f"scan_peak_{name}"]) and bw == float(g[f"scan_bw_{name}"])


@pytest.mark.parametrize("name", GOLDEN)
def test_classify(g, name):
    """test_classify_signal's bars: label and bandwidth equal, the float32 modulation index bit for bit, flatness to 1e-5."""
    x = A.by_name(name).iq
    with np.errstate(all="ignore"):
        lab, bw, mi, fl, _ = O.classify(x, FS)
    assert lab == str(g[f"cls_label_{name}"]) and bw == float(g[f"cls_bw_{name}"]), (lab, bw, g[f"cls_label_{name}"], g[f"cls_bw_{name}"])
    assert A.same_bits(np.array(mi), g[f"cls_mi_{name}"]), (mi, g[f"cls_mi_{name}"])
    rfl = float(g[f"cls_flat_{name}"])
    assert float(fl) == rfl or abs(float(fl) - rfl) <= 1e-5 * abs(rfl) or (np.isnan(fl) and np.isnan(rfl)), (fl, rfl)


def test_history_cells(g):
    """draw_waterfall / draw_persistence over the 1024-sample cases' rows, all-zero buffer first: where the reference drew, the oracle's
    grids are its grids; where it raised (a flat history: max == min), only that fact is stored."""
    H, W = [int(v) for v in g["hist_hw"]]
    dh, dw = H - 4, W - 8
    rows = np.stack([g[f"post_{n}"] for n in g["hist_cases"]])
    assert int(g["wf_err"][0]) == 1 and not g["wf_err"][1:].any() and not g["ps_err"].any()
    assert np.ptp(rows[0]) == 0
    with np.errstate(all="ignore"):
        for i in range(len(rows)):
            if not g["wf_err"][i]:
                gl, co = O.waterfall_cells(rows[max(0, i + 1 - 30):i + 1], dh, dw)
                assert np.array_equal(gl, g["wf_glyph"][i]) and np.array_equal(co, g["wf_colour"][i]), i
            assert np.array_equal(O.persistence_cells(rows[max(0, i + 1 - 10):i + 1], dh, dw), g["ps_colour"][i]), i

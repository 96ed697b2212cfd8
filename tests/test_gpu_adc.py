"""ADC-quantised read buffers (tests/adc_cases.py) through every device entry point and kernel family, every frame against the CPU oracle
and the fixture's cases against tests/golden/adc.npz as well.

What these buffers hold that no other test input does: components that are exactly zero, of either sign; runs of equal magnitude on the
rails; discriminator products that cancel exactly, so that atan2 sits on its +-pi branch; all-zero, stuck and one-sample frames.  Batches
interleave unlike cases frame by frame (a dead frame beside a clipped one), so a lane-per-frame kernel holds unlike neighbours; every
frame is compared with the oracle's result for that frame ALONE, which is the isolation check.

Contracts are those of the per-path tests, unchanged: bits (adc_cases.same_bits: -0 is not +0, NaN equals NaN) wherever the contract is
"bit-exact"; float32 dB rows within 1e-4 relative, db_exact / float64 rows within spectrum_bounds' float64 allowance; register-Hilbert
SSB audio within 2e-14 on frames of 2^k samples and bits under hilbert_exact; the float32-arithmetic pipeline as
test_full_size_headline_properties treats it.  Output buffers start as 0x7f bytes (test_gpu_squelch.sentinel).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import adc_cases as A
import gpu_util as G
import oracle_lib as O
import spectrum_bounds as SB
import squelch_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats
from pyspecsdr_amd.engine import h_squelch_gate

FS = A.FS
W, H = 112, 36
SSB_ATOL = 2e-14
DB_REL = 1e-4
SCAN_DIFF_RATE = 3 / 146912        # test_gpu_full_batch: two float64 transforms can round a weak bin either way in float32


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def _mixed(n):
    """The cases of length n as (a live one, a clipped one, a dead one) and so on while each kind lasts: frame 0 is live (a waterfall's
    history must not start flat) and dead frames have a frame on the rails for a neighbour."""
    pool = A.of_length(n)
    kinds = [[c for c in pool if c.kind != "dead" and "_clip_" not in c.name], [c for c in pool if c.kind != "dead" and "_clip_" in c.name],
             [c for c in pool if c.kind == "dead"]]
    out = []
    while any(kinds):
        for k in kinds:
            out += k[:1]
            del k[:1]
    return out


class Batch:
    def __init__(self, label, cases):
        self.label, self.cases = label, cases
        self.nf, self.n = len(cases), cases[0].n
        self.iq = np.stack([c.iq for c in cases])
        self.names = [c.name for c in cases]

    def dev(self):
        return G.dev(self.iq.view(np.float32).reshape(self.nf, self.n, 2))

    def __repr__(self):
        return self.label


_BATCHES = {}


def batch(label):
    """'<nf>x<n>': nf frames cycled from the mixed cases of length n; '1x1024': the sprinkled noise-floor case alone."""
    if label not in _BATCHES:
        nf, n = (int(v) for v in label.split("x"))
        pool = _mixed(n)
        if nf == 1:
            pool = [A.by_name("i8_floor_mpx_1024_sprinkle")] if n == 1024 else pool[:1]
        _BATCHES[label] = Batch(label, [pool[k % len(pool)] for k in range(nf)])
    return _BATCHES[label]


def batch_8192():
    """The 16 384-sample cases cut to their first 8192 samples (k_ssb_rfft's other length); compared with the oracle only."""
    if "8192" not in _BATCHES:
        cs = [A.Case(c.name + "_cut8192", np.ascontiguousarray(c.iq[:8192]), c.kind) for c in _mixed(16384)]
        _BATCHES["8192"] = Batch("5x8192", [cs[k % len(cs)] for k in range(5)])
    return _BATCHES["8192"]


SMALL = ["1x1024", "70x1024", "130x1024", "9x29", "70x1000", "5x4096", "5x16384", "12x32768"]


def sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0x7F)
    return t


# ---- the oracle, once per case ----------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle(what, b, fn):
    """[fn(case.iq) for the batch's frames], each distinct case evaluated once."""
    with np.errstate(all="ignore"):
        todo = [c for c in {c.name: c for c in b.cases}.values() if (what, c.name) not in _ORACLE]
        for c, r in zip(todo, O.map_frames(fn, [c.iq for c in todo])):
            _ORACLE[(what, c.name)] = r
    return [_ORACLE[(what, name)] for name in b.names]


_GOLD = None


def gold():
    global _GOLD
    if _GOLD is None:
        import os
        _GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adc.npz"))
    return _GOLD


class Report:
    """Failing frames per criterion; check() names them with their cases."""

    def __init__(self, label, b):
        self.label, self.b, self.bad = label, b, {}

    def frames(self, what, got, want, same=A.same_bits):
        for k in range(self.b.nf):
            if not same(got[k], want[k]):
                self.bad.setdefault(what, []).append(k)

    def golden(self, what, got, key, same=A.same_bits):
        """Frames whose case is in the fixture, against the reference's own output `key`_<case>."""
        g = gold()
        seen = set()
        for k, c in enumerate(self.b.cases):
            name = f"{key}_{c.name}"
            if c.golden and name in g.files and c.name not in seen:
                seen.add(c.name)
                if not same(got[k], g[name]):
                    self.bad.setdefault(what + " (adc.npz)", []).append(k)

    def add(self, what, frames):
        if len(frames):
            self.bad.setdefault(what, []).extend(int(f) for f in frames)

    def check(self):
        msg = [f"{what}: {len(f)} frames, first {[(k, self.b.names[k]) for k in f[:6]]}" for what, f in self.bad.items()]
        assert not msg, f"{self.label} [{self.b.label}]: " + "; ".join(msg)


def eq(a, b):
    return bool(np.array_equal(a, b))


def close(atol):
    def same(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        na, nb = np.isnan(a), np.isnan(b)
        with np.errstate(invalid="ignore"):
            return a.shape == b.shape and bool(np.all(np.where(na | nb, na & nb, np.abs(a - b) <= atol)))
    return same


def db_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= DB_REL * np.maximum(np.abs(b), 1.0)))


class options:
    """Engine options for the length of a with block, restored to the given defaults after it."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, (v, _) in self.kv.items():
            G.engine().set_option(k, v)

    def __exit__(self, *exc):
        G.engine().sync()
        for k, (_, d) in self.kv.items():
            G.engine().set_option(k, d)


def _filters(e):
    taps, sos, zi = e.nfm_filters(FS)
    lp, pil, lmr, alpha = e.wfm_filters(FS)
    am = np.empty((5, 6))
    e.lib.pss_am_bandpass_sos(am.ctypes.data)
    return {"nfm": (taps, sos, zi), "wfm": dict(lp_sos=lp, pilot_sos=pil, lmr_sos=lmr, alpha=alpha, dec_sos=sos, dec_zi=zi), "am": am,
            "ssb": e.ssb_taps(FS)}


def _demod(e, mode, d_iq, b, signal=False):
    n_out = e.demod_out_len(mode, b.n, FS)
    pcm = sentinel((b.nf, n_out, 2), torch.int16)
    au = sentinel((b.nf, n_out, 2) if mode == L.MODE_WFM else (b.nf, n_out), torch.float64)
    (e.demod_signal if signal else e.demod)(mode, d_iq, b.nf, b.n, FS, pcm, au)
    e.sync()
    return G.host(pcm), G.host(au)


def int16_of(a):
    v = np.asarray(a, np.float64) * 32767.0
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), 0.0, np.trunc(v)).astype(np.int32).astype(np.int16)


def test_the_batches_interleave_unlike_cases():
    b = batch("130x1024")
    kinds = [c.kind for c in b.cases]
    assert kinds[0] != "dead" and kinds.count("dead") >= 30 and all(kinds[k] != "dead" or kinds[k - 1] != "dead" for k in range(1, b.nf))
    assert len(set(b.names)) == len(A.of_length(1024)) >= 30
    assert sum(kinds[k] == "dead" and "_clip_" in b.names[k - 1] for k in range(1, b.nf)) >= 12     # dead frames right after a clipped one
    neg = sum(A.counts(c.iq)["neg_zero_words"] > 0 for c in b.cases)
    assert neg >= 20
    assert batch("12x32768").nf == 12 and len(set(batch("12x32768").names)) == len(A.of_length(32768))


# ---- NFM --------------------------------------------------------------------------------------------------------------------------------
NFM_FAMILIES = {"small_batch": dict(), "fused": dict(small_batch=(0, 1)), "three_kernel": dict(small_batch=(0, 1), nfm_fused=(0, 1))}


@pytest.mark.parametrize("family", list(NFM_FAMILIES))
@pytest.mark.parametrize("label", SMALL + ["8193x1024"])
def test_nfm(label, family):
    """8193 x 1024: one frame past small_batch_max = 8192 (the dispatcher leaves the small-batch array there whatever the option says)."""
    e, b = G.engine(), batch(label)
    f = _filters(e)
    want = oracle("nfm", b, lambda x: O.demod_nfm(x, FS, *f["nfm"]))
    with options(**NFM_FAMILIES[family]):
        pcm, au = _demod(e, L.MODE_NFM, b.dev(), b)
    R = Report(f"NFM {family}", b)
    R.frames("float64 audio bits", au, want)
    R.frames("int16 PCM", pcm, [O.pcm16_stereo(a) for a in want], eq)
    R.golden("float64 audio bits", au, "nfm")
    R.golden("int16 PCM", pcm, "nfm_pcm", eq)
    R.check()


# ---- WFM, iq_correction, RAW ------------------------------------------------------------------------------------------------------------
WFM_FAMILIES = {"small_batch": dict(), "fused": dict(small_batch=(0, 1)), "fused_corr_copy": dict(small_batch=(0, 1), wfm_corr_copy=(1, 0)),
                "unfused": dict(small_batch=(0, 1), wfm_fused=(0, 1))}


@pytest.mark.parametrize("family", list(WFM_FAMILIES))
@pytest.mark.parametrize("label", SMALL + ["6001x1024"])
def test_wfm(label, family):
    """demodulate_signal(WFM) = iq_correction + demodulate_wfm from the buffers as read (the correction inside the forward kernel, or a
    corrected copy first), and pss_iq_correction + pss_demod as separate calls.  6001 x 1024: one frame past wfm_small_batch_max."""
    e, b = G.engine(), batch(label)
    f = _filters(e)
    want = oracle("wfm", b, lambda x: O.demod_wfm(O.iq_correction(x), FS, f["wfm"]))
    d_iq = b.dev()
    with options(**WFM_FAMILIES[family]):
        pcm, au = _demod(e, L.MODE_WFM, d_iq, b, signal=True)
        corr = sentinel((b.nf, b.n, 2), torch.float32)
        e.iq_correction(d_iq, b.nf, b.n, corr, None)
        pcm2, au2 = _demod(e, L.MODE_WFM, corr, b)
    R = Report(f"WFM {family}", b)
    for tag, p, a in (("dispatcher", pcm, au), ("correction + demod", pcm2, au2)):
        R.frames(f"{tag}: float64 audio bits", a, want)
        R.frames(f"{tag}: int16 PCM", p, [int16_of(w) for w in want], eq)
        R.golden(f"{tag}: float64 audio bits", a, "wfm")
        R.golden(f"{tag}: int16 PCM", p, "wfm_pcm", eq)
    R.check()


@pytest.mark.parametrize("label", SMALL + ["6001x1024"])
def test_iq_correction_and_raw(label):
    e, b = G.engine(), batch(label)
    want = oracle("corr", b, O.iq_correction)
    out, raw = sentinel((b.nf, b.n, 2), torch.float32), sentinel((b.nf, b.n), torch.float32)
    e.iq_correction(b.dev(), b.nf, b.n, out, raw)
    e.sync()
    out, raw = G.host(out).view(np.complex64).reshape(b.nf, b.n), G.host(raw)
    R = Report("iq_correction / RAW", b)
    R.frames("corrected samples, bits", out, want)
    R.frames("RAW, bits", raw, [w.real.copy() for w in want])
    R.golden("corrected samples, bits", out, "corr")
    R.golden("RAW, bits", raw, "raw")
    R.check()
    signed = [k for k, c in enumerate(b.cases) if A.counts(c.iq)["neg_zero_words"] and np.isfinite(want[k].view(np.float32)).all()]
    if label == "130x1024":
        assert len(signed) >= 20        # the comparison above saw -0 input words, and the signs of the zeros that came out of them


# ---- AM, SSB ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small_batch", [1, 0])
@pytest.mark.parametrize("label", SMALL)
def test_am(label, small_batch):
    e, b = G.engine(), batch(label)
    f = _filters(e)
    want = oracle("am", b, lambda x: O.demod_am(x, f["am"]))
    with options(small_batch=(small_batch, 1)):
        pcm, au = _demod(e, L.MODE_AM, b.dev(), b)
    R = Report(f"AM small_batch={small_batch}", b)
    R.frames("float64 audio bits", au, want)
    R.frames("int16 PCM", pcm, [O.pcm16_stereo(a) for a in want], eq)
    R.golden("float64 audio bits", au, "am")
    R.golden("int16 PCM", pcm, "am_pcm", eq)
    R.check()


SSB_FAMILIES = {"default": dict(), "hilbert_exact": dict(hilbert_exact=(1, 0)), "no_hilbert": dict(ssb_hilbert=(0, 1)), "no_rfft": dict(ssb_rfft=(0, 1)),
                "no_rfft_exact": dict(ssb_rfft=(0, 1), hilbert_exact=(1, 0))}


SSB_CASES = [(label, family) for label in SMALL + ["5x8192"] for family in SSB_FAMILIES
             if not family.startswith("no_rfft") or label in ("5x8192", "5x16384")]      # ssb_rfft selects a kernel at 8192 / 16 384 samples only


@pytest.mark.parametrize("mode", [L.MODE_USB, L.MODE_LSB], ids=["usb", "lsb"])
@pytest.mark.parametrize("label,family", SSB_CASES)
def test_ssb(label, family, mode):
    """USB = LSB in the reference.  Frames of 2^k samples: the register Hilbert round trip within 2e-14 (int16 equal), every bit under
    hilbert_exact; other lengths and ssb_hilbert = 0: every bit of the oracle's audio.  ssb_rfft acts at 8192 / 16 384 samples."""
    e = G.engine()
    b = batch_8192() if label == "5x8192" else batch(label)
    f = _filters(e)
    hil = family != "no_hilbert"
    want = oracle("ssb" if hil else "ssb_nohil", b, lambda x: O.demod_ssb(x, f["ssb"], hilbert=hil))
    with options(**SSB_FAMILIES[family]):
        pcm, au = _demod(e, mode, b.dev(), b)
    pow2 = b.n & (b.n - 1) == 0
    R = Report(f"SSB {family}", b)
    if pow2 and hil and "exact" not in family:
        R.frames("float64 audio beyond 2e-14", au, want, close(SSB_ATOL))
        R.golden("float64 audio beyond 2e-14", au, "usb", close(SSB_ATOL))
    else:
        R.frames("float64 audio bits", au, want)
        if hil and pow2:
            R.golden("float64 audio bits", au, "usb")
        elif hil:
            R.golden("float64 audio beyond 2e-14", au, "usb", close(SSB_ATOL))
    R.frames("int16 PCM", pcm, [O.pcm16_stereo(a) for a in want], eq)
    if hil:
        R.golden("int16 PCM", pcm, "usb_pcm", eq)
    R.check()


# ---- power, demod_power -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", SMALL)
def test_power_and_demod_power(label):
    e, b = G.engine(), batch(label)
    want = oracle("power", b, O.power_db)
    d_iq = b.dev()
    pw = sentinel((b.nf,), torch.float32)
    e.power_db(d_iq, b.nf, b.n, pw)
    e.sync()
    R = Report("power_db / demod_power", b)
    R.frames("power_db bits", G.host(pw), [np.float32(w) for w in want])
    R.golden("power_db bits", G.host(pw), "power", lambda a, g: A.same_bits(np.array(a), g))
    for mode in (L.MODE_NFM, L.MODE_AM, L.MODE_USB):
        pcm, _ = _demod(e, mode, d_iq, b)
        n_out = e.demod_out_len(mode, b.n, FS)
        pcm2, pw2 = sentinel((b.nf, n_out, 2), torch.int16), sentinel((b.nf,), torch.float32)
        e.demod_power(mode, d_iq, b.nf, b.n, FS, pcm2, None, pw2)
        e.sync()
        R.frames(f"demod_power({mode}) PCM != demod", G.host(pcm2), pcm, eq)
        R.frames(f"demod_power({mode}) power bits", G.host(pw2), [np.float32(w) for w in want])
    R.check()


# ---- spectrum rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", SMALL + ["5x8192"])
def test_spectrum_rows(label):
    """float32 rows within 1e-4; db_exact: the float32 rounding of a value within float64 accuracy of the row; float64 rows (register and
    f64_plain kernels) within the float64 allowance; an all-zero frame: exactly -100 in every row type."""
    e = G.engine()
    b = batch_8192() if label == "5x8192" else batch(label)
    want = np.stack(oracle("db", b, O.compute_fft))
    allow = SB.db_allowance(want, SB.delta(b.iq))
    d_iq = b.dev()
    R = Report("spectrum_db", b)
    db = sentinel((b.nf, b.n), torch.float32)
    e.spectrum_db(d_iq, b.nf, b.n, db)
    e.sync()
    db = G.host(db)
    R.frames("float32 rows beyond 1e-4", db, want, db_rel)
    R.golden("float32 rows beyond 1e-4", db, "db", db_rel)
    dbx = sentinel((b.nf, b.n), torch.float32)
    with options(db_exact=(1, 0)):
        e.spectrum_db(d_iq, b.nf, b.n, dbx)
    dbx = G.host(dbx)
    R.add("db_exact rows outside the float64 allowance", [k for k in range(b.nf) if SB.check_exact(dbx[k:k + 1], want[k:k + 1], allow[k:k + 1])])
    rows = {"db_exact": dbx}
    if b.n & (b.n - 1) == 0 and 16 <= b.n <= 65536:
        for plain in (0, 1):
            d64 = sentinel((b.nf, b.n), torch.float64)
            with options(f64_plain=(plain, 0)):
                e.spectrum_db_f64(d_iq, b.nf, b.n, d64)
            d64 = G.host(d64)
            R.add(f"float64 rows (f64_plain={plain}) outside the float64 allowance",
                  [k for k in range(b.nf) if SB.check_f64(d64[k:k + 1], want[k:k + 1], allow[k:k + 1])])
            rows[f"f64_plain={plain}"] = d64
    for k, c in enumerate(b.cases):
        if not c.iq.any():
            for tag, r in rows.items():
                if not (r[k] == -100.0).all():
                    R.add(f"{tag}: an all-zero frame is not -100 everywhere", [k])
    R.check()


def _post_numpy(rows):
    """np.convolve(row, np.ones(5) / 5, 'valid'), np.median - 10, the clamp (pyspecsdr.py:2278-2283), as the float64 kernels' test states it."""
    m = rows.shape[1] - 4
    out = []
    for r in rows:
        sm = r[0:m] * 0.2
        for j in range(1, 5):
            sm = sm + r[j:j + m] * 0.2
        with np.errstate(invalid="ignore"):
            med = np.median(sm)
            sm = sm.copy()
            sm[sm < med - 10] = med - 10
        out.append(sm)
    return np.stack(out)


@pytest.mark.parametrize("label", SMALL + ["5x8192"])
def test_post_process(label):
    """The caller's post-process on the oracle's rows of these buffers (flat rows, rows of rounding noise around -100, heavy ties): float64
    kernels (register select and f64_plain) bit for bit NumPy's formula with the rows' extremes; float32 kernels (sort up to 8192 bins,
    select above) within 1e-4."""
    e = G.engine()
    b = batch_8192() if label == "5x8192" else batch(label)
    rows = np.stack(oracle("db", b, O.compute_fft))
    want = _post_numpy(rows)
    R = Report("post-process", b)
    if b.n >= 8:
        for plain in (0, 1):
            d_p, d_lo, d_hi = sentinel((b.nf, b.n - 4), torch.float64), sentinel((b.nf,), torch.float64), sentinel((b.nf,), torch.float64)
            with options(f64_plain=(plain, 0)):
                e.spectrum_post_f64(G.dev(rows), b.nf, b.n, d_p, d_lo, d_hi)
            R.frames(f"float64 rows (f64_plain={plain}), bits", G.host(d_p), want, lambda a, w: bool(np.array_equal(a, w, equal_nan=True)))
            R.frames(f"row minimum (f64_plain={plain})", G.host(d_lo), want.min(axis=1), eq)
            R.frames(f"row maximum (f64_plain={plain})", G.host(d_hi), want.max(axis=1), eq)
    r32 = rows.astype(np.float32)
    w32 = _post_numpy(r32.astype(np.float64))
    d_p, d_lo, d_hi = sentinel((b.nf, b.n - 4), torch.float32), sentinel((b.nf,), torch.float32), sentinel((b.nf,), torch.float32)
    e.spectrum_post_extremes(G.dev(r32), b.nf, b.n, d_p, d_lo, d_hi)
    e.sync()
    p = G.host(d_p)
    R.frames("float32 rows beyond 1e-4", p, w32, db_rel)
    R.frames("float32 row minimum", G.host(d_lo), p.min(axis=1), eq)
    R.frames("float32 row maximum", G.host(d_hi), p.max(axis=1), eq)
    R.check()


# ---- the main-loop steps ----------------------------------------------------------------------------------------------------------------
PIPE = ["70x1024", "130x1024", "12x32768"]        # the float64 transform of the cell-exact steps serves powers of two


@pytest.mark.parametrize("display", ["waterfall", "persistence"])
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("label", PIPE)
def test_cell_exact_steps(label, fuse, display):
    """pss_frame_pipeline_cells (NFM and WFM), pss_frame_pipeline_nfm_f64 and pss_frame_pipeline_f64: the display lines are the oracle's
    cells computed from the IQ in float64, the PCM the demodulator's, the float32 row the float64 row rounded once."""
    e, b = G.engine(), batch(label)
    f = _filters(e)
    win = 30 if display == "waterfall" else 10
    with np.errstate(all="ignore"):
        o = O.headline_f64(b.iq, FS, *f["nfm"], win, W, min(O.threads_available(), 16), pcm=True, keep_db=True, display=display, disp_h=H)
    want_wfm = [int16_of(a) for a in oracle("wfm", b, lambda x: O.demod_wfm(O.iq_correction(x), FS, f["wfm"]))]
    allow = SB.db_allowance(o["db"], SB.delta(b.iq))
    d_iq = b.dev()
    R = Report(f"cell-exact steps fuse_post={fuse} {display}", b)

    def lines(tag, a, c):
        R.frames(f"{tag}: line a", G.host(a), o["glyph"], eq)
        if display == "waterfall":
            R.frames(f"{tag}: colours", G.host(c), o["colour"], eq)

    with options(fuse_post=(fuse, 1)):
        for mode, pcm_want in ((L.MODE_NFM, o["pcm"]), (L.MODE_WFM, want_wfm)):
            n_out = e.demod_out_len(mode, b.n, FS)
            db32, db64 = sentinel((b.nf, b.n), torch.float32), sentinel((b.nf, b.n), torch.float64)
            lo, hi = sentinel((b.nf,), torch.float64), sentinel((b.nf,), torch.float64)
            la, lb, pcm = sentinel((b.nf, W), torch.int8), sentinel((b.nf, W), torch.int8), sentinel((b.nf, n_out, 2), torch.int16)
            e.frame_pipeline_cells(mode, d_iq, b.nf, b.n, FS, db32, db64, lo, hi, W, la, lb, pcm, display=display, disp_h=H)
            e.sync()
            tag = f"cells({mode})"
            lines(tag, la, lb)
            R.frames(f"{tag}: PCM", G.host(pcm), pcm_want, eq)
            d64 = G.host(db64)
            R.add(f"{tag}: float64 rows outside the float64 allowance", [k for k in range(b.nf) if SB.check_f64(d64[k:k + 1], o["db"][k:k + 1], allow[k:k + 1])])
            R.frames(f"{tag}: the float32 row is not the float64 row rounded once", G.host(db32), d64.astype(np.float32))
            R.frames(f"{tag}: row minimum", G.host(lo), o["lo"], close(1e-9))
            R.frames(f"{tag}: row maximum", G.host(hi), o["hi"], close(1e-9))
        n_out = e.demod_out_len(L.MODE_NFM, b.n, FS)
        db64, lo, hi = sentinel((b.nf, b.n), torch.float64), sentinel((b.nf,), torch.float64), sentinel((b.nf,), torch.float64)
        la, lb, pcm = sentinel((b.nf, W), torch.int8), sentinel((b.nf, W), torch.int8), sentinel((b.nf, n_out, 2), torch.int16)
        if display == "waterfall":
            e.frame_pipeline_nfm_f64(d_iq, b.nf, b.n, FS, db64, None, lo, hi, W, la, lb, pcm)
        else:
            e.frame_pipeline_f64(L.MODE_NFM, d_iq, b.nf, b.n, FS, db64, None, lo, hi, W, la, lb, pcm, display=display, disp_h=H)
        e.sync()
        lines("nfm_f64", la, lb)
        R.frames("nfm_f64: PCM", G.host(pcm), o["pcm"], eq)
    R.check()


@pytest.mark.parametrize("label", PIPE + ["70x1000"])
def test_float32_step(label):
    """pss_frame_pipeline_nfm as test_full_size_headline_properties treats it: PCM equal, dB rows within 1e-4, the post-processed rows
    within 1e-4 of the post-process of the device's own rows, the lines those of the device's own post-processed rows; without
    materialised post-processed rows: the same bytes."""
    e, b = G.engine(), batch(label)
    f = _filters(e)
    want = oracle("nfm", b, lambda x: O.demod_nfm(x, FS, *f["nfm"]))
    rows = np.stack(oracle("db", b, O.compute_fft))
    d_iq = b.dev()
    n_out = e.demod_out_len(L.MODE_NFM, b.n, FS)
    outs = []
    for materialise in (True, False):
        o = dict(db=sentinel((b.nf, b.n), torch.float32), post=sentinel((b.nf, b.n - 4), torch.float32) if materialise else None,
                 lo=sentinel((b.nf,), torch.float32), hi=sentinel((b.nf,), torch.float32), g=sentinel((b.nf, W), torch.int8),
                 c=sentinel((b.nf, W), torch.int8), pcm=sentinel((b.nf, n_out, 2), torch.int16))
        e.frame_pipeline_nfm(d_iq, b.nf, b.n, FS, o["db"], o["post"], o["lo"], o["hi"], W, o["g"], o["c"], o["pcm"])
        e.sync()
        outs.append(o)
    R = Report("float32 step", b)
    for k in ("db", "lo", "hi", "g", "c", "pcm"):
        if not torch.equal(outs[0][k].view(torch.uint8), outs[1][k].view(torch.uint8)):
            R.add(f"{k}: differs without materialised post-processed rows", [0])
    o = {k: G.host(v) for k, v in outs[0].items()}
    R.frames("int16 PCM", o["pcm"], [O.pcm16_stereo(a) for a in want], eq)
    R.frames("dB rows beyond 1e-4", o["db"], rows, db_rel)
    R.frames("post-processed rows beyond 1e-4 of the post-process of the device's rows", o["post"], [O.postprocess(r.astype(np.float64)) for r in o["db"]], db_rel)
    buf = O.HeadlineBuffers(b.nf, b.n, FS, W)
    O.lib().pss_o_waterfall_rows(np.ascontiguousarray(o["post"]).reshape(-1), b.nf, b.n - 4, 30, W, buf.glyph.reshape(-1), buf.colour.reshape(-1), 1)
    R.frames("waterfall glyphs of the device's rows", o["g"], buf.glyph, eq)
    R.frames("waterfall colours of the device's rows", o["c"], buf.colour, eq)
    R.check()


# ---- squelch, meter, bars, gradient lines -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["70x1024", "130x1024", "12x32768", "70x1000"])
def test_meter_gate_bars_gradient(label):
    """On the post-processed float64 rows of these buffers (NumPy's formula on the oracle's rows): np.max / np.mean bit for bit, the gate
    against the host gate at a squelch inside the peaks' range, the spectrum bars expanded against the oracle's spectrogram cells, the
    gradient view's newest line of every frame against the oracle's grid of the last 30 rows."""
    e, b = G.engine(), batch(label)
    rows = _post_numpy(np.stack(oracle("db", b, O.compute_fft)))
    nr, ln = rows.shape
    d_rows = G.dev(rows)
    R = Report("meter / gate / bars / gradient", b)
    d_peak, d_avg = sentinel((nr,), torch.float64), sentinel((nr,), torch.float64)
    e.row_meter(d_rows, nr, ln, d_peak, d_avg)
    e.sync()
    want_peak, want_avg = S.meter_model(rows)
    peak = G.host(d_peak)
    R.frames("Peak", peak, want_peak, S.same_bits)
    R.frames("Avg", G.host(d_avg), want_avg, S.exact_bits)
    squelch = float(np.median(want_peak))
    assert want_peak.min() < squelch <= want_peak.max()
    for every, phase in ((3, 0), (1, 0), (7, 5), (0, 0)):
        d_open, d_idx = sentinel((nr,), torch.uint8), sentinel((nr,), torch.int32)
        n_open, held = e.squelch_gate(d_peak, nr, squelch, every, phase, 0.0, d_open, d_idx)
        want_open, want_n, want_held = h_squelch_gate(want_peak, squelch, every, phase, 0.0)
        assert eq(G.host(d_open), want_open) and n_open == want_n and S.exact_bits(held, want_held), (label, every, phase)
        assert eq(G.host(d_idx)[:n_open], np.flatnonzero(want_open).astype(np.int32))
        if every:
            assert 0 < n_open < nr
    d_h, d_l, d_r = sentinel((nr, W), torch.int8), sentinel((nr, W), torch.int8), sentinel((nr, 2), torch.float64)
    e.spectrum_bars(d_rows, nr, ln, H, W, d_h, d_l, d_r, f64=True)
    e.sync()
    gl, co = formats.bars_cells(G.host(d_h), G.host(d_l), H)
    res = [O.spectrogram_cells(r, H, W) for r in rows]
    R.frames("bars: glyphs", gl, [r[0] for r in res], eq)
    R.frames("bars: colours", co, [r[1] for r in res], eq)
    R.frames("bars: range", G.host(d_r), [np.array([r[2], r[3]]) for r in res], eq)
    lo, hi = sentinel((nr,), torch.float64), sentinel((nr,), torch.float64)
    e.row_extremes(d_rows, nr, ln, lo, hi, f64=True)
    ga, gb = sentinel((nr, W), torch.int8), sentinel((nr, W), torch.int8)
    e.gradient_rows(d_rows, nr, ln, lo, hi, W, ga, gb, window=30, f64=True)
    e.sync()
    ga, gb = G.host(ga), G.host(gb)
    og = [O.gradient_cells(rows[max(0, i - 29):i + 1], 1, W) for i in range(nr)]
    R.frames("gradient: glyphs", ga, [g[0][0] for g in og], eq)
    R.frames("gradient: colours", gb, [g[1][0] for g in og], eq)
    R.check()


# ---- scanner slice, classify ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", SMALL)
def test_scanner_slice(label):
    """test_cfg4_scanner_every_slice's criteria: every value within one component ulp of scan_slice, the share of differing values within
    the per-family rate, peak / count / bandwidth equal to the oracle's on bit-equal rows and to the device's own row's elsewhere."""
    e, b = G.engine(), batch(label)
    want = oracle("scan", b, lambda x: O.scan_slice(x, FS))
    db, pk = sentinel((b.nf, b.n), torch.float32), sentinel((b.nf,), torch.float32)
    bw, cnt = sentinel((b.nf,), torch.float64), sentinel((b.nf,), torch.int32)
    e.scan(b.dev(), b.nf, b.n, FS, db, pk, bw, cnt)
    e.sync()
    g, gp, gb, gc = G.host(db), G.host(pk), G.host(bw), G.host(cnt)
    R = Report("scanner", b)
    diff = 0
    for k in range(b.nf):
        w = want[k][0]
        with np.errstate(invalid="ignore"):
            far = np.abs(g[k].astype(np.float64) - w) > SB.scan_ulp_bound(w)
        if far.any() or np.isnan(g[k]).any():
            R.add("dB value beyond one component ulp of scan_slice", [k])
        same = A.same_bits(g[k], w)
        diff += int((g[k].view(np.uint32) != w.view(np.uint32)).sum())
        if same:
            ok = gp[k].tobytes() == np.float32(want[k][1]).tobytes() and int(gc[k]) == want[k][3] and float(gb[k]) == want[k][2]
        else:
            p = g[k].max()
            c = int(np.sum(g[k] > p - np.float32(20)))
            ok = gp[k].tobytes() == p.tobytes() and int(gc[k]) == c and float(gb[k]) == c * (FS / b.n)
        if not ok:
            R.add("peak / count / bandwidth", [k])
    R.check()
    print(f"scanner {label}: {diff} of {g.size} dB values differ from the oracle")
    assert diff <= max(SCAN_DIFF_RATE * g.size, 3), (diff, g.size)


@pytest.mark.parametrize("label", SMALL)
def test_classify(label):
    """test_classify_batch_vs_oracle's criteria; a NaN feature (an all-zero read) must be NaN on both sides."""
    e, b = G.engine(), batch(label)
    want = oracle("classify", b, lambda x: O.classify(x, FS))
    d_lab, d_bw = sentinel((b.nf,), torch.int32), sentinel((b.nf,), torch.float64)
    d_mi, d_fl, d_psd = sentinel((b.nf,), torch.float32), sentinel((b.nf,), torch.float32), sentinel((b.nf, 1024), torch.float32)
    e.classify(b.dev(), b.nf, b.n, FS, d_lab, d_bw, d_mi, d_fl, d_psd)
    e.sync()
    lab, bw, mi, fl, psd = (G.host(a) for a in (d_lab, d_bw, d_mi, d_fl, d_psd))
    R = Report("classify", b)
    g = gold()
    for k, c in enumerate(b.cases):
        olab, obw, omi, ofl, opsd = want[k]
        if not (O.CLASS_LABELS[lab[k]] == olab and bw[k] == obw):
            R.add("label / bandwidth", [k])
        if not A.same_bits(np.array(mi[k]), np.array(omi)):
            R.add("modulation index bits", [k])
        flat_ok = (float(fl[k]) == float(ofl) or abs(float(fl[k]) - float(ofl)) <= 1e-5 * abs(float(ofl)) or (np.isnan(fl[k]) and np.isnan(ofl)))
        if not flat_ok:
            R.add("spectral flatness beyond 1e-5", [k])
        m = len(opsd)
        if not np.all(np.abs(psd[k][:m] - opsd) <= 1e-6 * (opsd + 1e-10)):
            R.add("Welch PSD beyond 1e-6", [k])
        if c.golden:
            if not (O.CLASS_LABELS[lab[k]] == str(g[f"cls_label_{c.name}"]) and bw[k] == float(g[f"cls_bw_{c.name}"])
                    and A.same_bits(np.array(mi[k]), g[f"cls_mi_{c.name}"])):
                R.add("label / bandwidth / modulation index (adc.npz)", [k])
    R.check()


# ---- isolation, on the device itself ----------------------------------------------------------------------------------------------------
def test_a_dead_neighbour_changes_nothing():
    """A live frame alone, between two all-zero frames and between a stuck-rails and a one-sample frame: the same bytes from every
    demodulator, the correction, the power and the spectrum (the device against itself; the oracle comparisons above say the same)."""
    e = G.engine()
    live = A.by_name("i8_floor_mpx_1024_sprinkle")
    trios = [[live], [A.by_name("dead_zero_1024"), live, A.by_name("dead_zero_1024")],
             [A.by_name("dead_rails_1024"), live, A.by_name("dead_one_live_1024")], [A.by_name("i8_clip_mpx_1024"), live, A.by_name("dead_i_only_1024")]]
    outs = []
    for t in trios:
        b = Batch("trio", t)
        k = t.index(live)
        d_iq = b.dev()
        o = {}
        for mode in (L.MODE_NFM, L.MODE_AM, L.MODE_USB, L.MODE_WFM):
            for sb in (1, 0):
                with options(small_batch=(sb, 1)):
                    pcm, au = _demod(e, mode, d_iq, b, signal=True)
                o[f"pcm{mode}/{sb}"], o[f"au{mode}/{sb}"] = pcm[k], au[k]
        corr, pw, db = sentinel((b.nf, b.n, 2), torch.float32), sentinel((b.nf,), torch.float32), sentinel((b.nf, b.n), torch.float32)
        e.iq_correction(d_iq, b.nf, b.n, corr, None)
        e.power_db(d_iq, b.nf, b.n, pw)
        e.spectrum_db(d_iq, b.nf, b.n, db)
        e.sync()
        o["corr"], o["power"], o["db"] = G.host(corr)[k], G.host(pw)[k], G.host(db)[k]
        outs.append(o)
    for i, o in enumerate(outs[1:]):
        for key in o:
            assert outs[0][key].tobytes() == o[key].tobytes(), (i + 1, key)

"""Frame lengths swept through the demodulators, the classifier and the NumPy-sum kernels: one launch set per length, every frame against
the CPU oracle (oracle/pss_oracle.c), over the lists of tests/length_cases.py.

What depends on the length and is walked here: the summation plans (pss_npsum.h's build_forest behind get_plan / get_red_plan and k_pairwise<0/1>,
k_pairwise2, the three k_iqcorr variants, k_cls_modidx and the float64 twins k_power_c128 / k_am_env_c128), the chunk phases of the
forward kernels (k_nfm_fwd, k_wfm_fwd, k_wfm_mrg, k_iir4_sys, k_nfm_front, k_ssb_fir, k_am_grp), n_out = ceil((n - 1) / q), and the
classifier's segment count and unwrap chunks.

Criteria are those of the per-path tests, unchanged: everything bit for bit (NaN matching NaN) except
  - SSB float64 audio where the reference's hilbert() round trip runs in the oracle (a power-of-two length: the device runs its register
    transform from 256 samples on and skips the round trip below, the oracle replays pocketfft): 2e-14, as test_ssb_vs_golden; at the
    other lengths neither side runs it and the audio is equal bit for bit.  Option "ssb_hilbert" = 0 is bit for bit against
    demod_ssb(hilbert=False) at every length, option "hilbert_exact" against demod_ssb at the power-of-two lengths from 256 up; the
    int16 PCM equals the full oracle's at every length;
  - the classifier's PSD (1e-6) and flatness (1e-5), the bounds of test_classify_batch_vs_oracle; label, bandwidth and modulation
    index are exact.
No frame of a batch repeats another (asserted on the host).  Every launch of a test is queued before one synchronisation, the inputs and
outputs of all lengths in one device buffer each (blocks aligned to 256 bytes).  A failing case is reported as (entry point, path, fs, n,
criterion, frame indices): all of them as MISMATCH lines, then one assertion; the SWEEP lines count the (length, frame) cases per entry
point and path (profiles/length_sweep.txt keeps them).

The reference raises at none of the AM / SSB lengths (tools/fuzz_oracle_vs_reference.py --lengths ran it over all of them), so the
engine may raise at none either; NFM raises ValueError at n = 28 on every path as the reference's sosfiltfilt does.

Each test takes its own Engine: a sweep leaves a summation plan (one small device allocation) per length in its context, which the
session's shared engine should not carry into the later tests.

Measured on one MI355X, the host oracle included (the first test of a group pays for the frames and the reference its paths share): the
whole file 17 s for 34 tests, none above 1.4 s — test_wfm_lengths 1.35 / 0.76 s on the small-batch path (2.4 MS/s / 250 kS/s) and 0.2 s on
the two others, test_power_db_lengths 1.0 + 0.7 s, test_iq_correction_lengths 1.1 + 0.7 s and 0.5 + 0.15 s with RAW, test_am_mean_lengths
1.1 + 1.0 s and 0.5 + 0.4 s through pss_demod_power, test_nfm_lengths 0.9 / 0.3 s and 0.1 s, test_ssb_lengths 0.84 / 0.34 s and 0.15 s for
LSB, test_am_lengths 0.7 s, test_wfm_factor_one_lengths 0.7 s and 0.02 s, test_c128_lengths 0.6 s, test_classify_lengths 0.35 s,
test_nfm_right_extension_across_two_work_items 0.3 s.

The channel rates (tests/channel_rate_cases.py): the same sweeps at the rates the channelisers hand to the demodulators — NFM at 37 500
(q = 1), 44 100, 48 000, 50 000 (q = 2), 75 000 (q = 3) and 110 250 S/s (q = 5), WFM at 108 000 (q = 4), 110 250, 120 000 (q = 5) and
240 000 S/s (q = 10), SSB at 22 050 and 50 000 S/s — under the same criteria, then the product's own frame lengths (4096, 32 768 and
32 770 samples, every one of the n_out outputs) and the rates at which the reference raises.  tests/test_channel_rates_golden.py pins the
oracle to the reference at these rates.  Measured the same way: the 47 new cases about 12 s together, none above 0.75 s — test_wfm_lengths
0.6 .. 0.75 s per rate on the small-batch path and 0.18 .. 0.25 s on the two others, test_nfm_lengths 0.3 .. 0.4 s and 0.1 s,
test_ssb_lengths 0.54 / 0.35 s and 0.15 s for LSB, test_nfm_product_lengths and test_wfm_product_lengths below 0.1 s each,
test_refused_rates_leave_the_outputs_untouched 0.1 s.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import channel_rate_cases as CR
import length_cases as LC
import oracle_lib as O
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

SSB_ATOL = 2e-14           # test_ssb_vs_golden: the register Hilbert transform against pocketfft's round trip
PSD_REL, FLAT_REL = 1e-6, 1e-5    # test_classify_batch_vs_oracle
ALIGN = 256                # bytes: every length's block starts as a fresh allocation would
FULL_TILE = set(range(129, 153)) | set(range(1020, 1030)) | set(range(2044, 2054))   # 65 frames: one full 64-frame tile plus one
IS_G1 = 17                 # the small-batch array's group of 16 frames plus one
AM_G1 = 13                 # one k_am_grp group of 12 frames plus one
DEFAULTS = {"small_batch": 1, "nfm_fused": 1, "wfm_fused": 1, "wfm_corr_copy": 0, "ssb_hilbert": 1, "hilbert_exact": 0}
NFM_PATHS = {"small_batch": {}, "fused": {"small_batch": 0}, "three_kernel": {"small_batch": 0, "nfm_fused": 0}}
WFM_PATHS = {"small_batch": {}, "fused": {"small_batch": 0}, "plain": {"small_batch": 0, "wfm_fused": 0}}
# the rates of the existing sweeps, then those the channelisers feed the demodulators (tests/channel_rate_cases.py; q = 1 .. 10)
NFM_FS = [2.4e6, 250e3] + [fs for fs, _, _ in CR.NFM_RATES]
WFM_FS = [2.4e6, 250e3] + [fs for fs, _, _ in CR.WFM_RATES]
SSB_FS = [2.4e6, 48e3] + [fs for fs, _, _ in CR.SSB_RATES]
FS_IDS = {2.4e6: "2.4M_q108", 250e3: "250k_q11"}
REDUCE_PARTS = {"1..2199": [n for n in LC.REDUCE_LENGTHS if n < 2200], "chunk_and_group_edges": [n for n in LC.REDUCE_LENGTHS if n >= 2200]}


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def _engine():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return Engine(0)


class Flat:
    """One device buffer with a block per length (block i: sizes[i] elements)."""

    def __init__(self, sizes, dtype, host=None):
        step = ALIGN // torch.empty((), dtype=dtype).element_size()
        self.sizes = [int(s) for s in sizes]
        self.off = [0]
        for s in self.sizes:
            self.off.append(self.off[-1] + -(-max(s, 1) // step) * step)
        if host is None:
            self.t = torch.zeros(self.off[-1], dtype=dtype, device="cuda")
        else:
            flat = np.zeros(self.off[-1], host[0].dtype)
            for o, a in zip(self.off, host):
                flat[o:o + a.size] = a.reshape(-1)
            self.t = torch.from_numpy(flat).cuda()

    def at(self, i):
        return self.t[self.off[i]:]

    def host(self):
        a = self.t.cpu().numpy()
        return [a[o:o + s] for o, s in zip(self.off, self.sizes)]


def _f32(x):
    """complex64 / complex128 frames as interleaved reals."""
    x = np.ascontiguousarray(x)
    return x.view(np.float64 if x.dtype == np.complex128 else np.float32).reshape(-1)


class Sweep:
    """Failures and (length, frame) counts of one test, per (entry point, path, fs)."""

    def __init__(self):
        self.fails, self.counts = [], {}

    def cases(self, key, n, nf):
        c = self.counts.setdefault(key, [0, set()])
        c[0] += nf

    def bad(self, key, n, what, frames):
        frames = [int(f) for f in np.asarray(frames).reshape(-1)]
        if frames:
            self.fails.append(key + (n, what, frames[:8] + (["..."] if len(frames) > 8 else [])))
            self.counts.setdefault(key, [0, set()])[1].update((n, f) for f in frames)

    def raised(self, key, n, nf, ex):
        self.fails.append(key + (n, f"raised {type(ex).__name__}: {ex}", list(range(min(nf, 8)))))
        self.counts.setdefault(key, [0, set()])[1].update((n, f) for f in range(nf))

    def report(self):
        for (entry, path, fs), (c, b) in self.counts.items():
            print(f"SWEEP {entry} | {path} | fs={fs} | cases={c} differing={len(b)}")
        for f in self.fails:
            print("MISMATCH", f)
        assert not self.fails, self.fails[:10]


def _rows(a, k):
    return np.ascontiguousarray(a).reshape(k, -1)


def bits_bad(got, want):
    """Frames (first axis) whose values differ in any bit; NaN matches NaN whatever its payload."""
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want)
    if g.dtype.kind == "c":
        g, w = g.view(g.real.dtype), w.view(w.real.dtype)
    if g.shape != w.shape or g.dtype != w.dtype:
        return np.arange(len(g))
    u = np.uint64 if g.dtype.itemsize == 8 else np.uint32
    same = (g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))
    return np.nonzero(~_rows(same, len(g)).all(axis=1))[0]


def close_bad(got, want, atol):
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    gn, wn = np.isnan(g), np.isnan(w)
    with np.errstate(invalid="ignore"):
        ok = np.where(gn | wn, gn & wn, np.abs(g - w) <= atol)
    return np.nonzero(~_rows(ok, len(g)).all(axis=1))[0]


def eq_bad(got, want):
    g, w = np.asarray(got), np.asarray(want)
    if g.shape != w.shape:
        return np.arange(len(g))
    return np.nonzero(_rows(g != w, len(g)).any(axis=1))[0]


def int16_of(a):
    """np.int16(a * 32767) as the reference evaluates it on x86: truncation toward zero, NaN -> 0."""
    v = np.asarray(a, np.float64) * 32767.0
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), 0.0, np.trunc(v)).astype(np.int32).astype(np.int16)


def _pcm_mono(a):
    return np.stack([O.pcm16_stereo(r) for r in a])


def _options(e, opts):
    for k, v in opts.items():
        e.set_option(k, v)


def _restore(e, opts):
    for k in opts:
        e.set_option(k, DEFAULTS[k])


_REF = {}


def _shared(key, make):
    """A reference computed once per session and left unchanged (the paths of one entry point compare against the same arrays)."""
    if key not in _REF:
        with np.errstate(all="ignore"):
            _REF[key] = make()
    return _REF[key]


def _batches(kind, lengths, nf_of, maker):
    """[(n, frames)] with no frame repeating another in its batch — shared between the tests that sweep the same frames."""
    def make():
        out = []
        for n in lengths:
            x = maker(nf_of(n), n)
            assert LC.repeats(x) == 0, (kind, n)
            out.append((n, x))
        return out
    return _shared(("frames", kind), make)


def _refs(key, batches, fn):
    """fn over every frame of every batch (oracle_lib's thread pool) -> one list of per-frame results per batch."""
    def make():
        flat = O.map_frames(fn, [r for _, x in batches for r in x])
        out, p = [], 0
        for _, x in batches:
            out.append(flat[p:p + len(x)])
            p += len(x)
        return out
    return _shared(("ref",) + key, make)


def _am_sos(e):
    sos = np.empty((5, 6))
    e.lib.pss_am_bandpass_sos(sos.ctypes.data)
    return sos


def _wfm_filt(e, fs):
    lp, pil, lmr, alpha = e.wfm_filters(fs)
    _, sos, zi = e.nfm_filters(fs)
    return dict(lp_sos=lp, pilot_sos=pil, lmr_sos=lmr, alpha=alpha, dec_sos=sos, dec_zi=zi)


def _launch_demod(e, S, key, mode, fs, batches, nf_of, stereo=False, call="demod", with_power=False):
    """One demodulator call per length on the first nf_of(n) frames of its batch, all queued before one synchronisation.
    -> per length (audio [nf][n_out](,2), pcm [nf][n_out][2], power [nf] or None), or None where the call raised (recorded in S)."""
    ch = 2 if stereo else 1
    nfs = [nf_of(n) for n, _ in batches]
    n_out = [e.demod_out_len(mode, n, fs) for n, _ in batches]
    assert all(m >= 0 for m in n_out)
    d_in = Flat([k * n * 2 for k, (n, _) in zip(nfs, batches)], torch.float32, [_f32(x[:k]) for k, (_, x) in zip(nfs, batches)])
    d_au = Flat([k * m * ch for k, m in zip(nfs, n_out)], torch.float64)
    d_pcm = Flat([k * m * 2 for k, m in zip(nfs, n_out)], torch.int16)
    d_pw = Flat(nfs, torch.float32) if with_power else None
    failed = set()
    for i, (n, _) in enumerate(batches):
        try:
            if with_power:
                e.demod_power(mode, d_in.at(i), nfs[i], n, fs, d_pcm.at(i), d_au.at(i), d_pw.at(i))
            else:
                getattr(e, call)(mode, d_in.at(i), nfs[i], n, fs, d_pcm.at(i), d_au.at(i))
        except (ValueError, RuntimeError) as ex:
            S.raised(key, n, nfs[i], ex)
            failed.add(i)
    e.sync()
    au, pcm, pw = d_au.host(), d_pcm.host(), d_pw.host() if with_power else None
    out = []
    for i, (k, m) in enumerate(zip(nfs, n_out)):
        if i in failed:
            out.append(None)
        else:
            out.append((au[i].reshape((k, m, 2) if stereo else (k, m)), pcm[i].reshape(k, m, 2), pw[i] if with_power else None))
    return out


# ---- NumPy's summation tree: power_db, iq_correction, the AM mean -------------------------------------------------------------------------
def _reduce_batches(kind, part, maker):
    return _batches((kind, part), REDUCE_PARTS[part], lambda n: 3, maker)


@pytest.mark.parametrize("part", list(REDUCE_PARTS))
def test_power_db_lengths(part):
    """measure_signal_power (k_pairwise<0>): float32 bits of every frame."""
    batches = _reduce_batches("power", part, LC.power_frames)
    want = _refs(("power_db", part), batches, O.power_db)
    S, key = Sweep(), ("power_db", "k_pairwise<0>", None)
    e = _engine()
    try:
        d_in = Flat([x.size * 2 for _, x in batches], torch.float32, [_f32(x) for _, x in batches])
        d_p = Flat([len(x) for _, x in batches], torch.float32)
        for i, (n, x) in enumerate(batches):
            e.power_db(d_in.at(i), len(x), n, d_p.at(i))
        e.sync()
        got = d_p.host()
    finally:
        e.close()
    for i, (n, x) in enumerate(batches):
        S.cases(key, n, len(x))
        S.bad(key, n, "power bits", bits_bad(got[i], np.array(want[i], np.float32)))
    S.report()


@pytest.mark.parametrize("raw", [0, 1], ids=["corrected", "corrected_and_raw"])
@pytest.mark.parametrize("part", list(REDUCE_PARTS))
def test_iq_correction_lengths(part, raw):
    """iq_correction (the three k_iqcorr variants: n = 1024, other n <= 8192, n > 8192), with and without the RAW output
    (demodulate_signal's RAW mode: the real part of the corrected samples)."""
    batches = _reduce_batches("iq", part, LC.iq_frames)
    want = _refs(("iq_correction", part), batches, O.iq_correction)
    S, key = Sweep(), ("iq_correction", "RAW output" if raw else "no RAW output", None)
    e = _engine()
    try:
        d_in = Flat([x.size * 2 for _, x in batches], torch.float32, [_f32(x) for _, x in batches])
        d_out = Flat([x.size * 2 for _, x in batches], torch.float32)
        d_raw = Flat([x.size for _, x in batches], torch.float32) if raw else None
        for i, (n, x) in enumerate(batches):
            e.iq_correction(d_in.at(i), len(x), n, d_out.at(i), d_raw.at(i) if raw else None)
        e.sync()
        got, got_raw = d_out.host(), d_raw.host() if raw else None
    finally:
        e.close()
    for i, (n, x) in enumerate(batches):
        S.cases(key, n, len(x))
        S.bad(key, n, "corrected samples", bits_bad(got[i].reshape(len(x), n, 2), _f32(np.stack(want[i])).reshape(len(x), n, 2)))
        if raw:
            S.bad(key, n, "RAW", bits_bad(got_raw[i].reshape(len(x), n), np.ascontiguousarray(np.stack(want[i]).real)))
    S.report()


@pytest.mark.parametrize("entry", ["demod", "demod_power"])
@pytest.mark.parametrize("part", list(REDUCE_PARTS))
def test_am_mean_lengths(part, entry):
    """demodulate_am's np.mean of the envelope (k_pairwise<1>) and, through pss_demod_power, the two means of k_pairwise2: float64 audio
    bits, int16 PCM and the power bits of every frame."""
    fs = 2.4e6
    batches = _reduce_batches("power", part, LC.power_frames)
    e = _engine()
    try:
        sos = _am_sos(e)
        want = _refs(("demod_am", part), batches, lambda r: O.demod_am(r, sos))
        want_pw = _refs(("power_db", part), batches, O.power_db)
        S, key = Sweep(), (entry + "(AM)", "k_pairwise2" if entry == "demod_power" else "k_pairwise<1>", fs)
        got = _launch_demod(e, S, key, L.MODE_AM, fs, batches, lambda n: 3, with_power=entry == "demod_power")
    finally:
        e.close()
    for i, (n, x) in enumerate(batches):
        S.cases(key, n, len(x))
        if got[i] is None:
            continue
        a = np.stack(want[i])
        S.bad(key, n, "float64 audio bits", bits_bad(got[i][0], a))
        S.bad(key, n, "int16 PCM", eq_bad(got[i][1], _pcm_mono(a)))
        if entry == "demod_power":
            S.bad(key, n, "power bits", bits_bad(got[i][2], np.array(want_pw[i], np.float32)))
    S.report()


def test_c128_lengths():
    """The float64 twins (k_power_c128, k_am_env_c128) through the device batch entries: mean power bits, float64 audio bits, int16 PCM."""
    batches = _batches("c128", LC.C128_LENGTHS, lambda n: 3, LC.c128_frames)
    S, kp, ka = Sweep(), ("mean_power_c128", "k_power_c128", None), ("demod_am_c128", "k_am_env_c128", None)
    e = _engine()
    try:
        sos = _am_sos(e)
        d_in = Flat([x.size * 2 for _, x in batches], torch.float64, [_f32(x) for _, x in batches])
        d_pw = Flat([len(x) for _, x in batches], torch.float64)
        d_au = Flat([x.size for _, x in batches], torch.float64)
        d_pcm = Flat([x.size * 2 for _, x in batches], torch.int16)
        for i, (n, x) in enumerate(batches):
            e.mean_power_c128(d_in.at(i), len(x), n, d_pw.at(i))
            e.demod_am_c128(d_in.at(i), len(x), n, d_pcm.at(i), d_au.at(i))
        e.sync()
        pw, au, pcm = d_pw.host(), d_au.host(), d_pcm.host()
    finally:
        e.close()
    want_pw = _refs(("mean_power_c128",), batches, O.mean_power_c128)
    want_au = _refs(("demod_am_c128",), batches, lambda r: O.demod_am_c128(r, sos))
    for i, (n, x) in enumerate(batches):
        S.cases(kp, n, len(x))
        S.cases(ka, n, len(x))
        a = np.stack(want_au[i])
        S.bad(kp, n, "mean power bits", bits_bad(pw[i], np.array(want_pw[i], np.float64)))
        S.bad(ka, n, "float64 audio bits", bits_bad(au[i].reshape(len(x), n), a))
        S.bad(ka, n, "int16 PCM", eq_bad(pcm[i].reshape(len(x), n, 2), _pcm_mono(a)))
    S.report()


# ---- classifier ------------------------------------------------------------------------------------------------------------------------------
def test_classify_lengths():
    """classify_signal's five outputs for 3 frames per length (k_cls_welch_short below 1024, the segment count stepping at 1024 + 512 k,
    k_cls_modidx's plans for n and n - 1 and its 2048-sample unwrap chunks), and pss_classify_gated with the list [2, 0] on the same
    batch: its rows are those of frames 2 and 0."""
    fs = 2.4e6
    batches = _batches("classify", LC.CLASSIFY_LENGTHS, lambda n: 3, LC.fm_frames)
    want = _refs(("classify", fs), batches, lambda r: O.classify(r, fs))
    S = Sweep()
    names = (("label", torch.int32, 1), ("bw", torch.float64, 1), ("mi", torch.float32, 1), ("flat", torch.float32, 1), ("psd", torch.float32, 1024))
    e = _engine()
    try:
        d_in = Flat([x.size * 2 for _, x in batches], torch.float32, [_f32(x) for _, x in batches])
        d_idx = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
        full = {k: Flat([3 * w] * len(batches), dt) for k, dt, w in names}
        gated = {k: Flat([2 * w] * len(batches), dt) for k, dt, w in names}
        for i, (n, x) in enumerate(batches):
            e.classify(d_in.at(i), 3, n, fs, *[full[k].at(i) for k, _, _ in names])
            e.classify_gated(d_in.at(i), 3, n, fs, d_idx, 2, *[gated[k].at(i) for k, _, _ in names])
        e.sync()
        full = {k: v.host() for k, v in full.items()}
        gated = {k: v.host() for k, v in gated.items()}
    finally:
        e.close()
    for entry, got, frames in (("classify", full, (0, 1, 2)), ("classify_gated", gated, (2, 0))):
        key = (entry, "all five outputs", fs)
        for i, (n, x) in enumerate(batches):
            S.cases(key, n, len(frames))
            m = min(n, 1024)
            for row, f in enumerate(frames):
                olab, obw, omi, ofl, opsd = want[i][f]
                psd = got["psd"][i].reshape(-1, 1024)[row, :m]
                with np.errstate(all="ignore"):
                    if O.CLASS_LABELS[int(got["label"][i][row])] != olab:
                        S.bad(key, n, "label", [f])
                    if not (got["bw"][i][row] == obw or (np.isnan(got["bw"][i][row]) and np.isnan(obw))):
                        S.bad(key, n, "bandwidth", [f])
                    S.bad(key, n, "modulation index bits", np.array([f])[bits_bad(got["mi"][i][row:row + 1], np.array([omi], np.float32))])
                    fl = float(got["flat"][i][row])
                    if not (fl == float(ofl) or abs(fl - float(ofl)) <= FLAT_REL * abs(float(ofl)) or (np.isnan(fl) and np.isnan(float(ofl)))):
                        S.bad(key, n, "flatness beyond 1e-5", [f])
                    if not np.all((np.abs(psd - opsd) <= PSD_REL * (opsd + 1e-10)) | (np.isnan(psd) & np.isnan(opsd))):
                        S.bad(key, n, "PSD beyond 1e-6", [f])
    S.report()


# ---- NFM and WFM -------------------------------------------------------------------------------------------------------------------------
def _nf_of(small):
    return (lambda n: IS_G1) if small else (lambda n: 65 if n in FULL_TILE else 5)


def _demod_batches():
    """65 frames at the full-tile lengths, 17 elsewhere; every path takes the first frames of these (5, 17 or 65)."""
    return _batches("demod", LC.DEMOD_LENGTHS, lambda n: 65 if n in FULL_TILE else IS_G1, LC.fm_frames)


def _compare(S, key, batches, got, want, nf_of, pcm_of, audio_bad=bits_bad):
    for i, (n, x) in enumerate(batches):
        k = nf_of(n)
        S.cases(key, n, k)
        if got[i] is None:
            continue
        a = np.stack(want[i][:k])
        S.bad(key, n, "float64 audio", audio_bad(got[i][0], a))
        S.bad(key, n, "int16 PCM", eq_bad(got[i][1], pcm_of(a)))


def _fs_id(fs):
    return FS_IDS.get(fs) or CR.rate_id(fs)


@pytest.mark.parametrize("path", list(NFM_PATHS))
@pytest.mark.parametrize("fs", NFM_FS, ids=_fs_id)
def test_nfm_lengths(fs, path):
    """demodulate_nfm with the engine's own designed filters on the small-batch array, the fused forward kernel (from n - 1 >= 128; the
    three-kernel path below) and the three-kernel path: float64 audio bits and int16 PCM of every frame; n = 28 raises ValueError.
    At the channel rates q = 1 .. 5: at 37 500 S/s nothing is dropped (n_out = n - 1, cheby1(8, 0.05, 0.8) still runs)."""
    batches = _demod_batches()
    S, key, nf_of = Sweep(), ("demod(NFM)", path, fs), _nf_of(path == "small_batch")
    e = _engine()
    try:
        taps, sos, zi = e.nfm_filters(fs)
        want = _refs(("nfm", fs), batches, lambda r: O.demod_nfm(r, fs, taps, sos, zi))
        _options(e, NFM_PATHS[path])
        try:
            short = LC.fm_frames(5, 28)
            try:     # (outputs sized for 28 samples per frame: more than any n_out)
                e.demod(L.MODE_NFM, torch.from_numpy(_f32(short).copy()).cuda(), 5, 28, fs, torch.zeros((5, 28, 2), dtype=torch.int16, device="cuda"),
                        torch.zeros((5, 28), dtype=torch.float64, device="cuda"))
                S.bad(key, 28, "no ValueError (sosfiltfilt's padlen)", range(5))
            except ValueError:
                pass
            got = _launch_demod(e, S, key, L.MODE_NFM, fs, batches, nf_of)
        finally:
            _restore(e, NFM_PATHS[path])
    finally:
        e.close()
    _compare(S, key, batches, got, want, nf_of, _pcm_mono)
    S.report()


STRADDLE_LENGTHS = [1031, 1040, 1051, 1052, 1053, 2075, 2076, 2077, 3074, 3100, 3101]


@pytest.mark.parametrize("path", ["small_batch", "three_kernel"])
def test_nfm_right_extension_across_two_work_items(path):
    """What the sweep found at n = 1026..1029 and 2050..2053: k_nfm_front cuts a frame into work items of 1024 outputs, and where the last
    28 outputs (the operands of sosfiltfilt's right odd extension) straddle two of them — M = n - 1 with M mod 1024 in 1..27 — neither
    wrote the extension, so the decimator read stale scratch.  k_nfm_edge writes it there now.  The rest of that range, both of its
    ends (M mod 1024 = 27 and 28) and the third work item, at both rates."""
    S, nf_of = Sweep(), _nf_of(path == "small_batch")
    batches = _batches("straddle", STRADDLE_LENGTHS, lambda n: IS_G1, LC.fm_frames)
    e = _engine()
    try:
        _options(e, NFM_PATHS[path])
        try:
            for fs in (2.4e6, 250e3):
                key = ("demod(NFM)", path + ", straddling lengths", fs)
                taps, sos, zi = e.nfm_filters(fs)
                want = _refs(("nfm_straddle", fs), batches, lambda r: O.demod_nfm(r, fs, taps, sos, zi))
                _compare(S, key, batches, _launch_demod(e, S, key, L.MODE_NFM, fs, batches, nf_of), want, nf_of, _pcm_mono)
        finally:
            _restore(e, NFM_PATHS[path])
    finally:
        e.close()
    S.report()


@pytest.mark.parametrize("path", list(WFM_PATHS))
@pytest.mark.parametrize("fs", WFM_FS, ids=_fs_id)
def test_wfm_lengths(fs, path):
    """demodulate_wfm on the small-batch array (k_wfm_mrg), the fused forward kernel and the plain kernels; for n <= 160 also
    demodulate_signal (iq_correction first: the correction pre-pass, and option "wfm_corr_copy" = 1, the corrected copy)."""
    batches = _demod_batches()
    short = [b for b in batches if b[0] <= 160]
    S, nf_of = Sweep(), _nf_of(path == "small_batch")
    e = _engine()
    try:
        filt = _wfm_filt(e, fs)
        want = _refs(("wfm", fs), batches, lambda r: O.demod_wfm(r, fs, filt))
        want_sig = _refs(("wfm_signal", fs), short, lambda r: O.demod_wfm(O.iq_correction(r), fs, filt))
        _options(e, WFM_PATHS[path])
        try:
            key = ("demod(WFM)", path, fs)
            _compare(S, key, batches, _launch_demod(e, S, key, L.MODE_WFM, fs, batches, nf_of, stereo=True), want, nf_of, int16_of)
            for copy in (0, 1):
                key = ("demod_signal(WFM)", path + (", wfm_corr_copy" if copy else ", correction pre-pass"), fs)
                e.set_option("wfm_corr_copy", copy)
                try:
                    got = _launch_demod(e, S, key, L.MODE_WFM, fs, short, nf_of, stereo=True, call="demod_signal")
                finally:
                    e.set_option("wfm_corr_copy", 0)
                _compare(S, key, short, got, want_sig, nf_of, int16_of)
        finally:
            _restore(e, WFM_PATHS[path])
    finally:
        e.close()
    S.report()


@pytest.mark.parametrize("path", list(WFM_PATHS))
def test_wfm_factor_one_lengths(path):
    """n = 29..160 at a decimation factor of one (250 kS/s, target rate 130 000, as test_wfm_factor_one_past_the_cap): the reference skips
    decimate() and n_out = n - 1."""
    fs, tr = 250000.0, 130000
    batches = [b for b in _demod_batches() if b[0] <= 160]
    S, key, nf_of = Sweep(), ("demod(WFM), q = 1", path, fs), _nf_of(path == "small_batch")
    e = _engine()
    try:
        filt = _wfm_filt(e, fs)
        want = _refs(("wfm_q1", fs), batches, lambda r: O.demod_wfm(r, fs, filt, target_rate=tr))
        _options(e, WFM_PATHS[path])
        e.set_target_rate(float(tr))
        try:
            assert all(e.demod_out_len(L.MODE_WFM, n, fs) == n - 1 for n, _ in batches)
            got = _launch_demod(e, S, key, L.MODE_WFM, fs, batches, nf_of, stereo=True)
        finally:
            e.set_target_rate(22050)
            _restore(e, WFM_PATHS[path])
    finally:
        e.close()
    _compare(S, key, batches, got, want, nf_of, int16_of)
    S.report()


# ---- the product's own frame lengths at the channel rates ---------------------------------------------------------------------------------
PRODUCT_NF = {"small_batch": lambda n: 3, "fused": lambda n: 65 if n == 4096 else 5, "other": lambda n: 5}


def _product_batches():
    """The chain tests' 4096 (65 frames: a full 64-frame tile plus one), the default frame_len 32 768 and 32 770, one past the switch
    (n - 1) * 8 >= 262144 of both demodulators (5 frames each)."""
    assert CR.PRODUCT_LENGTHS == [4096, 32768, 32770] and (32768 - 1) * 8 < 262144 <= (32770 - 1) * 8
    return _batches("product", CR.PRODUCT_LENGTHS, PRODUCT_NF["fused"], LC.fm_frames)


def _product_nf(path):
    return PRODUCT_NF.get(path, PRODUCT_NF["other"])


@pytest.mark.parametrize("path", list(NFM_PATHS))
@pytest.mark.parametrize("fs", CR.PRODUCT_NFM_RATES, ids=CR.rate_id)
def test_nfm_product_lengths(fs, path):
    """demodulate_nfm at the frame lengths demodulate_channels / demodulate_bank / monitor_channels cut, at 37 500 S/s (q = 1: 32 769
    outputs per frame) and 48 000 S/s: all n_out outputs of every frame, float64 audio bits and int16 PCM."""
    batches = _product_batches()
    S, key, nf_of = Sweep(), ("demod(NFM)", path + ", product lengths", fs), _product_nf(path)
    e = _engine()
    try:
        taps, sos, zi = e.nfm_filters(fs)
        want = _refs(("nfm_product", fs), batches, lambda r: O.demod_nfm(r, fs, taps, sos, zi))
        assert [len(w[0]) for w in want] == [-(-(n - 1) // CR.factor(fs)) for n in CR.PRODUCT_LENGTHS]
        _options(e, NFM_PATHS[path])
        try:
            got = _launch_demod(e, S, key, L.MODE_NFM, fs, batches, nf_of)
        finally:
            _restore(e, NFM_PATHS[path])
    finally:
        e.close()
    _compare(S, key, batches, got, want, nf_of, _pcm_mono)
    S.report()


@pytest.mark.parametrize("path", list(WFM_PATHS))
@pytest.mark.parametrize("fs", CR.PRODUCT_WFM_RATES, ids=CR.rate_id)
def test_wfm_product_lengths(fs, path):
    """demodulate_wfm at the same frame lengths, at 110 250 S/s (plan_audio's WFM rate, q = 5) and 240 000 S/s (q = 10): all n_out
    outputs of every frame, both channels."""
    batches = _product_batches()
    S, key, nf_of = Sweep(), ("demod(WFM)", path + ", product lengths", fs), _product_nf(path)
    e = _engine()
    try:
        filt = _wfm_filt(e, fs)
        want = _refs(("wfm_product", fs), batches, lambda r: O.demod_wfm(r, fs, filt))
        assert [len(w[0]) for w in want] == [-(-(n - 1) // CR.factor(fs)) for n in CR.PRODUCT_LENGTHS]
        _options(e, WFM_PATHS[path])
        try:
            got = _launch_demod(e, S, key, L.MODE_WFM, fs, batches, nf_of, stereo=True)
        finally:
            _restore(e, WFM_PATHS[path])
    finally:
        e.close()
    _compare(S, key, batches, got, want, nf_of, int16_of)
    S.report()


CANARY16, CANARY64 = -12345, -7.25


def test_refused_rates_leave_the_outputs_untouched():
    """Where the reference's SciPy calls raise ValueError the engine raises it too, with the library's reason, on every path and through
    both entry points, and writes nothing: NFM at 30 000 and 22 050 S/s (firwin's 15 kHz at or above Nyquist), WFM at 106 000 S/s
    (butter's 53 kHz band edge at Nyquist).  Below 22 050 S/s the decimation factor is 0: demod_out_len is negative and the call is an
    argument error."""
    from pyspecsdr_amd.engine import PssError
    nf, n = 5, 256
    assert CR.NFM_REFUSED == [30000.0, 22050.0] and CR.WFM_REFUSED == [106000.0]
    cases = [(L.MODE_NFM, fs, NFM_PATHS, "firwin: invalid cutoff frequency") for fs in CR.NFM_REFUSED]
    cases += [(L.MODE_WFM, fs, WFM_PATHS, "butter: digital filter critical frequencies must be 0 < Wn < 1") for fs in CR.WFM_REFUSED]
    e = _engine()
    try:
        d_in = torch.from_numpy(_f32(LC.fm_frames(nf, n)).copy()).cuda()
        d_pcm = torch.full((nf, n, 2), CANARY16, dtype=torch.int16, device="cuda")
        d_au = torch.full((nf, n, 2), CANARY64, dtype=torch.float64, device="cuda")
        for mode, fs, paths, reason in cases:
            assert e.demod_out_len(mode, n, fs) == -(-(n - 1) // CR.factor(fs))          # the length exists; the design does not
            for path, opts in paths.items():
                _options(e, opts)
                try:
                    for call in ("demod", "demod_signal"):
                        with pytest.raises(ValueError) as err:
                            getattr(e, call)(mode, d_in, nf, n, fs, d_pcm, d_au)
                        assert reason in str(err.value), (mode, fs, path, call, str(err.value))
                finally:
                    _restore(e, opts)
        for mode in (L.MODE_NFM, L.MODE_WFM):
            for fs in (22049.0, 20000.0, 11025.0):
                assert e.demod_out_len(mode, n, fs) < 0, (mode, fs)
                with pytest.raises(PssError) as err:
                    e.demod(mode, d_in, nf, n, fs, d_pcm, d_au)
                assert err.value.code == L.PSS_E_ARG, (mode, fs)
        e.sync()
        assert bool(torch.all(d_pcm == CANARY16)) and bool(torch.all(d_au == CANARY64))
    finally:
        e.close()


# ---- AM and SSB --------------------------------------------------------------------------------------------------------------------------
def _am_ssb_batches(kind, maker):
    return _batches(kind, LC.AM_SSB_LENGTHS, lambda n: AM_G1, maker)


def test_am_lengths():
    """demodulate_am from one sample up, 13 frames (one k_am_grp group of 12 plus one): float64 audio bits and int16 PCM."""
    fs = 2.4e6
    batches = _am_ssb_batches("am", LC.iq_frames)
    S, key = Sweep(), ("demod(AM)", "k_am_grp", fs)
    e = _engine()
    try:
        sos = _am_sos(e)
        want = _refs(("am",), batches, lambda r: O.demod_am(r, sos))
        got = _launch_demod(e, S, key, L.MODE_AM, fs, batches, lambda n: AM_G1)
    finally:
        e.close()
    _compare(S, key, batches, got, want, lambda n: AM_G1, _pcm_mono)
    S.report()


def _pow2(n):
    return n >= 2 and not n & (n - 1)


@pytest.mark.parametrize("mode", [L.MODE_USB, L.MODE_LSB], ids=["usb", "lsb"])
@pytest.mark.parametrize("fs", SSB_FS, ids=["2.4M", "48k", "22050", "50k"])
def test_ssb_lengths(fs, mode):
    """demodulate_ssb from one sample up, 13 frames: the default path (int16 equal to the full oracle at every length; float64 within
    2e-14 where the oracle runs the hilbert() round trip, equal bit for bit elsewhere), option "ssb_hilbert" = 0 (bit for bit against the
    oracle without the round trip) and, at the power-of-two lengths from 256 up, option "hilbert_exact" (bit for bit against the oracle)."""
    name = "USB" if mode == L.MODE_USB else "LSB"
    batches = _am_ssb_batches("ssb", LC.fm_frames)
    exact = [b for b in batches if _pow2(b[0]) and b[0] >= 256]
    assert [n for n, _ in exact] == [256, 1024, 2048]
    S, nf_of = Sweep(), (lambda n: AM_G1)
    e = _engine()
    try:
        taps = e.ssb_taps(fs)
        want = _refs(("ssb", fs), batches, lambda r: O.demod_ssb(r, taps))
        want_nh = _refs(("ssb_no_hilbert", fs), batches, lambda r: O.demod_ssb(r, taps, hilbert=False))
        want_x = [want[i] for i, (n, _) in enumerate(batches) if _pow2(n) and n >= 256]
        key = (f"demod({name})", "default", fs)
        got = _launch_demod(e, S, key, mode, fs, batches, nf_of)
        for i, (n, x) in enumerate(batches):
            S.cases(key, n, len(x))
            if got[i] is None:
                continue
            a = np.stack(want[i])
            if _pow2(n):
                S.bad(key, n, "float64 audio beyond 2e-14", close_bad(got[i][0], a, SSB_ATOL))
            else:
                S.bad(key, n, "float64 audio bits", bits_bad(got[i][0], a))
            S.bad(key, n, "int16 PCM", eq_bad(got[i][1], _pcm_mono(a)))
        for path, opts, sub, ref in (("ssb_hilbert = 0", {"ssb_hilbert": 0}, batches, want_nh), ("hilbert_exact", {"hilbert_exact": 1}, exact, want_x)):
            key = (f"demod({name})", path, fs)
            _options(e, opts)
            try:
                got = _launch_demod(e, S, key, mode, fs, sub, nf_of)
            finally:
                _restore(e, opts)
            _compare(S, key, sub, got, ref, nf_of, _pcm_mono)
    finally:
        e.close()
    S.report()

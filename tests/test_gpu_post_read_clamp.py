"""k_spectrum_post clamps the smoothed row where the display reads it (pss_post.h: post_row_staged<..., READ_CLAMP>, ClampedStagedRow) instead of
forming the clamped row: the step's outputs against the oracle's own step from the IQ (as tools/bench_configs.check_from_iq compares them) and,
bit for bit, against the two-kernel form (option fuse_post = 0: k_spectrum_r16<D64> -> k_post_sel<double>, which still clamps and stores every
element).  No entry point returns the resampled values themselves: they are compared through the cells they become and through the two-kernel
form's cells.

Batches of 5, 37 and 260 frames of 1024 points (a partial group of four; a range boundary of the one-round grid; more than the 30-row window),
display widths 1, 2, 111, 112, 120 (interp_at's W == 1 branch, its last-column branch, odd and even widths).  The frames of a batch cycle through
the IQ families below — among them a stepped floor whose band edges, elements 0, 1 and 1019 of the row included, lie far below median - 10, so
that every width's reads, the W == 1 read and the last column's are clamped values, and the cells provably change when the clamp is left out
(asserted on the CPU from the oracle's rows); the last frame carries one infinite sample (its row is compared with the two-kernel form only: what an infinity becomes
in a transform is the transform's own business, tests/test_gpu_parity.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bracket_ladder as B  # noqa: E402  (the families of the bracket statistics: the same signals)

pytestmark = pytest.mark.gpu

N, M, FS, WINDOW = 1024, 1020, 2.4e6, 30
CYCLE = ("fm", "step", "nan", "noise", "comb", "zero", "int8")
STEP_DB = 60.0                 # the stepped floor's drop
FRAMES = (5, 37, 260)
WIDTHS = (1, 2, 111, 112, 120)
_BATCH = {}


def clean_comb(nf):
    """A strong tone on EVERY bin centre and no noise, the tones' phases such that the frame is three impulses in time (1, 0.3 and 0.2 at
    neighbouring samples): |X| ripples slowly between 0.5 and 1.5 times the window's value there, 9.5 dB from trough to crest — the smoothed
    minimum stays above median - 10 on every row."""
    x = np.zeros((nf, N), np.complex128)
    for f in range(nf):
        p = 300 + (7 * f) % 400
        x[f, p], x[f, p + 1], x[f, p + 3] = 1.0, 0.3 * np.exp(0.3j * f), 0.2 * np.exp(-0.7j * f)
    return x.astype(np.complex64)


def stepped_floor(nf):
    """Strong noise over the middle 60 % of the band and STEP_DB less over the rest, the band edges included: the median lies on the strong part
    and some 400 smoothed values, the row's first and last elements among them, lie tens of dB below median - 10 (the window's leakage from the
    strong part fills the weak one to about 45 dB below it)."""
    rng = np.random.default_rng(24)
    spec = rng.standard_normal((nf, N)) + 1j * rng.standard_normal((nf, N))       # in display order (after fftshift)
    weak = np.abs(np.arange(N) - N // 2) > 0.3 * N
    spec[:, weak] *= 10.0 ** (-STEP_DB / 20.0)
    return (np.fft.ifft(np.fft.ifftshift(spec, axes=1), axis=1) * 4.0).astype(np.complex64)


def batch(nf):
    """(iq [nf][1024] complex64, family name per frame), built once per batch size."""
    if nf not in _BATCH:
        fam = [CYCLE[i % len(CYCLE)] for i in range(nf)]
        fam[-1] = "inf"
        src = {"fm": B.synth("fm", nf, 21), "noise": B.synth("noise", nf, 22), "comb": clean_comb(nf), "zero": B.synth("zero", nf, 0),
               "int8": B.synth("int8", nf, 23), "step": stepped_floor(nf)}
        src["nan"] = src["fm"].copy()
        src["inf"] = src["fm"].copy()
        iq = np.stack([src[fam[i]][i] for i in range(nf)])
        for i in range(nf):
            if fam[i] == "nan":
                iq[i, (37 * i) % N] = complex(np.nan, 0.25)
        iq[nf - 1, 700] = complex(0.1, np.inf)
        _BATCH[nf] = (np.ascontiguousarray(iq, np.complex64), fam)
    return _BATCH[nf]


def read_elements(disp_w):
    """The elements of a 1020-point row interp_at reads for a display of disp_w columns (np.linspace(0, 1019, disp_w): knots j and j + 1, the
    last column the last element)."""
    stop, out = float(M - 1), set()
    for x in range(disp_w):
        xp = 0.0 if disp_w == 1 else (stop if x == disp_w - 1 else x * (stop / (disp_w - 1)))
        if xp >= stop:
            out.add(M - 1)
        else:
            out.update((int(xp), int(xp) + 1))
    return np.array(sorted(out))


def clamp_changes(db, post, disp_w):
    """Per oracle row: how many of the elements the display reads the clamp changed (-1: the row holds a NaN)."""
    idx = read_elements(disp_w)
    sm = np.zeros((db.shape[0], M))
    for k in range(5):
        sm = sm + db[:, k:k + M] * 0.2
    changed = np.count_nonzero(post[:, idx] != sm[:, idx], axis=1)
    return np.where(np.isnan(sm).any(axis=1), -1, changed)


def smoothed(db):
    sm = np.zeros((db.shape[0], M))
    for k in range(5):
        sm = sm + db[:, k:k + M] * 0.2
    return sm


def oracle_cells(rows, o, disp_w):
    """The oracle's waterfall lines of `rows` (any rows in place of the post-processed ones) with the step's own extremes."""
    import oracle_lib as O
    nf = rows.shape[0]
    g, c = np.empty((nf, disp_w), np.int8), np.empty((nf, disp_w), np.int8)
    O.lib().pss_o_waterfall_rows_f64(np.ascontiguousarray(rows).reshape(-1), o["lo"], o["hi"], nf, M, WINDOW, disp_w, g.reshape(-1), c.reshape(-1), 1)
    return g, c


def oracle_step(nf, disp_w, pcm=False):
    import oracle_lib as O
    import gpu_util as G
    iq, fam = batch(nf)
    taps, sos, zi = G.engine().nfm_filters(FS)
    return O.headline_f64(iq, FS, taps, sos, zi, WINDOW, disp_w, O.threads_available(), pcm=pcm, keep_db=True)


def test_the_batches_hold_every_class_of_row():
    """From the ORACLE's rows: clamped elements among those the display reads (the benchmark's signal, noise, quantised IQ), none (the same families,
    the clean comb and the constant row, every row of theirs), rows with a NaN.  Each family supplies its class or the test fails."""
    o = oracle_step(260, 112)
    _, fam = batch(260)
    fam = np.array(fam)
    ch = clamp_changes(o["db"], o["post"], 112)
    for f in ("fm", "noise", "int8"):
        assert np.any(ch[fam == f] > 0), f"{f}: no row with a clamped element among those read"
        assert np.any(ch[fam == f] == 0), f"{f}: no row without one"
    for f in ("comb", "zero"):
        assert np.all(ch[fam == f] == 0), f"{f}: the clamp changes {ch[fam == f].max()} read elements of a row"
    assert np.all(ch[fam == "nan"] == -1) and np.count_nonzero(fam == "nan") >= 30
    # the widths' classes: the first knot pair (W = 1), the same and the last element (W = 2), more than 200 elements at the display's widths
    assert [len(read_elements(w)) for w in WIDTHS[:2]] == [2, 3] and all(200 < len(read_elements(w)) <= 2 * w for w in WIDTHS[2:])
    for nf in FRAMES:
        ch = clamp_changes(*(lambda q: (q["db"], q["post"]))(oracle_step(nf, 120)), 120)
        assert np.any(ch == -1) and np.any(ch == 0), nf
        assert nf == 5 or np.any(ch > 0), nf


@pytest.mark.parametrize("disp_w", WIDTHS)
@pytest.mark.parametrize("nf", FRAMES)
def test_the_clamp_shows_in_the_cells_of_every_batch_and_width(nf, disp_w):
    """Per batch and per width, from the ORACLE's rows on the CPU: a finite row (the stepped floor) has clamped values among the elements the
    display reads — element 0 or 1 for the W == 1 read, element 1019 for the last column — and the oracle's cells of that row change when the clamp
    is left out of all of it, of its first two elements alone, and of its last element alone.  So a kernel that read an unclamped value at any of
    these places would fail the cell comparisons below."""
    o = oracle_step(nf, disp_w)
    _, fam = batch(nf)
    step = np.flatnonzero(np.array(fam) == "step")
    assert step.size >= 1
    sm = smoothed(o["db"])
    idx = read_elements(disp_w)
    clamped = o["post"] != sm                                     # (finite rows here)
    assert np.all(np.isfinite(sm[step]))
    assert np.all(clamped[step][:, idx].sum(axis=1) >= (1 if disp_w <= 2 else 50)), "clamped values among the elements read, on every such row"
    assert np.all(clamped[step, 0] | clamped[step, 1]) and np.all(clamped[step, M - 1])
    assert np.all(sm[step, 0] < o["post"][step, 0] - 20.0) and np.all(sm[step, M - 1] < o["post"][step, M - 1] - 20.0)
    want = oracle_cells(o["post"], o, disp_w)
    assert np.array_equal(want[0], o["glyph"]) and np.array_equal(want[1], o["colour"])       # the helper draws what the step drew
    def differs(rows):
        got = oracle_cells(rows, o, disp_w)
        return (got[0] != want[0]) | (got[1] != want[1])
    unclamped = o["post"].copy(); unclamped[step] = sm[step]
    d = differs(unclamped)
    assert np.all(d[step].any(axis=1)), "every stepped row's cells change without the clamp"
    assert not d[np.setdiff1d(np.arange(nf), step)].any()
    first = o["post"].copy(); first[step, 0:2] = sm[step, 0:2]
    assert np.all(differs(first)[step, 0]), "the first column sees the clamp of elements 0 and 1"
    if disp_w >= 2:
        last = o["post"].copy(); last[step, M - 1] = sm[step, M - 1]
        assert np.all(differs(last)[step, disp_w - 1]), "the last column sees the clamp of element 1019"


@pytest.mark.parametrize("disp_w", WIDTHS)
@pytest.mark.parametrize("nf", FRAMES)
def test_display_half_against_the_oracle_and_the_two_kernel_form(nf, disp_w):
    import torch
    import gpu_util as G
    e = G.engine()
    iq, fam = batch(nf)
    d_iq = G.dev(iq)
    outs = []
    try:
        for fuse in (1, 0):
            e.set_option("fuse_post", fuse)
            o = dict(db32=G.empty((nf, N), torch.float32), lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64),
                     a=torch.zeros((nf, disp_w), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, disp_w), dtype=torch.int8, device="cuda"))
            e.spectrum_cells(d_iq, nf, N, o["db32"], None, o["lo"], o["hi"], disp_w, o["a"], o["b"], window=WINDOW)
            e.sync()
            outs.append(o)
    finally:
        e.set_option("fuse_post", 1)
    for k in outs[0]:
        assert torch.equal(outs[0][k].view(torch.uint8), outs[1][k].view(torch.uint8)), (nf, disp_w, k, "fused against fuse_post = 0")
    _against_oracle(outs[0], oracle_step(nf, disp_w), fam)


@pytest.mark.parametrize("nf", FRAMES)
def test_the_step_with_the_demodulator_beside_it(nf):
    import torch
    import gpu_util as G
    from pyspecsdr_amd import _lib as L
    e = G.engine()
    iq, fam = batch(nf)
    d_iq = G.dev(iq)
    W = 112
    n_out = e.demod_out_len(L.MODE_NFM, N, FS)
    outs = []
    try:
        for fuse in (1, 0):
            e.set_option("fuse_post", fuse)
            o = dict(db32=G.empty((nf, N), torch.float32), lo=G.empty((nf,), torch.float64), hi=G.empty((nf,), torch.float64),
                     a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"),
                     pcm=G.empty((nf, n_out, 2), torch.int16))
            e.frame_pipeline_cells(L.MODE_NFM, d_iq, nf, N, FS, o["db32"], None, o["lo"], o["hi"], W, o["a"], o["b"], o["pcm"], window=WINDOW)
            e.sync()
            outs.append(o)
    finally:
        e.set_option("fuse_post", 1)
    for k in outs[0]:
        assert torch.equal(outs[0][k].view(torch.uint8), outs[1][k].view(torch.uint8)), (nf, k, "fused against fuse_post = 0")
    want = oracle_step(nf, W, pcm=True)
    _against_oracle(outs[0], want, fam)
    finite = np.array([f not in ("nan", "inf") for f in fam])
    assert np.array_equal(G.host(outs[0]["pcm"])[finite], want["pcm"][finite])


def _against_oracle(got, want, fam):
    """The dB rows to the spectrum's own tolerance (1e-4 relative for the float32 row, check_from_iq's); extremes to 1e-9, the float64 rows'
    own tolerance there; the neutral pair for a row without a finite value; every cell equal.  The last frame (an infinite sample) apart."""
    import gpu_util as G
    fam = np.array(fam)
    finite = (fam != "nan") & (fam != "inf")
    db, lo, hi = G.host(got["db32"]).astype(np.float64), G.host(got["lo"]), G.host(got["hi"])
    ref = want["db"]
    assert np.all(np.abs(db[finite] - ref[finite]) <= 1e-4 * np.maximum(np.abs(ref[finite]), 1.0))
    assert np.all(np.isnan(db[fam == "nan"]))
    assert np.max(np.abs(lo[finite] - want["lo"][finite])) <= 1e-9 and np.max(np.abs(hi[finite] - want["hi"][finite])) <= 1e-9
    assert np.all(lo[fam == "nan"] == np.inf) and np.all(hi[fam == "nan"] == -np.inf)
    keep = slice(0, len(fam) - 1)
    assert np.array_equal(G.host(got["a"])[keep], want["glyph"][keep]) and np.array_equal(G.host(got["b"])[keep], want["colour"][keep])

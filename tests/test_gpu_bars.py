"""The spectrum display as bars and the gradient view as a line per frame, on the GPU through the C ABI (include/pss.h, "spectrum bars",
pss_gradient_rows):

- pss_spectrum_bars_f64 -> pss_bars_cells / pss_h_bars_cells against the reference's own grids (tests/golden/display.npz, every `sg` case);
- the expanded bars against pss_spectrogram_cells[_f64], every cell, on seeded batches built to take every path of the new kernels
  (tests/bars_util.py) — zero differing cells is the requirement: the two kernels call the same device functions behind their selects;
- pss_frame_pipeline_bars from IQ: its rows and PCM byte-equal to the existing entry points', its bars equal to the oracle's cells computed
  from the same IQ;
- pss_gradient_rows[_f64] against the reference's `gw` grids and the oracle, and display = 2 through every batched step.
Failures name the family / geometry, the row and the cell."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bars_util as B
import display_cases as D
import gpu_util as G
import oracle_lib as O
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F

FS = 2.4e6
MODES = (L.MODE_NFM, L.MODE_AM, L.MODE_USB, L.MODE_LSB, L.MODE_WFM)


def _bars(e, rows, disp_h, disp_w, f64=True):
    """pss_spectrum_bars[_f64] of rows [k][len] -> (height, level, range) on the host, and the device bars."""
    k, ln = rows.shape
    d = G.dev(rows)
    d_h, d_l = G.empty((k, disp_w), torch.int8), G.empty((k, disp_w), torch.int8)
    d_r = G.empty((k, 2), torch.float64)
    e.spectrum_bars(d, k, ln, disp_h, disp_w, d_h, d_l, d_r, f64=f64)
    return d_h, d_l, d_r


def _expand_device(e, d_h, d_l, disp_h):
    k, disp_w = d_h.shape
    d_g, d_c = G.empty((k, disp_h, disp_w), torch.int8), G.empty((k, disp_h, disp_w), torch.int8)
    e.bars_cells(d_h, d_l, k, disp_h, disp_w, d_g, d_c)
    e.sync()
    return G.host(d_g), G.host(d_c)


def _first(got, want, names=None):
    bad = np.argwhere(got != want)
    r, y, x = bad[0]
    tag = f" ({names[r]})" if names else ""
    return f"{len(bad)} cells differ, first row {r}{tag} y={y} x={x}: got {got[r, y, x]} want {want[r, y, x]}"


# ---- 4. the reference's cells -----------------------------------------------------------------------------------------------------------
def test_bars_of_every_golden_sg_case_expand_to_the_reference_grids():
    e = G.engine()
    bad = []
    sg = [c for c in D.cases() if c.kind == "sg"]
    assert len(sg) == 92
    for c in sg:
        assert c.disp_h <= 127
        row = c.rows[-1:].copy()
        d_h, d_l, d_r = _bars(e, row, c.disp_h, c.disp_w)
        gl, co = _expand_device(e, d_h, d_l, c.disp_h)
        hg, hc = F.bars_cells(G.host(d_h), G.host(d_l), c.disp_h)
        for what, got, want in (("device glyph", gl[0], c.a), ("device colour", co[0], c.b), ("host glyph", hg[0], c.a), ("host colour", hc[0], c.b)):
            if not np.array_equal(got, want):
                bad.append(f"{c.name()} {what}: {D.first_diff(got, want)}")
        rg = G.host(d_r)[0]
        if not np.allclose(rg, c.sg_range, rtol=1e-14, atol=0):
            bad.append(f"{c.name()} range {rg} want {c.sg_range}")
    assert not bad, "\n".join(bad[:20])


# ---- 5. equal to the existing kernel, every cell ----------------------------------------------------------------------------------------
RANGE_BITS = {"rows": 0, "differ": 0}       # how many finite ranges were compared in this module and how many were not bit-equal (reported)


def _against_spectrogram(e, rows, names, disp_h, disp_w, f64, tag, bad):
    k, ln = rows.shape
    d = G.dev(rows)
    d_g, d_c = G.empty((k, disp_h, disp_w), torch.int8), G.empty((k, disp_h, disp_w), torch.int8)
    d_r0 = G.dev(np.full((k, 2), np.nan))          # (the existing kernel leaves the range of a row without a finite value unwritten)
    e.spectrogram_cells(d, k, ln, disp_h, disp_w, d_g, d_c, d_r0, f64=f64)
    d_h, d_l, d_r = _bars(e, rows, disp_h, disp_w, f64)
    gl, co = _expand_device(e, d_h, d_l, disp_h)
    want_g, want_c = G.host(d_g), G.host(d_c)
    h, l = G.host(d_h), G.host(d_l)
    if not np.array_equal(gl, want_g):
        bad.append(f"{tag} glyph: {_first(gl, want_g, names)}")
    if not np.array_equal(co, want_c):
        bad.append(f"{tag} colour: {_first(co, want_c, names)}")
    hg, hc = F.bars_cells(h, l, disp_h)
    if not (np.array_equal(hg, gl) and np.array_equal(hc, co)):
        bad.append(f"{tag}: pss_h_bars_cells and pss_bars_cells differ")
    if not ((h >= -1).all() and (h <= disp_h).all() and (l >= -1).all() and (l <= 3).all() and np.array_equal(h < 0, l < 0)):
        bad.append(f"{tag}: bars outside their ranges")
    r0, r1 = G.host(d_r0), G.host(d_r)
    finite = np.isfinite(rows.astype(np.float64)).any(axis=1)
    if not np.isnan(r1[~finite]).all():
        bad.append(f"{tag}: the range of a row without a finite value must be (NaN, NaN)")
    if not (h[~finite] == -1).all():
        bad.append(f"{tag}: a row without a finite value draws no column")
    if not np.allclose(r1[finite], r0[finite], rtol=1e-14, atol=0):
        i = int(np.argwhere(~np.isclose(r1[finite], r0[finite], rtol=1e-14, atol=0))[0][0])
        bad.append(f"{tag} range: finite row {i}: got {r1[finite][i]} want {r0[finite][i]}")
    RANGE_BITS["rows"] += int(finite.sum())
    RANGE_BITS["differ"] += int(np.count_nonzero((r1[finite].view(np.int64) != r0[finite].view(np.int64)).any(axis=1)))


def _geometries(ln):
    """(disp_h, disp_w): every width with the heights cycled, every height at 112 columns (the widest screens not at 127 lines: host time)."""
    widths = (1, 2, 112, ln, ln + 1, 2 * ln + 1)
    heights = (36, 1, 127)
    out = [(heights[i % 3] if w <= 4096 else heights[i % 2], w) for i, w in enumerate(widths)]
    out += [(h, 112) for h in heights]
    return sorted(set(out))


@pytest.mark.parametrize("ln", [2, 3, 12, 60, 252, 1020, 1021, 2044, 4092, 4093, 16380])
def test_expanded_bars_equal_the_spectrogram_kernel(ln):
    e = G.engine()
    names, rows = B.row_families(ln, 4200 + ln)
    bad = []
    for f64 in (True, False):
        r = rows if f64 else rows.astype(np.float32)
        for disp_h, disp_w in _geometries(ln):
            _against_spectrogram(e, r, names, disp_h, disp_w, f64, f"len={ln} {'f64' if f64 else 'f32'} disp {disp_h}x{disp_w}", bad)
        for k in (1, 3):
            _against_spectrogram(e, r[4:4 + k].copy(), names[4:4 + k], 36, 112, f64, f"len={ln} {'f64' if f64 else 'f32'} batch of {k}", bad)
    print(f"len={ln}: ranges compared so far {RANGE_BITS['rows']}, not bit-equal {RANGE_BITS['differ']}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("ln", [252, 1020, 2044, 4092, 4093])
def test_one_row_past_each_launch_cap(ln):
    """rows_per_launch + 1 rows (the grid-stride loops of k_spectrum_bars / k_spectrogram<T, true> take a second turn; the cells of
    the batch are past k_bars_cells' cap as well), every row different, NaN rows among them."""
    e = G.engine()
    k = B.rows_per_launch(ln) + 1
    disp_h = 36 if k * 36 * 112 > B.BARS_CELLS_PER_LAUNCH else 48
    assert k * disp_h * 112 > B.BARS_CELLS_PER_LAUNCH
    rng = np.random.default_rng(77 + ln)
    names, fam = B.row_families(ln, 99 + ln)
    rows = rng.standard_normal((k, ln)) * 6.0 - 50.0
    rows[:, ln // 4] += 40.0
    rows[::5] = np.round(rows[::5])
    rows[-len(fam):] = fam                  # the tail of the batch (the second turn of the loop): every family
    bad = []
    for f64 in (True, False):
        _against_spectrogram(e, rows if f64 else rows.astype(np.float32), None, disp_h, 112, f64, f"len={ln} {k} rows {'f64' if f64 else 'f32'}", bad)
    assert not bad, "\n".join(bad[:20])


def test_bars_argument_checks():
    e = G.engine()
    lib, h = e.lib, e.h
    rows = G.dev(np.zeros((2, 8)))
    d_h, d_l, d_g = G.empty((2, 4), torch.int8), G.empty((2, 4), torch.int8), G.empty((2, 127, 4), torch.int8)
    p = lambda t: t.data_ptr()
    assert lib.pss_spectrum_bars_f64(h, p(rows), 2, 8, 3, 4, p(d_h), p(d_l), None) == 0
    assert lib.pss_spectrum_bars_f64(h, p(rows), 2, 1, 3, 4, p(d_h), p(d_l), None) == 0       # len 1: one knot
    for args in ((p(rows), 2, 0, 3, 4, p(d_h), p(d_l)), (p(rows), 2, 8, 0, 4, p(d_h), p(d_l)), (p(rows), 2, 8, 128, 4, p(d_h), p(d_l)),
                 (p(rows), 2, 8, 3, 0, p(d_h), p(d_l)), (p(rows), -1, 8, 3, 4, p(d_h), p(d_l)), (None, 2, 8, 3, 4, p(d_h), p(d_l)),
                 (p(rows), 2, 8, 3, 4, None, p(d_l)), (p(rows), 2, 8, 3, 4, p(d_h), None)):
        assert lib.pss_spectrum_bars_f64(h, *args, None) == L.PSS_E_ARG, args
        assert lib.pss_spectrum_bars(h, *args, None) == L.PSS_E_ARG, args
    assert lib.pss_spectrum_bars(h, None, 0, 8, 3, 4, None, None, None) == 0
    assert lib.pss_bars_cells(h, p(d_h), p(d_l), 2, 3, 4, p(d_g), p(d_g)) == 0
    for args in ((p(d_h), p(d_l), 2, 0, 4, p(d_g), p(d_g)), (p(d_h), p(d_l), 2, 128, 4, p(d_g), p(d_g)), (p(d_h), p(d_l), 2, 3, 0, p(d_g), p(d_g)),
                 (None, p(d_l), 2, 3, 4, p(d_g), p(d_g)), (p(d_h), p(d_l), 2, 3, 4, None, p(d_g)), (p(d_h), p(d_l), -1, 3, 4, p(d_g), p(d_g))):
        assert lib.pss_bars_cells(h, *args) == L.PSS_E_ARG, args
    iq = G.dev(np.zeros((2, 64), np.complex64))
    db32 = G.empty((2, 64), torch.float32)
    ok = (L.MODE_AM, p(iq), 2, 64, FS, p(db32), None, None, 3, 4, p(d_h), p(d_l), None, None)
    assert lib.pss_frame_pipeline_bars(h, *ok) == 0
    for i, v in ((0, 9), (3, 48), (3, 8), (8, 0), (8, 128), (9, 0), (5, None), (10, None), (11, None), (1, None), (2, -1)):
        a = list(ok)
        a[i] = v
        assert lib.pss_frame_pipeline_bars(h, *a) == L.PSS_E_ARG, (i, v)
    e.sync()


# ---- 6. from IQ -------------------------------------------------------------------------------------------------------------------------
def _fm_frames(nf, n, seed):
    """Seeded FM-like read buffers: the generator of tests/test_gpu_display_geometry.py for any frame count."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    f = np.arange(nf).reshape(-1, 1)
    iq = (0.5 + 0.4 * (f % 3)) * np.exp(1j * (2 * np.pi * (90e3 + 7e3 * (f % 46)) * t + 0.3 * f))
    iq = iq + 0.03 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))
    return iq.astype(np.complex64)


def _pipeline_bars_checks(e, iq, disp_h, disp_w, modes, tag):
    nf, n = iq.shape
    m = n - 4
    d_iq = G.dev(iq)
    # the existing entry points on the same buffers
    d_db32, d_db64 = G.empty((nf, n), torch.float32), G.empty((nf, n), torch.float64)
    d_lo, d_hi = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64)
    d_a, d_b = G.empty((nf, disp_w), torch.int8), G.empty((nf, disp_w), torch.int8)
    e.spectrum_cells(d_iq, nf, n, d_db32, d_db64, d_lo, d_hi, disp_w, d_a, d_b)
    d_post = G.empty((nf, m), torch.float64)
    e.spectrum_post_f64(d_db64, nf, n, d_post)
    w_h, w_l, w_r = _bars(e, G.host(d_post), disp_h, disp_w)         # item 5's route on those rows
    e.sync()
    for mode in modes:
        n_out = 0 if mode is None else e.demod_out_len(mode, n, FS)
        g_db32, g_db64, g_post = G.empty((nf, n), torch.float32), G.empty((nf, n), torch.float64), G.empty((nf, m), torch.float64)
        g_h, g_l, g_r = G.empty((nf, disp_w), torch.int8), G.empty((nf, disp_w), torch.int8), G.empty((nf, 2), torch.float64)
        g_pcm = None if mode is None else G.empty((nf, n_out, 2), torch.int16)
        for t in (g_db32, g_db64, g_post, g_r):
            t.fill_(float("nan"))
        g_h.fill_(99)
        g_l.fill_(99)
        e.frame_pipeline_bars(L.MODE_NFM if mode is None else mode, d_iq, nf, n, FS, g_db32, g_db64, g_post, disp_h, disp_w, g_h, g_l, g_r, g_pcm)
        e.sync()
        what = f"{tag} mode {mode}"
        assert torch.equal(g_db32.view(torch.int32), d_db32.view(torch.int32)), what + ": d_db32 bytes"
        assert torch.equal(g_db64.view(torch.int64), d_db64.view(torch.int64)), what + ": d_db64 bytes"
        assert torch.equal(g_post.view(torch.int64), d_post.view(torch.int64)), what + ": d_post bytes"
        assert torch.equal(g_h, w_h) and torch.equal(g_l, w_l), what + ": bars of the rows"
        assert torch.equal(g_r.view(torch.int64), w_r.view(torch.int64)), what + ": range of the rows"
        if mode is not None:
            w_pcm = G.empty((nf, n_out, 2), torch.int16)
            e.demod_signal(mode, d_iq, nf, n, FS, w_pcm)
            e.sync()
            assert torch.equal(g_pcm, w_pcm), what + ": PCM bytes"
    # without the optional buffers (context scratch): the same bars
    g_h, g_l = G.empty((nf, disp_w), torch.int8), G.empty((nf, disp_w), torch.int8)
    g_db32 = G.empty((nf, n), torch.float32)
    e.frame_pipeline_bars(L.MODE_NFM, d_iq, nf, n, FS, g_db32, None, None, disp_h, disp_w, g_h, g_l, None, None)
    e.sync()
    assert torch.equal(g_h, w_h) and torch.equal(g_l, w_l) and torch.equal(g_db32.view(torch.int32), d_db32.view(torch.int32)), tag + ": scratch rows"
    return G.host(w_h), G.host(w_l), G.host(w_r), G.host(d_post)


def _against_oracle_from_iq(e, iq, h, l, rg, post_dev, disp_h, disp_w, tag):
    """The pin outside the library: the expanded bars against oracle_lib.spectrogram_cells of the ORACLE's post-processed rows from the same IQ."""
    taps, sos, zi = e.nfm_filters(FS)
    o = O.headline_f64(iq, FS, taps, sos, zi, 30, 1, min(O.threads_available(), 16), pcm=False)
    post = o["post"]
    res = O.map_frames(lambda row: O.spectrogram_cells(row, disp_h, disp_w), list(post))
    want_g, want_c = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    want_r = np.array([[r[2], r[3]] for r in res])
    gl, co = F.bars_cells(h, l, disp_h)
    report = []
    for what, got, want in (("glyph", gl, want_g), ("colour", co, want_c)):
        for f, y, x in np.argwhere(got != want)[:10]:
            report.append(f"{tag} {what} frame {f} y={y} x={x}: got {got[f, y, x]} want {want[f, y, x]}; device row range {rg[f]}, oracle {want_r[f]}; "
                          f"max |row difference| {np.max(np.abs(post_dev[f] - post[f])):.3e} dB")
    assert not report, "\n".join(report)
    assert np.max(np.abs(rg - want_r)) <= 1e-10, f"{tag}: range {np.max(np.abs(rg - want_r)):.3e} dB from the oracle's"


def test_frame_pipeline_bars_on_the_golden_read_buffers(golden):
    e = G.engine()
    iq = np.ascontiguousarray(golden["caller_iq"]["iq"])
    assert iq.shape == (34, 1024)
    h, l, rg, post = _pipeline_bars_checks(e, iq, 36, 112, MODES + (None,), "caller_iq")
    _against_oracle_from_iq(e, iq, h, l, rg, post, 36, 112, "caller_iq")


def test_frame_pipeline_bars_on_2048_fm_frames():
    e = G.engine()
    iq = _fm_frames(2048, 1024, 31337)
    h, l, rg, post = _pipeline_bars_checks(e, iq, 36, 112, MODES + (None,), "2048 x 1024")
    _against_oracle_from_iq(e, iq, h, l, rg, post, 36, 112, "2048 x 1024")


@pytest.mark.parametrize("n", [256, 4096])
def test_frame_pipeline_bars_off_the_headline_length(n):
    e = G.engine()
    iq = _fm_frames(64, n, 500 + n)
    h, l, rg, post = _pipeline_bars_checks(e, iq, 36, 112, (L.MODE_NFM, L.MODE_AM, None), f"64 x {n}")
    _against_oracle_from_iq(e, iq, h, l, rg, post, 36, 112, f"64 x {n}")


def test_frame_pipeline_bars_of_no_frames():
    e = G.engine()
    d_h = G.dev(np.full((1, 4), 7, np.int8))
    e.frame_pipeline_bars(L.MODE_NFM, None, 0, 1024, FS, None, None, None, 36, 4, None, None, None, None)
    e.frame_pipeline_bars(L.MODE_WFM, None, 0, 1024, FS, None, None, None, 36, 4, d_h, d_h, None, d_h)
    e.sync()
    assert (G.host(d_h) == 7).all()


# ---- 7. gradient lines ------------------------------------------------------------------------------------------------------------------
def _gradient_lines(e, rows, disp_w, f64=True, window=30, cut=None):
    """pss_gradient_rows[_f64] of a history pushed as one batch (cut: as two calls joined by the halo of row extremes) -> (glyph, colour)."""
    nf, ln = rows.shape
    tdt = torch.float64 if f64 else torch.float32
    d = G.dev(rows)
    lo, hi = G.empty((nf,), tdt), G.empty((nf,), tdt)
    e.row_extremes(d, nf, ln, lo, hi, f64=f64)
    a, b = G.empty((nf, disp_w), torch.int8), G.empty((nf, disp_w), torch.int8)
    a.fill_(77)
    b.fill_(77)
    if cut is None:
        e.gradient_rows(d, nf, ln, lo, hi, disp_w, a, b, window=window, f64=f64)
    else:
        halo = min(cut, window - 1)
        e.gradient_rows(d[:cut], cut, ln, lo, hi, disp_w, a[:cut], b[:cut], window=window, f64=f64)
        e.gradient_rows(d[cut:], nf - cut, ln, lo[cut - halo:], hi[cut - halo:], disp_w, a[cut:], b[cut:], n_halo=halo, window=window, f64=f64)
    e.sync()
    return G.host(a), G.host(b)


def test_gradient_rows_newest_line_of_every_golden_gw_case():
    e = G.engine()
    gw = [c for c in D.cases() if c.kind == "gw"]
    assert len(gw) == 116
    bad, top = [], 0
    for c in gw:
        assert not c.raised
        a, b = _gradient_lines(e, c.rows, c.disp_w)
        if not np.array_equal(a[-1], c.a[0]):
            bad.append(f"{c.name()} glyph: {D.first_diff(a[-1:], c.a[:1])}")
        if not np.array_equal(b[-1], c.b[0]):
            bad.append(f"{c.name()} colour: {D.first_diff(b[-1:], c.b[:1])}")
        top = max(top, int(c.a[0].max()))
    assert top == 8
    assert not bad, "\n".join(bad[:20])


def _history(nf, ln, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((nf, ln)) * 7.0 - 45.0
    rows[:, ln // 3:ln // 3 + 4] += 30.0
    rows += np.linspace(0.0, 12.0, nf).reshape(-1, 1) * np.sin(np.arange(nf) / 9.0).reshape(-1, 1)
    return rows


@pytest.mark.parametrize("f64", [True, False])
def test_gradient_rows_every_frame_of_a_history_against_the_oracle(f64):
    e = G.engine()
    nf, ln = 100, 252
    rows = _history(nf, ln, 1640)
    rows[41, 7] = np.nan                      # a NaN / +-inf bin beside a knot (disp_w = len: every bin is a knot; 112: between knots)
    rows[63, 100] = np.inf
    rows[80, ln - 1] = -np.inf
    r = rows if f64 else rows.astype(np.float32)
    wide = r.astype(np.float64)
    for disp_w in (112, ln, 2 * ln - 1, 1):
        a, b = _gradient_lines(e, r, disp_w, f64)
        for i in range(nf):
            og, oc = O.gradient_cells(wide[max(0, i - 29):i + 1], 1, disp_w)
            assert np.array_equal(a[i], og[0]) and np.array_equal(b[i], oc[0]), (f64, disp_w, i, D.first_diff(a[i:i + 1], og[:1]))
        assert (a[41] == -1).any() and (a[63] == -1).any() or disp_w == 1
        a2, b2 = _gradient_lines(e, r, disp_w, f64, cut=37)
        assert np.array_equal(a2, a) and np.array_equal(b2, b), f"two calls joined by the halo, disp_w={disp_w}"
        a3, b3 = _gradient_lines(e, r, disp_w, f64, cut=5)
        assert np.array_equal(a3, a) and np.array_equal(b3, b), f"two calls joined by a short halo, disp_w={disp_w}"


def test_gradient_rows_of_a_constant_history():
    """range 0 -> 1 (pyspecsdr.py:1657-1659): every cell glyph 0, colour 0 (the plain waterfall has no such guard)."""
    e = G.engine()
    for f64 in (True, False):
        rows = np.full((5, 60), -42.5, np.float64 if f64 else np.float32)
        a, b = _gradient_lines(e, rows, 50, f64)
        assert (a == 0).all() and (b == 0).all()


def test_gradient_rows_argument_checks():
    e = G.engine()
    lib, h = e.lib, e.h
    p = lambda t: t.data_ptr()
    rows, lo = G.dev(np.zeros((2, 8))), G.dev(np.zeros(2))
    a = G.empty((2, 4), torch.int8)
    assert lib.pss_gradient_rows_f64(h, p(rows), 2, 8, p(lo), p(lo), 0, 30, 4, p(a), p(a)) == 0
    for args in ((p(rows), 2, 1, p(lo), p(lo), 0, 30, 4, p(a), p(a)), (p(rows), 2, 8, p(lo), p(lo), 0, 30, 0, p(a), p(a)),
                 (p(rows), 2, 8, p(lo), p(lo), 0, 0, 4, p(a), p(a)), (p(rows), 2, 8, p(lo), p(lo), -1, 30, 4, p(a), p(a)),
                 (p(rows), 2, 8, p(lo), p(lo), 0, 30, 4, p(a), None), (p(rows), 2, 8, None, p(lo), 0, 30, 4, p(a), p(a))):
        assert lib.pss_gradient_rows_f64(h, *args) == L.PSS_E_ARG, args
        assert lib.pss_gradient_rows(h, *args) == L.PSS_E_ARG, args
    e.sync()


@pytest.mark.parametrize("n", [1024, 2048])
def test_display_2_through_every_batched_step(n):
    """display = 2 returns pss_gradient_rows*' lines on the materialised rows; every other output is byte-equal to the display = 0 call."""
    e = G.engine()
    nf, dw, m = 70, 112, n - 4
    iq = _fm_frames(nf, n, 2000 + n)
    d_iq = G.dev(iq)
    n_out = e.demod_out_len(L.MODE_NFM, n, FS)
    i8 = lambda: G.empty((nf, dw), torch.int8)

    def run(call, tdt, display):
        out = dict(lo=G.empty((nf,), tdt), hi=G.empty((nf,), tdt), a=i8(), b=i8(), pcm=G.empty((nf, n_out, 2), torch.int16),
                   db32=G.empty((nf, n), torch.float32), db=G.empty((nf, n), tdt), post=G.empty((nf, m), tdt),
                   pcm_am=G.empty((nf, e.demod_out_len(L.MODE_AM, n, FS), 2), torch.int16))
        for t in out.values():
            t.zero_()
        out["ret"] = call(out, display)
        e.sync()
        return out

    steps = {
        "frame_pipeline_cells": (torch.float64, lambda o, d: e.frame_pipeline_cells(L.MODE_NFM, d_iq, nf, n, FS, o["db32"], o["db"], o["lo"], o["hi"], dw,
                                                                                    o["a"], o["b"], o["pcm"], display=d)),
        "frame_pipeline_cells (AM)": (torch.float64, lambda o, d: e.frame_pipeline_cells(L.MODE_AM, d_iq, nf, n, FS, o["db32"], None, o["lo"], o["hi"], dw,
                                                                                         o["a"], o["b"], o["pcm_am"], display=d)),
        "frame_pipeline_f64": (torch.float64, lambda o, d: e.frame_pipeline_f64(L.MODE_NFM, d_iq, nf, n, FS, o["db"], None, o["lo"], o["hi"], dw, o["a"],
                                                                                o["b"], o["pcm"], display=d)),
        "frame_pipeline_f64 rows": (torch.float64, lambda o, d: e.frame_pipeline_f64(L.MODE_NFM, d_iq, nf, n, FS, o["db"], o["post"], o["lo"], o["hi"], dw,
                                                                                     o["a"], o["b"], o["pcm"], display=d)),
        "frame_pipeline": (torch.float32, lambda o, d: e.frame_pipeline(L.MODE_NFM, d_iq, nf, n, FS, o["db"], None, o["lo"], o["hi"], dw, o["a"], o["b"],
                                                                        o["pcm"], display=d)),
        "frame_pipeline rows": (torch.float32, lambda o, d: e.frame_pipeline(L.MODE_NFM, d_iq, nf, n, FS, o["db"], o["post"], o["lo"], o["hi"], dw, o["a"],
                                                                             o["b"], o["pcm"], display=d)),
        "spectrum_cells": (torch.float64, lambda o, d: e.spectrum_cells(d_iq, nf, n, o["db32"], o["db"], o["lo"], o["hi"], dw, o["a"], o["b"], display=d)),
        "frame_pipeline_squelch": (torch.float64, lambda o, d: e.frame_pipeline_squelch(L.MODE_NFM, d_iq, nf, n, FS, o["db32"], o["db"], o["lo"], o["hi"], dw,
                                                                                       o["a"], o["b"], o["pcm"], -60.0, o["lo"].new_empty(nf), display=d)),
    }
    # the materialised rows of either type and the gradient lines of those
    d_db64, d_p64 = G.empty((nf, n), torch.float64), G.empty((nf, m), torch.float64)
    e.spectrum_db_f64(d_iq, nf, n, d_db64)
    e.spectrum_post_f64(d_db64, nf, n, d_p64)
    d_db32, d_p32 = G.empty((nf, n), torch.float32), G.empty((nf, m), torch.float32)
    e.spectrum_db(d_iq, nf, n, d_db32)
    e.spectrum_post(d_db32, nf, n, d_p32)
    e.sync()
    want = {torch.float64: _gradient_lines(e, G.host(d_p64), dw, True), torch.float32: _gradient_lines(e, G.host(d_p32), dw, False)}
    assert want[torch.float64][0].max() >= 6 and want[torch.float64][1].max() >= 4        # (the gradient's own glyph indices, past the waterfall's 0 .. 3)
    for name, (tdt, call) in steps.items():
        g, w = run(call, tdt, "gradient"), run(call, tdt, "waterfall")
        assert np.array_equal(G.host(g["a"]), want[tdt][0]), f"n={n} {name}: gradient glyphs"
        assert np.array_equal(G.host(g["b"]), want[tdt][1]), f"n={n} {name}: gradient colours"
        assert not torch.equal(g["a"], w["a"]), f"n={n} {name}: the waterfall's glyphs"
        for k in ("lo", "hi", "pcm", "pcm_am", "db32", "db", "post"):
            assert torch.equal(g[k].view(torch.uint8), w[k].view(torch.uint8)), f"n={n} {name}: {k} differs between display 2 and display 0"
        assert g["ret"] == w["ret"], f"n={n} {name}: return values"

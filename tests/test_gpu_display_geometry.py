"""The display quantisers and the batched display lines on the GPU across screen sizes, row lengths and history depths — cell for cell
against the oracle, and for the stateless quantisers against the reference's own grids (tests/golden/display.npz, tools/make_goldens_display.py).

- every golden case through pss_{waterfall,persistence,gradient,spectrogram}_cells[_f64], pss_surface_cells[_f64] and the device rings;
  float32 entry points get the rows rounded to float32 and are compared with the oracle on those values widened (the kernels widen them too);
- rings pushed 120 times (several wraps) with the screen size changed between pushes, against the stateless call on the same window;
- the batched lines (frame_pipeline_cells / _f64 / float32, spectrum_cells, waterfall_rows / persistence_rows and their _db twins) at
  n_fft 16 .. 16384, display widths 1 .. 2m - 1 and heights 1 .. 127, a batch cut in two with a halo of row extremes;
- caller rows with NaN / +-inf bins through the line kernels; a constant history (the reference raises in draw_waterfall).
Failures name the case / geometry, the frame and the cell."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import display_cases as D
import gpu_util as G
import oracle_lib as O
from pyspecsdr_amd import _lib as L


def _cells(e, c, rows, f64):
    """The GPU grids of case c on `rows` (float32 or float64): (a, b or None, range or None)."""
    n, ln = rows.shape
    dh, dw = c.disp_h, c.disp_w
    d = G.dev(rows)
    if c.kind == "sf":
        d_a = G.empty((c.H, c.W), torch.int8)
        e.surface_cells(d[-1].contiguous(), ln, c.H, c.W, d_a, f64=f64)
        e.sync()
        return G.host(d_a), None, None
    d_a = G.empty((dh, dw), torch.int8)
    d_b = G.empty((dh, dw), torch.int8)
    d_r = None
    if c.kind == "wf":
        e.waterfall_cells(d, n, ln, dh, dw, d_a, d_b, f64=f64)
    elif c.kind == "gw":
        e.gradient_cells(d, n, ln, dh, dw, d_a, d_b, f64=f64)
    elif c.kind == "ps":
        e.persistence_cells(d, n, ln, dh, dw, d_a, f64=f64)
    else:
        d_r = G.empty((1, 2), torch.float64)
        e.spectrogram_cells(d[-1:].contiguous(), 1, ln, dh, dw, d_a, d_b, d_r, f64=f64)
    e.sync()
    b = None if c.kind == "ps" else G.host(d_b)
    return G.host(d_a), b, (G.host(d_r)[0] if d_r is not None else None)


def _check(bad, tag, got, want):
    if not np.array_equal(got, want):
        bad.append(f"{tag}: {D.first_diff(got, want)}")


@pytest.mark.parametrize("kind", ["wf", "ps", "gw", "sf", "sg"])
def test_stateless_quantisers_at_every_golden_case(kind):
    e = G.engine()
    bad = []
    for c in D.cases():
        if c.kind != kind or c.raised:
            continue
        # float64 rows: the reference's own grids
        a, b, rg = _cells(e, c, c.rows, True)
        _check(bad, f"{c.name()} f64 a", a, c.a)
        if c.b is not None:
            _check(bad, f"{c.name()} f64 b", b, c.b)
        if kind == "sg" and not np.allclose(rg, c.sg_range, rtol=1e-14, atol=0):
            bad.append(f"{c.name()} f64 range {rg} want {c.sg_range}")
        # float32 rows: the oracle on the same values
        r32 = c.rows.astype(np.float32)
        oa, ob, org = D.oracle(c, r32.astype(np.float64))
        a, b, rg = _cells(e, c, r32, False)
        _check(bad, f"{c.name()} f32 a", a, oa)
        if ob is not None:
            _check(bad, f"{c.name()} f32 b", b, ob)
        if kind == "sg" and not np.allclose(rg, org, rtol=1e-14, atol=0):
            bad.append(f"{c.name()} f32 range {rg} want {org}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("kind", ["wf", "ps"])
def test_rings_at_every_golden_case(kind):
    """pss_ring_waterfall / pss_ring_persistence after pushing a golden case's rows (float32) into a ring of the reference's depth."""
    e = G.engine()
    bad = []
    for c in D.cases():
        if c.kind != kind or c.raised:
            continue
        r32 = c.rows.astype(np.float32)
        ring = e.ring_create(D.WINDOW[kind], c.length)
        try:
            d = G.dev(r32)
            for i in range(len(r32)):
                e.ring_push(ring, d[i])
            d_a = G.empty((c.disp_h, c.disp_w), torch.int8)
            if kind == "wf":
                d_b = G.empty((c.disp_h, c.disp_w), torch.int8)
                e.ring_waterfall(ring, c.disp_h, c.disp_w, d_a, d_b)
            else:
                e.ring_persistence(ring, c.disp_h, c.disp_w, d_a)
            e.sync()
        finally:
            e.ring_destroy(ring)
        oa, ob, _ = D.oracle(c, r32.astype(np.float64))
        _check(bad, f"{c.name()} ring a", G.host(d_a), oa)
        if kind == "wf":
            _check(bad, f"{c.name()} ring b", G.host(d_b), ob)
    assert not bad, "\n".join(bad[:20])


def test_rings_wrap_with_the_screen_resized_between_pushes():
    """120 pushes into 30- and 10-deep rings (four and twelve wraps), a different screen after every push (heights 1 .. 60 around the
    depth, widths 1 .. 2 len - 1): the ring's cells equal the stateless call on the same window, and the oracle's on every tenth push."""
    e = G.engine()
    rng = np.random.default_rng(2718)
    ln = 60
    rows = (rng.standard_normal((120, ln)) * 7.0 - 45.0).astype(np.float32)
    rows[:, 20:24] += 30.0
    rows[37, 5] = np.nan
    rows[64, 0] = np.inf
    rows[90, ln - 1] = -np.inf
    heights = (1, 2, 9, 29, 30, 31, 36, 60)
    widths = (1, 2, 3, ln - 1, ln, ln + 1, 2 * ln - 1, 112)
    d_rows = G.dev(rows)
    wf, ps = e.ring_create(30, ln), e.ring_create(10, ln)
    try:
        for i in range(len(rows)):
            e.ring_push(wf, d_rows[i])
            e.ring_push(ps, d_rows[i])
            dh, dw = heights[(i * 5) % len(heights)], widths[(i * 3 + i // 8) % len(widths)]
            a_g, a_c, b_c, r_g, r_c, q_c = (G.empty((dh, dw), torch.int8) for _ in range(6))
            e.ring_waterfall(wf, dh, dw, a_g, a_c)
            e.ring_persistence(ps, dh, dw, b_c)
            w0, p0 = max(0, i + 1 - 30), max(0, i + 1 - 10)
            e.waterfall_cells(d_rows[w0:i + 1].contiguous(), i + 1 - w0, ln, dh, dw, r_g, r_c)
            e.persistence_cells(d_rows[p0:i + 1].contiguous(), i + 1 - p0, ln, dh, dw, q_c)
            e.sync()
            geo = f"push {i} screen {dh}x{dw}"
            for got, want, what in ((a_g, r_g, "waterfall glyph"), (a_c, r_c, "waterfall colour"), (b_c, q_c, "persistence")):
                assert torch.equal(got, want), f"{geo} {what}: {D.first_diff(G.host(got), G.host(want))}"
            if i % 10 == 9:
                og, oc = O.waterfall_cells(rows[w0:i + 1].astype(np.float64), dh, dw)
                op = O.persistence_cells(rows[p0:i + 1].astype(np.float64), dh, dw)
                for got, want, what in ((a_g, og, "waterfall glyph"), (a_c, oc, "waterfall colour"), (b_c, op, "persistence")):
                    assert np.array_equal(G.host(got), want), f"{geo} {what} vs oracle: {D.first_diff(G.host(got), want)}"
    finally:
        e.ring_destroy(wf)
        e.ring_destroy(ps)


# ---- batched display lines ----------------------------------------------------------------------------------------------------------
NF, CUT, FS = 46, 13, 2.4e6          # 46 frames = 13 + 33: neither call a multiple of k_disp_vals_win's 32 rows, the second with a halo of 13


def _geometries(m):
    """(display, disp_w, disp_h): every width for both displays, the persistence heights cycled over the widths and all at 112."""
    widths = sorted({1, 2, 3, 72, 112, 192, 256, 257, m - 1, m, m + 1, 2 * m - 1} - {0})
    heights = (1, 2, 20, 36, 127)
    out = [("waterfall", w, 36) for w in widths]
    out += [("persistence", w, heights[k % len(heights)]) for k, w in enumerate(widths)]
    out += [("persistence", 112, h) for h in heights]
    return out


def _iq(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    iq = np.stack([(0.5 + 0.4 * (f % 3)) * np.exp(1j * (2 * np.pi * (90e3 + 7e3 * f) * t + 0.3 * f)) for f in range(NF)])
    iq += 0.03 * (rng.standard_normal((NF, n)) + 1j * rng.standard_normal((NF, n)))
    return iq.astype(np.complex64)


def _oracle_lines_f64(post, lo, hi, window, display, disp_w, disp_h):
    nf, ln = post.shape
    a, b = np.empty((nf, disp_w), np.int8), np.empty((nf, disp_w), np.int8)
    Lo = O.lib()
    if display == "waterfall":
        Lo.pss_o_waterfall_rows_f64(post.reshape(-1), lo, hi, nf, ln, window, disp_w, a.reshape(-1), b.reshape(-1), 1)
        return a, b
    Lo.pss_o_persistence_rows_f64(post.reshape(-1), lo, hi, nf, ln, window, disp_h, disp_w, a.reshape(-1), 1)
    return a, None


def _oracle_lines_f32(post, display, disp_w, disp_h):
    if display == "waterfall":
        return O.waterfall_rows(post, 30, disp_w)
    return O.persistence_rows(post, 10, disp_h, disp_w), None


def _compare_lines(bad, tag, got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            continue
        if not np.array_equal(g, w):
            f, x = np.argwhere(g != w)[0]
            bad.append(f"{tag} line {'ab'[k]}: {int(np.count_nonzero(g != w))} cells differ, first frame {f} x {x}: got {g[f, x]} want {w[f, x]}")


def _two_calls(call, disp_w, lo_dtype):
    """Run `call(lo, hi, a, b, lo_off, sl, n_halo)` over frames [0, CUT) and then [CUT, NF) with a halo of CUT row extremes."""
    lo, hi = G.empty((NF,), lo_dtype), G.empty((NF,), lo_dtype)
    a, b = G.empty((NF, disp_w), torch.int8), G.empty((NF, disp_w), torch.int8)
    call(lo, hi, a, b, slice(0, CUT), 0)
    call(lo, hi, a, b, slice(CUT, NF), CUT)
    return lo, hi, a, b


@pytest.mark.parametrize("n", [16, 256, 1024, 4096, 16384])
def test_batched_lines_across_widths_and_heights(n):
    e = G.engine()
    m = n - 4
    iq = _iq(n, 900 + n)
    d_iq = G.dev(iq)
    taps, sos, zi = e.nfm_filters(FS)
    o = O.headline_f64(iq, FS, taps, sos, zi, 30, 1, min(O.threads_available(), 16), pcm=False)
    post, lo, hi = o["post"], o["lo"], o["hi"]
    mode = L.MODE_NFM if n > 28 else L.MODE_AM      # (demodulate_nfm's filtfilt needs more than 28 samples: PSS_E_PADLEN, as the reference raises)
    n_out = e.demod_out_len(mode, n, FS)
    d_pcm = G.empty((NF, n_out, 2), torch.int16)
    d_db64, d_db32, d_post64 = G.empty((NF, n), torch.float64), G.empty((NF, n), torch.float32), G.empty((NF, m), torch.float64)
    d_db32b, d_post32 = G.empty((NF, n), torch.float32), G.empty((NF, m), torch.float32)
    bad = []
    fuse = (1, 0) if n == 1024 else (1,)
    for display, dw, dh in _geometries(m):
        geo = f"n_fft={n} {display} disp_w={dw} disp_h={dh}"
        win = 30 if display == "waterfall" else 10
        want = _oracle_lines_f64(post, lo, hi, win, display, dw, dh)
        kw = dict(display=display, disp_h=dh)
        for fp in fuse:
            e.set_option("fuse_post", fp)
            try:
                runs = {
                    "frame_pipeline_cells": lambda lo_, hi_, a, b, s, h: e.frame_pipeline_cells(
                        mode, d_iq[s], s.stop - s.start, n, FS, d_db32[s], None, lo_, hi_, dw, a[s], b[s], d_pcm[s], n_halo=h, **kw),
                    "frame_pipeline_f64 rows": lambda lo_, hi_, a, b, s, h: e.frame_pipeline_f64(
                        mode, d_iq[s], s.stop - s.start, n, FS, d_db64[s], d_post64[s], lo_, hi_, dw, a[s], b[s], d_pcm[s], n_halo=h, **kw),
                    "frame_pipeline_f64": lambda lo_, hi_, a, b, s, h: e.frame_pipeline_f64(
                        mode, d_iq[s], s.stop - s.start, n, FS, d_db64[s], None, lo_, hi_, dw, a[s], b[s], d_pcm[s], n_halo=h, **kw),
                    "spectrum_cells": lambda lo_, hi_, a, b, s, h: e.spectrum_cells(
                        d_iq[s], s.stop - s.start, n, d_db32[s], None, lo_, hi_, dw, a[s], b[s], n_halo=h, **kw),
                }
                if fp == 0:
                    runs = {k + " fuse_post=0": v for k, v in runs.items() if k in ("frame_pipeline_cells", "spectrum_cells")}
                for name, call in runs.items():
                    _, _, a, b = _two_calls(call, dw, torch.float64)
                    e.sync()
                    got = (G.host(a), G.host(b))
                    _compare_lines(bad, f"{geo} {name}", got, want)
            finally:
                e.set_option("fuse_post", 1)
        # float32 rows: the lines against the oracle on the post-processed rows the same call returned
        for name, with_post in (("frame_pipeline rows", True), ("frame_pipeline", False)):
            call = lambda lo_, hi_, a, b, s, h: e.frame_pipeline(
                mode, d_iq[s], s.stop - s.start, n, FS, d_db32b[s], d_post32[s] if with_post else None, lo_, hi_, dw, a[s], b[s], d_pcm[s],
                n_halo=h, **kw)
            if with_post:
                _, _, a, b = _two_calls(call, dw, torch.float32)
                e.sync()
                p32 = G.host(d_post32)
                want32 = _oracle_lines_f32(p32, display, dw, dh)
            else:
                _, _, a, b = _two_calls(call, dw, torch.float32)
                e.sync()
            _compare_lines(bad, f"{geo} {name}", (G.host(a), G.host(b)), want32)
        # the accumulators' own entry points on those rows: materialised (waterfall_rows) and rebuilt from the dB rows (*_rows_db)
        d_thr, lo2, hi2 = G.empty((NF,), torch.float32), G.empty((NF,), torch.float32), G.empty((NF,), torch.float32)
        lo1, hi1 = G.empty((NF,), torch.float32), G.empty((NF,), torch.float32)
        d_p = G.empty((NF, m), torch.float32)
        e.spectrum_post_extremes(d_db32b, NF, n, d_p, lo1, hi1)
        e.spectrum_post_thresholds(d_db32b, NF, n, d_thr, lo2, hi2)
        e.sync()
        assert torch.equal(d_p, d_post32), geo
        for name in ("rows", "rows_db"):
            a, b = G.empty((NF, dw), torch.int8), G.empty((NF, dw), torch.int8)
            for s, h in ((slice(0, CUT), 0), (slice(CUT, NF), CUT)):
                k = s.stop - s.start
                if name == "rows" and display == "waterfall":
                    e.waterfall_rows(d_p[s], k, m, lo1[s.start - h:], hi1[s.start - h:], dw, a[s], b[s], n_halo=h, window=30)
                elif name == "rows":
                    e.persistence_rows(d_p[s], k, m, lo1[s.start - h:], hi1[s.start - h:], dh, dw, a[s], n_halo=h, window=10)
                elif display == "waterfall":
                    e.waterfall_rows_db(d_db32b[s], k, n, d_thr[s], lo2[s.start - h:], hi2[s.start - h:], dw, a[s], b[s], n_halo=h, window=30)
                else:
                    e.persistence_rows_db(d_db32b[s], k, n, d_thr[s], lo2[s.start - h:], hi2[s.start - h:], dh, dw, a[s], n_halo=h, window=10)
            e.sync()
            _compare_lines(bad, f"{geo} {name}", (G.host(a), G.host(b)), want32)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("display", ["waterfall", "persistence"])
def test_lines_of_caller_rows_with_non_finite_bins(display):
    """The golden cases' rows with NaN / +-inf bins, and a constant history, through pss_waterfall_rows / pss_persistence_rows (float32 and
    float64): every frame's line against the oracle; the float64 waterfall's newest line against the reference's top grid row."""
    e = G.engine()
    bad = []
    kind = "wf" if display == "waterfall" else "ps"
    sel = [c for c in D.cases() if c.kind == kind and len(c.rows) == 3 and not np.isfinite(c.rows).all()]
    assert len(sel) == 24
    for c in sel:
        rows = c.rows
        nf, ln = rows.shape
        dw, dh = c.disp_w, min(c.disp_h, 127)
        win = 30 if display == "waterfall" else 10
        for f64, r in ((True, rows), (False, rows.astype(np.float32))):
            tdt = torch.float64 if f64 else torch.float32
            d = G.dev(r)
            lo, hi = G.empty((nf,), tdt), G.empty((nf,), tdt)
            e.row_extremes(d, nf, ln, lo, hi, f64=f64)
            a, b = G.empty((nf, dw), torch.int8), G.empty((nf, dw), torch.int8)
            if display == "waterfall":
                e.waterfall_rows(d, nf, ln, lo, hi, dw, a, b, window=win, f64=f64)
            else:
                e.persistence_rows(d, nf, ln, lo, hi, dh, dw, a, window=win, f64=f64)
            e.sync()
            if f64:
                want = _oracle_lines_f64(rows, G.host(lo), G.host(hi), win, display, dw, dh)
                if display == "waterfall":
                    _compare_lines(bad, f"{c.name()} newest line vs reference", (G.host(a)[-1:], G.host(b)[-1:]), (c.a[:1], c.b[:1]))
            else:
                want = _oracle_lines_f32(r, display, dw, dh)
            _compare_lines(bad, f"{c.name()} {'f64' if f64 else 'f32'}", (G.host(a), G.host(b)), want)
    assert not bad, "\n".join(bad[:20])


def test_constant_history_where_the_reference_raises():
    """draw_waterfall of a constant history divides 0 by 0 and raises (int(NaN), pyspecsdr.py:1389).  The library draws every cell of the
    history's rows as glyph 0 ('.') in colour 0 — the same in the stateless quantiser, the ring and the line — and leaves the rows below
    undrawn (PARITY.md).  The guarded displays (persistence, gradient, surface) and the spectrogram equal the reference's grids."""
    e = G.engine()
    zr = [c for c in D.cases() if np.all(c.rows == -42.5)]
    assert sorted(c.kind for c in zr) == sorted(["wf", "ps", "gw", "sf", "sg"] * 2)
    for c in zr:
        for f64 in (True, False):
            a, b, _ = _cells(e, c, c.rows if f64 else c.rows.astype(np.float32), f64)
            if c.kind != "wf":
                assert c.a is not None and np.array_equal(a, c.a), c.name()
                assert c.b is None or np.array_equal(b, c.b), c.name()
                continue
            assert c.raised, c.name()
            n = len(c.rows)
            assert np.all(a[:n] == 0) and np.all(b[:n] == 0), (c.name(), f64)
            assert np.all(a[n:] == -1) and np.all(b[n:] == -1), (c.name(), f64)
        if c.kind == "wf":
            ring = e.ring_create(30, c.length)
            try:
                d = G.dev(c.rows.astype(np.float32))
                for i in range(len(c.rows)):
                    e.ring_push(ring, d[i])
                d_a, d_b = G.empty((c.disp_h, c.disp_w), torch.int8), G.empty((c.disp_h, c.disp_w), torch.int8)
                e.ring_waterfall(ring, c.disp_h, c.disp_w, d_a, d_b)
                e.sync()
            finally:
                e.ring_destroy(ring)
            assert np.array_equal(G.host(d_a), a) and np.array_equal(G.host(d_b), b), c.name()
            d = G.dev(c.rows)
            lo, hi = G.empty((len(c.rows),), torch.float64), G.empty((len(c.rows),), torch.float64)
            e.row_extremes(d, len(c.rows), c.length, lo, hi, f64=True)
            la, lb = G.empty((len(c.rows), c.disp_w), torch.int8), G.empty((len(c.rows), c.disp_w), torch.int8)
            e.waterfall_rows(d, len(c.rows), c.length, lo, hi, c.disp_w, la, lb, f64=True)
            e.sync()
            assert np.all(G.host(la) == 0) and np.all(G.host(lb) == 0), c.name()

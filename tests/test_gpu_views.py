"""The surface plot and the constellation in their compact forms for batches, on the GPU through the C ABI (include/pss.h, "surface
magnitudes" / "constellation masks"):

- pss_surface_mags_f64 -> pss_mags_cells / pss_h_mags_cells against the reference's own grids (tests/golden/display.npz, every `sf` case) and
  pss_surface_cells_f64 of the same row; d_range bit-equal to pss_row_extremes_f64;
- the expanded magnitudes of seeded batches against pss_surface_cells[_f64] of every row and against the oracle, both row types, every kernel
  configuration, one row past each launch cap;
- pss_vector_masks against the reference's grids (tests/golden/views.npz), and every frame of interleaved batches against pss_vector_cells
  and the oracle;
- pss_frame_pipeline_surface / _vector from IQ: rows and PCM byte-equal to pss_frame_pipeline_bars', magnitudes and masks equal to the
  stand-alone entry points', and the expanded surface equal to the oracle's cells computed from the same IQ.
Zero differing cells is the requirement everywhere.  Failures name the geometry, the row / frame and the cell."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bars_util as B
import display_cases as D
import gpu_util as G
import oracle_lib as O
import views_cases as V
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F

FS = 2.4e6
MODES = (L.MODE_NFM, L.MODE_AM, L.MODE_USB, L.MODE_LSB, L.MODE_WFM)
# rows / frames one launch covers without its grid-stride loop (pss_fft.hip: MAGS_* / MASK_* and the 2048-workgroup caps)
MAGS_ROWS_PER_LAUNCH = ((1024, 2048 * 4), (4092, 2048), (1 << 20, 2048))       # (longest row, rows): one wavefront per row; four, in LDS; four, re-read
MASK_WAVE_MAX_N, MASK_FRAMES_WAVE, MASK_FRAMES_GROUP = 4096, 2048 * 4, 2048
CELLS_PER_LAUNCH = 16384 * 256                                                 # k_mags_cells / k_masks_cells: one thread per cell


def _mags(e, rows, disp_w, f64=True):
    k, ln = rows.shape
    d_m, d_r = G.empty((k, disp_w), torch.int8), G.empty((k, 2), torch.float64)
    d_m.fill_(99)
    e.surface_mags(G.dev(rows), k, ln, disp_w, d_m, d_r, f64=f64)
    return d_m, d_r


def _expand_device(e, d_m, H, W):
    k = d_m.shape[0]
    d_c = G.empty((k, H, W), torch.int8)
    d_c.fill_(77)
    e.mags_cells(d_m, k, H, W, d_c)
    e.sync()
    return G.host(d_c)


def _surface_cells_loop(e, rows, idx, H, W, f64):
    """pss_surface_cells[_f64] of rows[idx], one launch per row -> int8 [len(idx)][H][W]."""
    d = G.dev(rows)
    out = G.empty((len(idx), H, W), torch.int8)
    for j, i in enumerate(idx):
        e.surface_cells(d[i], rows.shape[1], H, W, out[j], f64=f64)
    e.sync()
    return G.host(out)


def _extremes(e, rows, f64):
    k, ln = rows.shape
    tdt = torch.float64 if f64 else torch.float32
    lo, hi = G.empty((k,), tdt), G.empty((k,), tdt)
    e.row_extremes(G.dev(rows), k, ln, lo, hi, f64=f64)
    e.sync()
    return np.stack([G.host(lo).astype(np.float64), G.host(hi).astype(np.float64)], axis=1)


def _first(got, want, names=None):
    bad = np.argwhere(got != want)
    r, y, x = bad[0]
    tag = f" ({names[r]})" if names else ""
    return f"{len(bad)} cells differ, first row {r}{tag} y={y} x={x}: got {got[r, y, x]} want {want[r, y, x]}"


# ---- surface magnitudes on the goldens --------------------------------------------------------------------------------------------------
def test_mags_of_every_golden_sf_case_expand_to_the_reference_grids():
    e = G.engine()
    sf = [c for c in D.cases() if c.kind == "sf"]
    assert len(sf) == 92
    bad = []
    for c in sf:
        row = c.rows[-1:].copy()
        d_m, d_r = _mags(e, row, c.disp_w)
        dev = _expand_device(e, d_m, c.H, c.W)[0]
        mag = G.host(d_m)
        want_mag, _ = V.surface_mags_numpy(row[0], c.disp_w)
        if not np.array_equal(mag[0], want_mag):
            x = int(np.argwhere(mag[0] != want_mag)[0][0])
            bad.append(f"{c.name()} magnitudes: {np.count_nonzero(mag[0] != want_mag)} differ, first x={x}: got {mag[0, x]} want {want_mag[x]}")
        host = F.surface_cells(mag, c.H, c.W)[0]
        old = _surface_cells_loop(e, row, [0], c.H, c.W, True)[0]
        for what, got, want in (("device expansion", dev, c.a), ("host expansion", host, c.a), ("pss_surface_cells_f64", old, c.a)):
            if not np.array_equal(got, want):
                bad.append(f"{c.name()} {what}: {D.first_diff(got, want)}")
        if not np.array_equal(G.host(d_r).view(np.int64), _extremes(e, row, True).view(np.int64)):
            bad.append(f"{c.name()} range {G.host(d_r)} is not pss_row_extremes_f64's {_extremes(e, row, True)}")
    assert not bad, "\n".join(bad[:20])


# ---- surface magnitudes on seeded batches -----------------------------------------------------------------------------------------------
def _families(ln, seed):
    """bars_util's families (constant rows, rows without a finite value, values that differ only in their low words, NaN / +-inf at random
    places and at both ends) plus non-finite bins beside interior knots."""
    names, rows = B.row_families(ln, seed)
    rng = np.random.default_rng(seed + 1)
    extra = []
    if ln > 3:
        for what, tag in ((np.nan, "NaN"), (np.inf, "+inf"), (-np.inf, "-inf")):
            r = rng.standard_normal(ln) * 6.0 - 50.0
            r[[1, ln // 2, ln - 2]] = what
            extra.append((f"{tag} at bins 1, len / 2, len - 2", r))
    zeros = np.abs(rng.standard_normal(ln)) * 3.0
    zeros[rng.random(ln) < 0.4] = 0.0
    zeros[rng.random(ln) < 0.5] *= -1.0          # zeros of both signs as the row's extremes (minimum here, maximum in the negated row): d_range's bits
    extra += [("a zero minimum with both signs", np.abs(zeros) * np.where(zeros == 0, np.sign(np.copysign(1.0, zeros)), 1.0)),
              ("a zero maximum with both signs", -np.abs(zeros) * np.where(zeros == 0, np.sign(np.copysign(1.0, zeros)), 1.0))]
    return names + [n for n, _ in extra], np.ascontiguousarray(np.concatenate([rows] + [r[None] for _, r in extra]))


def _against_surface_cells(e, rows, names, H, W, f64, tag, bad, loop_idx=None):
    """Every row's expansion (device and host) against the oracle; rows loop_idx (default: all) against pss_surface_cells[_f64] too."""
    k, ln = rows.shape
    d_m, d_r = _mags(e, rows, W - 8, f64)
    dev = _expand_device(e, d_m, H, W)
    mag = G.host(d_m)
    if not ((mag >= -1) & (mag <= 20)).all():
        bad.append(f"{tag}: magnitudes outside [-1, 20]")
    host = F.surface_cells(mag, H, W)
    if not np.array_equal(host, dev):
        bad.append(f"{tag}: pss_h_mags_cells and pss_mags_cells differ: {_first(dev, host, names)}")
    wide = rows.astype(np.float64)
    want = np.stack(O.map_frames(lambda r: O.surface_cells(r, H, W), list(wide)))
    if not np.array_equal(dev, want):
        bad.append(f"{tag} against the oracle: {_first(dev, want, names)}")
    idx = list(range(k)) if loop_idx is None else loop_idx
    old = _surface_cells_loop(e, rows, idx, H, W, f64)
    if not np.array_equal(dev[idx], old):
        bad.append(f"{tag} against pss_surface_cells: {_first(dev[idx], old, [names[i] for i in idx] if names else None)}")
    rg, ex = G.host(d_r), _extremes(e, rows, f64)
    if not np.array_equal(rg.view(np.int64), ex.view(np.int64)):
        i = int(np.argwhere((rg != ex).any(axis=1) | (np.signbit(rg) != np.signbit(ex)).any(axis=1))[0][0])
        bad.append(f"{tag} range: row {i}: got {rg[i]} want pss_row_extremes' {ex[i]}")
    finite = np.isfinite(wide).any(axis=1)
    if not ((mag[~finite] == -1).all() and np.array_equal(rg[~finite], np.tile([np.inf, -np.inf], (int((~finite).sum()), 1)))):
        bad.append(f"{tag}: a row without a finite value gives (+inf, -inf) and draws no column")


def _screens(ln):
    """(max_h, max_w): widths 2 .. 2 len + 1 with the heights cycled (the widest screens low: host time)."""
    widths = sorted({2, 3, 112, max(2, ln - 1), ln, ln + 1, 2 * ln + 1})
    heights = (36, 4, 130, 25)
    return [(heights[i % 4] if w <= 2048 else 6, w + 8) for i, w in enumerate(widths)]


@pytest.mark.parametrize("ln", [2, 3, 12, 60, 252, 1020, 1024, 1025, 2044, 4092, 4093, 16380])
def test_expanded_mags_equal_the_surface_kernel_and_the_oracle(ln):
    e = G.engine()
    names, rows = _families(ln, 5200 + ln)
    bad = []
    for f64 in (True, False):
        r = rows if f64 else rows.astype(np.float32)
        ty = "f64" if f64 else "f32"
        for H, W in _screens(ln):
            _against_surface_cells(e, r, names, H, W, f64, f"len={ln} {ty} screen {H}x{W}", bad)
        for k in (1, 3):
            _against_surface_cells(e, r[4:4 + k].copy(), names[4:4 + k], 40, 120, f64, f"len={ln} {ty} batch of {k}", bad)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("ln", [60, 1024, 1025, 4092, 4093])
def test_mags_one_row_past_each_launch_cap(ln):
    """rows_per_launch + 1 rows (the grid-stride loop of every k_surface_mags configuration takes a second turn; the cells of the batch are
    past k_mags_cells' cap as well), every row different, the families at the tail.  Every row against the oracle; the head and the whole
    second turn against pss_surface_cells (one launch per row)."""
    e = G.engine()
    per = next(r for m, r in MAGS_ROWS_PER_LAUNCH if ln <= m)
    names, fam = _families(ln, 6300 + ln)
    k = per + 1
    H, W = 36, 120
    assert k * H * W > CELLS_PER_LAUNCH or per == 2048
    if k * H * W <= CELLS_PER_LAUNCH:
        H = 130
        assert k * H * W > CELLS_PER_LAUNCH
    rng = np.random.default_rng(88 + ln)
    rows = rng.standard_normal((k, ln)) * 6.0 - 50.0
    rows[:, ln // 4] += 40.0
    rows[::5] = np.round(rows[::5])
    rows[-len(fam):] = fam
    loop = list(range(40)) + list(range(k - 160, k))
    bad = []
    for f64 in (True, False):
        _against_surface_cells(e, rows if f64 else rows.astype(np.float32), None, H, W, f64, f"len={ln} {k} rows {'f64' if f64 else 'f32'}", bad, loop)
    assert not bad, "\n".join(bad[:20])


def test_surface_argument_checks():
    e = G.engine()
    lib, h = e.lib, e.h
    p = lambda t: t.data_ptr()
    rows, rows32 = G.dev(np.zeros((2, 8))), G.dev(np.zeros((2, 8), np.float32))
    d_m, d_r, d_c = G.empty((2, 4), torch.int8), G.empty((2, 2), torch.float64), G.empty((2, 6, 12), torch.int8)
    for fn, r in ((lib.pss_surface_mags_f64, rows), (lib.pss_surface_mags, rows32)):
        assert fn(h, p(r), 2, 8, 4, p(d_m), p(d_r)) == 0
        assert fn(h, p(r), 2, 8, 4, p(d_m), None) == 0                      # d_range is optional
        assert fn(h, p(r), 2, 2, 2, p(d_m), None) == 0                      # the smallest row and width
        for args in ((p(r), 2, 1, 4, p(d_m)), (p(r), 2, 8, 1, p(d_m)), (p(r), -1, 8, 4, p(d_m)), (None, 2, 8, 4, p(d_m)), (p(r), 2, 8, 4, None)):
            assert fn(h, *args, None) == L.PSS_E_ARG, args
        assert fn(h, None, 0, 8, 4, None, None) == 0                        # an empty batch touches nothing
    assert lib.pss_mags_cells(h, p(d_m), 2, 6, 12, p(d_c)) == 0
    for args in ((p(d_m), 2, 3, 12, p(d_c)), (p(d_m), 2, 6, 9, p(d_c)), (p(d_m), -1, 6, 12, p(d_c)), (None, 2, 6, 12, p(d_c)), (p(d_m), 2, 6, 12, None)):
        assert lib.pss_mags_cells(h, *args) == L.PSS_E_ARG, args
    assert lib.pss_mags_cells(h, None, 0, 6, 12, None) == 0
    iq = G.dev(np.zeros((2, 64), np.complex64))
    db32 = G.empty((2, 64), torch.float32)
    ok = (L.MODE_AM, p(iq), 2, 64, FS, p(db32), None, None, 4, p(d_m), None, None)
    assert lib.pss_frame_pipeline_surface(h, *ok) == 0
    for i, v in ((0, 9), (0, -1), (3, 48), (3, 8), (3, 131072), (8, 1), (5, None), (9, None), (1, None), (2, -1)):
        a = list(ok)
        a[i] = v
        assert lib.pss_frame_pipeline_surface(h, *a) == L.PSS_E_ARG, (i, v)
    e.sync()


# ---- constellation masks ----------------------------------------------------------------------------------------------------------------
def _masks(e, iq2d, H, W):
    nf, n = iq2d.shape
    words = (W + 31) // 32
    d_mask = G.empty((nf, H, words), torch.int32)
    d_mask.fill_(-1)
    e.vector_masks(G.dev(iq2d) if n else G.empty((nf, 1), torch.float32), nf, n, H, W, d_mask)
    return d_mask


def _mask_grids(e, d_mask, H, W):
    nf = d_mask.shape[0]
    d_g = G.empty((nf, H, W), torch.int8)
    d_g.fill_(77)
    e.masks_cells(d_mask, nf, H, W, d_g)
    e.sync()
    return G.host(d_mask).view(np.uint32), G.host(d_g)


def test_masks_of_every_fixture_case():
    e = G.engine()
    bad = []
    for name in V.buffer_names():
        x = V.buffer(name)
        for H, W in V.SCREENS:
            mask, grid = _mask_grids(e, _masks(e, x[None], H, W), H, W)
            want = V.grid(name, H, W)
            if not np.array_equal(mask[0], V.masks_of_grid(want)):
                bad.append(f"{name} {H}x{W}: mask words differ (unused bits must be 0): {D.first_diff(F.vector_cells(mask[0], H, W), want)}")
            if not np.array_equal(grid[0], want):
                bad.append(f"{name} {H}x{W} pss_masks_cells: {D.first_diff(grid[0], want)}")
    g = np.load(V.PATH.replace("views.npz", "caller.npz"))
    for tag, H, W in (("a", 40, 120), ("b", 25, 81)):
        mask, grid = _mask_grids(e, _masks(e, g["vec_iq"][None], H, W), H, W)
        if not (np.array_equal(grid[0], g[f"vec_grid_{tag}"]) and np.array_equal(mask[0], V.masks_of_grid(g[f"vec_grid_{tag}"]))):
            bad.append(f"caller.npz vec_grid_{tag}")
    assert not bad, "\n".join(bad[:20])


def _interleaved(names, nf):
    """nf frames: the fixture buffers `names` (equal lengths) in turn, frame k scaled by a float32 factor of its own so that no two frames
    of a turn draw the same cells."""
    bufs = [V.buffer(n) for n in names]
    out = np.empty((nf, len(bufs[0])), np.complex64)
    for k in range(nf):
        out[k] = bufs[k % len(bufs)] * np.float32(0.25 + 0.125 * ((k // len(bufs)) % 23))
    return out


def _against_vector_cells(e, iq2d, H, W, tag, bad):
    """Every frame's mask and expanded grid against pss_vector_cells of that frame and the oracle."""
    nf, n = iq2d.shape
    mask, grid = _mask_grids(e, _masks(e, iq2d, H, W), H, W)
    if not np.array_equal(F.vector_cells(mask, H, W), grid):
        bad.append(f"{tag}: pss_h_masks_cells and pss_masks_cells differ")
    if not np.array_equal(mask, V.masks_of_grid(grid)):
        bad.append(f"{tag}: unused mask bits are not zero")
    d_iq, d_g = G.dev(iq2d), G.empty((H, W), torch.int8)
    report = 0
    for f in range(nf):
        want = O.vector_cells(iq2d[f], H, W)
        e.vector_cells(d_iq[f], n, H, W, d_g)
        e.sync()
        old = G.host(d_g)
        for what, w in (("the oracle", want), ("pss_vector_cells", old)):
            if not np.array_equal(grid[f], w) and report < 10:
                bad.append(f"{tag} frame {f} against {what}: {D.first_diff(grid[f], w)}")
                report += 1


BATCHES = [
    # (buffers, frames, screen)
    (("i8_mid_am_1",), 70, (24, 80)),
    (("u8o_clip_mpx_29_x3",), 1, (25, 81)),
    (("u8o_clip_mpx_29_x3",), 70, (40, 120)),
    (("i8_mid_fm_600", "i12_weak_ssb_600_x3"), 70, (25, 81)),
    (("i8_clip_ssb_1024_x3", "tone_1024", "noise_1024"), 70, (24, 80)),
    (("i8_clip_ssb_1024_x3", "tone_1024", "noise_1024"), 3, (130, 1100)),       # four masks do not fit in LDS: the workgroup kernel on short frames
    (("i16_mid_mpx_32768_x3", "noise_32768"), 1, (40, 120)),
    (("i16_mid_mpx_32768_x3", "noise_32768"), 70, (25, 81)),
    (("i8_mid_fm_40001_x3", "i8_clip_mpx_40001"), 3, (24, 80)),                 # odd length: every other frame starts on an odd sample
    (("i8_mid_fm_40001_x3", "i8_clip_mpx_40001"), 70, (40, 120)),
    (("u8o_clip_mpx_29_x3",), MASK_FRAMES_WAVE + 1, (25, 81)),                  # one frame past the wavefront kernel's cap
    (("i8_mid_fm_600", "i12_weak_ssb_600_x3"), MASK_FRAMES_WAVE + 1, (4, 10)),
    (("u8o_clip_mpx_29_x3",), MASK_FRAMES_GROUP + 1, (130, 1100)),              # ... and past the workgroup kernel's (and k_masks_cells')
]


@pytest.mark.parametrize("names,nf,screen", BATCHES, ids=lambda v: str(v).replace(" ", ""))
def test_masks_of_interleaved_batches(names, nf, screen):
    e = G.engine()
    H, W = screen
    bad = []
    _against_vector_cells(e, _interleaved(names, nf), H, W, f"{'+'.join(names)} x {nf} on {H}x{W}", bad)
    assert not bad, "\n".join(bad[:20])


def test_masks_past_the_workgroup_cap_on_full_read_buffers():
    """MASK_FRAMES_GROUP + 1 frames of 8192 samples (the shortest of the reference's read buffers: one workgroup per frame): the tail of the
    batch, the loop's second turn, frame by frame; the rest against the batch's own first turn (the frames repeat with period 46)."""
    e = G.engine()
    base = _interleaved(("i16_mid_mpx_32768_x3", "noise_32768"), 46)[:, :8192]
    nf = MASK_FRAMES_GROUP + 1
    iq = np.ascontiguousarray(np.tile(base, (nf // 46 + 1, 1))[:nf])
    H, W = 25, 81
    mask, grid = _mask_grids(e, _masks(e, iq, H, W), H, W)
    bad = []
    _against_vector_cells(e, iq[nf - 47:], H, W, "tail", bad)
    assert not bad, "\n".join(bad)
    tail, _ = _mask_grids(e, _masks(e, iq[nf - 47:], H, W), H, W)
    assert np.array_equal(mask[nf - 47:], tail)
    assert all(np.array_equal(mask[f], mask[f % 46]) for f in range(46, nf))


def test_masks_non_finite_samples_draw_nothing_and_empty_frames():
    e = G.engine()
    for name, (H, W) in (("u8o_clip_mpx_29_x3", (25, 81)), ("i8_clip_ssb_1024_x3", (24, 80)), ("i8_mid_fm_40001_x3", (40, 120))):
        x = V.buffer(name)
        n = len(x)
        clean = np.stack([x, x[::-1]])
        dirty = clean.copy()
        holes = sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n)))
        for j, i in enumerate(holes):
            dirty[:, i] = (complex(np.inf, 0.1), complex(0.1, -np.inf), complex(np.nan, 0.2), complex(0.3, np.nan), complex(np.inf, np.nan))[j % 5]
            clean[:, i] = clean[:, 2]                          # a sample that is drawn anyway
        got, _ = _mask_grids(e, _masks(e, dirty, H, W), H, W)
        want, _ = _mask_grids(e, _masks(e, clean, H, W), H, W)
        assert np.array_equal(got, want), name
        big = np.full((2, 5), 3e38 * (1 + 1j), np.complex64)            # finite samples whose coordinates overflow to infinity
        m, _ = _mask_grids(e, _masks(e, big, H, W), H, W)
        assert not m.any()
    m, g = _mask_grids(e, _masks(e, np.empty((3, 0), np.complex64), 25, 81), 25, 81)
    assert not m.any() and not g.any()                          # n = 0: empty masks


def test_vector_argument_checks():
    e = G.engine()
    lib, h = e.lib, e.h
    p = lambda t: t.data_ptr()
    iq = G.dev(np.zeros((2, 64), np.complex64))
    d_mask, d_g = G.empty((2, 5, 2), torch.int32), G.empty((2, 5, 40), torch.int8)
    assert lib.pss_vector_masks(h, p(iq), 2, 64, 5, 40, p(d_mask)) == 0
    assert lib.pss_vector_masks(h, p(iq), 2, 64, 1, 1, p(d_mask)) == 0
    big = G.empty((130 * 35,), torch.int32)
    assert lib.pss_vector_masks(h, p(iq), 1, 64, 130, 1100, p(big)) == 0          # the budget holds 130 x 1100
    for args in ((p(iq), 2, 64, 0, 40, p(d_mask)), (p(iq), 2, 64, 5, 0, p(d_mask)), (p(iq), -1, 64, 5, 40, p(d_mask)), (p(iq), 2, -1, 5, 40, p(d_mask)),
                 (None, 2, 64, 5, 40, p(d_mask)), (p(iq), 2, 64, 5, 40, None),
                 (p(iq), 2, 64, 16385, 32, p(d_mask)), (p(iq), 2, 64, 513, 1025, p(d_mask))):    # masks above 16384 words
        assert lib.pss_vector_masks(h, *args) == L.PSS_E_ARG, args
    assert lib.pss_vector_masks(h, None, 0, 64, 5, 40, None) == 0                 # an empty batch touches nothing
    assert lib.pss_masks_cells(h, p(d_mask), 2, 5, 40, p(d_g)) == 0
    for args in ((p(d_mask), 2, 0, 40, p(d_g)), (p(d_mask), 2, 5, 0, p(d_g)), (p(d_mask), -1, 5, 40, p(d_g)), (None, 2, 5, 40, p(d_g)),
                 (p(d_mask), 2, 5, 40, None)):
        assert lib.pss_masks_cells(h, *args) == L.PSS_E_ARG, args
    assert lib.pss_masks_cells(h, None, 0, 5, 40, None) == 0
    db32 = G.empty((2, 64), torch.float32)
    ok = (L.MODE_AM, p(iq), 2, 64, FS, p(db32), None, None, 5, 40, p(d_mask), None)
    assert lib.pss_frame_pipeline_vector(h, *ok) == 0
    for i, v in ((0, 9), (3, 48), (3, 8), (8, 0), (9, 0), (8, 16385), (5, None), (10, None), (1, None), (2, -1)):
        a = list(ok)
        a[i] = v
        assert lib.pss_frame_pipeline_vector(h, *a) == L.PSS_E_ARG, (i, v)
    e.sync()
    want = np.zeros((2, 5, 2), np.uint32)
    want[:, 2, 0] = 1 << 20                                      # the all-zero buffers draw the centre cell (2, 20) alone
    assert np.array_equal(G.host(d_mask).view(np.uint32), want)


# ---- the pipelines ----------------------------------------------------------------------------------------------------------------------
def _fm_frames(nf, n, seed):
    """Seeded FM-like read buffers: the generator of tests/test_gpu_bars.py."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    f = np.arange(nf).reshape(-1, 1)
    iq = (0.5 + 0.4 * (f % 3)) * np.exp(1j * (2 * np.pi * (90e3 + 7e3 * (f % 46)) * t + 0.3 * f))
    iq = iq + 0.03 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))
    return iq.astype(np.complex64)


def _pipeline_checks(e, iq, H, W, modes, tag):
    """Both pipelines in `modes` (None: the display half alone) against pss_frame_pipeline_bars on the same input and the stand-alone entry
    points -> (magnitudes, ranges, device post-processed rows) on the host."""
    nf, n = iq.shape
    m, disp_w, words = n - 4, W - 8, (W + 31) // 32
    d_iq = G.dev(iq)
    bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)
    w_mask = _masks(e, iq, H, W)
    w_mag = w_rng = w_post = None
    for mode in modes:
        n_out = 0 if mode is None else e.demod_out_len(mode, n, FS)
        run = L.MODE_NFM if mode is None else mode
        b_db32, b_db64, b_post = G.empty((nf, n), torch.float32), G.empty((nf, n), torch.float64), G.empty((nf, m), torch.float64)
        b_h, b_l = G.empty((nf, disp_w), torch.int8), G.empty((nf, disp_w), torch.int8)
        b_pcm = None if mode is None else G.empty((nf, n_out, 2), torch.int16)
        e.frame_pipeline_bars(run, d_iq, nf, n, FS, b_db32, b_db64, b_post, H - 4, disp_w, b_h, b_l, None, b_pcm)
        e.sync()
        if w_mag is None:
            w_mag, w_rng = _mags(e, G.host(b_post), disp_w)
            w_post = b_post
        for view in ("surface", "vector"):
            g_db32, g_db64, g_post = G.empty((nf, n), torch.float32), G.empty((nf, n), torch.float64), G.empty((nf, m), torch.float64)
            g_pcm = None if mode is None else G.empty((nf, n_out, 2), torch.int16)
            for t in (g_db32, g_db64, g_post):
                t.fill_(float("nan"))
            what = f"{tag} {view} mode {mode}"
            if view == "surface":
                g_mag, g_rng = G.empty((nf, disp_w), torch.int8), G.empty((nf, 2), torch.float64)
                g_mag.fill_(99)
                e.frame_pipeline_surface(run, d_iq, nf, n, FS, g_db32, g_db64, g_post, disp_w, g_mag, g_rng, g_pcm)
                e.sync()
                assert torch.equal(g_mag, w_mag), what + ": magnitudes are pss_surface_mags_f64's of d_post"
                assert torch.equal(bits(g_rng), bits(w_rng)), what + ": range"
            else:
                g_mask = G.empty((nf, H, words), torch.int32)
                g_mask.fill_(-1)
                e.frame_pipeline_vector(run, d_iq, nf, n, FS, g_db32, g_db64, g_post, H, W, g_mask, g_pcm)
                e.sync()
                assert torch.equal(g_mask, w_mask), what + ": masks are pss_vector_masks' of d_iq"
            assert torch.equal(bits(g_db32), bits(b_db32)), what + ": d_db32 bytes"
            assert torch.equal(bits(g_db64), bits(b_db64)), what + ": d_db64 bytes"
            assert torch.equal(bits(g_post), bits(b_post)), what + ": d_post bytes"
            if mode is not None:
                assert torch.equal(g_pcm, b_pcm), what + ": PCM bytes"
    # without the optional buffers (context scratch): the same results
    g_db32, g_mag, g_mask = G.empty((nf, n), torch.float32), G.empty((nf, disp_w), torch.int8), G.empty((nf, H, words), torch.int32)
    e.frame_pipeline_surface(L.MODE_NFM, d_iq, nf, n, FS, g_db32, None, None, disp_w, g_mag, None, None)
    e.frame_pipeline_vector(L.MODE_NFM, d_iq, nf, n, FS, g_db32, None, None, H, W, g_mask, None)
    e.sync()
    assert torch.equal(g_mag, w_mag) and torch.equal(g_mask, w_mask), tag + ": scratch rows"
    return G.host(w_mag), G.host(w_rng), G.host(w_post)


def _against_oracle_from_iq(e, iq, mag, rg, post_dev, H, W, tag):
    """The pin outside the library: the expanded magnitudes against oracle_lib.surface_cells of the ORACLE's post-processed rows from the
    same IQ, every cell.  Device and oracle dB values differ by about 1e-12, so the oracle's own columns must not sit on a quantisation edge:
    asserted here for every column, none excluded (value * 20 further than 1e-9 from an integer unless the value is exactly 0 or 1)."""
    taps, sos, zi = e.nfm_filters(FS)
    post = O.headline_f64(iq, FS, taps, sos, zi, 30, 1, min(O.threads_available(), 16), pcm=False)["post"]
    disp_w = W - 8
    for f, row in enumerate(post):
        lo, hi = row.min(), row.max()
        v = np.interp(np.linspace(0, len(row) - 1, disp_w), np.arange(len(row)), (row - lo) / ((hi - lo) or 1))
        edge = np.abs(v * 20 - np.rint(v * 20))
        edge[(v == 0) | (v == 1)] = 1
        assert edge.min() > 1e-9, f"{tag}: frame {f} column {int(edge.argmin())} of the oracle's row lies {edge.min():.3e} from a quantisation edge"
    want = np.stack(O.map_frames(lambda r: O.surface_cells(r, H, W), list(post)))
    got = F.surface_cells(mag, H, W)
    report = [f"{tag} frame {f} y={y} x={x}: got {got[f, y, x]} want {want[f, y, x]}; max |row difference| {np.max(np.abs(post_dev[f] - post[f])):.3e} dB"
              for f, y, x in np.argwhere(got != want)[:10]]
    assert not report, "\n".join(report)
    ex = np.stack([post.min(axis=1), post.max(axis=1)], axis=1)
    assert np.max(np.abs(rg - ex)) <= 1e-10, f"{tag}: extremes {np.max(np.abs(rg - ex)):.3e} dB from the oracle's"


def test_pipelines_on_the_golden_read_buffers(golden):
    e = G.engine()
    iq = np.ascontiguousarray(golden["caller_iq"]["iq"])
    assert iq.shape == (34, 1024)
    mag, rg, post = _pipeline_checks(e, iq, 40, 120, MODES + (None,), "caller_iq")
    _against_oracle_from_iq(e, iq, mag, rg, post, 40, 120, "caller_iq")


@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_pipelines_on_seeded_frames(n):
    e = G.engine()
    iq = _fm_frames(64, n, 500 + n)
    mag, rg, post = _pipeline_checks(e, iq, 40, 120, (L.MODE_NFM, L.MODE_AM, None) if n != 1024 else MODES + (None,), f"64 x {n}")
    _against_oracle_from_iq(e, iq, mag, rg, post, 40, 120, f"64 x {n}")


def test_pipelines_of_no_frames():
    e = G.engine()
    d = G.dev(np.full((1, 4), 7, np.int8))
    e.frame_pipeline_surface(L.MODE_NFM, None, 0, 1024, FS, None, None, None, 4, None, None, None)
    e.frame_pipeline_surface(L.MODE_WFM, None, 0, 1024, FS, None, None, None, 4, d, None, d)
    e.frame_pipeline_vector(L.MODE_NFM, None, 0, 1024, FS, None, None, None, 1, 4, None, None)
    e.frame_pipeline_vector(L.MODE_WFM, None, 0, 1024, FS, None, None, None, 1, 4, d, d)
    e.sync()
    assert (G.host(d) == 7).all()

"""Replaying a capture (include/pss.h "replaying a capture"): pss_live_frames against its host twin and NumPy, and pss_h_stream_frames
against the resident steps on the whole capture in one call — every view, with and without a squelch, dead reads inserted, ADC codes —
and against the reference's own cells (tests/golden/caller.npz, squelch.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_util as G
import oracle_lib as O
import stream_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine, PssError, h_squelch_gate

FS = S.FS
H, W = 36, 112
VIEWS = ("waterfall", "persistence", "gradient", "spectrum", "surface", "vector")
SENTINEL = -7
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyspecsdr_amd", "csrc")


# ---- pss_live_frames ---------------------------------------------------------------------------------------------------------------------
def live_on_device(frames, shift=0, want_flags=True):
    """pss_live_frames of frames [nf][n]; shift: the batch starts that many samples (8 bytes each) into its allocation."""
    e = G.engine()
    frames = np.ascontiguousarray(frames)
    nf, n = frames.shape
    flat = torch.zeros(2 * (nf * n + shift) + 4, dtype=torch.float32, device="cuda")
    d_iq = flat[2 * shift:2 * (shift + nf * n)]
    if nf:
        d_iq.copy_(torch.from_numpy(frames.view(np.float32).reshape(-1)))
    d_live = G.dev(np.full(max(nf, 1), 9, np.uint8)) if want_flags else None
    d_idx = G.dev(np.full(max(nf, 1), SENTINEL, np.int32))
    n_live = e.live_frames(d_iq, nf, n, d_live, d_idx)
    return (G.host(d_live)[:nf] if want_flags else None), G.host(d_idx)[:nf], n_live


def check_live(frames, name, shift=0):
    want, want_idx = Engine.h_live_frames(frames)
    assert np.array_equal(want, S.numpy_live(frames)), name
    live, idx, n_live = live_on_device(frames, shift)
    assert np.array_equal(live, want), f"{name}: flags differ from the host twin at frames {np.flatnonzero(live != want)[:8]}"
    assert n_live == len(want_idx) and np.array_equal(idx[:n_live], want_idx), name
    assert np.all(idx[n_live:] == SENTINEL), f"{name}: entries behind n_live were written"


def test_live_frames_cases_equal_the_host_twin():
    for name, frames in S.live_cases() + S.live_batches():
        check_live(frames, name)
        if frames.shape[1] % 2:
            check_live(frames, name + " (8 bytes off a 16-byte boundary)", shift=1)


def test_live_frames_without_flags_and_launch_source_pins():
    name, frames = S.live_batches()[4]
    _, idx, n_live = live_on_device(frames, want_flags=False)
    want = np.flatnonzero(S.numpy_live(frames))
    assert n_live == len(want) and np.array_equal(idx[:n_live], want)
    for fname, lines in S.LIVE_SOURCE.items():
        src = open(os.path.join(CSRC, fname)).read()
        for line in lines:
            assert line in src, f"{fname} no longer reads\n{line}\n-- restate tests/stream_cases.py LIVE_CAPS"


@pytest.mark.parametrize("which,n", [("boundary", S.LIVE_WAVE_MAX_N), ("boundary", S.LIVE_WAVE_MAX_N + 1), ("wave", 16), ("workgroup", S.LIVE_WAVE_MAX_N + 1),
                                     ("tiles", 1)])
def test_live_frames_one_frame_past_each_cap(which, n):
    """One frame past the wavefront / workgroup boundary (frames of 2048 and 2049 samples, the live word in the LAST tile), and one frame past
    what one pass of each capped grid covers: the grid-stride loops take a second turn."""
    nf = 9 if which == "boundary" else S.LIVE_CAPS[which] + 1
    rng = np.random.default_rng(nf + n)
    w = np.zeros((nf, 2 * n), np.uint32)
    w[:, 1::2] = 0x80000000
    alive = np.flatnonzero(rng.random(nf) < 0.5)
    w[alive, 2 * n - 1 - rng.integers(0, min(2 * n, 5), len(alive))] = 0x00000001
    w[nf - 1, 2 * n - 1] = 0x7fc00000                                    # the frame past the cap is live
    check_live(w.view(np.complex64).reshape(nf, n), f"{which} n={n} nf={nf}", shift=1 if n % 2 else 0)


def test_live_frames_seeded_batch_and_argument_errors():
    rng = np.random.default_rng(1000)
    x = (rng.standard_normal((1000, 29)) + 1j * rng.standard_normal((1000, 29))).astype(np.complex64)
    x[rng.random(1000) < 0.5] = 0
    check_live(x, "1000 x 29, half dead")
    e = G.engine()
    assert e.live_frames(None, 0, 29) == 0
    d = G.dev(x[:4])
    n_live = C.c_long(5)
    for args in ((d.data_ptr(), 4, 0), (d.data_ptr(), -1, 29), (d.data_ptr(), 2 ** 31, 29), (None, 4, 29), (d.data_ptr() + 4, 3, 29)):
        assert e.lib.pss_live_frames(e.h, args[0], args[1], args[2], None, None, C.byref(n_live)) == L.PSS_E_ARG, args
        assert b"pss_live_frames" in e.lib.pss_last_error(e.h)
    assert e.lib.pss_live_frames(e.h, d.data_ptr(), 4, 29, None, None, None) == L.PSS_E_ARG
    assert n_live.value == 5


# ---- the resident steps on a whole capture ------------------------------------------------------------------------------------------------
HALO = (np.linspace(-71.0, -64.5, 7), np.linspace(-20.25, -3.0, 7))


def resident(view, mode, frames, squelch=None, halo=None, every=3, phase=1, held_in=0.0, window=S.WINDOW):
    """The resident step of `view` on the whole capture in one call, in Engine.stream_frames' keys."""
    e = G.engine()
    nf, n = frames.shape
    v = VIEWS.index(view)
    n_out = e.demod_out_len(mode, n, FS)
    d_iq = G.dev(frames)
    d_db, d_pcm = G.empty((nf, n), torch.float32), G.empty((nf, n_out, 2), torch.int16)
    d_peak, d_avg, d_open = G.empty((nf,), torch.float64), G.empty((nf,), torch.float64), G.empty((nf,), torch.uint8)
    out = {}
    n_open, held = nf, held_in
    if v <= 2:
        nh = 0 if halo is None else len(halo[0])
        lo, hi = np.zeros(nh + nf), np.zeros(nh + nf)
        if nh:
            lo[:nh], hi[:nh] = halo
        d_lo, d_hi = G.dev(lo), G.dev(hi)
        d_a, d_b = G.empty((nf, W), torch.int8), (G.empty((nf, W), torch.int8) if v != 1 else None)
        kw = dict(n_halo=nh, window=window, display=view, disp_h=H)
        if squelch is None:
            e.frame_pipeline_cells(mode, d_iq, nf, n, FS, d_db, None, d_lo, d_hi, W, d_a, d_b, d_pcm, **kw)
        else:
            n_open, held = e.frame_pipeline_squelch(mode, d_iq, nf, n, FS, d_db, None, d_lo, d_hi, W, d_a, d_b, d_pcm, squelch, d_peak, d_avg, d_open,
                                                    every=every, phase=phase, held_in=held_in, **kw)
        e.sync()
        out.update(lines=(G.host(d_a),) if v == 1 else (G.host(d_a), G.host(d_b)), row_lo=G.host(d_lo)[nh:], row_hi=G.host(d_hi)[nh:])
    else:
        d_post = G.empty((nf, n - 4), torch.float64)
        d_range = G.empty((nf, 2), torch.float64)
        pcm_now = d_pcm if squelch is None else None
        if v == 3:
            d_h, d_l = G.empty((nf, W), torch.int8), G.empty((nf, W), torch.int8)
            e.frame_pipeline_bars(mode, d_iq, nf, n, FS, d_db, None, d_post, H, W, d_h, d_l, d_range, pcm_now)
            out.update(height=d_h, level=d_l, range=d_range)
        elif v == 4:
            d_m = G.empty((nf, W), torch.int8)
            e.frame_pipeline_surface(mode, d_iq, nf, n, FS, d_db, None, d_post, W, d_m, d_range, pcm_now)
            out.update(mag=d_m, range=d_range)
        else:
            d_mask = G.empty((nf, H + 4, (W + 8 + 31) // 32), torch.int32)
            e.frame_pipeline_vector(mode, d_iq, nf, n, FS, d_db, None, d_post, H + 4, W + 8, d_mask, pcm_now)
            out.update(mask=d_mask)
        if squelch is not None:
            d_idx = G.empty((nf,), torch.int32)
            e.row_meter(d_post, nf, n - 4, d_peak, d_avg)
            n_open, held = e.squelch_gate(d_peak, nf, squelch, every, phase, held_in, d_open, d_idx)
            e.demod_gated(mode, d_iq, nf, n, FS, d_idx, n_open, d_pcm)
        e.sync()
        out = {k: G.host(t).view(np.uint32) if k == "mask" else G.host(t) for k, t in out.items()}
    out.update(db=G.host(d_db), pcm=G.host(d_pcm)[:n_open], n_live=nf, n_open=n_open)
    if squelch is not None:
        out.update(peak=G.host(d_peak), avg=G.host(d_avg), open=G.host(d_open), held_out=held, phase_out=(phase + nf) % every)
    return out


def geometry(view):
    return (H + 4, W + 8) if view == "vector" else (H, W)


def stream(view, mode, h_in, squelch=None, halo=None, chunk=S.CHUNK, skip_dead=True, every=3, phase=1, held_in=0.0, **kw):
    dh, dw = geometry(view)
    return G.engine().stream_frames(h_in, FS, chunk, mode=mode, view=view, skip_dead=skip_dead, squelch=squelch, meter_every=every, phase=phase,
                                    peak_power=held_in, window=S.WINDOW if VIEWS.index(view) <= 2 else None, disp_h=dh, disp_w=dw,
                                    halo=halo if VIEWS.index(view) <= 2 else None, want_db=True, **kw)


def assert_same(got, want, tag):
    for k, w in want.items():
        g = got[k]
        if k == "lines":
            assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)), f"{tag}: lines"
        elif isinstance(w, np.ndarray):
            assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{tag}: {k}"      # bytes: a NaN equals itself
        else:
            assert g == w, f"{tag}: {k} {g} != {w}"


_medians = {}


def median_peak(n):
    """The median of the capture's peaks (they do not depend on the demodulation mode or on the gate's level)."""
    if n not in _medians:
        _medians[n] = float(np.median(resident("spectrum", L.MODE_NFM, S.capture(n)[0], squelch=0.0)["peak"]))
    return _medians[n]


@pytest.mark.parametrize("n,mode", [(1024, L.MODE_NFM), (1024, L.MODE_WFM), (1024, L.MODE_AM), (1024, L.MODE_USB), (256, L.MODE_NFM), (2048, L.MODE_NFM)])
def test_stream_equals_the_resident_calls(n, mode):
    frames = S.capture(n)[0]
    sq = median_peak(n)
    for view in VIEWS:
        for squelch in (None, sq):
            for halo in ((None, HALO) if VIEWS.index(view) <= 2 else (None,)):
                tag = f"n={n} mode={mode} {view} squelch={squelch} halo={halo is not None}"
                want = resident(view, mode, frames, squelch, halo)
                got = stream(view, mode, frames, squelch, halo)
                assert_same(got, want, tag)
                assert got["live"].all()
                if squelch is not None:
                    o, n_open, held = h_squelch_gate(got["peak"], squelch, 3, 1, 0.0)
                    assert np.array_equal(got["open"], o) and got["n_open"] == n_open and got["held_out"] == held, tag
                    assert got["phase_out"] == (1 + S.N_FRAMES) % 3 and 0 < n_open < S.N_FRAMES, tag


# ---- dead reads ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", VIEWS)
def test_dead_reads_neither_enter_the_history_nor_advance_the_gate(view):
    frames = S.capture(1024)[0]
    holed, live = S.insert_dead(frames, S.DEAD_AT)
    assert len(holed) == 50 and not holed[16:24].any() and not holed[31:34].any() and not holed[0].any() and not holed[-1].any()
    for mode, squelch in ((L.MODE_NFM, median_peak(1024)), (L.MODE_WFM, None)):
        want = stream(view, mode, frames, squelch)
        got = stream(view, mode, holed, squelch)
        assert np.array_equal(got["live"], live), view
        want = {k: v for k, v in want.items() if k not in ("live", "buffers")}
        assert_same(got, want, f"{view} mode={mode}: the capture with dead reads against the capture without them")


@pytest.mark.parametrize("view,squelch", [("waterfall", -40.0), ("spectrum", -40.0), ("vector", None)])
def test_a_capture_of_dead_reads_only(view, squelch):
    e = G.engine()
    zeros = np.zeros((19, 1024), np.complex64)
    zeros.view(np.float32)[:, 1::2] = -0.0
    first = stream(view, L.MODE_NFM, zeros, squelch, held_in=-12.5, phase=2)
    buf = first["buffers"]
    for k, a in buf.items():
        a.view(np.uint8)[...] = 0xa5
    got = stream(view, L.MODE_NFM, zeros, squelch, held_in=-12.5, phase=2, out=first)
    assert got["n_live"] == 0 and got["n_open"] == 0 and not got["live"].any()
    assert got["held_out"] == -12.5 and got["phase_out"] == (2 if squelch is not None else 0)
    for k, a in buf.items():
        if k != "live":
            assert (a.view(np.uint8) == 0xa5).all(), f"{k} was written although no frame is live"
    assert e.stream_frames(np.zeros((0, 1024), np.complex64), FS, 8, mode=L.MODE_NFM, view=view, disp_h=geometry(view)[0], disp_w=geometry(view)[1],
                           squelch=squelch, peak_power=3.0)["held_out"] == 3.0


@pytest.mark.parametrize("view", ["waterfall", "spectrum"])
def test_skip_dead_off_draws_the_flat_rows(view):
    holed, _ = S.insert_dead(S.capture(1024)[0], S.DEAD_AT)
    for squelch in (None, median_peak(1024)):
        want = resident(view, L.MODE_NFM, holed, squelch)
        got = stream(view, L.MODE_NFM, holed, squelch, skip_dead=False)
        assert got["live"].all() and got["n_live"] == len(holed)
        assert_same(got, want, f"{view} skip_dead=0 squelch={squelch}")
        assert (got["db"][0] == -100.0).all()


# ---- the reference's own cells ------------------------------------------------------------------------------------------------------------
def golden_capture(golden):
    iq = np.ascontiguousarray(golden["caller_iq"]["iq"])
    parts, live = [], []
    for i, f in enumerate(iq):
        parts.append(f)
        live.append(1)
        if i in (0, 11, 33):
            parts.append(np.zeros_like(f))
            live.append(0)
    return iq, np.stack(parts), np.array(live, np.uint8)


def test_reference_waterfall_and_persistence_lines_with_dead_reads(golden):
    g = golden["caller"]
    iq, holed, live = golden_capture(golden)
    e = G.engine()
    got = e.stream_frames(holed, FS, S.CHUNK, mode=L.MODE_NFM, view="waterfall", disp_h=H, disp_w=W)
    assert np.array_equal(got["live"], live) and got["n_live"] == 34
    gl, co = got["lines"]
    for i in range(34):                                     # line y = 0 of the reference's grid at frame i is the newest row
        assert np.array_equal(gl[i], g["wf_glyph"][i][0]) and np.array_equal(co[i], g["wf_colour"][i][0]), i
    got = e.stream_frames(holed, FS, S.CHUNK, mode=L.MODE_NFM, view="persistence", disp_h=H, disp_w=W)
    ys = got["lines"][0]
    for i in range(g["ps_colour"].shape[0]):
        n_hist = min(i + 1, 10)
        cp_new = int(1 + 5 * (1 - 0.7 ** (10 - (n_hist - 1))))
        assert np.all(g["ps_colour"][i][ys[i], np.arange(W)] == cp_new), i
    # every frame, the frames behind the 14 golden grids included: the resident step on the capture without the dead reads
    assert np.array_equal(ys, resident("persistence", L.MODE_NFM, iq, window=10)["lines"][0])   # PERSISTENCE_LENGTH, the stream's default


def test_reference_spectrum_cells_with_dead_reads(golden):
    iq, holed, live = golden_capture(golden)
    e = G.engine()
    got = e.stream_frames(holed, FS, S.CHUNK, mode=L.MODE_WFM, view="spectrum", disp_h=H, disp_w=W + 1)
    assert np.array_equal(got["live"], live)
    taps, sos, zi = e.nfm_filters(FS)
    post = O.headline_f64(iq, FS, taps, sos, zi, 30, 1, min(O.threads_available(), 16), pcm=False)["post"]
    res = O.map_frames(lambda row: O.spectrogram_cells(row, H, W + 1), list(post))
    gl, co = F.bars_cells(got["height"], got["level"], H)
    assert np.array_equal(gl, np.stack([r[0] for r in res])) and np.array_equal(co, np.stack([r[1] for r in res]))
    assert np.max(np.abs(got["range"] - np.array([[r[2], r[3]] for r in res]))) <= 1e-10


def test_golden_squelch_trace_with_a_dead_read_at_a_metered_position(golden):
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "squelch.npz"))
    iq = np.ascontiguousarray(golden["caller_iq"]["iq"])
    picked = [(m, o, h) for m, o, h in zip(gold["trace_meta"], gold["trace_open"], gold["trace_held"]) if int(m[1]) == 3 and 0 < o.sum() < 34]
    assert picked
    holed, live = S.insert_dead(iq, (2,))                 # frame 2 would be the first metered one (counter 3)
    for view in ("waterfall", "spectrum"):
        for meta, want_open, want_held in picked[:3]:
            got = G.engine().stream_frames(holed, FS, S.CHUNK, mode=L.MODE_NFM, view=view, squelch=float(meta[0]), meter_every=3, phase=0, peak_power=0.0,
                                           disp_h=H, disp_w=W)
            assert np.array_equal(got["live"], live)
            assert np.array_equal(got["open"], want_open) and got["n_open"] == int(want_open.sum()), (view, meta)
            assert abs(got["held_out"] - want_held[-1]) <= 1e-9, (view, meta)


# ---- ADC codes -----------------------------------------------------------------------------------------------------------------------------
SOAPY = (np.arange(256).astype(np.float32) - np.float32(127.4)) * (np.float32(1.0) / np.float32(128.0))      # SoapyRTLSDR's float32 formula


@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
def test_codes_equal_the_unpacked_capture(fmt):
    frames, codes16 = S.capture(1024)
    if fmt == "cu8":
        codes = np.clip(np.rint(frames.view(np.float32).reshape(len(frames), 1024, 2) * 128.0 + 127.4), 0, 255).astype(np.uint8)
    else:
        codes, table = np.array(codes16), None
    codes, live = S.insert_dead(codes, (3, 8, 9))
    if fmt == "cu8":
        codes[[3, 8, 9]] = 128
        table = SOAPY.copy()
        table[128] = 0.0                                  # a driver table with a representable zero: code 128 -> +0.0
    unpacked = F.unpack_iq(codes, fmt, table)
    assert np.array_equal(S.numpy_live(unpacked), live)
    for mode, view, squelch in ((L.MODE_WFM, "spectrum", median_peak(1024)), (L.MODE_NFM, "waterfall", None)):
        want = stream(view, mode, unpacked, squelch)
        got = stream(view, mode, codes, squelch, fmt=fmt, table=table)
        assert np.array_equal(got["live"], live)
        assert_same(got, {k: v for k, v in want.items() if k != "buffers"}, f"{fmt} {view}")
    if fmt == "cu8":                                      # SoapyRTLSDR's own table has no zero: the same codes are live reads
        got = stream("spectrum", L.MODE_WFM, codes, None, fmt=fmt, table=SOAPY)
        assert got["live"].all() and got["n_live"] == len(codes)
        assert_same(got, {k: v for k, v in stream("spectrum", L.MODE_WFM, F.unpack_iq(codes, fmt, SOAPY), None).items() if k != "buffers"}, "cu8 soapy")


# ---- edges and errors ----------------------------------------------------------------------------------------------------------------------
def test_chunk_sizes_and_pinned_input():
    e = G.engine()
    holed, live = S.insert_dead(S.capture(1024)[0][:11], (0, 5, 6, 13))
    want = stream("waterfall", L.MODE_NFM, holed, -30.0, chunk=4)
    pinned = e.pinned_empty(holed.shape, np.complex64)
    pinned[...] = holed
    try:
        for chunk, src in ((100, holed), (1, holed), (len(holed), holed), (4, pinned)):
            got = stream("waterfall", L.MODE_NFM, src, -30.0, chunk=chunk)
            assert_same(got, {k: v for k, v in want.items() if k != "buffers"}, f"chunk_frames={chunk}")
    finally:
        e.pinned_free(pinned)
    empty = stream("waterfall", L.MODE_NFM, np.zeros((0, 1024), np.complex64), -30.0, held_in=1.5, phase=2)
    assert empty["n_live"] == 0 and empty["n_open"] == 0 and empty["held_out"] == 1.5 and empty["phase_out"] == 2 and empty["pcm"].shape[0] == 0


def _request(**kw):
    frames = S.capture(1024)[0][:4]
    buf = {k: np.empty(s, dt) for k, (s, dt) in dict(line_a=((4, W), np.int8), line_b=((4, W), np.int8), height=((4, W), np.int8), level=((4, W), np.int8),
                                                     mag=((4, W), np.int8), mask=((4, H, 4), np.uint32), pcm=((4, 10, 2), np.int16),
                                                     peak=((4,), np.float64)).items()}
    req = dict(size=C.sizeof(L.StreamReq), container=-1, h_in=frames.ctypes.data, n_frames=4, chunk_frames=2, fs=FS, n=1024, mode=L.MODE_NFM, view=0, window=30,
               disp_h=H, disp_w=W, skip_dead=1, squelch=float("nan"))
    res = dict(size=C.sizeof(L.StreamRes), line_a=buf["line_a"].ctypes.data, line_b=buf["line_b"].ctypes.data, pcm=buf["pcm"].ctypes.data)
    drop = kw.pop("drop", ())
    for k, v in kw.items():
        if k.startswith("res_"):
            res[k[4:]] = buf[k[4:]].ctypes.data if v is True else v
        else:
            req[k] = v
    for k in drop:
        res.pop(k)
    return frames, buf, L.StreamReq(**req), L.StreamRes(**res)


@pytest.mark.parametrize("kw,text", [
    (dict(size=C.sizeof(L.StreamReq) + 8), b"size"), (dict(res_size=4), b"size"),
    (dict(view=6), b"view"), (dict(view=-1), b"view"), (dict(mode=5), b"mode"),
    (dict(view=3, res_height=True, res_level=True, n_halo=2), b"halo"),
    (dict(n=1000), b"power of two"), (dict(n=8), b"power of two"),
    (dict(view=5, res_mask=True, disp_h=130, disp_w=130 * 32), b"vector"),
    (dict(squelch=-60.0, every=-1), b"every"), (dict(squelch=-60.0, every=3, phase=3), b"phase"), (dict(squelch=-60.0, every=0, phase=1), b"phase"),
    (dict(drop=("line_b",)), b"requires"), (dict(view=1, drop=("line_a",)), b"requires"), (dict(view=3, res_height=True), b"requires"),
    (dict(view=4), b"requires"), (dict(view=5), b"requires"),
    (dict(res_peak=True), b"squelch"),
    (dict(container=7), b"container"), (dict(container=L.IQ_S16, scale=0.0), b"scale"), (dict(container=L.IQ_U8), b"table"),
    (dict(chunk_frames=0), b"chunk_frames"), (dict(n_frames=-1), b"frame count"), (dict(window=0), b"window"), (dict(view=3, res_height=True, res_level=True, disp_h=128), b"disp_h"),
])
def test_argument_errors_carry_a_text(kw, text):
    e = G.engine()
    keep = _request(**kw)
    assert e.lib.pss_h_stream_frames(e.h, C.byref(keep[2]), C.byref(keep[3])) == L.PSS_E_ARG, kw
    assert text in e.lib.pss_last_error(e.h), (kw, e.lib.pss_last_error(e.h))
    assert e.lib.pss_h_stream_frames(e.h, None, C.byref(keep[3])) == L.PSS_E_ARG
    keep = _request()
    assert e.lib.pss_h_stream_frames(e.h, C.byref(keep[2]), C.byref(keep[3])) == L.PSS_OK and keep[3].n_live == 4 and keep[3].n_open == 4


# ---- formats.replay_recording -------------------------------------------------------------------------------------------------------------
def test_replay_recording(tmp_path):
    from pyspecsdr_amd import signal_processing as SP
    frames, _ = S.insert_dead(S.capture(1024, nf=18, seed=78)[0], (4, 17))
    npy = tmp_path / "rec.npy"
    np.save(npy, np.concatenate([frames.reshape(-1), np.ones(100, np.complex64)]))       # an incomplete tail buffer is dropped
    samples = F.load_iq_recording(str(npy))
    e = SP.get_engine()
    for view, screen in (("spectrum", (40, 120)), ("surface", (40, 120)), ("vector", (25, 81)), ("waterfall", (40, 120)), ("gradient", (40, 120))):
        dh, dw = F.view_geometry(view, screen)
        assert (dh, dw) == {"spectrum": (36, 113), "surface": (36, 112), "vector": (25, 81), "waterfall": (36, 112), "gradient": (36, 110)}[view]
        got = F.replay_recording(samples, FS, mode="WFM", view=view, frame_len=1024, chunk_frames=8, squelch=-60, screen=screen, cells=True)
        want = e.stream_frames(np.ascontiguousarray(F.cut_frames(samples, 1024)), FS, 8, mode=L.MODE_WFM, view=view, squelch=-60, disp_h=dh, disp_w=dw)
        assert got["n_live"] == 18 and not got["live"][4] and not got["live"][17]
        assert_same(got, {k: v for k, v in want.items() if k != "buffers"}, view)
        if view == "spectrum":
            assert all(np.array_equal(a, b) for a, b in zip(got["cells"], F.bars_cells(got["height"], got["level"], dh)))
        elif view == "surface":
            assert np.array_equal(got["cells"], F.surface_cells(got["mag"], *screen))
        elif view == "vector":
            assert np.array_equal(got["cells"], F.vector_cells(got["mask"], *screen)) and got["cells"].any()
        else:
            assert "cells" not in got
    cu8 = np.clip(np.rint(frames.view(np.float32) * 128.0 + 128.0), 0, 255).astype(np.uint8)
    path = tmp_path / "rec.cu8"
    cu8.tofile(path)
    codes = F.load_iq_codes(str(path), "cu8")
    table = F.iq_table((L.IQ_U8, 128.0, 128.0))
    got = F.replay_recording(codes, FS, frame_len=1024, chunk_frames=8, codes_format="cu8", table=table, cells=True)
    want = e.stream_frames(np.ascontiguousarray(codes).reshape(20, 1024, 2), FS, 8, mode=L.MODE_WFM, view="spectrum", fmt="cu8", table=table, squelch=-60,
                           disp_h=36, disp_w=113)
    assert got["n_live"] == 18 and not got["live"][4]
    assert_same(got, {k: v for k, v in want.items() if k != "buffers"}, "cu8 file")
    assert all(np.array_equal(a, b) for a, b in zip(got["cells"], F.bars_cells(got["height"], got["level"], 36)))

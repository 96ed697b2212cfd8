"""The streamed calls share one context's slot table (csrc/pss_ctx.h: PssStreaming): pss_h_stream_spectrum_nfm, the pss_h_stream_display_nfm*
family and pss_h_stream_frames pick the same device buffers for the same roles, grow-only.  The other tests compare each call with its
resident twin; this one holds that the calls can follow each other on ONE Engine in any order — forwards, backwards, then with every slot
smaller than its capacity and larger than it — and still return, array for array and byte for byte, what the same call returns on a fresh
Engine of its own.  The sizes are the smallest that reach three chunks, a short last chunk, chunks of one frame, both row types, both
planes, the codes pair, the grids' tail and the gather area."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stream_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

FS = S.FS
H, W = 36, 112


def cu8(iq):
    """The capture as rtl_sdr would have written it: offset-binary bytes [nf][n][2]."""
    z = np.stack([iq.real, iq.imag], axis=-1)
    return np.clip(np.rint(z * 128.0 + 127.4), 0, 255).astype(np.uint8)


def holed(iq, at):
    out = iq.copy()
    out[list(at)] = 0
    return out


_squelch = []


def squelch_level():
    """The median peak of the capture: a gate at it opens and closes (peaks come with a squelch, so one metering call on a context of its own)."""
    if not _squelch:
        e = Engine(0)
        _squelch.append(float(np.median(e.stream_frames(S.capture(1024, 9)[0], FS, 9, mode=L.MODE_NFM, view="spectrum", squelch=0.0)["peak"])))
        e.close()
    return _squelch[0]


def spectrum_nfm(nf, n):
    def call(e):
        db, pcm = e.stream_spectrum_nfm(S.capture(n, nf)[0], FS, 2, h_db=np.empty((nf, n), np.float32))
        return {"db": db, "pcm": pcm}
    return call


def display_f32(nf, n):
    return lambda e: e.stream_display_nfm(S.capture(n, nf)[0], FS, 4, mode="waterfall", disp_h=H, disp_w=W, want_db=True)


def display_f64_grids(e):
    return e.stream_display_nfm_f64(S.capture(1024, 7)[0], FS, 3, mode="persistence", disp_h=H, disp_w=W, grids=True)


def display_codes(e):
    halo = (np.linspace(-71.0, -64.5, 29, dtype=np.float32), np.linspace(-20.25, -3.0, 29, dtype=np.float32))   # window - 1 rows
    return e.stream_display_nfm_codes(cu8(S.capture(1024, 9)[0]), FS, 4, "cu8", mode="waterfall", window=30, disp_h=H, disp_w=W, halo=halo)


def frames_vector(e):
    return e.stream_frames(holed(S.capture(1024, 9)[0], (3, 4)), FS, 2, mode=L.MODE_NFM, view="vector", skip_dead=True, squelch=squelch_level(),
                           disp_h=H + 4, disp_w=W + 8)


def frames_codes(e):
    return e.stream_frames(S.capture(1024, 9)[1], FS, 1, mode=L.MODE_WFM, view="waterfall", fmt="cs16", disp_h=H, disp_w=W)


SIX = [("stream_spectrum_nfm 7 x 1024", spectrum_nfm(7, 1024)), ("stream_display_nfm 9 x 2048", display_f32(9, 2048)),
       ("stream_display_nfm_f64 grids", display_f64_grids), ("stream_display_nfm_codes cu8", display_codes),
       ("stream_frames vector", frames_vector), ("stream_frames cs16 waterfall", frames_codes)]
SEQUENCE = SIX + SIX[::-1] + [("stream_display_nfm 5 x 1024", display_f32(5, 1024)), ("stream_spectrum_nfm 11 x 2048", spectrum_nfm(11, 2048))]


def arrays(res, prefix=""):
    """The result as (name, value) pairs; stream_frames' untrimmed "buffers" (their tails are never written) left out."""
    out = []
    for k, v in res.items():
        if k == "buffers":
            continue
        if isinstance(v, tuple):
            out += [(f"{prefix}{k}[{i}]", a) for i, a in enumerate(v)]
        else:
            out.append((prefix + k, v))
    return out


_fresh = {}


def on_a_fresh_engine(name, call):
    if name not in _fresh:
        e = Engine(0)
        try:
            _fresh[name] = arrays(call(e))
        finally:
            e.close()
    return _fresh[name]


def test_streamed_calls_share_one_context_in_any_order():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    squelch_level()
    want = [on_a_fresh_engine(name, call) for name, call in SEQUENCE]
    e = Engine(0)
    try:
        for step, ((name, call), w) in enumerate(zip(SEQUENCE, want)):
            got = arrays(call(e))
            assert [k for k, _ in got] == [k for k, _ in w], (step, name)
            for (k, g), (_, x) in zip(got, w):
                tag = f"call {step} ({name}): {k}"
                if isinstance(x, np.ndarray):
                    assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g.view(np.uint8), x.view(np.uint8)), tag   # bytes: a NaN equals itself
                else:
                    assert g == x or (g is None and x is None), tag
    finally:
        e.close()

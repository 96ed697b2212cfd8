"""The rational resampler on the device: pss_resample (k_resample) against the host twin pss_h_resample, which
tests/test_resample_golden.py pins to SciPy's resample_poly without a GPU.

Device against twin: every byte, all three row types (both run the statements of pyspecsdr_amd/csrc/pss_resample.h; the sign of a zero
and the positions of NaNs are part of the contract).  The shapes come from the launch constants restated below: the outputs of a thread,
the workgroup's threads and the grid cap, and from the lengths at which an item changes from the testing path to the plain one (hpp).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bytes_util import same, same_bytes
import resample_cases as RC
from gpu_util import engine
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine, PssError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RS_T, RS_R, RS_GRID_CAP = 256, 4, 4096
SENTINEL = -7.25


def test_launch_constants_read_as_restated():
    src = open(os.path.join(ROOT, "pyspecsdr_amd", "csrc", "pss_resample.hip")).read()
    for line in ("constexpr int RS_T = 256;", "constexpr int RS_R = 4;", "constexpr long RS_GRID_CAP = 4096;",
                 "for (long id = (long)blockIdx.x * RS_T + threadIdx.x; id < G.n_items; id += step) {",
                 "dim3((unsigned)(n_groups < RS_GRID_CAP ? n_groups : RS_GRID_CAP)), dim3(RS_T)", "G.S = p.up * ((64 + p.up - 1) / p.up);"):
        assert line in src, line


_TAPS = {}


def taps_of(up, down):
    key = RC.reduced(up, down)
    if key not in _TAPS:
        _TAPS[key] = Engine.resample_default_taps(up, down)
    return _TAPS[key]


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


def from_dev(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.complex64) if np.dtype(dtype) == np.complex64 else a


def device(x, up, down, taps, **kw):
    """x [n_rows][n_buf] through pss_resample -> [n_rows][j_end - j_begin] on the host."""
    e = engine()
    n_rows, n_buf = x.shape
    n_in = kw.get("n_in", n_buf)
    j0, j1 = kw.get("j_begin", 0), kw.get("j_end", Engine.resample_out_len(n_in, up, down))
    width = 2 if x.dtype == np.complex64 else 1
    d_x = to_dev(x) if x.size else None
    d_y = torch.full((n_rows, max(j1 - j0, 0) * width), SENTINEL, dtype=torch.float64 if x.dtype == np.float64 else torch.float32, device="cuda")
    e.resample(d_x, x.dtype, n_rows, n_buf, up, down, d_y, taps=taps, **kw)
    e.sync()
    return from_dev(d_y, x.dtype)


@pytest.mark.parametrize("up,down", RC.RATIOS)
def test_device_equals_twin_on_every_byte(up, down):
    taps = taps_of(up, down)
    hpp = RC.geometry(RC.LONG, up, down, len(taps))["hpp"]
    for n in sorted({1, 2, max(hpp, 1), 63, 64, 65, 257, RC.LONG}):
        for t, dt in enumerate(RC.DTYPES):
            x = np.stack([RC.row(7000 + 10 * r + t, n, dt) for r in range(70)])
            want = Engine.h_resample(x, up, down, taps=taps)
            for n_rows in (1, 3, 70):
                got = device(x[:n_rows], up, down, taps)
                assert same_bytes(got, want[:n_rows]), (n, np.dtype(dt).name, n_rows)


def test_special_values_reach_the_outputs_they_reach_on_the_host():
    for dt in (np.float32, np.float64):
        x = RC.special_row(dt)[None, :]
        for up, down in ((2, 3), (441, 500), (5, 1), (1, 4)):
            want = Engine.h_resample(x, up, down, taps=taps_of(up, down))
            assert np.isnan(want).any() and same_bytes(device(x, up, down, taps_of(up, down)), want), (up, down)
    # complex64 rows with inf / NaN are outside the contract with SciPy: they must run, and equal the statement
    x = RC.row(5, 300, np.complex64)[None, :].copy()
    x[0, 7], x[0, 150] = np.nan + 1j, np.inf
    assert same_bytes(device(x, 3, 2, taps_of(3, 2)), Engine.h_resample(x, 3, 2, taps=taps_of(3, 2)))


def test_one_item_past_the_grid_cap():
    """Many rows of 10 samples: rows x 15 items pass the RS_GRID_CAP x RS_T items of one pass of the grid, so the last rows are walked by the
    grid-stride loop's second pass."""
    up, down, n = 3, 2, 10
    n_rows = RS_GRID_CAP * RS_T // 15 + 100
    assert (n_rows - 100) * 15 <= RS_GRID_CAP * RS_T < n_rows * 15
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((n_rows, n)) + 1j * rng.standard_normal((n_rows, n))).astype(np.complex64)
    assert same_bytes(device(x, up, down, taps_of(up, down)), Engine.h_resample(x, up, down, taps=taps_of(up, down)))
    x64 = rng.standard_normal((65536, n))
    assert same_bytes(device(x64, 3969, 4000, taps_of(3969, 4000)), Engine.h_resample(x64, 3969, 4000, taps=taps_of(3969, 4000)))


def test_a_window_of_long_rows_from_a_halo_only_buffer_with_strides():
    e = engine()
    n_in, n_rows = 300000, 3
    for (up, down), dt in (((441, 500), np.complex64), ((147, 320), np.complex64), ((3, 2), np.float64), ((1, 4), np.float32)):
        taps = taps_of(up, down)
        n_out = Engine.resample_out_len(n_in, up, down)
        j0, j1 = n_out // 2 + 13, n_out // 2 + 13 + 6001
        lo, hi = RC.halo(n_in, up, down, len(taps), j0, j1)
        buf = np.stack([RC.row(40 + r, hi - lo, dt) for r in range(n_rows)])
        want = Engine.h_resample(buf, up, down, taps=taps, buf_index0=lo, n_in=n_in, j_begin=j0, j_end=j1)
        assert same_bytes(device(buf, up, down, taps, buf_index0=lo, n_in=n_in, j_begin=j0, j_end=j1), want)
        # strided input and output, sentinels between the rows
        xs, ys = hi - lo + 9, j1 - j0 + 5
        x = np.full((n_rows, xs), 1e30, dt)
        x[:, :hi - lo] = buf
        width = 2 if dt == np.complex64 else 1
        d_y = torch.full((n_rows, ys * width), SENTINEL, dtype=torch.float64 if dt == np.float64 else torch.float32, device="cuda")
        e.resample(to_dev(x), dt, n_rows, hi - lo, up, down, d_y, taps=taps, x_stride=xs, buf_index0=lo, n_in=n_in, j_begin=j0, j_end=j1, y_stride=ys)
        e.sync()
        y = from_dev(d_y, dt)
        assert same_bytes(y[:, :j1 - j0], want)
        assert np.all(y[:, j1 - j0:].view(np.float64 if dt == np.float64 else np.float32) == SENTINEL)
        # the ends of the same virtual rows: the testing path at both ends of a row, from buffers that hold only what is needed
        for a, b in ((0, 700), (n_out - 700, n_out)):
            lo2, hi2 = RC.halo(n_in, up, down, len(taps), a, b)
            buf2 = np.ascontiguousarray(buf[:, :hi2 - lo2])
            assert same_bytes(device(buf2, up, down, taps, buf_index0=lo2, n_in=n_in, j_begin=a, j_end=b),
                              Engine.h_resample(buf2, up, down, taps=taps, buf_index0=lo2, n_in=n_in, j_begin=a, j_end=b))


def test_goldens_through_the_device(golden):
    g = golden["resample"]
    for name, up, down, x in RC.golden_cases():
        assert RC.crc(x) == g["crc_" + name]
        assert same_bytes(device(x[None, :], up, down, taps_of(up, down))[0], g["out_" + name]), name


def test_refused_calls_leave_the_output_untouched():
    e = engine()
    n, up, down, n_rows = 41, 3, 2, 2
    taps = taps_of(up, down)
    x = np.stack([RC.row(r, n, np.float64) for r in range(n_rows)])
    d_x = to_dev(x)
    d_y = torch.full((n_rows, 70), SENTINEL, dtype=torch.float64, device="cuda")
    bad_taps = taps.copy()
    bad_taps[3] = np.nan
    good = dict(dtype=np.float64, n_rows=n_rows, n_buf=n, up=up, down=down, taps=taps, x_stride=n, buf_index0=0, n_in=n, j_begin=0, j_end=62, y_stride=70)
    bad = [("up or down outside", dict(up=0)), ("up or down outside", dict(down=4097)), ("n_taps outside", dict(taps=np.ones(98))),
           ("a tap that is not finite", dict(taps=bad_taps)), ("unknown dtype", dict(dtype=np.int16)), ("not inside the row", dict(n_buf=n + 1)),
           ("not inside the row", dict(buf_index0=1)), ("outside [0, ceil", dict(j_end=63)), ("outside [0, ceil", dict(j_begin=-1)),
           ("y_stride <", dict(y_stride=61)), ("x_stride <", dict(x_stride=n - 1)), ("needs a sample", dict(n_buf=n - 1)),
           ("needs a sample", dict(n_buf=n - 1, buf_index0=1)), ("null input", dict(x=None)), ("null output", dict(y=None)),
           ("not aligned", dict(x=d_x.data_ptr() + 4)), ("not aligned", dict(y=d_y.data_ptr() + 4))]
    for what, change in bad:
        a = dict(good, x=d_x, y=d_y)
        a.update(change)
        with pytest.raises(PssError, match="pss_resample: ") as err:
            e.resample(a["x"], a["dtype"], a["n_rows"], a["n_buf"], a["up"], a["down"], a["y"], taps=a["taps"], x_stride=a["x_stride"],
                       buf_index0=a["buf_index0"], n_in=a["n_in"], j_begin=a["j_begin"], j_end=a["j_end"], y_stride=a["y_stride"])
        assert what in str(err.value) and err.value.code == L.PSS_E_ARG, (what, str(err.value))
    # nothing to do: no rows, an empty window
    e.resample(d_x, np.float64, 0, n, up, down, d_y, taps=taps, y_stride=70)
    e.resample(d_x, np.float64, n_rows, n, up, down, d_y, taps=taps, j_begin=5, j_end=5, y_stride=70)
    e.sync()
    assert torch.all(d_y == SENTINEL)
    e.resample(d_x, np.float64, n_rows, n, up, down, d_y, taps=taps, y_stride=70)       # and the call that is fine
    e.sync()
    y = d_y.cpu().numpy()
    assert same_bytes(y[:, :62], Engine.h_resample(x, up, down, taps=taps)) and np.all(y[:, 62:] == SENTINEL)


def test_the_shim_and_the_streaming_helper_give_scipys_bytes():
    ss = pytest.importorskip("scipy.signal")
    from pyspecsdr_amd import formats as F
    from pyspecsdr_amd import signal_processing as sp
    for dt in RC.DTYPES:
        x = RC.row(61, 3001, dt)
        assert same_bytes(sp.resample_poly(x, 441, 500), ss.resample_poly(x, 441, 500))
        x2 = np.stack([RC.row(62 + r, 500, dt) for r in range(4)])
        for axis in (0, 1, -1):
            assert same_bytes(sp.resample_poly(x2, 2, 3, axis=axis), np.ascontiguousarray(ss.resample_poly(x2, 2, 3, axis=axis)))
        assert same_bytes(sp.resample_poly(x, 8, 6, window="hamming", cval=0), ss.resample_poly(x, 8, 6, window="hamming", cval=0))
        want = ss.resample_poly(x2, 160, 147, axis=1)
        for chunk in (1 << 22, 97, 13):
            assert same_bytes(F.resample_recording(x2, 160, 147, chunk_samples=chunk), want), chunk
        assert same_bytes(F.resample_recording(x, 12, 50), ss.resample_poly(x, 12, 50))


# ---- exact-rate listening: a small synthetic 2.4 MS/s capture on its 12.5 kHz grid (192 channels, 50 kS/s rows) --------------------------------
FS, SPACING, CENTRE, N_CAP, FRAME = 2.4e6, 12.5e3, 446.0e6, 460000, 4096
NFM_STATIONS = ((+25e3, 1000.0), (-37.5e3, 1700.0))      # offset, tone
AM_STATION = (+100e3, 600.0)


@pytest.fixture(scope="module")
def capture():
    rng = np.random.default_rng(2024)
    t = np.arange(N_CAP) / FS
    x = 0.002 * (rng.standard_normal(N_CAP) + 1j * rng.standard_normal(N_CAP))
    for off, tone in NFM_STATIONS:
        x += 0.2 * np.exp(1j * (2 * np.pi * off * t + (2500.0 / tone) * np.sin(2 * np.pi * tone * t)))
    off, tone = AM_STATION
    x += 0.2 * (1 + 0.5 * np.cos(2 * np.pi * tone * t)) * np.exp(2j * np.pi * off * t)
    return x.astype(np.complex64)


def audio_peak(pcm):
    """The largest bin of a 2048-sample audio spectrum (left channel, Hann window, the two DC bins dropped)."""
    a = pcm[:2048, 0].astype(np.float64)
    spec = np.abs(np.fft.rfft(a * np.hanning(len(a))))
    spec[:2] = 0
    return int(np.argmax(spec))


def compose(capture, listed, mode, exact):
    """What monitor_channels promises, done by the test: channelize_plan's rows -> (h_resample) -> cut -> demod_signal."""
    from pyspecsdr_amd import formats as F
    from pyspecsdr_amd.signal_processing import get_engine
    e = get_engine()
    ch, _, rate = F.channelize_plan(capture, FS, SPACING)
    assert rate == 50000.0
    sel = ch[F.plan_rows(FS, CENTRE, listed, SPACING)]
    if exact:
        up, down, rate = F.plan_audio(rate, mode)
        sel = Engine.h_resample(sel, up, down)
    n_frames = sel.shape[1] // FRAME
    batch = np.ascontiguousarray(sel[:, :n_frames * FRAME])
    m = {"NFM": L.MODE_NFM, "AM": L.MODE_AM}[mode]
    demod_rate = 22050.0 if mode == "AM" else rate
    n_out = e.demod_out_len(m, FRAME, demod_rate)
    d_pcm = torch.empty((len(listed) * n_frames, n_out, 2), dtype=torch.int16, device="cuda")
    e.demod_signal(m, to_dev(batch), len(listed) * n_frames, FRAME, demod_rate, d_pcm)
    e.sync()
    return d_pcm.cpu().numpy().reshape(len(listed), n_frames, n_out, 2), rate


_TWIN = {}


def oracle_pcm(capture, listed, mode):
    """The exact-rate chain on the host: the twins (h_bank's rows, h_resample) cut into frames, then the CPU oracle with the dispatcher's
    semantics (demodulate_signal corrects neither NFM nor AM buffers) and the engine's own tables."""
    import oracle_lib as O
    from pyspecsdr_amd import formats as F
    from pyspecsdr_amd.signal_processing import get_engine
    e = get_engine()
    M, D = F.plan_bank(FS, SPACING)
    assert (M, D) == (192, 48)
    if "bank" not in _TWIN:                                   # (one pass of each for the NFM and the AM case)
        _TWIN["bank"] = Engine.h_bank(capture, M, D), F.channelize_plan(capture, FS, SPACING)[0]
    twin, dev = _TWIN["bank"]
    rate = FS / D
    rows = F.plan_rows(FS, CENTRE, listed, SPACING)
    sel = twin[rows]
    assert same(dev[rows], sel)                               # the device's channels are the twin's (test_gpu_bank's criterion)
    up, down, rate = F.plan_audio(rate, mode)
    sel = Engine.h_resample(sel, up, down)
    n_frames = sel.shape[1] // FRAME
    frames = np.ascontiguousarray(sel[:, :n_frames * FRAME]).reshape(len(listed) * n_frames, FRAME)
    with np.errstate(all="ignore"):
        if mode == "NFM":
            taps, sos, zi = e.nfm_filters(rate)
            audio = [O.demod_nfm(f, rate, taps, sos, zi) for f in frames]
        else:
            sos = np.empty((5, 6))
            e.lib.pss_am_bandpass_sos(sos.ctypes.data)
            audio = [O.demod_am(f, sos) for f in frames]
    return np.stack([O.pcm16_stereo(a) for a in audio]).reshape(len(listed), n_frames, -1, 2)


def test_monitor_channels_at_the_exact_rate(capture):
    from pyspecsdr_amd import formats as F
    listed = [CENTRE + off for off, _ in NFM_STATIONS]
    pcm, rows, rate = F.monitor_channels(capture, FS, CENTRE, listed, SPACING, mode="NFM", frame_len=FRAME, exact_rate=True, chunk_samples=100000)
    assert rate == 44100.0 and rows.tolist() == [2, 189] and pcm.dtype == np.int16 and pcm.shape == (2, 2, 2048, 2)
    want, want_rate = compose(capture, listed, "NFM", True)
    assert want_rate == rate and same_bytes(pcm, want)
    assert same_bytes(pcm, oracle_pcm(capture, listed, "NFM"))          # 44 100 S/s, q = 2: against the CPU oracle, not the device's own kernels
    for k, (_, tone) in enumerate(NFM_STATIONS):
        there, not_there = round(tone * 2048 / 22050), round(tone * 2048 / 25000)
        assert there != not_there and audio_peak(pcm[k, 1]) == there, (tone, audio_peak(pcm[k, 1]))
    off, tone = AM_STATION
    pcm, rows, rate = F.monitor_channels(capture, FS, CENTRE, [CENTRE + off], SPACING, mode="AM", frame_len=FRAME, exact_rate=True)
    assert rate == 22050.0 and rows.tolist() == [8] and pcm.shape == (1, 1, FRAME, 2)
    want, want_rate = compose(capture, [CENTRE + off], "AM", True)
    assert want_rate == rate and same_bytes(pcm, want)
    assert same_bytes(pcm, oracle_pcm(capture, [CENTRE + off], "AM"))   # 22 050 S/s
    there, not_there = round(tone * 2048 / 22050), round(tone * 2048 / 50000)
    assert there != not_there and audio_peak(pcm[0, 0]) == there, audio_peak(pcm[0, 0])
    # the other two entry points take the keyword too
    words_off = [off for off, _ in NFM_STATIONS]
    p2 = F.demodulate_channels(capture, FS, words_off, 48, mode="NFM", frame_len=FRAME, exact_rate=True)
    assert p2.shape == (2, 2, 2048, 2) and [audio_peak(p2[k, 1]) for k in range(2)] == [round(t * 2048 / 22050) for _, t in NFM_STATIONS]
    with pytest.raises(TypeError):
        F.monitor_channels(capture, FS, CENTRE, listed, SPACING, nonsense=1)


def test_without_exact_rate_every_byte_is_todays(capture):
    from pyspecsdr_amd import formats as F
    listed = [CENTRE + off for off, _ in NFM_STATIONS]
    for mode, wrong in (("NFM", 25000.0), ("AM", 50000.0)):
        a = F.monitor_channels(capture, FS, CENTRE, listed, SPACING, mode=mode, frame_len=FRAME)
        b = F.monitor_channels(capture, FS, CENTRE, listed, SPACING, mode=mode, frame_len=FRAME, exact_rate=False)
        want, _ = compose(capture, listed, mode, False)
        assert a[2] == b[2] == 50000.0 and same_bytes(a[0], b[0]) and same_bytes(a[0], want) and a[1].tolist() == b[1].tolist() == [2, 189]
        assert a[0].shape[1] == (N_CAP + 47) // 48 // FRAME == 2
    tone = NFM_STATIONS[0][1]
    nfm = F.monitor_channels(capture, FS, CENTRE, listed, SPACING, mode="NFM", frame_len=FRAME)[0]
    assert audio_peak(nfm[0, 1]) == round(tone * 2048 / 25000)          # today's NFM audio plays at 25 000 Hz

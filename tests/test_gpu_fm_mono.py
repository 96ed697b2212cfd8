"""FM mono on the device: pss_decode_mono (k_mono_fwd, k_mono_bwd, k_mono_out) and pss_lfilter (k_lfilter) against the reference's goldens
(tests/golden/fm_mono.npz) and against the host twins, which tests/test_fm_mono_golden.py pins to the same goldens without a GPU.

Criterion everywhere: bit for bit, NaN matching NaN — the int16 result, the float64 value the cast sees and the float32 decimated row.
Nothing here is a tolerance: both sides run the statements of pyspecsdr_amd/csrc/pss_mono.h, and the goldens are those statements as
NumPy and SciPy executed them.

Measured on one MI355X: the whole file 5.3 s for 22 tests, the slowest 1.6 s (one frame past the backward kernel's cap: 131 073 host-twin
calls), the next 0.6 s.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fm_mono_cases as M
import length_cases as LC
from gpu_util import engine
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_constants():
    """The tile sizes, loop strides and grid caps of pyspecsdr_amd/csrc/pss_mono.hip, each beside the source line it restates."""
    return {
        "FWD_T": (256, "constexpr int FWD_T = 256;"),                  # k_mono_fwd: a lane's second output of a tile starts here
        "FWD_TILE": (512, "constexpr int FWD_TILE = 512;"),            # outputs of a tile: a frame's second tile starts here
        "FWD_GRID_CAP": (16384, "constexpr long FWD_GRID_CAP = 16384;"),   # tiles of one pass of the grid
        "BWD_F": (64, "constexpr int BWD_F = 64;"),                    # k_mono_bwd: frames of a workgroup, and its lanes' stride along a row
        "BWD_CH": (32, "constexpr int BWD_CH = 32;"),                  # outputs of a staged chunk
        "BWD_GRID_CAP": (2048, "constexpr long BWD_GRID_CAP = 2048;"),     # workgroups (of BWD_F frames) of one pass of the grid
        "OUT_T": (256, "constexpr int OUT_T = 256;"),                  # k_mono_out: outputs of a tile
        "OUT_GRID_CAP": (16384, "constexpr long OUT_GRID_CAP = 16384;"),   # tiles of one pass of the grid
        "LF_T": (64, "constexpr int LF_T = 64;"),                      # k_lfilter: rows of a workgroup
        "LF_GRID_CAP": (1024, "constexpr long LF_GRID_CAP = 1024;"),
    }


K = {k: v[0] for k, v in launch_constants().items()}


def n_for(n_out):
    """The shortest frame with n_out outputs: n - 1 = 6 (n_out - 1) + 1."""
    return 6 * (n_out - 1) + 2


# n_out one short of, at and one past every tile size and stride above (and NumPy's 128-element summation leaf, pss_npsum.h)
EDGE_N_OUT = sorted({e + d for e in (K["BWD_CH"], K["BWD_F"], 128, K["FWD_T"], K["OUT_T"], K["FWD_TILE"]) for d in (-1, 0, 1)})
SWEEP_LENGTHS = [2, 3, 7, 8, 13, 14, 67, 127, 128, 133, 134, 1024, 2049, 8193] + [n_for(o) for o in EDGE_N_OUT] + [n_for(K["FWD_TILE"] + 1) + 5]
BATCHES = [1, 3, 65]


def test_launch_constants_read_as_restated():
    src = open(os.path.join(ROOT, "pyspecsdr_amd", "csrc", "pss_mono.hip")).read()
    for name, (_, line) in launch_constants().items():
        assert line in src, f"pss_mono.hip no longer reads `{line}`: restate {name} here"
    for line in ("for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {", "for (int jr = tid; jr < cnt; jr += FWD_T)",
                 "for (long g = blockIdx.x; g < n_groups; g += gridDim.x) {",
                 "for (long r = (long)blockIdx.x * LF_T + threadIdx.x; r < n_rows; r += (long)gridDim.x * LF_T)",
                 "dim3((unsigned)(n_tiles < FWD_GRID_CAP ? n_tiles : FWD_GRID_CAP)), dim3(FWD_T)",
                 "dim3((unsigned)(n_groups < BWD_GRID_CAP ? n_groups : BWD_GRID_CAP)), dim3(BWD_F)",
                 "dim3((unsigned)(n_out_tiles < OUT_GRID_CAP ? n_out_tiles : OUT_GRID_CAP)), dim3(OUT_T)",
                 "const dim3 grid((unsigned)(blocks < LF_GRID_CAP ? blocks : LF_GRID_CAP));"):
        assert line in src, line
    assert [L.load().pss_decode_mono_len(n_for(o)) for o in EDGE_N_OUT] == EDGE_N_OUT


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def device_mono(frames, fs, want=("pcm", "audio", "dec"), offset=True):
    """frames complex64 [nf][n] through pss_decode_mono -> dict of host arrays.  offset: d_iq starts one complex sample (8 bytes) into its
    allocation, so no load of the kernel may assume more than a sample's alignment."""
    e = engine()
    frames = np.ascontiguousarray(frames, np.complex64)
    nf, n = frames.shape
    n_out = e.decode_mono_len(n)
    flat = np.zeros(2 * nf * n + 2, np.float32)
    flat[2 if offset else 0:][:2 * nf * n] = frames.view(np.float32).reshape(-1)
    d_all = torch.from_numpy(flat).cuda()
    d_iq = d_all[2:] if offset else d_all
    assert d_iq.data_ptr() % 16 == (8 if offset else 0)
    out = {"pcm": torch.full((nf, n_out), 0x5a5a, dtype=torch.int16, device="cuda"),
           "audio": torch.full((nf, n_out), -7.0, dtype=torch.float64, device="cuda"),
           "dec": torch.full((nf, n_out), -7.0, dtype=torch.float32, device="cuda")}
    e.decode_mono(d_iq, nf, n, fs, *(out[k] if k in want else None for k in ("pcm", "audio", "dec")))
    e.sync()
    return {k: out[k].cpu().numpy() for k in want}


def host_mono(frames, fs):
    """The host twin on every frame, through one preallocated output set (the raw ctypes call: 131 073 frames take about a second)."""
    lib = L.load()
    frames = np.ascontiguousarray(frames, np.complex64)
    nf, n = frames.shape
    n_out = lib.pss_decode_mono_len(n)
    pcm, audio, dec = np.empty((nf, n_out), np.int16), np.empty((nf, n_out), np.float64), np.empty((nf, n_out), np.float32)
    pi, pp, pa, pd = frames.ctypes.data, pcm.ctypes.data, audio.ctypes.data, dec.ctypes.data
    fn, fs = lib.pss_h_decode_mono, float(fs)
    for f in range(nf):
        if fn(pi + 8 * n * f, n, fs, pp + 2 * n_out * f, pa + 8 * n_out * f, pd + 4 * n_out * f) != 0:
            raise AssertionError("pss_h_decode_mono failed")
    return {"pcm": pcm, "audio": audio, "dec": dec}


def differing(got, want):
    """Frames of a batch whose rows differ in any bit, per output."""
    bad = {}
    for k in got:
        rows = [f for f in range(len(got[k])) if not same_bits(got[k][f], want[k][f])]
        if rows:
            bad[k] = rows[:8]
    return bad


@pytest.fixture(scope="module")
def g(golden):
    return golden["fm_mono"]


def _golden_ok(g, key, got, long):
    if not long:
        return same_bits(got, g[key])
    return (np.array_equal(M.digest(got), g[key + "_digest"]) and same_bits(got[:M.EDGE], g[key + "_head"])
            and same_bits(got[-M.EDGE:], g[key + "_tail"]))


@pytest.mark.parametrize("fs", M.RATES)
def test_every_golden_case_on_the_device(g, fs):
    bad = []
    cases = [(str(n), M.frame(n), n >= M.LONG) for n in M.LENGTHS] + [("sp_" + s, g["in_sp_" + s], False) for s in M.SPECIALS]
    for c, x, long in cases:
        got = device_mono(x[None, :], fs)
        for name in ("pcm", "audio", "dec"):
            if not _golden_ok(g, f"{name}_{c}_{int(fs)}", got[name][0], long):
                bad.append((c, name))
    assert not bad, bad
    k = f"sp_wrap_{int(2.4e6)}"
    assert np.abs(g[f"audio_{k}"]).max() >= 32768       # the wrap case went through the comparison above


@pytest.mark.parametrize("nf", BATCHES)
def test_device_equals_host_twin_over_lengths_and_batches(nf):
    bad = []
    for n in SWEEP_LENGTHS:
        frames = M.frames(nf, n, seed=nf)
        assert LC.repeats(frames) == 0
        d = differing(device_mono(frames, 2.4e6), host_mono(frames, 2.4e6))
        if d:
            bad.append((n, d))
    assert not bad, bad


@pytest.mark.parametrize("fs", [250e3, 1.024e6])
def test_device_equals_host_twin_at_the_other_rates(fs):
    bad = []
    for n in (8, 134, 1024, n_for(K["FWD_TILE"] + 1)):
        frames = M.frames(5, n, seed=9)
        d = differing(device_mono(frames, fs), host_mono(frames, fs))
        if d:
            bad.append((n, d))
    assert not bad, bad


def test_rows_longer_than_numpys_summation_chunk():
    """n_out past 8192 and 16 384: np.add.reduce adds 8192-element chunks in order, and k_mono_bwd's streamed mean crosses them."""
    bad = []
    for n_out in (8191, 8193, 16384 + 7):
        frames = M.frames(3, n_for(n_out), seed=10)
        d = differing(device_mono(frames, 2.4e6), host_mono(frames, 2.4e6))
        if d:
            bad.append((n_out, d))
    assert not bad, bad


def test_one_frame_past_the_forward_and_output_caps():
    """n_out = 2: one tile a frame in k_mono_fwd and in k_mono_out, one tile more than either grid's cap — the first workgroup of both
    walks its grid-stride loop a second time."""
    assert K["FWD_GRID_CAP"] == K["OUT_GRID_CAP"]
    nf, n = K["FWD_GRID_CAP"] + 1, 8
    frames = M.frames(nf, n, seed=3)
    assert LC.repeats(frames) == 0
    assert not differing(device_mono(frames, 2.4e6), host_mono(frames, 2.4e6))


def test_one_frame_past_the_forward_cap_with_two_tiles_a_frame():
    tiles = 2
    nf, n = K["FWD_GRID_CAP"] // tiles + 1, n_for(K["FWD_TILE"] + 1)
    base = M.frames(64, n, seed=4)                          # 64 drawn frames, each copy scaled by its own factor: every frame different
    frames = base[np.arange(nf) % 64] * (1 + np.arange(nf, dtype=np.float32) / 65536)[:, None]
    assert frames.dtype == np.complex64
    got = device_mono(frames, 2.4e6, want=("dec", "pcm"))  # k_mono_out: three tiles a frame, past its cap as well
    pick = [0, 1, nf // 2, nf - 2, nf - 1]                 # the host twin on the frames either side of the wrap-around
    want = host_mono(frames[pick], 2.4e6)
    assert same_bits(got["dec"][pick], want["dec"]) and same_bits(got["pcm"][pick], want["pcm"])
    # every other frame: finite and not the fill value (a skipped tile would leave -7 / 0x5a5a)
    assert np.isfinite(got["dec"]).all() and not (got["dec"] == -7.0).any() and not (got["pcm"] == 0x5a5a).all(axis=1).any()


def test_one_frame_past_the_backward_cap():
    nf, n = K["BWD_GRID_CAP"] * K["BWD_F"] + 1, 8
    frames = M.frames(nf, n, seed=5)
    assert LC.repeats(frames) == 0
    assert not differing(device_mono(frames, 2.4e6), host_mono(frames, 2.4e6))


def test_special_frames_between_ordinary_ones(g):
    n = M.SPECIAL_N
    ordinary = M.frames(6, n, seed=6)
    rows = [ordinary[0], g["in_sp_zeros"], ordinary[1], g["in_sp_nan"], ordinary[2], g["in_sp_negzero"], g["in_sp_tiny"], ordinary[3],
            g["in_sp_wrap"], ordinary[4]]
    frames = np.stack(rows)
    got, want = device_mono(frames, 2.4e6), host_mono(frames, 2.4e6)
    assert not differing(got, want)
    assert not got["pcm"][1].any() and not got["pcm"][3].any() and np.isnan(got["audio"][3]).all()
    assert same_bits(got["pcm"][8], g[f"pcm_sp_wrap_{int(2.4e6)}"]) and np.abs(got["audio"][8]).max() >= 32768
    assert np.isfinite(got["audio"][[0, 2, 4, 7, 9]]).all()        # a NaN frame does not leak into its neighbours


def test_optional_outputs_and_empty_calls():
    frames = M.frames(3, 134, seed=7)
    full = device_mono(frames, 2.4e6)
    assert same_bits(device_mono(frames, 2.4e6, want=("pcm",))["pcm"], full["pcm"])
    assert same_bits(device_mono(frames, 2.4e6, want=("audio",), offset=False)["audio"], full["audio"])
    assert same_bits(device_mono(frames, 2.4e6, want=("dec",))["dec"], full["dec"])
    e = engine()
    d = torch.zeros(16, dtype=torch.float32, device="cuda")
    guard = torch.full((4,), 0x1234, dtype=torch.int16, device="cuda")
    for n in (0, 1):
        e.decode_mono(d, 4, n, 2.4e6, guard)               # succeeds, writes nothing
    e.decode_mono(d, 0, 8, 2.4e6, guard)
    e.sync()
    assert (guard.cpu().numpy() == 0x1234).all()
    with pytest.raises(Exception):
        e.decode_mono(d, 1, 8, 2.4e6)                      # no output at all
    with pytest.raises(Exception):
        e.decode_mono(d[1:], 1, 4, 2.4e6, guard)           # 4-byte aligned


def test_shim_decode_mono_equals_the_golden(g):
    from pyspecsdr_amd import signal_processing as sp
    for n in (2, 134, 1024):
        for fs in (250e3, 2.4e6):
            got = sp.decode_mono(M.frame(n), fs)
            assert got.dtype == np.int16 and same_bits(got, g[f"pcm_{n}_{int(fs)}"]), (n, fs)
    assert same_bits(sp.decode_mono(M.frame(1024), 2400000), g[f"pcm_1024_{2400000}"])     # the reference's signature says int
    for n in (0, 1):
        out = sp.decode_mono(np.zeros(n, np.complex64), 2.4e6)
        assert out.shape == (0,) and out.dtype == np.int16


def test_chunked_host_batch_equals_the_resident_call():
    e = engine()
    frames = M.frames(11, 1024, seed=8)
    want = device_mono(frames, 1.024e6, want=("pcm",))["pcm"]
    for chunk in (1, 4, 11, 4096):
        assert same_bits(e.h_decode_mono_batch(frames, 1.024e6, chunk_frames=chunk), want), chunk


def test_recording_from_cu8_codes_equals_the_complex64_call():
    from pyspecsdr_amd import formats
    rng = np.random.default_rng(21)
    frame_len, nf = 1024, 5
    n = frame_len * nf + 100                                    # an incomplete tail buffer is dropped
    ph = np.cumsum(rng.standard_normal(n) * 0.4)
    codes = np.clip(np.rint(127.4 + 100 * np.stack([np.cos(ph), np.sin(ph)], axis=1) + rng.standard_normal((n, 2))), 0, 255).astype(np.uint8)
    iq = formats.unpack_iq(codes, "cu8")
    want = formats.decode_mono_recording(iq, 2.4e6, frame_len=frame_len)
    assert want.shape == (nf, 171) and want.dtype == np.int16 and want.any()
    assert same_bits(formats.decode_mono_recording(codes, 2.4e6, frame_len=frame_len, codes_format="cu8"), want)
    assert same_bits(formats.decode_mono_recording(codes, 2.4e6, frame_len=frame_len, codes_format="cu8", chunk_frames=2), want)
    assert same_bits(want, host_mono(iq[:nf * frame_len].reshape(nf, frame_len), 2.4e6)["pcm"])


def test_shim_lowpass_filter_equals_the_goldens(g):
    from pyspecsdr_amd import signal_processing as sp
    bad = []
    for p, (cutoff, fs, order) in enumerate(M.LP_PARAMS):
        for dt in ("float32", "float64"):
            for n in M.LP_LENGTHS:
                x = M.lp_row(n, dt)
                y = sp.lowpass_filter(x, cutoff, fs, order) if p else sp.lowpass_filter(x)
                if y.dtype != np.float64 or not _golden_ok(g, f"lp_out_{dt}_{n}_{p}", y, n >= M.LP_LONG):
                    bad.append((p, dt, n))
    assert not bad, bad
    rows = np.stack([M.lp_row(5000, "float32"), M.lp_row(5000, "float32")[::-1]])
    y = sp.lowpass_filter(rows)
    assert y.shape == rows.shape and same_bits(y[0], g["lp_out_float32_5000_0"]) and same_bits(y[1], sp.lowpass_filter(rows[1]))
    assert sp.lowpass_filter(np.zeros(0)).shape == (0,)


@pytest.mark.parametrize("nr", [1, 3, K["LF_GRID_CAP"] * K["LF_T"] + 1])
def test_device_lfilter_equals_host_twin(g, nr):
    e = engine()
    n = 5 if nr > 3 else 700
    x = M.lp_rows(nr, n, seed=nr)
    for p in range(len(M.LP_PARAMS)):
        b, a = g[f"lp_b_{p}"], g[f"lp_a_{p}"]
        d_x = torch.from_numpy(x).cuda()
        d_y = torch.full_like(d_x, -7.0)
        e.lfilter(d_x, nr, n, b, a, d_y)
        e.sync()
        assert same_bits(d_y.cpu().numpy(), Engine.h_lfilter(x, b, a)), (nr, p)
    # every coefficient count has a kernel of its own
    rng = np.random.default_rng(5)
    x = M.lp_rows(3, 64, seed=1)
    for nc in range(2, 10):
        b, a = rng.standard_normal(nc), np.concatenate([[1.5], 0.1 * rng.standard_normal(nc - 1)])
        d_x = torch.from_numpy(x).cuda()
        d_y = torch.empty_like(d_x)
        e.lfilter(d_x, 3, 64, b, a, d_y)
        e.sync()
        assert same_bits(d_y.cpu().numpy(), Engine.h_lfilter(x, b, a)), nc

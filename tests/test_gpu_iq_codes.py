"""-m gpu: read buffers as ADC codes (include/pss.h "ADC codes").  The device widening against the host restatement, word for word, at
every alignment of input and output and past 2^31 words; the streamed display call and the batch demodulator on codes against the same
calls on the complex64 buffers the codes stand for.  Every comparison is equality of bits or bytes."""
import numpy as np
import pytest
import torch

import adc_cases as A
from gpu_util import engine
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F

pytestmark = pytest.mark.gpu

FS = A.FS
GRID_OF = {"cu8": "u8o", "cs8": "i8", "cs12": "i12", "cs16": "i16"}
DTYPE_OF = {"cu8": np.uint8, "cs8": np.int8, "cs12": np.int16, "cs16": np.int16}
SENTINEL = 0x5EA7BEEF   # an int32 word no table entry and no quotient below equals


def codes_of(case, fmt):
    """The integer codes a '+'-signed ADC case was built from (tests/test_iq_codes.py checks that they reproduce the case bit for bit)."""
    scale, lo, hi, off = A.GRIDS[GRID_OF[fmt]]
    w = case.iq.view(np.float32)
    assert not np.any((w == 0) & np.signbit(w)), case.name
    code = np.rint(w.astype(np.float64) * scale + off)
    assert code.min() >= lo and code.max() <= hi
    return code.astype(DTYPE_OF[fmt]).reshape(-1, 2)


def capture(fmt, names, n_frames):
    """(codes [n_frames, n, 2], iq complex64 [n_frames, n], case names per frame): the named cases cycled."""
    picked = [A.by_name(names[k % len(names)]) for k in range(n_frames)]
    codes = np.ascontiguousarray(np.stack([codes_of(c, fmt) for c in picked]))
    iq = np.ascontiguousarray(np.stack([c.iq for c in picked]))
    assert A.same_bits(F.unpack_iq(codes, fmt), iq)
    return codes, iq, [c.name for c in picked]


# ---- 1. pss_unpack_iq against pss_h_unpack_iq ---------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65537)
# (label, fmt triple, code type): both 8-bit containers on a random table; int16 on a power-of-two scale (the multiply path) and on one
# that is none (the IEEE division)
VARIANTS = [("u8", (L.IQ_U8, 1.0, 0.0), np.uint8), ("s8", (L.IQ_S8, 1.0, 0.0), np.int8), ("s16_32768", (L.IQ_S16, 32768.0, 0.0), np.int16),
            ("s16_1000", (L.IQ_S16, 1000.0, 0.0), np.int16)]


def random_table(seed):
    """256 distinct float32 words in no order: an index that is off by anything shows."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(256).astype(np.float32)
    bits = t.view(np.uint32).copy()
    bits[17], bits[201] = 0x7FC00123, 0x80000000          # a NaN with a payload, and -0: no special cases
    assert len(set(bits.tolist())) == 256 and SENTINEL & 0xFFFFFFFF not in set(bits.tolist())
    return bits.view(np.float32)


@pytest.mark.parametrize("label,fmt,dt", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_unpack_matches_the_host_restatement_at_every_alignment(label, fmt, dt):
    e = engine()
    rng = np.random.default_rng(11)
    info = np.iinfo(dt)
    every = np.arange(info.min, info.max + 1).astype(dt)
    n_max = max(SIZES)
    words = np.concatenate([rng.permutation(every) for _ in range(-(-2 * n_max // len(every)))])[:2 * n_max]
    assert len(np.unique(words)) == len(every)            # every code of the container is in the buffer
    codes = np.ascontiguousarray(words.reshape(n_max, 2))
    table = random_table(3) if dt != np.int16 else None
    want = F.unpack_iq(codes, fmt, table=table)
    if dt == np.int16:
        assert A.same_bits(want.view(np.float32), words.astype(np.float32) / np.float32(fmt[1]))
    d_want = torch.from_numpy(want.view(np.int32)).cuda()
    unit = np.dtype(dt).itemsize
    raw = torch.from_numpy(codes.view(np.uint8).reshape(-1).copy())
    d_buf = torch.zeros(raw.numel() + 16, dtype=torch.uint8, device="cuda")
    assert d_buf.data_ptr() % 16 == 0
    pad = 4                                               # sentinel samples behind the output range
    bad = []
    for in_off in range(0, 16, unit):
        d_buf[in_off:in_off + raw.numel()] = raw.cuda()
        for n in SIZES:
            for out_off in (0, 1, 3):
                d_out = torch.full((2 * (out_off + n + pad),), SENTINEL, dtype=torch.int32, device="cuda")
                assert d_out.data_ptr() % 16 == 0
                e.unpack_iq(d_buf.data_ptr() + in_off, n, d_out.data_ptr() + 8 * out_off, fmt, table)
                lo, hi = 2 * out_off, 2 * (out_off + n)
                ok = torch.equal(d_out[lo:hi], d_want[:2 * n]) and bool((d_out[:lo] == SENTINEL).all()) and bool((d_out[hi:] == SENTINEL).all())
                if not ok:
                    bad.append((in_off, n, out_off))
    assert not bad, f"{len(bad)} of {len(range(0, 16, unit)) * len(SIZES) * 3} (input offset, n_samples, output offset) differ: {bad[:12]}"


def test_unpack_argument_errors():
    e = engine()
    lib = e.lib
    d_c = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_o = torch.zeros(64, dtype=torch.float32, device="cuda")
    table = np.zeros(256, np.float32)
    tp = table.ctypes.data

    def err(r, text):
        assert r == L.PSS_E_ARG
        assert text in lib.pss_last_error(e.h), lib.pss_last_error(e.h)

    err(lib.pss_unpack_iq(e.h, 7, d_c.data_ptr(), 4, 1.0, tp, d_o.data_ptr()), b"container")
    err(lib.pss_unpack_iq(e.h, L.IQ_U8, d_c.data_ptr(), 4, 1.0, None, d_o.data_ptr()), b"table")
    err(lib.pss_unpack_iq(e.h, L.IQ_S16, d_c.data_ptr(), 4, 2048.0, tp, d_o.data_ptr()), b"NULL")
    err(lib.pss_unpack_iq(e.h, L.IQ_S16, d_c.data_ptr(), 4, 0.0, None, d_o.data_ptr()), b"scale")
    err(lib.pss_unpack_iq(e.h, L.IQ_S16, d_c.data_ptr() + 1, 4, 2048.0, None, d_o.data_ptr()), b"2-byte")
    err(lib.pss_unpack_iq(e.h, L.IQ_U8, d_c.data_ptr(), 4, 0.0, tp, d_o.data_ptr() + 4), b"8-byte")
    err(lib.pss_unpack_iq(e.h, L.IQ_U8, d_c.data_ptr(), -1, 0.0, tp, d_o.data_ptr()), b"n_samples")
    err(lib.pss_unpack_iq(e.h, L.IQ_U8, None, 4, 0.0, tp, d_o.data_ptr()), b"null")
    assert lib.pss_unpack_iq(e.h, L.IQ_U8, None, 0, 0.0, tp, None) == 0
    c8 = np.zeros((8, 1024, 2), np.uint8)
    pcm = np.empty((8, 10, 2), np.int16)
    err(lib.pss_h_demodulate_batch_codes(e.h, 5, 0.0, tp, L.MODE_NFM, c8.ctypes.data, 8, 1024, FS, 4, pcm.ctypes.data), b"container")
    err(lib.pss_h_demodulate_batch_codes(e.h, L.IQ_U8, 0.0, None, L.MODE_NFM, c8.ctypes.data, 8, 1024, FS, 4, pcm.ctypes.data), b"table")
    la = np.empty((8, 112), np.int8)
    # a negative container is unknown like any other: it must not select the complex64 path and read 8 B/sample from the code buffer
    err(lib.pss_h_demodulate_batch_codes(e.h, -1, 0.0, tp, L.MODE_NFM, c8.ctypes.data, 8, 1024, FS, 4, pcm.ctypes.data), b"container")
    err(lib.pss_h_stream_display_nfm_codes(e.h, -1, 0.0, tp, c8.ctypes.data, 4, 1024, FS, 4, 1, 5, 36, 112, None, None, 0, la.ctypes.data,
                                           None, pcm.ctypes.data, None, None, None), b"container")
    err(lib.pss_unpack_iq(e.h, -1, d_c.data_ptr(), 4, 1.0, tp, d_o.data_ptr()), b"container")
    err(lib.pss_h_stream_display_nfm_codes(e.h, L.IQ_S16, -2.0, None, c8.ctypes.data, 4, 1024, FS, 4, 1, 5, 36, 112, None, None, 0, la.ctypes.data,
                                           None, pcm.ctypes.data, None, None, None), b"scale")
    err(lib.pss_h_stream_display_nfm_codes_f64(e.h, -1, 0.0, tp, c8.ctypes.data, 8, 1024, FS, 4, 1, 5, 36, 112, None, None, 0, la.ctypes.data, None,
                                               pcm.ctypes.data, None, None, None, None, None), b"container")
    for dt in (np.uint8, np.int8, np.int16):             # pinned_empty serves the code types
        p = e.pinned_empty((3, 5, 2), dt)
        assert p.dtype == dt and p.shape == (3, 5, 2)
        e.pinned_free(p)


# ---- 2. one buffer whose word index passes 2^31 and whose byte offset passes 2^32 -----------------------------------------------------------
def test_unpack_past_2_31_words():
    e = engine()
    n = (1 << 30) + 3
    try:
        d_codes = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
        d_out = torch.empty(2 * n + 8, dtype=torch.int32, device="cuda")
    except torch.cuda.OutOfMemoryError as ex:             # 2 GiB of codes + 8 GiB of float32
        pytest.skip(f"no room for a 2 GiB code buffer and its 8 GiB of complex64 on this device: {ex}")
    step = 1 << 28
    gen = torch.Generator(device="cuda").manual_seed(7)
    for s in range(0, 2 * n, step):                       # codes made on the device, a piece at a time
        m = min(step, 2 * n - s)
        d_codes[s:s + m] = torch.randint(0, 256, (m,), dtype=torch.uint8, device="cuda", generator=gen)
    d_out[2 * n:] = SENTINEL
    table = random_table(9)
    d_table = torch.from_numpy(table.view(np.int32)).cuda()
    e.unpack_iq(d_codes, n, d_out, "cu8", table)
    half = 32768
    windows = [(0, 2 * half), (n - 2 * half, n)] + [(c - half, min(c + half, n)) for c in (1 << 28, 1 << 29, 1 << 30)]   # the last one ends with the buffer, 3 samples past 2^30
    bad = []
    for a, b in windows:
        want = d_table[d_codes[2 * a:2 * b].long()]
        if not torch.equal(d_out[2 * a:2 * b], want):
            bad.append((a, b, int((d_out[2 * a:2 * b] != want).sum())))
    tail_ok = bool((d_out[2 * n:] == SENTINEL).all())
    del d_codes, d_out
    torch.cuda.empty_cache()
    assert not bad, f"windows (first sample, end, differing words): {bad}"
    assert tail_ok, "words behind the output range were written"


# ---- 3. the streamed display call on codes ------------------------------------------------------------------------------------------------
STREAM_CASES = {
    "cs8": ["i8_floor_mpx_1024", "i8_floor_fm_1024", "i8_mid_ssb_1024", "i8_clip_mpx_1024", "dead_zero_1024"],
    "cu8": ["u8o_weak_am_1024", "u8o_mid_mpx_1024"],
    "cs12": ["i12_mid_fm_1024"],
    "cs16": ["i16_weak_fm_1024"],
}
SHORT_CASES = {"cu8": ["u8o_clip_mpx_29"], "cs8": ["i8_clip_fm_29", "dead_first_zero_29", "dead_const_eq_29"]}
_GOLDEN = None


def golden_pcm(name):
    global _GOLDEN
    if _GOLDEN is None:
        import os
        _GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adc.npz"))
    key = "nfm_pcm_" + name
    return _GOLDEN[key] if key in _GOLDEN.files else None


def same_results(got, want):
    """Every array of two result dicts byte-equal (tuples of arrays element by element; None only against None)."""
    assert set(got) == set(want)
    for k in want:
        a, b = got[k], want[k]
        a, b = (a, b) if isinstance(b, tuple) else ((a,), (b,))
        assert len(a) == len(b), k
        for x, y in zip(a, b):
            assert (x is None) == (y is None), k
            if y is not None:
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{k}: the code stream differs from the complex64 stream"


def check_golden_pcm(res, names):
    n_golden = 0
    for f, name in enumerate(names):
        g = golden_pcm(name)
        if g is not None:
            assert np.array_equal(res["pcm"][f], g), f"frame {f} ({name}): PCM differs from tests/golden/adc.npz"
            n_golden += 1
    return n_golden


@pytest.mark.parametrize("mode", ["waterfall", "persistence"])
@pytest.mark.parametrize("fmt", sorted(STREAM_CASES))
def test_stream_display_on_codes_equals_the_complex64_stream(fmt, mode):
    e = engine()
    codes, iq, names = capture(fmt, STREAM_CASES[fmt], 11)
    kw = dict(mode=mode, window=5, disp_h=36, disp_w=112, want_db=True)     # chunk_frames 4: three chunks, the last partial, a buffer set reused
    halo32 = (np.array([-71.5, -80.25, -64.0], np.float32), np.array([-12.0, -3.5, -20.75], np.float32))
    halo64 = (halo32[0].astype(np.float64) + 1e-9, halo32[1].astype(np.float64) - 1e-9)
    n_golden = 0
    for halo in (None, halo32):
        got = e.stream_display_nfm_codes(codes, FS, 4, fmt, halo=halo, **kw)
        same_results(got, e.stream_display_nfm(iq, FS, 4, halo=halo, **kw))
        n_golden += check_golden_pcm(got, names)
    for halo, grids in ((None, True), (halo64, False)):
        got = e.stream_display_nfm_codes_f64(codes, FS, 4, fmt, halo=halo, grids=grids, **kw)
        same_results(got, e.stream_display_nfm_f64(iq, FS, 4, halo=halo, grids=grids, **kw))
        assert ("grids" in got) == grids
        n_golden += check_golden_pcm(got, names)
    if fmt == "cs8":
        assert n_golden >= 4 * 4        # i8_floor_mpx_1024 and dead_zero_1024 are fixture cases: frames 0, 4, 5, 9, 10 of each run


def test_stream_display_with_a_driver_table():
    # a caller's table (SoapyRTLSDR's float32 formula: 64 entries differ from the format's own) reaches the device unchanged
    e = engine()
    codes, _, _ = capture("cu8", STREAM_CASES["cu8"], 11)
    soapy = (np.arange(256).astype(np.float32) - np.float32(127.4)) * (np.float32(1.0) / np.float32(128.0))
    iq = F.unpack_iq(codes, "cu8", table=soapy)
    assert not A.same_bits(iq, F.unpack_iq(codes, "cu8"))
    kw = dict(mode="waterfall", window=5, disp_h=36, disp_w=112, want_db=True)
    same_results(e.stream_display_nfm_codes(codes, FS, 4, "cu8", table=soapy, **kw), e.stream_display_nfm(iq, FS, 4, **kw))


@pytest.mark.parametrize("mode", ["waterfall", "persistence"])
@pytest.mark.parametrize("fmt", sorted(SHORT_CASES))
def test_stream_display_on_codes_29_sample_frames(fmt, mode):
    # 7 frames of 29 samples in chunks of 3: the chunks start at host byte offsets 174 and 348 — no multiples of 16
    e = engine()
    codes, iq, names = capture(fmt, SHORT_CASES[fmt], 7)
    kw = dict(mode=mode, window=5, disp_h=36, disp_w=112, want_db=True)
    got = e.stream_display_nfm_codes(codes, FS, 3, fmt, **kw)
    same_results(got, e.stream_display_nfm(iq, FS, 3, **kw))
    assert check_golden_pcm(got, names) == 7                                # every one of these cases is in the fixture


def test_stream_display_from_pinned_codes():
    e = engine()
    codes, iq, _ = capture("cs16", STREAM_CASES["cs16"], 11)
    pinned = e.pinned_empty(codes.shape, codes.dtype)
    pinned[:] = codes
    kw = dict(mode="persistence", window=5, disp_h=36, disp_w=112)
    same_results(e.stream_display_nfm_codes(pinned, FS, 4, "cs16", **kw), e.stream_display_nfm(iq, FS, 4, **kw))
    e.pinned_free(pinned)


# ---- 4. the batch demodulator and formats.demodulate_recording on codes ---------------------------------------------------------------------
MODES = {"NFM": L.MODE_NFM, "WFM": L.MODE_WFM, "AM": L.MODE_AM, "USB": L.MODE_USB, "LSB": L.MODE_LSB}


@pytest.mark.parametrize("fmt", ["cs8", "cu8", "cs16"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_demodulate_batch_and_recording_on_codes(mode, fmt):
    e = engine()
    codes, iq, _ = capture(fmt, STREAM_CASES[fmt], 9)
    got = e.h_demodulate_batch_codes(MODES[mode], codes, FS, fmt, chunk_frames=4)
    want = e.h_demodulate_batch(MODES[mode], iq, FS, chunk_frames=4)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    flat_codes, flat_iq = codes.reshape(-1, 2), iq.reshape(-1)
    rec = F.demodulate_recording(flat_codes, FS, mode, frame_len=1024, chunk_frames=4, codes_format=fmt)
    ref = F.demodulate_recording(flat_iq, FS, mode, frame_len=1024, chunk_frames=4)
    assert rec.shape == ref.shape and rec.tobytes() == ref.tobytes()
    # the squelch branch, the gate at the median peak: some buffers open, some closed
    _, _, peak, _ = F.demodulate_recording(flat_iq, FS, mode, frame_len=1024, chunk_frames=4, squelch=-1e300)
    squelch = float(np.median(peak))
    rs = F.demodulate_recording(flat_codes, FS, mode, frame_len=1024, chunk_frames=4, squelch=squelch, codes_format=fmt)
    ws = F.demodulate_recording(flat_iq, FS, mode, frame_len=1024, chunk_frames=4, squelch=squelch)
    for a, b in zip(rs, ws):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert 0 < int(ws[1].sum()) <= 9


def test_recording_to_wav_from_a_raw_code_file(tmp_path):
    import wave
    codes, iq, _ = capture("cu8", STREAM_CASES["cu8"], 9)
    raw, npy = tmp_path / "capture.cu8", tmp_path / "capture.npy"
    codes.tofile(raw)
    np.save(npy, iq.reshape(-1))
    a = F.recording_to_wav(str(raw), str(tmp_path / "a.wav"), FS, "NFM", frame_len=1024, codes_format="cu8")
    b = F.recording_to_wav(str(npy), str(tmp_path / "b.wav"), FS, "NFM", frame_len=1024)
    assert a.tobytes() == b.tobytes()
    with wave.open(str(tmp_path / "a.wav")) as wa, wave.open(str(tmp_path / "b.wav")) as wb:
        assert wa.readframes(wa.getnframes()) == wb.readframes(wb.getnframes())

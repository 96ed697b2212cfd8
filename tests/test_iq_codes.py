"""CPU-side checks of the ADC-code formats (include/pss.h "ADC codes"): the host table and the host restatement of the widening against
NumPy's own arithmetic, bit for bit; every ADC case of tests/adc_cases.py that can be written as codes reproduced from its codes; argument
errors; raw capture files.  Needs the library, not a GPU."""
import numpy as np
import pytest

import adc_cases as A
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F

# adc_cases' grid of each format
GRID_OF = {"cu8": "u8o", "cs8": "i8", "cs12": "i12", "cs16": "i16"}
FMT_OF = {g: f for f, g in GRID_OF.items()}
DTYPE_OF = {"cu8": np.uint8, "cs8": np.int8, "cs12": np.int16, "cs16": np.int16}


def all_codes(fmt):
    """Every code of the format's container, as (I, Q) pairs: Q runs through the codes backwards."""
    dt = np.dtype(DTYPE_OF[fmt])
    info = np.iinfo(dt)
    c = np.arange(info.min, info.max + 1, dtype=np.int64).astype(dt)
    return np.stack([c, c[::-1]], axis=1)


def numpy_words(codes, fmt):
    """adc_cases.quantise's arithmetic on integer codes."""
    scale, _, _, off = A.GRIDS[GRID_OF[fmt]]
    code = codes.astype(np.int64)
    w = ((code - off) / scale).astype(np.float32) if off else (code.astype(np.float32) / np.float32(scale))
    return np.ascontiguousarray(w).view(np.complex64).reshape(codes.shape[:-1])


def grid_of_case(case):
    parts = case.name.split("_")
    if parts[0] == "dead":
        return parts[-1] if parts[-1] in A.GRIDS else "i8"
    return parts[0]


def test_formats_are_the_adc_grids():
    assert set(F.IQ_FORMATS) == set(GRID_OF)
    for fmt, (container, scale, offset) in F.IQ_FORMATS.items():
        g_scale, lo, hi, g_off = A.GRIDS[GRID_OF[fmt]]
        assert (scale, offset) == (g_scale, g_off)
        info = np.iinfo(DTYPE_OF[fmt])
        assert info.min <= lo and hi <= info.max
        assert L.load().pss_iq_code_bytes(container) == 2 * np.dtype(DTYPE_OF[fmt]).itemsize
    assert L.load().pss_iq_code_bytes(3) < 0 and L.load().pss_iq_code_bytes(-1) < 0


@pytest.mark.parametrize("fmt", sorted(GRID_OF))
def test_every_code_widens_to_numpys_word(fmt):
    codes = all_codes(fmt)
    want = numpy_words(codes, fmt)
    if fmt in ("cu8", "cs8"):
        # the table itself: entry i is the word of code i (cu8) or i - 128 (cs8)
        table = F.iq_table(fmt)
        code_i = np.arange(256) - (128 if fmt == "cs8" else 0)
        scale, _, _, off = A.GRIDS[GRID_OF[fmt]]
        assert A.same_bits(table, ((code_i.astype(np.float64) - off) / scale).astype(np.float32))
        assert A.same_bits(table, want.view(np.float32)[0::2])
    assert A.same_bits(F.unpack_iq(codes, fmt), want), A.diff_bits(F.unpack_iq(codes, fmt), want)


def test_driver_tables_pass_through_unchanged():
    c = np.arange(256)
    pyrtlsdr = (c / 127.5 - 1).astype(np.float32)
    soapy = (c.astype(np.float32) - np.float32(127.4)) * (np.float32(1.0) / np.float32(128.0))      # SoapyRTLSDR's float32 formula
    own = F.iq_table("cu8")
    # the finding behind the caller-supplied table: the float32 formula is not the float64 one rounded once
    assert int(np.sum(soapy.view(np.uint32) != own.view(np.uint32))) == 64
    odd = np.random.default_rng(5).standard_normal(256).astype(np.float32)
    odd[3], odd[200], odd[77] = np.float32(-0.0), np.float32(np.inf), np.float32(0.0)
    odd_bits = odd.view(np.uint32).copy()
    odd_bits[9], odd_bits[130] = 0x7FC12345, 0xFF800001                 # NaNs with payloads: words, not values
    odd = odd_bits.view(np.float32)
    for fmt in ("cu8", "cs8"):
        codes = all_codes(fmt)
        idx = codes.astype(np.int64) + (128 if fmt == "cs8" else 0)
        for table in (pyrtlsdr, soapy, odd):
            got = F.unpack_iq(codes, fmt, table=table)
            assert np.array_equal(got.view(np.uint32).reshape(-1, 2), table.view(np.uint32)[idx])


def test_adc_cases_reproduce_from_their_codes():
    n_ok = 0
    for case in A.cases():
        w = case.iq.view(np.float32)
        if np.any((w == 0) & np.signbit(w)):
            continue            # a -0 word is no code's word on these grids (the sign variants of adc_cases.with_sign)
        grid = grid_of_case(case)
        fmt = FMT_OF[grid]
        scale, lo, hi, off = A.GRIDS[grid]
        code = np.rint(w.astype(np.float64) * scale + off)
        assert code.min() >= lo and code.max() <= hi, case.name
        codes = code.astype(DTYPE_OF[fmt]).reshape(-1, 2)
        got = F.unpack_iq(codes, fmt)
        assert A.same_bits(got, case.iq), f"{case.name}: {A.diff_bits(got, case.iq)}"
        n_ok += 1
    assert n_ok >= 40, f"only {n_ok} ADC cases could be written as codes"


@pytest.mark.parametrize("scale", [1000.0, 3.0])
def test_s16_division_is_numpys_float32_division(scale):
    codes = all_codes("cs16")
    want = (codes.astype(np.float32) / np.float32(scale)).view(np.complex64).reshape(-1)
    got = F.unpack_iq(codes, (L.IQ_S16, scale, 0.0))
    assert A.same_bits(got, want), A.diff_bits(got, want)


def test_unpack_at_odd_addresses():
    # the host restatement takes codes at any address (the int16 words are assembled from their bytes)
    lib = L.load()
    codes = all_codes("cs16")[:1000]
    raw = np.zeros(codes.nbytes + 1, np.uint8)
    raw[1:] = codes.view(np.uint8).reshape(-1)
    out = np.empty(1000, np.complex64)
    assert lib.pss_h_unpack_iq(L.IQ_S16, raw.ctypes.data + 1, 1000, 2048.0, None, out.ctypes.data) == 0
    assert A.same_bits(out, F.unpack_iq(codes, "cs12"))


def test_argument_errors():
    lib = L.load()
    table, out = np.zeros(256, np.float32), np.empty(4, np.complex64)
    c8, c16 = np.zeros((4, 2), np.uint8), np.zeros((4, 2), np.int16)
    tp, op = table.ctypes.data, out.ctypes.data

    def err(r, text):
        assert r == L.PSS_E_ARG
        assert text in lib.pss_last_error(None), lib.pss_last_error(None)

    err(lib.pss_h_unpack_iq(3, c8.ctypes.data, 4, 1.0, tp, op), b"container")
    err(lib.pss_h_unpack_iq(-1, c8.ctypes.data, 4, 1.0, tp, op), b"container")
    err(lib.pss_h_unpack_iq(L.IQ_U8, c8.ctypes.data, 4, 1.0, None, op), b"table")
    err(lib.pss_h_unpack_iq(L.IQ_S8, c8.ctypes.data, 4, 1.0, None, op), b"table")
    err(lib.pss_h_unpack_iq(L.IQ_S16, c16.ctypes.data, 4, 2048.0, tp, op), b"NULL")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        err(lib.pss_h_unpack_iq(L.IQ_S16, c16.ctypes.data, 4, bad, None, op), b"scale")
    err(lib.pss_h_unpack_iq(L.IQ_U8, c8.ctypes.data, -1, 0.0, tp, op), b"bad arguments")
    err(lib.pss_h_unpack_iq(L.IQ_U8, None, 4, 0.0, tp, op), b"bad arguments")
    err(lib.pss_h_unpack_iq(L.IQ_U8, c8.ctypes.data, 4, 0.0, tp, None), b"bad arguments")
    assert lib.pss_h_unpack_iq(L.IQ_U8, None, 0, 0.0, tp, None) == 0       # nothing to do: PSS_OK; scale is ignored for 8-bit codes
    err(lib.pss_h_iq_table(L.IQ_S16, 2048.0, 0.0, tp), b"8-bit")
    err(lib.pss_h_iq_table(L.IQ_U8, 0.0, 0.0, tp), b"scale")
    err(lib.pss_h_iq_table(L.IQ_U8, 128.0, float("nan"), tp), b"offset")
    err(lib.pss_h_iq_table(L.IQ_U8, 128.0, 0.0, None), b"null")
    # the Python layer: a code array of another type is an error, not a cast; int16 formats take no table
    with pytest.raises(ValueError):
        F.unpack_iq(np.zeros((4, 2), np.int16), "cu8")
    with pytest.raises(ValueError):
        F.unpack_iq(np.zeros((4, 3), np.uint8), "cu8")
    with pytest.raises(ValueError):
        F.unpack_iq(c16, "cs16", table=table)
    with pytest.raises(ValueError):
        F.unpack_iq(c8, "cu8", table=np.zeros(255, np.float32))
    with pytest.raises(KeyError):
        F.unpack_iq(c8, "cu12")


@pytest.mark.parametrize("fmt", sorted(GRID_OF))
def test_load_iq_codes_round_trip(fmt, tmp_path):
    codes = all_codes(fmt)[:200]
    path = tmp_path / ("capture." + fmt)
    codes.tofile(path)
    back = F.load_iq_codes(str(path), fmt)
    assert back.shape == (200, 2) and back.dtype == codes.dtype and np.array_equal(back, codes)
    assert A.same_bits(F.unpack_iq(back, fmt), F.unpack_iq(codes, fmt))
    unit = codes.dtype.itemsize
    with open(path, "ab") as f:
        f.write(b"\x00" * unit)            # one I without its Q
    with pytest.raises(ValueError):
        F.load_iq_codes(str(path), fmt)
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    assert F.load_iq_codes(str(empty), fmt).shape == (0, 2)


def test_demodulate_recording_checks_codes_before_the_gpu():
    with pytest.raises(ValueError):
        F.demodulate_recording(np.zeros((64, 2), np.int16), 2.4e6, "NFM", frame_len=32, codes_format="cu8")
    with pytest.raises(ValueError):
        F.demodulate_recording(np.zeros(64, np.uint8), 2.4e6, "NFM", frame_len=32, codes_format="cu8")

"""The batched decoders against tests/golden/decode_batch.npz (CPU only): the new symbols, the regenerated recordings, the host twins
(pss_h_morse_decode on NumPy's edges, pss_h_ax25_frame on the fixture's bit rows) against what the reference returned buffer by buffer,
the NumPy statement of pss_real_normalise, and decode_recording's argument checks.  Every comparison is equality of bytes or bits."""
import json
import os
import re

import numpy as np
import pytest

import decode_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import decoders as D
from pyspecsdr_amd import formats as F
from pyspecsdr_amd import signal_processing as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pss_morse_text", "pss_ax25_frames", "pss_real_normalise", "pss_decode_morse_batch", "pss_decode_aprs_batch")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "decode_batch.npz"))


def numpy_edges(buf, threshold=S.THRESHOLD):
    """decoders.py:149-163 in NumPy (the front half is pinned bit for bit by decoders.npz; the fixture's buffers sit far from the cut)"""
    env = np.abs(buf)
    env = env / np.max(env)
    tr = np.diff((20 * np.log10(env + 1e-10) > threshold).astype(int))
    return np.where(tr == 1)[0].astype(np.int32), np.where(tr == -1)[0].astype(np.int32)


def test_every_new_symbol_is_declared_exported_and_in_the_ctypes_table():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} is not declared in include/pss.h"
        assert hasattr(lib, name) and name in L._SIGS
    units = [u for u, _ in __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS]
    assert "pss_decode_dev.hip" in units


def test_the_grid_caps_the_gpu_tests_go_one_past_are_the_sources():
    import test_gpu_decode_batch as T
    src = open(os.path.join(ROOT, "pyspecsdr_amd", "csrc", "pss_decode_dev.hip")).read()
    for line in (f"constexpr int MT_GRID_MAX = {T.MT_GRID_MAX};", f"constexpr int AX_GRID_MAX = {T.AX_GRID_MAX};", f"constexpr int RN_GRID_MAX = {T.RN_GRID_MAX};",
                 "constexpr int MT_STAGE = 4096;", "dim3((unsigned)(n_frames < MT_GRID_MAX ? n_frames : MT_GRID_MAX)), dim3(256)",
                 "dim3((unsigned)(groups < AX_GRID_MAX ? groups : AX_GRID_MAX)), dim3(256)", "const long groups = (n_rows + 3) / 4;",
                 "dim3((unsigned)(n_rows < RN_GRID_MAX ? n_rows : RN_GRID_MAX)), dim3(256)"):
        assert line in src, line
    assert 4096 in T.COUNTS and 4097 in T.COUNTS


def test_the_regenerated_recordings_are_the_generators(gold):
    assert [str(c) for c in gold["cases"]] == [c.name for c in S.CASES]
    cond = json.loads(str(gold["conditions"]))
    assert len(cond["seeds"]) >= 4
    for c in S.CASES:
        codes, x = S.codes(c), S.frames(c)
        assert codes.dtype == np.int16 and codes.shape == (x.size, 2) and x.dtype == np.complex64 and x.shape[1] == c.n == int(c.fs * 0.5)
        assert S.crc(codes) == int(gold[f"crc_{c.name}"]), "the regenerated codes are the generator's"
        assert cond[c.name]["buffers"] == len(x)
    for c in S.APRS:
        packets = json.loads(str(gold[f"packets_{c.name}"]))
        assert len(packets) == len(S.frames(c)) == 40 and 3 * sum(1 for p in packets if p) >= len(packets)
        assert gold[f"bits_{c.name}"].shape == (40, L.load().pss_afsk_n_bits(c.n, c.fs))
    assert sum(len(S.frames(c)) for c in S.MORSE) >= 64


@pytest.mark.parametrize("c", S.MORSE, ids=lambda c: c.name)
def test_host_morse_twin_on_numpys_edges_equals_the_reference(gold, c):
    texts, timing = gold[f"text_{c.name}"], gold[f"timing_{c.name}"]
    cut_start = cut_end = 0
    for f, buf in enumerate(S.frames(c)):
        rise, fall = numpy_edges(buf)
        if len(rise) and len(fall):
            cut_start += fall[0] < rise[0]
            cut_end += rise[-1] > fall[-1]
        text, tm = D.morse_from_edges(rise, fall, c.fs)
        assert text == str(texts[f]), (f, text)
        got = np.array([float(tm["dot"]), float(tm["dash"]), float(tm["gap"])])
        assert np.array_equal(got.view(np.uint64), timing[f]), (f, got)
    assert cut_start and cut_end, "buffer boundaries cut pulses at either end"


@pytest.mark.parametrize("c", S.APRS, ids=lambda c: c.name)
def test_host_ax25_twin_on_the_fixtures_bit_rows_equals_the_reference(gold, c):
    packets = json.loads(str(gold[f"packets_{c.name}"]))
    for f, row in enumerate(gold[f"bits_{c.name}"]):
        pk = D.decode_ax25_frame(row)
        assert ([pk] if pk else []) == packets[f], f


def test_the_numpy_statement_of_real_normalise_divides_in_float32():
    x = S.frames(S.case("aprs_9600"))[:3]
    r = np.real(x)
    assert r.dtype == np.float32 and (r / np.max(np.abs(r), axis=-1, keepdims=True)).dtype == np.float32
    got = S.real_normalise_np(x)
    assert got.dtype == np.float64 and np.array_equal(got, got.astype(np.float32).astype(np.float64))
    for k in range(3):    # row by row it is the reference's expression on one buffer
        one = np.real(x[k]) / np.max(np.abs(np.real(x[k])))
        assert np.array_equal(got[k].view(np.uint64), one.astype(np.float64).view(np.uint64))
    wide = np.real(x).astype(np.float64)
    wide = wide / np.max(np.abs(wide), axis=-1, keepdims=True)
    assert (wide != got).mean() > 0.5, "the float64 quotients are other numbers"
    with np.errstate(all="ignore"):
        assert np.isnan(S.real_normalise_np(np.zeros((1, 4), np.complex64))).all()


def test_decode_recording_checks_its_arguments_before_the_gpu(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(SP, "get_engine", no_engine)
    monkeypatch.setattr(F, "get_engine", no_engine)
    x = np.zeros(100, np.complex64)
    for bad in (dict(decoder="rtty"), dict(decoder="morse", frame_len=0), dict(decoder="morse", frame_len=2.5),
                dict(decoder="morse", chunk_frames=0), dict(decoder="aprs", sample_rate=800.0), dict(decoder="morse", sample_rate=0.0)):
        kw = dict(sample_rate=48000.0, decoder="morse")
        kw.update(bad)
        with pytest.raises(ValueError):
            F.decode_recording(x, **kw)
    with pytest.raises(ValueError):
        F.decode_recording(np.zeros((4, 4), np.complex64), 48000.0, "morse", frame_len=4)
    with pytest.raises(ValueError):       # codes of another type than the format's
        F.decode_recording(np.zeros((64, 2), np.int16), 48000.0, "morse", frame_len=32, codes_format="cu8")
    with pytest.raises(ValueError):
        F.decode_recording(np.zeros(64, np.int16), 48000.0, "aprs", frame_len=32, codes_format="cs16")
    with pytest.raises(ValueError):
        F.decode_recording(np.zeros((64, 2), np.int16), 48000.0, "aprs", frame_len=32, codes_format="cs16", table=np.zeros(256, np.float32))

"""Dead reads on the host (pss_h_live_frames, pure C): the reference's loop skips a read buffer with np.all(samples == 0)
(pyspecsdr.py:2237).  The rule is decided on the bits and must agree with NumPy's `== 0` for -0.0, denormals, NaN and inf."""
import ctypes as C

import numpy as np
import pytest

import stream_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

SENTINEL = -7


def run(frames, want_idx=True):
    lib = L.load()
    frames = np.ascontiguousarray(frames)
    nf, n = frames.shape
    live = np.full(nf, 9, np.uint8)
    idx = np.full(nf, SENTINEL, np.int32)
    n_live = C.c_long(-1)
    r = lib.pss_h_live_frames(frames.ctypes.data, nf, n, live.ctypes.data, idx.ctypes.data if want_idx else None, C.byref(n_live))
    assert r == L.PSS_OK
    return live, idx, n_live.value


def check(frames, name):
    want = S.numpy_live(frames)
    live, idx, n_live = run(frames)
    assert np.array_equal(live, want), f"{name}: flags differ from ~np.all(frames == 0, axis=1) at frames {np.flatnonzero(live != want)[:8]}"
    assert n_live == int(want.sum()), name
    assert np.array_equal(idx[:n_live], np.flatnonzero(want)), f"{name}: the index list is not the live frames in ascending order"
    assert np.all(idx[n_live:] == SENTINEL), f"{name}: entries behind n_live were written"


@pytest.mark.parametrize("name,frames", S.live_cases(), ids=[c[0] for c in S.live_cases()])
def test_host_flags_equal_numpy(name, frames):
    if "dead" in name:
        assert not S.numpy_live(frames).any()
    else:
        assert S.numpy_live(frames).sum() == len(S.word_positions(frames.shape[1])), "every placed word must count as live for NumPy"
    check(frames, name)


@pytest.mark.parametrize("name,frames", S.live_batches(), ids=[c[0] for c in S.live_batches()])
def test_host_batch_sizes(name, frames):
    check(frames, name)


def test_outputs_are_optional_and_engine_wrapper_agrees():
    name, frames = S.live_cases()[4]
    want = S.numpy_live(frames)
    lib = L.load()
    n_live = C.c_long(-1)
    assert lib.pss_h_live_frames(np.ascontiguousarray(frames).ctypes.data, len(frames), frames.shape[1], None, None, C.byref(n_live)) == L.PSS_OK
    assert n_live.value == want.sum()
    live, idx = Engine.h_live_frames(frames)
    assert np.array_equal(live, want) and np.array_equal(idx, np.flatnonzero(want))


def test_unaligned_host_pointer():
    raw = np.zeros(4 + 8 * 3 * 5, np.uint8)
    frames = raw[4:].view(np.uint32).reshape(5, 6)      # 4 bytes off: the host twin takes any address
    frames[3, 5] = 0x80000001
    n_live, live = C.c_long(), np.empty(5, np.uint8)
    assert L.load().pss_h_live_frames(frames.ctypes.data, 5, 3, live.ctypes.data, None, C.byref(n_live)) == L.PSS_OK
    assert live.tolist() == [0, 0, 0, 1, 0] and n_live.value == 1


def test_argument_errors():
    lib = L.load()
    x = np.zeros((2, 4), np.complex64)
    n_live = C.c_long(5)
    assert lib.pss_h_live_frames(x.ctypes.data, 2, 0, None, None, C.byref(n_live)) == L.PSS_E_ARG          # n < 1
    assert lib.pss_h_live_frames(x.ctypes.data, -1, 4, None, None, C.byref(n_live)) == L.PSS_E_ARG         # n_frames < 0
    assert lib.pss_h_live_frames(x.ctypes.data, 2 ** 31, 4, None, None, C.byref(n_live)) == L.PSS_E_ARG    # n_frames >= 2^31
    assert lib.pss_h_live_frames(None, 2, 4, None, None, C.byref(n_live)) == L.PSS_E_ARG                   # null frames
    assert lib.pss_h_live_frames(x.ctypes.data, 2, 4, None, None, None) == L.PSS_E_ARG                     # null count
    assert n_live.value == 5, "a rejected call writes nothing"
    assert lib.pss_h_live_frames(None, 0, 4, None, None, C.byref(n_live)) == L.PSS_OK and n_live.value == 0


def test_stream_structs_match_the_header():
    """The ctypes structures restate include/pss.h field by field, in order."""
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pss.h")).read()
    for cname, struct in (("pss_stream_req", L.StreamReq), ("pss_stream_res", L.StreamRes)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        fields = [re.search(r"(\w+);", line).group(1) for line in body.strip().splitlines()]
        assert fields == [f[0] for f in struct._fields_], cname

"""pyspecsdr_amd/csrc/pss_npsum.h, host side, against this machine's np.add.reduce — no GPU.

The header is the library's one statement of NumPy's pairwise sum.  tests/npsum_host.cpp is compiled with plain g++ (the header must not need
HIP) and gives two sums per array: the header's plain sum, and its TABLES (the forest the kernels walk) evaluated on the host — leaf rule,
inner nodes level by level, roots in chunk order.  Both must have np.add.reduce's bits at every length of length_cases.REDUCE_LENGTHS, in
float32, float64 and complex64, on power_frames' data (terms 2^-8 .. 2^3 apart: another order of additions rounds differently).  The second
form ties the kernels' tables to NumPy; it is also what keeps the Morse host-versus-device comparison honest, now that both sides call
the same function."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import length_cases as LC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pyspecsdr_amd", "csrc")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("npsum") / "npsum_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                    os.path.join(HERE, "npsum_host.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    f32, f64 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS"), np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    lib.npsum_f32.restype, lib.npsum_f32.argtypes = C.c_float, [f32, C.c_long]
    lib.npsum_f64.restype, lib.npsum_f64.argtypes = C.c_double, [f64, C.c_long]
    lib.npsum_c64.restype, lib.npsum_c64.argtypes = None, [f32, C.c_long, f32]
    lib.tabsum_f32.restype, lib.tabsum_f32.argtypes = C.c_float, [f32, C.c_int]
    lib.tabsum_f64.restype, lib.tabsum_f64.argtypes = C.c_double, [f64, C.c_int]
    lib.tabsum_c64.restype, lib.tabsum_c64.argtypes = None, [f32, C.c_int, f32]
    lib.wave_tree.restype, lib.wave_tree.argtypes = C.c_int, [C.c_int, C.c_int]
    return lib


def bits(x):
    x = np.asarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]).tolist() if x.dtype.kind != "c" else bits(np.atleast_1d(x).view(np.float32))


def test_plain_sum_and_tables_have_numpys_bits_at_every_length(host):
    bad = []
    for n in LC.REDUCE_LENGTHS:
        x = LC.power_frames(1, n)[0]                                           # complex64
        p64 = x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2   # the power's terms, all 53 bits in use
        p32 = p64.astype(np.float32)
        xf = np.ascontiguousarray(x).view(np.float32)
        got_c, tab_c = np.empty(2, np.float32), np.empty(2, np.float32)
        host.npsum_c64(xf, n, got_c)
        host.tabsum_c64(xf, n, tab_c)
        for what, want, got, tab in (("float32", np.add.reduce(p32), np.float32(host.npsum_f32(p32, n)), np.float32(host.tabsum_f32(p32, n))),
                                     ("float64", np.add.reduce(p64), np.float64(host.npsum_f64(p64, n)), np.float64(host.tabsum_f64(p64, n))),
                                     ("complex64", np.add.reduce(x), got_c.view(np.complex64)[0], tab_c.view(np.complex64)[0])):
            assert want.dtype == got.dtype == tab.dtype
            if bits(got) != bits(want):
                bad.append((n, what, "plain sum"))
            if bits(tab) != bits(want):
                bad.append((n, what, "tables"))
    assert not bad, (len(bad), bad[:20])


def test_wave_tree_is_set_for_1024_elements_only(host):
    for cplx in (0, 1):
        assert host.wave_tree(1024, cplx) == 1
        assert host.wave_tree(1000, cplx) == 0 and host.wave_tree(2048, cplx) == 0
    assert [n for n in range(1, 4200) for cplx in (0, 1) if host.wave_tree(n, cplx)] == [1024, 1024]

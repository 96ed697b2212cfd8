"""The rational resampler without a GPU: pss_h_resample (the host twin of k_resample: the statements of pyspecsdr_amd/csrc/pss_resample.h
on one thread) against SciPy's own resample_poly — the goldens of tests/golden/resample.npz and, where SciPy is importable, a live call —
bit for bit; every split of the output window and every chunking with exactly the needed halo; a window of a virtual row of 2^41 samples
against Python integers; strides, refusals; the tap designer against SciPy's Kaiser firwin; the plan helpers of formats; the header alone
under the sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bytes_util import same_bytes
import resample_cases as RC
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")

CASES = RC.golden_cases()


_TAPS = {}


def taps_of(up, down):
    key = RC.reduced(up, down)
    if key not in _TAPS:
        _TAPS[key] = Engine.resample_default_taps(up, down)
    return _TAPS[key]


def h_call(x, dtype, n_rows, x_stride, n_buf, buf_index0, n_in, up, down, taps, j_begin, j_end, y, y_stride, n_taps=None):
    """pss_h_resample as it is declared -> (code, reason)."""
    lib = L.load()
    taps = None if taps is None else np.ascontiguousarray(taps, np.float64)
    r = lib.pss_h_resample(None if x is None else x.ctypes.data, dtype, n_rows, x_stride, n_buf, buf_index0, n_in, up, down,
                           None if taps is None else taps.ctypes.data, (0 if taps is None else len(taps)) if n_taps is None else n_taps, j_begin, j_end,
                           None if y is None else y.ctypes.data, y_stride)
    return r, lib.pss_last_error(None).decode()


def test_goldens_are_scipys_bytes(golden):
    g = golden["resample"]
    assert "stamp" in g.files and len(CASES) > 190
    for name, up, down, x in CASES:
        assert RC.crc(x) == g["crc_" + name], f"{name}: resample_cases no longer regenerates the row the golden was taken on"
        got = Engine.h_resample(x, up, down, taps=taps_of(up, down))
        assert same_bytes(got, g["out_" + name]), name


def test_live_scipy_where_importable():
    ss = pytest.importorskip("scipy.signal")
    for name, up, down, x in CASES:
        with np.errstate(invalid="ignore"):
            want = ss.resample_poly(x, up, down)
        assert same_bytes(Engine.h_resample(x, up, down, taps=taps_of(up, down)), want), name
    # rows of a batch, and a table that is not the default one (an even count, another window)
    x = np.stack([RC.row(50 + r, 131, np.float32) for r in range(3)])
    assert same_bytes(Engine.h_resample(x, 3, 7, taps=taps_of(3, 7)), ss.resample_poly(x, 3, 7, axis=1))
    # (float64 rows: SciPy takes an array window as it is, so its type must be the row's — mixed types are out of scope)
    x = RC.row(7, 200, np.float64)
    win = ss.firwin(44, 0.2, window="hamming")
    assert same_bytes(Engine.h_resample(x, 4, 5, taps=win), ss.resample_poly(x, 4, 5, window=win))


@pytest.mark.parametrize("up,down", [(2, 3), (5, 1), (1, 4), (441, 500), (12, 50), (7, 7)])
def test_every_split_and_every_chunking_gives_the_one_calls_bytes(up, down):
    n = 157
    taps = taps_of(up, down)
    for dt in (np.float32, np.complex64):
        x = RC.row(3, n, dt)
        whole = Engine.h_resample(x, up, down, taps=taps)
        n_out = len(whole)
        assert n_out == Engine.resample_out_len(n, up, down) == RC.geometry(n, up, down, len(taps))["n_out"]
        for cut in range(0, n_out + 1):
            a = Engine.h_resample(x, up, down, taps=taps, j_end=cut)
            b = Engine.h_resample(x, up, down, taps=taps, j_begin=cut)
            assert same_bytes(np.concatenate([a, b]), whole), cut
        for chunk in (1, 7, 64):
            parts = []
            for j0 in range(0, n_out, chunk):
                j1 = min(n_out, j0 + chunk)
                lo, hi = RC.halo(n, up, down, len(taps), j0, j1)
                parts.append(Engine.h_resample(x[lo:hi], up, down, taps=taps, buf_index0=lo, n_in=n, j_begin=j0, j_end=j1))
                if hi - lo > 1:       # one sample less on either side is refused: the halo is exact
                    for cut_lo, cut_hi in ((lo + 1, hi), (lo, hi - 1)):
                        with pytest.raises(ValueError, match="needs a sample"):
                            Engine.h_resample(x[cut_lo:cut_hi], up, down, taps=taps, buf_index0=cut_lo, n_in=n, j_begin=j0, j_end=j1)
            assert same_bytes(np.concatenate(parts), whole), chunk
    from pyspecsdr_amd import formats
    assert formats.resample_halo(n, up, down, len(taps), 3, 30) == RC.halo(n, up, down, len(taps), 3, 30)


def test_a_window_of_a_virtual_row_of_2_to_the_41_samples():
    n_in = 1 << 41
    for up, down, dt in ((441, 500, np.complex64), (3, 2, np.float64), (1, 4, np.float32), (160, 147, np.float32)):
        taps = taps_of(up, down)
        n_out = Engine.resample_out_len(n_in, up, down)
        assert n_out == -(-n_in * up // down)
        for j0 in (n_out // 3 + 11, n_out - 40):
            j1 = j0 + 40
            lo, hi = RC.halo(n_in, up, down, len(taps), j0, j1)
            assert 0 < lo < hi <= n_in and hi - lo < 4000
            buf = RC.row(j0 % 1000, hi - lo, dt)
            got = Engine.h_resample(buf, up, down, taps=taps, buf_index0=lo, n_in=n_in, j_begin=j0, j_end=j1)
            want = np.array([RC.output_py(j, n_in, up, down, taps, dt, lambda i: buf[i - lo]) for j in range(j0, j1)], dt)
            assert same_bytes(got, want), (up, down, j0)


def test_strided_rows_leave_the_gaps_untouched():
    up, down, n, n_rows = 3, 2, 41, 3
    taps = taps_of(up, down)
    for dt in RC.DTYPES:
        rows = np.stack([RC.row(20 + r, n, dt) for r in range(n_rows)])
        want = Engine.h_resample(rows, up, down, taps=taps)
        n_out = want.shape[1]
        xs, ys = n + 5, n_out + 3
        x = np.full((n_rows, xs), 99, dt)
        x[:, :n] = rows
        y = np.full((n_rows, ys), -7.25, dt)
        r, why = h_call(x, RC.CODES[np.dtype(dt)], n_rows, xs, n, 0, n, up, down, taps, 0, n_out, y, ys)
        assert r == 0, why
        assert same_bytes(y[:, :n_out], want) and np.all(y[:, n_out:] == dt(-7.25))
        # a window of it
        y = np.full((n_rows, ys), -7.25, dt)
        r, why = h_call(x, RC.CODES[np.dtype(dt)], n_rows, xs, n, 0, n, up, down, taps, 5, 17, y, ys)
        assert r == 0 and same_bytes(y[:, :12], want[:, 5:17]) and np.all(y[:, 12:] == dt(-7.25)), why


def refusals(n=41, up=3, down=2):
    """(what, keyword changes) of every refusal pss.h lists, for a call that is otherwise fine."""
    bad_taps = taps_of(up, down).copy()
    bad_taps[7] = np.inf
    return [("up or down outside", dict(up=0)), ("up or down outside", dict(down=4097)), ("n_taps outside", dict(n_taps=0)),
            ("n_taps outside", dict(taps=np.ones(32 * 3 + 2))), ("a tap that is not finite", dict(taps=bad_taps)), ("null taps", dict(taps=None, n_taps=5)),
            ("unknown dtype", dict(dtype=3)), ("unknown dtype", dict(dtype=-1)), ("null output", dict(y=None)), ("null input", dict(x=None)),
            ("not aligned", dict(x_off=4)), ("not aligned", dict(y_off=4)), ("not inside the row", dict(n_buf=n + 1)),
            ("not inside the row", dict(buf_index0=1)), ("not inside the row", dict(buf_index0=-1)), ("outside [0, ceil", dict(j_end=63)),
            ("outside [0, ceil", dict(j_begin=-1)), ("outside [0, ceil", dict(j_begin=9, j_end=8)), ("y_stride <", dict(y_stride=61)),
            ("x_stride <", dict(x_stride=n - 1)), ("needs a sample", dict(n_buf=n - 1)), ("n_rows < 0", dict(n_rows=-1)),
            ("n_in outside", dict(n_in=(1 << 48) + 1, n_buf=0, j_end=0))]


def test_every_refusal_names_itself_and_writes_nothing():
    n, up, down = 41, 3, 2
    x8 = np.zeros(2 * (n + 8), np.float64)
    y8 = np.zeros(2 * 80, np.float64)
    for what, change in refusals():
        a = dict(dtype=1, n_rows=2, x_stride=n, n_buf=n, buf_index0=0, n_in=n, up=up, down=down, taps=taps_of(up, down), j_begin=0, j_end=62, y_stride=62,
                 n_taps=None, x=x8, y=y8, x_off=0, y_off=0)
        a.update(change)
        y8[:] = -7.25
        x = None if a["x"] is None else a["x"].view(np.uint8)[a["x_off"]:].view(np.uint8)
        y = None if a["y"] is None else a["y"].view(np.uint8)[a["y_off"]:].view(np.uint8)
        r, why = h_call(x, a["dtype"], a["n_rows"], a["x_stride"], a["n_buf"], a["buf_index0"], a["n_in"], a["up"], a["down"], a["taps"], a["j_begin"],
                        a["j_end"], y, a["y_stride"], n_taps=a["n_taps"])
        assert r == L.PSS_E_ARG and why.startswith("pss_h_resample: ") and what in why, (what, change, r, why)
        assert np.all(y8 == -7.25), what
    # nothing to do is not an error, and writes nothing
    y8[:] = -7.25
    assert h_call(x8, 1, 0, n, n, 0, n, up, down, taps_of(up, down), 0, 62, y8, 62)[0] == 0
    assert h_call(x8, 1, 2, n, n, 0, n, up, down, taps_of(up, down), 9, 9, y8, 0)[0] == 0
    assert h_call(None, 1, 2, 0, 0, 0, 0, up, down, taps_of(up, down), 0, 0, None, 0)[0] == 0
    assert np.all(y8 == -7.25)
    lib = L.load()
    assert lib.pss_resample_out_len(-1, 1, 1) < 0 and lib.pss_resample_out_len(5, 0, 1) < 0 and lib.pss_resample_out_len(5, 1, 4097) < 0
    assert lib.pss_resample_out_len(50000, 441, 500) == 44100 and lib.pss_resample_out_len(50000, 882, 1000) == 44100
    n_t = C.c_int()
    assert lib.pss_resample_default_taps(0, 1, None, C.byref(n_t)) == L.PSS_E_ARG
    assert lib.pss_resample_default_taps(12, 50, None, C.byref(n_t)) == 0 and n_t.value == 501
    assert lib.pss_resample_default_taps(7, 7, None, C.byref(n_t)) == 0 and n_t.value == 1


def test_default_taps_are_scipys_kaiser_firwin():
    """pss_resample_default_taps against scipy.signal.firwin(20 m + 1, 1 / m, window=('kaiser', 5.0)): every bit (0 ulp measured on the
    build image for every m below; PARITY.md "Resampler")."""
    ss = pytest.importorskip("scipy.signal")
    for m in list(range(2, 65)) + [147, 160, 441, 500, 1000, 4096]:
        want = ss.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0))
        for up, down in ((1, m), (m, 1)):
            got = Engine.resample_default_taps(up, down)
            assert same_bytes(got, want), (m, int(np.sum(got != want)))


def test_header_table_and_library_agree_on_the_new_entry_points():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pss.h")).read(), flags=re.S)
    want = {"pss_resample_out_len": (3, "long"), "pss_resample_default_taps": (4, "int"), "pss_resample": (16, "int"), "pss_h_resample": (15, "int")}
    for name, (n_args, res) in want.items():
        m = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, f"{name} is not declared in include/pss.h"
        assert len(m.group(1).split(",")) == n_args == len(L._SIGS[name][1]), name
        assert L._SIGS[name][0] is (C.c_long if res == "long" else C.c_int) and hasattr(lib, name)
    for name, val in (("PSS_RS_F32", L.RS_F32), ("PSS_RS_F64", L.RS_F64), ("PSS_RS_C64", L.RS_C64)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(val) + r"\b", txt), name
    assert ("pss_resample.hip", ["-ffp-contract=off"]) in __import__("pyspecsdr_amd.build", fromlist=["UNITS"]).UNITS
    from pyspecsdr_amd import signal_processing as sp
    assert "resample_poly" in sp.__all__ and callable(sp.resample_poly)


def test_the_shims_fall_through_cases_are_scipys():
    """Integer input, array windows, other padtypes, three axes: handed to scipy.signal.resample_poly unchanged (no GPU involved)."""
    ss = pytest.importorskip("scipy.signal")
    from pyspecsdr_amd import signal_processing as sp
    xi = np.arange(40, dtype=np.int64) % 7
    assert same_bytes(sp.resample_poly(xi, 3, 2), ss.resample_poly(xi, 3, 2))
    xf = RC.row(1, 60, np.float64)
    win = ss.firwin(31, 0.3)
    assert same_bytes(sp.resample_poly(xf, 2, 3, window=win), ss.resample_poly(xf, 2, 3, window=win))
    assert same_bytes(sp.resample_poly(xf, 2, 3, padtype="mean"), ss.resample_poly(xf, 2, 3, padtype="mean"))
    assert same_bytes(sp.resample_poly(xf, 2, 3, cval=1.5), ss.resample_poly(xf, 2, 3, cval=1.5))
    x3 = xf.reshape(3, 4, 5)
    assert same_bytes(sp.resample_poly(x3, 2, 3, axis=1), ss.resample_poly(x3, 2, 3, axis=1))
    xc = RC.row(2, 30, np.complex64).astype(np.complex128)
    assert same_bytes(sp.resample_poly(xc, 5, 4), ss.resample_poly(xc, 5, 4))
    assert same_bytes(sp.resample_poly(xf, 7, 7), xf) and sp.resample_poly(xf, 7, 7) is not xf
    with pytest.raises(ValueError):
        sp.resample_poly(xf, 0, 3)
    with pytest.raises(ValueError):
        sp.resample_poly(xf, 2.5, 3)


def test_plan_resample_and_plan_audio():
    from pyspecsdr_amd import formats as F
    assert F.plan_resample(50000, 44100) == (441, 500) and F.plan_resample(50000.0, 22050) == (441, 1000)
    assert F.plan_resample(240000, 110250) == (147, 320) and F.plan_resample(48000, 48000) == (1, 1)
    assert F.plan_audio(50000, "NFM") == (441, 500, 44100.0) and F.plan_audio(50000, "AM") == (441, 1000, 22050.0)
    assert F.plan_audio(240000, "WFM") == (147, 320, 110250.0)
    for mode in ("USB", "LSB", "RAW"):
        assert F.plan_audio(50000, mode) == (441, 1000, 22050.0)
    with pytest.raises(ValueError, match="rate_in"):
        F.plan_resample(50000.5, 44100)
    with pytest.raises(ValueError, match="rate_out"):
        F.plan_resample(50000, 44100.25)
    with pytest.raises(ValueError, match="down"):
        F.plan_resample(2400000, 44100)          # 147 / 8000
    with pytest.raises(ValueError, match="up"):
        F.plan_resample(44100, 2400000)
    with pytest.raises(ValueError, match="mode"):
        F.plan_audio(50000, "FM")
    with pytest.raises(TypeError):
        F.monitor_channels(np.zeros(10, np.complex64), 2.4e6, 0.0, [0.0], 12.5e3, nonsense=1)


def test_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/resample_host.cpp: pss_resample.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan, as
    a program of its own."""
    exe = str(tmp_path / "resample_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "resample_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "resample_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

"""The RDS kernels (k_rds_front, k_rds_energy, k_rds_bits, k_rds_groups) against their host twins on every byte, the chain from IQ on the
device against the golden groups of tests/golden/rds.npz, and formats.rds_stations on a synthetic capture of the band.  The shapes are
the smallest at which a kernel takes each of its paths: more than one tile and a partial one, one (row, tile) pair past the grid cap,
rows around the 1024-sample segments, fewer segments than the smoothing span, the timing wraps, groups at the row's end; one row past
the caps of k_rds_energy, k_rds_bits and k_rds_groups, and a row of more segments than one pass of k_rds_bits' scan.  The caps come from
tests/launch_caps.py, where tests/test_launch_caps.py pins them to the source lines."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rds_cases as R
from bytes_util import same, same_bytes
from gpu_util import dev, empty, host
from launch_caps import BITS_SCAN_PASS, BT_GRID_CAP, EN_GRID_CAP, FRONT_GRID_CAP, GR_GRID_CAP, RDS_SEGMENT, RECEIVER_CAPS   # pinned by tests/test_launch_caps.py
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rds.npz"))
NAMES = [str(n) for n in GOLD["names"]]


@pytest.fixture(scope="module")
def e():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    eng = Engine(0)
    yield eng
    eng.close()


def capture(shape, seed):
    rng = np.random.default_rng([57, seed])
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-3, 2, shape))).astype(np.complex64)


def taps_of(T, seed):
    return np.random.default_rng([58, T, seed]).standard_normal(T) / np.sqrt(T)


def tile_outputs(D, T):
    """csrc/pss_ddc.h: tile_outputs, restated."""
    nb = (T + 63) // 64
    M = 1792 // nb
    while M > 1 and D * ((M - 1 + (T + D - 1) // D) | 1) > 8192:
        M -= 1
    return M


def front_on_device(e, x, fs, D, taps, m_begin=0, m_end=None, index0=0, n_capture=None):
    """x [rows][n_buf] -> complex64 [rows][m_end - m_begin], through a buffer and an output with strides of their own."""
    rows, n_buf = x.shape
    n_capture = n_buf if n_capture is None else n_capture
    m_end = -(-n_capture // D) if m_end is None else m_end
    wide = np.full((rows, n_buf + 3), np.nan, np.complex64)
    wide[:, :n_buf] = x
    d_out = torch.full((rows, 2 * (m_end - m_begin + 5)), 9.0, dtype=torch.float32, device="cuda")
    e.rds_front(dev(wide), rows, n_buf, fs, D, d_out, taps=taps, x_stride=n_buf + 3, buf_index0=index0, n_capture=n_capture, m_begin=m_begin, m_end=m_end,
                out_stride=m_end - m_begin + 5)
    e.sync()
    out = host(d_out).view(np.complex64)
    assert np.all(out[:, m_end - m_begin:] == 9 + 9j)               # nothing between the rows is touched
    return out[:, :m_end - m_begin]


@pytest.mark.parametrize("D", [1, 12, 13, 21, 126, 204])
def test_front_is_the_twin(e, D):
    fs = 19000.0 * D + 12000.0 if D > 6 else 240000.0
    for T in sorted({1, D, 20 * D + 1, 4097}):
        M = tile_outputs(D, T)
        n_out = M + 3 if M < 1792 else M + 40                         # a whole tile and a partial one
        n = D * (n_out - 1) + 1 + (D > 1)
        x = capture((2, n), D * 10000 + T)
        taps = taps_of(T, D)
        want = Engine.h_rds_front(x, fs, D, taps=taps)
        assert want.shape == (2, n_out)
        assert same_bytes(front_on_device(e, x, fs, D, taps), want), (D, T)
        # a window that starts inside the first tile's halo, from a buffer that holds exactly what it needs
        lead, m0, m1 = (T - 1) // 2, 1, n_out - 1
        lo, hi = max(0, m0 * D + lead - (T - 1) - 1), min(n, (m1 - 1) * D + lead + 1)
        got = front_on_device(e, np.ascontiguousarray(x[:, lo:hi]), fs, D, taps, m0, m1, lo, n)
        assert same_bytes(got, want[:, m0:m1]), (D, T, "window")


def test_front_one_pair_past_the_grid_cap(e):
    D, T, rows = 12, 241, FRONT_GRID_CAP + 1                          # one tile a row: 2049 (row, tile) pairs on 2048 workgroups
    x = capture((rows, 97), 3)
    taps = taps_of(T, 3)
    assert same_bytes(front_on_device(e, x, 240000.0, D, taps), Engine.h_rds_front(x, 240000.0, D, taps=taps))


def test_front_nan_row_and_far_index(e):
    D = 12
    x = capture((3, 5000), 4)
    x[1, 2500] = np.nan
    x[2, 100:200] = 0
    got, want = front_on_device(e, x, 240000.0, D, None), Engine.h_rds_front(x, 240000.0, D)
    assert np.isnan(want[1]).any() and same(got, want)
    assert same_bytes(got[[0, 2]], want[[0, 2]])                     # the NaN stays in its row
    # the last 5000 samples of a row of more than 2^40
    big = 2 ** 40 + 777
    index0 = big - 5000
    taps = Engine.ddc_default_taps(D)
    m0, m1 = -(-(index0 + 1 + 120) // D), -(-big // D)
    want = Engine.h_rds_front(x[:1], 240000.0, D, buf_index0=index0, n_capture=big, m_begin=m0, m_end=m1)
    assert same_bytes(front_on_device(e, x[:1], 240000.0, D, taps, m0, m1, index0, big), want)


def test_front_table_cache(e):
    """tests/test_gpu_table_cache.py's pattern: a table, the same again, a larger one, the first once more."""
    x = capture((1, 4001), 5)
    tab = {"A": taps_of(41, 1), "B": taps_of(81, 2)}
    for call, k in enumerate("AABA"):
        assert same_bytes(front_on_device(e, x, 240000.0, 4, tab[k]), Engine.h_rds_front(x, 240000.0, 4, taps=tab[k])), (call, k)


def baseband(name):
    iq, _ = R.case_iq(name)
    D, up, down = Engine.rds_plan(R.CASES[name][0])
    return Engine.h_resample(Engine.h_rds_front(iq, R.CASES[name][0], D), up, down)


def bits_on_device(e, rows, n, pulse=None, max_bits=None):
    """rows [r][>= n] -> (bits uint8 [r][max_bits], n_bits) of the first n samples of each row."""
    r = rows.shape[0]
    max_bits = Engine.rds_max_bits(n) if max_bits is None else max_bits
    d_bits = torch.full((r, max(max_bits, 1)), 7, dtype=torch.uint8, device="cuda")
    d_n = empty(r, torch.int32)
    e.rds_bits(dev(rows), r, n, d_bits, max_bits, d_n, pulse=pulse, row_stride=rows.shape[1])
    e.sync()
    return host(d_bits)[:, :max_bits], host(d_n)


def test_bits_are_the_twin(e):
    src = np.stack([baseband("fs240k_plain")[:9 * 1024 + 1], baseband("fs250k_slow_wrap")[:9 * 1024 + 1], capture(9 * 1024 + 1, 6)])
    src[2, 4000] = np.nan
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, 3000, 9 * 1024 - 1, 9 * 1024, 9 * 1024 + 1):
        bits, n_bits = bits_on_device(e, src, n)
        for r in range(3):
            want = Engine.h_rds_bits(src[r, :n])
            assert n_bits[r] == len(want) and np.array_equal(bits[r, :len(want)], want), (n, r)
            assert np.all(bits[r, len(want):] == 7)
    # the wrap cases whole, another pulse table, and fewer bits stored than found
    for name in ("fs240k_plain", "fs400k_fast_clock", "fs250k_slow_wrap"):
        bb = baseband(name)[None, :]
        for pulse in (None, Engine.rds_default_pulse(8), np.ones(1)):
            want = Engine.h_rds_bits(bb[0], pulse=pulse)
            bits, n_bits = bits_on_device(e, bb, bb.shape[1], pulse=pulse)
            assert n_bits[0] == len(want) and np.array_equal(bits[0, :len(want)], want), name
        want = Engine.h_rds_bits(bb[0])
        bits, n_bits = bits_on_device(e, bb, bb.shape[1], max_bits=100)
        assert n_bits[0] == len(want) > 100 and np.array_equal(bits[0], want[:100])


def groups_on_device(e, bits, n_bits, max_groups):
    r, max_bits = bits.shape
    d_g = torch.full((r, max(max_groups, 1), 4), -1, dtype=torch.int16, device="cuda")
    d_pos = torch.full((r, max(max_groups, 1)), -1, dtype=torch.int32, device="cuda")
    d_n = empty(r, torch.int32)
    e.rds_groups(dev(bits), dev(np.asarray(n_bits, np.int32)), r, max_bits, d_g, d_pos, max_groups, d_n)
    e.sync()
    return host(d_g).view(np.uint16)[:, :max_groups], host(d_pos)[:, :max_groups], host(d_n)


def test_groups_are_the_twin(e):
    tx = R.station_groups()
    stream = R.group_bits(tx)                                         # eight groups back to back: 832 bits
    rng = np.random.default_rng(59)
    wrong = stream[:104].copy()                                       # A B C D with the version bit of block 2 turned: C where C' belongs
    info = int(tx[0, 1]) | 0x0800
    wrong[26:52] = R.block_bits(info, R.OFFSETS['B'])
    max_bits = 1100
    rows = np.zeros((6, max_bits), np.uint8)
    n_bits = np.array([832, 832 + 7 - 1, 700, 104, 1100, 103], np.int32)
    rows[0, :832] = stream
    rows[1, 7:7 + 832] = stream                                       # the last group is cut by the row's end, one bit short
    rows[2, :832] = stream                                            # n_bits stops inside the seventh group; what lies behind it is not read
    rows[3, :104] = wrong
    rows[4] = rng.integers(0, 2, max_bits)
    rows[4, 300:404] = stream[104:208]
    rows[5, :104] = stream[:104]
    for max_groups in (8, 3, 0):
        got, pos, n = groups_on_device(e, rows, n_bits, max_groups)
        want, wpos, wn = Engine.h_rds_groups(rows, n_bits, max_groups=max_groups)
        assert np.array_equal(n, wn) and wn.tolist() == [8, 7, 6, 0, 1, 0]
        for r in range(6):
            k = min(int(wn[r]), max_groups)
            assert np.array_equal(got[r, :k], want[r, :k]) and np.array_equal(pos[r, :k], wpos[r, :k]), (max_groups, r)
            assert np.all(got[r, k:] == 0xFFFF) and np.all(pos[r, k:] == -1)
    got, pos, n = groups_on_device(e, rows, n_bits, 8)
    assert np.array_equal(got[0], tx) and pos[0].tolist() == [104 * k for k in range(8)] and pos[4, 0] == 300
    # more positions than one pass of the workgroup, groups in several wavefronts of a pass
    long_row = np.tile(stream, 5)[None, :]
    got, pos, n = groups_on_device(e, long_row, [long_row.shape[1]], 64)
    want, wpos, wn = Engine.h_rds_groups(long_row, max_groups=64)
    assert n[0] == wn[0] == 40 and np.array_equal(got[0, :40], want[0, :40]) and np.array_equal(pos[0, :40], wpos[0, :40])


@pytest.mark.parametrize("name", NAMES)
def test_chain_from_iq_gives_the_golden_groups(e, name):
    iq, _ = R.case_iq(name)
    fs = R.CASES[name][0]
    tx = GOLD[name + "/groups"]
    out = F.rds_recording(iq, fs)
    idx = R.find_groups(tx, out["groups"])
    assert idx is not None and set(range(1, len(tx) - 1)) <= set(idx), idx
    D, up, down = Engine.rds_plan(fs)
    want, wpos, wn = Engine.h_rds_groups(Engine.h_rds_bits(Engine.h_resample(Engine.h_rds_front(iq, fs, D), up, down)))
    assert np.array_equal(out["groups"], want[:wn]) and np.array_equal(out["pos"], wpos[:wn])
    if name == "fs240k_plain":
        assert (out["pi"], out["ps"], out["radiotext"]) == (R.PI, R.PS, R.RADIOTEXT)
        cut = F.rds_recording(iq, fs, chunk_samples=50000)           # four chunks: the same groups at the same bits
        assert np.array_equal(cut["groups"], out["groups"]) and np.array_equal(cut["pos"], out["pos"])


def test_stations_of_a_band_capture(e):
    stations = [(-700e3, 0x1111, "STATION1"), (100e3, 0x2222, "RADIO 22"), (900e3, 0x3333, "THIRD FM")]
    x = R.band_capture(stations)
    got = F.rds_stations(x, 2.4e6, 98.0e6)
    assert got == [(98.0e6 + f, pi, ps, R.RADIOTEXT, 8) for f, pi, ps in stations]


def test_drop_in_hooks(e):
    import pyspecsdr_amd.signal_processing as sp
    iq, _ = R.case_iq("fs240k_plain")
    demod = np.angle(iq[1:] * np.conj(iq[:-1]))
    bb, rate = sp.extract_rds(demod, 240000)
    assert rate == 19000 and bb.dtype == np.complex64
    bits = sp.demodulate_rds_bpsk(bb, rate)
    groups, _, n = Engine.h_rds_groups(np.array(bits, np.uint8))
    idx = R.find_groups(GOLD["fs240k_plain/groups"], groups[:n])
    assert idx is not None and set(range(1, 7)) <= set(idx)


# ---- past the grid caps of k_rds_energy, k_rds_bits and k_rds_groups, and past one pass of k_rds_bits' scan
def test_bits_one_row_past_each_grid_cap(e):
    """16 385 rows of two segments: one energy tile a row, so k_rds_energy is one tile past its cap, and every workgroup of k_rds_bits
    walks four or five rows, resetting its carry for each.  The rows repeat a pool of seven, so a row that took its neighbour's offsets,
    prefix or carry shows."""
    rows, n = EN_GRID_CAP + 1, 1100
    assert RECEIVER_CAPS["rds_energy"].cover(n) == EN_GRID_CAP and rows > 4 * BT_GRID_CAP and RDS_SEGMENT < n <= 2 * RDS_SEGMENT
    pulse = Engine.rds_default_pulse(1)
    assert len(pulse) == 17
    pool = []
    for name in ("fs240k_plain", "fs400k_fast_clock", "fs250k_slow_wrap"):
        bb = baseband(name)
        pool += [bb[:n], bb[3000:3000 + n]]
    pool.append(capture(n, 7))
    pool = np.stack(pool)
    assert len({row.tobytes() for row in pool}) == 7
    want = Engine.h_rds_bits(pool, pulse=pulse)                      # the twin walks its rows one by one: row r's bits are pool row r % 7's
    assert len({w.tobytes() for w in want}) > 1 and all(60 <= len(w) <= 70 for w in want)
    max_bits = Engine.rds_max_bits(n)
    bits, n_bits = bits_on_device(e, pool[np.arange(rows) % 7], n, pulse=pulse)
    assert bits.shape == (rows, max_bits)
    full = np.full((7, max_bits), 7, np.uint8)                       # the sentinel behind n_bits
    for k, w in enumerate(want):
        full[k, :len(w)] = w
    idx = np.arange(rows) % 7
    assert np.array_equal(n_bits, np.array([len(w) for w in want], np.int32)[idx])
    bad = np.flatnonzero((bits != full[idx]).any(axis=1))
    assert len(bad) == 0, bad[:10]


def test_bits_more_segments_than_one_pass_of_the_scan(e):
    """A row of 258 segments (13.8 s of baseband): the strobe counts' prefix carries into a second pass of 256 segments."""
    n = (BITS_SCAN_PASS + 1) * RDS_SEGMENT + 17
    bb = baseband("fs240k_plain")
    long_row = np.tile(bb, -(-(n + 5) // len(bb)))                   # the joins move the timing: wanted
    for src in (long_row[None, :n], np.stack([long_row[:n], long_row[5:5 + n]])):
        want = Engine.h_rds_bits(src)
        assert all(len(w) > 16000 for w in want)
        bits, n_bits = bits_on_device(e, src, n)
        for r, w in enumerate(want):
            assert n_bits[r] == len(w) and np.array_equal(bits[r, :len(w)], w), r
            assert np.all(bits[r, len(w):] == 7)
        # and the groups of those bits, from the device's rows as they stand (the sentinels lie behind n_bits)
        got, pos, n_groups = groups_on_device(e, bits, n_bits, 200)
        wg, wpos, wn = Engine.h_rds_groups(bits, n_bits, max_groups=200)
        assert np.array_equal(n_groups, wn) and np.all(wn > 100) and np.all(wn <= 200)
        for r in range(len(want)):
            k = int(wn[r])
            assert np.array_equal(got[r, :k], wg[r, :k]) and np.array_equal(pos[r, :k], wpos[r, :k])
            assert np.all(got[r, k:] == 0xFFFF) and np.all(pos[r, k:] == -1)


def test_groups_one_row_past_the_grid_cap(e):
    rows, max_bits, max_groups = GR_GRID_CAP + 1, 130, 2
    stream = R.group_bits(R.station_groups())[:104]
    r = np.arange(rows)
    offset, n_bits = r % 23, (104 + r % 27).astype(np.int32)
    bits = np.zeros((rows, max_bits), np.uint8)
    for k in range(rows):
        bits[k, offset[k]:offset[k] + 104] = stream
    fits = offset + 104 <= n_bits
    assert fits[-1] and fits[:GR_GRID_CAP].any() and not fits.all()   # the row past the cap holds a group
    got, pos, n_groups = groups_on_device(e, bits, n_bits, max_groups)
    wg, wpos, wn = Engine.h_rds_groups(bits, n_bits, max_groups=max_groups)
    assert np.array_equal(wn, fits.astype(np.int32)) and np.array_equal(n_groups, wn)
    assert np.array_equal(pos[fits, 0], offset[fits]) and np.array_equal(got[fits, 0], wg[fits, 0])
    assert np.all(got[fits, 0] == R.station_groups()[0])
    assert np.all(pos[fits, 1:] == -1) and np.all(pos[~fits] == -1) and np.all(got[fits, 1:] == 0xFFFF) and np.all(got[~fits] == 0xFFFF)

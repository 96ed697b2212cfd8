"""The one start list (csrc/pss_starts.h: ctx->starts, two grow-only buffers and one pinned word) behind pss_apt_syncs, pss_pocsag_batches,
pss_adsb_frames and pss_ais_frames: all four in turn on ONE context, every call against its host twin on every byte of every output and
the count (the check() of each receiver's own GPU suite, which also lays the input between NaNs and a sentinel behind every output).

What a receiver can get wrong here and nowhere else: it reads a tile's count, offset or list that another receiver left in buffer 0; it
lays its arrays over buffer 1 as if the buffer were its own size; it keeps a pointer across a regrowth; it leaves the list in a state the
next receiver trips over after an early return (no survivor, an empty window) or a refused call.  Each test states its calls as a table:
the receiver, the tiles (buffer 0 holds 16 + 8 tiles bytes rounded up to 16, and 8192 bytes a tile) and the listed starts (buffer 1 holds
LIST_BYTES of the receiver a start).  Both buffers grow to exactly what a call asks for and never shrink (pss_ensure_buffer), so the
table itself says which call makes, grows or reuses which buffer, and the test asserts that from the table before it runs a call.  Inputs
are a few tiles each; the caps and the bytes a start come from tests/apt_caps.py, tests/pocsag_caps.py, tests/ais_caps.py and
tests/launch_caps.py, which the pin tests hold to the source."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adsb_cases as ADSB
import ais_caps
import ais_cases as AIS
import apt_caps
import apt_cases as A
import pocsag_caps
import pocsag_cases as P
import test_gpu_adsb as on_adsb          # on_device() and check() of each receiver's suite: device == twin on every byte, plus the count
import test_gpu_ais as on_ais
import test_gpu_apt as on_apt
import test_gpu_pocsag as on_pocsag
from gpu_util import dev
from launch_caps import ADSB_LIST_BYTES, DETECT_TILE as TILE
from pyspecsdr_amd.engine import Engine, PssError
from test_gpu_table_cache import adsb_capture, ais_rows

pytestmark = pytest.mark.gpu

BYTES = {"apt": apt_caps.LIST_BYTES, "pocsag": pocsag_caps.LIST_BYTES, "ais": ais_caps.LIST_BYTES, "adsb": ADSB_LIST_BYTES}
assert apt_caps.TILE == pocsag_caps.TILE == ais_caps.TILE == TILE


@pytest.fixture
def e():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    eng = Engine(0)
    yield eng
    eng.close()


def tiles_of(n_rows, n, near, s_begin=0, s_end=None):
    """Tiles of a call: the window with `near` - 1 starts either side, clipped to the row, in tiles of TILE starts, times the rows."""
    s_end = n if s_end is None else s_end
    e0, e1 = max(0, s_begin - (near - 1)), min(n, s_end + near - 1)
    return -(-(e1 - e0) // TILE) * n_rows


# ---- the inputs, each with its tiles and its listed starts counted on the host by the NumPy statement of the receiver's candidate test -------
def apt_sparse():
    """Two rows of three tiles, a sync on either side of a tile boundary and one more: three survivors at sync_errors 0."""
    n = 2 * TILE + 300
    env = np.stack([A.sync_env(n, [TILE - 1, TILE + 3500]), A.sync_env(n, [200])])
    listed = sum(len(A.candidates(r, 0)[0]) for r in env)
    return env, dict(sync_errors=0), tiles_of(2, n, A.NEAR), listed


def apt_dense():
    """One row of three tiles, full syncs back to back at sync_errors 4: nine survivors a sync, one record."""
    n = 3 * TILE
    env = A.sync_env(n, list(range(5, n - A.REACH, A.REACH)), full=True)
    return env, dict(sync_errors=4), tiles_of(1, n, A.NEAR), len(A.candidates(env, 4)[0])


def apt_constant():
    env = np.full(2 * TILE, 0.2, np.float32)
    return env, dict(sync_errors=4), tiles_of(1, len(env), A.NEAR), len(A.candidates(env, 4)[0])


def pocsag_listed(y, spb):
    stats = {}
    P.numpy_batches(y, spb, stats=stats)
    return stats["survivors"]


def pocsag_rows():
    """Three rows of five tiles at 16 samples a bit, one batch a row, the first across a tile boundary: three survivors."""
    spb = 16
    n = 2 * TILE + P.LAST_K * spb + 100
    y = np.stack([P.batch_row(spb, s, n, inverted=bool(k & 1)) for k, s in enumerate((TILE - 5, 2 * TILE + 50, 60))])
    return y, spb, tiles_of(3, n, spb), pocsag_listed(y, spb)


def pocsag_train():
    """Back-to-back sync words at 2 samples a bit over four tiles: two survivors a word."""
    y, _ = P.sync_train(200)
    return y, 2, tiles_of(1, len(y), 2), pocsag_listed(y, 2)


def pocsag_one():
    y = P.batch_row(2, 33, 3000)
    return y, 2, tiles_of(1, len(y), 2), pocsag_listed(y, 2)


def ais_listed(y):
    stats = {}
    AIS.numpy_frames(y, stats=stats)
    return stats["survivors"]


def adsb_listed(x, spc, **window):
    """ADS-B lists the ACCEPTED starts (preamble and parity): at least the frames the twin reports, at most the preamble's survivors."""
    stats = {}
    ADSB.numpy_frames(x, spc, stats=stats, **window)
    return stats["survivors"]


# ---- the ledger: which call makes, grows or reuses which buffer ----------------------------------------------------------------------------
class Ledger:
    def __init__(self):
        self.cap = [0, 0]
        self.rows = []

    def call(self, who, what, tiles, listed, reaches_list=True):
        """-> ('made' | 'grows' | 'reuses' | '-') for buffer 0 and buffer 1.  A refused call and an empty window touch neither buffer; a call
        without a listed start stops behind buffer 0."""
        need = [tiles, listed * BYTES[who] if reaches_list and listed else 0]
        if tiles == 0:
            need = [0, 0]
        said = []
        for b in range(2):
            if need[b] == 0:
                said.append("-")
            elif need[b] > self.cap[b]:
                said.append("made" if self.cap[b] == 0 else "grows")
                self.cap[b] = need[b]
            else:
                said.append("reuses")
        self.rows.append((len(self.rows), who, what, tiles, listed, need[1], said[0], said[1]))
        return said

    def show(self):
        print("\ncall  receiver  input                      tiles  listed  buffer 1 bytes  buffer 0  buffer 1")
        for k, who, what, tiles, listed, b1, s0, s1 in self.rows:
            print(f"{k:4d}  {who:8s}  {what:25s}  {tiles:5d}  {listed:6d}  {b1:14d}  {s0:8s}  {s1}")


def refused_pocsag(e):
    """spb = 1 is refused by the host check: the outputs keep their sentinels, the count included."""
    y = P.batch_row(16, 50, 50 + 544 * 16 + 20)
    out = [torch.full((4, 16), -7, dtype=torch.int32, device="cuda"), torch.full((4, 16), 0xA5, dtype=torch.uint8, device="cuda"),
           torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int64, device="cuda"),
           torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7.0, dtype=torch.float32, device="cuda"),
           torch.full((1,), -7, dtype=torch.int32, device="cuda")]
    with pytest.raises(PssError, match=re.escape("pss_pocsag_batches: spb outside [2, 128]")):
        e.pocsag_batches(dev(y), 1, len(y), 1, *out, 4)
    e.sync()
    assert bool((out[1] == 0xA5).all()) and all(bool((t == -7).all()) for t in out[:1] + out[2:])


def refused_apt(e):
    """sync_errors = 5 is refused by the host check: the outputs keep their sentinels, the count included."""
    env = A.sync_env(9000, [4000])
    out = [torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int64, device="cuda"),
           torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7.0, dtype=torch.float32, device="cuda"),
           torch.full((1,), -7, dtype=torch.int32, device="cuda")]
    with pytest.raises(PssError, match=re.escape("pss_apt_syncs: sync_errors outside [0, 4]")):
        e.apt_syncs(dev(env), 1, len(env), *out, 4, sync_errors=5)
    e.sync()
    assert all(bool((t == -7).all()) for t in out)


def test_every_receiver_in_turn_on_one_context(e):
    """APT first (so far the first user of a context's list has always been ADS-B), then the calls of the table this test prints: buffer 0
    grows under POCSAG and is reused by ADS-B and APT with POCSAG's counts and lists still in it; buffer 1 grows under the dense APT row,
    is regrown by POCSAG for FEWER starts that need MORE bytes, and is reused by APT with more starts than POCSAG listed; a call without a
    survivor, an empty window and two refused calls each stand between two calls that list starts."""
    led = Ledger()
    sparse, dense, constant = apt_sparse(), apt_dense(), apt_constant()
    rows16, train, one = pocsag_rows(), pocsag_train(), pocsag_one()
    x, spc, at = adsb_capture()
    window = {"s_begin": TILE - 1000, "s_end": TILE + 1000}
    ais3 = ais_rows(3)
    assert constant[3] == 0 and train[3] < dense[3] and train[3] * BYTES["pocsag"] > dense[3] * BYTES["apt"]

    # 0: first use, by APT
    assert led.call("apt", "2 rows, 3 syncs", sparse[2], sparse[3]) == ["made", "made"]
    r = on_apt.check(e, sparse[0], **sparse[1])
    assert r[0].tolist() == [0, 0, 1] and r[1].tolist() == [TILE - 1, TILE + 3500, 200]
    # 1: more tiles and more bytes: both buffers grow
    assert led.call("pocsag", "3 rows at spb 16", rows16[2], rows16[3]) == ["grows", "grows"]
    r = on_pocsag.check(e, rows16[0], rows16[1])
    assert r[2].tolist() == [0, 1, 2] and r[3].tolist() == [TILE - 5, 2 * TILE + 50, 60]
    # 2: fewer tiles: buffer 0 as POCSAG left it
    assert led.call("adsb", "3 frames", tiles_of(1, len(x), 2 * spc), adsb_listed(x, spc)) == ["reuses", "reuses"]   # (its bytes are an upper bound: they fit)
    assert on_adsb.check(e, x, spc)[1].tolist() == at
    # 3: a dense APT row: buffer 1 grows
    assert led.call("apt", "full syncs back to back", dense[2], dense[3]) == ["reuses", "grows"]
    assert on_apt.check(e, dense[0], **dense[1])[1].tolist() == [4]
    # 4: fewer starts, more bytes: buffer 1 regrown
    assert led.call("pocsag", "sync train at spb 2", train[2], train[3]) == ["reuses", "grows"]
    r = on_pocsag.check(e, train[0], train[1])
    assert r[6] == 200 - 16 and r[3].tolist() == [3 + 64 * k for k in range(200 - 16)]
    # 5: APT with more starts than POCSAG listed, in POCSAG's buffer
    assert led.call("apt", "full syncs back to back", dense[2], dense[3]) == ["reuses", "reuses"]
    assert on_apt.check(e, dense[0], **dense[1])[1].tolist() == [4]
    # 6: AIS
    assert led.call("ais", "3 rows, a burst each", tiles_of(3, ais3.shape[1], 5), ais_listed(ais3)) == ["reuses", "reuses"]
    assert on_ais.check(e, ais3)[2].tolist() == [0, 1, 2]
    # 7, 8: no survivor at all, then a call that has one
    assert led.call("apt", "a constant row", constant[2], 0) == ["reuses", "-"]
    assert on_apt.check(e, constant[0], **constant[1])[4] == 0
    assert led.call("pocsag", "one batch at spb 2", one[2], one[3]) == ["reuses", "reuses"]
    assert on_pocsag.check(e, one[0], one[1])[3].tolist() == [33]
    # 9, 10: an empty window, then a window of one tile
    assert led.call("ais", "s_begin == s_end", 0, 0) == ["-", "-"]
    assert on_ais.check(e, ais3, s_begin=7, s_end=7)[5] == 0
    assert led.call("adsb", "a window of 2000 starts", tiles_of(1, len(x), 2 * spc, **window), adsb_listed(x, spc, **window)) == ["reuses", "reuses"]   # (its bytes are an upper bound: they fit)
    assert on_adsb.check(e, x, spc, **window)[1].tolist() == at[1:2]
    # 11 .. 14: a refused call between two good ones, twice
    assert led.call("pocsag", "refused: spb 1", 0, 0) == ["-", "-"]
    refused_pocsag(e)
    assert led.call("ais", "2 rows, a burst each", tiles_of(2, ais3.shape[1], 5), ais_listed(ais3[:2])) == ["reuses", "reuses"]
    assert on_ais.check(e, ais3[:2])[2].tolist() == [0, 1]
    assert led.call("apt", "refused: sync_errors 5", 0, 0) == ["-", "-"]
    refused_apt(e)
    assert led.call("apt", "2 rows, 3 syncs", sparse[2], sparse[3]) == ["reuses", "reuses"]
    assert on_apt.check(e, sparse[0], **sparse[1])[1].tolist() == [TILE - 1, TILE + 3500, 200]
    led.show()
    assert [r[3] for r in led.rows] == [6, 15, 3, 3, 4, 3, 12, 2, 1, 0, 1, 0, 8, 0, 6]


def test_the_receivers_in_the_opposite_order(e):
    """POCSAG first; AIS grows buffer 0 behind it; ADS-B and APT reuse it; the dense APT row grows buffer 1 and the POCSAG train regrows it;
    then a call without a survivor, a window and the sparse APT rows in what the others left."""
    led = Ledger()
    sparse, dense, constant = apt_sparse(), apt_dense(), apt_constant()
    one, train = pocsag_one(), pocsag_train()
    x, spc, at = adsb_capture()
    window = {"s_begin": TILE - 1000, "s_end": TILE + 1000}
    ais3 = ais_rows(3)
    assert led.call("pocsag", "one batch at spb 2", one[2], one[3]) == ["made", "made"]
    assert on_pocsag.check(e, one[0], one[1])[3].tolist() == [33]
    assert led.call("ais", "3 rows, a burst each", tiles_of(3, ais3.shape[1], 5), ais_listed(ais3)) == ["grows", "grows"]
    assert on_ais.check(e, ais3)[2].tolist() == [0, 1, 2]
    assert led.call("adsb", "3 frames", tiles_of(1, len(x), 2 * spc), adsb_listed(x, spc)) == ["reuses", "reuses"]   # (its bytes are an upper bound: they fit)
    assert on_adsb.check(e, x, spc)[1].tolist() == at
    assert led.call("apt", "full syncs back to back", dense[2], dense[3]) == ["reuses", "grows"]
    assert on_apt.check(e, dense[0], **dense[1])[1].tolist() == [4]
    assert led.call("pocsag", "sync train at spb 2", train[2], train[3]) == ["reuses", "grows"]
    assert on_pocsag.check(e, train[0], train[1])[6] == 200 - 16
    assert led.call("apt", "a constant row", constant[2], 0) == ["reuses", "-"]
    assert on_apt.check(e, constant[0], **constant[1])[4] == 0
    assert led.call("adsb", "a window of 2000 starts", tiles_of(1, len(x), 2 * spc, **window), adsb_listed(x, spc, **window)) == ["reuses", "reuses"]   # (its bytes are an upper bound: they fit)
    assert on_adsb.check(e, x, spc, **window)[1].tolist() == at[1:2]
    assert led.call("apt", "2 rows, 3 syncs", sparse[2], sparse[3]) == ["reuses", "reuses"]
    assert on_apt.check(e, sparse[0], **sparse[1])[1].tolist() == [TILE - 1, TILE + 3500, 200]
    led.show()

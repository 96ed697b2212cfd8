"""The cached device tables of the channel family (pss_table_sync, csrc/pss_api.cpp): every member through four calls on one context —
a small table A, A again (nothing to upload), a table B with more bytes (the buffer regrows and the old pointer dies), A once more (an
upload into the larger buffer) — each result against the host twin of the same call.  The shapes are the smallest with a whole tile and
a partial one.  Nothing here counts uploads: a stale or a torn table shows in the outputs.  The last test is about the one start list
(csrc/pss_starts.h) behind pss_adsb_frames and pss_ais_frames: the two in turn on one context, its buffers regrown and reused."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adsb_cases as ADSB
import ais_cases as AIS
import welch_bounds as WB
import welch_cases as WC
from bytes_util import same, same_bytes
from gpu_util import dev, empty, host
from pyspecsdr_amd.engine import Engine, PssError

pytestmark = pytest.mark.gpu

ORDER = "AABA"   # A, A again, B (more bytes), A once more


def capture(n, seed):
    rng = np.random.default_rng([91, n, seed])
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.exp2(rng.integers(-3, 2, n))).astype(np.complex64)


def taps_of(T, seed):
    return np.random.default_rng([92, T, seed]).standard_normal(T) / np.sqrt(T)


@pytest.fixture
def e():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    eng = Engine(0)
    yield eng
    eng.close()


def test_ddc(e):
    n, D = 4001, 4
    x = capture(n, 1)
    words = [Engine.ddc_word(f, 1.0)[0] for f in (0.11, -0.23, 0.37)]
    tab = {"A": (taps_of(41, 1), words[:2]), "B": (taps_of(81, 2), words)}
    want = {k: Engine.h_ddc(x, w, D, taps=t) for k, (t, w) in tab.items()}
    d_iq = dev(x)
    n_out = want["A"].shape[1]
    for call, k in enumerate(ORDER):
        t, w = tab[k]
        d_out = empty((len(w), 2 * n_out), torch.float32)
        e.ddc(d_iq, n, w, D, d_out, taps=t)
        e.sync()
        assert same(host(d_out).view(np.complex64), want[k]), (call, k)


def channeliser(e, entry, twin, x, M, D, T, seed):
    """One call of pss_pfb / pss_bank with T taps of this seed, against its twin."""
    t = taps_of(T, seed)
    want = twin(x, M, D, taps=t)
    d_out = empty((M, 2 * want.shape[1]), torch.float32)
    entry(dev(x), len(x), M, D, d_out, taps=t)
    e.sync()
    return same(host(d_out).view(np.complex64), want)


def test_pfb(e):
    n, M, D = 4097, 8, 4                       # ceil(n / D) = 1025: tile_instants(8) = 1024 and one more
    assert -(-n // D) == 8192 // M + 1
    x = capture(n, 2)
    for call, k in enumerate(ORDER):
        assert channeliser(e, e.pfb, Engine.h_pfb, x, M, D, *{"A": (41, 1), "B": (161, 2)}[k]), (call, k)


def test_bank(e):
    n, M, D = 3401, 12, 5                      # ceil(n / D) = 681: tile_instants(12) = 8 (1024 // 12) = 680 and one more
    assert -(-n // D) == 8 * (1024 // M) + 1
    x = capture(n, 3)
    for call, k in enumerate(ORDER):
        assert channeliser(e, e.bank, Engine.h_bank, x, M, D, *{"A": (50, 1), "B": (241, 2)}[k]), (call, k)


def test_pfb_and_bank_alternating_with_one_tap_count(e):
    """pss_pfb and pss_bank in turn on one context, the same number of taps in both (other values): each unit has its own table."""
    x = capture(4097, 4)
    for call in range(4):
        if call % 2 == 0:
            assert channeliser(e, e.pfb, Engine.h_pfb, x, 8, 4, 41, 1), call
        else:
            assert channeliser(e, e.bank, Engine.h_bank, x[:3401], 12, 5, 41, 2), call


def test_resample(e):
    """up / down = 3 / 2 takes at most 32 * 3 + 1 = 97 taps (pss_resample.h: max_taps), so B is the longest table the call admits; a longer
    one (121) is refused by the device call and by the twin alike and leaves the cached table as it was."""
    up, down = 3, 2
    x = np.random.default_rng(93).standard_normal((2, 1001)).astype(np.float32)
    tab = {"A": taps_of(31, 1), "B": taps_of(97, 2)}
    d_x = dev(x)
    n_out = Engine.resample_out_len(x.shape[1], up, down)
    for call, k in enumerate(ORDER):
        d_y = empty((2, n_out), torch.float32)
        e.resample(d_x, np.float32, 2, x.shape[1], up, down, d_y, taps=tab[k])
        e.sync()
        assert same_bytes(host(d_y), Engine.h_resample(x, up, down, taps=tab[k])), (call, k)
        if call == 1:
            with pytest.raises(PssError, match="n_taps outside"):
                e.resample(d_x, np.float32, 2, x.shape[1], up, down, d_y, taps=taps_of(121, 3))
            with pytest.raises(ValueError, match="n_taps outside"):
                Engine.h_resample(x, up, down, taps=taps_of(121, 3))


def test_welch(e):
    n, fs = 2048, WC.FS
    x = np.stack([WC.signal("noise", n, 95), WC.signal("tone", n, 96)])
    d_iq = dev(x)
    for call, k in enumerate(ORDER):
        N, S = {"A": (256, 128), "B": (512, 256)}[k]
        d_mean, d_max = empty((2, N), torch.float64), empty((2, N), torch.float64)
        e.welch(d_iq, 2, n, N, S, d_mean, d_max, fs=fs)
        e.sync()
        mean, mx = host(d_mean), host(d_max)
        h_mean, h_max = Engine.h_welch(x, N, S, fs=fs)
        w = Engine.welch_default_window(N)
        scale = WC.scale_of(w, "density", fs)
        for r in range(2):
            b_mean, b_max = WB.bounds(WB.restate(x[r], N, S, w, True, scale), N, scale, WB.KAPPA_TWIN)
            f = max(WB.fraction(mean[r], h_mean[r], b_mean), WB.fraction(mx[r], h_max[r], b_max))
            print(f"call {call} ({k}), row {r}: fraction of the twin bound {f:.4f}")
            assert f <= 1.0, (call, k, r, f)


# ---- the start list that pss_adsb_frames and pss_ais_frames share -------------------------------------------------------------------------
TILE = 4096
assert ADSB.TILE == TILE and AIS.TILE == TILE


def adsb_capture():
    """spc 2, two tiles plus a frame's reach: a frame in the first tile, one across the tile boundary, one that starts in the third tile
    and ends a sample before the capture does."""
    spc = 2
    n = 2 * TILE + 241 * spc
    at = [100, TILE - 200, 2 * TILE + 1]
    frames = [(m, p, 10.0, 0.3 * k) for k, (m, p) in enumerate(zip((ADSB.IDENT, ADSB.POS_EVEN, ADSB.VELOCITY), at))]
    return ADSB.synth(n, spc, frames, seed=[94, 1]), spc, at


def ais_rows(n_rows):
    """Rows of two tiles plus a start's reach at 48 kS/s through the front's twin, one burst a row: the first flag a few samples in front of
    the tile boundary, the others further on."""
    n = 2 * TILE + AIS.REACH
    at = [TILE - AIS.SPB * (AIS.TRAINING + 1), 6000, 300][:n_rows]
    x = np.stack([AIS.synth(n, [(AIS.with_crc(AIS.SHIPS[k]), a, 1.0, 150.0 * k)], snr_db=20.0, seed=[94, 2, k]) for k, a in enumerate(at)])
    return Engine.h_ais_front(x)


def adsb_on_device(e, d_iq, n, spc, room, **window):
    out = [torch.full((room, 14), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((room,), -7, dtype=torch.int64, device="cuda"),
           torch.full((room,), -7, dtype=torch.int32, device="cuda"), torch.full((room,), -7.0, dtype=torch.float32, device="cuda")]
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    e.adsb_frames(d_iq, n, spc, *out, d_count, room, **window)
    e.sync()
    count = int(host(d_count)[0])
    return [host(t)[:min(count, room)] for t in out], count


def ais_on_device(e, y, room):
    out = [torch.full((room, 128), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((room,), -7, dtype=torch.int32, device="cuda"),
           torch.full((room,), -7, dtype=torch.int32, device="cuda"), torch.full((room,), -7, dtype=torch.int64, device="cuda"),
           torch.full((room,), -7.0, dtype=torch.float32, device="cuda")]
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    e.ais_frames(dev(y), y.shape[0], y.shape[1], *out, d_count, room)
    e.sync()
    count = int(host(d_count)[0])
    return [host(t)[:min(count, room)] for t in out], count


def test_adsb_and_ais_alternating_on_one_start_list(e):
    """pss_adsb_frames (3 tiles: the list's buffers are made), pss_ais_frames on two rows (8 tiles: they grow), pss_adsb_frames through a
    smaller window (1 tile: reused as they are, the other receiver's bytes still in them), pss_ais_frames on three rows (12 tiles: they grow
    again) — every field and the count of each call against its host twin."""
    room = 8
    x, spc, at = adsb_capture()
    d_iq = dev(x)
    rows = ais_rows(3)
    for call, window in ((0, {}), (2, {"s_begin": TILE - 1000, "s_end": TILE + 1000})):
        want = Engine.h_adsb_frames(x, spc, max_frames=room, **window)
        assert want[1].tolist() == (at if call == 0 else at[1:2]) and want[4] == len(want[1]), (call, want[1], want[4])
        got, count = adsb_on_device(e, d_iq, len(x), spc, room, **window)
        assert count == want[4], (call, count, want[4])
        for g, w, what in zip(got, want[:4], ("msg", "pos", "meta", "score")):
            assert same_bytes(g.view(w.dtype), w), (call, what, g, w)
        y = rows[:2] if call == 0 else rows
        want = Engine.h_ais_frames(y, max_frames=room)
        assert want[2].tolist() == list(range(len(y))) and want[5] == len(y), (call, want[2], want[5])   # one burst a row, and nothing else
        got, count = ais_on_device(e, y, room)
        assert count == want[5], (call + 1, count, want[5])
        for g, w, what in zip(got, want[:5], ("msg", "len", "row", "pos", "score")):
            assert same_bytes(g, w), (call + 1, what, g, w)

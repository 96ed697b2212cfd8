"""The band-plan channeliser on the device: pss_bank (k_bank: grids of 2^a 3^b 5^c channels) against the host twin pss_h_bank, which
tests/test_bank_golden.py pins to the 80-bit truth and to pss_h_ddc without a GPU.

Device against twin: bit for bit (both run the statements of pyspecsdr_amd/csrc/pss_bank.h; the sign of a zero is not part of the
contract, so +0 and -0 compare equal and everything else by its bits).  The goldens go through the device under the statement's bound.
The shapes come from the launch constants restated below: the workgroup's threads, the items of a thread, the instants of a tile and
the grid cap.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bytes_util import same
import bank_cases as BC
from gpu_util import engine
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine, PssError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

SWEEP_M = [3, 5, 6, 9, 10, 12, 15, 18, 20, 24, 25, 27, 30, 45, 48, 60, 75, 81, 96, 100, 120, 125, 192, 240, 243, 250, 384, 400, 625, 729, 768,
           800, 960, 1000]


def launch_constants():
    """The constants of pyspecsdr_amd/csrc/pss_bank.h and pss_bank.hip that shape a launch, each beside the source line it restates."""
    return {
        "BANK_T": (1024, "pss_bank.h", "constexpr int BANK_T = 1024;"),            # threads: W = M (BANK_T // M) of them work in phases 1 and 2
        "ITEMS": (8, "pss_bank.h", "constexpr int ITEMS = 8;"),                    # (instant, branch) pairs of a thread, BANK_T // M instants apart
        "TILE_SLOTS": (9520, "pss_bank.h", "constexpr int TILE_SLOTS = 9520;"),    # float64 slots of each part of the tile in LDS
        "BANK_GRID_CAP": (1024, "pss_bank.hip", "constexpr long BANK_GRID_CAP = 1024;"),   # tiles of one pass of the grid
    }


K = {k: v[0] for k, v in launch_constants().items()}


def tile_instants(M):
    return K["ITEMS"] * (K["BANK_T"] // M)


def test_launch_constants_read_as_restated():
    src = {f: open(os.path.join(ROOT, "pyspecsdr_amd", "csrc", f)).read() for f in ("pss_bank.h", "pss_bank.hip")}
    for name, (_, f, line) in launch_constants().items():
        assert line in src[f], f"{f} no longer reads `{line}`: restate {name} here"
    for line in ("inline int tile_group(int M) { return BANK_T / M; }", "inline int tile_instants(int M) { return ITEMS * tile_group(M); }",
                 "inline int tile_row(int M) { return M | 1; }"):
        assert line in src["pss_bank.h"], line
    for line in ("for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {", "for (int i = 0; i < ITEMS; i++) {", "const bool act = tid < M * G;",
                 "dim3((unsigned)(n_tiles < BANK_GRID_CAP ? n_tiles : BANK_GRID_CAP)), dim3(BANK_T)"):
        assert line in src["pss_bank.hip"], line
    assert tile_instants(3) == 2728 and tile_instants(192) == 40 and tile_instants(1000) == 8
    for M in SWEEP_M:                                  # the tile fits its LDS image with rows an odd number of slots apart
        assert tile_instants(M) * (M | 1) <= K["TILE_SLOTS"] and tile_instants(M) * M <= 8192, M


CANARY = np.float32(-7.25)


def device_bank(buf, M, D, taps=None, pad=3, **kw):
    """buf (complex64 window of the capture) through pss_bank -> complex64 [M][m_end - m_begin].  d_iq starts one complex sample (8 bytes)
    into its allocation, so no load may assume more than a sample's alignment; the rows of d_out are `pad` elements apart beyond their
    length, and a canary fills everything beforehand: what lies between the rows must survive."""
    e = engine()
    buf = np.ascontiguousarray(buf, np.complex64)
    flat = np.zeros(2 * len(buf) + 2, np.float32)
    flat[2:] = buf.view(np.float32)
    d_all = torch.from_numpy(flat).cuda()
    d_iq = d_all[2:]
    assert d_iq.data_ptr() % 16 == 8
    taps_a, a, b, width = Engine._bank_args(e.lib, len(buf), M, D, taps, kw.get("buf_index0", 0), kw.get("n_capture"), kw.get("lead"),
                                            kw.get("m_begin", 0), kw.get("m_end"), None)
    stride = width + pad
    d_out = torch.full((M, 2 * stride), float(CANARY), dtype=torch.float32, device="cuda")
    e.bank(d_iq, len(buf), M, D, d_out, taps=taps_a, out_stride=stride, **kw)
    e.sync()
    out = d_out.cpu().numpy()
    assert np.all(out[:, 2 * width:] == CANARY), "the elements between the rows were written"
    return out[:, :2 * width].copy().view(np.complex64)


_BASE = None


def samples(n, seed=0):
    """n samples of one long random capture (amplitudes over a few binades), cut at an offset that depends on the seed."""
    global _BASE
    if _BASE is None:
        rng = np.random.default_rng(65)
        nb = 1 << 18
        _BASE = ((rng.standard_normal(nb) + 1j * rng.standard_normal(nb)) * np.exp2(rng.integers(-3, 2, nb))).astype(np.complex64)
    o = (seed * 7919) % 1000
    assert o + n <= len(_BASE)
    return _BASE[o:o + n]


def taps_of(T, seed=0):
    rng = np.random.default_rng([66, T, seed])
    return rng.standard_normal(T) / np.sqrt(T)


def non_divisor(M):
    """A decimation in (1, M) that does not divide M: 7 (no 5-smooth M has it) where it fits, else the smallest."""
    return 7 if M > 7 else next(d for d in range(2, M) if M % d)


# (M, D, T, lead, n_out wanted, slack): n_capture = (n_out - 1) D + 1 + slack, slack < D.  Output counts R - 1, R, R + 1 (one instant short
# of a tile — its tail empty —, exactly one tile, one instant into a second tile), 2 R + 1 and 2 R + 4 (three tiles); with lead = 0 the first
# outputs' spans start before sample 0, with lead = T - 1 the last outputs' spans end after n_capture; in the three-tile cases the middle tile's
# spans lie inside the capture (the kernel's untested loads) while the first and the last do not: once with D = M, where every item of a
# thread has the same branch, and once with D = M - 1, which divides no M > 2, so that the untested loads' addressing and the stepping of the
# branch from item to item run for every factorisation.
def sweep_cases():
    c = []
    for M in SWEEP_M:
        R, nd, half = tile_instants(M), non_divisor(M), max(M // 2, 1)
        c += [(M, M, 1, 0, R + 1, 0),
              (M, 1, M - 1, M - 2, R - 1, 0),
              (M, nd, M, 0, R, nd - 1),
              (M, M, M + 1, 0, 2 * R + 1, min(2, M - 1)),
              (M, half, 20 * M + 1, 10 * M, R + 1, 0),
              (M, nd, 32 * M, 32 * M - 1, R + 1, 1),
              (M, M, 4 * M + 3, 2 * M, 2 * R + 4, 0),
              (M, M - 1, 4 * M + 3, 2 * M, 2 * R + 4, 0),
              (M, half, M + 1, M, R, half - 1)]
    return c


def test_the_sweep_holds_every_shape_the_contract_names():
    cases = sweep_cases()
    want = {3, 5, 6, 9, 10, 12, 15, 18, 20, 24, 25, 27, 30, 45, 48, 60, 75, 81, 96, 100, 120, 125, 192, 240, 243, 250, 384, 400, 625, 729, 768, 800, 960, 1000}
    assert {c[0] for c in cases} == want and all(BC.bank_ok(M) and M & (M - 1) for M in want)
    for M in want:
        mine = [c for c in cases if c[0] == M]
        R = tile_instants(M)
        assert {c[2] for c in mine} >= {1, M - 1, M, M + 1, 20 * M + 1, 32 * M}, M
        ds = {c[1] for c in mine}
        assert {1, M // 2 if M > 3 else 1, M} <= ds and any(1 < d < M and M % d for d in ds), M
        assert any(c[3] == 0 for c in mine) and any(c[3] == c[2] - 1 and c[2] > 1 for c in mine), M
        assert {c[4] - R for c in mine} >= {-1, 0, 1}, M
        assert all(2 <= -(-c[4] // R) <= 3 or c[4] <= R for c in mine), M
        # a whole tile whose every span lies inside the capture: tile 1 of the (M, D, 4 M + 3, 2 M, 2 R + 4) cases, D = M and D = M - 1 (which
        # does not divide M, and moves the branch by a step other than 0 from one item of a thread to the next)
        for D in (M, M - 1):
            T, lead, n_out = 4 * M + 3, 2 * M, 2 * R + 4
            n = (n_out - 1) * D + 1
            assert (M, D, T, lead, n_out, 0) in mine and R * D + lead - (T - 1) >= 0 and (2 * R - 1) * D + lead < n, M
        assert M % (M - 1) and (K["BANK_T"] // M) * (M - 1) % M, M
    assert any(c[1] > 1 and ((c[4] - 1) * c[1] + 1 + c[5]) % c[1] for c in cases)


@pytest.mark.parametrize("M", SWEEP_M)
def test_device_equals_host_twin_over_the_sweep(M):
    bad = []
    for i, (m, D, T, lead, n_out, slack) in enumerate(sweep_cases()):
        if m != M:
            continue
        assert 0 <= slack < D and 1 <= D <= M and 0 <= lead < T
        n = (n_out - 1) * D + 1 + slack
        x, h = samples(n, i), taps_of(T, i)
        got = device_bank(x, M, D, h, lead=lead)
        want = Engine.h_bank(x, M, D, h, lead=lead)
        assert got.shape == (M, n_out)
        if not same(got, want):
            bad.append((M, D, T, lead, n, int(np.sum(got.view(np.uint32) != want.view(np.uint32)))))
    assert not bad, bad[:10]


@pytest.mark.parametrize("M, D, T, n, lead", [(192, 48, 700, 9001, 340), (45, 7, 300, 9001, 140)])
def test_windows_of_a_capture_and_the_call_shape_change_no_bit(M, D, T, n, lead):
    """[m_begin, m_end) split at arbitrary points; the capture fed as buffers of awkward lengths with exactly the halo each needs
    (buf_index0 > 0) — all against the one call on the whole capture, and that against the twin."""
    x, h = samples(n, 5), taps_of(T, 5)
    n_out = -(-n // D)
    R = tile_instants(M)
    whole = device_bank(x, M, D, h, lead=lead)
    assert same(whole, Engine.h_bank(x, M, D, h, lead=lead))
    cuts = [0, 1, 2, R - 1, R, R + 1, 2 * R + 3, n_out - 1, n_out]
    assert cuts == sorted(set(cuts))
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert same(device_bank(x, M, D, h, lead=lead, m_begin=a, m_end=b), whole[:, a:b]), (a, b)
        lo, hi = max(0, a * D + lead - (T - 1)), min(n, (b - 1) * D + lead + 1)        # exactly the samples these outputs need
        assert same(device_bank(x[lo:hi], M, D, h, lead=lead, buf_index0=lo, n_capture=n, m_begin=a, m_end=b), whole[:, a:b]), (a, b, lo, hi)


def test_a_window_past_2_to_the_40_in_a_capture_of_2_to_the_41():
    """The branch of an item follows from its 64-bit capture index modulo M = 240.  The remainder of a value above 2^32 is taken on the host
    (pss_bank hands the kernel (m_begin D + lead) mod M; the kernel's own 64-bit remainder is of m0 D, counted from m_begin, and stays
    small): what is pinned here is that hand-over and the kernel's 64-bit sample addressing — a remainder taken in 32 bits, or a mask, lands
    the sums in other branches."""
    M, D, T, lead, n_buf = 240, 7, 500, 130, 2500
    index0, n_cap = (1 << 40) + 12345, 1 << 41
    x, h = samples(n_buf, 9), taps_of(T, 9)
    a = -(-(index0 + (T - 1) - lead) // D)
    b = (index0 + n_buf - 1 - lead) // D + 1
    kw = dict(lead=lead, buf_index0=index0, n_capture=n_cap, m_begin=a, m_end=b)
    got = device_bank(x, M, D, h, **kw)
    assert got.shape == (M, b - a) and b - a > 2 * tile_instants(M)
    assert same(got, Engine.h_bank(x, M, D, h, **kw))
    assert (index0 % M, (index0 & 0xFFFFFFFF) % M) == (121, 105)         # what a 32-bit remainder would have made of it
    # the phase is the capture's: the same buffer at index 0 gives other bits
    assert not same(got[:, :100], device_bank(x, M, D, h, lead=lead, m_begin=60, m_end=160))


def test_one_tile_past_the_grid_cap():
    M, R = 1000, tile_instants(1000)
    n = K["BANK_GRID_CAP"] * R + 1                     # D = 1: as many outputs, one more than the grid's first pass holds
    assert n == 8193
    rng = np.random.default_rng(67)
    x = rng.integers(-512, 512, 2 * n).astype(np.float32).view(np.complex64)
    h = [0.75, -0.5, 0.25]
    got = device_bank(x, M, 1, h, lead=0)
    assert got.shape == (M, n)
    assert same(got, Engine.h_bank(x, M, 1, h, lead=0))
    # row 0 is the plain filter: exact on these inputs
    x0 = np.concatenate((np.zeros(2, np.complex64), x))
    assert np.array_equal(got[0], 0.75 * x0[2:] - 0.5 * x0[1:-1] + 0.25 * x0[:-2])


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "bank.npz"))


def test_golden_cases_through_the_device(g):
    worst = []
    for name, M, D, T, n, lead, _, _ in BC.CASES:
        x, h = BC.case_capture(name), BC.case_taps(name)
        ins, ch = BC.case_instants(name), BC.case_channels(name)
        if len(ins) == -(-n // D):
            y = device_bank(x, M, D, h, lead=lead)
            assert same(y, Engine.h_bank(x, M, D, h, lead=lead))
        else:
            a, b = min(ins), max(ins) + 1
            y = device_bank(x, M, D, h, lead=lead, m_begin=a, m_end=b)
            y = y[:, [m - a for m in ins]]
        y = y[ch]
        excess, used = BC.bound_excess(y, g[f"ref_hi_{name}"], g[f"ref_lo_{name}"], M, T, float(g[f"sumh_{name}"]), float(g[f"xmax_{name}"]))
        print(f"{name}: excess {excess:.3e}; error beyond the float32 half ulp: {used:.3f} of {BC.f64_units(M, T)} units")
        worst.append((excess, name))
    assert max(worst)[0] < 0, max(worst)


def test_a_power_of_two_is_the_polyphase_channelisers_bytes():
    e = engine()
    for M, D, T, n, lead in ((2, 2, 5, 9001, 2), (64, 24, 300, 9001, 140), (1024, 512, 2049, 9001, 1024)):
        x, h = samples(n, 11), taps_of(T, 11)
        n_out = -(-n // D)
        d_iq = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
        d_a = torch.full((M, 2 * n_out), float(CANARY), dtype=torch.float32, device="cuda")
        d_b = torch.full((M, 2 * n_out), float(CANARY), dtype=torch.float32, device="cuda")
        e.bank(d_iq, n, M, D, d_a, taps=h, lead=lead)
        e.pfb(d_iq, n, M, D, d_b, taps=h, lead=lead)
        e.sync()
        assert torch.equal(d_a.view(torch.int32), d_b.view(torch.int32)), M
        assert np.array_equal(device_bank(x, M, D, h, lead=lead).view(np.uint32), d_b.cpu().numpy().view(np.uint32)), M


def audio_peak(pcm):
    """The largest bin of a 2048-sample audio spectrum (left channel, Hann window, the two DC bins dropped)."""
    a = pcm[:2048, 0].astype(np.float64)
    spec = np.abs(np.fft.rfft(a * np.hanning(len(a))))
    spec[:2] = 0
    return int(np.argmax(spec))


@pytest.fixture(scope="module")
def chain(g):
    """Two NFM stations of one 2.4 MS/s capture on its 12.5 kHz grid: plan_bank -> (192, 48); Engine.bank (default taps) then
    demod_signal(NFM) of all 192 rows at 50 kS/s, without leaving the device."""
    from pyspecsdr_amd import formats as F
    x = BC.chain_capture()
    assert BC.crc(x) == int(g["chain_crc"]) and int(g["chain_seed"]) == BC.CHAIN_SEED
    assert F.plan_bank(BC.CHAIN_FS, BC.CHAIN_SPACING) == (BC.CHAIN_M, BC.CHAIN_D) == (192, 48)
    e = engine()
    M, D = BC.CHAIN_M, BC.CHAIN_D
    n_out = BC.CHAIN_N // D
    d_iq = torch.from_numpy(x.view(np.float32)).cuda()
    d_ch = torch.empty((M, 2 * n_out), dtype=torch.float32, device="cuda")
    e.bank(d_iq, len(x), M, D, d_ch)
    fs2 = BC.CHAIN_FS / D
    n_audio = e.demod_out_len(L.MODE_NFM, n_out, fs2)
    d_pcm = torch.empty((M, n_audio, 2), dtype=torch.int16, device="cuda")
    e.demod_signal(L.MODE_NFM, d_ch, M, n_out, fs2, d_pcm)
    e.sync()
    return {"x": x, "d_iq": d_iq, "channels": d_ch.cpu().numpy().view(np.complex64), "pcm": d_pcm.cpu().numpy(), "fs2": fs2, "n_out": n_out,
            "n_audio": n_audio}


def test_chain_hears_each_station_in_its_row_as_the_down_converter_does(chain, g):
    from pyspecsdr_amd import formats as F
    e = engine()
    M, D = BC.CHAIN_M, BC.CHAIN_D
    assert chain["fs2"] == 50000.0 and chain["pcm"].shape == (M, 3072, 2)
    h_ch = Engine.h_bank(chain["x"], M, D)
    assert same(chain["channels"], h_ch)
    # the PCM of all 192 rows against the CPU oracle on the twin's channels (demodulate_signal does not correct NFM buffers; the engine's
    # own tables at 50 kS/s, q = 2)
    import oracle_lib as O
    taps, sos, zi = e.nfm_filters(chain["fs2"])
    with np.errstate(all="ignore"):
        want = np.stack(O.map_frames(lambda row: O.pcm16_stereo(O.demod_nfm(row, chain["fs2"], taps, sos, zi)), list(h_ch)))
    assert np.array_equal(chain["pcm"], want), np.nonzero((chain["pcm"] != want).any(axis=(1, 2)))[0]
    rows =[row for _, row, _ in BC.CHAIN_STATIONS]
    assert rows == [24, 159] and F.plan_rows(BC.CHAIN_FS, 0.0, [off for off, _, _ in BC.CHAIN_STATIONS], BC.CHAIN_SPACING).tolist() == rows
    peaks = [audio_peak(chain["pcm"][r]) for r in rows]
    assert peaks == [int(b) for b in g["chain_bins"]] == [82, 205], peaks
    # the same two channels through pss_ddc with the bank's taps, then the same demodulator
    taps = Engine.bank_default_taps(M)
    words = [Engine.ddc_word(off, BC.CHAIN_FS)[0] for off, _, _ in BC.CHAIN_STATIONS]
    assert words == [(r << 64) // M for r in rows] and all((r << 64) % M == 0 for r in rows)   # both rows' words are exact
    d_dd = torch.empty((2, 2 * chain["n_out"]), dtype=torch.float32, device="cuda")
    e.ddc(chain["d_iq"], len(chain["x"]), words, D, d_dd, taps=taps)
    d_pcm = torch.empty((2, chain["n_audio"], 2), dtype=torch.int16, device="cuda")
    e.demod_signal(L.MODE_NFM, d_dd, 2, chain["n_out"], chain["fs2"], d_pcm)
    e.sync()
    dd, pcm = d_dd.cpu().numpy().view(np.complex64), d_pcm.cpu().numpy()
    for k, r in enumerate(rows):
        a, b = chain["channels"][r].view(np.uint32), dd[k].view(np.uint32)
        share = float(np.mean(a != b))
        diff = int(np.max(np.abs(chain["pcm"][r].astype(np.int32) - pcm[k].astype(np.int32))))
        print(f"row {r}: {100 * share:.3f} % of the complex64 parts differ from pss_ddc's, largest PCM difference {diff} LSB")
        if share == 0:
            assert np.array_equal(chain["pcm"][r], pcm[k])
        else:                                                   # the two statements round differently: a distance, not equality
            assert audio_peak(pcm[k]) == peaks[k] and diff <= 1


def test_channelize_plan_is_independent_of_the_chunking_and_takes_codes(chain):
    from pyspecsdr_amd import formats as F
    M, D = BC.CHAIN_M, BC.CHAIN_D
    span_and_tile = 20 * M + 1 + tile_instants(M) * D
    for chunk in (1000, 32 * 777, 1 << 22):
        ch, off, rate = F.channelize_plan(chain["x"], BC.CHAIN_FS, BC.CHAIN_SPACING, chunk_samples=chunk)
        assert rate == 50000.0 and ch.shape == chain["channels"].shape and np.array_equal(off, F.plan_offsets(BC.CHAIN_FS, M))
        assert np.array_equal(ch.view(np.uint32), chain["channels"].view(np.uint32)), chunk
    assert 1000 < span_and_tile and off[24] == 300e3 and off[159] == -412.5e3
    rng = np.random.default_rng(68)
    codes = rng.integers(0, 256, (30011, 2), dtype=np.uint8)
    wide = F.unpack_iq(codes, "cu8")
    one = device_bank(wide, 96, 96)
    ch, _, rate = F.channelize_plan(codes, BC.CHAIN_FS, 25e3, decim=96, chunk_samples=7001, codes_format="cu8")
    assert rate == BC.CHAIN_FS / 96 and np.array_equal(ch.view(np.uint32), one.view(np.uint32))


def test_monitor_channels_gives_the_listed_rows_of_the_whole_grid(chain):
    from pyspecsdr_amd import formats as F
    centre = 446.0e6
    listed = [centre + 300e3, centre - 412.5e3, centre + 37.5e3]
    pcm, rows, rate = F.monitor_channels(chain["x"], BC.CHAIN_FS, centre, listed, BC.CHAIN_SPACING, frame_len=chain["n_out"], chunk_samples=60000)
    assert rows.tolist() == [24, 159, 3] and rate == 50000.0 and pcm.shape == (3, 1, 3072, 2) and pcm.dtype == np.int16
    assert np.array_equal(pcm[:, 0], chain["pcm"][rows])               # those rows of demodulating all 192
    assert [audio_peak(pcm[0, 0]), audio_peak(pcm[1, 0])] == [82, 205]
    with pytest.raises(ValueError, match="446300040.0"):
        F.monitor_channels(chain["x"], BC.CHAIN_FS, centre, [centre + 300e3 + 40.0], BC.CHAIN_SPACING, frame_len=chain["n_out"])


def test_refused_arguments_leave_the_output_untouched():
    e = engine()
    n, M, D, T = 1000, 12, 5, 101
    x, h = samples(n, 1), taps_of(T, 1)
    d_iq = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    d_out = torch.full((M, 2 * 200), float(CANARY), dtype=torch.float32, device="cuda")
    good = dict(taps=h, buf_index0=0, n_capture=n, lead=50, m_begin=0, m_end=200, out_stride=200)
    nan_taps = h.copy()
    nan_taps[7] = np.nan
    bad = [dict(n_chan=0), dict(n_chan=7), dict(n_chan=14), dict(n_chan=1080), dict(n_chan=2048), dict(decim=0), dict(decim=M + 1), dict(taps=np.zeros(32 * M + 1)),
           dict(taps=np.zeros(0)), dict(taps=nan_taps), dict(taps=np.full(3, np.inf)), dict(lead=-1), dict(lead=T), dict(m_end=201), dict(m_begin=-1),
           dict(m_begin=5, m_end=4), dict(out_stride=199), dict(buf_index0=1), dict(n_capture=n - 1), dict(buf_index0=-1),
           dict(n_buf=n - 1),                        # the last outputs need a sample behind the buffer
           dict(d_iq=d_iq.data_ptr() + 4), dict(d_out=d_out.data_ptr() + 4), dict(d_iq=None), dict(d_out=None)]
    for b in bad:
        kw = dict(good)
        kw.update({k: v for k, v in b.items() if k in good})
        with pytest.raises(PssError) as err:
            e.bank(b.get("d_iq", d_iq), b.get("n_buf", n), b.get("n_chan", M), b.get("decim", D), b.get("d_out", d_out), **kw)
        assert err.value.code == L.PSS_E_ARG and "pss_bank: " in str(err.value), b
    e.sync()
    assert bool(torch.all(d_out == float(CANARY)))
    e.bank(d_iq, n, M, D, d_out, **good)
    e.sync()
    assert same(d_out.cpu().numpy().view(np.complex64), Engine.h_bank(x, M, D, h, lead=50))

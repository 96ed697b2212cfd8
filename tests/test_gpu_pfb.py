"""The polyphase channeliser on the device: pss_pfb (k_pfb) against the host twin pss_h_pfb, which tests/test_pfb_golden.py pins to the
80-bit truth and to pss_h_ddc without a GPU.

Device against twin: bit for bit (both run the statements of pyspecsdr_amd/csrc/pss_pfb.h; the sign of a zero is not part of the
contract, so +0 and -0 compare equal and everything else by its bits).  The goldens go through the device under the statement's bound.
The shapes come from the launch constants restated below: the (instant, branch) pairs of a tile, the row padding in LDS, the
workgroup's threads and the grid cap.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bytes_util import same
import pfb_cases as PC
from gpu_util import engine
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine, PssError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def launch_constants():
    """The constants of pyspecsdr_amd/csrc/pss_pfb.h and pss_pfb.hip that shape a launch, each beside the source line it restates."""
    return {
        "TILE_ELEMS": (8192, "pss_pfb.h", "constexpr int TILE_ELEMS = 8192;"),     # (instant, branch) pairs of a tile: R = TILE_ELEMS / M instants
        "PAD_FROM": (32, "pss_pfb.h", "constexpr int PAD_FROM = 32;"),             # rows M + 1 slots apart in LDS from this M on
        "PFB_T": (1024, "pss_pfb.hip", "constexpr int PFB_T = 1024;"),             # threads: a thread owns TILE_ELEMS / PFB_T pairs, PFB_T / M instants apart
        "PFB_GRID_CAP": (1024, "pss_pfb.hip", "constexpr long PFB_GRID_CAP = 1024;"),   # tiles of one pass of the grid
    }


K = {k: v[0] for k, v in launch_constants().items()}


def tile_instants(M):
    return K["TILE_ELEMS"] // M


def test_launch_constants_read_as_restated():
    src = {f: open(os.path.join(ROOT, "pyspecsdr_amd", "csrc", f)).read() for f in ("pss_pfb.h", "pss_pfb.hip")}
    for name, (_, f, line) in launch_constants().items():
        assert line in src[f], f"{f} no longer reads `{line}`: restate {name} here"
    for line in ("inline int tile_instants(int M) { return TILE_ELEMS / M; }", "inline int tile_row(int M) { return M >= PAD_FROM ? M + 1 : M; }"):
        assert line in src["pss_pfb.h"], line
    for line in ("for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {", "constexpr int PFB_ITEMS = TILE_ELEMS / PFB_T;", "for (int i = 0; i < PFB_ITEMS; i++) {",
                 "for (int q = tid; q < cnt * (M >> 1); q += PFB_T) {", "for (int e = tid; e < TILE_ELEMS; e += PFB_T) {",
                 "dim3((unsigned)(n_tiles < PFB_GRID_CAP ? n_tiles : PFB_GRID_CAP)), dim3(PFB_T)"):
        assert line in src["pss_pfb.hip"], line
    assert tile_instants(2) == 4096 and tile_instants(64) == 128 and tile_instants(1024) == 8


CANARY = np.float32(-7.25)


def device_pfb(buf, M, D, taps=None, pad=3, **kw):
    """buf (complex64 window of the capture) through pss_pfb -> complex64 [M][m_end - m_begin].  d_iq starts one complex sample (8 bytes)
    into its allocation, so no load may assume more than a sample's alignment; the rows of d_out are `pad` elements apart beyond their
    length, and a canary fills everything beforehand: what lies between the rows must survive."""
    e = engine()
    buf = np.ascontiguousarray(buf, np.complex64)
    flat = np.zeros(2 * len(buf) + 2, np.float32)
    flat[2:] = buf.view(np.float32)
    d_all = torch.from_numpy(flat).cuda()
    d_iq = d_all[2:]
    assert d_iq.data_ptr() % 16 == 8
    taps_a, a, b, width = Engine._pfb_args(e.lib, len(buf), M, D, taps, kw.get("buf_index0", 0), kw.get("n_capture"), kw.get("lead"),
                                           kw.get("m_begin", 0), kw.get("m_end"), None)
    stride = width + pad
    d_out = torch.full((M, 2 * stride), float(CANARY), dtype=torch.float32, device="cuda")
    e.pfb(d_iq, len(buf), M, D, d_out, taps=taps_a, out_stride=stride, **kw)
    e.sync()
    out = d_out.cpu().numpy()
    assert np.all(out[:, 2 * width:] == CANARY), "the elements between the rows were written"
    return out[:, :2 * width].copy().view(np.complex64)


_BASE = None


def samples(n, seed=0):
    """n samples of one long random capture (amplitudes over a few binades), cut at an offset that depends on the seed."""
    global _BASE
    if _BASE is None:
        rng = np.random.default_rng(61)
        nb = 1 << 18
        _BASE = ((rng.standard_normal(nb) + 1j * rng.standard_normal(nb)) * np.exp2(rng.integers(-3, 2, nb))).astype(np.complex64)
    o = (seed * 7919) % 1000
    assert o + n <= len(_BASE)
    return _BASE[o:o + n]


def taps_of(T, seed=0):
    rng = np.random.default_rng([62, T, seed])
    return rng.standard_normal(T) / np.sqrt(T)


def outs(M, k):
    """Output counts around a tile of R(M) instants: k = -1, 0, 1 -> R - 1, R, R + 1."""
    return tile_instants(M) + k


# (M, D, T, lead, n_out wanted, slack): n_capture = (n_out - 1) D + 1 + slack, slack < D, so n_capture is no multiple of D wherever
# D > 1 and slack != D - 1.  Every output count is R - 1, R, R + 1 (one tile short, full, one instant into a second tile) or 2 R + 1;
# with lead = 0 the first outputs' spans start before sample 0, with lead = T - 1 the last outputs' spans end after n_capture, and at
# T >= 2 both happen at the middle lead.
def sweep_cases():
    c = []
    # M = 2: one stage; T = 1, M, M + 1, 32 M; D = 1, M
    c += [(2, 2, 1, 0, outs(2, 1), 0), (2, 1, 2, 1, outs(2, -1), 0), (2, 2, 3, 0, outs(2, 0), 1), (2, 2, 64, 63, outs(2, 1), 0), (2, 1, 64, 31, 2 * outs(2, 0) + 1, 0)]
    # M = 8: D = M, M / 2, 1 and 3
    c += [(8, 8, 161, 80, outs(8, 1), 3), (8, 4, 161, 0, outs(8, 0), 1), (8, 1, 17, 16, outs(8, 1), 0), (8, 3, 50, 13, outs(8, 1), 1), (8, 3, 9, 0, outs(8, -1), 0),
          (8, 8, 1, 0, outs(8, 1), 5), (8, 8, 8, 7, outs(8, 0), 0)]
    # M = 16: the largest bank whose rows are not padded in LDS
    c += [(16, 8, 321, 160, outs(16, 1), 2), (16, 16, 17, 0, outs(16, -1), 0)]
    # M = 32, 64: several instants (M = 32) or one (M = 64) in a wavefront; the first padded rows
    c += [(32, 32, 32, 0, outs(32, 1), 7), (32, 16, 33, 32, outs(32, 0), 3), (32, 1, 641, 320, outs(32, 1), 0), (32, 32, 1, 0, outs(32, -1), 0)]
    c += [(64, 64, 64, 63, outs(64, 1), 9), (64, 32, 65, 0, outs(64, -1), 5), (64, 32, 2048, 1024, outs(64, 1), 0), (64, 64, 2048, 0, outs(64, 0), 63),
          (64, 3, 1281, 640, 2 * outs(64, 0) + 1, 1), (64, 64, 1, 0, outs(64, 1), 0)]
    # M = 128: an instant's branches cross wavefronts
    c += [(128, 128, 129, 0, outs(128, 1), 100), (128, 64, 2561, 1280, outs(128, 0), 0), (128, 1, 128, 127, outs(128, -1), 0), (128, 128, 1, 0, outs(128, 0), 0)]
    # M = 1024: the largest; T = 20 M + 1: the span (20 481 samples) is larger than LDS
    c += [(1024, 512, 20481, 10240, outs(1024, 1), 17), (1024, 1024, 20481, 0, outs(1024, -1), 0), (1024, 1024, 1, 0, outs(1024, 0), 3),
          (1024, 1024, 1024, 1023, outs(1024, 1), 1), (1024, 1, 1025, 512, 2 * outs(1024, 0) + 1, 0), (1024, 768, 32768, 32767, outs(1024, 0), 5)]
    return c


def test_the_sweep_holds_every_shape_the_contract_names():
    cases = sweep_cases()
    ms = {c[0] for c in cases}
    assert {2, 32, 64, 128, 1024} <= ms
    assert {(8, 8), (8, 4), (8, 1), (8, 3)} <= {(c[0], c[1]) for c in cases}
    for M in (2, 64):
        assert any(c[0] == M and c[2] == 32 * M for c in cases)
    for M in ms - {16}:
        assert any(c[0] == M and c[2] == 1 for c in cases), M                       # T = 1
        assert any(c[0] == M and c[2] == M for c in cases), M                       # one tap per branch
        assert any(c[0] == M and c[2] == M + 1 for c in cases), M                   # one branch has a second tap
        assert {c[4] - tile_instants(M) for c in cases if c[0] == M} >= {-1, 0, 1}, M
    assert any(c[:3] == (1024, 512, 20481) for c in cases) and 20481 * 8 > 160 * 1024
    assert any(c[3] == 0 for c in cases) and any(c[3] == c[2] - 1 and c[2] > 1 for c in cases)
    assert any(c[1] > 1 and ((c[4] - 1) * c[1] + 1 + c[5]) % c[1] for c in cases)


@pytest.mark.parametrize("M", sorted({c[0] for c in sweep_cases()}))
def test_device_equals_host_twin_over_the_sweep(M):
    bad = []
    for i, (m, D, T, lead, n_out, slack) in enumerate(sweep_cases()):
        if m != M:
            continue
        assert 0 <= slack < D
        n = (n_out - 1) * D + 1 + slack
        x, h = samples(n, i), taps_of(T, i)
        got = device_pfb(x, M, D, h, lead=lead)
        want = Engine.h_pfb(x, M, D, h, lead=lead)
        assert got.shape == (M, n_out)
        if not same(got, want):
            bad.append((M, D, T, lead, n, int(np.sum(got.view(np.uint32) != want.view(np.uint32)))))
    assert not bad, bad[:10]


def test_windows_of_a_capture_and_the_call_shape_change_no_bit():
    """[m_begin, m_end) split at arbitrary points; the capture fed as buffers of awkward lengths with exactly the halo each needs
    (buf_index0 > 0) — all against the one call on the whole capture, and that against the twin."""
    M, D, T, n, lead = 64, 24, 300, 9001, 140
    x, h = samples(n, 5), taps_of(T, 5)
    n_out = -(-n // D)
    whole = device_pfb(x, M, D, h, lead=lead)
    assert same(whole, Engine.h_pfb(x, M, D, h, lead=lead))
    cuts = [0, 1, 2, 127, 128, 129, 300, n_out - 1, n_out]
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert same(device_pfb(x, M, D, h, lead=lead, m_begin=a, m_end=b), whole[:, a:b]), (a, b)
        lo, hi = max(0, a * D + lead - (T - 1)), min(n, (b - 1) * D + lead + 1)        # exactly the samples these outputs need
        assert same(device_pfb(x[lo:hi], M, D, h, lead=lead, buf_index0=lo, n_capture=n, m_begin=a, m_end=b), whole[:, a:b]), (a, b, lo, hi)


def test_a_window_past_2_to_the_40_in_a_capture_of_2_to_the_41():
    M, D, T, lead, n_buf = 8, 3, 50, 13, 9000
    index0, n_cap = (1 << 40) + 12345, 1 << 41
    x, h = samples(n_buf, 9), taps_of(T, 9)
    a = -(-(index0 + (T - 1) - lead) // D)
    b = (index0 + n_buf - 1 - lead) // D + 1
    kw = dict(lead=lead, buf_index0=index0, n_capture=n_cap, m_begin=a, m_end=b)
    got = device_pfb(x, M, D, h, **kw)
    assert got.shape == (M, b - a) and b - a > 2 * tile_instants(M)
    assert same(got, Engine.h_pfb(x, M, D, h, **kw))
    # the phase is the capture's: the same buffer at index 0 gives other bits
    assert not same(got[:, :100], device_pfb(x, M, D, h, lead=lead, m_begin=20, m_end=120))


def test_one_tile_past_the_grid_cap():
    M, R = 2, tile_instants(2)
    n = K["PFB_GRID_CAP"] * R + 1                      # D = 1: as many outputs, one more than the grid's first pass holds
    rng = np.random.default_rng(63)
    x = rng.integers(-512, 512, 2 * n).astype(np.float32).view(np.complex64)
    got = device_pfb(x, M, 1, [0.75], lead=0)
    assert got.shape == (2, n)
    assert same(got[:, -3:], Engine.h_pfb(x[-3:], M, 1, [0.75], lead=0, buf_index0=n - 3, n_capture=n, m_begin=n - 3, m_end=n))
    # one tap, D = 1: row 0 is 0.75 x, row 1 is 0.75 x (-1)^m — exact on these inputs
    sign = 1.0 - 2.0 * (np.arange(n) & 1)
    assert np.array_equal(got[0], 0.75 * x) and np.array_equal(got[1], (0.75 * sign).astype(np.float32) * x)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "pfb.npz"))


def test_golden_cases_through_the_device(g):
    worst = []
    for name, M, D, T, n, lead, _, _ in PC.CASES:
        x, h = PC.case_capture(name), PC.case_taps(name)
        ins, ch = PC.case_instants(name), PC.case_channels(name)
        if len(ins) == -(-n // D):
            y = device_pfb(x, M, D, h, lead=lead)
            assert same(y, Engine.h_pfb(x, M, D, h, lead=lead))
        else:
            a, b = min(ins), max(ins) + 1
            y = device_pfb(x, M, D, h, lead=lead, m_begin=a, m_end=b)
            y = y[:, [m - a for m in ins]]
        y = y[ch]
        excess, used = PC.bound_excess(y, g[f"ref_hi_{name}"], g[f"ref_lo_{name}"], M, T, float(g[f"sumh_{name}"]), float(g[f"xmax_{name}"]))
        print(f"{name}: excess {excess:.3e}; error beyond the float32 half ulp: {used:.3f} of {PC.f64_units(M, T)} units")
        worst.append((excess, name))
    assert max(worst)[0] <= 0, max(worst)


def audio_peak(pcm):
    """The largest bin of a 2048-sample audio spectrum (left channel, Hann window, the two DC bins dropped)."""
    a = pcm[:2048, 0].astype(np.float64)
    spec = np.abs(np.fft.rfft(a * np.hanning(len(a))))
    spec[:2] = 0
    return int(np.argmax(spec))


@pytest.fixture(scope="module")
def chain(g):
    """Two NFM stations of one 2.4 MS/s capture on the grid of the M = 64 bank: Engine.pfb (D = 32, default taps) then demod_signal(NFM)
    of all 64 rows at 75 kS/s, without leaving the device."""
    x = PC.chain_capture()
    assert PC.crc(x) == int(g["chain_crc"]) and int(g["chain_seed"]) == PC.CHAIN_SEED
    e = engine()
    M, D = PC.CHAIN_M, PC.CHAIN_D
    n_out = PC.CHAIN_N // D
    d_iq = torch.from_numpy(x.view(np.float32)).cuda()
    d_ch = torch.empty((M, 2 * n_out), dtype=torch.float32, device="cuda")
    e.pfb(d_iq, len(x), M, D, d_ch)
    fs2 = PC.CHAIN_FS / D
    n_audio = e.demod_out_len(L.MODE_NFM, n_out, fs2)
    d_pcm = torch.empty((M, n_audio, 2), dtype=torch.int16, device="cuda")
    e.demod_signal(L.MODE_NFM, d_ch, M, n_out, fs2, d_pcm)
    e.sync()
    return {"x": x, "d_iq": d_iq, "channels": d_ch.cpu().numpy().view(np.complex64), "pcm": d_pcm.cpu().numpy(), "fs2": fs2, "n_out": n_out,
            "n_audio": n_audio}


def test_chain_hears_each_station_in_its_row_as_the_down_converter_does(chain, g):
    e = engine()
    M, D = PC.CHAIN_M, PC.CHAIN_D
    assert chain["fs2"] == 75000.0 and chain["pcm"].shape == (M, 2048, 2)
    h_ch = Engine.h_pfb(chain["x"], M, D)
    assert same(chain["channels"], h_ch)
    # the PCM of all 64 rows against the CPU oracle on the twin's channels (demodulate_signal does not correct NFM buffers; the engine's
    # own tables at 75 kS/s, q = 3)
    import oracle_lib as O
    taps, sos, zi = e.nfm_filters(chain["fs2"])
    with np.errstate(all="ignore"):
        want = np.stack(O.map_frames(lambda row: O.pcm16_stereo(O.demod_nfm(row, chain["fs2"], taps, sos, zi)), list(h_ch)))
    assert np.array_equal(chain["pcm"], want), np.nonzero((chain["pcm"] != want).any(axis=(1, 2)))[0]
    rows =[row for _, row, _ in PC.CHAIN_STATIONS]
    assert rows == [16, 48]
    peaks = [audio_peak(chain["pcm"][r]) for r in rows]
    assert peaks == [int(b) for b in g["chain_bins"]] == [82, 205], peaks
    # the same two channels through pss_ddc with the bank's taps, then the same demodulator
    taps = Engine.pfb_default_taps(M)
    words = [Engine.ddc_word(off, PC.CHAIN_FS)[0] for off, _, _ in PC.CHAIN_STATIONS]
    assert words == [r * ((1 << 64) // M) for r in rows]
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


def test_channelize_recording_is_independent_of_the_chunking_and_takes_codes(chain):
    from pyspecsdr_amd import formats as F
    M, D = PC.CHAIN_M, PC.CHAIN_D
    span_and_tile = 20 * M + 1 + tile_instants(M) * D
    for chunk in (1000, 32 * 777, 1 << 22):
        ch, off, rate = F.channelize_recording(chain["x"], PC.CHAIN_FS, M, chunk_samples=chunk)
        assert rate == 75000.0 and ch.shape == chain["channels"].shape and np.array_equal(off, F.bank_offsets(PC.CHAIN_FS, M))
        assert np.array_equal(ch.view(np.uint32), chain["channels"].view(np.uint32)), chunk
    assert 1000 < span_and_tile and off[16] == 600e3 and off[48] == -600e3
    rng = np.random.default_rng(64)
    codes = rng.integers(0, 256, (30011, 2), dtype=np.uint8)
    wide = F.unpack_iq(codes, "cu8")
    one = device_pfb(wide, 16, 16)
    ch, _, rate = F.channelize_recording(codes, PC.CHAIN_FS, 16, decim=16, chunk_samples=7001, codes_format="cu8")
    assert rate == PC.CHAIN_FS / 16 and np.array_equal(ch.view(np.uint32), one.view(np.uint32))


def test_demodulate_bank_gives_the_chains_pcm(chain):
    from pyspecsdr_amd import formats as F
    pcm = F.demodulate_bank(chain["x"], PC.CHAIN_FS, PC.CHAIN_M, mode="NFM", frame_len=chain["n_out"], chunk_samples=60000)
    assert pcm.shape == (PC.CHAIN_M, 1, 2048, 2) and np.array_equal(pcm[:, 0], chain["pcm"])


def test_refused_arguments_leave_the_output_untouched():
    e = engine()
    n, M, D, T = 1000, 8, 5, 101
    x, h = samples(n, 1), taps_of(T, 1)
    d_iq = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    d_out = torch.full((M, 2 * 200), float(CANARY), dtype=torch.float32, device="cuda")
    good = dict(taps=h, buf_index0=0, n_capture=n, lead=50, m_begin=0, m_end=200, out_stride=200)
    nan_taps = h.copy()
    nan_taps[7] = np.nan
    bad = [dict(n_chan=0), dict(n_chan=6), dict(n_chan=2048), dict(decim=0), dict(decim=M + 1), dict(taps=np.zeros(32 * M + 1)), dict(taps=np.zeros(0)),
           dict(taps=nan_taps), dict(taps=np.full(3, np.inf)), dict(lead=-1), dict(lead=T), dict(m_end=201), dict(m_begin=-1), dict(m_begin=5, m_end=4),
           dict(out_stride=199), dict(buf_index0=1), dict(n_capture=n - 1), dict(buf_index0=-1),
           dict(n_buf=n - 1),                        # the last outputs need a sample behind the buffer
           dict(d_iq=d_iq.data_ptr() + 4), dict(d_out=d_out.data_ptr() + 4), dict(d_iq=None), dict(d_out=None)]
    for b in bad:
        kw = dict(good)
        kw.update({k: v for k, v in b.items() if k in good})
        with pytest.raises(PssError) as err:
            e.pfb(b.get("d_iq", d_iq), b.get("n_buf", n), b.get("n_chan", M), b.get("decim", D), b.get("d_out", d_out), **kw)
        assert err.value.code == L.PSS_E_ARG and len(str(err.value)) > len("libpss error -1: "), b
    e.sync()
    assert bool(torch.all(d_out == float(CANARY)))
    e.pfb(d_iq, n, M, D, d_out, **good)
    e.sync()
    assert same(d_out.cpu().numpy().view(np.complex64), Engine.h_pfb(x, M, D, h, lead=50))

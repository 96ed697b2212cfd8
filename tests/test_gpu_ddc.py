"""The down-converter on the device: pss_ddc (k_ddc) against the host twin pss_h_ddc, which tests/test_ddc_golden.py pins to SciPy and
to 80-bit truth without a GPU.

Device against twin: bit for bit (both run the statements of pyspecsdr_amd/csrc/pss_ddc.h; the sign of a zero is not part of the
contract, so +0 and -0 compare equal and everything else by its bits).  The goldens go through the device under the statement's bound.
The shapes come from the launch constants restated below: the outputs of a tile M(D, T), the staging capacity, the tap block, the
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
import ddc_cases as DC
from gpu_util import engine
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine, PssError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def launch_constants():
    """The constants of pyspecsdr_amd/csrc/pss_ddc.h and pss_ddc.hip that shape a launch, each beside the source line it restates."""
    return {
        "B": (64, "pss_ddc.h", "constexpr int B = 64;"),                           # taps of a block: a second block sum per output from 65 taps on
        "STAGE_CAP": (8192, "pss_ddc.h", "constexpr int STAGE_CAP = 8192;"),       # mixed samples a tile may stage
        "PART_CAP": (1792, "pss_ddc.h", "constexpr int PART_CAP = 1792;"),         # (output, block) sums of a tile
        "DDC_T": (1024, "pss_ddc.hip", "constexpr int DDC_T = 1024;"),             # threads: a lane's second staged sample / second output starts here
        "DDC_GRID_CAP": (2048, "pss_ddc.hip", "constexpr long DDC_GRID_CAP = 2048;"),   # (tile, channel) pairs of one pass of the grid
    }


K = {k: v[0] for k, v in launch_constants().items()}


def tile_row(M, D, T):
    return (M - 1 + (T + D - 1) // D) | 1


def tile_outputs(D, T):
    """pss_ddc.h's tile_outputs: the outputs of a tile."""
    M = K["PART_CAP"] // ((T + K["B"] - 1) // K["B"])
    while M > 1 and D * tile_row(M, D, T) > K["STAGE_CAP"]:
        M -= 1
    return M


def test_launch_constants_read_as_restated():
    src = {f: open(os.path.join(ROOT, "pyspecsdr_amd", "csrc", f)).read() for f in ("pss_ddc.h", "pss_ddc.hip")}
    for name, (_, f, line) in launch_constants().items():
        assert line in src[f], f"{f} no longer reads `{line}`: restate {name} here"
    for line in ("inline int tile_row(int M, int D, int T) { return (M - 1 + (T + D - 1) / D) | 1; }", "int M = PART_CAP / n_blocks(T);",
                 "while (M > 1 && (long)D * tile_row(M, D, T) > STAGE_CAP) M--;"):
        assert line in src["pss_ddc.h"], line
    for line in ("for (long p = blockIdx.x; p < n_pairs; p += gridDim.x) {", "for (int j = tid; j < span; j += DDC_T) {",
                 "for (int t = wave; t < n_tasks; t += DDC_WAVES) {", "for (int m = tid; m < cnt; m += DDC_T) {",
                 "dim3((unsigned)(n_pairs < DDC_GRID_CAP ? n_pairs : DDC_GRID_CAP)), dim3(DDC_T)"):
        assert line in src["pss_ddc.hip"], line
    # the tiles the sweep below leans on
    assert tile_outputs(1, 1) == 1792 and tile_outputs(50, 1001) == 112 and tile_outputs(4096, 4097) == 1 and tile_outputs(1, 4097) == 27


CANARY = np.float32(-7.25)


def device_ddc(buf, words, D, taps=None, pad=3, **kw):
    """buf (complex64 window of the capture) through pss_ddc -> complex64 [K][m_end - m_begin].  d_iq starts one complex sample (8 bytes)
    into its allocation, so no load may assume more than a sample's alignment; the rows of d_out are `pad` elements apart beyond their
    length, and a canary fills everything beforehand: what lies between the rows must survive."""
    e = engine()
    buf = np.ascontiguousarray(buf, np.complex64)
    flat = np.zeros(2 * len(buf) + 2, np.float32)
    flat[2:] = buf.view(np.float32)
    d_all = torch.from_numpy(flat).cuda()
    d_iq = d_all[2:]
    assert d_iq.data_ptr() % 16 == 8
    words, taps_a, a, b, c, width = Engine._ddc_args(e.lib, len(buf), words, D, taps, kw.get("buf_index0", 0), kw.get("n_capture"), kw.get("lead"),
                                                      kw.get("m_begin", 0), kw.get("m_end"), None)
    stride = width + pad
    d_out = torch.full((len(words), 2 * stride), float(CANARY), dtype=torch.float32, device="cuda")
    e.ddc(d_iq, len(buf), words, D, d_out, taps=taps_a, out_stride=stride, **kw)
    e.sync()
    out = d_out.cpu().numpy()
    assert np.all(out[:, 2 * width:] == CANARY), "the elements between the rows were written"
    return out[:, :2 * width].copy().view(np.complex64)


_BASE = None


def samples(n, seed=0):
    """n samples of one long random capture (amplitudes over a few binades), cut at an offset that depends on the seed."""
    global _BASE
    if _BASE is None:
        rng = np.random.default_rng(31)
        nb = 1 << 18
        _BASE = ((rng.standard_normal(nb) + 1j * rng.standard_normal(nb)) * np.exp2(rng.integers(-3, 2, nb))).astype(np.complex64)
    o = (seed * 7919) % 1000
    assert o + n <= len(_BASE)
    return _BASE[o:o + n]


def taps_of(T, seed=0):
    rng = np.random.default_rng([32, T, seed])
    return rng.standard_normal(T) / np.sqrt(T)


WORDS17 = [int(w) for w in np.random.default_rng(33).integers(0, 1 << 64, 17, dtype=np.uint64)]

# D -> the tap counts it is swept with.  Every T of {1, 2, 63, 64, 65, 128, 129, 20 D + 1, 4097} appears; every T above B appears with
# D = 1 and with D > 1 (20 D + 1 is 21 at D = 1; the 20 D + 1 of the larger D are swept at D = 1 too).
SWEEP_T = {
    1: [1, 2, 21, 63, 64, 65, 128, 129, 141, 1001, 1281, 4097],
    2: [1, 41, 65, 129],
    3: [2, 61, 64, 128],
    7: [63, 141, 129, 4097],
    50: [1001, 65, 128],
    64: [1281, 64, 129],
    4096: [1, 129, 4097],
}
LEADS = ["zero", "mid", "last"]
CHANNELS = [1, 3, 17]


def sweep_lengths(D, T):
    """n_capture: 1, 2, D - 1, D, D + 1, T - 1, T, T + 1, and the shortest captures with one output short of, at and one past one tile and
    two tiles of M(D, T) outputs."""
    M = tile_outputs(D, T)
    n = {1, 2, D - 1, D, D + 1, T - 1, T, T + 1}
    n |= {(o - 1) * D + 1 for o in (M - 1, M, M + 1, 2 * M - 1, 2 * M, 2 * M + 1) if o >= 1}
    return sorted(v for v in n if v >= 1)


def sweep_cases():
    i = 0
    for D, ts in SWEEP_T.items():
        for T in ts:
            for n in sweep_lengths(D, T):
                yield D, T, n, LEADS[i % 3], CHANNELS[(i // 3 + i) % 3]
                i += 1


def lead_of(name, T):
    return {"zero": 0, "mid": (T - 1) // 2, "last": T - 1}[name]


def test_the_sweep_holds_every_value_the_contract_names():
    cases = list(sweep_cases())
    assert {c[0] for c in cases} == {1, 2, 3, 7, 50, 64, 4096}
    ts = {c[1] for c in cases}
    assert {1, 2, 63, 64, 65, 128, 129, 4097} <= ts and all(20 * D + 1 in ts for D in (1, 2, 3, 7, 50, 64))
    for T in ts:
        if T > K["B"]:
            assert any(c[0] == 1 and c[1] == T for c in cases) and any(c[0] > 1 and c[1] == T for c in cases), T
    assert {c[3] for c in cases} == set(LEADS) and {c[4] for c in cases} == set(CHANNELS)
    for D, T in ((1, 1), (50, 1001), (4096, 4097)):
        M = tile_outputs(D, T)
        outs = {-(-c[2] // D) for c in cases if c[0] == D and c[1] == T}
        assert {M - 1, M, M + 1, 2 * M - 1, 2 * M, 2 * M + 1} - {0} <= outs


@pytest.mark.parametrize("D", sorted(SWEEP_T))
def test_device_equals_host_twin_over_the_sweep(D):
    bad = []
    for i, (d, T, n, lead_name, k) in enumerate(sweep_cases()):
        if d != D:
            continue
        x, h, lead, words = samples(n, i), taps_of(T, i), lead_of(lead_name, T), WORDS17[:k]
        got = device_ddc(x, words, D, h, lead=lead)
        want = Engine.h_ddc(x, words, D, h, lead=lead)
        if not same(got, want):
            bad.append((D, T, n, lead_name, k, int(np.sum(got.view(np.uint32) != want.view(np.uint32)))))
    assert not bad, bad[:10]


def test_windows_of_a_capture_and_the_call_shape_change_no_bit():
    """K channels in one call against K calls; [m_begin, m_end) split at arbitrary points; the capture fed as buffers of awkward lengths
    with exactly the halo each needs (buf_index0 > 0) — all against the one call on the whole capture, and that against the twin."""
    D, T, n = 7, 141, 9001
    x, h, lead = samples(n, 5), taps_of(T, 5), 70
    words = WORDS17[:3]
    n_out = -(-n // D)
    whole = device_ddc(x, words, D, h, lead=lead)
    assert same(whole, Engine.h_ddc(x, words, D, h, lead=lead))
    for c, w in enumerate(words):
        assert same(device_ddc(x, [w], D, h, lead=lead)[0], whole[c])
    cuts = [0, 1, 2, 113, 114, 700, n_out - 1, n_out]
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert same(device_ddc(x, words, D, h, lead=lead, m_begin=a, m_end=b), whole[:, a:b]), (a, b)
        lo, hi = max(0, a * D + lead - (T - 1)), min(n, (b - 1) * D + lead + 1)        # exactly the samples these outputs need
        assert same(device_ddc(x[lo:hi], words, D, h, lead=lead, buf_index0=lo, n_capture=n, m_begin=a, m_end=b), whole[:, a:b]), (a, b, lo, hi)


def test_an_index_past_2_to_the_40_in_a_capture_of_2_to_the_41():
    D, T, lead, n_buf = 3, 61, 30, 3000
    index0, n_cap = (1 << 40) + 12345, 1 << 41
    x, h = samples(n_buf, 9), taps_of(T, 9)
    a = -(-(index0 + (T - 1) - lead) // D)
    b = (index0 + n_buf - 1 - lead) // D + 1
    kw = dict(lead=lead, buf_index0=index0, n_capture=n_cap, m_begin=a, m_end=b)
    got = device_ddc(x, WORDS17[:3], D, h, **kw)
    assert got.shape == (3, b - a) and b - a > 900
    assert same(got, Engine.h_ddc(x, WORDS17[:3], D, h, **kw))
    # the phase is the capture's: the same buffer at index 0 gives other bits
    assert not same(got[:, :100], device_ddc(x, WORDS17[:3], D, h, lead=lead, m_begin=20, m_end=120))


@pytest.mark.parametrize("index0", [0, 1, 2, 3])
def test_identity_and_quarter_turn_are_exact_on_the_device(index0):
    x = DC.special_identity_input()
    n = len(x)
    kw = dict(lead=0, buf_index0=index0, n_capture=index0 + n, m_begin=index0, m_end=index0 + n)
    got = device_ddc(x, [0, 1 << 62], 1, [1.0], **kw)
    assert same(got[0], x)
    turn = np.array([1, -1j, -1, 1j])[(index0 + np.arange(n)) & 3]
    want = (x.astype(np.complex128) * turn).astype(np.complex64)       # exact: a swap of the parts and sign changes
    assert same(got[1], want)


def test_one_pair_past_the_grid_cap():
    k = 17
    M = tile_outputs(1, 1)
    tiles = -(-(K["DDC_GRID_CAP"] + 1) // k)
    assert (tiles - 1) * k <= K["DDC_GRID_CAP"] < tiles * k
    n = (tiles - 1) * M + 1
    x = samples(n, 3)
    h = [0.75]
    assert same(device_ddc(x, WORDS17, 1, h, lead=0), Engine.h_ddc(x, WORDS17, 1, h, lead=0))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "ddc.npz"))


def test_golden_cases_through_the_device(g):
    worst = []
    for name, D, n, zero_phase, _ in DC.CASES:
        x, h, ref = DC.case_capture(name), g[f"h_{name}"], g[f"ref_{name}"]
        y = device_ddc(x, g[f"words_{name}"], D, h, lead=(len(h) - 1) // 2 if zero_phase else 0)
        assert same(y, Engine.h_ddc(x, g[f"words_{name}"], D, h, lead=(len(h) - 1) // 2 if zero_phase else 0))
        for c in range(len(ref)):
            excess, used = DC.bound_excess(y[c], ref[c], len(h), np.abs(h).sum(), g[f"zmax_{name}"][c])
            print(f"{name}[{c}]: excess {excess:.3e}, float64 term used {used:.4f}")
            worst.append((excess, name, c))
    assert max(worst)[0] <= 0, max(worst)


def audio_peak(pcm):
    """The largest bin of a 2048-sample audio spectrum (left channel, Hann window, the two DC bins dropped)."""
    a = pcm[:2048, 0].astype(np.float64)
    spec = np.abs(np.fft.rfft(a * np.hanning(len(a))))
    spec[:2] = 0
    return int(np.argmax(spec))


@pytest.fixture(scope="module")
def chain(g):
    """Two NFM stations of one 2.4 MS/s capture: Engine.ddc (D = 50, default taps, K = 2 — and the untuned centre as a third channel)
    then demod_signal(NFM) at 48 kS/s on the device."""
    x = DC.chain_capture()
    assert DC.crc(x) == int(g["chain_crc"]) and int(g["chain_seed"]) == DC.CHAIN_SEED
    e = engine()
    words = [Engine.ddc_word(off, DC.CHAIN_FS)[0] for off, _ in DC.CHAIN_STATIONS] + [0]
    n_out = DC.CHAIN_N // DC.CHAIN_D
    d_iq = torch.from_numpy(x.view(np.float32)).cuda()
    d_ch = torch.empty((3, 2 * n_out), dtype=torch.float32, device="cuda")
    e.ddc(d_iq, len(x), words, DC.CHAIN_D, d_ch)
    fs2 = DC.CHAIN_FS / DC.CHAIN_D
    n_audio = e.demod_out_len(L.MODE_NFM, n_out, fs2)
    d_pcm = torch.empty((3, n_audio, 2), dtype=torch.int16, device="cuda")
    e.demod_signal(L.MODE_NFM, d_ch, 3, n_out, fs2, d_pcm)
    e.sync()
    return {"x": x, "words": words, "channels": d_ch.cpu().numpy().view(np.complex64), "pcm": d_pcm.cpu().numpy(), "fs2": fs2}


def test_chain_equals_the_host_chain_and_finds_both_tones(chain, g):
    e = engine()
    assert chain["fs2"] == 48000.0 and chain["pcm"].shape == (3, 2048, 2)
    h_ch = Engine.h_ddc(chain["x"], chain["words"], DC.CHAIN_D)
    assert same(chain["channels"], h_ch)
    assert np.array_equal(chain["pcm"], e.h_demodulate_batch(L.MODE_NFM, h_ch, chain["fs2"]))
    # h_demodulate_batch runs the same kernels behind a staging copy: the CPU oracle on the twin's channels is what anchors the PCM
    # (demodulate_signal does not correct NFM buffers; the engine's own tables at 48 kS/s, q = 2)
    import oracle_lib as O
    taps, sos, zi = e.nfm_filters(chain["fs2"])
    with np.errstate(all="ignore"):
        want = np.stack([O.pcm16_stereo(O.demod_nfm(row, chain["fs2"], taps, sos, zi)) for row in h_ch])
    assert np.array_equal(chain["pcm"], want), np.nonzero((chain["pcm"] != want).any(axis=(1, 2)))[0]
    peaks =[audio_peak(chain["pcm"][c]) for c in range(3)]
    assert peaks[:2] == [int(b) for b in g["chain_bins"]] == [85, 213], peaks
    assert peaks[2] not in (85, 213), peaks        # the untuned channel hears neither station


def test_tune_recording_is_independent_of_the_chunking_and_takes_codes(chain):
    from pyspecsdr_amd import formats as F
    offsets = [off for off, _ in DC.CHAIN_STATIONS] + [0.0]
    for chunk in (1000, 50 * 777, 1 << 22):
        ch, rate, eff = F.tune_recording(chain["x"], DC.CHAIN_FS, offsets, DC.CHAIN_D, chunk_samples=chunk)
        assert rate == 48000.0 and list(eff) == offsets and ch.shape == chain["channels"].shape
        assert np.array_equal(ch.view(np.uint32), chain["channels"].view(np.uint32)), chunk
    rng = np.random.default_rng(34)
    codes = rng.integers(0, 256, (30011, 2), dtype=np.uint8)
    wide = F.unpack_iq(codes, "cu8")
    one = device_ddc(wide, chain["words"], DC.CHAIN_D)
    ch, _, _ = F.tune_recording(codes, DC.CHAIN_FS, offsets, DC.CHAIN_D, chunk_samples=7001, codes_format="cu8")
    assert np.array_equal(ch.view(np.uint32), one.view(np.uint32))


def test_demodulate_channels_gives_the_chains_pcm(chain):
    from pyspecsdr_amd import formats as F
    offsets = [off for off, _ in DC.CHAIN_STATIONS] + [0.0]
    pcm = F.demodulate_channels(chain["x"], DC.CHAIN_FS, offsets, DC.CHAIN_D, mode="NFM", frame_len=4096, chunk_samples=60000)
    assert pcm.shape == (3, 1, 2048, 2) and np.array_equal(pcm[:, 0], chain["pcm"])


def test_refused_arguments_leave_the_output_untouched():
    e = engine()
    n, D, T = 1000, 5, 101
    x, h = samples(n, 1), taps_of(T, 1)
    d_iq = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    d_out = torch.full((2, 2 * 200), float(CANARY), dtype=torch.float32, device="cuda")
    good = dict(taps=h, buf_index0=0, n_capture=n, lead=50, m_begin=0, m_end=200, out_stride=200)
    nan_taps = h.copy()
    nan_taps[7] = np.nan
    bad = [dict(decim=0), dict(decim=4097), dict(taps=np.zeros(4098)), dict(taps=np.zeros(0)), dict(taps=nan_taps), dict(taps=np.full(3, np.inf)),
           dict(lead=-1), dict(lead=T), dict(m_end=201), dict(m_begin=-1), dict(m_begin=5, m_end=4), dict(out_stride=199),
           dict(buf_index0=1), dict(n_capture=n - 1), dict(buf_index0=-1), dict(words=[]),
           dict(n_buf=n - 1),                        # the last outputs need a sample behind the buffer
           dict(d_iq=d_iq.data_ptr() + 4), dict(d_out=d_out.data_ptr() + 4), dict(d_iq=None), dict(d_out=None)]
    for b in bad:
        kw = dict(good)
        kw.update({k: v for k, v in b.items() if k in good})
        with pytest.raises(PssError) as err:
            e.ddc(b.get("d_iq", d_iq), b.get("n_buf", n), b.get("words", WORDS17[:2]), b.get("decim", D), b.get("d_out", d_out), **kw)
        assert err.value.code == L.PSS_E_ARG and len(str(err.value)) > len("libpss error -1: "), b
    e.sync()
    assert bool(torch.all(d_out == float(CANARY)))
    e.ddc(d_iq, n, WORDS17[:2], D, d_out, **good)
    e.sync()
    assert same(d_out.cpu().numpy().view(np.complex64), Engine.h_ddc(x, WORDS17[:2], D, h, lead=50))

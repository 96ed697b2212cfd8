"""Every capped launch grid of tests/launch_caps.py walked one step past its cap: a batch of at least cap + 2 frames (rows, bits or
elements), every output against the CPU oracle (oracle/pss_oracle.c over oracle_lib.map_frames) or, for pss_row_normalise and the
default Hilbert transform, against the same statements in NumPy.

Past the cap a workgroup (or thread) handles frame f, then f + grid: LDS state, per-workgroup scratch or a reduction left over from the
first frame, or an output a one-pass loop never writes, shows up only there.  So every batch is made of frames that differ from each
other (checked on the host), with a NaN-sample frame at 0, a silent frame at 1 and an Inf-sample frame at 2 (where the path takes one)
ahead of the second frames of workgroups 0 .. 2, clean frames at cap - 1, cap and cap + 1, and a tiny-amplitude (1e-19) or extreme
frame last; element-wise kernels get special values at 0, 1, cap, cap + 1 and the last index.  Every output buffer is filled with
0x7f bytes before the call, so a value the kernel never writes fails.  Criteria are those of the per-path tests of
test_gpu_parity.py, unchanged.  A failure names the entry point, kernel, cap, the first failing frame (before or past the cap) and its
first offending value.

The Hilbert rows carry no Inf-sample frame: on such a row oracle_lib.hilbert keeps two imaginary values finite where SciPy's hilbert()
has none, so neither the bit-exact nor the NumPy comparison defines the expected values there.

Measured on one MI355X: 29.8 s for the whole file (43 tests; classify at 600 samples the longest, 5.0 s).  Device memory in use
(hipMemGetInfo after each test, this process's torch cache and the library's grow-only scratch included) peaks at 5.2 GiB, after
the 8192-point float64 spectrum test.
"""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle_lib as O
import gpu_util as G
from launch_caps import CAPS
import spectrum_bounds as SB
from spectrum_bounds import scan_ulp_bound
from pyspecsdr_amd import _lib as L

CHUNK = 2048
SSB_ATOL = 2e-14          # test_ssb_vs_golden / test_round6_complex128_buffers_vs_reference_goldens
HIL_REL = 1e-13           # test_hilbert_rows: |got - ref| / max|x| of the row
SCAN_DIFF_RATE = 3 / 146912   # test_scanner_rows_equal_the_oracle_on_every_kernel_family: share of dB values that may differ at all


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def sentinel(shape, dtype):
    """A device buffer of 0x7f bytes: no result of these kernels has that value (float32 3.4e38, float64 1.4e306, int 0x7f..)."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0x7F)
    return t


def distinct(x, what):
    x = np.ascontiguousarray(x)
    d = {hashlib.blake2b(r.tobytes(), digest_size=16).digest() for r in x.reshape(len(x), -1)}
    assert len(d) == len(x), f"{what}: {len(x) - len(d)} input frames repeat another frame"


def same_bits(g, w):
    """Equal in every bit, or both NaN."""
    g, w = np.asarray(g), np.asarray(w, dtype=np.asarray(g).dtype)
    if g.dtype.kind != "f":
        return g == w
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    return (np.ascontiguousarray(g).view(u) == np.ascontiguousarray(w).view(u)) | (np.isnan(g) & np.isnan(w))


def within(g, w, tol):
    """|g - w| <= tol, NaN only where the other is NaN."""
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    gn, wn = np.isnan(g), np.isnan(w)
    with np.errstate(invalid="ignore"):
        return np.where(gn | wn, gn & wn, (g == w) | (np.abs(g - w) <= tol))


class Report:
    """Failures of one batch, per criterion: how many frames fail, the first of them (before or past the cap) and its first value."""

    def __init__(self, name, n, nf, label=""):
        self.row, self.nf, self.fails = CAPS[name], nf, []
        self.cap = self.row.cover(n)
        assert nf > self.cap, f"{self.row.entry}: a batch of {nf} {self.row.unit} does not pass the cap of {self.cap}"
        self.head = f"{self.row.entry} [{self.row.kernels}] {label}, cap {self.cap} {self.row.unit}, batch {nf}"

    def where(self, f):
        return f"{f} ({'before' if f < self.cap else 'past'} the cap)"

    def add(self, what, ok, got, want, f0=0, unit_of=None):
        """ok: [frames, ...] booleans (True: the value passes) for frames f0 .., with got / want of the same layout."""
        ok = np.asarray(ok).reshape(len(ok), -1)
        bad = np.nonzero(~ok.all(axis=1))[0]
        if bad.size:
            f = int(bad[0])
            i = int(np.nonzero(~ok[f])[0][0])
            g = np.asarray(got).reshape(len(ok), -1)[f, i]
            w = np.asarray(want).reshape(len(ok), -1)[f, i]
            first = f0 + f if unit_of is None else unit_of(f0 + f, i)
            self.fails.append(f"{what}: {bad.size} frames fail, first frame {self.where(f0 + f)}, index {i}"
                              f"{'' if unit_of is None else f' ({self.row.unit[:-1]} {self.where(first)})'}: got {g!r}, want {w!r}")

    def check(self):
        assert not self.fails, self.head + ":\n  " + "\n  ".join(self.fails)


def chunks(nf, size=CHUNK):
    for f0 in range(0, nf, size):
        yield f0, min(nf, f0 + size)


def plant(x, cap, nan=True, inf=True, last="tiny"):
    """Edge frames (in place, host array [nf][n] real or complex): NaN sample at 0, silent 1, Inf sample at 2; the last frame tiny
    (1e-19: float32 |x|^2 below the normal range) or near full scale.  Frames cap - 1 .. cap + 1 stay clean."""
    nf, n = x.shape[:2]
    assert nf >= cap + 3
    if nan:
        x[0, n // 3] = np.nan
    x[1] = 0
    if inf:
        x[2, n // 2] = np.inf
    if last == "tiny":
        x[-1] *= 1e-19
    elif last == "full":
        x[-1] *= 0.999 / np.max(np.abs(x[-1]))
    return x


def noise_iq(rng, nf, n, dtype=np.complex64):
    return ((rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))) * 10.0 ** rng.uniform(-2, 0, (nf, 1))).astype(dtype)


def fm_iq(rng, nf, n, fs):
    """Distinct reads of a scanner sweep: carriers at random offsets, FM at four deviations, noise at random levels."""
    t = np.arange(n) / fs
    off = rng.uniform(-6e5, 6e5, (nf, 1))
    dev = np.array([0.0, 5e3, 75e3, 3e5])[np.arange(nf) % 4][:, None]
    fm = rng.uniform(300, 15e3, (nf, 1))
    ph = 2 * np.pi * dev * np.cumsum(np.sin(2 * np.pi * fm * t), axis=1) / fs + 2 * np.pi * off * t
    x = 0.5 * np.exp(1j * ph)
    x += 10.0 ** rng.uniform(-3, -1, (nf, 1)) * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))
    return x.astype(np.complex64)


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _rows_of(d, f0, f1):
    return d[f0:f1].cpu().numpy()


# ---- pss_classify: k_cls_modidx + k_cls_welch / k_cls_welch_short ---------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("classify", 1024), ("classify_short", 600)])
def test_classify_past_the_cap(name, n):
    """test_classify_batch_vs_oracle's criteria: label and bandwidth equal, modulation index bit-exact, flatness within 1e-5
    relative, PSD within 1e-6 relative of the oracle's plus the 1e-10 floor."""
    e, fs = G.engine(), 2.4e6
    cap = CAPS[name].cover(n)
    nf = cap + 3
    R = Report(name, n, nf, f"n={n}")
    iq = plant(fm_iq(np.random.default_rng(nf + n), nf, n, fs), cap, last="full")
    distinct(iq, R.head)
    d_lab, d_bw = sentinel((nf,), torch.int32), sentinel((nf,), torch.float64)
    d_mi, d_fl, d_psd = sentinel((nf,), torch.float32), sentinel((nf,), torch.float32), sentinel((nf, 1024), torch.float32)
    e.classify(G.dev(iq), nf, n, fs, d_lab, d_bw, d_mi, d_fl, d_psd)
    e.sync()
    lab, bw, mi, fl = (G.host(a) for a in (d_lab, d_bw, d_mi, d_fl))
    m = min(n, 1024)
    with np.errstate(all="ignore"):
        for f0, f1 in chunks(nf):
            want = O.map_frames(lambda x: O.classify(x, fs), iq[f0:f1])
            wl = np.array([O.CLASS_LABELS.index(w[0]) for w in want], np.int32)
            R.add("label", lab[f0:f1] == wl, lab[f0:f1], wl, f0)
            wb = np.array([w[1] for w in want])
            R.add("bandwidth", same_bits(bw[f0:f1], wb), bw[f0:f1], wb, f0)
            wm = np.array([w[2] for w in want], np.float32)
            R.add("modulation index bits", same_bits(mi[f0:f1], wm), mi[f0:f1], wm, f0)
            wf = np.array([w[3] for w in want], np.float32)
            R.add("flatness (1e-5 relative)", within(fl[f0:f1], wf, 1e-5 * np.abs(wf.astype(np.float64))), fl[f0:f1], wf, f0)
            wp = np.stack([w[4] for w in want])
            gp = _rows_of(d_psd, f0, f1)[:, :m]
            R.add("PSD (1e-6 relative + 1e-10)", within(gp, wp, 1e-6 * (wp.astype(np.float64) + 1e-10)), gp, wp, f0)
    R.check()


# ---- pss_morse_edges: k_morse_edges ---------------------------------------------------------------------------------------------------
def test_morse_edges_past_the_cap():
    """test_decoder_front_halves' batch criteria: counts and indices exact, at the reference's -20 dB and at -33.3 dB."""
    e, n = G.engine(), 300
    cap = CAPS["morse"].cover(n)
    nf = cap + 3
    rng = np.random.default_rng(9)
    key = np.repeat(rng.integers(0, 2, (nf, n // 20 + 1)), 20, axis=1)[:, :n] * rng.uniform(0.05, 1.0, (nf, 1))
    iq = (key * np.exp(0.2j * np.arange(n)) + 10.0 ** rng.uniform(-4, -1, (nf, 1)) *
          (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
    plant(iq, cap)
    distinct(iq, "pss_morse_edges")
    ecap = n // 2 + 1
    d_iq = G.dev(iq)
    for thr in (-20.0, -33.3):
        R = Report("morse", n, nf, f"n={n} threshold {thr} dB")
        d_r, d_f, d_c = sentinel((nf, ecap), torch.int32), sentinel((nf, ecap), torch.int32), sentinel((nf, 2), torch.int32)
        e.morse_edges(d_iq, nf, n, ecap, d_r, d_f, d_c, threshold_db=thr)
        e.sync()
        r, f, c = G.host(d_r), G.host(d_f), G.host(d_c)
        with np.errstate(all="ignore"):
            for f0, f1 in chunks(nf):
                want = O.map_frames(lambda x: O.morse_edges(x, thr), iq[f0:f1])
                wc = np.array([[len(a), len(b)] for a, b in want], np.int32)
                R.add("rise / fall counts", c[f0:f1] == wc, c[f0:f1], wc, f0)
                for k, (wr, wf) in enumerate(want):
                    g = f0 + k
                    if c[g, 0] == len(wr) and c[g, 1] == len(wf):
                        R.add("rise indices", (r[g, :len(wr)] == wr)[None], r[g, :len(wr)][None], wr[None], g)
                        R.add("fall indices", (f[g, :len(wf)] == wf)[None], f[g, :len(wf)][None], wf[None], g)
        R.check()


# ---- pss_afsk_bits: k_afsk_bits (one thread per bit) ----------------------------------------------------------------------------------
def test_afsk_bits_past_the_cap(golden):
    """test_afsk_bits' batch criterion: every bit equal to the oracle's; the cap counts bits (one thread each)."""
    g = golden["afsk"]
    s1, s2 = g["sos1200_a"], g["sos2200_a"]
    e, n, fs = G.engine(), 5000, 22050.0
    nb = e.afsk_n_bits(n, fs)
    cap = CAPS["afsk"].cover(n)
    rows = cap // nb + 2
    R = Report("afsk", n, rows * nb, f"{rows} rows of {n} samples, {nb} bits each")
    rng = np.random.default_rng(8)
    x = rng.standard_normal((rows, n)) * 10.0 ** rng.uniform(-2, 1, (rows, 1))
    x[0, n // 3] = np.nan
    x[1] = 0
    x[2, n // 2] = np.inf
    x[-1] *= 1e-19
    distinct(x, R.head)
    d_bits = sentinel((rows, nb), torch.uint8)
    e.afsk_bits(G.dev(x), rows, n, fs, d_bits, s1, s2)
    e.sync()
    bits = G.host(d_bits)
    with np.errstate(all="ignore"):
        for f0, f1 in chunks(rows, 512):
            want = np.stack(O.map_frames(lambda r: O.afsk_bits(r, fs, s1, s2), x[f0:f1]))
            R.add("bits", bits[f0:f1] == want, bits[f0:f1], want, f0, unit_of=lambda f, i: f * nb + i)
    R.check()


# ---- pss_row_normalise: k_row_normalise -----------------------------------------------------------------------------------------------
def test_row_normalise_past_the_cap():
    """test_decoder_front_halves' criterion: IEEE division by the row's max |x|, NaN as NaN."""
    e, n = G.engine(), 257
    cap = CAPS["row_normalise"].cover(n)
    nf = cap + 3
    R = Report("row_normalise", n, nf, f"n={n}")
    rng = np.random.default_rng(12)
    x = rng.standard_normal((nf, n)) * 10.0 ** rng.uniform(-3, 3, (nf, 1))
    plant(x, cap)
    distinct(x, R.head)
    d_y = sentinel((nf, n), torch.float64)
    e.row_normalise(G.dev(x), nf, n, d_y)
    e.sync()
    y = G.host(d_y)
    with np.errstate(all="ignore"):
        want = x / np.max(np.abs(x), axis=1, keepdims=True)
    R.add("x / max|x|", same_bits(y, want), y, want)
    R.check()


# ---- complex128 buffers: pss_demod_am_c128, pss_mean_power_c128, pss_demod_ssb_c128 -----------------------------------------------------
def test_am_and_power_c128_past_the_cap():
    """test_round6_complex128_buffers_vs_reference_goldens' criteria: float64 audio, int16 PCM and mean power bit-exact."""
    e, n = G.engine(), 512
    cap = CAPS["am_c128"].cover(n)
    assert CAPS["power_c128"].cover(n) == cap
    nf = cap + 3
    rng = np.random.default_rng(66)
    x = noise_iq(rng, nf, n, np.complex128) + 0.3 * np.exp(2j * np.pi * rng.uniform(-0.4, 0.4, (nf, 1)) * np.arange(n))
    plant(x, cap)
    d_iq = G.dev(x.view(np.float64).reshape(nf, n, 2))
    sos = np.empty((5, 6))
    e.lib.pss_am_bandpass_sos(sos.ctypes.data)
    R = Report("am_c128", n, nf, f"n={n}")
    P = Report("power_c128", n, nf, f"n={n}")
    distinct(x, R.head)
    d_pcm, d_au, d_pw = sentinel((nf, n, 2), torch.int16), sentinel((nf, n), torch.float64), sentinel((nf,), torch.float64)
    e.demod_am_c128(d_iq, nf, n, d_pcm, d_au)
    e.mean_power_c128(d_iq, nf, n, d_pw)
    e.sync()
    pw = G.host(d_pw)
    with np.errstate(all="ignore"):
        for f0, f1 in chunks(nf):
            want = np.stack(O.map_frames(lambda r: O.demod_am_c128(r, sos), x[f0:f1]))
            au, pcm = _rows_of(d_au, f0, f1), _rows_of(d_pcm, f0, f1)
            R.add("float64 audio bits", same_bits(au, want), au, want, f0)
            wp = np.stack([O.pcm16_stereo(a) for a in want])
            R.add("int16 PCM", pcm == wp, pcm, wp, f0)
            wm = np.array(O.map_frames(O.mean_power_c128, x[f0:f1]))
            P.add("mean power bits", same_bits(pw[f0:f1], wm), pw[f0:f1], wm, f0)
    R.check()
    P.check()


def test_ssb_c128_past_the_cap():
    """Frames of 1000 samples (no hilbert() round trip: k_ssb_fir, k_ssb_edge, k_finalize): float64 audio within 2e-14 of the oracle,
    int16 PCM equal."""
    e, n, fs = G.engine(), 1000, 48000.0
    cap = CAPS["ssb_c128"].cover(n)
    nf = cap + 3
    R = Report("ssb_c128", n, nf, f"n={n}")
    rng = np.random.default_rng(67)
    x = noise_iq(rng, nf, n, np.complex128) * (1.0 + 1e-9 * rng.standard_normal((nf, 1)))
    plant(x, cap, last="full")
    distinct(x, R.head)
    taps = e.ssb_taps(fs)
    d_pcm, d_au = sentinel((nf, n, 2), torch.int16), sentinel((nf, n), torch.float64)
    e.demod_ssb_c128(G.dev(x.view(np.float64).reshape(nf, n, 2)), nf, n, fs, d_pcm, d_au)
    e.sync()
    with np.errstate(all="ignore"):
        for f0, f1 in chunks(nf):
            want = np.stack(O.map_frames(lambda r: O.demod_ssb_c128(r, taps), x[f0:f1]))
            au, pcm = _rows_of(d_au, f0, f1), _rows_of(d_pcm, f0, f1)
            R.add("float64 audio (2e-14)", within(au, want, SSB_ATOL), au, want, f0)
            wp = np.stack([O.pcm16_stereo(a) for a in want])
            R.add("int16 PCM", pcm == wp, pcm, wp, f0)
    R.check()


# ---- element-wise kernels: pss_np_f32, pss_vector_cells --------------------------------------------------------------------------------
def f32_specials(golden):
    """The special operands of test_numpy_float32_primitives' atan2f fixture: zeros, denormals, +-3e38, infinities, NaN (10 values)."""
    g = golden["atan2f"]
    v = np.concatenate([g["x"], g["y"]])
    v = v[~np.isfinite(v) | (v == 0) | (np.abs(v) < 1.2e-38) | (np.abs(v) > 1e38)]
    return np.unique(v.view(np.uint32)).view(np.float32)


@pytest.mark.parametrize("op", ["arctan2", "log10", "abs"])
def test_np_f32_past_the_cap(op, golden):
    """test_numpy_float32_primitives' criterion: every value bit-exact against the oracle, NaN as NaN.  Random bit patterns; the special
    operands of its atan2f fixture at 0, 1 and the last index, and every pair of them at the first indices of the second pass."""
    e = G.engine()
    cap = CAPS["np_f32"].cover(0)
    n = cap + 1000
    R = Report("np_f32", n, n, op)
    rng = np.random.default_rng(92)
    a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    b = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    sp = f32_specials(golden)
    assert len(sp) == 10 and np.isnan(sp).sum() == 1 and np.isinf(sp).sum() == 2
    pa, pb = np.meshgrid(sp, sp)
    a[cap:cap + pa.size], b[cap:cap + pb.size] = pa.ravel(), pb.ravel()
    a[[0, 1, n - 1]], b[[0, 1, n - 1]] = sp[[5, 4, 9]], sp[[4, 5, 0]]
    assert len(np.unique(a.view(np.uint32))) > n - 1000       # random words: frames distinct but for chance collisions
    code = {"arctan2": L.NP_ARCTAN2, "log10": L.NP_LOG10, "abs": L.NP_ABS}[op]
    d_out = sentinel((n,), torch.float32)
    e.np_f32(code, G.dev(a), None if op == "log10" else G.dev(b), n, d_out)
    e.sync()
    got = G.host(d_out)
    ref = {"arctan2": lambda s: O.atan2f(a[s], b[s]), "log10": lambda s: O.log10f(a[s]), "abs": lambda s: O.cabsf(a[s], b[s])}[op]
    step = 1 << 16
    want = np.concatenate(O.map_frames(ref, [slice(i, min(n, i + step)) for i in range(0, n, step)]))
    R.add("values (bit-exact)", same_bits(got, want).reshape(-1, 1), got.reshape(-1, 1), want.reshape(-1, 1))
    R.check()


@pytest.mark.parametrize("hh,ww", [(40, 120), (25, 81)])
def test_vector_cells_past_the_cap(hh, ww, golden):
    """test_vector_display_cells' criterion: the cell grid equal to the oracle's.  The samples of the grid's first pass stay in a small
    cluster at the centre; those past the cap are the vector_cells golden's read buffer (at the first indices of the second pass) and
    samples all over the grid, so that a walk which stops after one pass misses cells.  Special operands of the atan2f fixture at 0, 1,
    right after the golden buffer and at the last index."""
    e = G.engine()
    cap = CAPS["vector"].cover(0)
    n = cap + 1000
    R = Report("vector", n, n, f"{hh} x {ww}")
    rng = np.random.default_rng(hh)
    iq = (0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    iq[cap:] = (rng.uniform(-2.1, 2.1, n - cap) + 1j * rng.uniform(-2.1, 2.1, n - cap)).astype(np.complex64)
    g = golden["caller"]["vec_iq"]
    iq[cap:cap + len(g)] = g
    sp = f32_specials(golden)
    v = iq.view(np.float32).reshape(n, 2)
    for k, i in enumerate([0, 1, cap + len(g), cap + len(g) + 1, n - 1]):
        v[i] = sp[[(2 * k) % 10, (2 * k + 5) % 10]]
    assert len(np.unique(iq.view(np.uint64))) == n
    want = O.vector_cells(iq, hh, ww)
    first = O.vector_cells(iq[:cap], hh, ww)
    assert (want != first).sum() > 10, "the samples past the cap must draw cells of their own"
    d_g = sentinel((hh, ww), torch.int8)
    e.vector_cells(G.dev(iq), n, hh, ww, d_g)
    e.sync()
    got = G.host(d_g)
    R.add("grid (rows of cells)", got == want, got, want)
    R.check()


# ---- pss_spectrogram_cells: k_spectrogram<float / double>, 256 and 1024 threads ---------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("length", [2044, 5000])          # 256 threads (len <= 4096) / 1024 threads
def test_spectrogram_cells_past_the_cap(f64, length):
    """test_spectrogram_cells' criteria on every row: glyph and colour cells equal to the oracle's, d_range within 1e-14."""
    e, dh, dw = G.engine(), 30, 100
    cap = CAPS["spectrogram"].cover(length)
    nf = cap + 3
    R = Report("spectrogram", length, nf, f"{'float64' if f64 else 'float32'} rows of {length}")
    rng = np.random.default_rng(length + f64)
    rows = rng.standard_normal((nf, length)) * rng.uniform(1, 8, (nf, 1)) - rng.uniform(20, 80, (nf, 1))
    lo = rng.integers(0, length - 100, nf)
    rows[np.arange(nf)[:, None], lo[:, None] + np.arange(60)] += 35
    rows[0, 10] = np.nan                                  # excluded from the statistics; its columns stay undrawn
    rows[1] = -100.0                                      # a silent read: every bin on the floor
    rows[-1] = -40.0 + 1e-9 * rng.standard_normal(length)   # a near-flat row: a range of nano-dB
    rows = rows if f64 else rows.astype(np.float32)
    distinct(rows, R.head)
    d_gl, d_co, d_rg = sentinel((nf, dh, dw), torch.int8), sentinel((nf, dh, dw), torch.int8), sentinel((nf, 2), torch.float64)
    e.spectrogram_cells(G.dev(rows), nf, length, dh, dw, d_gl, d_co, d_rg, f64=f64)
    e.sync()
    rg = G.host(d_rg)
    for f0, f1 in chunks(nf):
        want = O.map_frames(lambda r: O.spectrogram_cells(np.asarray(r, np.float64), dh, dw), rows[f0:f1])
        gl, co = _rows_of(d_gl, f0, f1), _rows_of(d_co, f0, f1)
        wg, wc = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        R.add("glyph cells", gl == wg, gl, wg, f0)
        R.add("colour cells", co == wc, co, wc, f0)
        wr = np.array([[w[2], w[3]] for w in want])
        R.add("d_range (1e-14 relative)", within(rg[f0:f1], wr, 1e-14 * np.abs(wr)), rg[f0:f1], wr, f0)
    R.check()


# ---- pss_scan / pss_scan_threshold on Bluestein lengths: k_scan_reduce -------------------------------------------------------------------
def test_scan_past_the_cap():
    """test_cfg4_scanner_every_slice's criteria: every dB value within scan_ulp_bound of the oracle's plus, as
    test_scanner_rows_amplitude_sweep allows, the dB allowance of the reference's own complex64 transform (delta_f32_reference; at
    16 387 slices of 1000 samples one value, -0.67 dB, is 1.19e-6 dB off, 1.25 times scan_ulp_bound alone); the share that differs at
    all within the per-family test's rate; peak, count and bandwidth equal to the oracle's on bit-equal rows and to those recomputed from the
    device's own row elsewhere.  pss_scan (peak - 20 dB) and pss_scan_threshold (-30 dB, the sweep driver's)."""
    e, n, fs, thr = G.engine(), 1000, 2.4e6, -30.0
    cap = CAPS["scan"].cover(n)
    ns = cap + 3
    rng = np.random.default_rng(23)
    iq = (0.05 * (rng.standard_normal((ns, n)) + 1j * rng.standard_normal((ns, n))) +
          0.5 * np.exp(2j * np.pi * rng.uniform(-0.4, 0.4, (ns, 1)) * np.arange(n))).astype(np.complex64)
    plant(iq, cap, last="full")
    distinct(iq, "pss_scan")
    d_iq = G.dev(iq)
    for mode in ("scan", "scan_threshold"):
        R = Report("scan", n, ns, mode)
        d_db, d_pk = sentinel((ns, n), torch.float32), sentinel((ns,), torch.float32)
        d_bw, d_cnt = sentinel((ns,), torch.float64), sentinel((ns,), torch.int32)
        if mode == "scan":
            e.scan(d_iq, ns, n, fs, d_db, d_pk, d_bw, d_cnt)
        else:
            e.scan_threshold(d_iq, ns, n, fs, thr, d_db, d_pk, d_bw, d_cnt)
        e.sync()
        pk, bw, cnt = G.host(d_pk), G.host(d_bw), G.host(d_cnt)
        diff = total = 0
        with np.errstate(all="ignore"):
            for f0, f1 in chunks(ns):
                ref = (lambda x: O.scan_slice(x, fs)) if mode == "scan" else (lambda x: O.scan_threshold(x, fs, thr))
                want = O.map_frames(ref, iq[f0:f1])
                g = _rows_of(d_db, f0, f1)
                w = np.stack([v[0] for v in want])
                gn, wn = np.isnan(g), np.isnan(w)
                same = same_bits(g, w)
                with np.errstate(invalid="ignore", over="ignore"):
                    allow = scan_ulp_bound(w) + SB.db_allowance(np.where(np.isfinite(w), w, 0.0), SB.delta_f32_reference(iq[f0:f1]))
                far = ((np.abs(g.astype(np.float64) - w) > allow) & ~(gn & wn)) | (gn ^ wn)
                R.add("dB value beyond scan_ulp_bound + the reference transform's allowance", ~far, g, w, f0)
                diff += int((~same).sum())
                total += same.size
                ok = np.ones(f1 - f0, bool)
                for k in range(f1 - f0):
                    if same[k].all():
                        ok[k] = (pk[f0 + k].tobytes() == np.float32(want[k][1]).tobytes() and int(cnt[f0 + k]) == want[k][3]
                                 and same_bits(bw[f0 + k], want[k][2]))
                    else:
                        p = g[k].max()
                        c = int(np.sum(g[k] > (p - np.float32(20) if mode == "scan" else np.float32(thr))))
                        ok[k] = pk[f0 + k].tobytes() == p.tobytes() and int(cnt[f0 + k]) == c and float(bw[f0 + k]) == c * (fs / n)
                wc = np.array([v[3] for v in want])
                R.add("peak / count / bandwidth", ok, cnt[f0:f1], wc, f0)
        assert diff <= max(3, SCAN_DIFF_RATE * total), f"{R.head}: {diff} of {total} dB values differ from the oracle's"
        R.check()


# ---- pss_hilbert ----------------------------------------------------------------------------------------------------------------------
def _hilbert_rows(rng, nf, n, cap, inf=True):
    x = rng.standard_normal((nf, n)) * 10.0 ** rng.uniform(-2, 1, (nf, 1))
    x[3] = np.cos(2 * np.pi * 37 * np.arange(n) / n)
    return plant(x, cap, inf=inf)


def _hilbert(x, exact):
    e = G.engine()
    nf, n = x.shape
    d_out = sentinel((nf, n, 2), torch.float64)
    e.set_option("hilbert_exact", int(exact))
    try:
        e.hilbert(G.dev(x), nf, n, d_out)
        e.sync()
    finally:
        e.set_option("hilbert_exact", 0)
    return d_out


def _check_default_hilbert(R, x, d_out):
    """test_hilbert_rows' bounds: |got - ifft(fft(x) h)| <= 1e-13 max|x| per row, |got.real - x| to the same bound, the cosine row
    within 1e-12 of exp(i w t); a row with a NaN sample NaN where NumPy's is, the silent row exactly zero."""
    nf, n = x.shape
    h = np.zeros(n)
    h[0] = h[n // 2] = 1
    h[1:n // 2] = 2
    for f0, f1 in chunks(nf, 32):
        got = _rows_of(d_out, f0, f1).view(np.complex128).reshape(f1 - f0, n)
        with np.errstate(all="ignore"):
            ref = np.fft.ifft(np.fft.fft(x[f0:f1], axis=1) * h, axis=1)
            scale = np.max(np.abs(x[f0:f1]), axis=1, keepdims=True)
            tol = HIL_REL * scale
            gn, wn = np.isnan(got), np.isnan(ref)
            ok = np.where(gn | wn, gn & wn, np.abs(got - ref) <= tol)
            fin = np.isfinite(x[f0:f1]).all(axis=1, keepdims=True)   # the real part is the input (a NaN row's is NaN throughout)
            ok &= within(got.real, x[f0:f1], tol) | ~fin
        R.add("analytic signal (1e-13 of the row's peak)", ok, got, ref, f0)
        if f0 <= 3 < f1:
            cw = np.exp(2j * np.pi * 37 * np.arange(n) / n)
            R.add("cosine row against exp(i w t) (1e-12)", (np.abs(got[3 - f0] - cw) < 1e-12)[None], got[3 - f0][None], cw[None], 3)


HIL_DEFAULT = {256: "hilbert_r16", 512: "hilbert_r16", 1024: "hilbert_r16", 2048: "hilbert_r16", 4096: "hilbert_r16",
               8192: "hilbert_xl", 16384: "hilbert_xl", 32768: "hilbert_long", 65536: "hilbert_long", 1 << 17: "hilbert_huge"}


@pytest.mark.parametrize("n", sorted(HIL_DEFAULT))
def test_hilbert_default_past_the_cap(n):
    """The default transform: k_hilbert_r16 (256 .. 4096), k_hilbert_xl (8192, 16384), hilbert_long's k_big_g with its per-workgroup
    pre-pass scratch (32768, 65536) and the Bluestein pass kernels with the Hilbert loaders and stores (2^17)."""
    name = HIL_DEFAULT[n]
    cap = CAPS[name].cover(n)
    nf = cap + 3
    R = Report(name, n, nf, f"n={n}")
    x = _hilbert_rows(np.random.default_rng(n), nf, n, cap, inf=False)
    distinct(x, R.head)
    d_out = _hilbert(x, False)
    _check_default_hilbert(R, x, d_out)
    R.check()
    del d_out
    _free()


@pytest.mark.parametrize("name,n", [("hilbert_exact_long", 1 << 20), ("hilbert_exact_long", 1 << 18), ("hilbert_exact", 16384),
                                    ("hilbert_exact", 256)])
def test_hilbert_exact_past_the_cap(name, n):
    """Option hilbert_exact: every row bit for bit equal to oracle_lib.hilbert (pocketfft's restatement), NaN as NaN."""
    cap = CAPS[name].cover(n)
    nf = cap + 3
    R = Report(name, n, nf, f"n={n}")
    x = _hilbert_rows(np.random.default_rng(n + 1), nf, n, cap, inf=False)   # (the oracle keeps two values of an Inf row finite; SciPy does not)
    distinct(x, R.head)
    d_out = _hilbert(x, True)
    step = 8 if n >= (1 << 18) else CHUNK
    with np.errstate(all="ignore"):
        for f0, f1 in chunks(nf, step):
            got = _rows_of(d_out, f0, f1).reshape(f1 - f0, 2 * n)
            want = np.stack(O.map_frames(O.hilbert, x[f0:f1])).view(np.float64)
            R.add("analytic signal bits", same_bits(got, want), got, want, f0)
    R.check()
    del d_out
    _free()


# ---- pss_demod WFM at decimation factor 1: k_wfm_rows_q1 ------------------------------------------------------------------------------
def test_wfm_factor_one_past_the_cap():
    """test_round6_complex128_buffers_vs_reference_goldens' factor-one WFM at 250 kS/s, target rate 130 000: float64 audio bits and
    np.int16(audio * 32767) equal to oracle_lib.demod_wfm(..., target_rate=130000) on every frame."""
    e, n, fs, tr = G.engine(), 512, 250000.0, 130000
    cap = CAPS["wfm_q1"].cover(n)
    nf = cap + 3
    R = Report("wfm_q1", n, nf, f"n={n} fs={fs:g} target {tr}")
    rng = np.random.default_rng(130)
    t = np.arange(n) / fs
    ph = 2 * np.pi * 75e3 * np.cumsum(np.sin(2 * np.pi * rng.uniform(300, 15e3, (nf, 1)) * t) +
                                      0.3 * np.sin(2 * np.pi * 19e3 * t), axis=1) / fs
    iq = (0.5 * np.exp(1j * ph) + 0.01 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))).astype(np.complex64)
    plant(iq, cap, last="full")
    distinct(iq, R.head)
    lp, pil, lmr, alpha = e.wfm_filters(fs)
    _, sos, zi = e.nfm_filters(fs)
    filt = dict(lp_sos=lp, pilot_sos=pil, lmr_sos=lmr, alpha=alpha, dec_sos=sos, dec_zi=zi)
    e.set_target_rate(float(tr))
    try:
        assert e.demod_out_len(L.MODE_WFM, n, fs) == n - 1
        d_pcm, d_au = sentinel((nf, n - 1, 2), torch.int16), sentinel((nf, n - 1, 2), torch.float64)
        e.demod(L.MODE_WFM, G.dev(iq), nf, n, fs, d_pcm, d_au)
        e.sync()
    finally:
        e.set_target_rate(22050)
    with np.errstate(all="ignore"):
        for f0, f1 in chunks(nf):
            want = np.stack(O.map_frames(lambda x: O.demod_wfm(x, fs, filt, target_rate=tr), iq[f0:f1]))
            au, pcm = _rows_of(d_au, f0, f1), _rows_of(d_pcm, f0, f1)
            R.add("float64 audio bits", same_bits(au, want), au, want, f0)
            wp = np.where(np.isnan(want * 32767.0), 0.0, np.trunc(want * 32767.0)).astype(np.int32).astype(np.int16)
            R.add("int16 PCM", pcm == wp, pcm, wp, f0)
    R.check()


# ---- the float64-row spectrum entry points -----------------------------------------------------------------------------------------------
def _tone_batch(n, nf, cap, dtype=np.complex64):
    """Distinct frames: a tone on a random (fractional) bin over noise 60 dB down, NaN / silent / Inf frames first, a tiny frame last."""
    rng = np.random.default_rng(n + nf)
    t = np.arange(n)
    x = np.exp(2j * np.pi * (rng.integers(0, n, (nf, 1)) + rng.random((nf, 1))) * t / n)
    x += 1e-3 * (rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n)))
    x = plant(x, cap)
    if dtype == np.complex128:
        x[3:] += 1e-9 * x[3:]                   # samples complex64 cannot hold
    return x.astype(dtype)


def _check_f64_rows(R, got, x, ref):
    """spectrum_bounds' float64 row bound on the finite frames (db_allowance of the norm-wise transform error, as
    test_spectrum_db_f64_rows applies it); the NaN-sample frame all NaN, the Inf-sample frame without a finite value."""
    R.add("NaN-sample frame all NaN", np.isnan(got[:1]), got[:1], ref[:1], 0)
    R.add("Inf-sample frame without a finite value", ~np.isfinite(got[2:3]), got[2:3], ref[2:3], 2)
    got[:1], got[2:3], ref[:1], ref[2:3], x = ref[1], ref[1], ref[1], ref[1], x.copy()     # the finite frames: 1 and 3 ..
    x[[0, 2]] = 0
    with np.errstate(all="ignore"):
        e = SB.db_allowance(ref, SB.delta(x))
        ok = (np.abs(got - ref) <= e) | SB._same_nonfinite(got, ref)
    R.add("float64 rows (spectrum_bounds)", ok, got, ref)


F64_CASES = [("spectrum_f64_r16", n, 0) for n in (256, 512, 1024, 2048, 4096)] + \
            [("spectrum_f64_plain", 16, 0), ("spectrum_f64_plain", 1024, 1), ("spectrum_f64_plain", 8192, 0)]


@pytest.mark.parametrize("name,n,plain", F64_CASES)
def test_spectrum_db_f64_past_the_cap(name, n, plain):
    e = G.engine()
    cap = CAPS[name].cover(n)
    nf = cap + 3
    R = Report(name, n, nf, f"n={n} f64_plain {plain}")
    x = _tone_batch(n, nf, cap)
    distinct(x, R.head)
    ref = np.stack(O.map_frames(O.compute_fft, x))
    d_db = sentinel((nf, n), torch.float64)
    e.set_option("f64_plain", plain)
    try:
        e.spectrum_db_f64(G.dev(x), nf, n, d_db)
        e.sync()
    finally:
        e.set_option("f64_plain", 0)
    _check_f64_rows(R, G.host(d_db), x, ref)
    R.check()


@pytest.mark.parametrize("n", [16, 4096])
def test_spectrum_db_c128_past_the_cap(n):
    e = G.engine()
    cap = CAPS["spectrum_c128"].cover(n)
    nf = cap + 3
    R = Report("spectrum_c128", n, nf, f"n={n}")
    x = _tone_batch(n, nf, cap, np.complex128)
    distinct(x, R.head)
    ref = np.stack(O.map_frames(O.compute_fft_c128, x))
    d_db = sentinel((nf, n), torch.float64)
    e.spectrum_db_c128(G.dev(x.view(np.float64).reshape(nf, n, 2)), nf, n, d_db)
    e.sync()
    _check_f64_rows(R, G.host(d_db), x, ref)
    R.check()


def test_spectrum_post_f64_past_the_cap():
    """k_post_f64 (option f64_plain): the post-processed rows bit for bit those of the oracle (np.convolve / np.median / the clamp), the
    rows' finite extremes equal, rows with a NaN, with infinities, a constant row and a row of nano-dB differences among them."""
    e, n = G.engine(), 1024
    cap = CAPS["post_f64"].cover(n)
    nf = cap + 3
    R = Report("post_f64", n, nf, f"n={n}")
    rng = np.random.default_rng(41)
    rows = rng.standard_normal((nf, n)) * rng.uniform(1, 8, (nf, 1)) - rng.uniform(20, 80, (nf, 1))
    rows[0, n // 2] = np.nan
    rows[1] = -47.25
    rows[2, 5:9] = np.inf
    rows[2, 700] = -np.inf
    rows[-1] = -50.0 + 1e-7 * rng.standard_normal(n)
    distinct(rows, R.head)
    d_p, d_lo, d_hi = sentinel((nf, n - 4), torch.float64), sentinel((nf,), torch.float64), sentinel((nf,), torch.float64)
    e.set_option("f64_plain", 1)
    try:
        e.spectrum_post_f64(G.dev(rows), nf, n, d_p, d_lo, d_hi)
        e.sync()
    finally:
        e.set_option("f64_plain", 0)
    post, lo, hi = G.host(d_p), G.host(d_lo), G.host(d_hi)
    with np.errstate(all="ignore"):
        want = np.stack(O.map_frames(O.postprocess, rows))
        fin = np.where(np.isfinite(want), want, np.nan)
        wlo = np.where(np.isfinite(want).any(axis=1), np.nanmin(fin, axis=1), np.inf)
        whi = np.where(np.isfinite(want).any(axis=1), np.nanmax(fin, axis=1), -np.inf)
    R.add("post-processed rows (bits)", same_bits(post, want), post, want)
    R.add("row minimum", same_bits(lo, wlo), lo, wlo)
    R.add("row maximum", same_bits(hi, whi), hi, whi)
    R.check()

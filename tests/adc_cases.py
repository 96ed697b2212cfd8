"""Shared by tests/test_adc_golden.py (CPU), tests/test_gpu_adc.py and tools/make_goldens_adc.py: read buffers as a radio delivers them —
8-, 12- and 16-bit ADC codes scaled to float32 — with the properties a continuous-valued test signal never has: components that are
exactly zero (of either sign), samples of equal magnitude, samples on a rail, discriminator products that cancel exactly.

Every buffer is built from INTEGER codes, so a zero is +0 unless the case says otherwise.  Plain seeded NumPy; no GPU import.

    grids    i8  code / 128        u8o  (code - 127.4) / 128  (no representable zero: a DC offset)
             i12 code / 2048       i16  code / 32768
    levels   floor ~0.7 LSB rms (mostly zeros)   weak ~2 LSB   mid 0.35 of full scale   clip 3 x full scale (long runs on the rails)
    signals  fm (phase walk)   am (carrier)   ssb (two tones)   mpx (stereo multiplex with a 19 kHz pilot, 75 kHz deviation)
    signs    "+" as built; "conj" (-0 in Q), "negre" (-0 in I), "neg" (-0 in both), "sprinkle" (-0 words at seeded positions)
    dead     all zero; a constant code; both rails stuck; one live sample; first / last sample zero

counts(x) returns what a case is there for; FLOORS holds, per case, lower bounds taken from what this generator yields (written beside
the numbers it yielded), so that a change to the generator cannot silently empty the cases.
"""
import zlib

import numpy as np

FS = 2.4e6
LENGTHS = (29, 1000, 1024, 4096, 16384, 32768)

# grid -> (scale, lowest code, highest code, offset)
GRIDS = {"i8": (128.0, -128, 127, 0.0), "u8o": (128.0, 0, 255, 127.4), "i12": (2048.0, -2048, 2047, 0.0), "i16": (32768.0, -32768, 32767, 0.0)}
LEVELS = ("floor", "weak", "mid", "clip")


def _signal(kind, n, fs, rng):
    """A unit-amplitude complex baseband signal of the named kind."""
    t = np.arange(n) / fs
    if kind == "fm":
        m = 0.5 * np.sin(2 * np.pi * 400 * t + 0.3) + 0.3 * np.sin(2 * np.pi * 1000 * t) + 0.2 * np.sin(2 * np.pi * 2500 * t)
        return np.exp(1j * (2 * np.pi * 5e3 * np.cumsum(m) / fs + rng.uniform(0, 6.28)))
    if kind == "am":
        m = 0.5 * np.sin(2 * np.pi * 40e3 * t) + 0.3 * np.sin(2 * np.pi * 90e3 * t + 0.1)
        return (1 + 0.5 * m) / 1.4 * np.exp(1j * 0.3)
    if kind == "ssb":
        return (0.65 * np.exp(2j * np.pi * 1500 * t) + 0.35 * np.exp(2j * np.pi * 2400 * t))
    if kind == "mpx":
        l, r = np.sin(2 * np.pi * 1000 * t), np.sin(2 * np.pi * 3000 * t + 0.3)
        mpx = 0.45 * (l + r) + 0.1 * np.sin(2 * np.pi * 19000 * t) + 0.45 * (l - r) * np.sin(2 * np.pi * 38000 * t)
        return np.exp(1j * (2 * np.pi * 75000 * np.cumsum(mpx) / fs + rng.uniform(0, 6.28)))
    raise ValueError(kind)


def quantise(z, grid):
    """Complex values in CODE units (1.0 = one LSB) -> complex64 on the grid: round to the nearest code, clip to the rails, scale."""
    scale, lo, hi, off = GRIDS[grid]
    out = np.empty(len(z), np.complex64)
    for part, comp in ((out.view(np.float32)[0::2], z.real), (out.view(np.float32)[1::2], z.imag)):
        code = np.clip(np.rint(comp + off), lo, hi).astype(np.int64)
        part[:] = ((code - off) / scale).astype(np.float32) if off else (code.astype(np.float32) / np.float32(scale))
    return out


def make(grid, level, kind, n, seed, fs=FS):
    """One quantised read buffer.  floor: 0.44 LSB rms of noise per component and the signal at 0.28 LSB (about 0.7 LSB rms in all);
    weak: 1.6 LSB of noise, the signal at 1.4; mid: the signal at 0.35 of full scale plus 1 LSB of noise; clip: the same at 3 x full
    scale."""
    rng = np.random.default_rng(seed)
    scale = GRIDS[grid][0]
    s = _signal(kind, n, fs, rng)
    noise = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    if level == "floor":
        z = 0.8 * (0.35 * s + noise * 0.55)
    elif level == "weak":
        z = 2.0 * (0.7 * s + noise * 0.8)
    elif level == "mid":
        z = 0.35 * scale * s + noise
    elif level == "clip":
        z = 3.0 * scale * s + noise
    else:
        raise ValueError(level)
    return quantise(z, grid)


def with_sign(x, sign, seed=0):
    """The zero-sign variants of a +0 buffer.  conj: -0 in Q wherever Q is zero; negre: -0 in I; neg: both; sprinkle: about a third of
    the zero words, at seeded positions, made -0."""
    x = np.array(x, np.complex64)
    w = x.view(np.float32)
    if sign == "+":
        return x
    if sign == "conj":
        w[1::2] = -w[1::2]
    elif sign == "negre":
        w[0::2] = -w[0::2]
    elif sign == "neg":
        w[:] = -w
    elif sign == "sprinkle":
        rng = np.random.default_rng(seed)
        zero = np.nonzero(w == 0)[0]
        pick = zero[rng.random(len(zero)) < 1 / 3]
        w[pick] = np.float32(-0.0)
    else:
        raise ValueError(sign)
    return x


def dead(which, n, grid="i8", seed=0):
    scale, lo, hi, off = GRIDS[grid]
    x = np.zeros(n, np.complex64)
    if which == "zero":
        pass
    elif which == "const":                      # a stuck converter: one nonzero code in both components
        x[:] = np.float32(3 / scale) + 1j * np.float32(-2 / scale)
    elif which == "const_eq":                   # I == Q exactly: sin(phi) = 1, cos(phi) = 0 in iq_correction
        x[:] = np.float32(5 / scale) * (1 + 1j)
    elif which == "rails":                      # both rails stuck
        x[:] = np.float32(hi / scale) + 1j * np.float32(lo / scale)
    elif which == "one_live":
        x[n // 3] = np.float32(7 / scale) + 1j * np.float32(-1 / scale)
    elif which == "i_only":                     # Q never leaves zero: q_amplitude = 0
        x = make(grid, "weak", "am", n, seed)
        x.view(np.float32)[1::2] = 0.0
    elif which in ("first_zero", "last_zero"):
        x = make(grid, "mid", "fm", n, seed)
        x[0 if which == "first_zero" else n - 1] = 0
    else:
        raise ValueError(which)
    return x


class Case:
    def __init__(self, name, iq, kind, golden=False):
        self.name, self.iq, self.kind, self.golden = name, iq, kind, golden
        self.n = len(iq)

    def __repr__(self):
        return f"Case({self.name}, n={self.n})"


# name, builder, golden?  (seeds are part of the name's meaning: changing one changes FLOORS and the fixture)
def _table():
    T = []

    def q(grid, level, kind, n, seed, sign="+", golden=False):
        x = with_sign(make(grid, level, kind, n, seed), sign, seed + 1000)
        T.append(Case(f"{grid}_{level}_{kind}_{n}" + ("" if sign == "+" else "_" + sign), x, kind, golden))

    def d(which, n, grid="i8", golden=False, seed=77):
        T.append(Case(f"dead_{which}_{n}" + ("" if grid == "i8" else "_" + grid), dead(which, n, grid, seed), "dead", golden))

    # the fixture's cases (tests/golden/adc.npz): short lengths, one full read buffer
    q("i8", "floor", "fm", 32768, 1, golden=True)
    for sign, seed in (("+", 2), ("conj", 2), ("negre", 2), ("neg", 2), ("sprinkle", 2)):
        q("i8", "floor", "mpx", 1024, seed, sign, golden=True)
    q("i8", "weak", "fm", 1000, 3, golden=True)
    q("i8", "weak", "fm", 1000, 3, "sprinkle", golden=True)
    q("u8o", "floor", "fm", 1000, 4, golden=True)
    q("u8o", "clip", "mpx", 29, 5, golden=True)
    q("i12", "weak", "ssb", 1024, 6, golden=True)
    q("i12", "clip", "am", 1000, 7, golden=True)
    q("i16", "mid", "mpx", 1024, 8, golden=True)
    q("i16", "floor", "am", 29, 9, "conj", golden=True)
    q("i8", "clip", "fm", 29, 10, golden=True)
    q("i8", "floor", "ssb", 29, 11, "neg", golden=True)
    q("i8", "mid", "am", 29, 12, "negre", golden=True)
    q("i12", "floor", "mpx", 29, 13, "sprinkle", golden=True)
    d("zero", 1024, golden=True)
    d("const", 1024, golden=True)
    d("rails", 1024, golden=True)
    d("one_live", 1024, golden=True)
    d("first_zero", 29, golden=True)
    d("last_zero", 1000, golden=True)
    d("const_eq", 29, golden=True)
    d("i_only", 29, golden=True)
    # beyond the fixture (compared with the oracle only): the other grid x level x signal x length combinations
    q("i8", "floor", "fm", 1024, 21)
    q("i8", "floor", "fm", 1024, 21, "conj")
    q("i8", "weak", "mpx", 1024, 22, "neg")
    q("i8", "mid", "ssb", 1024, 23)
    q("i8", "clip", "mpx", 1024, 24)
    q("i8", "clip", "am", 1024, 25, "negre")
    q("u8o", "weak", "am", 1024, 26)
    q("u8o", "mid", "mpx", 1024, 27)
    q("i12", "floor", "fm", 1024, 28, "sprinkle")
    q("i12", "mid", "fm", 1024, 29)
    q("i12", "clip", "ssb", 1024, 30)
    q("i16", "floor", "mpx", 1024, 31, "conj")
    q("i16", "weak", "fm", 1024, 32)
    q("i16", "clip", "fm", 1024, 33)
    d("zero", 1000); d("const", 1000, "i12"); d("rails", 1024, "i16"); d("one_live", 1000); d("first_zero", 1024); d("last_zero", 1024)
    d("i_only", 1024); d("const_eq", 1024)
    q("i8", "floor", "mpx", 4096, 41, "sprinkle")
    q("i12", "weak", "am", 4096, 42)
    q("i8", "clip", "ssb", 4096, 43)
    q("i8", "floor", "ssb", 16384, 44, "conj")
    q("i16", "weak", "mpx", 16384, 45)
    q("i8", "floor", "mpx", 32768, 46, "sprinkle")
    q("i12", "clip", "mpx", 32768, 47)
    q("u8o", "weak", "fm", 32768, 48)
    d("zero", 32768); d("one_live", 32768); d("rails", 16384)
    names = [c.name for c in T]
    assert len(set(names)) == len(names)
    return T


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _table()
    return _CASES


def golden_cases():
    return [c for c in cases() if c.golden]


def by_name(name):
    return {c.name: c for c in cases()}[name]


def of_length(n):
    return [c for c in cases() if c.n == n]


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


def counts(x):
    """What a buffer holds of the things the cases are there for (NumPy's own arithmetic; float32 like the demodulators')."""
    x = np.ascontiguousarray(x, np.complex64)
    w = x.view(np.float32)
    re, im = w[0::2], w[1::2]
    with np.errstate(all="ignore"):
        p = x[1:] * np.conj(x[:-1])
        ang = np.angle(p)
        a = np.abs(x)
        db = 10 * np.log10(np.abs(np.fft.fftshift(np.fft.fft(x * np.hamming(len(x))))) ** 2 + 1e-10)
    pw = p.view(np.float32)
    pre, pim = pw[0::2], pw[1::2]
    pi32 = np.float32(np.pi)
    return {
        "zero_samples": int(np.sum((re == 0) & (im == 0))),
        "neg_zero_words": int(np.sum((w == 0) & np.signbit(w))),
        "prod_im_neg0": int(np.sum((pim == 0) & np.signbit(pim))),
        "prod_im_pos0": int(np.sum((pim == 0) & ~np.signbit(pim))),
        "prod_re_neg0": int(np.sum((pre == 0) & np.signbit(pre))),
        "prod_re_pos0": int(np.sum((pre == 0) & ~np.signbit(pre))),
        "disc_pi": int(np.sum(np.abs(ang) == pi32)),
        "max_ties": int(np.sum(a == np.max(a))) if len(a) else 0,
        "rail_words": int(np.sum(np.abs(w) >= np.float32(127 / 128))),
        "db_m100": int(np.sum(db == -100.0)),
    }


def same_bits(a, b):
    """Equality of every bit of two float32 / float64 / complex arrays, -0 unequal to +0; NaN compared as NaN (any payload)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "c":
        f = np.float32 if a.dtype == np.complex64 else np.float64
        a, b = np.ascontiguousarray(a).view(f), np.ascontiguousarray(b).view(f)
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return bool(np.all((a.view(u) == b.view(u)) | nan))


def diff_bits(a, b):
    """For a failing same_bits: how many words differ, how many of them only in the sign of a zero, the largest absolute difference."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"dtype / shape {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    if a.dtype.kind == "c":
        f = np.float32 if a.dtype == np.complex64 else np.float64
        a, b = np.ascontiguousarray(a).view(f), np.ascontiguousarray(b).view(f)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    bad = ((a.view(u) != b.view(u)) & ~(na & nb)) | (na != nb)
    zero = bad & (a == 0) & (b == 0)
    with np.errstate(all="ignore"):
        d = np.abs(a - b)[bad & ~na & ~nb]
    return f"{int(bad.sum())} of {a.size} words differ ({int(zero.sum())} only in the sign of zero; NaN mismatch {int((na != nb).sum())}; max |d| {d.max() if d.size else 0})"


# Lower bounds on counts(), per case: about 0.9 of what the generator yielded when the case was written (the yielded number in the comment).
FLOORS = {
    "i8_floor_fm_32768": {'zero_samples': 14478, 'prod_im_neg0': 4226, 'prod_re_neg0': 1284, 'disc_pi': 1391, 'max_ties': 24},   # yielded: zero_samples 16087, prod_im_neg0 4696, prod_re_neg0 1427, disc_pi 1546, max_ties 27
    "i8_floor_mpx_1024": {'zero_samples': 444, 'prod_im_neg0': 151, 'prod_re_neg0': 44, 'disc_pi': 45, 'max_ties': 2},   # yielded: zero_samples 494, prod_im_neg0 168, prod_re_neg0 49, disc_pi 51, max_ties 2
    "i8_floor_mpx_1024_conj": {'zero_samples': 444, 'neg_zero_words': 655, 'prod_im_neg0': 144, 'prod_re_neg0': 44, 'disc_pi': 45, 'max_ties': 2},   # yielded: zero_samples 494, neg_zero_words 728, prod_im_neg0 161, prod_re_neg0 49, disc_pi 51, max_ties 2
    "i8_floor_mpx_1024_negre": {'zero_samples': 444, 'neg_zero_words': 633, 'prod_im_neg0': 144, 'prod_re_neg0': 44, 'disc_pi': 45, 'max_ties': 2},   # yielded: zero_samples 494, neg_zero_words 704, prod_im_neg0 161, prod_re_neg0 49, disc_pi 51, max_ties 2
    "i8_floor_mpx_1024_neg": {'zero_samples': 444, 'neg_zero_words': 1288, 'prod_im_neg0': 151, 'prod_re_neg0': 44, 'disc_pi': 45, 'max_ties': 2},   # yielded: zero_samples 494, neg_zero_words 1432, prod_im_neg0 168, prod_re_neg0 49, disc_pi 51, max_ties 2
    "i8_floor_mpx_1024_sprinkle": {'zero_samples': 444, 'neg_zero_words': 441, 'prod_im_neg0': 168, 'prod_re_neg0': 208, 'disc_pi': 209, 'max_ties': 2},   # yielded: zero_samples 494, neg_zero_words 491, prod_im_neg0 187, prod_re_neg0 232, disc_pi 233, max_ties 2
    "i8_weak_fm_1000": {'zero_samples': 48, 'prod_im_neg0': 37, 'prod_re_neg0': 25, 'disc_pi': 38},   # yielded: zero_samples 54, prod_im_neg0 42, prod_re_neg0 28, disc_pi 43
    "i8_weak_fm_1000_sprinkle": {'zero_samples': 48, 'neg_zero_words': 132, 'prod_im_neg0': 34, 'prod_re_neg0': 40, 'disc_pi': 53},   # yielded: zero_samples 54, neg_zero_words 147, prod_im_neg0 38, prod_re_neg0 45, disc_pi 59
    "u8o_floor_fm_1000": {'disc_pi': 71},   # yielded: disc_pi 79
    "u8o_clip_mpx_29": {'max_ties': 26, 'rail_words': 52},   # yielded: max_ties 29, rail_words 58
    "i12_weak_ssb_1024": {'zero_samples': 49, 'prod_im_neg0': 28, 'prod_re_neg0': 26, 'disc_pi': 34},   # yielded: zero_samples 55, prod_im_neg0 32, prod_re_neg0 29, disc_pi 38
    "i12_clip_am_1000": {'max_ties': 5, 'rail_words': 900},   # yielded: max_ties 5, rail_words 1000
    "i16_mid_mpx_1024": {},
    "i16_floor_am_29_conj": {'zero_samples': 12, 'neg_zero_words': 22, 'prod_im_neg0': 3, 'disc_pi': 1},   # yielded: zero_samples 14, neg_zero_words 25, prod_im_neg0 3, disc_pi 1
    "i8_clip_fm_29": {'rail_words': 26},   # yielded: rail_words 29
    "i8_floor_ssb_29_neg": {'zero_samples': 12, 'neg_zero_words': 38, 'prod_im_neg0': 4, 'disc_pi': 3, 'max_ties': 13},   # yielded: zero_samples 14, neg_zero_words 43, prod_im_neg0 4, disc_pi 3, max_ties 15
    "i8_mid_am_29_negre": {},
    "i12_floor_mpx_29_sprinkle": {'zero_samples': 11, 'neg_zero_words': 10, 'prod_im_neg0': 5, 'prod_re_neg0': 6, 'disc_pi': 8, 'max_ties': 2},   # yielded: zero_samples 13, neg_zero_words 12, prod_im_neg0 5, prod_re_neg0 6, disc_pi 8, max_ties 2
    "dead_zero_1024": {'zero_samples': 921, 'max_ties': 921, 'db_m100': 921},   # yielded: zero_samples 1024, max_ties 1024, db_m100 1024
    "dead_const_1024": {'max_ties': 921, 'db_m100': 1},   # yielded: max_ties 1024, db_m100 1
    "dead_rails_1024": {'max_ties': 921, 'rail_words': 1843, 'db_m100': 1},   # yielded: max_ties 1024, rail_words 2048, db_m100 1
    "dead_one_live_1024": {'zero_samples': 920, 'prod_im_neg0': 1},   # yielded: zero_samples 1023, prod_im_neg0 1
    "dead_first_zero_29": {'zero_samples': 1, 'prod_im_neg0': 1},   # yielded: zero_samples 1, prod_im_neg0 1
    "dead_last_zero_1000": {'zero_samples': 1},   # yielded: zero_samples 1
    "dead_const_eq_29": {'max_ties': 26},   # yielded: max_ties 29
    "dead_i_only_29": {'zero_samples': 5, 'prod_im_neg0': 5, 'disc_pi': 8},   # yielded: zero_samples 5, prod_im_neg0 5, disc_pi 8
    "i8_floor_fm_1024": {'zero_samples': 455, 'prod_im_neg0': 134, 'prod_re_neg0': 36, 'disc_pi': 37},   # yielded: zero_samples 506, prod_im_neg0 149, prod_re_neg0 40, disc_pi 42
    "i8_floor_fm_1024_conj": {'zero_samples': 455, 'neg_zero_words': 644, 'prod_im_neg0': 126, 'prod_re_neg0': 36, 'disc_pi': 37},   # yielded: zero_samples 506, neg_zero_words 716, prod_im_neg0 140, prod_re_neg0 40, disc_pi 42
    "i8_weak_mpx_1024_neg": {'zero_samples': 36, 'neg_zero_words': 362, 'prod_im_neg0': 20, 'prod_re_neg0': 18, 'disc_pi': 36},   # yielded: zero_samples 40, neg_zero_words 403, prod_im_neg0 23, prod_re_neg0 21, disc_pi 41
    "i8_mid_ssb_1024": {},
    "i8_clip_mpx_1024": {'max_ties': 182, 'rail_words': 1479},   # yielded: max_ties 203, rail_words 1644
    "i8_clip_am_1024_negre": {'rail_words': 921},   # yielded: rail_words 1024
    "u8o_weak_am_1024": {'disc_pi': 17},   # yielded: disc_pi 19
    "u8o_mid_mpx_1024": {},
    "i12_floor_fm_1024_sprinkle": {'zero_samples': 450, 'neg_zero_words': 432, 'prod_im_neg0': 174, 'prod_re_neg0': 189, 'disc_pi': 192},   # yielded: zero_samples 501, neg_zero_words 480, prod_im_neg0 194, prod_re_neg0 211, disc_pi 214
    "i12_mid_fm_1024": {},
    "i12_clip_ssb_1024": {'max_ties': 83, 'rail_words': 1324},   # yielded: max_ties 93, rail_words 1472
    "i16_floor_mpx_1024_conj": {'zero_samples': 441, 'neg_zero_words': 649, 'prod_im_neg0': 141, 'prod_re_neg0': 39, 'disc_pi': 48, 'max_ties': 3},   # yielded: zero_samples 491, neg_zero_words 722, prod_im_neg0 157, prod_re_neg0 44, disc_pi 54, max_ties 3
    "i16_weak_fm_1024": {'zero_samples': 39, 'prod_im_neg0': 20, 'prod_re_neg0': 24, 'disc_pi': 35},   # yielded: zero_samples 44, prod_im_neg0 23, prod_re_neg0 27, disc_pi 39
    "i16_clip_fm_1024": {'max_ties': 167, 'rail_words': 1405},   # yielded: max_ties 186, rail_words 1562
    "dead_zero_1000": {'zero_samples': 900, 'max_ties': 900, 'db_m100': 900},   # yielded: zero_samples 1000, max_ties 1000, db_m100 1000
    "dead_const_1000_i12": {'max_ties': 900, 'db_m100': 1},   # yielded: max_ties 1000, db_m100 1
    "dead_rails_1024_i16": {'max_ties': 921, 'rail_words': 1843, 'db_m100': 1},   # yielded: max_ties 1024, rail_words 2048, db_m100 1
    "dead_one_live_1000": {'zero_samples': 899, 'prod_im_neg0': 1},   # yielded: zero_samples 999, prod_im_neg0 1
    "dead_first_zero_1024": {'zero_samples': 1, 'prod_im_neg0': 1},   # yielded: zero_samples 1, prod_im_neg0 1
    "dead_last_zero_1024": {'zero_samples': 1},   # yielded: zero_samples 1
    "dead_i_only_1024": {'zero_samples': 184, 'prod_im_neg0': 135, 'disc_pi': 197},   # yielded: zero_samples 205, prod_im_neg0 150, disc_pi 219
    "dead_const_eq_1024": {'max_ties': 921, 'db_m100': 1},   # yielded: max_ties 1024, db_m100 1
    "i8_floor_mpx_4096_sprinkle": {'zero_samples': 1790, 'neg_zero_words': 1710, 'prod_im_neg0': 775, 'prod_re_neg0': 684, 'disc_pi': 698, 'max_ties': 6},   # yielded: zero_samples 1989, neg_zero_words 1901, prod_im_neg0 862, prod_re_neg0 760, disc_pi 776, max_ties 6
    "i12_weak_am_4096": {'zero_samples': 191, 'prod_im_neg0': 124, 'prod_re_neg0': 46, 'disc_pi': 168},   # yielded: zero_samples 213, prod_im_neg0 138, prod_re_neg0 52, disc_pi 187
    "i8_clip_ssb_4096": {'max_ties': 254, 'rail_words': 4302},   # yielded: max_ties 283, rail_words 4781
    "i8_floor_ssb_16384_conj": {'zero_samples': 7555, 'neg_zero_words': 10560, 'prod_im_neg0': 2038, 'prod_re_neg0': 595, 'disc_pi': 748, 'max_ties': 9},   # yielded: zero_samples 8395, neg_zero_words 11734, prod_im_neg0 2265, prod_re_neg0 662, disc_pi 832, max_ties 11
    "i16_weak_mpx_16384": {'zero_samples': 658, 'prod_im_neg0': 437, 'prod_re_neg0': 421, 'disc_pi': 619, 'max_ties': 2},   # yielded: zero_samples 732, prod_im_neg0 486, prod_re_neg0 468, disc_pi 688, max_ties 2
    "i8_floor_mpx_32768_sprinkle": {'zero_samples': 14396, 'neg_zero_words': 13939, 'prod_im_neg0': 6127, 'prod_re_neg0': 5363, 'disc_pi': 5526, 'max_ties': 35},   # yielded: zero_samples 15996, neg_zero_words 15488, prod_im_neg0 6808, prod_re_neg0 5959, disc_pi 6141, max_ties 39
    "i12_clip_mpx_32768": {'max_ties': 4692, 'rail_words': 45599},   # yielded: max_ties 5214, rail_words 50666
    "u8o_weak_fm_32768": {'disc_pi': 310},   # yielded: disc_pi 345
    "dead_zero_32768": {'zero_samples': 29491, 'max_ties': 29491, 'db_m100': 29491},   # yielded: zero_samples 32768, max_ties 32768, db_m100 32768
    "dead_one_live_32768": {'zero_samples': 29490, 'prod_im_neg0': 1},   # yielded: zero_samples 32767, prod_im_neg0 1
    "dead_rails_16384": {'max_ties': 14745, 'rail_words': 29491, 'db_m100': 1},   # yielded: max_ties 16384, rail_words 32768, db_m100 1
}

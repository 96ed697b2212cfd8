"""RDS test signals: from groups to the IQ of an FM broadcast station, NumPy only and no library code.

    groups -> 26-bit blocks (checkwords, offset words) -> differential coding -> biphase impulse pairs -> the standard's shaping filter
    H(f) = cos(pi f t_d / 4), |f| <= 2 / t_d, inverted NUMERICALLY on a fine grid (not the library's closed form) -> a 57 kHz subcarrier at a
    stated phase and frequency error -> multiplex with a 19 kHz pilot, an L + R tone and an L - R tone on 38 kHz -> FM at 75 kHz peak
    deviation, 4 kHz of it RDS -> a tuning error -> seeded noise.

tools/make_goldens_rds.py stores the seeds, the groups and the bits of every case in tests/golden/rds.npz; the IQ is regenerated here.
"""
import numpy as np

BIT_RATE = 1187.5
TD = 1.0 / BIT_RATE
POLY = 0x5B9                    # x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
OFFSETS = {'A': 0x0FC, 'B': 0x198, 'C': 0x168, "C'": 0x350, 'D': 0x1B4}
PAD_BITS = 16                   # filler bits in front of and behind the groups of a row
NOISE_SIGMA = 0.01              # per part, against a carrier of amplitude 1: 37 dB in the capture's own bandwidth
PI = 0x54A8
PS = "PSS TEST"
RADIOTEXT = "RADIO 1"


def checkword(info):
    r = int(info) << 10
    for b in range(25, 9, -1):
        if r & (1 << b):
            r ^= POLY << (b - 10)
    return r & 0x3FF


def block_bits(info, offset):
    w = (int(info) << 10) | (checkword(info) ^ offset)
    return [(w >> (25 - k)) & 1 for k in range(26)]


def group_bits(groups):
    """groups [n][4] information words -> the transmitted data bits, 104 a group."""
    out = []
    for g in np.asarray(groups).reshape(-1, 4):
        version_b = (int(g[1]) >> 11) & 1
        for info, name in zip(g, ('A', 'B', "C'" if version_b else 'C', 'D')):
            out += block_bits(info, OFFSETS[name])
    return np.array(out, np.uint8)


def station_groups(pi=PI, ps=PS, pty=10, tp=1):
    """Eight groups: 0A carrying the name, one 2B under the other text flag, two 2A carrying RADIOTEXT + 0x0D, one 0B."""
    def blk2(gtype, version_b, low5):
        return (gtype << 12) | (version_b << 11) | (tp << 10) | (pty << 5) | low5

    def two(s):
        return (ord(s[0]) << 8) | ord(s[1])

    rt = (RADIOTEXT + "\r").ljust(8)
    g0 = [[pi, blk2(0, 0, a), 0xE0CD, two(ps[2 * a:2 * a + 2])] for a in range(4)]
    g2a = [[pi, blk2(2, 0, a), two(rt[4 * a:4 * a + 2]), two(rt[4 * a + 2:4 * a + 4])] for a in range(2)]   # text flag 0
    g2b = [pi, blk2(2, 1, 0x10 | 0), pi, two("ab")]                                                            # text flag 1, address 0
    g0b = [pi, blk2(0, 1, 0), pi, two(ps[0:2])]
    return np.array([g0[0], g2b, g0[1], g2a[0], g0[2], g2a[1], g0[3], g0b], np.uint16)


_G_TABLE = None
G_STEP = 1.0 / 2048             # of a bit period
G_REACH = 6.0                   # bit periods either side


def shaping_table():
    """g(t), the impulse response of H(f), on a grid of G_STEP t_d over +-G_REACH t_d, scaled to g(0) = 1: the trapezoid rule over 4096
    steps of [0, 2 / t_d] (the integrand is even).  With v = f t_d the rule's error per value is below 2 h^2 / 12 (pi / 4 + 2 pi |tau|)^2
    over 4 / pi, h = 2 / 4096 (tests/test_rds_golden.py: PULSE_BOUND)."""
    global _G_TABLE
    if _G_TABLE is None:
        tau = np.arange(-int(G_REACH / G_STEP), int(G_REACH / G_STEP) + 1) * G_STEP          # t / t_d
        nu = np.linspace(0.0, 2.0, 4097)                                                      # f t_d
        w = np.full(nu.shape, nu[1] - nu[0])
        w[0] = w[-1] = 0.5 * (nu[1] - nu[0])
        hw = np.cos(np.pi * nu / 4.0) * w
        g = np.empty(tau.shape)
        for a in range(0, len(tau), 2048):
            g[a:a + 2048] = np.cos(2.0 * np.pi * np.outer(tau[a:a + 2048], nu)) @ hw
        _G_TABLE = g / (hw.sum())
    return _G_TABLE


def shaping(tau):
    """g at t = tau t_d by linear interpolation in the table (error below G_STEP^2 / 8 (4 pi)^2 = 5e-6); 0 outside the table."""
    g = shaping_table()
    x = (np.asarray(tau, np.float64) + G_REACH) / G_STEP
    return np.interp(x, np.arange(len(g)), g, left=0.0, right=0.0)


def golden_pulse(span_bits=4):
    """The receiver's matched filter from the numerical inversion: the biphase symbol sampled 16 times a bit, 16 span_bits + 1 taps."""
    k = np.arange(-8 * span_bits, 8 * span_bits + 1)
    return shaping((k + 4) / 16.0) - shaping((k - 4) / 16.0)


def data_bits(groups, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, 2, PAD_BITS).astype(np.uint8), group_bits(groups), rng.integers(0, 2, PAD_BITS).astype(np.uint8)])


def synth(groups, fs, seed, clock_ppm=0.0, sub_err_hz=0.0, sub_phase=0.7, tune_hz=0.0, wrap_side=-0.5, noise=NOISE_SIGMA, n_extra=0, audio=0.30):
    """-> (iq complex64, data bits uint8).  Symbol k of the row (k counts the filler bits too) is centred at t = (16 (k + 4) + wrap_side) /
    19000 s stretched by the clock error: wrap_side samples of the 19 kS/s grid from the wrap of the timing offset.  audio: the level of
    the L + R and of the L - R tone (0.30 each: 55 kHz peak deviation with the pilot and RDS)."""
    fs = float(fs)
    bits = data_bits(groups, seed)
    e = np.bitwise_xor.accumulate(bits)                       # differential coding from e[-1] = 0
    a = 2.0 * e.astype(np.float64) - 1.0
    td = TD / (1.0 + clock_ppm * 1e-6)
    t0 = (16 * 4 + wrap_side) / 19000.0
    n = int(np.ceil((t0 + (len(bits) + 4) * td) * fs)) + int(n_extra)
    t = np.arange(n) / fs
    s = np.zeros(n)
    for k in range(len(bits)):                                # the symbol: impulses a quarter bit either side of its centre
        c = t0 + k * td
        lo, hi = max(0, int((c - (G_REACH - 0.3) * td) * fs)), min(n, int((c + (G_REACH - 0.3) * td) * fs) + 1)
        tau = (t[lo:hi] - c) / td
        s[lo:hi] += a[k] * (shaping(tau + 0.25) - shaping(tau - 0.25))
    s /= 1.3                                                  # the symbol's peak is about 1.27
    mpx = (audio * np.sin(2 * np.pi * 1000.0 * t) + 0.09 * np.sin(2 * np.pi * 19000.0 * t)
           + audio * np.sin(2 * np.pi * 3000.0 * t) * np.sin(2 * np.pi * 38000.0 * t)
           + (4.0 / 75.0) * s * np.cos(2 * np.pi * (57000.0 + sub_err_hz) * t + sub_phase))
    phase = 2 * np.pi * np.cumsum(75e3 * mpx + tune_hz) / fs
    rng = np.random.default_rng(seed + 1)
    iq = np.exp(1j * phase) + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return iq.astype(np.complex64), bits


# name -> fs, clock error (ppm), subcarrier error (Hz), tuning error (Hz), wrap side, groups of the row, seed
CASES = {
    "fs240k_plain":      (240000, 0.0, 0.0, 0.0, -0.5, 8, 101),
    "fs240k_fast_clock": (240000, 100.0, 3.0, 10e3, -0.5, 8, 102),
    "fs250k_slow_clock": (250000, -100.0, -3.0, 0.0, -0.5, 8, 103),
    "fs400k_fast_clock": (400000, 100.0, 0.0, 10e3, 0.5, 8, 104),
    "fs400k_slow_clock": (400000, -100.0, 3.0, 0.0, 0.5, 8, 105),
    # the timing decision of a segment sees the mean position of its nine-segment window: a slow clock that starts half a sample below the wrap
    # is past it at the first decision, so this one starts a full sample below and crosses in the middle of the row
    "fs240k_fast_wrap":  (240000, 100.0, -3.0, 0.0, 0.4, 8, 108),
    "fs250k_slow_wrap":  (250000, -100.0, 3.0, 10e3, -1.0, 8, 109),
    "fs1024k":           (1024000, -100.0, 3.0, 10e3, -0.5, 6, 106),
    "fs2400k":           (2400000, 100.0, -3.0, 10e3, -0.5, 6, 107),
}


def case_groups(name):
    return station_groups()[:CASES[name][5]]


def case_iq(name):
    fs, ppm, sub, tune, side, _, seed = CASES[name]
    return synth(case_groups(name), fs, seed, clock_ppm=ppm, sub_err_hz=sub, tune_hz=tune, wrap_side=side)


def timing_offsets(bb, pulse):
    """The receiver's timing offset of every 1024-sample segment of a 19 kS/s row, restated with NumPy (float64 correlate, argmax): for
    tests that must know where a row's offset wraps."""
    bb = np.asarray(bb, np.complex128)
    c = (len(pulse) - 1) // 2
    y = np.correlate(np.concatenate([np.zeros(c), bb, np.zeros(c)]), np.asarray(pulse, np.float64), 'valid')
    n = len(bb)
    n_seg = (n + 1023) // 1024
    en = np.zeros((n_seg, 16))
    for s in range(n_seg):
        seg = np.abs(y[s * 1024:min(n, (s + 1) * 1024)]) ** 2
        for o in range(16):
            en[s, o] = seg[o::16].sum()
    return [int(np.argmax(en[max(0, s - 4):s + 5].sum(0))) for s in range(n_seg)]


def band_capture(stations, fs=2400000, seed=200):
    """A capture of the band: stations = [(offset_hz, pi, ps), ...], each a station_groups() row at half the audio level (33 kHz peak
    deviation: inside the +-90 kHz channel of a 100 kHz grid) moved to its offset, plus noise -> complex64."""
    rows = [synth(station_groups(pi=pi, ps=ps), fs, seed + 10 * k, audio=0.15, noise=0.0)[0] for k, (_, pi, ps) in enumerate(stations)]
    n = min(len(r) for r in rows)
    t = np.arange(n) / float(fs)
    x = sum(r[:n].astype(np.complex128) * np.exp(2j * np.pi * f * t) for r, (f, _, _) in zip(rows, stations))
    rng = np.random.default_rng(seed + 1)
    return (x + NOISE_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def noise_row(n, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def find_groups(tx_groups, rx_groups):
    """The indices in tx_groups of the received groups, in order -> list, or None where a received group was not transmitted in that order."""
    out, at = [], 0
    tx = [tuple(int(v) for v in g) for g in tx_groups]
    for g in rx_groups:
        g = tuple(int(v) for v in g)
        while at < len(tx) and tx[at] != g:
            at += 1
        if at == len(tx):
            return None
        out.append(at)
        at += 1
    return out

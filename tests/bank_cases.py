"""Captures and cases of the band-plan channeliser's fixtures (pss_bank: grids of 2^a 3^b 5^c channels) — shared by
tools/make_goldens_bank.py, tests/test_bank_golden.py and tests/test_gpu_bank.py (-m gpu).  NumPy only.

The fixture (tests/golden/bank.npz) stores results, never captures: every capture and every tap table is regenerated here from its seed
and pinned by a CRC.  The truth in it is the definition, y_c[m] = sum over k of h[k] x[m D + lead - k] exp(-2 pi i c j / M), evaluated
directly in np.longdouble (80-bit) with the phase reduced exactly, (c j) mod M in integers before any float.
"""
import numpy as np

from pfb_cases import capture, crc, half_ulp32  # noqa: F401  (re-exported to the tests)

VERSION = 1


def subset(M, n_out):
    """The instants and channels kept of a large case: first / last / middle instants; channels 0, 1, the band edge's neighbours, the
    last and one in between."""
    ins = sorted({0, 1, n_out // 2 - 1, n_out // 2, n_out // 2 + 1, n_out - 2, n_out - 1})
    ch = sorted({0, 1, M // 3 + 1, M // 2 - 1, M // 2, M // 2 + 1, M - 1})
    return tuple(ins), tuple(ch)


# (name, M, D, T, n, lead, instants, channels): instants / channels None = all of them
CASES = [
    ("m3", 3, 3, 7, 100, 3, None, None),
    ("m5_d2", 5, 2, 26, 203, 12, None, None),                    # D does not divide M
    ("m6", 6, 3, 121, 600, 60, None, None),
    ("m12_d5", 12, 5, 50, 500, 13, None, None),                  # D does not divide M
    ("m15_t1", 15, 15, 1, 203, 0, None, None),                   # odd, one tap
    ("m45_d1", 45, 1, 17, 150, 16, None, None),                  # no decimation
    ("m96", 96, 48, 1921, 4001, 960, None, None),
    ("m192", 192, 48, 3841, 8001, 1920) + subset(192, -(-8001 // 48)),
    ("m625", 625, 125, 2501, 6001, 1250) + subset(625, -(-6001 // 125)),     # only 5s
    ("m729", 729, 243, 2917, 7001, 1458) + subset(729, -(-7001 // 243)),     # only 3s
    ("m1000", 1000, 500, 20001, 40001, 10000) + subset(1000, -(-40001 // 500)),
]
TAP_CHANS = [3, 12, 192, 1000]             # pss_bank_default_taps against SciPy's firwin(20 M + 1, 1 / M), bit for bit

# the chain test's capture: two NFM stations in one 2.4 MS/s capture, on its 12.5 kHz grid (M = 192; plan_bank: D = 48, 50 kS/s)
CHAIN_FS = 2.4e6
CHAIN_SPACING = 12.5e3
CHAIN_M = 192
CHAIN_D = 48
CHAIN_N = 6144 * 48                      # 6144 samples a row at 50 kS/s: 3072 audio samples at 25 kS/s
CHAIN_SEED = 20261020
CHAIN_STATIONS = ((300e3, 24, 1000.0), (-412.5e3, 159, 2500.0))   # (offset from the centre, its row, tone)
CHAIN_DEVIATION = 2.5e3                  # a 12.5 kHz channel's deviation
CHAIN_SIGMA = 0.01


def factor(M):
    """M = 2^n2 3^n3 5^n5 -> (n2, n3, n5), or None."""
    e = []
    for p in (2, 3, 5):
        k = 0
        while M > 1 and M % p == 0:
            M //= p
            k += 1
        e.append(k)
    return tuple(e) if M == 1 else None


def bank_ok(M):
    return 2 <= M <= 1024 and factor(M) is not None


def case(name):
    for i, c in enumerate(CASES):
        if c[0] == name:
            return i, c
    raise KeyError(name)


def case_capture(name):
    i, c = case(name)
    return capture(c[4], 100 + i)


def case_taps(name):
    """As pfb_cases.case_taps: a Hamming-windowed sinc at 1 / M, scaled to unit sum, with a seeded ripple of 1e-3 so that no two taps
    are equal (a symmetric table would hide a reversed index)."""
    i, (_, M, _, T, _, _, _, _) = case(name)
    rng = np.random.default_rng([57, i])
    k = np.arange(T) - (T - 1) / 2
    w = 0.54 + 0.46 * np.cos(2 * np.pi * k / max(T - 1, 1)) if T > 1 else np.ones(1)
    h = np.sinc(k / M) * w
    h = h / h.sum() + 1e-3 / T * rng.standard_normal(T)
    return np.ascontiguousarray(h, np.float64)


def case_instants(name):
    _, (_, _, D, _, n, _, instants, _) = case(name)
    return list(range(-(-n // D))) if instants is None else list(instants)


def case_channels(name):
    _, (_, M, _, _, _, _, _, channels) = case(name)
    return list(range(M)) if channels is None else list(channels)


def chain_capture():
    """Two NFM stations (1 kHz tone at +300 kHz, 2.5 kHz tone at -412.5 kHz, 2.5 kHz deviation) and noise of sigma 0.01 a part, built as
    pfb_cases.chain_capture builds its own."""
    rng = np.random.default_rng(CHAIN_SEED)
    t = np.arange(CHAIN_N) / CHAIN_FS
    x = CHAIN_SIGMA * (rng.standard_normal(CHAIN_N) + 1j * rng.standard_normal(CHAIN_N))
    for off, _, tone in CHAIN_STATIONS:
        x = x + 0.5 * np.exp(1j * (2 * np.pi * off * t + (CHAIN_DEVIATION / tone) * np.sin(2 * np.pi * tone * t)))
    return x.astype(np.complex64)


U3, U5 = 7, 9       # roundings on the longest path of a radix-3 / radix-5 stage, as pyspecsdr_amd/csrc/pss_bank.h counts them


def f64_units(M, T):
    """The float64 term of the output bound in units of 2^-53 sum|h| max(|xr|, |xi|): the chain's ceil(T / M) steps, u(r) for every
    stage (u(2) = 4 as pfb_cases.f64_units counts it, u(3) = 7, u(5) = 9), and 8."""
    n2, n3, n5 = factor(M)
    return -(-T // M) + 4 * n2 + U3 * n3 + U5 * n5 + 8


def bound_excess(y32, ref_hi, ref_lo, M, T, sum_abs_h, xmax):
    """pfb_cases.bound_excess with this bank's unit count -> (the largest error minus its bound over both parts — negative when every
    output is inside; the largest float64-part error in units of 2^-53 sum|h| xmax)."""
    y = np.asarray(y32).astype(np.complex128)
    unit = 2.0 ** -53 * sum_abs_h * xmax
    worst, used = -np.inf, -np.inf
    for a, hi, lo in ((y.real, ref_hi.real, ref_lo.real), (y.imag, ref_hi.imag, ref_lo.imag)):
        err = np.abs((a - hi) - lo)
        half = half_ulp32(np.maximum(np.abs(a), np.abs(hi)))
        worst = max(worst, float(np.max(err - (half + f64_units(M, T) * unit))))
        used = max(used, float(np.max(err - half)) / unit)
    return worst, used

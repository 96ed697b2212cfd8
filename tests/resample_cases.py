"""The rational resampler's cases, shared by tests/test_resample_golden.py, tests/test_gpu_resample.py and tools/make_goldens_resample.py:
seeded rows (regenerated here, never stored: tests/golden/resample.npz pins their bytes with crc_<case>), the ratios and lengths the issue
lists, and the statement of pyspecsdr_amd/csrc/pss_resample.h restated in Python integers (geometry, halo, one output)."""
import math
import zlib

import numpy as np

# up, down as GIVEN: 12/50 is not reduced, 7/7 is a copy
RATIOS = ((2, 3), (3, 2), (1, 4), (5, 1), (24, 25), (441, 500), (441, 1000), (147, 160), (160, 147), (12, 50), (7, 7))
DTYPES = (np.float32, np.float64, np.complex64)
CODES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.complex64): 2}      # PSS_RS_*
LONG = 4099


def reduced(up, down):
    g = math.gcd(up, down)
    return up // g, down // g


def default_n_taps(up, down):
    u, d = reduced(up, down)
    return 1 if u == d == 1 else 20 * max(u, d) + 1


def geometry(n_in, up, down, n_taps):
    """pss_resample.h's plan in Python integers -> dict(up, down, n_out, n_pre_pad, n_post_pad, n_pre_remove, hpp)."""
    u, d = reduced(up, down)
    n_out = -(-n_in * u // d)
    if u == d == 1:
        return dict(up=1, down=1, n_out=n_out, n_pre_pad=0, n_post_pad=0, n_pre_remove=0, hpp=0)
    half_len = (n_taps - 1) // 2
    pre = d - half_len % d
    pre_remove = (half_len + pre) // d
    post = 0
    while ((n_in - 1) * u + n_taps + pre + post - 1) // d + 1 < n_out + pre_remove:       # SciPy's own loop
        post += 1
    return dict(up=u, down=d, n_out=n_out, n_pre_pad=pre, n_post_pad=post, n_pre_remove=pre_remove, hpp=-(-(pre + n_taps + post) // u))


def halo(n_in, up, down, n_taps, j_begin, j_end):
    """The samples [lo, hi) of the row that outputs [j_begin, j_end) read (j_begin < j_end); lo == hi: none."""
    g = geometry(n_in, up, down, n_taps)
    if g["up"] == g["down"] == 1:
        return j_begin, j_end
    lo = max(0, (j_begin + g["n_pre_remove"]) * g["down"] // g["up"] - g["hpp"] + 1)
    hi = min(n_in - 1, (j_end - 1 + g["n_pre_remove"]) * g["down"] // g["up"]) + 1
    return (lo, hi) if lo < hi else (0, 0)


def output_py(j, n_in, up, down, taps, dtype, sample):
    """One output by the statement, in NumPy scalars of the row's real type.  sample(i) -> the row's sample i (0 <= i < n_in)."""
    g = geometry(n_in, up, down, len(taps))
    real = np.float32 if np.dtype(dtype) != np.float64 else np.float64
    u, d, hpp = g["up"], g["down"], g["hpp"]
    q = (j + g["n_pre_remove"]) * d
    t, xi = q % u, q // u
    lo = xi - hpp + 1
    acc_r, acc_i = real(0), real(0)
    cplx = np.dtype(dtype) == np.complex64
    for i in range(max(lo, 0), min(xi, n_in - 1) + 1):
        k = (hpp - 1 - (i - lo)) * u + t - g["n_pre_pad"]
        h = real(taps[k]) * real(u) if 0 <= k < len(taps) else real(0)
        x = sample(i)
        if cplx:
            acc_r = acc_r + np.float32(x.real) * h
            acc_i = acc_i + np.float32(x.imag) * h
        else:
            acc_r = acc_r + real(x) * h
    return np.complex64(complex(acc_r, acc_i)) if cplx else acc_r


def lengths(up, down):
    """1, 2, hpp - 1, hpp, hpp + 1 (hpp: a long row's), 257, 4099 — duplicates dropped, order kept."""
    hpp = geometry(LONG, up, down, default_n_taps(up, down))["hpp"]
    out = []
    for n in (1, 2, hpp - 1, hpp, hpp + 1, 257, LONG):
        if n >= 1 and n not in out:
            out.append(n)
    return out


def row(seed, n, dtype):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if np.dtype(dtype) == np.complex64:
        x = x + 1j * rng.standard_normal(n)
    return x.astype(dtype)


def special_row(dtype):
    """300 samples with a NaN, an inf and a -0."""
    x = row(977, 300, dtype)
    x[5], x[100], x[200], x[299] = np.nan, np.inf, -0.0, -np.inf
    return x


def golden_cases():
    """-> list of (name, up, down, x).  Every ratio at every length; the short lengths in all three types, the long row in one type per
    ratio (the types rotate), which keeps the golden file small."""
    cases = []
    for r, (up, down) in enumerate(RATIOS):
        for n in lengths(up, down):
            for t, dt in enumerate(DTYPES):
                if n == LONG and t != r % 3:
                    continue
                cases.append((f"r{up}_{down}_n{n}_{np.dtype(dt).name}", up, down, row(1000 * r + 10 * n + t, n, dt)))
    for dt in (np.float32, np.float64):
        for up, down in ((2, 3), (441, 500), (5, 1), (1, 4)):
            cases.append((f"special_{up}_{down}_{np.dtype(dt).name}", up, down, special_row(dt)))
    return cases


def crc(x):
    return np.uint32(zlib.crc32(np.ascontiguousarray(x).tobytes()))

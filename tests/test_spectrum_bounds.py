"""The float64 bounds of spectrum_bounds.py catch partial losses of precision that the 1e-4 contract lets through, and an independent
float64 FFT (scipy.fft) meets them with a wide margin.  CPU only: the oracle (oracle/pss_oracle.c) gives the reference rows."""
import numpy as np
import pytest
import scipy.fft

import oracle_lib as O
import spectrum_bounds as SB

LENGTHS = [256, 1024, 4096, 32768]


def _frames(n):
    """Tone on a bin + noise ~120 dB down, and white noise (complex64, as the SDR delivers them)."""
    rng = np.random.default_rng(n)
    t = np.arange(n)
    tone = np.exp(2j * np.pi * (n // 8) * t / n) + 1e-6 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    noise = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return np.stack([tone, noise]).astype(np.complex64)


def _db(X):
    return 10 * np.log10(np.abs(np.fft.fftshift(X, axes=-1)) ** 2 + 1e-10)


def _four_step_f32_intermediate(xw):
    """X = DFT_n of xw by the n = n1 x n2 split (n1 = 256, or 16 for n = 256), the column transforms' output rounded to complex64."""
    n = xw.shape[-1]
    n1 = 16 if n == 256 else 256
    n2 = n // n1
    a = xw.reshape(-1, n2, n1)                                       # a[j2, j1] = x[j1 + n1 j2]
    y = scipy.fft.fft(a, axis=1)                                     # over j2 -> k2
    k2, j1 = np.arange(n2)[:, None], np.arange(n1)[None, :]
    y = (y * np.exp(-2j * np.pi * k2 * j1 / n)).astype(np.complex64).astype(np.complex128)
    z = scipy.fft.fft(y, axis=2)                                     # over j1 -> k1; X[k2 + n2 k1]
    return np.transpose(z, (0, 2, 1)).reshape(-1, n)


@pytest.mark.parametrize("n", LENGTHS)
def test_bounds_catch_float32_losses_and_admit_float64(n):
    x = _frames(n)
    ref = np.stack(O.map_frames(O.compute_fft, list(x)))
    e = SB.db_allowance(ref, SB.delta(x))
    w64 = np.hamming(n)
    xw = x.astype(np.complex128) * w64

    mutants = {
        "float32 window": _db(scipy.fft.fft(x.astype(np.complex128) * w64.astype(np.float32).astype(np.float64), axis=1)),
        "float32 intermediate": _db(_four_step_f32_intermediate(xw)),
        "complex64 transform": _db(scipy.fft.fft(xw.astype(np.complex64), axis=1).astype(np.complex128)),
    }
    for name, rows in mutants.items():
        for chk in (SB.check_f64, SB.check_fast):
            bad = chk(rows, ref, e)
            assert bad is not None and bad[2] >= min(64, n // 8), f"{name} at {n}: {chk.__name__} finds {bad}"
        assert SB.check_exact(rows.astype(np.float32), ref, e) is not None, f"{name} at {n}: check_exact passes it"

    good = _db(scipy.fft.fft(xw, axis=1))
    assert np.all(np.abs(good - ref) <= 0.1 * e), f"scipy.fft at {n}: margin {np.max(np.abs(good - ref) / e):.3g} of the bound"
    assert SB.check_exact(good.astype(np.float32), ref, e) is None
    assert SB.check_fast(good.astype(np.float32), ref, e) is None


def test_bound_constants():
    """KAPPA from the norm-wise FFT bound (not fitted); the fast allowance never looser than the golden test's 1e-6 max(|ref|, 1)."""
    assert SB.KAPPA == 21
    ref = np.concatenate([np.linspace(-3100, 3100, 20001), np.linspace(-2, 2, 4001), [-100.0, 0.0]])
    assert np.all(SB.fast_allowance(ref) <= 1e-6 * np.maximum(np.abs(ref), 1.0))
    # on the -100 dB floor of an all-zero frame the allowance is the evaluation's alone, and finite
    e = SB.db_allowance(np.full((1, 8), -100.0), SB.delta(np.zeros((1, 8), np.complex64)))
    assert np.all(np.isfinite(e)) and np.all(e < 1e-12)
    # a near-zero bin beside a large one: the exact form stays finite and covers delta^2 >> 1e-10
    e = SB.db_allowance(np.array([[-100.0, 300.0]]), np.array([1e-3]))
    assert np.isfinite(e).all() and e[0, 0] > 39
    assert SB.transform_len(1) == 1 and SB.transform_len(16) == 16 and SB.transform_len(8) == 1 << 17
    assert SB.transform_len(65537) == 1 << 18 and SB.transform_len(240000) == 1 << 19

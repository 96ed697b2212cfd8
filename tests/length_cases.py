"""Frame lengths and seeded read buffers of the length sweeps — shared by tests/test_gpu_length_sweep.py (-m gpu), tests/test_lengths_golden.py
and tools/make_goldens_lengths.py.  NumPy only.

Every kernel family has structure that depends on the frame length; the lists walk each regime and its edges:

  REDUCE_LENGTHS    NumPy's summation tree as pss_npsum.h states it (build_forest; get_plan / get_red_plan group it): sequential below 8, eight accumulators and
                    a tail up to 128, uneven halves above (129..255 the first), 8192-element chunks and 8-chunk groups with tails of
                    fewer than 8 elements (b + d, d = -9..9), a full group plus one chunk (73 728) and two groups plus one (139 264).
  DEMOD_LENGTHS     every residue of M = n - 1 modulo the forward kernels' chunk sizes (24 for k_nfm_fwd after a 64-output prologue, 16
                    for k_wfm_fwd, the 64-sample blocks of L = n + 53 in k_wfm_mrg / k_iir4_sys) and of n_out = ceil((n - 1) / q).
  AM_SSB_LENGTHS    the same after 1..28 (AM and SSB take any length).
  CLASSIFY_LENGTHS  k_cls_welch_short below 1024, the segment count stepping at 1024 + 512 k, the 2048-sample unwrap chunks.
"""
import hashlib

import numpy as np


def _window(b, ds):
    return [b + d for d in ds]


REDUCE_LENGTHS = sorted(set(range(1, 2200))
                        | {n for b in (8192, 16384, 24576, 32768, 65536, 131072) for n in _window(b, range(-9, 10))}
                        | {n for b in (73728, 139264) for n in _window(b, (-1, 0, 1, 7, 8, 9))})
DEMOD_LENGTHS = list(range(29, 420)) + list(range(1020, 1030)) + list(range(2044, 2054))
AM_SSB_LENGTHS = list(range(1, 29)) + DEMOD_LENGTHS
CLASSIFY_LENGTHS = (list(range(1, 40)) + list(range(1018, 1032)) + list(range(1530, 1542)) + list(range(2044, 2054))
                    + list(range(4094, 4100)) + [6145, 6146])
C128_LENGTHS = list(range(1, 301)) + list(range(8185, 8201))
# the lengths tests/golden/lengths.npz pins the oracle at (tools/make_goldens_lengths.py): demodulators and classifier at the first 24,
# the scalar and iq_correction outputs at all 28
GOLDEN_DEMOD_LENGTHS = [29, 30, 37, 52, 53, 64, 89, 100, 128, 129, 152, 153, 200, 255, 256, 257, 333, 419, 1023, 1024, 1025, 2047, 2048, 2049]
GOLDEN_LONG_LENGTHS = [8193, 8199, 65537, 65543]
GOLDEN_LENGTHS = GOLDEN_DEMOD_LENGTHS + GOLDEN_LONG_LENGTHS

assert len(REDUCE_LENGTHS) == 2325 and len(DEMOD_LENGTHS) == 411 and len(AM_SSB_LENGTHS) == 439 and len(CLASSIFY_LENGTHS) == 83
assert set(GOLDEN_DEMOD_LENGTHS) <= set(DEMOD_LENGTHS) and set(GOLDEN_LONG_LENGTHS) <= set(REDUCE_LENGTHS) and len(GOLDEN_LENGTHS) == 28

_KINDS = {"fm": 1, "iq": 2, "power": 3, "c128": 4}


def _rng(kind, n, seed):
    return np.random.default_rng([_KINDS[kind], int(n), int(seed)])


def _noise(rng, nf, n):
    return rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))


def fm_frames(nf, n, seed=0):
    """FM-like read buffers for the demodulators and the classifier: a random phase walk (its step size drawn per frame) plus noise."""
    rng = _rng("fm", n, seed)
    ph = np.cumsum(rng.standard_normal((nf, n)) * rng.uniform(0.05, 0.3, (nf, 1)), axis=1)
    return (0.5 * np.exp(1j * ph) + 0.02 * _noise(rng, nf, n)).astype(np.complex64)


def iq_frames(nf, n, seed=0):
    """The offset, imbalanced noise of test_iq_correction_batch_vs_oracle: what iq_correction is meant to repair."""
    rng = _rng("iq", n, seed)
    return ((rng.standard_normal((nf, n)) * 0.3 + 0.04) + 1j * (rng.standard_normal((nf, n)) * 0.2 - 0.03)).astype(np.complex64)


def power_frames(nf, n, seed=0):
    """Noise times 2^k, k drawn per sample from -8..3: terms of very different size, so that a float32 sum taken in another order than
    NumPy's rounds differently."""
    rng = _rng("power", n, seed)
    return (_noise(rng, nf, n) * np.exp2(rng.integers(-8, 4, (nf, n)))).astype(np.complex64)


def c128_frames(nf, n, seed=0):
    """complex128 read buffers whose values complex64 cannot hold: a tone over noise times 2^k."""
    rng = _rng("c128", n, seed)
    x = _noise(rng, nf, n) * np.exp2(rng.integers(-8, 4, (nf, n))) + 0.3 * np.exp(2j * np.pi * rng.uniform(-0.4, 0.4, (nf, 1)) * np.arange(n))
    return np.ascontiguousarray(x * (1.0 + 1e-9 * rng.standard_normal((nf, n))), dtype=np.complex128)


def repeats(frames):
    """How many frames of a batch repeat another one (0 for every batch the sweeps use: asserted on the host)."""
    digests = {hashlib.blake2b(np.ascontiguousarray(row).tobytes(), digest_size=16).digest() for row in frames}
    return len(frames) - len(digests)

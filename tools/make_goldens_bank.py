"""Write tests/golden/bank.npz: the truth the band-plan channeliser's host twin (pss_h_bank, and through it k_bank) is held to.  NumPy
and SciPy only; DATA only.  Captures and tap tables are not stored: tests/bank_cases.py regenerates them from their seeds, `crc_<case>`
and `hcrc_<case>` pin their bytes.

    python tools/make_goldens_bank.py

  cases   the definition, evaluated directly as tools/make_goldens_pfb.py does (80-bit long double, the phase reduced exactly in
          integers; aborts where longdouble is narrower).  That file's `truth` pins cos / sin at q = M // 2, M // 4 and 3 M // 4 to the
          quarter turns, which is right only where 4 divides M; `truth_any` below is the same evaluation with each quarter turn pinned
          only where M holds it, and is checked against `truth` on every case with 4 | M.  Stored as a float64 pair (hi, lo) through
          that file's `hi_lo`, for the instants and channels bank_cases names, beside sum|h| and max(|xr|, |xi|).
  taps    SciPy's firwin(20 M + 1, 1 / M) for M = 3, 12, 192, 1000.
  chain   the seed of the two-station capture and the audio bins its tones land in (1 kHz -> 82, 2.5 kHz -> 205 of a 2048-sample
          spectrum at 25 kS/s), checked here with a plain mixer, SciPy's filter and a plain discriminator.
"""
import os
import sys

import numpy as np
import scipy
import scipy.signal as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bank_cases as BC  # noqa: E402
from make_goldens_pfb import LD, hi_lo, truth  # noqa: E402  (the import aborts where np.longdouble is narrower than 80 bits)


def truth_any(x, h, M, D, lead, instants, channels):
    """make_goldens_pfb.truth for any M -> (re, im) long double [len(channels)][len(instants)]."""
    n, T = len(x), len(h)
    two_pi = LD(8) * np.arctan(LD(1))
    ang = two_pi * (np.arange(M).astype(LD) / LD(M))
    cos_t, sin_t = np.cos(ang), np.sin(ang)
    for num, (c, s) in ((0, (1, 0)), (1, (0, 1)), (2, (-1, 0)), (3, (0, -1))):
        if (num * M) % 4 == 0:
            cos_t[num * M // 4], sin_t[num * M // 4] = LD(c), LD(s)          # the quarter turns exactly, where M has them
    xr, xi, hl = x.real.astype(LD), x.imag.astype(LD), h.astype(LD)
    re = np.zeros((len(channels), len(instants)), LD)
    im = np.zeros_like(re)
    k = np.arange(T, dtype=np.int64)
    for a, m in enumerate(instants):
        j = m * D + lead - k
        ok = (j >= 0) & (j < n)
        jj, hh = j[ok], hl[k[ok]]
        pr, pi = hh * xr[jj], hh * xi[jj]                         # 53 x 24 bits of mantissa: rounded once to 64
        for b, c in enumerate(channels):
            q = (c * jj) % M                                      # int64: c < 2^10, j < 2^40 here
            C, S = cos_t[q], sin_t[q]
            re[b, a] = np.sum(pr * C + pi * S)                    # (pr + i pi) (C - i S)
            im[b, a] = np.sum(pi * C - pr * S)
    return re, im


def main():
    d = {"version": np.array(BC.VERSION), "scipy": np.array(scipy.__version__)}
    for M in BC.TAP_CHANS:
        d[f"taps_{M}"] = ss.firwin(20 * M + 1, 1.0 / M)
    for name, M, D, T, n, lead, _, _ in BC.CASES:
        x, h = BC.case_capture(name), BC.case_taps(name)
        assert len(x) == n and len(h) == T
        d[f"crc_{name}"] = np.array(BC.crc(x), np.uint32)
        d[f"hcrc_{name}"] = np.array(BC.crc(h), np.uint32)
        ins, ch = BC.case_instants(name), BC.case_channels(name)
        re, im = truth_any(x, h, M, D, lead, ins, ch)
        if M % 4 == 0:
            re0, im0 = truth(x, h, M, D, lead, ins[:3], ch)
            assert np.array_equal(re0, re[:, :3]) and np.array_equal(im0, im[:, :3]), name
        (rh, rl), (ih, il) = hi_lo(re), hi_lo(im)
        d[f"ref_hi_{name}"] = rh + 1j * ih
        d[f"ref_lo_{name}"] = rl + 1j * il
        d[f"sumh_{name}"] = np.array(np.abs(h).sum())
        d[f"xmax_{name}"] = np.array(max(np.abs(x.real).max(), np.abs(x.imag).max()), np.float64)
        print(name, d[f"ref_hi_{name}"].shape, flush=True)
    # the chain: which audio bin each station's tone lands in
    x = BC.chain_capture()
    d["chain_seed"] = np.array(BC.CHAIN_SEED)
    d["chain_crc"] = np.array(BC.crc(x), np.uint32)
    bins = []
    h = ss.firwin(20 * BC.CHAIN_M + 1, 1.0 / BC.CHAIN_M)
    t = np.arange(BC.CHAIN_N)
    for off, _, _ in BC.CHAIN_STATIONS:
        z = x.astype(np.complex128) * np.exp(-2j * np.pi * (off / BC.CHAIN_FS) * t)
        z = ss.lfilter(h, 1.0, np.concatenate((z, np.zeros(len(h) // 2))))[len(h) // 2:][::BC.CHAIN_D]
        audio = np.angle(z[1:] * np.conj(z[:-1]))[::2][:2048]            # a plain discriminator at 50 kS/s, every second sample: 25 kS/s
        spec = np.abs(np.fft.rfft((audio - audio.mean()) * np.hanning(len(audio))))
        spec[:2] = 0
        bins.append(int(np.argmax(spec)))
    assert bins == [82, 205], bins
    d["chain_bins"] = np.array(bins, np.int32)
    out = os.path.join(ROOT, "tests", "golden", "bank.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

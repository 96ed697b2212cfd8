"""Write tests/golden/pfb.npz: the truth the polyphase channeliser's host twin (and through it the kernel) is held to.  NumPy and SciPy
only; DATA only.  Captures and tap tables are not stored: tests/pfb_cases.py regenerates them from their seeds, `crc_<case>` and
`hcrc_<case>` pin their bytes.

    python tools/make_goldens_pfb.py

  cases   the definition, evaluated directly: y_c[m] = sum over k of h[k] x[j] exp(-2 pi i c j / M), j = m D + lead - k, x = 0 outside
          the capture — every product and the sum in np.longdouble (80-bit; aborts where longdouble is narrower), the phase reduced
          exactly, q = (c j) mod M in Python-sized integers, and cos / sin of 2 pi q / M from a long double table.  Stored as a float64
          pair (hi, lo) with hi + lo the 80-bit value, for the instants and channels pfb_cases names, beside sum|h| and max(|xr|, |xi|).
  taps    SciPy's firwin(20 M + 1, 1 / M) for M = 2, 64, 1024.
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
import pfb_cases as PC  # noqa: E402

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    sys.exit("np.longdouble has fewer than 64 bits of precision here: the truth needs the 80-bit format")


def truth(x, h, M, D, lead, instants, channels):
    """-> (re, im) long double [len(channels)][len(instants)]."""
    n, T = len(x), len(h)
    two_pi = LD(8) * np.arctan(LD(1))
    ang = two_pi * (np.arange(M).astype(LD) / LD(M))             # q / M is exact for a power of two
    cos_t, sin_t = np.cos(ang), np.sin(ang)
    for q, (c, s) in ((0, (1, 0)), (M // 2, (-1, 0))) + (((M // 4, (0, 1)), (3 * M // 4, (0, -1))) if M >= 4 else ()):
        cos_t[q], sin_t[q] = LD(c), LD(s)                         # the quarter turns exactly
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


def hi_lo(v):
    hi = v.astype(np.float64)
    return hi, (v - hi.astype(LD)).astype(np.float64)


def main():
    d = {"version": np.array(PC.VERSION), "scipy": np.array(scipy.__version__)}
    for M in PC.TAP_CHANS:
        d[f"taps_{M}"] = ss.firwin(20 * M + 1, 1.0 / M)
    for name, M, D, T, n, lead, _, _ in PC.CASES:
        x, h = PC.case_capture(name), PC.case_taps(name)
        assert len(x) == n and len(h) == T
        d[f"crc_{name}"] = np.array(PC.crc(x), np.uint32)
        d[f"hcrc_{name}"] = np.array(PC.crc(h), np.uint32)
        re, im = truth(x, h, M, D, lead, PC.case_instants(name), PC.case_channels(name))
        (rh, rl), (ih, il) = hi_lo(re), hi_lo(im)
        d[f"ref_hi_{name}"] = rh + 1j * ih
        d[f"ref_lo_{name}"] = rl + 1j * il
        d[f"sumh_{name}"] = np.array(np.abs(h).sum())
        d[f"xmax_{name}"] = np.array(max(np.abs(x.real).max(), np.abs(x.imag).max()), np.float64)
        print(name, d[f"ref_hi_{name}"].shape, flush=True)
    # the chain: which audio bin each station's tone lands in
    x = PC.chain_capture()
    d["chain_seed"] = np.array(PC.CHAIN_SEED)
    d["chain_crc"] = np.array(PC.crc(x), np.uint32)
    bins = []
    h = ss.firwin(20 * PC.CHAIN_M + 1, 1.0 / PC.CHAIN_M)
    t = np.arange(PC.CHAIN_N)
    for off, _, _ in PC.CHAIN_STATIONS:
        z = x.astype(np.complex128) * np.exp(-2j * np.pi * (off / PC.CHAIN_FS) * t)
        z = ss.lfilter(h, 1.0, np.concatenate((z, np.zeros(len(h) // 2))))[len(h) // 2:][::PC.CHAIN_D]
        audio = np.angle(z[1:] * np.conj(z[:-1]))[::3][:2048]            # a plain discriminator at 75 kS/s, every third sample: 25 kS/s
        spec = np.abs(np.fft.rfft((audio - audio.mean()) * np.hanning(len(audio))))
        spec[:2] = 0
        bins.append(int(np.argmax(spec)))
    assert bins == [82, 205], bins
    d["chain_bins"] = np.array(bins, np.int32)
    out = os.path.join(ROOT, "tests", "golden", "pfb.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

"""Write tests/golden/ddc.npz: the truth the down-converter's host twin (and through it the kernel) is held to.  NumPy and SciPy only;
DATA only.  Captures are not stored: tests/ddc_cases.py regenerates them from their seeds, `crc_<case>` pins their bytes.

    python tools/make_goldens_ddc.py

  rotor   for every word of ddc_cases.rotor_words() and every index of rotor_indices(): the phase (-w i) mod 2^64 as an exact Python
          integer, cos and sin of 2 pi phase / 2^64 in np.longdouble, stored as a float64 pair (hi, lo) with hi + lo the 80-bit value.
  cases   the capture mixed with that rotor (rounded to float64) in float64, then scipy.signal.decimate(z, D, ftype='fir',
          zero_phase=True), or lfilter(h, 1, z)[::D] for the lead = 0 cases; SciPy's taps beside them, and max |z| for the bound.
  chain   the seed of the two-station capture and the audio bins its tones land in (1 kHz -> 85, 2.5 kHz -> 213 of a 2048-sample
          spectrum at 24 kS/s), checked here with SciPy's decimate and a plain discriminator.
"""
import os
import sys

import numpy as np
import scipy
import scipy.signal as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ddc_cases as DC  # noqa: E402

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    sys.exit("np.longdouble has fewer than 64 bits of precision here: the rotor truth needs the 80-bit format")


def rotor_truth(word, indices):
    """cos, sin of -2 pi word i / 2^64 in long double, from exact integer phases read as signed."""
    p = [(-word * int(i)) % (1 << 64) for i in indices]
    p = [v - (1 << 64) if v >= (1 << 63) else v for v in p]
    x = np.array([LD(v) for v in p]) / LD(2) ** 64          # exact: 64-bit integers, a power of two
    a = (LD(8) * np.arctan(LD(1))) * x                        # 2 pi to 64 bits, not float64's
    return np.cos(a), np.sin(a)


def hi_lo(v):
    hi = v.astype(np.float64)
    return hi, (v - hi.astype(LD)).astype(np.float64)


def main():
    d = {"version": np.array(DC.VERSION), "scipy": np.array(scipy.__version__)}
    words, idx = DC.rotor_words(), DC.rotor_indices()
    d["rotor_words"] = np.array(words, np.uint64)
    d["rotor_indices"] = np.array(idx, np.int64)
    c = np.empty((len(words), len(idx)), LD)
    s = np.empty_like(c)
    for k, w in enumerate(words):
        c[k], s[k] = rotor_truth(w, idx)
    d["rotor_c_hi"], d["rotor_c_lo"] = hi_lo(c)
    d["rotor_s_hi"], d["rotor_s_lo"] = hi_lo(s)
    for D in DC.TAP_DECIMS:
        d[f"taps_{D}"] = ss.firwin(20 * D + 1, 1.0 / D)
    for name, D, n, zero_phase, fractions in DC.CASES:
        x = DC.case_capture(name)
        d[f"crc_{name}"] = np.array(DC.crc(x), np.uint32)
        h = ss.firwin(20 * D + 1, 1.0 / D)
        d[f"h_{name}"] = h
        ref, zmax, ws = [], [], []
        for f in fractions:
            w = DC.word_of(f)
            rc, rs = rotor_truth(w, range(n))
            z = x.astype(np.complex128) * (rc.astype(np.float64) + 1j * rs.astype(np.float64))
            y = ss.decimate(z, D, ftype="fir", zero_phase=True) if zero_phase else ss.lfilter(h, 1.0, z)[::D]
            assert len(y) == -(-n // D)
            ref.append(y)
            zmax.append(np.abs(z).max())
            ws.append(w)
        d[f"ref_{name}"] = np.array(ref, np.complex128)
        d[f"zmax_{name}"] = np.array(zmax, np.float64)
        d[f"words_{name}"] = np.array(ws, np.uint64)
    # the chain: which audio bin each station's tone lands in
    x = DC.chain_capture()
    d["chain_seed"] = np.array(DC.CHAIN_SEED)
    d["chain_crc"] = np.array(DC.crc(x), np.uint32)
    bins = []
    for off, _ in DC.CHAIN_STATIONS:
        w = DC.word_of(off / DC.CHAIN_FS)
        rc, rs = rotor_truth(w, range(DC.CHAIN_N))
        z = ss.decimate(x.astype(np.complex128) * (rc.astype(np.float64) + 1j * rs.astype(np.float64)), DC.CHAIN_D, ftype="fir", zero_phase=True)
        audio = np.angle(z[1:] * np.conj(z[:-1]))[::2][:2048]            # a plain discriminator at 48 kS/s, every second sample: 24 kS/s
        spec = np.abs(np.fft.rfft((audio - audio.mean()) * np.hanning(len(audio))))
        spec[:2] = 0
        bins.append(int(np.argmax(spec)))
    assert bins == [85, 213], bins
    d["chain_bins"] = np.array(bins, np.int32)
    out = os.path.join(ROOT, "tests", "golden", "ddc.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The first guess bracket of the compacting selects (pss_post.h: select_kth64_compact / select_kth32_compact, bracket_db), chosen on the CPU.

The select tries brackets [mean - d, mean + d] around the row's mean, in dB, narrowest first.  A bracket that holds rank k and at most
CAP = 64 CPL = 128 keys costs two sweeps over the row (one count, one compaction); more than CAP keys cost halving sweeps and a second compaction;
a bracket that misses rank k costs its two sweeps and the next rung.  For every half-width of the first rung and every row family this prints the
distribution of M (the keys of a 1020-point smoothed row inside the bracket), the share of rows with M > CAP, the share with ranks k and k + 1 inside,
and the mean number of full-row sweeps of the whole ladder (first rung, then +-0.5, then +-2, then select_kth64's plain search taken as 12 sweeps).
The hint is modelled twice: a float32 running sum of float32 roundings (sum32), and a float64 sum rounded once (sum64).

    python tools/bracket_ladder.py [rows per family = 16384] [half-widths = 0.2,0.25,0.3,0.35,0.4,0.5]

NumPy only; the rows are the float64 arithmetic of compute_fft (Hamming, FFT, fftshift, 10 log10(|X|^2 + 1e-10)) and the 5-tap mean."""
import sys

import numpy as np

N, M_ROW, CAP = 1024, 1020, 128
K1 = (M_ROW - 1) >> 1
LADDER_TAIL = (0.5, 2.0)       # the rungs behind the first (pss_post.h: bracket_db)
FALLBACK_SWEEPS = 12           # select_kth64 from the row's extremes (NOTEBOOK R6-14: 10.4-10.7 counting passes + the low-word sweeps)
FAMILIES = ("fm", "noise", "comb", "zero", "int8")


def synth(family, nf, seed, fs=2.4e6):
    """Rows of complex IQ: bench.synth_fm_iq's signal ("fm": three audio tones, 5 kHz deviation, A = 0.5, sigma = 0.02) and the other families."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / fs
    noise = lambda s: (s * (rng.standard_normal((nf, N)) + 1j * rng.standard_normal((nf, N))))
    if family in ("fm", "int8"):
        ph0 = 0.1 * np.arange(nf)[:, None]
        m = 0.5 * np.sin(2 * np.pi * 400 * t + ph0) + 0.3 * np.sin(2 * np.pi * 1000 * t + 2 * ph0) + 0.2 * np.sin(2 * np.pi * 2500 * t + 3 * ph0)
        x = 0.5 * np.exp(1j * (2 * np.pi * 5e3 * np.cumsum(m, axis=1) / fs + ph0)) + noise(0.02)
        if family == "int8":
            x = (np.clip(np.round(x.real * 127.5 - 0.5), -128, 127) + 0.5) / 127.5 + 1j * (np.clip(np.round(x.imag * 127.5 - 0.5), -128, 127) + 0.5) / 127.5
    elif family == "noise":
        x = noise(0.02)
    elif family == "comb":
        # a strong tone on every bin centre: the smoothed minimum stays above median - 10
        x = np.fft.ifft(np.exp(2j * np.pi * rng.random((nf, N))), axis=1) * 8 + noise(1e-4)
    elif family == "zero":
        x = np.zeros((nf, N), np.complex128)
    else:
        raise ValueError(family)
    return x.astype(np.complex64)


def smoothed_rows(iq):
    x = iq.astype(np.complex128) * np.hamming(N)
    X = np.fft.fftshift(np.fft.fft(x, axis=1), axes=1)
    a = np.abs(X)
    db = 10.0 * np.log10(a * a + 1e-10)
    acc = np.zeros((db.shape[0], M_ROW))
    for k in range(5):
        acc = acc + db[:, k:k + M_ROW] * 0.2
    return acc


def hi_word(v):
    """The high word of the order-preserving integer image of float64 values (pss_post.h: d2ord >> 32)."""
    u = np.ascontiguousarray(v, np.float64).view(np.uint64)
    neg = (u >> np.uint64(63)).astype(bool)
    o = np.where(neg, ~u, u | np.uint64(1 << 63))
    return (o >> np.uint64(32)).astype(np.int64)


def hint(sm, mode):
    if mode == "sum32":
        s = np.zeros(sm.shape[0], np.float32)
        for lane in range(0, M_ROW, 16):           # a lane's 16 values in order, then the lanes (the order of the additions is not the device's tree)
            part = np.zeros(sm.shape[0], np.float32)
            for r in range(min(16, M_ROW - lane)):
                part = part + sm[:, lane + r].astype(np.float32)
            s = s + part
        return s / np.float32(M_ROW)
    return sm.sum(axis=1).astype(np.float32) / np.float32(M_ROW)


def rung(kh_sorted, guess, d):
    """(n_lo, M) of one row for the bracket [guess - d, guess + d] on the high words."""
    g = np.float32(guess)
    lo, hi = (int(x) for x in hi_word(np.array([g - np.float32(d), g + np.float32(d)], np.float64)))
    n_lo = int(np.searchsorted(kh_sorted, lo, "left"))
    return n_lo, int(np.searchsorted(kh_sorted, hi, "right")) - n_lo, lo, hi


def sweeps_of_rung(kh_sorted, n_lo, M, lo, hi):
    """Full-row sweeps of a rung that holds rank k: the count and the compaction, and for M > CAP the halving counts and the second compaction
    (None: more than CAP keys share one high word, the select gives up)."""
    if M <= CAP:
        return 2
    n, n_hi = 2, n_lo + M
    while n_hi - n_lo > CAP and lo < hi:
        trial = lo + ((hi - lo + 1) >> 1)
        c = int(np.searchsorted(kh_sorted, trial, "left"))
        n += 1
        if c <= K1:
            lo, n_lo = trial, c
        else:
            hi, n_hi = trial - 1, c
    return None if n_hi - n_lo > CAP else n + 1


def table(sm, widths, mode):
    """One dict per half-width: the statistics of the first rung and the ladder's mean number of full-row sweeps."""
    guess = hint(sm, mode)
    kh = np.sort(hi_word(sm), axis=1)
    out = []
    for d in widths:
        Ms, over, in_k, in_k1, total = [], 0, 0, 0, 0
        for r in range(sm.shape[0]):
            row = kh[r]
            n_lo, M, lo, hi = rung(row, guess[r], d)
            Ms.append(M)
            over += M > CAP
            in_k += n_lo <= K1 < n_lo + M
            in_k1 += n_lo <= K1 and K1 + 1 < n_lo + M
            cost = 0
            for dd in (d,) + tuple(w for w in LADDER_TAIL if w > d):
                n_lo, M, lo, hi = rung(row, guess[r], dd)
                if n_lo <= K1 < n_lo + M:
                    s = sweeps_of_rung(row, n_lo, M, lo, hi)
                    cost += s if s is not None else 2 + FALLBACK_SWEEPS
                    break
                cost += 2
            else:
                cost += FALLBACK_SWEEPS
            total += cost
        Ms = np.array(Ms)
        n = float(sm.shape[0])
        out.append({"half_width": d, "M_mean": float(Ms.mean()), "M_p50": float(np.percentile(Ms, 50)), "M_p99": float(np.percentile(Ms, 99)),
                    "M_max": int(Ms.max()), "over_cap": over / n, "k_inside": in_k / n, "k_k1_inside": in_k1 / n, "sweeps": total / n})
    return out


COLUMNS = ("half_width", "M_mean", "M_p50", "M_p99", "M_max", "over_cap", "k_inside", "k_k1_inside", "sweeps")


def main():
    nf = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    widths = tuple(float(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else (0.2, 0.25, 0.3, 0.35, 0.4, 0.5)
    mean_sweeps = {d: [] for d in widths}
    for fi, fam in enumerate(FAMILIES):
        rows = nf if fam != "zero" else min(nf, 64)          # (every all-zero row is the same row)
        sm = np.concatenate([smoothed_rows(synth(fam, min(2048, rows - s), 1000 * fi + s)) for s in range(0, rows, 2048)])
        for mode in ("sum32", "sum64"):
            print(f"# family {fam}, {rows} rows, hint {mode}; CAP = {CAP}")
            print("  " + "  ".join(f"{c:>11s}" for c in COLUMNS))
            for rec in table(sm, widths, mode):
                print("  " + "  ".join(f"{rec[c]:11.4f}" if c != "M_max" else f"{rec[c]:11d}" for c in COLUMNS))
                if mode == "sum64":
                    mean_sweeps[rec["half_width"]].append(rec["sweeps"])
    print("# mean full-row sweeps over the families (hint sum64), per half-width of the first rung")
    for d in widths:
        print(f"  {d:6.3f}  {np.mean(mean_sweeps[d]):8.4f}   benchmark family alone: {mean_sweeps[d][0]:8.4f}")


if __name__ == "__main__":
    main()

"""The three-rung bracket ladder of the compacting selects (pss_post.h: bracket_db, select_kth64_compact, select_kth32_compact): crafted float64 and
float32 dB rows of 1024 points through the separate post-process entry points (pss_spectrum_post_f64, pss_spectrum_post_extremes) against NumPy
bit for bit — np.convolve's sums, np.median, the clamp, the finite extremes.

The rows are base + spread * noise with the spread swept so that the number M of candidates of each rung runs across CAP, plus rows built for the
ladder's other exits.  A host emulation of the ladder (the constants below mirror pss_post.h: bracket_db and PSS_POST_CPL) classifies every row,
and the test asserts that each class is present in what it sends to the device:
    M <= 64;  64 < M <= CAP;  every M from CAP - 2 to CAP + 2 (first rung, rank k inside);
    M > CAP at the first compaction and <= CAP after the halving sweeps (a bracket is only ever left for a WIDER one when rank k lies outside it,
    so "the second" is the same rung's second compaction);
    rank k outside rung 1 but inside rung 2;  outside rungs 1 and 2, inside rung 3;  outside all rungs;
    rank k the accepted bracket's last key (rank k + 1 above the bracket);  ties at the median;
    more than CAP keys sharing one high word (float32 rows: more than CAP equal keys);  NaN mean (and an infinite one).
The emulation's hint is the float32 mean summed in its own order: M of a row on the device may differ by a key at a bracket's edge.  That moves
single rows between neighbouring classes, which several rows each populate; every result is decided by exact counts either way."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M_ROW = 1024, 1020
K1 = (M_ROW - 1) >> 1
LADDER = (0.35, 0.5, 2.0)      # pss_post.h: bracket_db(0 .. 2)
CAP = 64 * 2                   # pss_post.h: 64 * PSS_POST_CPL


def smooth(rows):
    sm = rows[:, 0:M_ROW] * 0.2
    for j in range(1, 5):
        sm = sm + rows[:, j:j + M_ROW] * 0.2
    return sm


def keys(v):
    """What the select brackets: the high word of the ordered image of a float64, the whole ordered image of a float32."""
    if v.dtype == np.float32:
        u = v.view(np.uint32).astype(np.int64)
        return np.where(u >> 31, (~u) & 0xffffffff, u | 0x80000000)
    u = v.view(np.uint64)
    return (np.where((u >> np.uint64(63)).astype(bool), ~u, u | np.uint64(1 << 63)) >> np.uint64(32)).astype(np.int64)


def classify(sm):
    """The classes of one smoothed row (float64 or float32 values) under the ladder."""
    out = set()
    with np.errstate(invalid="ignore", over="ignore"):
        guess = np.float32(np.sum(sm.astype(np.float32), dtype=np.float32) / np.float32(M_ROW))
    if not np.isfinite(guess):
        return {"nan_mean" if np.isnan(guess) else "inf_mean"}
    ks = np.sort(keys(sm))
    srt = np.sort(sm)
    if srt[K1] == srt[K1 + 1]:
        out.add("ties")
    if np.count_nonzero(ks == ks[K1]) > CAP:
        out.add("shared")
    for rung, d in enumerate(LADDER):
        edge = np.array([guess - np.float32(d), guess + np.float32(d)], np.float32).astype(sm.dtype)
        lo, hi = (int(x) for x in keys(edge))
        n_lo = int(np.searchsorted(ks, lo, "left"))
        Mc = int(np.searchsorted(ks, hi, "right")) - n_lo
        if not (n_lo <= K1 < n_lo + Mc):
            continue
        out.add(f"rung{rung + 1}")
        if rung == 0:
            out.add("M<=64" if Mc <= 64 else "64<M<=CAP" if Mc <= CAP else "M>CAP")
            if abs(Mc - CAP) <= 2:
                out.add(f"M={Mc}")
        n_hi = n_lo + Mc
        while n_hi - n_lo > CAP and lo < hi:             # the halving sweeps
            trial = lo + ((hi - lo + 1) >> 1)
            c = int(np.searchsorted(ks, trial, "left"))
            if c <= K1:
                lo, n_lo = trial, c
            else:
                hi, n_hi = trial - 1, c
        if Mc > CAP and n_hi - n_lo <= CAP:
            out.add("halved")
        if n_hi - n_lo <= CAP and K1 + 1 == n_hi:
            out.add("last_key")
        return out
    out.add("outside_all")
    return out


NEEDED = ["M<=64", "64<M<=CAP", "M>CAP", "halved"] + [f"M={v}" for v in range(CAP - 2, CAP + 3)] + \
         ["rung2", "rung3", "outside_all", "last_key", "ties", "shared", "nan_mean", "inf_mean"]


def crafted(dtype):
    """<= 512 rows of `dtype` and their classes: a fixed pool of candidates, of which the rows that populate a class not yet full are kept."""
    rng = np.random.default_rng(2024)
    pool = []
    for spread in np.concatenate([np.linspace(3.0, 9.0, 700), np.linspace(12.0, 40.0, 60), np.linspace(0.2, 2.5, 40)]):
        pool.append(-50.0 + spread * rng.standard_normal(N))
    for frac, lift in ((0.01, 30.0), (0.02, 25.0), (0.03, 20.0), (0.05, 30.0), (0.1, 40.0), (0.2, 60.0), (0.3, 80.0)):   # a mean off the median
        for spread in (3.0, 5.0, 8.0):
            r = -50.0 + spread * rng.standard_normal(N)
            r[rng.random(N) < frac] += lift
            pool.append(r)
    for run in range(10, 60):           # two levels and a run of low values that pulls the mean: rank k ends as a bracket's last key
        r = np.where(np.arange(N) < 512, -50.0, -48.0) + 1e-3 * rng.standard_normal(N)
        r[40:40 + run] = -60.0
        pool.append(r)
    for _ in range(6):                  # runs of equal values: exact ties among the smoothed values
        pool.append(np.repeat(rng.integers(-52, -47, N // 8).astype(np.float64), 8))
    for _ in range(4):                  # values that differ in the low words of their float64 keys only (float32: equal)
        pool.append(-50.0 + 1e-7 * rng.standard_normal(N))
    r = -50.0 + 5.0 * rng.standard_normal(N); r[300] = np.nan; pool.append(r)
    r = -50.0 + 5.0 * rng.standard_normal(N); r[17] = np.inf; pool.append(r)
    pool = np.array(pool).astype(dtype)
    with np.errstate(invalid="ignore"):
        sm = smooth(pool.astype(np.float64)).astype(dtype)
    have, keep, classes = {c: 0 for c in NEEDED}, [], []
    for i in range(len(pool)):
        cl = classify(sm[i])
        if any(have[c] < 24 for c in cl if c in have):
            keep.append(i)
            classes.append(cl)
            for c in cl:
                if c in have:
                    have[c] += 1
    assert len(keep) <= 512
    return pool[keep], classes, have


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ladder_classes_against_numpy(dtype):
    import torch
    import gpu_util as G
    rows, classes, have = crafted(dtype)
    missing = [c for c in NEEDED if have[c] == 0]
    assert not missing, f"classes without a row: {missing}"
    nf = rows.shape[0]
    e = G.engine()
    tt = torch.float64 if dtype == np.float64 else torch.float32
    d_p, d_lo, d_hi = G.empty((nf, M_ROW), tt), G.empty((nf,), tt), G.empty((nf,), tt)
    if dtype == np.float64:
        e.spectrum_post_f64(G.dev(rows), nf, N, d_p, d_lo, d_hi)
    else:
        e.spectrum_post_extremes(G.dev(rows), nf, N, d_p, d_lo, d_hi)
    e.sync()
    post, lo, hi = G.host(d_p), G.host(d_lo), G.host(d_hi)
    with np.errstate(invalid="ignore"):
        sm = smooth(rows.astype(np.float64)).astype(dtype)          # float32 rows: the float64 sum rounded once
        for k in range(nf):
            med = np.median(sm[k].astype(np.float64))
            thr = dtype(med - 10.0)
            want = sm[k].copy()
            want[want < thr] = thr
            assert np.array_equal(post[k].view(np.uint8), want.view(np.uint8)) or np.array_equal(post[k], want, equal_nan=True), (k, sorted(classes[k]))
            fin = want[np.isfinite(want)]
            assert lo[k] == fin.min() and hi[k] == fin.max(), (k, sorted(classes[k]))

#!/usr/bin/env python3
"""The band-plan channeliser (pss_bank, k_bank) on captures resident on the device, in one process (profiles/bank.txt).

    python tools/bench_bank.py [repeats] > profiles/bank.txt
    python tools/bench_bank.py counters       # two short launches of k_bank and of k_pfb per shape and nothing else: the program a counter collection runs

Two captures: the cfg 5 capture (99 999 744 samples at 10 MS/s) with M = 800 at D = 200 and D = 400 and M = 400 at D = 200 (12.5 and
25 kHz grids), and 24 000 000 samples at 2.4 MS/s with M = 192 at D = 48 and M = 96 at D = 48.  Per shape, alternating, host clock
around call + synchronise, min - max (median) of `repeats` regions (default 5) after one warm-up round of every route:
  - pss_bank, all M rows, default taps (20 M + 1);
  - the bar's pair with ONE tap table pss_ddc can take (the default where it has at most 4097 taps, else firwin(4097, 1 / M)):
    pss_bank for all M rows against pss_ddc (unchanged) for ceil(M / 8) of the bank's own centres in one call.  The bar, the project's
    own from the pss_pfb work: the bank is the faster of the two;
  - pss_pfb (unchanged) at the next power of two M' above M with 20 M' + 1 taps and the same output rate ratio D' / M' = D / M.
Every route is handed its tap table ready made: no filter design runs inside a timed region.
Then the kernels from the context's per-kernel events, again `repeats` alternating launches a route, and from THOSE (the median of each)
the time per (output instant x channel) of k_bank beside k_pfb's: no bar is set for that ratio; the idle threads (1024 / W) and the 3- and
5-point kernels' operations are printed beside it, and whether the ratio stays inside what the two explain.  The same ratio from the host
clock's medians is printed on a line of its own, named as such.  Last, 16 instants of all rows against the host twin.  A record; bench.py
and its line are not touched by any of this.
"""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

DDC_MAX_TAPS = 4097
SHAPES = [("cfg 5 capture", 99_999_744, 10e6, 800, 200), ("cfg 5 capture", 99_999_744, 10e6, 800, 400), ("cfg 5 capture", 99_999_744, 10e6, 400, 200),
          ("2.4 MS/s capture", 24_000_000, 2.4e6, 192, 48), ("2.4 MS/s capture", 24_000_000, 2.4e6, 96, 48)]


def capture(n):
    rng = np.random.default_rng(51)
    block = (0.5 * (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20))).astype(np.complex64)
    return torch.from_numpy(block.view(np.float32)).cuda().repeat((n + (1 << 20) - 1) >> 20)[:2 * n].contiguous()


def firwin(e, numtaps, cutoff):
    h = np.empty(numtaps, np.float64)
    assert e.lib.pss_design_firwin(numtaps, float(cutoff), h.ctypes.data) == 0
    return h


def factors(M):
    e = []
    for p in (2, 3, 5):
        k = 0
        while M % p == 0:
            M //= p
            k += 1
        e.append(k)
    return e


def dft_ops(M):
    """float64 operations (a fma counted as one) of one M-point DFT as csrc/pss_bank.h writes it: a twiddle is 4, the radix-2 sum and
    difference 4, the 3-point kernel 12, the 5-point kernel 36."""
    n2, n3, n5 = factors(M)
    return n2 * (M // 2) * (4 + 4) + n3 * (M // 3) * (2 * 4 + 12) + n5 * (M // 5) * (4 * 4 + 36)


def shape(e, name, d_iq, n, fs, M, D, rep):
    taps = Engine.bank_default_taps(M)
    T = len(taps)
    short = taps if T <= DDC_MAX_TAPS else firwin(e, DDC_MAX_TAPS, 1.0 / M)      # what pss_ddc can take
    n_out = e.lib.pss_ddc_out_len(n, D)
    K = -(-M // 8)
    rows = np.arange(K) * (M // K)                                                # centres of the bank's grid, spread over it
    words = np.array([((int(c) << 64) + M // 2) // M for c in rows], np.uint64)
    M2 = 1 << M.bit_length()                                                      # the next power of two above M
    taps2 = Engine.pfb_default_taps(M2)
    D2 = M2 * D // M
    assert D2 * M == M2 * D
    n_out2 = e.lib.pss_ddc_out_len(n, D2)
    d_out = torch.empty((max(M, M2), 2 * max(n_out, n_out2)), dtype=torch.float32, device="cuda")
    d_dd = torch.empty((K, 2 * n_out), dtype=torch.float32, device="cuda")

    def bank(h=taps):
        e.bank(d_iq, n, M, D, d_out, taps=h, out_stride=n_out)

    def ddc():
        e.ddc(d_iq, n, words, D, d_dd, taps=short, out_stride=n_out)

    def pfb():
        e.pfb(d_iq, n, M2, D2, d_out, taps=taps2, out_stride=n_out2)

    l_bank, l_bar, l_ddc, l_pfb = (f"pss_bank, all {M} rows, {T} taps", f"pss_bank, all {M} rows, {len(short)} taps (the bar's table)",
                                   f"pss_ddc K = {K}, {len(short)} taps", f"pss_pfb, all {M2} rows at D = {D2}, {len(taps2)} taps")
    routes = [(l_bank, bank), (l_bar, lambda: bank(short)), (l_ddc, ddc), (l_pfb, pfb)]
    W = M * (1024 // M)
    print(f"\n{name}: {n} samples ({n * 8 / 1e6:.0f} MB) at {fs / 1e6} MS/s, M = {M} (spacing {fs / M / 1e3:g} kHz), D = {D} -> {M} rows at {fs / D / 1e3:g} kS/s, "
          f"{n_out} instants ({M * n_out * 8 / 1e6:.0f} MB out); W = {W} of 1024 threads, {8 * (1024 // M)} instants a tile")
    for _, fn in routes:
        timed(e, fn)
    t = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    for k, (label, _) in enumerate(routes):
        print(f"    {label.ljust(58)} {stats(t[k])}")
    kt = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            kt[k].append(kernels(e, fn))
    kmed = {}
    for (label, _), v in zip(routes, kt):
        assert all(len(d) == 1 and set(d) == set(v[0]) for d in v), "one kernel a launch"
        name = next(iter(v[0]))
        kmed[label] = statistics.median(d[name] for d in v)
        print(f"    kernel events, {label}: {name} {stats([d[name] for d in v])}")
    med = {label: statistics.median(v) for (label, _), v in zip(routes, t)}
    print(f"    the bar (host clock): pss_bank for {M} rows {med[l_bar]:.3f} ms against pss_ddc for K = {K} {med[l_ddc]:.3f} ms, both with {len(short)} taps: "
          f"ratio {med[l_bar] / med[l_ddc]:.4f} -> {'met' if med[l_bar] < med[l_ddc] else 'MISSED'}")
    per_bank, per_pfb = kmed[l_bank] * 1e6 / (M * n_out), kmed[l_pfb] * 1e6 / (M2 * n_out2)
    ops_bank, ops_pfb = 2 * T + dft_ops(M), 2 * len(taps2) + dft_ops(M2)
    explained = 1024 / W * (ops_bank / M) / (ops_pfb / M2)
    print(f"    per (instant x channel), kernel events: k_bank {per_bank:.5f} ns, k_pfb at M' = {M2} {per_pfb:.5f} ns: ratio {per_bank / per_pfb:.3f}; idle "
          f"threads 1024 / W = {1024 / W:.3f}; float64 operations an instant and channel {ops_bank / M:.1f} against {ops_pfb / M2:.1f}: ratio "
          f"{(ops_bank / M) / (ops_pfb / M2):.3f}; the two together {explained:.3f} -> "
          f"{'inside what the two explain' if per_bank / per_pfb <= explained else 'ABOVE what the two explain: a counter run is due'}")
    print(f"    per (instant x channel), host clock around call + synchronise: pss_bank {med[l_bank] * 1e6 / (M * n_out):.5f} ns, pss_pfb "
          f"{med[l_pfb] * 1e6 / (M2 * n_out2):.5f} ns: ratio {med[l_bank] * n_out2 * M2 / (med[l_pfb] * n_out * M):.3f}")
    bank()
    e.sync()
    m0 = n_out // 2
    lo, hi = m0 * D - T, (m0 + 16) * D + T
    want = Engine.h_bank(d_iq[2 * lo:2 * hi].cpu().numpy().view(np.complex64), M, D, taps=taps, buf_index0=lo, n_capture=n, m_begin=m0, m_end=m0 + 16)
    got = d_out.view(-1)[:M * 2 * n_out].view(M, 2 * n_out)[:, 2 * m0:2 * (m0 + 16)].cpu().numpy().view(np.complex64)
    assert np.array_equal(got, want), "the device's outputs are not the host twin's"
    print("    16 instants of all rows from the middle of the capture equal the host twin bit for bit")


def counters():
    """Two launches of k_bank per shape on short captures and two of k_pfb (unchanged) at the next power of two with the same D / M, nothing
    else on the device: what a hardware-counter collection runs (profiles/bank_counters.txt)."""
    e = Engine(0, order="none")
    for n, M, D in ((8_000_000, 800, 200), (8_000_000, 400, 200), (4_000_000, 192, 48), (4_000_000, 96, 48)):
        d_iq = capture(n)
        M2 = 1 << M.bit_length()
        D2 = M2 * D // M
        taps, taps2 = Engine.bank_default_taps(M), Engine.pfb_default_taps(M2)
        n_out, n_out2 = e.lib.pss_ddc_out_len(n, D), e.lib.pss_ddc_out_len(n, D2)
        d_out = torch.empty((max(M, M2), 2 * max(n_out, n_out2)), dtype=torch.float32, device="cuda")
        for _ in range(2):
            e.bank(d_iq, n, M, D, d_out, taps=taps, out_stride=n_out)
        for _ in range(2):
            e.pfb(d_iq, n, M2, D2, d_out, taps=taps2, out_stride=n_out2)
        e.sync()
        print(f"k_bank x 2: {n} samples, M = {M}, D = {D}, {len(taps)} taps, {n_out} instants, {-(-n_out // (8 * (1024 // M)))} tiles;  "
              f"k_pfb x 2: M' = {M2}, D' = {D2}, {len(taps2)} taps, {n_out2} instants, {-(-n_out2 // (8192 // M2))} tiles")
    e.close()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    if len(sys.argv) > 1 and sys.argv[1] == "counters":
        return counters()
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"band-plan channeliser; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    d_iq, held = None, None
    for name, n, fs, M, D in SHAPES:
        if held != n:
            del d_iq
            d_iq, held = capture(n), n
        shape(e, name, d_iq, n, fs, M, D, rep)
    e.close()


if __name__ == "__main__":
    main()

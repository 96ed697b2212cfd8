#!/usr/bin/env python3
"""The polyphase channeliser (pss_pfb, k_pfb) on captures resident on the device, in one process (profiles/pfb.txt).

    python tools/bench_pfb.py [repeats] > profiles/pfb.txt
    python tools/bench_pfb.py counters        # two short launches of k_pfb and nothing else: the program a counter collection runs

Two captures: the cfg 5 capture (99 999 744 samples at 10 MS/s) with M = 256 at D = 256 and D = 128, and 24 000 000 samples at 2.4 MS/s
with M = 64 at D = 64 and D = 32, default taps (20 M + 1).  Beside each: a device-to-device copy of the capture's bytes, pss_ddc
(unchanged) on K = 1, 16 and M / 8 of the bank's own channel centres at the same D, and the user path pfb + demod_signal(NFM) of all
rows.  pss_ddc takes at most 4097 taps, so where the bank's table is longer (M = 256: 5121) pss_ddc runs firwin(4097, 1 / M) and the
bank is timed with that table too.  Host clock around call + synchronise, the routes alternating, min - max (median) of `repeats`
regions (default 5) after one warm-up round of every route; then the kernels from the context's per-kernel events.  The count-based
floors are computed here from the shapes.  The bar: pss_pfb for all M rows in less time than pss_ddc for M / 8 of them.  A record;
bench.py and its line are not touched by any of this.
"""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

CUS, CLOCK, HBM = 256, 2.4e9, 8e12   # MI355X: compute units, shader clock and memory rate the floors are stated at
FRAME = 4096                         # read-buffer length of the rows' NFM step
DDC_MAX_TAPS = 4097


def capture(n):
    rng = np.random.default_rng(51)
    block = (0.5 * (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20))).astype(np.complex64)
    return torch.from_numpy(block.view(np.float32)).cuda().repeat((n + (1 << 20) - 1) >> 20)[:2 * n].contiguous()


def firwin(e, numtaps, cutoff):
    h = np.empty(numtaps, np.float64)
    assert e.lib.pss_design_firwin(numtaps, float(cutoff), h.ctypes.data) == 0
    return h


def shape(e, name, d_iq, n, fs, M, D, rep):
    d_copy = torch.empty_like(d_iq)
    taps = Engine.pfb_default_taps(M)
    T = len(taps)
    short = taps if T <= DDC_MAX_TAPS else firwin(e, DDC_MAX_TAPS, 1.0 / M)      # what pss_ddc can take
    n_out = e.lib.pss_ddc_out_len(n, D)
    m_end = n_out // FRAME * FRAME                     # whole read buffers for the NFM step
    fs2 = fs / D
    KS = sorted({1, 16, M // 8})
    words = np.array([c * ((1 << 64) // M) for c in range(M)], np.uint64)[np.arange(max(KS)) * (M // max(KS))]   # centres of the bank's grid, spread over it
    d_out = torch.empty((M, 2 * n_out), dtype=torch.float32, device="cuda")
    d_dd = torch.empty((max(KS), 2 * n_out), dtype=torch.float32, device="cuda")
    nf = M * (m_end // FRAME)
    d_pcm = torch.empty((nf, e.demod_out_len(L.MODE_NFM, FRAME, fs2), 2), dtype=torch.int16, device="cuda")

    def pfb(h=taps, end=n_out, stride=n_out):
        e.pfb(d_iq, n, M, D, d_out, taps=h, m_end=end, out_stride=stride)

    def ddc(k):
        e.ddc(d_iq, n, words[:k], D, d_dd, taps=short, out_stride=n_out)

    def chain():
        pfb(end=m_end, stride=m_end)
        e.demod_signal(L.MODE_NFM, d_out, nf, FRAME, fs2, d_pcm)

    routes = [("device-to-device copy of the capture  ", lambda: d_copy.copy_(d_iq)),
              (f"pss_pfb, all {M} rows, {T} taps".ljust(38), pfb)]
    if short is not taps:
        routes.append((f"pss_pfb, all {M} rows, {len(short)} taps".ljust(38), lambda: pfb(short)))
    routes += [(f"pss_ddc K = {k}, {len(short)} taps".ljust(38), (lambda k: lambda: ddc(k))(k)) for k in KS]
    routes.append((f"pss_pfb + demod_signal NFM, {M} rows".ljust(38), chain))
    print(f"\n{name}: {n} samples ({n * 8 / 1e6:.0f} MB) at {fs / 1e6} MS/s, M = {M}, D = {D} -> {M} rows at {fs2 / 1e3:g} kS/s, {T} taps, {n_out} instants "
          f"({M * n_out * 8 / 1e6:.0f} MB out)")
    lb = M.bit_length() - 1
    steps, flies = n_out * T, n_out * (M // 2) * lb
    wave_op = 4 / (64 * 4 * CUS * CLOCK) * 1e3          # a wave64 float64 operation issues in 4 clocks on each of a CU's 4 SIMDs
    print(f"    floors: {steps:.3e} tap steps, 2 float64 fma each: {steps * 2 * wave_op:.3f} ms; {flies:.3e} butterflies, 8 float64 operations each: "
          f"{flies * 8 * wave_op:.3f} ms")
    print(f"            vector cache: 16 B a tap step (sample and tap) at 64 B / clk / CU: {steps * 16 / (64 * CUS * CLOCK) * 1e3:.3f} ms; "
          f"LDS: 64 B a butterfly and 64 B an output at 256 B / clk / CU: {(flies * 64 + M * n_out * 64) / (256 * CUS * CLOCK) * 1e3:.3f} ms")
    print(f"            HBM: {n * 8 / 1e9:.2f} GB in, {M * n_out * 8 / 1e9:.2f} GB out at {HBM / 1e12:g} TB/s: {(n * 8 + M * n_out * 8) / HBM * 1e3:.3f} ms")
    for _, fn in routes:
        timed(e, fn)
    t = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    for k, (label, fn) in enumerate(routes):
        print(f"    {label} {stats(t[k])}")
    for label, fn in routes[1:]:
        print(f"    kernels of {label.strip()}: " + "  ".join(f"{k}={v:.3f}" for k, v in kernels(e, fn).items()) + " ms")
    med = {label.strip(): statistics.median(v) for (label, _), v in zip(routes, t)}
    bank = med[f"pss_pfb, all {M} rows, {len(short)} taps"]
    bar = med[f"pss_ddc K = {M // 8}, {len(short)} taps"]
    print(f"    the bar: pss_pfb for {M} rows {bank:.3f} ms against pss_ddc for K = {M // 8} {bar:.3f} ms, both with {len(short)} taps: ratio {bank / bar:.3f} "
          f"-> {'met' if bank < bar else 'MISSED'}; a row costs {bank / M * 1e3:.1f} us in the bank and {med[f'pss_ddc K = 16, {len(short)} taps'] / 16 * 1e3:.1f} us "
          "in the 16-channel down-converter")
    pfb()
    e.sync()
    m0 = n_out // 2
    lo, hi = m0 * D - T, (m0 + 16) * D + T
    want = Engine.h_pfb(d_iq[2 * lo:2 * hi].cpu().numpy().view(np.complex64), M, D, taps=taps, buf_index0=lo, n_capture=n, m_begin=m0, m_end=m0 + 16)
    got = d_out[:, 2 * m0:2 * (m0 + 16)].cpu().numpy().view(np.complex64)
    assert np.array_equal(got, want), "the device's outputs are not the host twin's"
    print("    16 instants of all rows from the middle of the capture equal the host twin bit for bit")


def counters():
    """Two launches of k_pfb per shape on short captures, nothing else on the device: what a hardware-counter collection runs."""
    e = Engine(0, order="none")
    for n, M, D in ((8_000_000, 256, 256), (8_000_000, 256, 128), (4_000_000, 64, 32)):
        d_iq = capture(n)
        n_out = e.lib.pss_ddc_out_len(n, D)
        d_out = torch.empty((M, 2 * n_out), dtype=torch.float32, device="cuda")
        for _ in range(2):
            e.pfb(d_iq, n, M, D, d_out)
        e.sync()
        print(f"k_pfb x 2: {n} samples, M = {M}, D = {D}, {20 * M + 1} taps, {n_out} instants, {-(-n_out // (8192 // M))} tiles")
    e.close()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    if len(sys.argv) > 1 and sys.argv[1] == "counters":
        return counters()
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"polyphase channeliser; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating; floors at {CUS} CUs, {CLOCK / 1e9} GHz")
    d_iq = capture(99_999_744)
    shape(e, "cfg 5 capture", d_iq, 99_999_744, 10e6, 256, 256, rep)
    shape(e, "cfg 5 capture", d_iq, 99_999_744, 10e6, 256, 128, rep)
    del d_iq
    d_iq = capture(24_000_000)
    shape(e, "2.4 MS/s capture", d_iq, 24_000_000, 2.4e6, 64, 64, rep)
    shape(e, "2.4 MS/s capture", d_iq, 24_000_000, 2.4e6, 64, 32, rep)
    e.close()


if __name__ == "__main__":
    main()

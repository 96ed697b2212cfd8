#!/usr/bin/env python3
"""Times of the squelch path next to the calls it is built beside, in one process (profiles/squelch_step.txt).

    python tools/bench_squelch.py [n_frames] [repeats]

(a) pss_frame_pipeline_squelch with every frame open against pss_frame_pipeline_cells, (b) the same with the squelch at the median of the
batch's peaks — host clock around call + synchronise, the two calls alternating, median and range of `repeats` timed regions after two
warm-up rounds; (c) the demodulator kernels of pss_demod_gated with k of n frames open (sum of the per-kernel events, the gather listed
separately) against pss_demod_signal on a batch of the same k frames; (d) the row meter alone, in GB/s of rows read.  1024-point NFM frames
whose amplitude varies from frame to frame.  bench.py and its line are not touched by any of this.
"""
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

NF = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 7
N, FS, W = 1024, 2.4e6, 112


def clocks():
    out = []
    for p in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))[:1]:
        try:
            out += [ln.strip() for ln in open(p) if "*" in ln]
        except OSError:
            pass
    return ", ".join(out) or "not readable"


def frames(nf, n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    k = torch.arange(nf, device="cuda", dtype=torch.float64)[:, None]
    ph = 2 * np.pi * (0.01 + 0.0001 * (k % 97)) * t + 3.0 * torch.sin(2 * np.pi * t * (0.002 + 1e-5 * (k % 31)))
    amp = 0.05 + 0.9 * torch.rand((nf, 1), generator=gen, device="cuda", dtype=torch.float64)
    iq = torch.stack([amp * torch.cos(ph), amp * torch.sin(ph)], dim=-1).float()
    return (iq + 0.02 * torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32)).contiguous()


def timed(fn, e):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f}, {len(v)} regions)"


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    e = Engine(0, order="none")
    iq = frames(NF, N, 2025)
    n_out = e.demod_out_len(L.MODE_NFM, N, FS)
    emp = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    db32, lo, hi = emp((NF, N), torch.float32), emp(NF, torch.float64), emp(NF, torch.float64)
    a, b, pcm = emp((NF, W), torch.int8), emp((NF, W), torch.int8), emp((NF, n_out, 2), torch.int16)
    peak, avg, opened = emp(NF, torch.float64), emp(NF, torch.float64), emp(NF, torch.uint8)
    torch.cuda.synchronize()
    print(f"squelch step: {NF} x {N} NFM frames, fs {FS:g}; device {torch.cuda.get_device_name(0)}; shader clock at start: {clocks()}")

    cells = lambda: e.frame_pipeline_cells(L.MODE_NFM, iq, NF, N, FS, db32, None, lo, hi, W, a, b, pcm)
    count = [0]

    def squelch(level):
        def run():
            count[0], _ = e.frame_pipeline_squelch(L.MODE_NFM, iq, NF, N, FS, db32, None, lo, hi, W, a, b, pcm, level, peak, avg, opened)
        return run

    squelch(-1e9)()
    e.sync()
    median = float(torch.median(peak).item())
    for name, level in (("(a) every frame open", -1e9), (f"(b) squelch at the median peak {median:.2f} dB", median)):
        run = squelch(level)
        for _ in range(2):
            cells(); run()
        e.sync()
        tc, ts = [], []
        for _ in range(REP):
            tc.append(timed(cells, e))
            ts.append(timed(run, e))
        print(f"{name}: {count[0]} of {NF} open")
        print(f"    pss_frame_pipeline_cells    {stats(tc)}")
        print(f"    pss_frame_pipeline_squelch  {stats(ts)}")
        e.enable_timing(True)
        e.kernel_times()
        run()
        e.sync()
        kt = e.kernel_times()
        e.enable_timing(False)
        print("    kernels of one squelch step: " + "  ".join(f"{k}={sum(v):.4f}" for k, v in kt.items()) + " ms")

    # (c) the demodulator with k of n frames open against pss_demod_signal on a k-frame batch
    idx = torch.nonzero(opened).flatten().to(torch.int32)
    k = int(idx.numel())
    sub = iq[idx.long()].contiguous()
    pcm_k = emp((max(k, 1), n_out, 2), torch.int16)
    torch.cuda.synchronize()
    e.enable_timing(True)
    gated, gather, plain = [], [], []
    for r in range(2 + 5):
        e.kernel_times()
        e.demod_gated(L.MODE_NFM, iq, NF, N, FS, idx, k, pcm, None)
        e.sync()
        kt = e.kernel_times()
        e.demod_signal(L.MODE_NFM, sub, k, N, FS, pcm_k, None)
        e.sync()
        kp = e.kernel_times()
        if r >= 2:
            gather.append(sum(kt.get("k_gather_frames", [0.0])))
            gated.append(sum(sum(v) for kk, v in kt.items() if kk != "k_gather_frames"))
            plain.append(sum(sum(v) for v in kp.values()))
    e.enable_timing(False)
    assert torch.equal(pcm[:k], pcm_k[:k])
    print(f"(c) demodulator kernels, {k} of {NF} frames open (per-kernel events, 5 repeats):")
    print(f"    pss_demod_gated, demodulator kernels  {stats(gated)}")
    print(f"    pss_demod_gated, k_gather_frames      {stats(gather)}   ({2 * k * N * 8 / statistics.median(gather) / 1e6:.0f} GB/s read + written)")
    print(f"    pss_demod_signal on the k-frame batch {stats(plain)}")

    # (d) the row meter alone
    for rows, ln in ((NF, N - 4), (max(1, NF // 8), 8188), (max(1, NF // 32), 32764)):
        x = torch.randn((rows, ln), device="cuda", dtype=torch.float64) * 6.0 - 40.0
        pk, av = emp(rows, torch.float64), emp(rows, torch.float64)
        torch.cuda.synchronize()
        for _ in range(2):
            e.row_meter(x, rows, ln, pk, av)
        e.sync()
        e.enable_timing(True)
        e.kernel_times()
        for _ in range(REP):
            e.row_meter(x, rows, ln, pk, av)
        e.sync()
        v = e.kernel_times()["k_row_meter"]
        e.enable_timing(False)
        print(f"(d) pss_row_meter_f64 {rows} x {ln}: {stats(v)}, {rows * ln * 8 / statistics.median(v) / 1e6:.0f} GB/s of rows read")
        del x
    print(f"shader clock at end: {clocks()}")
    e.close()


if __name__ == "__main__":
    main()

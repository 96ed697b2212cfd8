#!/usr/bin/env python3
"""A complete scanner sweep, two ways, in one process (profiles/sweep_report.txt).

    python tools/bench_sweep.py [repeats] > profiles/sweep_report.txt

(a) what a caller does without the sweep report: the scan and pss_classify of EVERY slice; (b) pss_sweep_report: scan -> gate -> classifier on
the detections.  Host clock around call + synchronise, the two alternating, min - max (median) of `repeats` timed regions after two warm-up
rounds.  Shapes: BASELINE's cfg 4 sweep (8192 slices x 4096 points at 2.4 MS/s, tools/bench_configs.synth("scan"): a wide carrier in 1 slice
of 8) through the inline kind, and 64 driver reads of 240 000 samples through the driver kind.  Hit rates of about 1/8, 1/2 and 1 are set
with the two limits of the gate: the threshold at a quantile of the scan's peaks, min_bw at 50 kHz (the reference's) or below every
bandwidth.  Then the kernels of one call of each, from per-kernel events.  bench.py and its line are not touched by any of this.
"""
import glob
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import torch

import bench_configs
from pyspecsdr_amd.engine import Engine

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 5
FS = 2.4e6


def clocks():
    out = []
    for p in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))[:1]:
        try:
            out += [ln.strip() for ln in open(p) if "*" in ln]
        except OSError:
            pass
    return ", ".join(out) or "not readable"


def timed(fn, e):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return f"{min(v):.3f} - {max(v):.3f} ms (median {statistics.median(v):.3f}, {len(v)} regions)"


def kernels(e, fn):
    e.enable_timing(True)
    e.kernel_times()
    fn()
    e.sync()
    kt = e.kernel_times()
    e.enable_timing(False)
    return "  ".join(f"{k}={sum(v):.4f}" for k, v in kt.items()) + " ms"


def shape(e, kind, ns, n, seed):
    iq = bench_configs.synth("scan", ns, n, FS, "cuda:0", seed)
    emp = lambda s, dt: torch.empty(s, dtype=dt, device="cuda")
    peak, bw, count, idx = emp(ns, torch.float32), emp(ns, torch.float64), emp(ns, torch.int32), emp(ns, torch.int32)
    lab, cbw, mi, flat = emp(ns, torch.int32), emp(ns, torch.float64), emp(ns, torch.float32), emp(ns, torch.float32)
    lab2 = emp(ns, torch.int32)
    print(f"\n{kind} sweep: {ns} slices x {n} samples ({ns * n * 8 / 1e6:.0f} MB of IQ)")

    def scan(thr):
        if kind == "inline":
            e.scan(iq, ns, n, FS, None, peak, bw, count)
        else:
            e.scan_threshold(iq, ns, n, FS, thr, None, peak, bw, count)

    scan(0.0)
    e.sync()
    pk = np.sort(peak.cpu().numpy().astype(np.float64))
    below = float(pk[0]) - 1.0
    cases = [("1/8", float(pk[(7 * ns) // 8 - 1]) if kind == "driver" else below, 50e3 if kind == "inline" else -1.0),
             ("1/2", float(pk[ns // 2 - 1]), -1.0), ("1", below, -1.0)]
    for name, thr, min_bw in cases:
        hits = [0]

        def every():
            scan(thr)
            e.classify(iq, ns, n, FS, lab2, cbw, mi, flat)

        def report():
            hits[0] = e.sweep_report(kind, iq, ns, n, FS, thr, peak, bw, idx, min_bw, d_count=count, d_label=lab, d_cls_bw=cbw, d_mi=mi, d_flat=flat)

        for _ in range(2):
            every(); report()
        e.sync()
        ta, tb = [], []
        for _ in range(REP):
            ta.append(timed(every, e))
            tb.append(timed(report, e))
        k = hits[0]
        assert torch.equal(lab[:k], lab2[idx[:k].long()]), "the detections' labels are pss_classify's"
        print(f"hit rate about {name}: threshold {thr:.2f} dB, min_bw {min_bw:g} Hz -> {k} of {ns} slices")
        print(f"    (a) scan + pss_classify of every slice  {stats(ta)}")
        print(f"    (b) pss_sweep_report                    {stats(tb)}")
        print(f"    kernels of (a): {kernels(e, every)}")
        print(f"    kernels of (b): {kernels(e, report)}")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    e = Engine(0, order="none")
    print(f"scanner sweep report; device {torch.cuda.get_device_name(0)}; shader clock at start: {clocks()}")
    shape(e, "inline", 8192, 4096, 20260928 + 4)
    shape(e, "driver", 64, 240000, 20260928 + 14)
    print(f"\nshader clock at end: {clocks()}")
    e.close()


if __name__ == "__main__":
    main()

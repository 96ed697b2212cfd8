#!/usr/bin/env python3
"""The capture survey (pss_welch: k_welch + k_welch_fold) on captures resident on the device, in one process (profiles/welch.txt).

    python tools/bench_welch.py [repeats] > profiles/welch.txt
    python tools/bench_welch.py counters       # two calls of the bar's shape and nothing else: the program a counter collection runs

Per shape, alternating, host clock around call + synchronise, min - max (median) of `repeats` regions (default 5) after one warm-up round
of every route, the window handed in ready made; then, for the bar's two routes, the kernels' own durations by HIP events (three calls):
  bar       65 536 x 1024 samples as one row, S = N, no detrend, no max row: pss_welch against pss_spectrum_db_f64 on the same buffer (the
            same transforms, a log10 per bin and 537 MB of rows more).  The bar: pss_welch takes less time.
  full      the same shape with detrend and the max row                                        (recorded, no bar)
  cfg 5     99 999 744 samples at N = 4096, S = 2048, beside a device-to-device copy of it     (recorded, no bar)
  bank      192 rows of 500 000 samples at N = 1024, S = 512                                   (recorded, no bar)
A record; bench.py and its line are not touched by any of this.
"""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

from pyspecsdr_amd.engine import Engine
from bench_util import stats, timed


def samples_on_device(n_floats):
    rng = np.random.default_rng(57)
    block = torch.from_numpy((0.5 * rng.standard_normal(1 << 20)).astype(np.float32)).cuda()
    return block.repeat((n_floats + (1 << 20) - 1) >> 20)[:n_floats].contiguous()


def alternate(e, routes, rep):
    for _, fn in routes:
        timed(e, fn)
    times = {name: [] for name, _ in routes}
    for _ in range(rep):
        for name, fn in routes:
            times[name].append(timed(e, fn))
    return times


def main():
    e = Engine(0)
    if len(sys.argv) > 1 and sys.argv[1] == "counters":
        n = 65536 * 1024
        d_iq, d_mean = samples_on_device(2 * n), torch.empty(1024, dtype=torch.float64, device="cuda")
        for _ in range(2):
            e.welch(d_iq, 1, n, 1024, 1024, d_mean, detrend=False)
        e.sync()
        return
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    print(f"pss_welch on {torch.cuda.get_device_name(0)}, host clock around call + synchronise, {rep} alternating regions per route")
    # the bar and its companion
    nf, N = 65536, 1024
    n = nf * N
    d_iq = samples_on_device(2 * n)
    d_db = torch.empty((nf, N), dtype=torch.float64, device="cuda")
    d_rows = torch.empty((2, N), dtype=torch.float64, device="cuda")
    w = Engine.welch_default_window(N)
    routes = [("welch", lambda: e.welch(d_iq, 1, n, N, N, d_rows[0], window=w, detrend=False)),
              ("spectrum_db_f64", lambda: e.spectrum_db_f64(d_iq, nf, N, d_db)),
              ("welch_full", lambda: e.welch(d_iq, 1, n, N, N, d_rows[0], d_rows[1], window=w, detrend=True))]
    t = alternate(e, routes, rep)
    ratio = statistics.median(t["welch"]) / statistics.median(t["spectrum_db_f64"])
    print(f"bar   65 536 x 1024, S = N, no detrend, no max row\n  pss_welch            {stats(t['welch'])}\n  pss_spectrum_db_f64  {stats(t['spectrum_db_f64'])}")
    print(f"  ratio of the medians {ratio:.3f}: the bar is {'met' if ratio < 1 else 'MISSED'}")
    print(f"full  the same with detrend and the max row\n  pss_welch            {stats(t['welch_full'])}")
    e.enable_timing(True)
    e.kernel_times()
    for name, fn in routes[:2]:
        for _ in range(3):
            fn()
        e.sync()
        print(f"  kernel events, {name}: " + ", ".join(f"{k} {statistics.median(v):.3f} ms" for k, v in sorted(e.kernel_times().items())))
    e.enable_timing(False)
    del d_db
    # cfg 5's capture
    n, N, S = 99_999_744, 4096, 2048
    d_iq = samples_on_device(2 * n)
    d_copy = torch.empty_like(d_iq)
    d_rows = torch.empty((2, N), dtype=torch.float64, device="cuda")
    w = Engine.welch_default_window(N)
    t = alternate(e, [("welch", lambda: e.welch(d_iq, 1, n, N, S, d_rows[0], d_rows[1], window=w)), ("copy", lambda: d_copy.copy_(d_iq))], rep)
    print(f"cfg 5 {n} samples, N = {N}, S = {S}, detrend, max row: {Engine.welch_segments(n, N, S)} segments\n  pss_welch            {stats(t['welch'])}\n"
          f"  device-to-device copy of the capture  {stats(t['copy'])}")
    del d_copy
    # bank rows
    K, n, N, S = 192, 500_000, 1024, 512
    d_iq = samples_on_device(2 * K * n)
    d_rows = torch.empty((2, K, N), dtype=torch.float64, device="cuda")
    w = Engine.welch_default_window(N)
    t = alternate(e, [("welch", lambda: e.welch(d_iq, K, n, N, S, d_rows[0], d_rows[1], window=w))], rep)
    print(f"bank  {K} rows of {n} samples, N = {N}, S = {S}, detrend, max row: {Engine.welch_segments(n, N, S)} segments a row\n  pss_welch            {stats(t['welch'])}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""FM mono (pss_decode_mono) beside the NFM and WFM steps of pss_demod on the same device frames, in one process (profiles/fm_mono.txt).

    python tools/bench_mono.py [repeats] > profiles/fm_mono.txt

Two shapes at 2.4 MS/s: 65 536 frames of 1024 samples (the bench line's) and 2048 frames of 32 768 (the recordings' default read
buffer).  The IQ is on the device; every route writes int16 PCM only.  Host clock around call + synchronise, the three routes alternating,
min - max (median) of `repeats` regions (default 5) after one warm-up round of every route.  Then the kernels of one call of each route, from
the context's per-kernel events.  A record, not a pass condition; bench.py and its line are not touched by any of this.
"""
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import torch

import fm_mono_cases as M
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 5
FS = 2.4e6


def stats(v):
    return f"{min(v):.3f} - {max(v):.3f} ms (median {statistics.median(v):.3f}, {len(v)} regions)"


def timed(e, fn):
    e.sync()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return (time.perf_counter() - t0) * 1e3


def kernels(e, fn):
    e.enable_timing(True)
    e.kernel_times()
    fn()
    e.sync()
    kt = e.kernel_times()
    e.enable_timing(False)
    return "  ".join(f"{k}={sum(v):.3f}" for k, v in kt.items()) + " ms"


def shape(e, nf, n):
    base = M.frames(64, n, seed=1)                       # 64 drawn frames, repeated: the kernels' time does not depend on the values
    d_iq = torch.from_numpy(base.view(np.float32)).cuda().repeat((nf + 63) // 64, 1)[:nf].contiguous()
    emp = lambda s: torch.empty(s, dtype=torch.int16, device="cuda")
    n_mono = e.decode_mono_len(n)
    pcm_m, pcm_n, pcm_w = emp((nf, n_mono)), emp((nf, e.demod_out_len(L.MODE_NFM, n, FS), 2)), emp((nf, e.demod_out_len(L.MODE_WFM, n, FS), 2))
    routes = [("pss_decode_mono      ", lambda: e.decode_mono(d_iq, nf, n, FS, pcm_m)),
              ("pss_demod NFM        ", lambda: e.demod(L.MODE_NFM, d_iq, nf, n, FS, pcm_n)),
              ("pss_demod_signal WFM ", lambda: e.demod_signal(L.MODE_WFM, d_iq, nf, n, FS, pcm_w))]
    print(f"\n{nf} frames x {n} samples ({nf * n * 8 / 1e6:.0f} MB of IQ), fs = {FS / 1e6} MS/s; mono: {n_mono} int16 samples a frame")
    torch.cuda.synchronize()
    for _, fn in routes:
        timed(e, fn)
    t = [[] for _ in routes]
    for _ in range(REP):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    for k, (name, fn) in enumerate(routes):
        print(f"    {name} {stats(t[k])}")
    for name, fn in routes:
        print(f"    kernels of {name.strip()}: {kernels(e, fn)}")
    want = Engine.h_decode_mono(base[5], FS)
    assert np.array_equal(pcm_m[5].cpu().numpy(), want), "the device's frame 5 is not the host twin's"
    print("    frame 5 of the mono route equals the host twin bit for bit")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    e = Engine(0, order="none")
    print(f"FM mono beside NFM and WFM; device {torch.cuda.get_device_name(0)}; {REP} timed regions per route, alternating")
    shape(e, 65536, 1024)
    shape(e, 2048, 32768)
    e.close()


if __name__ == "__main__":
    main()

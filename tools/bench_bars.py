#!/usr/bin/env python3
"""Times of the spectrum bars and the gradient lines next to the calls they stand beside, in one process (profiles/spectrum_bars.txt).

    python tools/bench_bars.py [n_frames] [repeats]

(a) pss_spectrum_bars_f64 on the post-processed float64 rows of the batch against the earlier route to the same picture,
pss_spectrogram_cells_f64 on the same rows; (b) pss_frame_pipeline_bars against pss_frame_pipeline_cells (waterfall); (c) pss_spectrum_cells
with display 2 (gradient) against display 0 (waterfall).  Host clock around call + synchronise, the two calls of a pair alternating, median
and range of `repeats` timed regions after two warm-up rounds; per-kernel times of one call from pss_kernel_times.  1024-point NFM frames
whose amplitude varies from frame to frame, 36 x 112 cells.  bench.py and its line are not touched by any of this.
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
N, FS, H, W = 1024, 2.4e6, 36, 112


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


def pair(e, title, name_a, fn_a, name_b, fn_b):
    """fn_a and fn_b alternating: two warm-up rounds, REP timed regions each, then the kernels of one call of each."""
    for _ in range(2):
        fn_a(); fn_b()
    e.sync()
    ta, tb = [], []
    for _ in range(REP):
        ta.append(timed(fn_a, e))
        tb.append(timed(fn_b, e))
    width = max(len(name_a), len(name_b))
    print(title)
    print(f"    {name_a:<{width}}  {stats(ta)}")
    print(f"    {name_b:<{width}}  {stats(tb)}")
    print(f"    ratio of the medians {name_a} / {name_b}: {statistics.median(ta) / statistics.median(tb):.2f}")
    for name, fn in ((name_a, fn_a), (name_b, fn_b)):
        e.enable_timing(True)
        e.kernel_times()
        fn()
        e.sync()
        kt = e.kernel_times()
        e.enable_timing(False)
        print(f"    kernels of one {name}: " + "  ".join(f"{k}={sum(v):.4f}" for k, v in kt.items()) + " ms")
    return statistics.median(ta), statistics.median(tb)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    e = Engine(0, order="none")
    iq = frames(NF, N, 2025)
    n_out = e.demod_out_len(L.MODE_NFM, N, FS)
    emp = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    db32, db64, post = emp((NF, N), torch.float32), emp((NF, N), torch.float64), emp((NF, N - 4), torch.float64)
    lo, hi = emp(NF, torch.float64), emp(NF, torch.float64)
    a, b, pcm = emp((NF, W), torch.int8), emp((NF, W), torch.int8), emp((NF, n_out, 2), torch.int16)
    height, level, rng, rng0 = emp((NF, W), torch.int8), emp((NF, W), torch.int8), emp((NF, 2), torch.float64), emp((NF, 2), torch.float64)
    torch.cuda.synchronize()
    print(f"spectrum bars: {NF} x {N} NFM frames, fs {FS:g}, {H} x {W} cells; device {torch.cuda.get_device_name(0)}; shader clock at start: {clocks()}")

    # (a) the bars against the grids, on the same post-processed rows
    e.spectrum_db_f64(iq, NF, N, db64)
    e.spectrum_post_f64(db64, NF, N, post)
    e.sync()
    chunk = min(NF, 8192)                          # the grids of the whole batch are 2 x NF x H x W bytes: drawn in chunks into one buffer pair
    glyph, colour = emp((chunk, H, W), torch.int8), emp((chunk, H, W), torch.int8)

    def grids():
        for c0 in range(0, NF, chunk):
            c = min(chunk, NF - c0)
            e.spectrogram_cells(post[c0:], c, N - 4, H, W, glyph, colour, rng0[c0:], f64=True)

    bars = lambda: e.spectrum_bars(post, NF, N - 4, H, W, height, level, rng, f64=True)
    tb, tg = pair(e, f"(a) the default view of {NF} post-processed float64 rows of {N - 4} values ({NF * (N - 4) * 8 / 1e6:.0f} MB)",
                  "pss_spectrum_bars_f64", bars, "pss_spectrogram_cells_f64", grids)
    print(f"    pss_spectrum_bars_f64 reads the rows at {NF * (N - 4) * 8 / tb / 1e6:.0f} GB/s and writes {NF * (2 * W + 16) / 1e6:.1f} MB; "
          f"the grids are {2 * NF * H * W / 1e6:.0f} MB")
    # the last chunk expanded: the same cells, the same range
    g2, c2 = emp((chunk, H, W), torch.int8), emp((chunk, H, W), torch.int8)
    c0 = ((NF - 1) // chunk) * chunk
    e.bars_cells(height[c0:], level[c0:], NF - c0, H, W, g2, c2)
    e.sync()
    k = NF - c0
    differing = int((g2[:k] != glyph[:k]).sum().item()) + int((c2[:k] != colour[:k]).sum().item())
    print(f"    cells of the last {k} rows differing between the two routes: {differing}; ranges bit-equal: {bool(torch.equal(rng.view(torch.int64), rng0.view(torch.int64)))}")

    # (b) the step with the default view against the step bench.py times
    pair(e, "(b) one loop iteration per read buffer, NFM",
         "pss_frame_pipeline_bars", lambda: e.frame_pipeline_bars(L.MODE_NFM, iq, NF, N, FS, db32, None, None, H, W, height, level, rng, pcm),
         "pss_frame_pipeline_cells", lambda: e.frame_pipeline_cells(L.MODE_NFM, iq, NF, N, FS, db32, None, lo, hi, W, a, b, pcm))

    # (c) the gradient line against the waterfall line: the same kernels with another quantiser
    pair(e, "(c) the display half alone",
         "pss_spectrum_cells display 2", lambda: e.spectrum_cells(iq, NF, N, db32, None, lo, hi, W, a, b, display="gradient"),
         "pss_spectrum_cells display 0", lambda: e.spectrum_cells(iq, NF, N, db32, None, lo, hi, W, a, b, display="waterfall"))
    print(f"shader clock at end: {clocks()}")
    e.close()


if __name__ == "__main__":
    main()

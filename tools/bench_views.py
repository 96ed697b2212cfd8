#!/usr/bin/env python3
"""Times of the surface magnitudes and the constellation masks next to the one-frame entry points they stand beside, in one process
(profiles/batched_views.txt).

    python tools/bench_views.py [repeats]

(a) pss_surface_mags_f64 on 65 536 float64 rows of 1020 values against pss_surface_cells_f64 looped over 512 of those rows (per-row time);
(b) pss_vector_masks on 65 536 x 1024 and on 2048 x 32 768 samples against pss_vector_cells looped over 512 (all 2048) of those frames;
(c) pss_frame_pipeline_surface / _vector against pss_frame_pipeline_bars, 65 536 x 1024 NFM frames.
The library runs on a torch stream; every number is the median of `repeats` (at least 20) timed calls, each between two events on that
stream, after three warm-up calls.  Screen 40 x 120 (36 x 112 cells).  bench.py and its line are not touched by any of this.
"""
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine

REP = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
FS, H, W = 2.4e6, 40, 120
LOOP = 512


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


def measure(stream, fn):
    """Median and range (ms) of REP calls of fn, each between two events on the library's stream, after three warm-up calls."""
    for _ in range(3):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(REP):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def line(name, m, per=1, unit="ms"):
    scale = 1e3 if unit == "us" else 1.0
    return f"    {name:<46} median {m[0] / per * scale:9.3f} {unit} (min {m[1] / per * scale:.3f}, max {m[2] / per * scale:.3f}, {REP} calls)"


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    stream = torch.cuda.Stream()
    e = Engine(0, stream=stream)
    emp = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    print(f"batched views: screen {H} x {W} ({H - 4} x {W - 8} cells); device {torch.cuda.get_device_name(0)}; shader clock at start: {clocks()}")

    # (a) surface magnitudes: the post-processed float64 rows of 65 536 NFM frames
    NF, N = 65536, 1024
    iq = frames(NF, N, 2025)
    db32, db64, post = emp((NF, N), torch.float32), emp((NF, N), torch.float64), emp((NF, N - 4), torch.float64)
    torch.cuda.synchronize()
    e.spectrum_db_f64(iq, NF, N, db64)
    e.spectrum_post_f64(db64, NF, N, post)
    e.sync()
    mag, rng = emp((NF, W - 8), torch.int8), emp((NF, 2), torch.float64)
    grid = emp((H, W), torch.int8)
    row_mb = NF * (N - 4) * 8 / 1e6
    ta = measure(stream, lambda: e.surface_mags(post, NF, N - 4, W - 8, mag, rng, f64=True))

    def loop_surface():
        for f in range(LOOP):
            e.surface_cells(post[f], N - 4, H, W, grid, f64=True)

    tb = measure(stream, loop_surface)
    print(f"(a) the surface view of {NF} float64 rows of {N - 4} values ({row_mb:.0f} MB)")
    print(line("pss_surface_mags_f64, the batch", ta))
    print(line("pss_surface_mags_f64, per row", ta, NF, "us"))
    print(line(f"pss_surface_cells_f64 looped over {LOOP} rows, per row", tb, LOOP, "us"))
    print(f"    per-row ratio loop / batch: {tb[0] / LOOP / (ta[0] / NF):.0f}; k_surface_mags reads the rows at {row_mb / ta[0] / 1e3:.2f} TB/s "
          f"and writes {NF * (W - 8 + 16) / 1e6:.1f} MB")
    cells = emp((LOOP, H, W), torch.int8)
    e.mags_cells(mag, LOOP, H, W, cells)
    differing = 0
    for f in range(LOOP):
        e.surface_cells(post[f], N - 4, H, W, grid, f64=True)
        stream.synchronize()
        differing += int((cells[f] != grid).sum().item())
    print(f"    cells of the first {LOOP} rows differing between the two routes: {differing}")

    # (b) constellation masks
    words = (W + 31) // 32
    for nf, n in ((65536, 1024), (2048, 32768)):
        x = iq if n == N else iq.view(nf, n, 2)
        mask = emp((nf, H, words), torch.int32)
        loop = min(LOOP, nf)
        tm = measure(stream, lambda: e.vector_masks(x, nf, n, H, W, mask))

        def loop_vector():
            for f in range(loop):
                e.vector_cells(x[f], n, H, W, grid)

        tv = measure(stream, loop_vector)
        mb = nf * n * 8 / 1e6
        print(f"(b) the constellation of {nf} read buffers of {n} samples ({mb:.0f} MB)")
        print(line("pss_vector_masks, the batch", tm))
        print(line("pss_vector_masks, per frame", tm, nf, "us"))
        print(line(f"pss_vector_cells looped over {loop} frames, per frame", tv, loop, "us"))
        print(f"    per-frame ratio loop / batch: {tv[0] / loop / (tm[0] / nf):.0f}; k_vector_masks reads the IQ at {mb / tm[0] / 1e3:.2f} TB/s "
              f"and writes {nf * H * words * 4 / 1e6:.1f} MB")
        grids = emp((loop, H, W), torch.int8)
        e.masks_cells(mask, loop, H, W, grids)
        differing = 0
        for f in range(loop):
            e.vector_cells(x[f], n, H, W, grid)
            stream.synchronize()
            differing += int((grids[f] != grid).sum().item())
        print(f"    cells of the first {loop} frames differing between the two routes: {differing}")

    # (c) one loop iteration per read buffer
    n_out = e.demod_out_len(L.MODE_NFM, N, FS)
    pcm = emp((NF, n_out, 2), torch.int16)
    height, level = emp((NF, W - 8), torch.int8), emp((NF, W - 8), torch.int8)
    mask = emp((NF, H, words), torch.int32)
    tbar = measure(stream, lambda: e.frame_pipeline_bars(L.MODE_NFM, iq, NF, N, FS, db32, None, None, H - 4, W - 8, height, level, rng, pcm))
    tsur = measure(stream, lambda: e.frame_pipeline_surface(L.MODE_NFM, iq, NF, N, FS, db32, None, None, W - 8, mag, rng, pcm))
    tvec = measure(stream, lambda: e.frame_pipeline_vector(L.MODE_NFM, iq, NF, N, FS, db32, None, None, H, W, mask, pcm))
    print(f"(c) one loop iteration per read buffer, NFM, {NF} x {N}")
    print(line("pss_frame_pipeline_bars", tbar))
    print(line("pss_frame_pipeline_surface", tsur))
    print(line("pss_frame_pipeline_vector", tvec))
    print(f"    ratios of the medians to the bars step: surface {tsur[0] / tbar[0]:.3f}, vector {tvec[0] / tbar[0]:.3f}")
    print(f"shader clock at end: {clocks()}")
    e.close()


if __name__ == "__main__":
    main()

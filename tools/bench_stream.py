"""Measurements behind pss_h_stream_frames and pss_live_frames (include/pss.h "replaying a capture") -> profiles/stream_frames.txt.

    python tools/bench_stream.py [--out profiles/stream_frames.txt] [--frames 48828]

One process; every route is timed over FIVE regions (wall time of the synchronous call, behind two warm-up calls), the routes alternating;
median and min .. max are reported.

  stream   the cfg 5 capture (frames x 2048 @ 10 MS/s, chunk_frames 4096, waterfall, window 30, 36 x 112, pinned host memory):
             parent   pss_h_stream_display_nfm_f64 (the code path of the commit before pss_h_stream_frames existed)
             plain    pss_h_stream_frames, NFM, waterfall, no squelch, skip_dead = 0 — the same work through the new call.  Both are bound by
                      the same link; the new call passes if its median lies within the parent call's own min .. max
           and four more routes, reported and not gated: skip_dead = 1 without a dead frame; 1 frame in 64 zeroed; a squelch at the median
           peak; the capture as cu8 codes with WFM and the spectrum bars (the reference's default configuration).
  kernel   k_live_flags alone at 65 536 x 1024 complex64 (device events around pss_live_frames' first launch, pss_timing_filter): all frames
           live (one tile per frame is read) and all frames dead (every byte is read: the achieved TB/s), beside pss_row_meter_f64 on the same
           number of bytes.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pyspecsdr_amd import _lib as L  # noqa: E402
from pyspecsdr_amd.engine import Engine, iq_table  # noqa: E402
from bench_configs import DISP_H, DISP_W, synth  # noqa: E402

N, FS, WINDOW, CHUNK, REGIONS = 2048, 10e6, 30, 4096, 5


def median(v):
    return sorted(v)[len(v) // 2]


def stream_section(lines, nf):
    eng = Engine(0)
    d_f = synth("fm", nf, N, FS, "cuda:0", 20260928 + 5)
    d_c8 = torch.clamp(torch.round(d_f * 128.0), -128, 127)     # the capture on the i8 grid: one set of read buffers, two carriers
    del d_f
    h_iq = eng.pinned_empty((nf, N), np.complex64)
    h_holed = eng.pinned_empty((nf, N), np.complex64)
    h_u8 = eng.pinned_empty((nf, N, 2), np.uint8)
    torch.from_numpy(h_iq.view(np.float32).reshape(nf, N, 2)).copy_(d_c8 / 128.0)
    torch.from_numpy(h_u8).copy_((d_c8 + 128.0).to(torch.uint8))
    del d_c8
    torch.cuda.synchronize()
    h_holed[...] = h_iq
    h_holed[::64] = 0
    table = iq_table((L.IQ_U8, 128.0, 128.0))
    n_out = eng.demod_out_len(L.MODE_NFM, N, FS)
    parent_out = {"lines": (eng.pinned_empty((nf, DISP_W), np.int8), eng.pinned_empty((nf, DISP_W), np.int8)), "pcm": eng.pinned_empty((nf, n_out, 2), np.int16),
                  "row_lo": eng.pinned_empty((nf,), np.float64), "row_hi": eng.pinned_empty((nf,), np.float64)}
    wf = dict(mode=L.MODE_NFM, view="waterfall", window=WINDOW, disp_h=DISP_H, disp_w=DISP_W)

    def pinned_like(first):
        """The route's output buffers, pinned: downloads into pageable memory are staged by the runtime and block the pipeline."""
        return {"buffers": {k: eng.pinned_empty(a.shape, a.dtype) for k, a in first["buffers"].items()}}

    peak = eng.stream_frames(h_iq[:CHUNK], FS, CHUNK, squelch=0.0, skip_dead=False, **wf)["peak"]
    level = float(np.median(peak))
    routes = {
        "parent": lambda o: eng.stream_display_nfm_f64(h_iq, FS, CHUNK, mode="waterfall", window=WINDOW, disp_h=DISP_H, disp_w=DISP_W, out=parent_out),
        "plain": lambda o: eng.stream_frames(h_iq, FS, CHUNK, skip_dead=False, out=o, **wf),
        "skip_dead, none dead": lambda o: eng.stream_frames(h_iq, FS, CHUNK, skip_dead=True, out=o, **wf),
        "skip_dead, 1 in 64 dead": lambda o: eng.stream_frames(h_holed, FS, CHUNK, skip_dead=True, out=o, **wf),
        "squelch at median peak": lambda o: eng.stream_frames(h_iq, FS, CHUNK, skip_dead=False, squelch=level, out=o, **wf),
        "cu8, WFM, bars": lambda o: eng.stream_frames(h_u8, FS, CHUNK, mode=L.MODE_WFM, view="spectrum", fmt=(L.IQ_U8, 128.0, 128.0), table=table,
                                                      skip_dead=True, disp_h=DISP_H, disp_w=DISP_W + 1, out=o),
    }
    outs, last = {}, {}
    for k, fn in routes.items():                      # warm-up per route: buffers, plans, first touch; the second call writes into pinned outputs
        first = fn(None)
        outs[k] = None if k == "parent" else pinned_like(first)
        last[k] = fn(outs[k])
    times = {k: [] for k in routes}
    for _ in range(REGIONS):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            last[k] = fn(outs[k])
            times[k].append((time.perf_counter() - t0) * 1e3)
    same = (all(np.array_equal(a, b) for a, b in zip(last["plain"]["lines"], last["parent"]["lines"])) and np.array_equal(last["plain"]["pcm"], last["parent"]["pcm"])
            and np.array_equal(last["plain"]["row_lo"], last["parent"]["row_lo"]))
    lines.append(f"stream: {nf} x {N} @ {FS / 1e6:g} MS/s, chunk_frames {CHUNK}, waterfall, window {WINDOW}, {DISP_H} x {DISP_W}, pinned host memory (inputs and outputs);")
    lines.append(f"        wall time of the synchronous call, the routes alternating, {REGIONS} timed regions each: median (min .. max)")
    lines.append(f"{'route':<26}{'ms':>9}{'min':>9}{'max':>9}{'/ parent':>10}{'live':>8}{'open':>8}")
    base = median(times["parent"])
    for k in routes:
        nl = last[k].get("n_live", nf)
        no = last[k].get("n_open", nf)
        lines.append(f"{k:<26}{median(times[k]):9.3f}{min(times[k]):9.3f}{max(times[k]):9.3f}{median(times[k]) / base:10.3f}{nl:8d}{no:8d}")
    lo, hi, mp = min(times["parent"]), max(times["parent"]), median(times["plain"])
    ok = lo <= mp <= hi
    lines.append(f"plain against parent: lines, PCM and extremes equal: {same}; median {mp:.3f} ms "
                 + (f"lies within the parent's own spread {lo:.3f} .. {hi:.3f} ms" if ok else
                    f"lies OUTSIDE the parent's own spread {lo:.3f} .. {hi:.3f} ms by {(mp - hi if mp > hi else mp - lo):+.3f} ms ({(mp / base - 1) * 100:+.1f} % of its median)"))
    eng.close()
    return ok and same


def kernel_section(lines):
    nf, n = 65536, 1024
    s = torch.cuda.Stream()
    eng = Engine(0, stream=s)
    d_live = torch.empty(nf, dtype=torch.uint8, device="cuda:0")
    d_peak = torch.empty(nf, dtype=torch.float64, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(3)
    total = nf * n * 8
    lines.append("")
    lines.append(f"kernel: k_live_flags alone, {nf} x {n} complex64 ({total / 1e6:.0f} MB), device events around the launch, {REGIONS} timed launches behind two warm-ups:")
    lines.append(f"{'case':<34}{'ms':>9}{'min':>9}{'max':>9}{'bytes read':>14}{'TB/s':>8}")
    eng.enable_timing(True)

    def timed(name, fn):
        eng.timing_filter(name)
        out = []
        for k in range(REGIONS + 2):
            eng.kernel_times()
            fn()
            eng.sync()
            v = eng.kernel_times().get(name, [])
            if k >= 2:
                out.append(sum(v))
        return out

    for name, d_iq, read in (("all live (one 1 KB tile per frame)", torch.randn(nf * n * 2, dtype=torch.float32, device="cuda:0", generator=g), nf * 1024),
                             ("all dead (every byte)", torch.zeros(nf * n * 2, dtype=torch.float32, device="cuda:0"), total)):
        torch.cuda.synchronize()
        t = timed("k_live_flags", lambda: eng.live_frames(d_iq, nf, n, d_live))
        assert int(d_live.sum().item()) == (nf if "live" in name else 0)
        lines.append(f"{name:<34}{median(t):9.4f}{min(t):9.4f}{max(t):9.4f}{read:14d}{read / median(t) / 1e9:8.3f}")
        del d_iq
    d_rows = torch.randn(nf * n, dtype=torch.float64, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    t = timed("k_row_meter", lambda: eng.row_meter(d_rows, nf, n, d_peak, None))
    lines.append(f"{'pss_row_meter_f64, same bytes':<34}{median(t):9.4f}{min(t):9.4f}{max(t):9.4f}{total:14d}{total / median(t) / 1e9:8.3f}")
    lines.append("every launch re-reads one buffer of twice the 256 MiB last-level cache; the row meter beside it runs under the same conditions.")
    eng.timing_filter(None)
    eng.enable_timing(False)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_frames.txt"))
    ap.add_argument("--frames", type=int, default=48828)
    ap.add_argument("--only", choices=("kernel", "stream"), default=None)
    a = ap.parse_args()
    lines = [f"tools/bench_stream.py --frames {a.frames}  ({torch.cuda.get_device_name(0)})", ""]
    ok = True
    if a.only != "kernel":
        ok = stream_section(lines, a.frames)
    if a.only != "stream":
        kernel_section(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

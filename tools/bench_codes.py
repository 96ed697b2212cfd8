"""Measurements behind the ADC-code entry points (include/pss.h "ADC codes") -> profiles/iq_codes.txt.

    python tools/bench_codes.py [--out profiles/iq_codes.txt] [--frames 48828] [--reps 7]

  kernel   pss_unpack_iq at frames x 2048 samples per container: device events, warm-up per shape, median of --reps; ms and TB/s of
           (code bytes read + 8 B/sample written), beside a plain device-to-device copy moving the same bytes (half read, half written),
           timed in the same process on the same stream.
  stream   the cfg 5 shape (frames x 2048 @ 10 MS/s, chunk_frames 4096, persistence, window 10, 36 x 112, pinned host memory):
           pss_h_stream_display_nfm on the complex64 capture against the _codes call on the same capture as cu8 and as cs16, alternating,
           median of --reps wall times (the calls are synchronous); the three carry the SAME read buffers (codes on the i8 grid: c / 128 =
           256 c / 32768 = table[c + 128]), and their lines and PCM are compared at the timed size.  Each with its H2D rate against this
           box's pinned-copy rate, and the kernels' summed time per capture (what a stream that is no longer link-bound waits for).
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

N, FS, WINDOW, CHUNK = 2048, 10e6, 10, 4096


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(stream, fn, reps):
    """Median of `reps` single launches between two events on `stream`, behind two warm-up launches."""
    out = []
    with torch.cuda.stream(stream):
        for k in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if k >= 2:
                out.append(e0.elapsed_time(e1))
    return median(out), min(out), max(out)


def kernel_section(lines, nf, reps):
    dev = "cuda:0"
    s = torch.cuda.Stream()
    eng = Engine(0, stream=s)
    n_samples = nf * N
    d_iq = torch.empty(2 * n_samples, dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    table = np.random.default_rng(2).standard_normal(256).astype(np.float32)
    lines.append(f"kernel: pss_unpack_iq, {nf} x {N} = {n_samples} complex samples, device events on one stream, median of {reps} (min .. max)")
    lines.append(f"{'container':<22}{'ms':>9}{'min':>9}{'max':>9}{'TB/s':>8}   {'d2d copy ms':>11}{'TB/s':>8}{'kernel / copy':>15}")
    for name, fmt, dt in (("PSS_IQ_U8", (L.IQ_U8, 1.0, 0.0), torch.uint8), ("PSS_IQ_S8", (L.IQ_S8, 1.0, 0.0), torch.int8),
                          ("PSS_IQ_S16 / 32768", (L.IQ_S16, 32768.0, 0.0), torch.int16), ("PSS_IQ_S16 / 1000", (L.IQ_S16, 1000.0, 0.0), torch.int16)):
        info = torch.iinfo(dt)
        d_codes = torch.randint(info.min, info.max + 1, (2 * n_samples,), dtype=dt, device=dev, generator=g)
        tab = table if dt != torch.int16 else None
        total = d_codes.numel() * d_codes.element_size() + 8 * n_samples
        src = torch.empty(total // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        ms, lo, hi = event_ms(s, lambda: eng.unpack_iq(d_codes, n_samples, d_iq, fmt, tab), reps)
        cms, _, _ = event_ms(s, lambda: dst.copy_(src), reps)
        lines.append(f"{name:<22}{ms:9.4f}{lo:9.4f}{hi:9.4f}{total / ms / 1e9:8.3f}   {cms:11.4f}{2 * src.numel() / cms / 1e9:8.3f}{ms / cms:15.3f}")
        del d_codes, src, dst
    eng.close()
    del d_iq
    torch.cuda.empty_cache()


def stream_section(lines, nf, reps):
    dev = "cuda:0"
    eng = Engine(0)
    # one capture, three carriers: synth's FM frames rounded to the i8 grid
    d_f = synth("fm", nf, N, FS, dev, 20260928 + 5)
    d_c8 = torch.clamp(torch.round(d_f * 128.0), -128, 127)
    del d_f
    h_iq = eng.pinned_empty((nf, N), np.complex64)
    h_u8 = eng.pinned_empty((nf, N, 2), np.uint8)
    h_s16 = eng.pinned_empty((nf, N, 2), np.int16)
    torch.from_numpy(h_iq.view(np.float32).reshape(nf, N, 2)).copy_(d_c8 / 128.0)
    torch.from_numpy(h_u8).copy_((d_c8 + 128.0).to(torch.uint8))
    torch.from_numpy(h_s16).copy_((d_c8 * 256.0).to(torch.int16))
    del d_c8
    torch.cuda.synchronize()
    table_u8 = iq_table((L.IQ_U8, 128.0, 128.0))          # offset binary around 128: table[c + 128] = c / 128
    n_out = eng.demod_out_len(L.MODE_NFM, N, FS)

    def outs():
        return {"lines": (eng.pinned_empty((nf, DISP_W), np.int8),), "pcm": eng.pinned_empty((nf, n_out, 2), np.int16),
                "row_lo": eng.pinned_empty((nf,), np.float32), "row_hi": eng.pinned_empty((nf,), np.float32)}
    kw = dict(mode="persistence", window=WINDOW, disp_h=DISP_H, disp_w=DISP_W)
    runs = {
        "cf32": (8, outs(), lambda o: eng.stream_display_nfm(h_iq, FS, CHUNK, out=o, **kw)),
        "cu8": (2, outs(), lambda o: eng.stream_display_nfm_codes(h_u8, FS, CHUNK, (L.IQ_U8, 128.0, 128.0), table=table_u8, out=o, **kw)),
        "cs16": (4, outs(), lambda o: eng.stream_display_nfm_codes(h_s16, FS, CHUNK, "cs16", out=o, **kw)),
    }
    times = {k: [] for k in runs}
    for k, (_, o, fn) in runs.items():                      # warm-up per shape: buffers, plans, first-touch
        fn(o); fn(o)
    for _ in range(reps):                                   # alternating
        for k, (_, o, fn) in runs.items():
            t0 = time.perf_counter()
            fn(o)
            times[k].append((time.perf_counter() - t0) * 1e3)
    ref = runs["cf32"][1]
    same = {k: all(np.array_equal(a, b) for a, b in zip(o["lines"], ref["lines"])) and np.array_equal(o["pcm"], ref["pcm"])
            and np.array_equal(o["row_lo"], ref["row_lo"]) and np.array_equal(o["row_hi"], ref["row_hi"]) for k, (_, o, _) in runs.items()}
    # the link: a plain pinned -> device copy of the complex64 capture
    src = torch.from_numpy(h_iq.view(np.float32).reshape(-1))
    dst = torch.empty(src.numel(), dtype=torch.float32, device=dev)
    dst.copy_(src, non_blocking=True); torch.cuda.synchronize()
    link = []
    for _ in range(max(reps, 5)):
        t0 = time.perf_counter()
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        link.append(nf * N * 8 / (time.perf_counter() - t0) / 1e9)
    link = median(link)
    del dst
    # what each stream's kernels cost per capture (events around every launch: a pass of its own, not a timed one)
    ksum = {}
    for k, (_, o, fn) in runs.items():
        eng.enable_timing(True)
        eng.kernel_times()
        fn(o)
        kt = eng.kernel_times()
        eng.enable_timing(False)
        ksum[k] = (sum(sum(v) for v in kt.values()), sum(sum(v) for n_, v in kt.items() if n_.startswith("k_unpack_iq")))
    lines.append("")
    lines.append(f"stream: {nf} x {N} @ {FS / 1e6:g} MS/s, chunk_frames {CHUNK}, persistence, window {WINDOW}, {DISP_H} x {DISP_W}, pinned host memory;")
    lines.append(f"        wall time of the synchronous call, the three alternating, median of {reps} (min .. max); pinned H2D copy rate of this box: {link:.1f} GB/s")
    lines.append(f"{'capture as':<12}{'B/sample':>9}{'ms':>9}{'min':>9}{'max':>9}{'H2D GB/s':>10}{'of link':>9}{'upload at link rate ms':>24}{'kernels ms':>12}{'unpack ms':>11}{'same results':>14}")
    for k, (bps, _, _) in runs.items():
        ms = median(times[k])
        rate = nf * N * bps / (ms * 1e-3) / 1e9
        lines.append(f"{k:<12}{bps:>9}{ms:9.3f}{min(times[k]):9.3f}{max(times[k]):9.3f}{rate:10.1f}{rate / link:9.2f}{nf * N * bps / link / 1e6:24.3f}"
                     f"{ksum[k][0]:12.3f}{ksum[k][1]:11.3f}{str(same[k]):>14}")
    base = median(times["cf32"])
    for k in ("cu8", "cs16"):
        lines.append(f"{k} / cf32 = {median(times[k]) / base:.3f}  ({'faster' if median(times[k]) < base else 'NOT faster'} than the complex64 stream of the same capture)")
    lines.append("kernels ms: every kernel of the capture, summed, from events around each launch in a separate pass (they overlap the copies in the timed passes);")
    lines.append("a stream whose wall time is near its kernels ms and far above its upload-at-link-rate ms waits for the chunk's compute, not for the link.")
    eng.close()
    return all(same.values()) and all(median(times[k]) < base for k in ("cu8", "cs16"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_codes.txt"))
    ap.add_argument("--frames", type=int, default=48828)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=("kernel", "stream"), default=None)
    a = ap.parse_args()
    assert a.reps >= 5
    lines = [f"tools/bench_codes.py --frames {a.frames} --reps {a.reps}  ({torch.cuda.get_device_name(0)})", ""]
    ok = True
    if a.only != "stream":
        kernel_section(lines, a.frames, a.reps)
    if a.only != "kernel":
        ok = stream_section(lines, a.frames, a.reps)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

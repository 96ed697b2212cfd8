#!/usr/bin/env python3
"""The rational resampler (pss_resample, k_resample) on rows resident on the device, in one process (profiles/resample.txt).

    python tools/bench_resample.py [repeats] > profiles/resample.txt
    python tools/bench_resample.py counters       # two launches of k_resample per shape and nothing else: the program a counter collection runs

Shapes: 192 x 500 000 complex64 at 441/500 (a 12.5 kHz plan's 50 kS/s rows to NFM's 44 100) and at 441/1000 (to AM's 22 050), 16 x
500 000 complex64 at 147/320 (240 kS/s rows to WFM's 110 250), 65 536 x 10 float64 at 3969/4000 (many short rows).  Per shape,
alternating, host clock around call + synchronise, min - max (median) of `repeats` regions (default 5) after one warm-up round of
every route, taps handed in ready made:
  - pss_resample, the outputs exact-rate listening computes (whole read buffers of 32 768 samples on the first two shapes, all elsewhere);
  - a device-to-device copy of as many bytes as the call reads plus writes (the memory floor: recorded, no bar);
  - on the first two shapes, pss_demod_signal (NFM resp. AM, unchanged) on the resampled rows.  The bar: pss_resample takes less time than
    that demodulation step.
Last, 64 outputs of every row from the middle against the host twin.  A record; bench.py and its line are not touched by any of this.
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
from bench_util import stats, timed

FRAME = 32768
SHAPES = [("12.5 kHz plan to NFM", 192, 500_000, np.complex64, 441, 500, L.MODE_NFM, 44100.0),
          ("12.5 kHz plan to AM", 192, 500_000, np.complex64, 441, 1000, L.MODE_AM, 22050.0),
          ("240 kS/s rows to WFM", 16, 500_000, np.complex64, 147, 320, None, 110250.0),
          ("many short rows", 65_536, 10, np.float64, 3969, 4000, None, None)]


def rows_on_device(n_rows, n, dtype):
    rng = np.random.default_rng(53)
    width = 2 if dtype == np.complex64 else 1
    real = np.float32 if dtype == np.complex64 else dtype
    block = (0.5 * rng.standard_normal(1 << 20)).astype(real)
    total = n_rows * n * width
    return torch.from_numpy(block).cuda().repeat((total + (1 << 20) - 1) >> 20)[:total].contiguous().view(n_rows, n * width)


def setup(e, n_rows, n, dtype, up, down, mode):
    taps = Engine.resample_default_taps(up, down)
    n_out = Engine.resample_out_len(n, up, down)
    j_end = n_out // FRAME * FRAME if mode is not None else n_out
    d_x = rows_on_device(n_rows, n, dtype)
    width = 2 if dtype == np.complex64 else 1
    d_y = torch.empty((n_rows, j_end * width), dtype=d_x.dtype, device="cuda")
    return taps, n_out, j_end, d_x, d_y


def shape(e, name, n_rows, n, dtype, up, down, mode, rate, rep):
    taps, n_out, j_end, d_x, d_y = setup(e, n_rows, n, dtype, up, down, mode)
    moved = d_x.numel() * d_x.element_size() + d_y.numel() * d_y.element_size()
    d_a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    d_b = torch.empty_like(d_a)

    def resample():
        e.resample(d_x, dtype, n_rows, n, up, down, d_y, taps=taps, j_end=j_end)

    def copy():
        d_b.copy_(d_a)

    routes = [(f"pss_resample {up}/{down}, {len(taps)} taps", resample), (f"device-to-device copy of {moved / 1e6:.0f} MB read + written", copy)]
    if mode is not None:
        n_frames = n_rows * (j_end // FRAME)
        demod_rate = 22050.0 if mode == L.MODE_AM else rate
        d_pcm = torch.empty((n_frames, e.demod_out_len(mode, FRAME, demod_rate), 2), dtype=torch.int16, device="cuda")
        routes.append((f"pss_demod_signal ({'NFM' if mode == L.MODE_NFM else 'AM'}) on the {n_frames} read buffers of {FRAME}",
                       lambda: e.demod_signal(mode, d_y, n_frames, FRAME, demod_rate, d_pcm)))
    print(f"\n{name}: {n_rows} rows x {n} {np.dtype(dtype).name} at {up}/{down} -> {n_out} outputs a row, {j_end} computed "
          f"({d_x.numel() * d_x.element_size() / 1e6:.0f} MB in, {d_y.numel() * d_y.element_size() / 1e6:.0f} MB out)")
    for _, fn in routes:
        timed(e, fn)
    t = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    for k, (label, _) in enumerate(routes):
        print(f"    {label.ljust(70)} {stats(t[k])}")
    med = [statistics.median(v) for v in t]
    print(f"    pss_resample over the copy: {med[0] / med[1]:.2f}; {n_rows * j_end / med[0] / 1e6:.3f} G outputs / s")
    if mode is not None:
        print(f"    the bar: pss_resample {med[0]:.3f} ms against the demodulation step {med[2]:.3f} ms: ratio {med[0] / med[2]:.4f} -> "
              f"{'met' if med[0] < med[2] else 'MISSED'}")
    resample()
    e.sync()
    j0 = j_end // 2
    j1 = min(j_end, j0 + 64)
    width = 2 if dtype == np.complex64 else 1
    x = d_x.cpu().numpy()
    x = x.view(np.complex64) if dtype == np.complex64 else x
    want = Engine.h_resample(x, up, down, taps=taps, j_begin=j0, j_end=j1)
    got = d_y[:, j0 * width:j1 * width].cpu().numpy()
    got = got.view(np.complex64) if dtype == np.complex64 else got
    assert got.tobytes() == want.tobytes(), "the device's outputs are not the host twin's"
    print(f"    {j1 - j0} outputs of every row from the middle equal the host twin byte for byte")


def counters():
    e = Engine(0, order="none")
    for name, n_rows, n, dtype, up, down, mode, rate in SHAPES:
        taps, n_out, j_end, d_x, d_y = setup(e, n_rows, n, dtype, up, down, mode)
        for _ in range(2):
            e.resample(d_x, dtype, n_rows, n, up, down, d_y, taps=taps, j_end=j_end)
        e.sync()
        print(f"k_resample x 2: {name}, {n_rows} x {n} {np.dtype(dtype).name} at {up}/{down}, {len(taps)} taps, {j_end} outputs a row")
    e.close()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    if len(sys.argv) > 1 and sys.argv[1] == "counters":
        return counters()
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"rational resampler; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    for s in SHAPES:
        shape(e, *s, rep)
    e.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""RDS for every row of a band plan (pss_rds_front, pss_resample, pss_rds_bits, pss_rds_groups) on rows resident on the device, in one
process (profiles/rds.txt).

    python tools/bench_rds.py [repeats] [rows] > profiles/rds.txt
    python tools/bench_rds.py counters        # two launches of k_rds_front on a short batch and nothing else: what a counter collection runs

The rows: 100 bank rows of 2 000 000 samples at 200 kS/s (plan_bank(fs, 100e3)'s channel rate: ten seconds of the whole FM band), noise.
Alternating, host clock around call + synchronise, min - max (median) of `repeats` regions (default 5) after one warm-up round of every
route:
  - the four RDS stages, all rows: "reading every station's name";
  - pss_demod_signal in WFM on the same rows cut into read buffers of 32 768 samples: "listening to every station".
  The bar: the first costs less than the second, both measured here.
Then k_rds_front alone beside a device-to-device copy of the bytes it reads and beside pss_decode_mono on the same samples (both run one
discriminator per sample), and the kernels of the four stages from the context's per-kernel events.  Last, 16 outputs of three rows of
the front against the host twin.  A record; bench.py and its line are not touched by any of this.
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

FS, N, ROWS, FRAME = 200000.0, 2_000_000, 100, 32768


def rows_of(rows, n):
    rng = np.random.default_rng(57)
    block = (0.5 * (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20))).astype(np.complex64)
    total = rows * n
    return torch.from_numpy(block.view(np.float32)).cuda().repeat((total + (1 << 20) - 1) >> 20)[:2 * total].contiguous().view(rows, 2 * n)


class Stages:
    """The four stages on preallocated buffers."""

    def __init__(self, e, d_iq, rows, n):
        self.e, self.d_iq, self.rows, self.n = e, d_iq, rows, n
        self.D, self.up, self.down = Engine.rds_plan(FS)
        self.taps = Engine.ddc_default_taps(self.D)
        self.rs_taps = Engine.resample_default_taps(self.up, self.down)
        self.pulse = Engine.rds_default_pulse()
        self.m = e.lib.pss_ddc_out_len(n, self.D)
        self.n19 = Engine.resample_out_len(self.m, self.up, self.down)
        self.max_bits = Engine.rds_max_bits(self.n19)
        self.max_groups = self.max_bits // 104 + 1
        f32 = dict(dtype=torch.float32, device="cuda")
        self.d_front = torch.empty((rows, 2 * self.m), **f32)
        self.d_bb = torch.empty((rows, 2 * self.n19), **f32)
        self.d_bits = torch.empty((rows, self.max_bits), dtype=torch.uint8, device="cuda")
        self.d_n_bits = torch.empty(rows, dtype=torch.int32, device="cuda")
        self.d_groups = torch.empty((rows, self.max_groups, 4), dtype=torch.int16, device="cuda")
        self.d_pos = torch.empty((rows, self.max_groups), dtype=torch.int32, device="cuda")
        self.d_n_groups = torch.empty(rows, dtype=torch.int32, device="cuda")

    def front(self):
        self.e.rds_front(self.d_iq, self.rows, self.n, FS, self.D, self.d_front, taps=self.taps)

    def rest(self):
        e = self.e
        e.resample(self.d_front, np.complex64, self.rows, self.m, self.up, self.down, self.d_bb, taps=self.rs_taps)
        e.rds_bits(self.d_bb, self.rows, self.n19, self.d_bits, self.max_bits, self.d_n_bits, pulse=self.pulse)
        e.rds_groups(self.d_bits, self.d_n_bits, self.rows, self.max_bits, self.d_groups, self.d_pos, self.max_groups, self.d_n_groups)

    def all(self):
        self.front()
        self.rest()


def counters():
    e = Engine(0, order="none")
    rows, n = 16, 1_000_000
    s = Stages(e, rows_of(rows, n), rows, n)
    for _ in range(2):
        s.front()
    e.sync()
    print(f"k_rds_front x 2: {rows} rows of {n} samples at {FS / 1e3:g} kS/s, D = {s.D}, {len(s.taps)} taps, {s.m} outputs a row")
    e.close()


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    if len(sys.argv) > 1 and sys.argv[1] == "counters":
        return counters()
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else ROWS
    e = Engine(0, order="none")
    d_iq = rows_of(rows, N)
    s = Stages(e, d_iq, rows, N)
    n_frames = rows * N // FRAME
    n_pcm = e.demod_out_len(L.MODE_WFM, FRAME, FS)
    d_pcm = torch.empty((n_frames, n_pcm, 2), dtype=torch.int16, device="cuda")
    n_mono = e.lib.pss_decode_mono_len(FRAME)
    d_mono = torch.empty((n_frames, n_mono), dtype=torch.int16, device="cuda")
    d_copy = torch.empty_like(d_iq)
    print(f"RDS of a band plan; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    print(f"{rows} rows of {N} samples at {FS / 1e3:g} kS/s ({rows * N * 8 / 1e6:.0f} MB): front D = {s.D}, {len(s.taps)} taps -> {s.m} a row; resampler "
          f"{s.up} / {s.down}, {len(s.rs_taps)} taps -> {s.n19} a row at 19 kS/s; {s.max_bits} bits and {s.max_groups} groups of room a row; "
          f"WFM and decode_mono: {n_frames} read buffers of {FRAME}")

    def wfm():
        e.demod_signal(L.MODE_WFM, d_iq, n_frames, FRAME, FS, d_pcm)

    def mono():
        e.decode_mono(d_iq, n_frames, FRAME, FS, d_mono)

    def copy():
        d_copy.copy_(d_iq)

    l_rds, l_wfm = "the four RDS stages, all rows", "pss_demod_signal WFM, the same rows"
    l_front, l_copy, l_mono = "pss_rds_front alone", "device-to-device copy of its input", "pss_decode_mono, the same samples"
    routes = [(l_rds, s.all), (l_wfm, wfm), (l_front, s.front), (l_copy, copy), (l_mono, mono), ("resampler + bits + groups", s.rest)]
    for _, fn in routes:
        timed(e, fn)
    t = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    med = {}
    for k, (label, _) in enumerate(routes):
        med[label] = statistics.median(t[k])
        print(f"    {label.ljust(40)} {stats(t[k])}")
    print(f"    the bar (host clock, medians): reading every station's name {med[l_rds]:.3f} ms against listening to every station {med[l_wfm]:.3f} ms: "
          f"ratio {med[l_rds] / med[l_wfm]:.4f} -> {'met' if med[l_rds] < med[l_wfm] else 'MISSED'}")
    gb = rows * N * 8 / 1e9
    print(f"    k_rds_front's call reads {gb:.2f} GB: {gb / med[l_front] * 1e3:.0f} GB/s; the copy moves the same bytes twice at {2 * gb / med[l_copy] * 1e3:.0f} GB/s; "
          f"front / copy {med[l_front] / med[l_copy]:.2f}, front / decode_mono {med[l_front] / med[l_mono]:.2f}")
    kt = [kernels(e, s.all) for _ in range(rep)]
    for name in kt[0]:
        print(f"    kernel events, {name}: {stats([d[name] for d in kt])}")
    per = statistics.median(d["k_rds_front"] for d in kt) * 1e6 / (rows * N)
    print(f"    k_rds_front: {per:.4f} ns an input sample (one discriminator, one rotor, {2 * len(s.taps) / s.D:.0f} float64 fma)")
    s.front()
    e.sync()
    m0 = s.m // 2
    T = len(s.taps)
    lo, hi = m0 * s.D - T, (m0 + 16) * s.D + T
    pick = [0, rows // 2, rows - 1]
    x = np.stack([d_iq[r, 2 * lo:2 * hi].cpu().numpy().view(np.complex64) for r in pick])
    want = Engine.h_rds_front(x, FS, s.D, taps=s.taps, buf_index0=lo, n_capture=N, m_begin=m0, m_end=m0 + 16)
    got = np.stack([s.d_front[r, 2 * m0:2 * (m0 + 16)].cpu().numpy().view(np.complex64) for r in pick])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the device's outputs are not the host twin's"
    print("    16 outputs of three rows from the middle of the front's result equal the host twin bit for bit")
    e.close()


if __name__ == "__main__":
    main()

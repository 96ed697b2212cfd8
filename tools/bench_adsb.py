#!/usr/bin/env python3
"""Mode S frames of a capture resident on the device (pss_adsb_frames), in one process (profiles/adsb.txt).

    python tools/bench_adsb.py [repeats] > profiles/adsb.txt

Two captures of unit noise with about 1000 frames a second at amplitude 10:
  - 20 000 000 samples taken as 2 MS/s (spc 1: ten seconds of a dongle);
  - 99 999 744 samples taken as 10 MS/s (spc 5).
Alternating, host clock around call + synchronise, min - max (median) of `repeats` regions (default 5) after one warm-up round of every route:
  - pss_adsb_frames on the whole capture;
  - a device-to-device copy of the capture;
  - pss_welch at N = 1024, step N, no detrend, no max row, on the same buffer: the other one-pass reader of a capture.
  The bar: k_adsb_detect (its events) costs less than pss_welch's survey (host clock) of the same capture in this run.
Then the kernels of pss_adsb_frames from the context's per-kernel events, and the records of one stretch against the host twin.  A record;
bench.py and its line are not touched by any of this.
"""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import torch

import adsb_cases as A
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

SHAPES = [(20_000_000, 1), (99_999_744, 5)]
MSGS = (A.IDENT, A.POS_EVEN, A.POS_ODD, A.VELOCITY, A.ALL_CALL)
ROOM = 1 << 18


def capture(n, spc):
    """Noise from one block of 2^20 samples, repeated, then about 1000 frames a second added on the device -> (float32 tensor [2 n], frames)."""
    rng = np.random.default_rng(1090)
    block = ((rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)) / np.sqrt(2.0)).astype(np.complex64)
    d = torch.from_numpy(block.view(np.float32)).cuda().repeat((n + (1 << 20) - 1) >> 20)[:2 * n].contiguous()
    n_frames = int(n / (2e6 * spc) * 1000)
    starts = np.sort(rng.integers(0, n - 240 * spc, n_frames))
    starts = starts[np.concatenate([[True], np.diff(starts) > 260 * spc])]
    for k, s in enumerate(starts):
        w = np.repeat(A.chips_of(MSGS[k % len(MSGS)]), spc) * (10.0 * np.exp(1j * 0.37 * k))
        d[2 * s:2 * (s + len(w))] += torch.from_numpy(w.astype(np.complex64).view(np.float32)).cuda()
    return d, len(starts)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"ADS-B frames of a resident capture; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    d_msg = torch.empty((ROOM, 14), dtype=torch.uint8, device="cuda")
    d_pos = torch.empty(ROOM, dtype=torch.int64, device="cuda")
    d_meta = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_score = torch.empty(ROOM, dtype=torch.float32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    window = Engine.welch_default_window(1024)
    for n, spc in SHAPES:
        d_iq, sent = capture(n, spc)
        d_copy = torch.empty_like(d_iq)
        d_mean = torch.empty(1024, dtype=torch.float64, device="cuda")

        def frames():
            e.adsb_frames(d_iq, n, spc, d_msg, d_pos, d_meta, d_score, d_count, ROOM)

        def copy():
            d_copy.copy_(d_iq)

        def welch():
            e.welch(d_iq, 1, n, 1024, 1024, d_mean, window=window, detrend=False)

        l_f, l_c, l_w = "pss_adsb_frames", "device-to-device copy of the capture", "pss_welch, N = 1024, step N"
        routes = [(l_f, frames), (l_c, copy), (l_w, welch)]
        for _, fn in routes:
            timed(e, fn)
        t = [[] for _ in routes]
        for _ in range(rep):
            for k, (_, fn) in enumerate(routes):
                t[k].append(timed(e, fn))
        found = int(d_count.cpu()[0])
        print(f"{n} samples at {2 * spc} MS/s (spc {spc}, {n * 8 / 1e6:.0f} MB), {sent} frames sent, {found} reported")
        med = {}
        for k, (label, _) in enumerate(routes):
            med[label] = statistics.median(t[k])
            print(f"    {label.ljust(40)} {stats(t[k])}")
        kt = [kernels(e, frames) for _ in range(rep)]
        for name in kt[0]:
            print(f"    kernel events, {name}: {stats([d[name] for d in kt])}")
        det = statistics.median(d["k_adsb_detect"] for d in kt)
        gb = n * 8 / 1e9
        print(f"    k_adsb_detect reads {gb:.2f} GB at {gb / det * 1e3:.0f} GB/s, {det * 1e6 / n:.4f} ns a start; the copy moves the same bytes twice at "
              f"{2 * gb / med[l_c] * 1e3:.0f} GB/s")
        print(f"    the bar (medians): k_adsb_detect {det:.3f} ms against pss_welch {med[l_w]:.3f} ms: ratio {det / med[l_w]:.3f} -> "
              f"{'met' if det < med[l_w] else 'MISSED'}; the whole call against pss_welch: {med[l_f] / med[l_w]:.3f}")
        # one stretch of the capture against the host twin
        s0, s1 = n // 2 + 64, n // 2 + 200_000
        lo_r, hi_r = A.reach(s0, s1, spc, n)
        x = d_iq[2 * lo_r:2 * hi_r].cpu().numpy().view(np.complex64)
        want = Engine.h_adsb_frames(x, spc, buf_index0=lo_r, n_capture=n, s_begin=s0, s_end=s1)
        k = min(found, ROOM)
        pos = d_pos[:k].cpu().numpy()
        sel = (pos >= s0) & (pos < s1)
        assert np.array_equal(pos[sel], want[1]) and np.array_equal(d_msg[:k].cpu().numpy()[sel], want[0]), "the device's records are not the host twin's"
        assert np.array_equal(d_score[:k].cpu().numpy()[sel].view(np.uint32), want[3].view(np.uint32))
        print(f"    the {len(want[1])} records of starts [{s0}, {s1}) equal the host twin's byte for byte")
        del d_iq, d_copy
    e.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""OOK messages of a capture resident on the device (pss_ook_levels, pss_ook_messages), in one process (profiles/ook.txt).

    python tools/bench_ook.py [repeats] > profiles/ook.txt

Unit-power complex noise with seeded sparse PPM traffic 15 dB above it (one transmission of three copies every 250 000 samples: 36 bits,
125-sample pulses, gaps of 250 / 500, 1000 between the copies), at two sizes:
  - 20 000 000 samples (80 s at 250 kS/s);
  - 99 999 744 samples (the cfg 5 capture).
Per route `repeats` timed regions (default 5), the routes alternating, host clock around call + synchronise:
  - pss_ook_levels on the whole capture;
  - pss_ook_messages on the whole capture (P = 9, R = 64, the thresholds from the levels);
  - pss_adsb_frames on the same buffer: existing code that is also one magnitude pass over every IQ sample with a list behind it;
  - a device-to-device copy of the capture.
  The bar: pss_ook_messages takes no longer than pss_adsb_frames on the same buffer in the same run.
Then the kernels of pss_ook_messages from the context's per-kernel events, and the records of one stretch against the host twin.  A record;
not part of the test suite."""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import torch

import ook_cases as K
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

SHAPES = [20_000_000, 99_999_744]
EVERY = 250_000
ROOM = 1 << 16
P, R = 9, 64


def capture(n):
    """Noise from one block of 2^20 samples, repeated, then the transmissions added on the device -> (float32 tensor [2 n], copies sent)."""
    rng = np.random.default_rng(433)
    block = ((rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)) / np.sqrt(2.0)).astype(np.complex64)
    d = torch.from_numpy(block.view(np.float32)).cuda().repeat((n + (1 << 20) - 1) >> 20)[:2 * n].contiguous()
    amp = 10.0 ** (15.0 / 20.0)
    sent = 0
    for k, s in enumerate(range(20_000, n - 80_000, EVERY)):
        bits = rng.integers(0, 2, 36).tolist()
        pulses = K.keying_ppm(bits)
        length = sum(a + b for a, b in pulses) + 1000
        key = K.key_row(3 * length, [(c * length, pulses) for c in range(3)])
        idx = np.flatnonzero(key)
        w = np.zeros(3 * length, np.complex64)
        w[idx] = (amp * np.exp(1j * (2 * np.pi * 0.0137 * idx + 0.3 * k))).astype(np.complex64)
        d[2 * s:2 * (s + len(w))] += torch.from_numpy(w.view(np.float32)).cuda()
        sent += 3
    return d, sent


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"OOK messages of a resident capture; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    spec = dict(K.PPM_SPEC)
    d_bits = torch.empty((ROOM, 32), dtype=torch.uint8, device="cuda")
    d_nb, d_row, d_span, d_meta = (torch.empty(ROOM, dtype=torch.int32, device="cuda") for _ in range(4))
    d_pos = torch.empty(ROOM, dtype=torch.int64, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    a_msg = torch.empty((1 << 18, 14), dtype=torch.uint8, device="cuda")
    a_pos = torch.empty(1 << 18, dtype=torch.int64, device="cuda")
    a_meta = torch.empty(1 << 18, dtype=torch.int32, device="cuda")
    a_score = torch.empty(1 << 18, dtype=torch.float32, device="cuda")
    a_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for n in SHAPES:
        d_iq, sent = capture(n)
        d_copy = torch.empty_like(d_iq)
        nb = n // K.BLOCK
        d_means = torch.empty((1, nb), dtype=torch.float64, device="cuda")
        e.ook_levels(d_iq, 1, n, d_means)
        e.sync()
        hi, lo = F.ook_levels(d_means.cpu().numpy()[0])

        def levels():
            e.ook_levels(d_iq, 1, n, d_means)

        def messages():
            e.ook_messages(d_iq, 1, n, hi, lo, spec, d_bits, d_nb, d_row, d_pos, d_span, d_meta, d_count, ROOM, P=P, R=R)

        def adsb():
            e.adsb_frames(d_iq, n, 1, a_msg, a_pos, a_meta, a_score, a_count, 1 << 18)

        def copy():
            d_copy.copy_(d_iq)

        l_l, l_m, l_a, l_c = "pss_ook_levels", "pss_ook_messages", "pss_adsb_frames (spc 1) on the same buffer", "device-to-device copy of the capture"
        routes = [(l_l, levels), (l_m, messages), (l_a, adsb), (l_c, copy)]
        for _, fn in routes:
            timed(e, fn)
        t = [[] for _ in routes]
        for _ in range(rep):
            for k, (_, fn) in enumerate(routes):
                t[k].append(timed(e, fn))
        messages()
        e.sync()
        found = int(d_count.cpu()[0])
        print(f"{n} samples ({n * 8 / 1e6:.0f} MB), thresholds hi {float(hi):.4f} lo {float(lo):.4f}, {sent} copies sent, {found} reported")
        med = {}
        for k, (label, _) in enumerate(routes):
            med[label] = statistics.median(t[k])
            print(f"    {label.ljust(44)} {stats(t[k])}")
        kt = [kernels(e, messages) for _ in range(rep)]
        for name in kt[0]:
            print(f"    kernel events, {name}: {stats([d[name] for d in kt])}")
        det = statistics.median(d["k_ook_detect"] for d in kt)
        whole = statistics.median(sum(d.values()) for d in kt)
        gb = n * 8 / 1e9
        print(f"    k_ook_detect reads {gb:.2f} GB at {gb / det * 1e3:.0f} GB/s, {det * 1e6 / n:.4f} ns a sample, {100 * det / whole:.0f} % of the call's kernel time; "
              f"the copy moves the same bytes twice at {2 * gb / med[l_c] * 1e3:.0f} GB/s")
        print(f"    the bar (medians): pss_ook_messages {med[l_m]:.3f} ms against pss_adsb_frames {med[l_a]:.3f} ms: ratio {med[l_m] / med[l_a]:.3f} -> "
              f"{'met' if med[l_m] <= med[l_a] else 'MISSED'}")
        # one stretch of the capture against the host twin
        s0, s1 = n // 2 + 64, n // 2 + 1_000_000
        before, after = Engine.ook_halo(P, R, spec['gap_limit'], spec['span'])
        b0, b1 = max(0, s0 - before), min(n, s1 + after)
        x = d_iq[2 * b0:2 * b1].cpu().numpy().view(np.complex64)
        want = Engine.h_ook_messages(x, hi, lo, spec, P=P, R=R, buf_index0=b0, n_row=n, s_begin=s0, s_end=s1)
        k = min(found, ROOM)
        pos = d_pos[:k].cpu().numpy()
        sel = (pos >= s0) & (pos < s1)
        assert np.array_equal(pos[sel], want[3]) and np.array_equal(d_bits[:k].cpu().numpy()[sel], want[0]), "the device's records are not the host twin's"
        assert np.array_equal(d_meta[:k].cpu().numpy()[sel].view(np.uint32), want[5]) and np.array_equal(d_span[:k].cpu().numpy()[sel], want[4])
        print(f"    the {len(want[3])} records of starts [{s0}, {s1}) equal the host twin's byte for byte")
        del d_iq, d_copy
    e.close()


if __name__ == "__main__":
    main()

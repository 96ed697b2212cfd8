#!/usr/bin/env python3
"""FLEX frames of channel rows resident on the device (pss_ais_front with the boxcar + pss_flex_frames), in one process (profiles/flex.txt).

    python tools/bench_flex.py [repeats] > profiles/flex.txt

4 rows x 23 040 000 complex64 samples at 38.4 kS/s (ten minutes of four channels, tools/bench_pocsag.py's) with 100 frames a row, their
modes cycling through the five, 20 dB above unit noise in the 38.4 kS/s band.  Per route `repeats` timed regions (default 5), the routes
alternating, host clock around call + synchronise:
  - the front alone, pss_flex_frames alone, front + frames;
  - pss_pocsag_batches at 1200 bit/s on the same rows;
  - pss_demod_signal NFM on the same rows cut into read buffers of 32 768 samples: listening to the channels;
  - a device-to-device copy of the bytes the front reads and writes (12 bytes a sample).
  The bar: reading the FLEX pagers of the rows takes less time than listening to them: front + frames < the NFM step.
Then the kernels from the context's per-kernel events (k_flex_detect beside k_pocsag_detect), and the records of one stretch against the
host twins.  A record; not part of the test suite."""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import torch

import flex_cases as F
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

ROWS, N = 4, 23_040_000
EVERY = 230_000
FRAME = 32768
ROOM = 1 << 12
H = 12


def rows_on_device():
    """Noise from one block of 2^20 samples, repeated, then the frames added on the device -> (float32 tensor [ROWS][2 N], frames sent per
    mode)."""
    rng = np.random.default_rng(154)
    block = ((rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)) / np.sqrt(2.0)).astype(np.complex64)
    d = torch.from_numpy(block.view(np.float32)).cuda().repeat((ROWS * N + (1 << 20) - 1) >> 20)[:2 * ROWS * N].contiguous().view(ROWS, 2 * N)
    amp = 10.0 ** (20.0 / 20.0)
    waves = []
    for mode in range(5):
        lv = F.frame_levels(mode, F.frame_words(mode, F.MESSAGES), cycle=mode, frame=100 + mode)
        w = (amp * F.fsk_iq(H * len(lv) + 20, H, [(lv, 10)], offset_hz=300.0 * (mode - 2), inverted=mode == 3)).astype(np.complex64)
        waves.append(torch.from_numpy(w.view(np.float32)).cuda())
    sent = [0] * 5
    for r in range(ROWS):
        for k, s in enumerate(range(1000 + 777 * r, N - EVERY, EVERY)):
            mode = (k + r) % 5
            w = waves[mode]
            d[r, 2 * s:2 * s + len(w)] += w
            sent[mode] += 1
    return d, sent


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"FLEX frames of resident channel rows; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    d_iq, sent = rows_on_device()
    d_y = torch.empty((ROWS, N), dtype=torch.float32, device="cuda")
    d_words = torch.empty((ROOM, 4, 88), dtype=torch.int32, device="cuda")
    d_fix = torch.empty((ROOM, 4, 88), dtype=torch.uint8, device="cuda")
    d_fiw = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_row = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_pos = torch.empty(ROOM, dtype=torch.int64, device="cuda")
    d_meta = torch.empty((ROOM, 2), dtype=torch.int32, device="cuda")
    d_score = torch.empty(ROOM, dtype=torch.float32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    p_cw = torch.empty((ROOM, 16), dtype=torch.int32, device="cuda")
    p_fix = torch.empty((ROOM, 16), dtype=torch.uint8, device="cuda")
    p_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    pulse = Engine.flex_default_pulse(H)
    n_frames = ROWS * N // FRAME
    n_out = e.demod_out_len(L.MODE_NFM, FRAME, float(F.RATE))
    d_pcm = torch.empty((n_frames, n_out, 2), dtype=torch.int16, device="cuda")
    flat = d_iq.view(-1)
    n_copy = ROWS * N * 6 // 4                                        # floats: 6 bytes a sample read, 6 written
    d_copy = torch.empty(n_copy, dtype=torch.float32, device="cuda")

    def front():
        e.ais_front(d_iq, ROWS, N, d_y, pulse=pulse)

    def frames():
        e.flex_frames(d_y, ROWS, N, H, d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, d_count, ROOM)

    def both():
        front()
        frames()

    def pocsag():
        e.pocsag_batches(d_y, ROWS, N, 32, p_cw, p_fix, d_row, d_pos, d_fiw, d_score, p_count, ROOM)

    def nfm():
        e.demod_signal(L.MODE_NFM, d_iq, n_frames, FRAME, float(F.RATE), d_pcm=d_pcm)

    def copy():
        d_copy.copy_(flat[:n_copy])

    l_b, l_n = "front + pss_flex_frames", f"pss_demod_signal NFM, {n_frames} buffers of {FRAME}"
    l_f, l_c = f"pss_ais_front, {len(pulse)}-tap boxcar", "device-to-device copy, 12 bytes a sample"
    routes = [(l_b, both), (l_f, front), ("pss_flex_frames", frames), ("pss_pocsag_batches, 1200 bit/s, the same rows", pocsag), (l_n, nfm), (l_c, copy)]
    for label, fn in routes:
        print(f"warm-up: {label}: {timed(e, fn):.3f} ms", file=sys.stderr, flush=True)
    t = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    both()
    e.sync()
    k = min(int(d_count.cpu()[0]), ROOM)
    modes = (d_meta[:k, 0].cpu().numpy().view(np.uint32) >> 12) & 15
    n_bad = d_meta[:k, 1].cpu().numpy().view(np.uint32) & 0xFFFF
    print(f"{ROWS} rows x {N} samples at 38.4 kS/s ({ROWS * N * 8 / 1e6:.0f} MB of IQ); frames sent per mode {sent}, reported "
          f"{[int((modes == m).sum()) for m in range(5)]} ({int(d_count.cpu()[0])} in all, {int((n_bad == 0).sum())} with n_bad = 0 at max_bad = 0)")
    med = {}
    for i, (label, _) in enumerate(routes):
        med[label] = statistics.median(t[i])
        print(f"    {label.ljust(48)} {stats(t[i])}")
    front()
    for what, fn in (("pss_flex_frames", frames), ("pss_pocsag_batches", pocsag), ("pss_ais_front", front)):
        kt = [kernels(e, fn) for _ in range(rep)]
        for name in kt[0]:
            print(f"    kernel events, {what}, {name}: {stats([d[name] for d in kt])}")
    gb = ROWS * N * 12 / 1e9
    print(f"    the front moves {gb:.2f} GB at {gb / med[l_f] * 1e3:.0f} GB/s; the copy moves as many at {gb / med[l_c] * 1e3:.0f} GB/s")
    print(f"    the bar (medians): front + frames {med[l_b]:.3f} ms against the NFM step {med[l_n]:.3f} ms: ratio {med[l_b] / med[l_n]:.3f} -> "
          f"{'met' if med[l_b] < med[l_n] else 'MISSED'}")
    # one stretch of row 1 against the host twins
    both()
    e.sync()
    s0, s1 = N // 2 + 64, N // 2 + 700_000
    lo, hi = F.reach(s0, s1, N, H)
    x = d_iq[1, 2 * (lo - 16):2 * (hi + 15)].cpu().numpy().view(np.complex64)
    y = Engine.h_ais_front(x, pulse=pulse, buf_index0=lo - 16, n_row=N, i_begin=lo, i_end=hi)
    assert np.array_equal(y.view(np.uint32), d_y[1, lo:hi].cpu().numpy().view(np.uint32)), "the device's front is not the host twin's"
    want = Engine.h_flex_frames(y, H, buf_index0=lo, n_row=N, s_begin=s0, s_end=s1)
    pos, row = d_pos[:k].cpu().numpy(), d_row[:k].cpu().numpy()
    sel = (row == 1) & (pos >= s0) & (pos < s1)
    assert np.array_equal(pos[sel], want[4]) and np.array_equal(d_words[:k].cpu().numpy().view(np.uint32)[sel], want[0]), "the device's records are not the host twin's"
    assert np.array_equal(d_score[:k].cpu().numpy()[sel].view(np.uint32), want[6].view(np.uint32)) and np.array_equal(d_fix[:k].cpu().numpy()[sel], want[1])
    assert np.array_equal(d_meta[:k].cpu().numpy().view(np.uint32)[sel], want[5]) and np.array_equal(d_fiw[:k].cpu().numpy().view(np.uint32)[sel], want[2])
    print(f"    the {len(want[4])} records of row 1's starts [{s0}, {s1}) and the front's samples under them equal the host twins' byte for byte")
    e.close()


if __name__ == "__main__":
    main()

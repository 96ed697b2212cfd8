#!/usr/bin/env python3
"""AIS frames of channel rows resident on the device (pss_ais_front + pss_ais_frames), in one process (profiles/ais.txt).

    python tools/bench_ais.py [repeats] > profiles/ais.txt

4 rows x 28 800 000 complex64 samples at 48 kS/s (ten minutes of four channels) with about 2000 GMSK bursts a row, 15 dB above unit noise
in the 48 kS/s band.  Per route `repeats` timed regions (default 5), the routes alternating, host clock around call + synchronise:
  - pss_ais_front + pss_ais_frames on the rows (and each of the two alone);
  - pss_demod_signal NFM on the same rows cut into read buffers of 32 768 samples: listening to the channels;
  - a device-to-device copy of the bytes pss_ais_front reads and writes (12 bytes a sample).
  The bar: reading every ship on the rows takes less time than listening to them: front + frames < the NFM step.
Then the kernels from the context's per-kernel events, and the records of one stretch against the host twins.  A record; not part of the
test suite."""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import torch

import ais_cases as A
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

ROWS, N = 4, 28_800_000
BURSTS = 2000
FRAME = 32768
ROOM = 1 << 16


def rows_on_device():
    """Noise from one block of 2^20 samples, repeated, then the bursts added on the device -> (float32 tensor [ROWS][2 N], bursts sent)."""
    rng = np.random.default_rng(162)
    block = ((rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)) / np.sqrt(2.0)).astype(np.complex64)
    d = torch.from_numpy(block.view(np.float32)).cuda().repeat((ROWS * N + (1 << 20) - 1) >> 20)[:2 * ROWS * N].contiguous().view(ROWS, 2 * N)
    amp = 10.0 ** (15.0 / 20.0)
    waves = []
    for k, m in enumerate(A.SHIPS):
        w = A.synth(5 * (A.TRAINING + 16 + 8 * len(m) + 60), [(A.with_crc(m), 10, amp, 200.0 * (k - 2))])
        waves.append(torch.from_numpy(w.view(np.float32)).cuda())
    sent = 0
    for r in range(ROWS):
        starts = np.sort(rng.integers(100, N - 4000, BURSTS))
        starts = starts[np.concatenate([[True], np.diff(starts) > 3500])]
        for k, s in enumerate(starts):
            w = waves[(k + r) % len(waves)]
            d[r, 2 * s:2 * s + len(w)] += w
        sent += len(starts)
    return d, sent


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"AIS frames of resident channel rows; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    d_iq, sent = rows_on_device()
    d_y = torch.empty((ROWS, N), dtype=torch.float32, device="cuda")
    d_msg = torch.empty((ROOM, 128), dtype=torch.uint8, device="cuda")
    d_len = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_row = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_pos = torch.empty(ROOM, dtype=torch.int64, device="cuda")
    d_score = torch.empty(ROOM, dtype=torch.float32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    pulse = Engine.ais_default_pulse(2)
    n_frames = ROWS * N // FRAME
    n_out = e.demod_out_len(L.MODE_NFM, FRAME, 48000.0)
    d_pcm = torch.empty((n_frames, n_out, 2), dtype=torch.int16, device="cuda")
    flat = d_iq.view(-1)
    n_copy = ROWS * N * 6 // 4                                        # floats: 6 bytes a sample read, 6 written
    d_copy = torch.empty(n_copy, dtype=torch.float32, device="cuda")

    def front():
        e.ais_front(d_iq, ROWS, N, d_y, pulse=pulse)

    def frames():
        e.ais_frames(d_y, ROWS, N, d_msg, d_len, d_row, d_pos, d_score, d_count, ROOM)

    def both():
        front()
        frames()

    def nfm():
        e.demod_signal(L.MODE_NFM, d_iq, n_frames, FRAME, 48000.0, d_pcm=d_pcm)

    def copy():
        d_copy.copy_(flat[:n_copy])

    l_b, l_n = "pss_ais_front + pss_ais_frames", f"pss_demod_signal NFM, {n_frames} buffers of {FRAME}"
    routes = [(l_b, both), ("pss_ais_front", front), ("pss_ais_frames", frames), (l_n, nfm), ("device-to-device copy, 12 bytes a sample", copy)]
    for label, fn in routes:
        print(f"warm-up: {label}: {timed(e, fn):.3f} ms", file=sys.stderr, flush=True)
    t = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    found = int(d_count.cpu()[0])
    print(f"{ROWS} rows x {N} samples at 48 kS/s ({ROWS * N * 8 / 1e6:.0f} MB of IQ), {sent} bursts sent, {found} frames reported")
    med = {}
    for k, (label, _) in enumerate(routes):
        med[label] = statistics.median(t[k])
        print(f"    {label.ljust(48)} {stats(t[k])}")
    for fn in (front, frames):
        kt = [kernels(e, fn) for _ in range(rep)]
        for name in kt[0]:
            print(f"    kernel events, {name}: {stats([d[name] for d in kt])}")
    gb = ROWS * N * 12 / 1e9
    print(f"    pss_ais_front moves {gb:.2f} GB at {gb / med['pss_ais_front'] * 1e3:.0f} GB/s; the copy moves as many at "
          f"{gb / med['device-to-device copy, 12 bytes a sample'] * 1e3:.0f} GB/s")
    print(f"    the bar (medians): front + frames {med[l_b]:.3f} ms against the NFM step {med[l_n]:.3f} ms: ratio {med[l_b] / med[l_n]:.3f} -> "
          f"{'met' if med[l_b] < med[l_n] else 'MISSED'}")
    # one stretch of row 1 against the host twins
    s0, s1 = N // 2 + 64, N // 2 + 400_000
    lo, hi = A.reach(s0, s1, N)
    x = d_iq[1, 2 * (lo - 6):2 * (hi + 5)].cpu().numpy().view(np.complex64)
    y = Engine.h_ais_front(x, pulse=pulse, buf_index0=lo - 6, n_row=N, i_begin=lo, i_end=hi)
    assert np.array_equal(y.view(np.uint32), d_y[1, lo:hi].cpu().numpy().view(np.uint32)), "the device's front is not the host twin's"
    want = Engine.h_ais_frames(y, buf_index0=lo, n_row=N, s_begin=s0, s_end=s1)
    k = min(found, ROOM)
    pos, row = d_pos[:k].cpu().numpy(), d_row[:k].cpu().numpy()
    sel = (row == 1) & (pos >= s0) & (pos < s1)
    assert np.array_equal(pos[sel], want[3]) and np.array_equal(d_msg[:k].cpu().numpy()[sel], want[0]), "the device's records are not the host twin's"
    assert np.array_equal(d_score[:k].cpu().numpy()[sel].view(np.uint32), want[4].view(np.uint32)) and np.array_equal(d_len[:k].cpu().numpy()[sel], want[1])
    print(f"    the {len(want[3])} records of row 1's starts [{s0}, {s1}) and the front's samples under them equal the host twins' byte for byte")
    e.close()


if __name__ == "__main__":
    main()

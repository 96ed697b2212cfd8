#!/usr/bin/env python3
"""POCSAG batches of channel rows resident on the device (pss_ais_front with the boxcar + pss_pocsag_batches), in one process
(profiles/pocsag.txt).

    python tools/bench_pocsag.py [repeats] > profiles/pocsag.txt

4 rows x 23 040 000 complex64 samples at 38.4 kS/s (ten minutes of four channels) with 100 transmissions a row, their rates cycling through
512, 1200 and 2400 bit/s, 15 dB above unit noise in the 38.4 kS/s band.  Per route `repeats` timed regions (default 5), the routes
alternating, host clock around call + synchronise:
  - front + batches at 1200 bit/s (and each of the two alone), at 512 and at 2400 bit/s, and the three rates one after the other;
  - pss_demod_signal NFM on the same rows cut into read buffers of 32 768 samples: listening to the channels;
  - a device-to-device copy of the bytes the front reads and writes (12 bytes a sample).
  The bar: reading the pagers of the rows at 1200 bit/s takes less time than listening to them: front + batches < the NFM step.
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

import pocsag_cases as P
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

ROWS, N = 4, 23_040_000
EVERY = 230_000
FRAME = 32768
ROOM = 1 << 16
BAUDS = (512, 1200, 2400)
MESSAGES = [(1234567, 3, "ten minutes of four channels"), (800001, 0, "0123456789")]


def rows_on_device():
    """Noise from one block of 2^20 samples, repeated, then the transmissions added on the device -> (float32 tensor [ROWS][2 N], batches
    sent per rate)."""
    rng = np.random.default_rng(153)
    block = ((rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)) / np.sqrt(2.0)).astype(np.complex64)
    d = torch.from_numpy(block.view(np.float32)).cuda().repeat((ROWS * N + (1 << 20) - 1) >> 20)[:2 * ROWS * N].contiguous().view(ROWS, 2 * N)
    amp = 10.0 ** (15.0 / 20.0)
    bits = P.transmission_bits(MESSAGES)
    n_batches = len(P.batches_of(MESSAGES))
    waves = {}
    for k, baud in enumerate(BAUDS):
        spb = P.SPB[baud]
        w = (amp * P.fsk_iq(spb * len(bits) + 20, spb, bits, 10, offset_hz=400.0 * (k - 1), inverted=k == 2)).astype(np.complex64)
        waves[baud] = torch.from_numpy(w.view(np.float32)).cuda()
    sent = dict.fromkeys(BAUDS, 0)
    for r in range(ROWS):
        for k, s in enumerate(range(1000 + 777 * r, N - EVERY, EVERY)):
            baud = BAUDS[(k + r) % 3]
            w = waves[baud]
            d[r, 2 * s:2 * s + len(w)] += w
            sent[baud] += n_batches
    return d, sent


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"POCSAG batches of resident channel rows; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    d_iq, sent = rows_on_device()
    d_y = torch.empty((ROWS, N), dtype=torch.float32, device="cuda")
    d_cw = torch.empty((ROOM, 16), dtype=torch.int32, device="cuda")
    d_fix = torch.empty((ROOM, 16), dtype=torch.uint8, device="cuda")
    d_row = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_pos = torch.empty(ROOM, dtype=torch.int64, device="cuda")
    d_meta = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_score = torch.empty(ROOM, dtype=torch.float32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    pulses = {baud: Engine.pocsag_default_pulse(P.SPB[baud]) for baud in BAUDS}
    n_frames = ROWS * N // FRAME
    n_out = e.demod_out_len(L.MODE_NFM, FRAME, float(P.RATE))
    d_pcm = torch.empty((n_frames, n_out, 2), dtype=torch.int16, device="cuda")
    flat = d_iq.view(-1)
    n_copy = ROWS * N * 6 // 4                                        # floats: 6 bytes a sample read, 6 written
    d_copy = torch.empty(n_copy, dtype=torch.float32, device="cuda")

    def front(baud=1200):
        e.ais_front(d_iq, ROWS, N, d_y, pulse=pulses[baud])

    def batches(baud=1200):
        e.pocsag_batches(d_y, ROWS, N, P.SPB[baud], d_cw, d_fix, d_row, d_pos, d_meta, d_score, d_count, ROOM)

    def both(baud=1200):
        front(baud)
        batches(baud)

    def three():
        for baud in BAUDS:
            both(baud)

    def nfm():
        e.demod_signal(L.MODE_NFM, d_iq, n_frames, FRAME, float(P.RATE), d_pcm=d_pcm)

    def copy():
        d_copy.copy_(flat[:n_copy])

    l_b, l_n = "front + pss_pocsag_batches, 1200 bit/s", f"pss_demod_signal NFM, {n_frames} buffers of {FRAME}"
    l_c = "device-to-device copy, 12 bytes a sample"
    routes = [(l_b, both), ("pss_ais_front, 31-tap boxcar", front), ("pss_pocsag_batches, 1200 bit/s", batches),
              ("front + pss_pocsag_batches, 512 bit/s", lambda: both(512)), ("front + pss_pocsag_batches, 2400 bit/s", lambda: both(2400)),
              ("the three rates one after the other", three), (l_n, nfm), (l_c, copy)]
    for label, fn in routes:
        print(f"warm-up: {label}: {timed(e, fn):.3f} ms", file=sys.stderr, flush=True)
    t = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    found = {}
    for baud in BAUDS:
        both(baud)
        e.sync()
        found[baud] = int(d_count.cpu()[0])
    print(f"{ROWS} rows x {N} samples at 38.4 kS/s ({ROWS * N * 8 / 1e6:.0f} MB of IQ); batches sent {sent}, reported {found}")
    med = {}
    for k, (label, _) in enumerate(routes):
        med[label] = statistics.median(t[k])
        print(f"    {label.ljust(48)} {stats(t[k])}")
    for baud in BAUDS:
        front(baud)
        kt = [kernels(e, lambda: batches(baud)) for _ in range(rep)]
        for name in kt[0]:
            print(f"    kernel events, {baud} bit/s, {name}: {stats([d[name] for d in kt])}")
    kt = [kernels(e, front) for _ in range(rep)]
    for name in kt[0]:
        print(f"    kernel events, {name}: {stats([d[name] for d in kt])}")
    gb = ROWS * N * 12 / 1e9
    print(f"    the front moves {gb:.2f} GB at {gb / med['pss_ais_front, 31-tap boxcar'] * 1e3:.0f} GB/s; the copy moves as many at {gb / med[l_c] * 1e3:.0f} GB/s")
    print(f"    the bar (medians): front + batches at 1200 bit/s {med[l_b]:.3f} ms against the NFM step {med[l_n]:.3f} ms: ratio {med[l_b] / med[l_n]:.3f} -> "
          f"{'met' if med[l_b] < med[l_n] else 'MISSED'}")
    # one stretch of row 1 at 1200 bit/s against the host twins
    both(1200)
    e.sync()
    spb = 32
    s0, s1 = N // 2 + 64, N // 2 + 700_000
    lo, hi = P.reach(s0, s1, N, spb)
    x = d_iq[1, 2 * (lo - 16):2 * (hi + 15)].cpu().numpy().view(np.complex64)
    y = Engine.h_ais_front(x, pulse=pulses[1200], buf_index0=lo - 16, n_row=N, i_begin=lo, i_end=hi)
    assert np.array_equal(y.view(np.uint32), d_y[1, lo:hi].cpu().numpy().view(np.uint32)), "the device's front is not the host twin's"
    want = Engine.h_pocsag_batches(y, spb, buf_index0=lo, n_row=N, s_begin=s0, s_end=s1)
    k = min(int(d_count.cpu()[0]), ROOM)
    pos, row = d_pos[:k].cpu().numpy(), d_row[:k].cpu().numpy()
    sel = (row == 1) & (pos >= s0) & (pos < s1)
    assert np.array_equal(pos[sel], want[3]) and np.array_equal(d_cw[:k].cpu().numpy().view(np.uint32)[sel], want[0]), "the device's records are not the host twin's"
    assert np.array_equal(d_score[:k].cpu().numpy()[sel].view(np.uint32), want[5].view(np.uint32)) and np.array_equal(d_fix[:k].cpu().numpy()[sel], want[1])
    assert np.array_equal(d_meta[:k].cpu().numpy().view(np.uint32)[sel], want[4])
    print(f"    the {len(want[3])} records of row 1's starts [{s0}, {s1}) and the front's samples under them equal the host twins' byte for byte")
    e.close()


if __name__ == "__main__":
    main()

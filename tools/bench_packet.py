#!/usr/bin/env python3
"""Packet-radio frames of channel rows resident on the device (pss_packet_front + pss_packet_frames), in one process
(profiles/packet.txt).

    python tools/bench_packet.py [repeats] > profiles/packet.txt

4 rows x 15 840 000 complex64 samples at 26.4 kS/s (ten minutes of four channels) on unit noise, each row carrying as many AFSK frames
of 7 000 to 13 000 samples, 15 dB above the noise in the 26.4 kS/s band and at the clock factors 1, 1.004 and 0.996 in turn, as fit between
2000 random starts a row.  Per route `repeats` timed regions (default 5), the routes alternating, host clock around call + synchronise:
  - pss_packet_front + pss_packet_frames on the rows (and each of the two alone);
  - pss_demod_signal NFM on the same rows cut into read buffers of 32 768 samples: listening to the channels.  NFM's 15 kHz low-pass
    does not exist at 26.4 kS/s (firwin refuses a cutoff above Nyquist, as the reference does), so the same bytes are declared at 38 400 S/s,
    the nearest rate of the project's receivers at which NFM runs: the same decimation (1), the same work a sample;
  - a device-to-device copy of the bytes pss_packet_front reads and writes (12 bytes a sample).
  The bar: reading every packet on the rows takes less time than listening to them: front + frames < the NFM step.
Then the kernels from the context's per-kernel events on the traffic rows and on one row of noise alone, the survivors of the flag test on
both (counted on the host from the device's z), the records of one stretch against the host twins, and a sensitivity table from the host
twins (frames out of frames sent at 6 .. 20 dB for the three clock factors): information, no pass mark.  A record; not part of the test
suite."""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import torch

import packet_cases as P
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

ROWS, N = 4, 15_840_000
DRAWS = 2000
FRAME = 32768
ROOM = 1 << 16
NFM_RATE = 38400.0                                    # see above: NFM refuses 26 400
CLOCKS = (1.0, 1.004, 0.996)


def rows_on_device():
    """Noise from one block of 2^20 samples, repeated, then the frames added on the device -> (float32 tensor [ROWS][2 N], frames sent)."""
    rng = np.random.default_rng(1448)
    block = ((rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)) / np.sqrt(2.0)).astype(np.complex64)
    d = torch.from_numpy(block.view(np.float32)).cuda().repeat((ROWS * N + (1 << 20) - 1) >> 20)[:2 * ROWS * N].contiguous().view(ROWS, 2 * N)
    amp = 10.0 ** (15.0 / 20.0)
    waves = []
    for k, name in enumerate(("position", "compressed", "status", "message", "position", "status")):
        bits = P.burst_bits(P.with_crc(P.FRAMES[name]), lead=6, tail=1)
        clock = CLOCKS[k % 3]
        w = amp * P.synth(int(len(bits) * P.SPB / clock) + 2, [(bits, 0, clock)])
        waves.append(torch.from_numpy(w.view(np.float32)).cuda())
    longest = max(len(w) for w in waves) // 2
    sent = 0
    for r in range(ROWS):
        starts = np.sort(rng.integers(100, N - longest - 100, DRAWS))
        keep, last = [], -longest
        for s in starts:
            if s - last > longest + 200:
                keep.append(int(s))
                last = s
        for k, s in enumerate(keep):
            w = waves[(k + r) % len(waves)]
            d[r, 2 * s:2 * s + len(w)] = w + d[r, 2 * s:2 * s + len(w)]
        sent += len(keep)
    return d, sent


def survivors(z):
    """How many starts of a host row pass the flag test (q_min = 0), vectorised."""
    n = len(z)
    s = np.arange(P.BACK, n - P.HEAD)
    lv = np.stack([z[s + P.SPB * k] > 0 for k in range(-1, 8)])
    b = lv[1:] == lv[:-1]
    return int(np.sum(np.all(b == np.array(P.FLAG, bool)[:, None], axis=0)))


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"packet-radio frames of resident channel rows; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    d_iq, sent = rows_on_device()
    d_z = torch.empty((ROWS, N), dtype=torch.float32, device="cuda")
    d_msg = torch.empty((ROOM, P.REC_BYTES), dtype=torch.uint8, device="cuda")
    d_len = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_row = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_pos = torch.empty(ROOM, dtype=torch.int64, device="cuda")
    d_score = torch.empty(ROOM, dtype=torch.float32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    tones = Engine.packet_default_tones()
    n_frames = ROWS * N // FRAME
    n_out = e.demod_out_len(L.MODE_NFM, FRAME, NFM_RATE)
    d_pcm = torch.empty((n_frames, n_out, 2), dtype=torch.int16, device="cuda")
    flat = d_iq.view(-1)
    n_copy = ROWS * N * 6 // 4                                        # floats: 6 bytes a sample read, 6 written
    d_copy = torch.empty(n_copy, dtype=torch.float32, device="cuda")

    def front():
        e.packet_front(d_iq, ROWS, N, d_z, tones=tones)

    def frames():
        e.packet_frames(d_z, ROWS, N, d_msg, d_len, d_row, d_pos, d_score, d_count, ROOM)

    def both():
        front()
        frames()

    def nfm():
        e.demod_signal(L.MODE_NFM, d_iq, n_frames, FRAME, NFM_RATE, d_pcm=d_pcm)

    def copy():
        d_copy.copy_(flat[:n_copy])

    l_b, l_n = "pss_packet_front + pss_packet_frames", f"pss_demod_signal NFM (as 38.4 kS/s), {n_frames} buffers of {FRAME}"
    routes = [(l_b, both), ("pss_packet_front", front), ("pss_packet_frames", frames), (l_n, nfm), ("device-to-device copy, 12 bytes a sample", copy)]
    for label, fn in routes:
        print(f"warm-up: {label}: {timed(e, fn):.3f} ms", file=sys.stderr, flush=True)
    t = [[] for _ in routes]
    for _ in range(rep):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    found = int(d_count.cpu()[0])
    print(f"{ROWS} rows x {N} samples at 26.4 kS/s ({ROWS * N * 8 / 1e6:.0f} MB of IQ), {sent} frames sent, {found} frames reported")
    med = {}
    for k, (label, _) in enumerate(routes):
        med[label] = statistics.median(t[k])
        print(f"    {label.ljust(48)} {stats(t[k])}")
    for fn in (front, frames):
        kt = [kernels(e, fn) for _ in range(rep)]
        for name in kt[0]:
            print(f"    kernel events, {name}: {stats([d[name] for d in kt])}")
    gb = ROWS * N * 12 / 1e9
    print(f"    pss_packet_front moves {gb:.2f} GB at {gb / med['pss_packet_front'] * 1e3:.0f} GB/s and runs {ROWS * N * 88 / 1e9:.2f} G float64 fma at "
          f"{ROWS * N * 88 / med['pss_packet_front'] / 1e9:.2f} T/s; the copy moves as many bytes at "
          f"{gb / med['device-to-device copy, 12 bytes a sample'] * 1e3:.0f} GB/s")
    print(f"    the bar (medians): front + frames {med[l_b]:.3f} ms against the NFM step {med[l_n]:.3f} ms: ratio {med[l_b] / med[l_n]:.3f} -> "
          f"{'met' if med[l_b] < med[l_n] else 'MISSED'}")
    # survivors of the flag test: the traffic rows, and one row of noise alone
    z0 = d_z[0].cpu().numpy()
    print(f"    survivors of the flag test, row 0 of the traffic rows: {survivors(z0)} of {N} starts")
    del z0
    rng = np.random.default_rng(7)
    block = ((rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)) / np.sqrt(2.0)).astype(np.complex64)
    d_noise = torch.from_numpy(block.view(np.float32)).cuda().repeat((N + (1 << 20) - 1) >> 20)[:2 * N].contiguous().view(1, 2 * N)
    d_zn = torch.empty((1, N), dtype=torch.float32, device="cuda")
    e.packet_front(d_noise, 1, N, d_zn, tones=tones)

    def noise_frames():
        e.packet_frames(d_zn, 1, N, d_msg, d_len, d_row, d_pos, d_score, d_count, ROOM)

    timed(e, noise_frames)
    kt = [kernels(e, noise_frames) for _ in range(rep)]
    print(f"    one row of noise alone: {survivors(d_zn[0].cpu().numpy())} of {N} starts survive, {int(d_count.cpu()[0])} frames reported")
    for name in kt[0]:
        print(f"    kernel events on the noise row, {name}: {stats([d[name] for d in kt])}")
    both()
    e.sync()
    # one stretch of row 1 against the host twins
    s0, s1 = N // 2 + 64, N // 2 + 300_000
    lo, hi = P.reach(s0, s1, N)
    x = d_iq[1, 2 * (lo - 12):2 * (hi + 10)].cpu().numpy().view(np.complex64)
    z = Engine.h_packet_front(x, tones=tones, buf_index0=lo - 12, n_row=N, i_begin=lo, i_end=hi)
    assert np.array_equal(z.view(np.uint32), d_z[1, lo:hi].cpu().numpy().view(np.uint32)), "the device's front is not the host twin's"
    want = Engine.h_packet_frames(z, buf_index0=lo, n_row=N, s_begin=s0, s_end=s1)
    k = min(found, ROOM)
    pos, row = d_pos[:k].cpu().numpy(), d_row[:k].cpu().numpy()
    sel = (row == 1) & (pos >= s0) & (pos < s1)
    assert np.array_equal(pos[sel], want[3]) and np.array_equal(d_msg[:k].cpu().numpy()[sel], want[0]), "the device's records are not the host twin's"
    assert np.array_equal(d_score[:k].cpu().numpy()[sel].view(np.uint32), want[4].view(np.uint32)) and np.array_equal(d_len[:k].cpu().numpy()[sel], want[1])
    print(f"    the {len(want[3])} records of row 1's starts [{s0}, {s1}) and the front's samples under them equal the host twins' byte for byte")
    e.close()
    # sensitivity, by the host twins on the CPU
    print("sensitivity (host twins, 20 frames a cell, frames out of frames sent; no false record counted as one):")
    print("    SNR in 26.4 kHz   " + "  ".join(f"clock {c:.3f}" for c in CLOCKS))
    for snr in range(6, 21, 2):
        cells = []
        for c in CLOCKS:
            x, frames_sent = P.many_frames(20, float(snr), c, 1000 + snr)
            r = Engine.h_packet_frames(Engine.h_packet_front(x))
            got = [bytes(m[:n]) for m, n in zip(r[0], r[1])]
            cells.append(f"{sum(f in got for f in frames_sent):2d} of 20" + ("" if all(g in frames_sent for g in got) else " (+false)"))
        print(f"    {snr:2d} dB             " + "     ".join(cells))


if __name__ == "__main__":
    main()

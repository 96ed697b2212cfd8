#!/usr/bin/env python3
"""NOAA APT lines of channel rows resident on the device (pss_apt_front + pss_apt_syncs + pss_apt_lines), in one process
(profiles/apt.txt).

    python tools/bench_apt.py [repeats] > profiles/apt.txt

4 rows x 56 160 000 complex64 samples at 62.4 kS/s (fifteen minutes of four satellites), each row a synthesised pass: one telemetry frame
of 128 lines (tests/apt_cases.py: a smooth image, +-17 kHz deviation, 20 dB in the row's band, a tuning offset and a clock error of its
own per row) repeated to the row's length from a start of its own.  Per route `repeats` timed regions (default 5), the routes alternating,
host clock around call + synchronise:
  - front, syncs and lines alone, and the three one after the other (the positions of the lines are the grid's of an earlier pass: the
    host's apt_grid between syncs and lines is not timed), on the rows behind apt_rows' carrier step;
  - that carrier step: pss_ais_front with the pulse [1.0], pss_resample 1 / 1024 of the float32 discriminator, pss_ddc at decimation 1
    with one tap, a row at a time (the offsets are those of an earlier pass: the host's apt_offset in between is not timed);
  - pss_demod_signal NFM on the same rows cut into read buffers of 32 768 samples: listening to the channels;
  - a device-to-device copy of the bytes the front reads and writes (8.8 bytes a sample).
  The bar: the three stages together take less time than listening to the rows: front + syncs + lines < the NFM step.
Then the kernels from the context's per-kernel events, and one stretch of a row against the host twins.  A record; not part of the test
suite."""
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import torch

import apt_cases as A
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

ROWS, N = 4, 56_160_000
N_ENV = N // 5
FRAME = 32768
ROOM = 1 << 14
PASSES = ((0.0, 0.0), (3000.0, 40.0), (-2000.0, -25.0), (1500.0, 60.0))   # tuning offset Hz, clock error ppm


def rows_on_device():
    """-> (float32 tensor [ROWS][2 N], lines sent per row): each row one 128-line frame repeated from a start of its own."""
    d = torch.empty((ROWS, 2 * N), dtype=torch.float32, device="cuda")
    sent = []
    for r, (off, ppm) in enumerate(PASSES):
        words = A.pass_words(128, "smooth", 200 + r, ids=(1 + r, 4))
        block = A.modulate(words, 0, off, ppm, 20.0, 300 + r, tail=0)
        start = 3000 + 7919 * r
        reps = (N - start + len(block) - 1) // len(block)
        t = torch.from_numpy(block.view(np.float32)).cuda()
        d[r, :2 * start] = t[-2 * start:]
        d[r, 2 * start:] = t.repeat(reps)[:2 * (N - start)]
        sent.append((N - start) // len(block) * 128 + ((N - start) % len(block)) * 128 // len(block))
    return d, sent


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    e = Engine(0, order="none")
    print(f"APT lines of resident channel rows; device {torch.cuda.get_device_name(0)}; {rep} timed regions per route, alternating")
    d_iq, sent = rows_on_device()
    d_env = torch.empty((ROWS, N_ENV), dtype=torch.float32, device="cuda")
    d_row = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_pos = torch.empty(ROOM, dtype=torch.int64, device="cuda")
    d_meta = torch.empty(ROOM, dtype=torch.int32, device="cuda")
    d_score = torch.empty(ROOM, dtype=torch.float32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    taps = Engine.apt_default_taps()
    one, box, mix = F._apt_tune_taps()
    d_disc = torch.empty((ROWS, N), dtype=torch.float32, device="cuda")
    n_blocks = e.resample_out_len(N, 1, F._APT_TUNE_BLOCK)
    d_means = torch.empty((ROWS, n_blocks), dtype=torch.float32, device="cuda")
    d_raw, d_iq = d_iq, torch.empty_like(d_iq)                      # d_iq: the rows behind the carrier step, which every stage below reads
    words = [np.zeros(1, np.uint64) for _ in range(ROWS)]

    def tune():
        e.ais_front(d_raw, ROWS, N, d_disc, pulse=one)
        e.resample(d_disc, np.float32, ROWS, N, 1, F._APT_TUNE_BLOCK, d_means, taps=box)
        for r in range(ROWS):
            e.ddc(d_raw[r], N, words[r], 1, d_iq[r], taps=mix)

    tune()
    e.sync()
    offsets = [F.apt_offset(m) for m in d_means.cpu().numpy()]
    words = [np.array([Engine.ddc_word(f, float(A.RATE))[0]], np.uint64) for f in offsets]
    tune()
    e.sync()
    n_frames = ROWS * N // FRAME
    n_out = e.demod_out_len(L.MODE_NFM, FRAME, float(A.RATE))
    d_pcm = torch.empty((n_frames, n_out, 2), dtype=torch.int16, device="cuda")
    flat = d_iq.view(-1)
    n_copy = ROWS * (N * 8 + N_ENV * 4) // 2 // 4                      # floats: half of the bytes read, half written
    d_copy = torch.empty(n_copy, dtype=torch.float32, device="cuda")

    def front():
        e.apt_front(d_iq, ROWS, N, d_env, taps=taps)

    def syncs():
        e.apt_syncs(d_env, ROWS, N_ENV, d_row, d_pos, d_meta, d_score, d_count, ROOM)

    # the grid of one pass, on the host: the positions the line gather is timed at
    front()
    syncs()
    e.sync()
    k = int(d_count.cpu()[0])
    assert k <= ROOM
    row, pos, meta, score = (t[:k].cpu().numpy() for t in (d_row, d_pos, d_meta, d_score))
    grids = [F.apt_grid(pos[row == r], meta[row == r], score[row == r], N_ENV) for r in range(ROWS)]
    line_row = np.concatenate([np.full(len(g[0]), r, np.int32) for r, g in enumerate(grids)])
    line_pos = np.concatenate([g[0] for g in grids])
    n_lines = len(line_pos)
    d_lr, d_lp = torch.from_numpy(line_row).cuda(), torch.from_numpy(line_pos).cuda()
    d_words = torch.empty((n_lines, 2080), dtype=torch.float32, device="cuda")

    def lines():
        e.apt_lines(d_env, ROWS, N_ENV, d_lr, d_lp, n_lines, d_words)

    def three():
        front()
        syncs()
        lines()

    def nfm():
        e.demod_signal(L.MODE_NFM, d_iq, n_frames, FRAME, float(A.RATE), d_pcm=d_pcm)

    def copy():
        d_copy.copy_(flat[:n_copy])

    l_t, l_n = "front + syncs + lines", f"pss_demod_signal NFM, {n_frames} buffers of {FRAME}"
    l_f, l_c = "pss_apt_front, 79 taps, decimation 5", "device-to-device copy, 8.8 bytes a sample"
    routes = [(l_t, three), (l_f, front), ("pss_apt_syncs, sync_errors 2", syncs), (f"pss_apt_lines, {n_lines} lines", lines),
              ("the carrier step: discriminator, means, mixer", tune), (l_n, nfm), (l_c, copy)]
    for label, fn in routes:
        print(f"warm-up: {label}: {timed(e, fn):.3f} ms", file=sys.stderr, flush=True)
    t = [[] for _ in routes]
    for _ in range(rep):
        for q, (_, fn) in enumerate(routes):
            t[q].append(timed(e, fn))
    found = [int(g[1].sum()) for g in grids]
    print(f"{ROWS} rows x {N} samples at 62.4 kS/s ({ROWS * N * 8 / 1e6:.0f} MB of IQ); lines sent {sent}, syncs reported {[int((row == r).sum()) for r in range(ROWS)]}, "
          f"grid lines {[len(g[0]) for g in grids]} of which found {found}")
    print(f"    carrier offsets put in {[p[0] for p in PASSES]} Hz, estimated and taken out {[round(f, 1) for f in offsets]} Hz")
    med = {}
    for q, (label, _) in enumerate(routes):
        med[label] = statistics.median(t[q])
        print(f"    {label.ljust(48)} {stats(t[q])}")
    for fn in (front, syncs, lines, tune):
        kt = [kernels(e, fn) for _ in range(rep)]
        for name in kt[0]:
            print(f"    kernel events, {name}: {stats([d[name] for d in kt])}")
    gb = ROWS * (N * 8 + N_ENV * 4) / 1e9
    print(f"    the front moves {gb:.2f} GB at {gb / med[l_f] * 1e3:.0f} GB/s; the copy moves as many at {gb / med[l_c] * 1e3:.0f} GB/s")
    print(f"    the bar (medians): front + syncs + lines {med[l_t]:.3f} ms against the NFM step {med[l_n]:.3f} ms: ratio {med[l_t] / med[l_n]:.3f} -> "
          f"{'met' if med[l_t] < med[l_n] else 'MISSED'}")
    l_s = "the carrier step: discriminator, means, mixer"
    print(f"    with the carrier step in front: {med[l_t] + med[l_s]:.3f} ms, ratio {(med[l_t] + med[l_s]) / med[l_n]:.3f}")
    # one stretch of row 1 against the host twins
    three()
    e.sync()
    m0, m1 = N_ENV // 2 + 64, N_ENV // 2 + 200_000
    lo, hi = m0 * 5 + 39 - 78 - 1, (m1 - 1) * 5 + 39 + 1
    x = d_iq[1, 2 * lo:2 * hi].cpu().numpy().view(np.complex64)
    env = Engine.h_apt_front(x, buf_index0=lo, n_row=N, m_begin=m0, m_end=m1)
    assert np.array_equal(env.view(np.uint32), d_env[1, m0:m1].cpu().numpy().view(np.uint32)), "the device's front is not the host twin's"
    s0, s1 = m0 + 3119, m1 - 3119 - 117
    want = Engine.h_apt_syncs(env, buf_index0=m0, n_row=N_ENV, s_begin=s0, s_end=s1)
    k = int(d_count.cpu()[0])
    pos, row = d_pos[:k].cpu().numpy(), d_row[:k].cpu().numpy()
    sel = (row == 1) & (pos >= s0) & (pos < s1)
    assert np.array_equal(pos[sel], want[1]) and np.array_equal(d_meta[:k].cpu().numpy().view(np.uint32)[sel], want[2]), "the device's records are not the host twin's"
    assert np.array_equal(d_score[:k].cpu().numpy()[sel].view(np.uint32), want[3].view(np.uint32))
    inside = np.flatnonzero((line_row == 1) & (line_pos >= m0) & (line_pos + 6240 <= m1))
    words = Engine.h_apt_lines(env, np.zeros(len(inside), np.int32), line_pos[inside] - m0)
    assert np.array_equal(words.view(np.uint32), d_words[torch.from_numpy(inside).cuda()].cpu().numpy().view(np.uint32)), "the device's lines are not the host twin's"
    print(f"    the {len(want[1])} records of row 1's starts [{s0}, {s1}), the envelope under them and the {len(inside)} lines cut from it equal the host twins' byte for byte")
    e.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The decoders for batches of read buffers, two ways, in one process (profiles/decode_batch.txt).

    python tools/bench_decode.py [repeats] > profiles/decode_batch.txt

Morse: 7200 read buffers of 24 000 samples (an hour of CW at 48 kS/s), the buffers of tests/decode_cases.py's three recordings repeated.
APRS: 2048 read buffers of 24 000 samples, the buffers of its 48 kS/s recording repeated.  The IQ is on the device in both routes.
(a) the route without the batched back halves: the device front half (pss_morse_edges; pss_row_normalise + pss_afsk_bits on float64 real
rows that are already on the device), ONE download of the edge lists [n_frames][cap] / bit rows, a Python loop of pss_h_morse_decode /
pss_h_ax25_frame.  (b) the one-call entries pss_decode_morse_batch / pss_decode_aprs_batch and a download of lengths, timing and the used
text columns.  Host clock around call + synchronise + downloads, the two alternating, min - max (median) of `repeats` regions after one
warm-up round.  Then the kernels of one call of (b), from per-kernel events.  The two routes' results are compared.  bench.py and its line
are not touched by any of this.
"""
import ctypes as C
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np
import torch

import decode_cases as S
from pyspecsdr_amd.engine import Engine

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 3


def stats(v):
    return f"{min(v):.1f} - {max(v):.1f} ms (median {statistics.median(v):.1f}, {len(v)} regions)"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def kernels(e, fn):
    e.enable_timing(True)
    e.kernel_times()
    fn()
    e.sync()
    kt = e.kernel_times()
    e.enable_timing(False)
    return "  ".join(f"{k}={sum(v):.3f}" for k, v in kt.items()) + " ms"


def repeat_to(x, nf):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda().repeat((nf + len(x) - 1) // len(x), 1)[:nf].contiguous()


def morse(e, nf=7200):
    n, fs, cap = 24000, S.MORSE_FS, 24000 // 2 + 1
    d_iq = repeat_to(np.concatenate([S.frames(c) for c in S.MORSE]), nf)
    emp = lambda s, dt: torch.empty(s, dtype=dt, device="cuda")
    rise, fall, cnt = emp((nf, cap), torch.int32), emp((nf, cap), torch.int32), emp((nf, 2), torch.int32)
    text, ln, tm, pulses = emp((nf, 2 * cap), torch.uint8), emp(nf, torch.int32), emp((nf, 3), torch.float64), emp(nf, torch.int32)
    lib = e.lib
    print(f"\nMorse: {nf} read buffers x {n} samples ({nf * n * 8 / 1e6:.0f} MB of IQ), cap {cap}")

    def parent():
        e.morse_edges(d_iq, nf, n, cap, rise, fall, cnt)
        e.sync()
        h_r, h_f, h_c = rise.cpu().numpy(), fall.cpu().numpy(), cnt.cpu().numpy()
        out, buf, t3 = [], C.create_string_buffer(4 * cap + 16), np.zeros(3)
        for k in range(nf):
            r = lib.pss_h_morse_decode(h_r[k].ctypes.data, int(h_c[k, 0]), h_f[k].ctypes.data, int(h_c[k, 1]), fs, buf, 4 * cap + 16, t3.ctypes.data)
            out.append((buf.raw[:r], t3.tobytes()))
        return out

    def batched():
        e.decode_morse_batch(d_iq, nf, n, fs, rise, fall, cnt, text, ln, tm, pulses)
        e.sync()
        h_l, h_t = ln.cpu().numpy(), tm.cpu().numpy()
        h_x = text[:, :max(int(h_l.max()), 1)].cpu().numpy()
        return [(h_x[k, :h_l[k]].tobytes(), h_t[k].tobytes()) for k in range(nf)]

    torch.cuda.synchronize()
    a, b = parent(), batched()
    assert a == b, "the two routes' texts and timing bits differ"
    ta, tb = [], []
    for _ in range(REP):
        ta.append(timed(parent)[0])
        tb.append(timed(batched)[0])
    print(f"    (a) pss_morse_edges + download + {nf} x pss_h_morse_decode  {stats(ta)}")
    print(f"    (b) pss_decode_morse_batch + download of the results        {stats(tb)}")
    print(f"    kernels of (b): {kernels(e, lambda: e.decode_morse_batch(d_iq, nf, n, fs, rise, fall, cnt, text, ln, tm, pulses))}")
    print(f"    texts equal in both routes; {sum(1 for t, _ in b if t)} of {nf} buffers carry text")


def aprs(e, nr=2048):
    c = S.case("aprs_48000")
    n, fs = c.n, c.fs
    nb = e.afsk_n_bits(n, fs)
    out_cap = nb // 8 + 64
    d_iq = repeat_to(S.frames(c), nr)
    d_real = d_iq.view(nr, n, 2)[:, :, 0].double().contiguous()          # the float64 real rows route (a) starts from
    emp = lambda s, dt: torch.empty(s, dtype=dt, device="cuda")
    audio, bits, out, ln = emp((nr, n), torch.float64), emp((nr, nb), torch.uint8), emp((nr, out_cap), torch.uint8), emp(nr, torch.int32)
    lib = e.lib
    print(f"\nAPRS: {nr} read buffers x {n} samples ({nr * n * 8 / 1e6:.0f} MB of IQ), {nb} bits per buffer")

    def parent(src=None):
        e.row_normalise(d_real, nr, n, audio) if src is None else e.real_normalise(d_iq, nr, n, audio)
        e.afsk_bits(audio, nr, n, fs, bits)
        e.sync()
        h_b = bits.cpu().numpy()
        res, buf, m = [], C.create_string_buffer(out_cap), C.c_long(0)
        for k in range(nr):
            r = lib.pss_h_ax25_frame(h_b[k].ctypes.data, nb, buf, out_cap, C.byref(m))
            res.append(buf.raw[:m.value] if r == 1 else None)
        return res

    def batched():
        e.decode_aprs_batch(d_iq, nr, n, fs, audio, bits, out_cap, out, ln)
        e.sync()
        h_l = ln.cpu().numpy()
        h_o = out[:, :max(int(h_l.max()), 1)].cpu().numpy()
        return [h_o[k, :h_l[k]].tobytes() if h_l[k] >= 0 else None for k in range(nr)]

    torch.cuda.synchronize()
    assert parent(src="f32") == batched(), "the two routes' packets differ on the same (float32) quotients"
    ta, tb = [], []
    for _ in range(REP):
        ta.append(timed(parent)[0])
        tb.append(timed(batched)[0])
    print(f"    (a) pss_row_normalise + pss_afsk_bits + download + {nr} x pss_h_ax25_frame  {stats(ta)}")
    print(f"    (b) pss_decode_aprs_batch + download of the results                         {stats(tb)}")
    print(f"    kernels of (b): {kernels(e, lambda: e.decode_aprs_batch(d_iq, nr, n, fs, audio, bits, out_cap, out, ln))}")
    print(f"    packets equal in both routes; {sum(1 for p in batched() if p is not None)} of {nr} buffers carry a packet")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    e = Engine(0, order="none")
    print(f"decoders for batches of read buffers; device {torch.cuda.get_device_name(0)}; {REP} timed regions per route")
    morse(e)
    aprs(e)
    e.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The down-converter (pss_ddc, k_ddc) on captures resident on the device, in one process (profiles/ddc.txt).

    python tools/bench_ddc.py [repeats] > profiles/ddc.txt

Two shapes: the cfg 5 capture (99 999 744 samples at 10 MS/s) to 50 kS/s (D = 200, 4001 taps) and 24 000 000 samples at 2.4 MS/s to 48 kS/s
(D = 50, 1001 taps), each with K = 1 and K = 16 channels and the default taps.  Beside them: a device-to-device copy of the capture's
bytes (the memory floor), K = 16 as 16 calls of K = 1, and the whole user path for K = 16 — ddc + demod_signal(NFM) of all channels —
against the NFM step on the untuned capture.  Host clock around call + synchronise, the routes alternating, min - max (median) of
`repeats` regions (default 5) after one warm-up round of every route; then k_ddc from the context's per-kernel events.  The count-based
floors are computed here from the shapes.  A record, not a pass condition; bench.py and its line are not touched by any of this.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

from pyspecsdr_amd import _lib as L
from pyspecsdr_amd.engine import Engine
from bench_util import kernels, stats, timed

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CUS, CLOCK = 256, 2.4e9          # MI355X: compute units, shader clock the floors are stated at
FRAME = 4096                     # read-buffer length of the channels' NFM step
FRAME_WIDE = 32768               # and of the untuned capture's


def shape(e, name, n, fs, decim):
    rng = np.random.default_rng(51)
    block = (0.5 * (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20))).astype(np.complex64)
    d_iq = torch.from_numpy(block.view(np.float32)).cuda().repeat((n + (1 << 20) - 1) >> 20)[:2 * n].contiguous()
    d_copy = torch.empty_like(d_iq)
    taps = Engine.ddc_default_taps(decim)
    T = len(taps)
    n_out = e.lib.pss_ddc_out_len(n, decim)
    m_end = n_out // FRAME * FRAME                     # whole read buffers for the NFM step
    offsets = [(k - 7.5) / 17.0 * fs / 2 for k in range(16)]
    words = np.array([Engine.ddc_word(f, fs)[0] for f in offsets], np.uint64)
    d_out = torch.empty((16, 2 * n_out), dtype=torch.float32, device="cuda")
    fs2 = fs / decim
    nf2, nfw = 16 * (m_end // FRAME), n // FRAME_WIDE
    d_pcm = torch.empty((nf2, e.demod_out_len(L.MODE_NFM, FRAME, fs2), 2), dtype=torch.int16, device="cuda")
    d_pcm_w = torch.empty((nfw, e.demod_out_len(L.MODE_NFM, FRAME_WIDE, fs), 2), dtype=torch.int16, device="cuda")

    def ddc(k0, k1, end=n_out):
        e.ddc(d_iq, n, words[k0:k1], decim, d_out[k0:], taps=taps, m_end=end, out_stride=n_out)

    def chain():
        e.ddc(d_iq, n, words, decim, d_out, taps=taps, m_end=m_end, out_stride=m_end)
        e.demod_signal(L.MODE_NFM, d_out, nf2, FRAME, fs2, d_pcm)

    routes = [("device-to-device copy of the capture  ", lambda: d_copy.copy_(d_iq)),
              ("pss_ddc K = 1                         ", lambda: ddc(0, 1)),
              ("pss_ddc K = 16, one call              ", lambda: ddc(0, 16)),
              ("pss_ddc K = 1, 16 calls               ", lambda: [ddc(k, k + 1) for k in range(16)]),
              ("pss_ddc K = 16 + demod_signal NFM     ", chain),
              ("demod_signal NFM, the untuned capture ", lambda: e.demod_signal(L.MODE_NFM, d_iq, nfw, FRAME_WIDE, fs, d_pcm_w))]
    print(f"\n{name}: {n} samples ({n * 8 / 1e6:.0f} MB) at {fs / 1e6} MS/s -> {fs2 / 1e3:g} kS/s, D = {decim}, {T} taps, {n_out} outputs a channel")
    steps = n_out * T                                  # tap steps of one channel
    for k in (1, 16):
        fma = k * steps * 2 * 4 / (64 * 4 * CUS * CLOCK) * 1e3       # a wave64 float64 fma issues in 4 clocks on each of a CU's 4 SIMDs
        lds = k * steps * 24 / (256 * CUS * CLOCK) * 1e3             # 16 B of z and 8 B of tap per step at 256 B / clk / CU
        print(f"    floors K = {k:2d}: {k * steps:.3e} tap steps; 2 float64 fma each: {fma:.3f} ms; 24 B of LDS each: {lds:.3f} ms "
              f"-> the {'LDS' if lds > fma else 'fma'} floor binds")
    for _, fn in routes:
        timed(e, fn)
    t = [[] for _ in routes]
    for _ in range(REP):
        for k, (_, fn) in enumerate(routes):
            t[k].append(timed(e, fn))
    for k, (label, fn) in enumerate(routes):
        print(f"    {label} {stats(t[k])}")
    for label, fn in routes[1:]:
        print(f"    kernels of {label.strip()}: " + "  ".join(f"{k}={v:.3f}" for k, v in kernels(e, fn).items()) + " ms")
    ddc(0, 16)
    e.sync()
    m0 = n_out // 2
    lo, hi = m0 * decim - T, (m0 + 64) * decim + T
    want = Engine.h_ddc(d_iq[2 * lo:2 * hi].cpu().numpy().view(np.complex64), words[[3, 11]], decim, taps=taps, buf_index0=lo, n_capture=n, m_begin=m0,
                        m_end=m0 + 64)
    got = d_out[[3, 11], 2 * m0:2 * (m0 + 64)].cpu().numpy().view(np.complex64)
    assert np.array_equal(got, want), "the device's outputs are not the host twin's"
    print("    64 outputs of channels 3 and 11 from the middle of the capture equal the host twin bit for bit")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    e = Engine(0, order="none")
    print(f"down-converter; device {torch.cuda.get_device_name(0)}; {REP} timed regions per route, alternating; floors at {CUS} CUs, {CLOCK / 1e9} GHz")
    shape(e, "cfg 5 capture", 99_999_744, 10e6, 200)
    shape(e, "2.4 MS/s capture", 24_000_000, 2.4e6, 50)
    e.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""When k_spectrum_post's workgroups start and end INSIDE the step (beside k_nfm_bwd), from the per-workgroup s_memrealtime stamps of a
timing-only build (-DPSS_EXP_POST_STAMPS: lane 0 of every workgroup stores the 100 MHz clock at its first and its last instruction):

    python tools/build_variant.py stamps -DPSS_EXP_POST_STAMPS
    PSS_LIBRARY=pyspecsdr_amd/libpss_stamps.so python tools/post_stamps.py [frames] [post_split values ...]      (default 65536, 0 and -1)
    POST_STAMPS_MODE=wfm: the WFM step; POST_STAMPS_ALONE=1: the display half alone (pss_spectrum_cells)

Per post_split value, for the last of a few steps: how many workgroups start within 20 us of the first and whether they are workgroups
0 .. CUs - 1 (the launch geometry's assumption), when the others start, when the first and the last workgroup end and the spread between
the two, and the mean of the late and of the early workgroups' ends.  Times in us from the first workgroup's start."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pyspecsdr_amd import _lib as L  # noqa: E402
from pyspecsdr_amd.engine import Engine  # noqa: E402


def main():
    args = [a for a in sys.argv[1:]]
    nf = int(args.pop(0)) if args and args[0].isdigit() and int(args[0]) > 64 else 65536
    splits = [int(a) for a in args] or [0, -1]
    n, fs, W = 1024, 2.4e6, 112
    eng = Engine(0, order="none")
    raw = C.CDLL(L.LIB_PATH)
    if not hasattr(raw, "pss_exp_post_stamps"):
        sys.exit("this library was built without -DPSS_EXP_POST_STAMPS (see the docstring)")
    raw.pss_exp_post_stamps.restype = C.c_long
    raw.pss_exp_post_stamps.argtypes = [C.c_void_p, C.c_long]
    mode = {"nfm": L.MODE_NFM, "wfm": L.MODE_WFM}[os.environ.get("POST_STAMPS_MODE", "nfm")]
    alone = os.environ.get("POST_STAMPS_ALONE") == "1"
    dev = torch.device("cuda", 0)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    iq = bench.synth_fm_iq(nf, n, fs, dev, seed=5)
    db32 = torch.zeros((nf, n), dtype=torch.float32, device=dev)
    lo, hi = torch.zeros(nf, dtype=torch.float64, device=dev), torch.zeros(nf, dtype=torch.float64, device=dev)
    g, c = torch.zeros((nf, W), dtype=torch.int8, device=dev), torch.zeros((nf, W), dtype=torch.int8, device=dev)
    pcm = torch.zeros((nf, eng.demod_out_len(mode, n, fs), 2), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    n_wg = min((nf + 3) // 4, 2 * ncu)
    buf = np.zeros((2 * ncu, 2), np.uint64)
    print(f"{nf} frames, {ncu} CUs, {n_wg} workgroups, {'display half alone' if alone else 'mode ' + str(mode)}; library {L.LIB_PATH}")
    for split in splits:
        eng.set_option("post_split", split)
        for _ in range(6):
            if alone:
                eng.spectrum_cells(iq, nf, n, db32, None, lo, hi, W, g, c, window=30)
            else:
                eng.frame_pipeline_cells(mode, iq, nf, n, fs, db32, None, lo, hi, W, g, c, pcm, window=30)
        eng.sync()
        got = raw.pss_exp_post_stamps(buf.ctypes.data, 2 * ncu)
        assert got >= n_wg, got
        t = (buf[:n_wg].astype(np.int64) - int(buf[:n_wg, 0].min())) / 100.0        # 100 MHz -> us
        start, end = t[:, 0], t[:, 1]
        early = np.flatnonzero(start <= 20.0)
        late = np.flatnonzero(start > 20.0)
        print(f"post_split = {split}:")
        print(f"  {early.size} workgroups start within 20 us of the first; they are workgroups 0 .. {ncu - 1}: "
              f"{bool(early.size == min(ncu, n_wg) and np.array_equal(early, np.arange(early.size)))}"
              f" (lowest {early.min()}, highest {early.max()}, {int(np.count_nonzero(early < ncu))} of them below {ncu})")
        if late.size:
            s = np.sort(start[late])
            print(f"  the other {late.size} start at {s[0]:.1f} .. {s[-1]:.1f} us (median {np.median(s):.1f}, 10 % / 90 %: {s[late.size // 10]:.1f} / {s[late.size * 9 // 10]:.1f})")
        print(f"  first workgroup ends at {end.min():.1f} us, last at {end.max():.1f} us: spread {end.max() - end.min():.1f} us"
              f" (10 % / 90 % of the ends: {np.sort(end)[n_wg // 10]:.1f} / {np.sort(end)[n_wg * 9 // 10]:.1f})")
        if late.size:
            print(f"  mean end of the early workgroups {end[early].mean():.1f} us, of the late ones {end[late].mean():.1f} us;"
                  f" mean run time early {np.mean(end[early] - start[early]):.1f} us, late {np.mean(end[late] - start[late]):.1f} us")
    eng.close()


if __name__ == "__main__":
    main()

"""k_spectrum_post's one-round grid with two shares (pss_post_split.h, pss_spec_post.h, pss_spec_post_chain): the partition on the host, and
every frame of batches around the grid's edges on the GPU, at every kind of skew."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")
FS, N, W, WIN = 2.4e6, 1024, 112, 30


def test_partition_header_alone_runs_clean_under_the_sanitizers(tmp_path):
    """tests/post_split_host.cpp: pss_post_split.h with the host compiler — the header must not need HIP — under AddressSanitizer and UBSan,
    as a program of its own: groups 1 .. 6000 x n_workgroups {1, 2, 255, 256, 257, 511, 512} x d {0, 1, 7, 16, 31, 32, 1000} x n_early
    {0, 1, 256, n_workgroups}; every group covered exactly once, no range past the batch, share_late >= 1 after clamping."""
    exe = str(tmp_path / "post_split_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(HERE, "post_split_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "post_split_host: ok" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- the header's two functions restated (only to find where a workgroup's range begins and ends: the planted frames below) ----------------
def _shares(groups, n_wg, n_early, d):
    ne = min(max(n_early, 0), n_wg)
    if d < 0 or ne == 0 or ne == n_wg:
        d = 0
    if groups < n_wg:
        return ne, 1, 1
    if d > 0 and n_wg + ne * d > groups:
        d = (groups - n_wg) // ne
    late = (groups - ne * d) // n_wg
    return ne, late + d, late


def _range(groups, n_wg, ne, se, sl, b):
    left = max(groups - (ne * se + (n_wg - ne) * sl), 0)
    first_extra = n_wg - left
    g0 = b * se if b < ne else ne * se + (b - ne) * sl
    g1 = g0 + (se if b < ne else sl) + (1 if b >= first_extra else 0)
    g0 += max(b - first_extra, 0)
    g1 += max(b - first_extra, 0)
    return min(g0, groups), min(g1, groups)


def test_restated_partition_covers_every_group():
    for groups in (1, 2, 255, 256, 257, 512, 513, 1542, 6000):
        for n_wg in (1, 256, 257, 512):
            for d in (0, 3, 1000):
                ne, se, sl = _shares(groups, n_wg, 256, d)
                at = 0
                for b in range(n_wg):
                    g0, g1 = _range(groups, n_wg, ne, se, sl, b)
                    assert g0 == at and g0 <= g1 <= groups
                    at = g1
                assert at == groups and sl >= 1


# 4 * 511 + 3: a full grid of 512 groups whose last one is ragged (on 256 CUs) — the same number as 2047, so it runs once
FRAME_COUNTS = list(dict.fromkeys([1, 5, 1023, 1024, 1025, 2047, 2049, 4 * 511 + 3, 6165]))
SPLITS = (-1, 0, 3, 1000)      # automatic, equal shares, a small skew, a skew far above the mean share (1 .. 4 groups here): clamped


def _planted(nf, ncu):
    """(NaN frame, +inf frame): the first and the last frame of a late workgroup's range under post_split = 3 (the middle one of the late
    workgroups; the last workgroup where the batch has none); None where the range has one frame only / the batch one frame."""
    groups = (nf + 3) // 4
    n_wg = min(groups, 2 * ncu)
    ne, se, sl = _shares(groups, n_wg, ncu, 3)
    b = ne + (n_wg - ne) // 2 if n_wg > ne else n_wg - 1
    g0, g1 = _range(groups, n_wg, ne, se, sl, b)
    assert g0 < g1
    first, last = 4 * g0, min(4 * g1, nf) - 1
    if nf == 1:
        return None, None
    return first, (last if last != first else None)


def _f64_failures(got, want, any_nonfinite):
    """tests/test_db_eval.py's rule for float64 rows: 1e-11 on finite bins, non-finite bins by kind — except the frame with a +inf sample,
    where which bins are +inf and which NaN is the transform's factorisation (NOTEBOOK R7-01): non-finite where the oracle's are."""
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        ok = np.where(fin, np.isclose(got, want, rtol=1e-11, atol=1e-11), (np.isnan(got) & np.isnan(want)) | (got == want))
    for f in any_nonfinite:
        ok[f] |= ~np.isfinite(got[f]) & ~fin[f]
    return ~ok


@pytest.mark.gpu
@pytest.mark.parametrize("nf", FRAME_COUNTS)
def test_every_frame_at_every_skew_equals_the_two_kernels_and_the_oracle(nf):
    """pss_frame_pipeline_cells (NFM) and pss_spectrum_cells on 1024-point frames, option post_split = -1, 0, 3 and 1000, both row types
    written: dB rows, row extremes, display cells and PCM of EVERY frame bit for bit the same call's with fuse_post = 0 (the float32 row: its
    float64 row rounded once), and the oracle's step from the IQ (cells and PCM bit for bit; float64 rows and extremes to 1e-11, the bound of
    tests/test_db_eval.py).  The batches end inside the early zone, exactly on it, one group past it, on the full grid with a ragged last
    group, one group past the full grid, and in the middle of a third round's worth of groups.  A frame with a NaN sample and one with a
    +inf sample sit at the first and the last frame of a late workgroup's range.  Every output buffer is pre-filled (with different values
    for the two calls that are compared), so a frame nobody wrote shows."""
    import torch
    import bench
    import gpu_util as G
    import oracle_lib as O
    from pyspecsdr_amd import _lib as L
    e = G.engine()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    iq = bench.synth_fm_iq(nf, N, FS, torch.device("cuda", 0), seed=4100 + nf)
    f_nan, f_inf = _planted(nf, ncu)
    iq = iq.reshape(nf, N, 2)
    if f_nan is not None:
        iq[f_nan, 17, 0] = float("nan")
    if f_inf is not None:
        iq[f_inf, 5, 1] = float("inf")
    torch.cuda.synchronize()
    x = iq.cpu().numpy().reshape(nf, 2 * N).view(np.complex64)
    taps, sos, zi = e.nfm_filters(FS)
    with np.errstate(all="ignore"):
        o = O.headline_f64(x, FS, taps, sos, zi, WIN, W, min(O.threads_available(), 16), keep_db=True)
    n_out = e.demod_out_len(L.MODE_NFM, N, FS)

    def bufs(fill):
        def full(shape, dtype, v):
            return torch.full(shape, v, dtype=dtype, device="cuda")
        return dict(db32=full((nf, N), torch.float32, -1000.0 - fill), db64=full((nf, N), torch.float64, -2000.0 - fill),
                    lo=full((nf,), torch.float64, -3000.0 - fill), hi=full((nf,), torch.float64, -4000.0 - fill),
                    a=full((nf, W), torch.int8, 100 + fill), b=full((nf, W), torch.int8, 110 + fill), pcm=full((nf, n_out, 2), torch.int16, 12345 + fill))

    def run(demod, fuse, split, fill):
        c = bufs(fill)
        e.set_option("fuse_post", fuse)
        e.set_option("post_split", split)
        if demod:
            e.frame_pipeline_cells(L.MODE_NFM, iq, nf, N, FS, c["db32"], c["db64"], c["lo"], c["hi"], W, c["a"], c["b"], c["pcm"], window=WIN)
        else:
            e.spectrum_cells(iq, nf, N, c["db32"], c["db64"], c["lo"], c["hi"], W, c["a"], c["b"], window=WIN)
        e.sync()
        return c

    fails = []
    try:
        for demod in (True, False):
            tag0 = "frame_pipeline_cells" if demod else "spectrum_cells"
            ref = run(demod, 0, -1, 1)
            keys = ("db32", "db64", "lo", "hi", "a", "b") + (("pcm",) if demod else ())
            # the two-kernel reference itself against the oracle, once
            d64 = G.host(ref["db64"])
            bad = _f64_failures(d64, o["db"], () if f_inf is None else (f_inf,))
            if bad.any():
                fails.append((tag0, "float64 rows outside 1e-11 of the oracle's", int(bad.sum()), np.argwhere(bad)[:3].tolist()))
            assert torch.equal(ref["db32"].view(torch.int32), ref["db64"].float().view(torch.int32)), (tag0, "the float32 row is the float64 row rounded once")
            for split in SPLITS:
                tag = f"{tag0} post_split={split}"
                c = run(demod, 1, split, 2)
                for k in keys:
                    if not torch.equal(c[k].view(torch.uint8), ref[k].view(torch.uint8)):
                        rows = torch.nonzero((c[k].view(torch.uint8).reshape(nf, -1) != ref[k].view(torch.uint8).reshape(nf, -1)).any(dim=1)).flatten()
                        fails.append((tag, k, "differs from fuse_post = 0 in", int(rows.numel()), "frames, first", rows[:5].tolist()))
                for k in ("lo", "hi"):
                    if not np.allclose(G.host(c[k]), o[k], rtol=1e-11, atol=1e-11, equal_nan=True):
                        fails.append((tag, k, "outside 1e-11 of the oracle's"))
                for k, ok in (("a", "glyph"), ("b", "colour")):
                    rows = np.flatnonzero((G.host(c[k]) != o[ok]).any(axis=1))
                    if rows.size:
                        fails.append((tag, ok, "cells differ from the oracle's in", int(rows.size), "frames, first", rows[:5].tolist()))
                if demod and not np.array_equal(G.host(c["pcm"]), o["pcm"]):
                    fails.append((tag, "pcm differs from the oracle's", int(np.count_nonzero((G.host(c["pcm"]) != o["pcm"]).any(axis=(1, 2))))))
    finally:
        e.set_option("fuse_post", 1)
        e.set_option("post_split", -1)
    for f in fails:
        print("MISMATCH", f)
    assert not fails, fails[:10]

"""Squelch and the header's Peak / Avg meter on the GPU: pss_row_meter_f64, pss_squelch_gate, pss_demod_gated,
pss_frame_pipeline_squelch and formats.demodulate_recording(squelch=...).  Every comparison is equality of bits or bytes (NaN compared
as NaN; np.max of a row of zeros may carry either sign): against tests/golden/squelch.npz (the reference's own draw_header and loop
condition), host np.max / np.mean, the host gate pss_h_squelch_gate, and the ungated entry points on the same frames.

New capped grids, each walked one row / frame past its cap here: k_row_meter<64> (8192 workgroups of 4 rows), k_row_meter<256> (4096
workgroups of one row), k_gate_flags / k_gate_index (4096 workgroups of 256 frames), k_gather_frames (2048 workgroups of one frame).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_util as G
import squelch_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats
from pyspecsdr_amd.engine import h_squelch_gate

FS = 2.4e6
MODES = (L.MODE_NFM, L.MODE_AM, L.MODE_USB, L.MODE_LSB, L.MODE_WFM)
METER_WAVE_CAP_ROWS = 8192 * 4      # pss_squelch.hip: rows of up to 2048 values, four per workgroup
METER_GROUP_CAP_ROWS = 4096         # longer rows, one per workgroup
GATE_CAP_FRAMES = 4096 * 256
GATHER_CAP_FRAMES = 2048


def sentinel(shape, dtype):
    """A device buffer of 0x7f bytes: a value the kernels never produce, so an element never written fails."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0x7F)
    return t


def is_sentinel(t):
    return bool((t.contiguous().view(torch.uint8) == 0x7F).all())


def meter(rows):
    e = G.engine()
    rows = np.ascontiguousarray(rows, np.float64)
    nr, ln = rows.shape
    d_peak, d_avg = sentinel((nr,), torch.float64), sentinel((nr,), torch.float64)
    e.row_meter(G.dev(rows), nr, ln, d_peak, d_avg)
    e.sync()
    return G.host(d_peak), G.host(d_avg)


# ---- row meter ------------------------------------------------------------------------------------------------------------------------
def test_row_meter_equals_the_golden_peaks_averages_and_texts():
    gold = S.golden()
    for i, row in enumerate(S.golden_rows()):
        peak, avg = meter(row[None, :])
        assert S.same_bits(peak[0], gold["peak"][i]), (i, len(row), peak[0], gold["peak"][i])
        assert S.exact_bits(avg[0], gold["avg"][i]), (i, len(row), avg[0], gold["avg"][i])
        assert formats.header_strength_text(peak[0], avg[0]) == str(gold["text"][i])
    rows = np.stack(S.golden_rows()[:34])                                    # and as one batch of 34 rows
    peak, avg = meter(rows)
    assert S.same_bits(peak, gold["peak"][:34]) and S.exact_bits(avg, gold["avg"][:34])


@pytest.mark.parametrize("length", [1, 4, 7, 8, 12, 124, 128, 132, 1020, 2044, 8188, 8192, 8193, 16380, 32764, 65532])
def test_row_meter_equals_numpy_on_random_rows(length):
    for n_rows in (1, 3, 1027):
        rows = S.random_rows(n_rows, length, 1000 * length + n_rows)
        want_peak, want_avg = S.meter_model(rows)
        peak, avg = meter(rows)
        bad = [r for r in range(n_rows) if not (S.same_bits(peak[r], want_peak[r]) and S.exact_bits(avg[r], want_avg[r]))]
        assert not bad, (length, n_rows, bad[:5], peak[bad[0]], want_peak[bad[0]], avg[bad[0]], want_avg[bad[0]])


def test_row_meter_tables_at_every_tree_regime():
    """The meter's tables come from the shared builder (pss_npsum.h: build_forest -> fill_plan): three random rows at every length
    below 300 (leaf and first uneven-split regimes, k_row_meter<64>) and at b - 9 .. b + 9 for b = 2048 (the switch to
    k_row_meter<256>), 8192, 16384 and 65536 (chunk edges), against np.max / np.mean; every failing length is reported."""
    from length_cases import REDUCE_LENGTHS
    lengths = [n for n in REDUCE_LENGTHS if n < 300] + [b + d for b in (2048, 8192, 16384, 65536) for d in range(-9, 10)]
    assert set(lengths) <= set(REDUCE_LENGTHS) and len(lengths) == 299 + 4 * 19
    bad = []
    for length in lengths:
        rows = S.random_rows(3, length, 31 * length)
        want_peak, want_avg = S.meter_model(rows)
        peak, avg = meter(rows)
        if not (S.same_bits(peak, want_peak) and S.exact_bits(avg, want_avg)):
            bad.append(length)
    assert not bad, bad


@pytest.mark.parametrize("length,cap", [(12, METER_WAVE_CAP_ROWS), (1020, METER_WAVE_CAP_ROWS), (2052, METER_GROUP_CAP_ROWS), (8193, METER_GROUP_CAP_ROWS)])
def test_row_meter_one_row_past_each_grid_cap(length, cap):
    n_rows = cap + 1
    rows = S.random_rows(n_rows, length, 77 + length)
    want_peak, want_avg = S.meter_model(rows)
    peak, avg = meter(rows)
    assert S.same_bits(peak, want_peak)
    assert S.exact_bits(avg, want_avg)


def test_row_meter_one_output_and_argument_errors():
    e = G.engine()
    rows = S.random_rows(5, 300, 9)
    want_peak, want_avg = S.meter_model(rows)
    d_rows, d_one = G.dev(rows), sentinel((5,), torch.float64)
    e.row_meter(d_rows, 5, 300, d_one, None)
    e.sync()
    assert S.same_bits(G.host(d_one), want_peak)
    e.row_meter(d_rows, 5, 300, None, d_one)
    e.sync()
    assert S.exact_bits(G.host(d_one), want_avg)
    e.row_meter(None, 0, 300, d_one, None)                                   # nothing to do
    for args in ((d_rows, 5, 300, None, None), (d_rows, 5, 0, d_one, None), (None, 5, 300, d_one, None), (d_rows, -1, 300, d_one, None)):
        with pytest.raises(Exception) as ei:
            e.row_meter(*args)
        assert getattr(ei.value, "code", None) == L.PSS_E_ARG


# ---- gate -----------------------------------------------------------------------------------------------------------------------------
def random_peaks(n, seed):
    rng = np.random.default_rng(seed)
    peak = 30.0 + 8.0 * rng.standard_normal(n)
    special = rng.integers(0, n, 300)
    peak[special[:100]] = np.nan
    peak[special[100:200]] = np.inf
    peak[special[200:]] = -np.inf
    return peak


def gate_on_device(peak, squelch, every, phase, held_in):
    e = G.engine()
    n = len(peak)
    d_open, d_idx = sentinel((n,), torch.uint8), sentinel((n,), torch.int32)
    n_open, held = e.squelch_gate(G.dev(peak), n, squelch, every, phase, held_in, d_open, d_idx)
    return G.host(d_open), G.host(d_idx), n_open, held


@pytest.mark.parametrize("every", [0, 1, 3, 7])
def test_gate_equals_the_host_gate_on_a_million_frames(every):
    peak = random_peaks(1_000_000, 5 + every)
    squelch = float(np.nanmedian(peak[np.isfinite(peak)]))
    for phase in range(max(every, 1)):
        for held_in in (0.0, 99.0, np.nan):
            want_open, want_n, want_held = h_squelch_gate(peak, squelch, every, phase, held_in)
            opened, idx, n_open, held = gate_on_device(peak, squelch, every, phase, held_in)
            assert np.array_equal(opened, want_open), (every, phase, held_in)
            assert n_open == want_n and S.exact_bits(held, want_held)
            assert np.array_equal(idx[:n_open], np.flatnonzero(want_open).astype(np.int32)), "open list: ascending and complete"
            assert np.all(idx[n_open:] == 0x7F7F7F7F), "nothing written past the count"
            if every:
                assert 0 < n_open < len(peak)


def test_gate_one_frame_past_the_grid_cap_and_small_batches():
    for n in (GATE_CAP_FRAMES + 1, 1, 63, 64, 65, 255, 256, 257):
        peak = random_peaks(max(n, 400), n)[:n]
        for every, phase in ((3, 1), (7, 6)):
            want_open, want_n, want_held = h_squelch_gate(peak, 30.0, every, phase, 31.0)
            opened, idx, n_open, held = gate_on_device(peak, 30.0, every, phase, 31.0)
            assert np.array_equal(opened, want_open) and n_open == want_n and S.exact_bits(held, want_held), (n, every)
            assert np.array_equal(idx[:n_open], np.flatnonzero(want_open).astype(np.int32)), (n, every)


def test_gate_golden_traces_no_frames_and_argument_errors():
    e = G.engine()
    gold = S.golden()
    for meta, want_open, want_held in zip(gold["trace_meta"], gold["trace_open"], gold["trace_held"]):
        opened, idx, n_open, held = gate_on_device(gold["peak"][:34], float(meta[0]), int(meta[1]), 0, 0.0)
        assert np.array_equal(opened, want_open) and n_open == int(want_open.sum()) and S.exact_bits(held, want_held[-1]), meta
    n_hand = int(gold["n_hand"])
    for meta, want_open, want_held in zip(gold["hand_trace_meta"], gold["hand_trace_open"], gold["hand_trace_held"]):
        opened, idx, n_open, held = gate_on_device(gold["peak"][35:35 + n_hand], float(meta[0]), int(meta[1]), 0, 0.0)
        assert np.array_equal(opened, want_open) and S.exact_bits(held, want_held[-1]), meta
    assert e.squelch_gate(None, 0, -60.0, 3, 2, 12.5) == (0, 12.5)
    d_peak = G.dev(np.zeros(8))
    assert e.squelch_gate(d_peak, 8, -60.0, 3, 0, 0.0) == (8, 0.0)           # both outputs optional
    for every, phase in ((-1, 0), (3, 3), (3, -1), (0, 1)):
        with pytest.raises(Exception) as ei:
            e.squelch_gate(d_peak, 8, -60.0, every, phase, 0.0)
        assert getattr(ei.value, "code", None) == L.PSS_E_ARG
    with pytest.raises(Exception):
        e.squelch_gate(None, 8, -60.0, 3, 0, 0.0)


# ---- gated demodulation ---------------------------------------------------------------------------------------------------------------
def frames_on_device(nf, n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    k = torch.arange(nf, device="cuda", dtype=torch.float64)[:, None]
    ph = 2 * np.pi * (0.01 + 0.0001 * (k % 97)) * t + 3.0 * torch.sin(2 * np.pi * t * (0.002 + 1e-5 * (k % 31)))
    amp = 0.05 + 0.9 * torch.rand((nf, 1), generator=gen, device="cuda", dtype=torch.float64)
    iq = torch.stack([amp * torch.cos(ph), amp * torch.sin(ph)], dim=-1).float()
    return (iq + 0.02 * torch.randn((nf, n, 2), generator=gen, device="cuda", dtype=torch.float32)).contiguous()


def audio_shape(mode, nf, n_out):
    return (nf, n_out, 2) if mode == L.MODE_WFM else (nf, n_out)


@pytest.mark.parametrize("mode", MODES)
def test_demod_gated_equals_the_open_frames_of_demod_signal(mode):
    e = G.engine()
    n = 1024
    n_out = e.demod_out_len(mode, n, FS)
    rng = np.random.default_rng(40 + mode)
    e.enable_timing(True)
    try:
        for nf in (1, 63, 64, 65, 1027, 3001):
            iq = frames_on_device(nf, n, 100 * mode + nf)
            pcm_all, au_all = G.empty((nf, n_out, 2), torch.int16), G.empty(audio_shape(mode, nf, n_out), torch.float64)
            e.demod_signal(mode, iq, nf, n, FS, pcm_all, au_all)
            e.sync()
            flags = {"all open": np.ones(nf, bool), "all closed": np.zeros(nf, bool), "last only": np.arange(nf) == nf - 1,
                     "random": rng.random(nf) < 0.5}
            for what, fl in flags.items():
                idx = np.flatnonzero(fl).astype(np.int32)
                k = len(idx)
                d_idx = G.dev(np.concatenate([idx, np.full(nf - k, -7, np.int32)]))
                pcm, au = sentinel((nf, n_out, 2), torch.int16), sentinel(audio_shape(mode, nf, n_out), torch.float64)
                e.kernel_times()
                e.demod_gated(mode, iq, nf, n, FS, d_idx, k, pcm, au)
                e.sync()
                times = e.kernel_times()
                sel = torch.from_numpy(idx.astype(np.int64)).cuda()
                assert torch.equal(pcm[:k], pcm_all[sel]), (mode, nf, what, "pcm")
                assert torch.equal(au[:k].view(torch.int64), au_all[sel].view(torch.int64)), (mode, nf, what, "audio")
                assert is_sentinel(pcm[k:]) and is_sentinel(au[k:]), (mode, nf, what, "written past the open frames")
                if k == 0:
                    assert times == {}, (what, times)                       # squelch closed: no kernel at all
                elif k == nf:
                    assert times and "k_gather_frames" not in times, (what, times)   # everything open: the demodulator reads d_iq itself
                else:
                    assert "k_gather_frames" in times and len(times) > 1, (what, times)
                # PCM alone, as the pipeline asks for it
                pcm2 = sentinel((nf, n_out, 2), torch.int16)
                e.demod_gated(mode, iq, nf, n, FS, d_idx, k, pcm2, None)
                e.sync()
                assert torch.equal(pcm2.view(torch.uint8), pcm.view(torch.uint8)), (mode, nf, what)
    finally:
        e.enable_timing(False)


def test_demod_gated_one_frame_past_the_gather_cap_odd_lengths_and_argument_errors():
    e = G.engine()
    mode, n = L.MODE_NFM, 256
    nf = GATHER_CAP_FRAMES + 40
    n_out = e.demod_out_len(mode, n, FS)
    iq = frames_on_device(nf, n, 8)
    pcm_all = G.empty((nf, n_out, 2), torch.int16)
    e.demod_signal(mode, iq, nf, n, FS, pcm_all, None)
    idx = np.delete(np.arange(nf, dtype=np.int32), np.arange(3, 3 + 39 * 50, 50))        # cap + 1 open frames
    assert len(idx) == GATHER_CAP_FRAMES + 1
    pcm = sentinel((nf, n_out, 2), torch.int16)
    e.demod_gated(mode, iq, nf, n, FS, G.dev(idx), len(idx), pcm, None)
    e.sync()
    assert torch.equal(pcm[:len(idx)], pcm_all[torch.from_numpy(idx.astype(np.int64)).cuda()]) and is_sentinel(pcm[len(idx):])
    # an odd frame length (8-byte copies) and a batch that starts 8 bytes off a 16-byte boundary
    for n2, shift in ((333, 0), (334, 1)):
        nf2 = 70
        base = frames_on_device(nf2 + 1, n2, n2).reshape(-1, 2)
        iq2 = base[shift:shift + nf2 * n2]
        n_out2 = e.demod_out_len(L.MODE_AM, n2, FS)
        all2, got2 = G.empty((nf2, n_out2, 2), torch.int16), sentinel((nf2, n_out2, 2), torch.int16)
        e.demod_signal(L.MODE_AM, iq2, nf2, n2, FS, all2, None)
        idx2 = np.arange(1, nf2, 3, dtype=np.int32)
        e.demod_gated(L.MODE_AM, iq2, nf2, n2, FS, G.dev(idx2), len(idx2), got2, None)
        e.sync()
        assert torch.equal(got2[:len(idx2)], all2[torch.from_numpy(idx2.astype(np.int64)).cuda()]), (n2, shift)
    d_idx = G.dev(np.arange(4, dtype=np.int32))
    for args in ((mode, iq, 4, n, FS, d_idx, 5, pcm, None), (mode, iq, 4, n, FS, d_idx, -1, pcm, None), (9, iq, 4, n, FS, d_idx, 2, pcm, None),
                 (mode, iq, 4, n, FS, None, 2, pcm, None), (mode, None, 4, n, FS, d_idx, 2, pcm, None),
                 (mode, iq.reshape(-1)[1:], 4, n, FS, d_idx, 2, pcm, None)):          # the last: not aligned to one sample, nothing to gather from
        with pytest.raises(Exception) as ei:
            e.demod_gated(*args)
        assert getattr(ei.value, "code", None) == L.PSS_E_ARG


# ---- the one-call step ----------------------------------------------------------------------------------------------------------------
def run_cells(mode, iq, nf, n, W, display, H, halo_lo=None, halo_hi=None, want64=True):
    e = G.engine()
    nh = 0 if halo_lo is None else len(halo_lo)
    n_out = e.demod_out_len(mode, n, FS)
    o = dict(db32=sentinel((nf, n), torch.float32), db64=sentinel((nf, n), torch.float64) if want64 else None,
             lo=sentinel((nh + nf,), torch.float64), hi=sentinel((nh + nf,), torch.float64),
             a=torch.zeros((nf, W), dtype=torch.int8, device="cuda"), b=torch.zeros((nf, W), dtype=torch.int8, device="cuda"),
             pcm=sentinel((nf, n_out, 2), torch.int16))
    if nh:
        o["lo"][:nh], o["hi"][:nh] = halo_lo, halo_hi
    return o, nh, n_out


def run_squelch(mode, iq, nf, n, W, display, H, squelch, every, phase, held_in, halo_lo=None, halo_hi=None, want64=True):
    e = G.engine()
    o, nh, n_out = run_cells(mode, iq, nf, n, W, display, H, halo_lo, halo_hi, want64)
    o.update(peak=sentinel((nf,), torch.float64), avg=sentinel((nf,), torch.float64), open=sentinel((nf,), torch.uint8))
    o["n_open"], o["held"] = e.frame_pipeline_squelch(mode, iq, nf, n, FS, o["db32"], o["db64"], o["lo"], o["hi"], W, o["a"], o["b"], o["pcm"], squelch,
                                                      o["peak"], o["avg"], o["open"], every=every, phase=phase, held_in=held_in, n_halo=nh,
                                                      display=display, disp_h=H)
    e.sync()
    return o


def reference_step(mode, iq, nf, n, W, display, H, halo_lo=None, halo_hi=None):
    """pss_frame_pipeline_cells (display results, PCM of every frame) and the post-processed rows pss_frame_pipeline_f64 materialises."""
    e = G.engine()
    c, nh, n_out = run_cells(mode, iq, nf, n, W, display, H, halo_lo, halo_hi)
    e.frame_pipeline_cells(mode, iq, nf, n, FS, c["db32"], c["db64"], c["lo"], c["hi"], W, c["a"], c["b"], c["pcm"], n_halo=nh, display=display, disp_h=H)
    f, _, _ = run_cells(mode, iq, nf, n, W, display, H, halo_lo, halo_hi)
    post = sentinel((nf, n - 4), torch.float64)
    e.frame_pipeline_f64(mode, iq, nf, n, FS, f["db64"], post, f["lo"], f["hi"], W, f["a"], f["b"], f["pcm"], n_halo=nh, display=display, disp_h=H)
    e.sync()
    return c, G.host(post)


def check_step(o, c, post, squelch, every, phase, held_in, tag):
    for k in ("db32", "db64", "lo", "hi", "a", "b"):
        if o[k] is not None:
            assert torch.equal(o[k].view(torch.uint8), c[k].view(torch.uint8)), (tag, k)
    want_peak, want_avg = S.meter_model(post)
    peak, avg = G.host(o["peak"]), G.host(o["avg"])
    assert S.same_bits(peak, want_peak), (tag, "peak")
    assert S.exact_bits(avg, want_avg), (tag, "avg")
    want_open, want_n, want_held = h_squelch_gate(peak, squelch, every, phase, held_in)
    assert np.array_equal(G.host(o["open"]), want_open), (tag, "open")
    assert o["n_open"] == want_n and S.exact_bits(o["held"], want_held), (tag, "count / carry")
    sel = torch.from_numpy(np.flatnonzero(want_open)).cuda()
    assert torch.equal(o["pcm"][:want_n], c["pcm"][sel]), (tag, "pcm of the open frames, compacted")
    assert is_sentinel(o["pcm"][want_n:]), (tag, "pcm past the open frames")
    return want_open


@pytest.mark.parametrize("mode", MODES)
def test_pipeline_squelch_equals_cells_meter_gate_and_gated_pcm(mode):
    n, W, H = 1024, 112, 36
    for nf, display in ((1, "waterfall"), (5, "persistence"), (1027, "waterfall"), (1027, "persistence")):
        iq = frames_on_device(nf, n, 7 * mode + nf)
        if nf >= 5:
            iq[1] = 0.0                      # a constant row: peak = avg = -100
            iq[3, 17, 0] = float("nan")      # every bin NaN: the peak is NaN and the gate stays closed while it is held
        torch.cuda.synchronize()
        c, post = reference_step(mode, iq, nf, n, W, display, H)
        fin = np.max(post, axis=1)
        squelch = float(np.median(fin[np.isfinite(fin)]))
        for s, every, phase, held_in, want64 in ((squelch, 3, 0, 0.0, True), (squelch, 1, 0, 99.0, False), (-60.0, 3, 2, 0.0, False),
                                                 (1e9, 7, 4, 0.0, True), (squelch, 0, 0, squelch, False)):
            o = run_squelch(mode, iq, nf, n, W, display, H, s, every, phase, held_in, want64=want64)
            opened = check_step(o, c, post, s, every, phase, held_in, (mode, nf, display, s, every))
            if s == -60.0 and nf == 1:
                assert opened.all()
            if s == 1e9:
                assert not opened.any()
        if nf == 1027 and display == "waterfall":           # two calls with the carry (held, phase, extremes halo) equal one
            one = run_squelch(mode, iq, nf, n, W, display, H, squelch, 3, 0, 0.0)
            cut = 500
            first = run_squelch(mode, iq[:cut], cut, n, W, display, H, squelch, 3, 0, 0.0)
            second = run_squelch(mode, iq[cut:], nf - cut, n, W, display, H, squelch, 3, cut % 3, first["held"], first["lo"][-30:].clone(),
                                 first["hi"][-30:].clone())
            assert first["n_open"] + second["n_open"] == one["n_open"] and S.exact_bits(second["held"], one["held"])
            for k in ("db32", "db64", "a", "b", "peak", "avg", "open"):
                assert torch.equal(torch.cat([first[k], second[k]]).view(torch.uint8), one[k].view(torch.uint8)), (mode, k, "two calls")
            assert torch.equal(torch.cat([first["lo"], second["lo"][30:]]).view(torch.uint8), one["lo"].view(torch.uint8))
            assert torch.equal(torch.cat([first["pcm"][:first["n_open"]], second["pcm"][:second["n_open"]]]), one["pcm"][:one["n_open"]])
            assert 0 < first["n_open"] < cut and 0 < second["n_open"] < nf - cut


def test_pipeline_squelch_other_lengths_no_frames_and_argument_errors():
    e = G.engine()
    W, H = 112, 36
    for nf, n in ((300, 512), (100, 2048), (9, 8192), (3, 32768)):
        iq = frames_on_device(nf, n, n)
        c, post = reference_step(L.MODE_NFM, iq, nf, n, W, "waterfall", H)
        squelch = float(np.median(np.max(post, axis=1)))
        for want64 in (True, False):
            o = run_squelch(L.MODE_NFM, iq, nf, n, W, "waterfall", H, squelch, 3, 1, 0.0, want64=want64)
            check_step(o, c, post, squelch, 3, 1, 0.0, (nf, n, want64))
    iq = frames_on_device(4, 1024, 1)
    assert e.frame_pipeline_squelch(L.MODE_NFM, iq, 0, 1024, FS, None, None, None, None, W, None, None, None, -60.0, None, held_in=4.5) == (0, 4.5)
    o, _, _ = run_cells(L.MODE_NFM, iq, 4, 1024, W, "waterfall", H)
    d_peak = G.empty((4,), torch.float64)
    ok = dict(every=3, phase=0)
    for kw, n_, peak_ in ((dict(every=-1, phase=0), 1024, d_peak), (dict(every=3, phase=3), 1024, d_peak), (dict(every=0, phase=1), 1024, d_peak),
                          (ok, 1000, d_peak), (ok, 1024, None)):
        with pytest.raises(Exception) as ei:
            e.frame_pipeline_squelch(L.MODE_NFM, iq, 4, n_, FS, o["db32"], None, o["lo"], o["hi"], W, o["a"], o["b"], o["pcm"], -60.0, peak_, **kw)
        assert getattr(ei.value, "code", None) == L.PSS_E_ARG, kw


def test_pipeline_squelch_reproduces_the_golden_traces_from_iq(golden):
    """caller_iq.npz's read buffers -> the open / closed traces the reference's loop produced on the rows of caller.npz (flags only: the
    device's dB values agree with the reference's to ~1e-12 dB, and the generator asserts that no golden peak lies within 1e-6 dB of a level)."""
    gold = S.golden()
    iq = G.dev(golden["caller_iq"]["iq"])
    nf, n, W, H = 34, 1024, 112, 36
    for meta, want_open, want_held in zip(gold["trace_meta"], gold["trace_open"], gold["trace_held"]):
        o = run_squelch(L.MODE_NFM, iq, nf, n, W, "waterfall", H, float(meta[0]), int(meta[1]), 0, 0.0, want64=False)
        assert np.array_equal(G.host(o["open"]), want_open), meta
        assert o["n_open"] == int(want_open.sum()) and abs(o["held"] - want_held[-1]) <= 1e-9, meta
    peak = G.host(o["peak"])
    assert np.max(np.abs(peak - gold["peak"][:34])) <= 1e-9      # the documented agreement of the rows themselves, not a criterion of the gate


def test_pipeline_squelch_full_batch_with_the_median_squelch():
    """65 536 x 1024 NFM, FM frames whose amplitude varies from frame to frame, the squelch at the median of the batch's peaks."""
    nf, n, W, H = 65536, 1024, 112, 36
    iq = frames_on_device(nf, n, 2025)
    c, post = reference_step(L.MODE_NFM, iq, nf, n, W, "waterfall", H)
    squelch = float(np.median(np.max(post, axis=1)))
    o = run_squelch(L.MODE_NFM, iq, nf, n, W, "waterfall", H, squelch, 3, 0, 0.0, want64=False)
    opened = check_step(o, c, post, squelch, 3, 0, 0.0, "full batch")
    assert opened.any() and not opened.all()
    runs = np.flatnonzero(np.diff(opened.astype(np.int8)))
    assert len(runs) > 100, "open and closed runs alternate along the batch"


# ---- recordings -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["NFM", "WFM", "AM"])
def test_demodulate_recording_with_squelch_picks_the_open_buffers(mode):
    nf, n = 40, 1024
    iq = G.host(frames_on_device(nf, n, 11)).reshape(-1, 2)
    samples = (iq[:, 0] + 1j * iq[:, 1]).astype(np.complex64)
    pcm_all = formats.demodulate_recording(samples, FS, mode, frame_len=n)
    assert pcm_all.shape[0] == nf
    _, _, peak0, _ = formats.demodulate_recording(samples, FS, mode, frame_len=n, squelch=-60)
    squelch = float(np.median(peak0))
    for every in (3, 1, 0):
        pcm, opened, peak, avg = formats.demodulate_recording(samples, FS, mode, frame_len=n, squelch=squelch, meter_every=every)
        want_open, _ = S.gate_model(peak, squelch, every)
        assert np.array_equal(opened, want_open) and S.exact_bits(peak, peak0)
        assert np.array_equal(pcm, pcm_all[want_open.astype(bool)]), (mode, every)
        chunked = formats.demodulate_recording(samples, FS, mode, frame_len=n, chunk_frames=7, squelch=squelch, meter_every=every)
        for a, b in zip(chunked, (pcm, opened, peak, avg)):
            assert np.array_equal(a.view(np.uint8) if a.dtype.kind == "f" else a, b.view(np.uint8) if b.dtype.kind == "f" else b), (mode, every, "chunks of 7")
        if every == 3:
            assert 0 < opened.sum() < nf
    pcm, opened, _, _ = formats.demodulate_recording(samples, FS, mode, frame_len=n, squelch=squelch, peak_power=1e9, meter_every=0)
    assert opened.all() and np.array_equal(pcm, pcm_all)

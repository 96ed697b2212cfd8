"""The FLEX kernels (k_flex_detect, pss_starts.h's k_starts_scan and k_starts_gather, k_flex_head, k_flex_keep, k_flex_walk, k_flex_compact)
against pss_h_flex_frames on every byte of every output, and formats.flex_recording end to end.  Buffers lie between NaNs, rows are strided
with NaNs in the gaps, and a sentinel sits behind max_frames.  The arrays are tests/flex_shapes.py's (tests/test_flex_shapes.py runs the
same ones on the CPU against the NumPy statement of the rules): every mode in both polarities at h = 1, 2, 12 and 64 (the cap), a frame that
ends with its row, sync codes, FIW and first data symbol across tile boundaries, one tile past the detect grid cap, a train of sync + FIW
stubs with more survivors than one pass of each list kernel and one step of the scan take, counts above max_frames, every sync_errors / fix
/ FIW sum / max_bad boundary, four-level symbols on their thresholds, equal scores, rows that must not run into each other, windows with
exactly their reach, non-finite samples.  The caps come from tests/flex_caps.py, where tests/test_flex_caps.py pins them to the source
lines.  A tile holds at most 4096 / 128 = 32 clean sync codes, so no tile built from valid codes has more survivors than a wavefront has
lanes; the survivors of the cases here fall into different wavefronts and passes of their tiles."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flex_cases as F
import flex_shapes as S
from bytes_util import same_bytes
from gpu_util import dev
from flex_caps import TILE   # pinned by tests/test_flex_caps.py
from pyspecsdr_amd import formats as FM
from pyspecsdr_amd.engine import Engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
WHAT = ("words", "fix", "fiw", "row", "pos", "meta", "score")
assert F.TILE == TILE


@pytest.fixture(scope="module")
def e():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    eng = Engine(0)
    yield eng
    eng.close()


def strided(rows, gap, fill=np.nan):
    """[R][n] -> a flat device tensor holding the rows `n + gap` apart between `fill`s, two elements of fill in front; -> (tensor, offset of
    row 0 in elements, stride)."""
    rows = np.ascontiguousarray(rows)
    r, n = rows.shape
    stride = n + gap
    wide = np.full(2 + r * stride + 2, fill, rows.dtype)
    for k in range(r):
        wide[2 + k * stride:2 + k * stride + n] = rows[k]
    return dev(wide), 2, stride


def buffers(room):
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    return (full((room, 4, 88), -7, torch.int32), full((room, 4, 88), SENTINEL, torch.uint8), full((room,), -7, torch.int32), full((room,), -7, torch.int32),
            full((room,), -7, torch.int64), full((room, 2), -7, torch.int32), full((room,), -7.0, torch.float32), full((2,), -7, torch.int32))


def on_device(e, y, h, sync_errors=2, fix=2, max_bad=0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, gap=3):
    """h_flex_frames' result from the device."""
    y = np.asarray(y, np.float32)
    rows = y[None, :] if y.ndim == 1 else y
    r, n = rows.shape
    n_row = buf_index0 + n if n_row is None else n_row
    s_end = n_row if s_end is None else s_end
    d_y, off, stride = strided(rows, gap)
    mf = 64 if max_frames is None else max_frames
    d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, d_count = buffers(mf + 3)
    e.flex_frames(d_y.data_ptr() + 4 * off, r, n, h, d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, d_count, mf, sync_errors=sync_errors, fix=fix,
                  max_bad=max_bad, y_stride=stride, buf_index0=buf_index0, n_row=n_row, s_begin=s_begin, s_end=s_end)
    e.sync()
    words, fx, fiw, rw, pos, meta, score, count = (t.cpu().numpy() for t in (d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, d_count))
    assert count[1] == -7
    k = min(int(count[0]), mf)
    assert np.all(words[k:] == -7) and np.all(fx[k:] == SENTINEL) and np.all(fiw[k:] == -7) and np.all(rw[k:] == -7) and np.all(pos[k:] == -7)
    assert np.all(meta[k:] == -7) and np.all(score[k:] == -7.0)
    return words[:k].view(np.uint32), fx[:k], fiw[:k].view(np.uint32), rw[:k], pos[:k], meta[:k].view(np.uint32), score[:k], int(count[0])


@pytest.fixture(scope="module")
def check(e):
    def run(y, h, max_frames=64, gap=3, numpy=None, **kw):
        """Device == twin on every byte -> the twin's result."""
        want = Engine.h_flex_frames(y, h, max_frames=max_frames, **kw)
        got = on_device(e, y, h, max_frames=max_frames, gap=gap, **kw)
        for g, w, what in zip(got[:7], want[:7], WHAT):
            assert same_bytes(g, w), (what, g, w)
        assert got[7] == want[7]
        return want
    return run


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_fixture_rows(check, name):
    mode, h, _, inverted, _ = F.CASES[name]
    r = check(F.case_row(name), h)
    assert r[7] == 1 and F.reported(FM.flex_messages(FM.flex_records(*r[:7]))) == F.expected(mode, F.MESSAGES)


@pytest.mark.parametrize("h", [1, 2, 12, 64])
def test_every_mode_both_polarities_and_the_rows_end(check, h):
    S.every_mode_both_polarities_and_the_rows_end(check, h)


@pytest.mark.parametrize("h", [1, 2, 12])
def test_sync_fiw_and_first_symbol_across_tile_boundaries(check, h):
    S.tile_boundaries(check, h)


def test_one_tile_past_the_detect_grid_cap(check):
    S.one_tile_past_the_detect_grid_cap(check)


def test_a_train_of_stubs_more_than_a_pass_of_every_list_kernel_and_a_step_of_the_scan(check):
    S.stub_train(check)


def test_sync_errors_against_marker_outer_code_and_mode_code(check):
    S.sync_errors_boundaries(check)


def test_fix_fiw_sum_and_max_bad_boundaries(check):
    S.fix_fiw_and_max_bad_boundaries(check)


def test_four_level_symbols_on_their_thresholds(check):
    S.four_level_thresholds(check)


def test_equal_scores_keep_the_earlier_start_and_a_neighbour_outside_the_window_drops(check):
    S.equal_scores_and_neighbours(check)


def test_rows_do_not_run_into_each_other(check):
    S.rows_do_not_run_into_each_other(check)


def test_windows_with_exactly_their_reach(check):
    S.windows_with_exactly_their_reach(check, same_bytes)


def test_non_finite_samples(check):
    S.non_finite_samples(check)


def test_a_refused_device_call_writes_nothing(e):
    from pyspecsdr_amd.engine import PssError
    h = 2
    n = 50 + F.FRAME_H * h + 20
    d_y = dev(F.frame_row(1, h, 50, n))
    d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, d_count = buffers(4)
    reach = "the buffer does not cover the window's reach (2 h - 1 starts either side, 5936 h samples forward)"
    for why, kw in (("n_rows outside [1, 2^20]", dict(n_rows=0)), ("h outside [1, 64]", dict(h=0)), ("h outside [1, 64]", dict(h=65)),
                    ("sync_errors outside [0, 3]", dict(sync_errors=4)), ("fix outside [0, 2]", dict(fix=-1)), ("max_bad outside [0, 352]", dict(max_bad=353)),
                    ("y_stride < n_buf", dict(y_stride=n - 1)), ("s_end < s_begin", dict(s_begin=5, s_end=4)),
                    ("the window does not lie inside the row", dict(s_end=n + 1)), (reach, dict(n_row=100000, s_end=900)),
                    (reach, dict(buf_index0=50, n_row=n + 50, s_begin=52, s_end=53)), ("max_frames < 0", dict(max_frames=-1)),
                    ("a misaligned pointer", dict(y=d_y.data_ptr() + 2)), ("null buffer", dict(count=None))):
        kw = dict(kw)
        args = dict(y=kw.pop("y", d_y), n_rows=kw.pop("n_rows", 1), max_frames=kw.pop("max_frames", 4), count=kw.pop("count", d_count), h=kw.pop("h", h))
        with pytest.raises(PssError, match=re.escape("pss_flex_frames: " + why)):
            e.flex_frames(args["y"], args["n_rows"], n, args["h"], d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, args["count"], args["max_frames"], **kw)
    e.sync()
    assert int(d_count.cpu()[0]) == -7 and bool((d_words == -7).all()) and bool((d_pos == -7).all()) and bool((d_fix == SENTINEL).all())
    assert bool((d_meta == -7).all()) and bool((d_fiw == -7).all())
    e.flex_frames(d_y, 1, n, h, d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, d_count, 4)      # and the same buffers are taken as they are
    e.sync()
    assert int(d_count.cpu()[0]) == 1 and int(d_pos.cpu()[0]) == 50


def test_recording_end_to_end(e):
    """Two channels at -50 and +50 kHz in a 240 kS/s capture, mode 0 and mode 3 inverted, 25 dB in the 38.4 kHz band: at that level the NumPy
    statement alone reports both frames with n_bad = 0 (tests/test_flex_golden.py asserts it on the CPU)."""
    fs = F.CAPTURE_FS
    assert Engine.pocsag_plan(fs) == (6, 24, 25)
    x = F.capture()
    channels = [150.0e6 + c[0] for c in F.CHANNELS]
    out = FM.flex_recording(x, fs, 150.0e6, channels)
    assert out["fs"] == 38400 and out["lines"] == F.capture_lines()
    for row, (_, mode, inverted, per_phase) in enumerate(F.CHANNELS):
        got = [m for m in out["messages"] if m["row"] == row]
        assert F.reported(got) == F.expected(mode, per_phase) and not any(m["damaged"] for m in got), (row, got)
        frames = [f for f in out["frames"] if f["row"] == row]
        assert len(frames) == 1 and frames[0]["mode"] == mode and frames[0]["inverted"] == inverted and frames[0]["n_bad"] == 0
        assert (frames[0]["cycle"], frames[0]["frame"]) == (7, 100)
    again = FM.flex_recording(x, fs, 150.0e6, channels, chunk_samples=77777)
    assert again["messages"] == out["messages"] and again["frames"] == out["frames"] and again["lines"] == out["lines"]

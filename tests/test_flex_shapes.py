"""The arrays of tests/test_gpu_flex.py (tests/flex_shapes.py) on the CPU: the host twin against the NumPy statement of the rules, and the
expectations each case states — no GPU.  A case that passes here and fails on the device is the kernels' fault alone."""
import numpy as np
import pytest

import flex_cases as F
import flex_shapes as S
from bytes_util import same_bytes
from pyspecsdr_amd.engine import Engine


def check(y, h, numpy=True, gap=None, **kw):
    kw.setdefault("max_frames", 64)
    want = Engine.h_flex_frames(y, h, **kw)
    if numpy:
        ref = F.numpy_frames(y, h, **kw)
        for g, w in zip(want[:7], ref[:7]):
            assert same_bytes(g, w), (g, w)
        assert want[7] == ref[7]
    return want


@pytest.mark.parametrize("h", [1, 2, 12, 64])
def test_every_mode_both_polarities_and_the_rows_end(h):
    S.every_mode_both_polarities_and_the_rows_end(check, h)


@pytest.mark.parametrize("h", [1, 2, 12])
def test_tile_boundaries(h):
    S.tile_boundaries(check, h)


def test_one_tile_past_the_detect_grid_cap():
    S.one_tile_past_the_detect_grid_cap(check)


def test_stub_train():
    S.stub_train(check)


def test_sync_errors_boundaries():
    S.sync_errors_boundaries(check)


def test_fix_fiw_and_max_bad_boundaries():
    S.fix_fiw_and_max_bad_boundaries(check)


def test_four_level_thresholds():
    S.four_level_thresholds(check)


def test_equal_scores_and_neighbours():
    S.equal_scores_and_neighbours(check)


def test_rows_do_not_run_into_each_other():
    S.rows_do_not_run_into_each_other(check)


def test_windows_with_exactly_their_reach():
    S.windows_with_exactly_their_reach(check, same_bytes)


def test_non_finite_samples():
    S.non_finite_samples(check)

"""tests/launch_caps.py against the launch code: every source line a row restates must still read as pinned (CPU only)."""
import os

import pytest

import launch_caps
from launch_caps import CAPS, RECEIVER_CAPS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyspecsdr_amd", "csrc")


def pinned(table, which, name, once=False):
    row = table[name]
    for fname, snippets in row.source.items():
        with open(os.path.join(CSRC, fname)) as f:
            src = f.read()
        for s in snippets:
            assert src.count(s) == 1 if once else s in src, (f"{row.entry} ({row.kernels}): {fname} no longer reads\n    {s}\n"
                              f"update tests/launch_caps.py ({which}'{name}') to the new launch grid")


@pytest.mark.parametrize("name", sorted(CAPS))
def test_pinned_launch_lines_are_in_the_source(name):
    pinned(CAPS, "", name)


@pytest.mark.parametrize("name", sorted(RECEIVER_CAPS))
def test_pinned_receiver_lines_are_in_the_source(name):
    """pss_rds.hip, pss_adsb.hip and pss_starts.h: the constants tests/test_gpu_rds.py, tests/test_gpu_adsb.py and (through tests/ais_caps.py)
    tests/test_gpu_ais.py import stand in these lines, each exactly once in its file."""
    pinned(RECEIVER_CAPS, "RECEIVER_CAPS ", name, once=True)


def test_receiver_caps_at_the_shapes_the_gpu_tests_run():
    c = launch_caps
    assert sorted(RECEIVER_CAPS) == ["adsb_detect", "adsb_list", "rds_bits", "rds_energy", "rds_front", "rds_groups", "starts_gather", "starts_scan"]
    assert (c.DETECT_TILE, c.DETECT_GRID_CAP, c.SCAN_STEP, c.LIST_PASS, c.FRONT_GRID_CAP, c.BITS_SCAN_PASS) == (4096, 1024, 4096, 8192, 2048, 256)
    assert RECEIVER_CAPS["rds_energy"].cover(1100) == 16384 and RECEIVER_CAPS["rds_energy"].cover(257 * 1024 + 17) == 16384 // 17
    assert RECEIVER_CAPS["adsb_list"].cover() == c.LIST_PASS and RECEIVER_CAPS["starts_scan"].cover() == c.SCAN_STEP
    assert (c.GATHER_GRID_CAP, c.ADSB_LIST_BYTES) == (2048, 9)
    assert RECEIVER_CAPS["starts_gather"].cover() == 2048 and RECEIVER_CAPS["rds_bits"].cover() == RECEIVER_CAPS["rds_groups"].cover() == 4096


def test_caps_at_the_lengths_the_gpu_tests_run():
    assert CAPS["ssb_c128"].cover(1000) == 16384                       # k_ssb_fir: one chunk per frame; k_finalize: 4194 frames
    assert CAPS["hilbert_exact_long"].cover(1 << 20) == 32 and CAPS["hilbert_exact_long"].cover(1 << 18) == 128
    assert CAPS["hilbert_exact_long"].cover(1 << 15) == 256
    assert [CAPS["hilbert_exact"].cover(n) for n in (256, 1024, 4096, 16384)] == [2048, 2048, 1024, 256]
    assert CAPS["wfm_q1"].cover(256) == 16384
    lengths = (256, 512, 1024, 2048, 4096)
    assert [CAPS["spectrum_f64_r16"].cover(n) for n in lengths] == [24576, 8192, 4096, 2048, 1024]   # launch_r16's caps: same Cfg, same grid
    assert [CAPS["hilbert_r16"].cover(n) for n in lengths] == [8192, 8192, 4096, 2048, 1024]
    assert [CAPS["spectrum_f64_plain"].cover(n) for n in (16, 1024, 4096, 8192)] == [8192, 8192, 2048, 2048]
    assert CAPS["spectrum_c128"].cover(4096) == 2048 and CAPS["post_f64"].cover(1024) == 2048
    assert [CAPS["hilbert_huge"].cover(1 << k) for k in (17, 18, 19, 20)] == [256, 128, 64, 32]

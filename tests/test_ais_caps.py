"""tests/ais_caps.py against pyspecsdr_amd/csrc/pss_ais.hip: the constants tests/test_gpu_ais.py imports stand in these source lines — no GPU."""
import os
import re

import ais_caps as C
import ais_cases as A

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyspecsdr_amd", "csrc", "pss_ais.hip")


def test_pinned_lines_are_in_the_source():
    lines = [ln.strip() for ln in open(SRC).read().splitlines()]
    for name, (value, line) in C.PINS.items():
        assert lines.count(line) == 1, (name, line)
        nums = [int(v) for v in re.findall(r"= (\d+)", line.split("//")[0])]
        prod = 1
        for v in nums:
            prod *= v
        assert prod == value, (name, nums, value)
    for line in C.LAUNCHES:
        assert lines.count(line) == 1, line


def test_the_cases_module_agrees():
    assert (A.TILE, A.FRONT_TILE) == (C.TILE, C.FRONT_TILE)
    assert C.LIST_PASS == 524288 and C.SCAN_STEP == 4096 and sorted(C.PINS) == ["DETECT_GRID_CAP", "DETECT_THREADS", "FRONT_GRID_CAP", "FRONT_THREADS",
                                                                               "FRONT_TILE", "LIST_GRID_CAP", "LIST_THREADS", "SCAN_STEP", "TILE"]

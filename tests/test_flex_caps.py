"""tests/flex_caps.py against pyspecsdr_amd/csrc/pss_flex.hip, pss_flex.h and pss_starts.h: the constants tests/test_gpu_flex.py imports
stand in these source lines — no GPU."""
import os
import re

import flex_caps as C
import flex_cases as F
import launch_caps as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyspecsdr_amd", "csrc")
SRC = os.path.join(CSRC, "pss_flex.hip")


def test_pinned_lines_are_in_the_source():
    lines = [ln.strip() for ln in open(SRC).read().splitlines()]
    for name, (value, line) in C.PINS.items():
        assert lines.count(line) == 1, (name, line)
    assert C.PINS["DETECT_LDS"][0] == L.DT_S + 126 * C.MAX_H
    assert 'static_assert(FD_V == 12160 && FD_V * sizeof(float) + 64 * sizeof(int) <= 64 * 1024, "the detect tile\'s LDS");' in lines
    for line in C.LINES:
        assert lines.count(line) == 1, line
    header = [ln.strip() for ln in open(os.path.join(CSRC, "pss_flex.h")).read().splitlines()]
    for line in C.HEADER_LINES:
        assert header.count(line) == 1, line


def test_the_shared_constants_come_from_the_start_list_header():
    src = open(SRC).read()
    assert '#include "pss_starts.h"' in src
    for name in ("DT_T", "DT_S", "DT_GRID_CAP", "SC_T", "SC_PER", "LS_T", "LS_GRID_CAP"):
        assert not re.search(rf"constexpr \w+ [^;]*\b{name} =", src), name
    shared = [ln.strip() for ln in open(os.path.join(CSRC, "pss_starts.h")).read().splitlines()]
    for line in (f"constexpr int DT_T = {L.DT_T};", f"constexpr int DT_S = {L.DT_S};", f"constexpr long DT_GRID_CAP = {L.DT_GRID_CAP};",
                 f"constexpr int LS_T = {L.LS_T};", f"constexpr long LS_GRID_CAP = {L.LS_GRID_CAP};"):
        assert sum(ln.startswith(line) for ln in shared) == 1, line


def test_the_cases_module_agrees():
    assert F.TILE == C.TILE
    assert (C.TILE, C.DETECT_GRID_CAP, C.LANE_PASS, C.GROUP_PASS, C.SCAN_STEP, C.LIST_BYTES) == (4096, 1024, 8192, 2048, 4096, 1796)
    assert sorted(C.PINS) == ["DETECT_LDS", "LANE_GRID_CAP"]

"""tests/ook_caps.py against pyspecsdr_amd/csrc/pss_ook.hip, pss_ook.h and pss_starts.h: the constants tests/test_gpu_ook.py and
tests/ook_cases.py size their cases by stand in these source lines — no GPU."""
import os
import re

import launch_caps as L
import ook_caps as C
import ook_cases as K

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyspecsdr_amd", "csrc")
SRC = os.path.join(CSRC, "pss_ook.hip")


def test_pinned_lines_are_in_the_source():
    lines = [ln.strip() for ln in open(SRC).read().splitlines()]
    for name, (value, line) in C.PINS.items():
        assert lines.count(line) == 1, (name, line)
    assert C.PINS["DETECT_HALO"][0] == C.MAX_R + C.MAX_P and C.PINS["DETECT_LDS"][0] == L.DT_S + C.MAX_R + C.MAX_P
    assert C.PINS["SCAN_PER"][0] == -(-(L.DT_S + C.MAX_R + 1) // L.DT_T)
    assert "static_assert(OD_M == 8257 && OD_PER == 9, \"the detect tile's LDS\");" in lines
    for line in C.LINES:
        assert lines.count(line) == 1, line
    header = [ln.strip() for ln in open(os.path.join(CSRC, "pss_ook.h")).read().splitlines()]
    for line in C.HEADER_LINES:
        assert header.count(line) == 1, line


def test_the_shared_constants_are_pinned_in_the_start_list_header():
    """The tile, the detect grid cap, the scan step and the list kernels' threads and grid cap: one line each in pss_starts.h, and pss_ook.hip
    takes them from there (it states none of them itself)."""
    shared = [ln.strip() for ln in open(os.path.join(CSRC, "pss_starts.h")).read().splitlines()]
    pinned = [s for row in C.SHARED_ROWS for s in L.RECEIVER_CAPS[row].source["pss_starts.h"]]
    for line in (f"constexpr int DT_T = {L.DT_T};", f"constexpr int DT_S = {L.DT_S};", f"constexpr long DT_GRID_CAP = {L.DT_GRID_CAP};",
                 f"constexpr int SC_T = {L.SC_T}, SC_PER = {L.SC_PER};", f"constexpr int LS_T = {L.LS_T};", f"constexpr long LS_GRID_CAP = {L.LS_GRID_CAP};",
                 "for (long b0 = 0; b0 < n; b0 += (long)SC_PER * SC_T) {"):
        assert line in pinned, line
        assert sum(ln.startswith(line) for ln in shared) == 1, line
    src = open(SRC).read()
    assert '#include "pss_starts.h"' in src
    for name in ("DT_T", "DT_S", "DT_GRID_CAP", "SC_T", "SC_PER", "LS_T", "LS_GRID_CAP"):
        assert not re.search(rf"constexpr \w+ [^;]*\b{name} =", src), name


def test_the_cases_module_agrees():
    assert (K.TILE, K.BLOCK, K.MAX_PULSES, K.MAX_BITS) == (C.TILE, C.BLOCK, C.MAX_PULSES, C.MAX_BITS)
    assert (C.TILE, C.DETECT_GRID_CAP, C.LANE_PASS, C.WAVE_PASS, C.SCAN_STEP) == (4096, 1024, 524288, 8192, 4096)
    assert (C.GATHER_GRID_CAP, C.EDGE_BYTES, C.MESSAGE_BYTES) == (2048, 25, 53)
    # the cases that are there for a cap reach past it
    cases = {c['name']: c for c in K.shape_cases()}
    assert cases['many_edges']['rows'].shape[1] > C.LANE_PASS + C.SCAN_STEP and cases['many_messages']['rows'].shape[1] // 3 > C.WAVE_PASS
    assert cases['grid_cap']['rows'].shape[1] == (C.DETECT_GRID_CAP + 1) * C.TILE and cases['rows4097']['rows'].shape[0] == 4097
    assert cases['alternate']['rows'].shape[1] >= 2 * C.TILE and cases['P65_R4096']['R'] == C.MAX_R and cases['P65_R4096']['P'] == C.MAX_P

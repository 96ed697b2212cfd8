"""tests/packet_caps.py against pyspecsdr_amd/csrc/pss_packet.hip and pss_starts.h: the constants tests/test_gpu_packet.py imports stand in
these source lines — no GPU."""
import os
import re

import launch_caps as L
import packet_caps as C
import packet_cases as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyspecsdr_amd", "csrc")
SRC = os.path.join(CSRC, "pss_packet.hip")


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


def test_the_shared_constants_are_pinned_in_the_start_list_header():
    """The tile, the detect grid cap, the scan step and the list kernels' threads and grid cap: one line each in pss_starts.h, and
    pss_packet.hip takes them from there (it states none of them itself)."""
    shared = [ln.strip() for ln in open(os.path.join(CSRC, "pss_starts.h")).read().splitlines()]
    pinned = [s for row in C.SHARED_ROWS for s in L.RECEIVER_CAPS[row].source["pss_starts.h"]]
    for line in (f"constexpr int DT_T = {L.DT_T};", f"constexpr int DT_S = {L.DT_S};", f"constexpr long DT_GRID_CAP = {L.DT_GRID_CAP};",
                 f"constexpr int SC_T = {L.SC_T}, SC_PER = {L.SC_PER};", f"constexpr int LS_T = {L.LS_T};", f"constexpr long LS_GRID_CAP = {L.LS_GRID_CAP};"):
        assert line in pinned, line
        assert sum(ln.startswith(line) for ln in shared) == 1, line
    src = open(SRC).read()
    assert '#include "pss_starts.h"' in src
    for name in ("DT_T", "DT_S", "DT_GRID_CAP", "SC_T", "SC_PER", "LS_T", "LS_GRID_CAP"):
        assert not re.search(rf"constexpr \w+ [^;]*\b{name} =", src), name


def test_the_header_states_the_reach_the_cases_use():
    head = open(os.path.join(CSRC, "pss_packet.h")).read()
    for line in ("constexpr int SPB = 22;", "constexpr int MAX_BYTES = 330;", "constexpr int REC_BYTES = 332;", "constexpr int NEAR = SPB;",
                 "static_assert(MAX_APPENDED == 2646 && LAST_K == 3183 && REACH == 73203, \"the reach of a walk\");"):
        assert head.count(line) == 1, line
    assert (P.SPB, P.BACK, P.HEAD, P.NEAR, P.LAST_K, P.REACH, P.MAX_BYTES, P.REC_BYTES) == (22, 22, 154, 22, 3183, 73203, 330, 332)


def test_the_cases_module_agrees():
    assert (P.TILE, P.FRONT_TILE) == (C.TILE, C.FRONT_TILE)
    assert (C.TILE, C.DETECT_GRID_CAP, C.LIST_PASS, C.SCAN_STEP) == (4096, 1024, 524288, 4096)
    assert (C.GATHER_GRID_CAP, C.LIST_BYTES) == (2048, 353)
    assert sorted(C.PINS) == ["FRONT_GRID_CAP", "FRONT_THREADS", "FRONT_TILE"]

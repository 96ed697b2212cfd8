"""The tile sizes, grid caps and list steps of pss_ais.hip that tests/test_gpu_ais.py sizes its cases by, restated from the source.

Each entry: the constant's value and the exact source line (pyspecsdr_amd/csrc/pss_ais.hip) it restates.  tests/test_ais_caps.py fails,
naming the line, as soon as a pinned line no longer reads as below: a GPU case sized by a stale constant would pass without walking the
loop it is there for."""

PINS = {
    "FRONT_TILE": (2048, "constexpr int FR_S = 2048;                       // outputs of a tile"),
    "FRONT_GRID_CAP": (2048, "constexpr long FR_GRID_CAP = 2048;               // workgroups of a launch: pairs past it are walked by a grid-stride loop"),
    "FRONT_THREADS": (256, "constexpr int FR_T = 256;                        // threads of a workgroup"),
    "TILE": (4096, "constexpr int DT_S = 4096;                       // start positions of a tile"),
    "DETECT_THREADS": (1024, "constexpr int DT_T = 1024;                       // threads of a workgroup: 16 wavefronts"),
    "DETECT_GRID_CAP": (1024, "constexpr long DT_GRID_CAP = 1024;               // workgroups of a launch: tiles past it are walked by a grid-stride loop"),
    "SCAN_STEP": (4096, "constexpr int SC_T = 1024, SC_PER = 4;           // the scan: 4096 counts a step"),
    "LIST_THREADS": (256, "constexpr int LS_T = 256;                        // the list kernels"),
    "LIST_GRID_CAP": (2048, "constexpr long LS_GRID_CAP = 2048;"),
}
# the launches the constants size, as the source states them
LAUNCHES = (
    "hipLaunchKernelGGL(k_ais_front, dim3((unsigned)(n_pairs < FR_GRID_CAP ? n_pairs : FR_GRID_CAP)), dim3(FR_T), 0, PSS_STREAM(ctx),",
    "hipLaunchKernelGGL(k_ais_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0,",
    "const dim3 lane_grid((unsigned)(lane_blocks < LS_GRID_CAP ? lane_blocks : LS_GRID_CAP));",
    "const dim3 wave_grid((unsigned)(wave_blocks < LS_GRID_CAP ? wave_blocks : LS_GRID_CAP));",
    "for (long b0 = 0; b0 < n; b0 += (long)SC_PER * SC_T) {",
)

FRONT_TILE, FRONT_GRID_CAP, TILE, DETECT_GRID_CAP = (PINS[k][0] for k in ("FRONT_TILE", "FRONT_GRID_CAP", "TILE", "DETECT_GRID_CAP"))
SCAN_STEP = PINS["SCAN_STEP"][0]
LIST_PASS = PINS["LIST_THREADS"][0] * PINS["LIST_GRID_CAP"][0]          # survivors one pass of a lane-per-survivor kernel covers: 524 288
WAVE = 64

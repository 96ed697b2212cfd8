"""The tile sizes, grid caps and list steps that tests/test_gpu_apt.py sizes its cases by, restated from the source.

pss_apt.hip's sync search states no launch constant of its own: the tile, the detect grid cap, the scan step and the list kernels' threads
and grid cap are those of the start list it shares with pss_adsb.hip, pss_ais.hip and pss_pocsag.hip (pss_starts.h); tests/launch_caps.py
pins them there and this module imports them.  What is pinned here are pss_apt.hip's own constants (the front's and the line gather's
grids, the detect tile's LDS) and the lines that USE them: the launches and the loops.  tests/test_apt_caps.py fails, naming the line, as
soon as a pinned line no longer reads as below: a GPU case sized by a stale constant would pass without walking the loop it is there for."""
import launch_caps as L

PINS = {
    "FRONT_THREADS": (1024, "constexpr int FR_T = 1024;                      // threads of a workgroup: 16 wavefronts beside the one LDS image of a CU"),
    "FRONT_GRID_CAP": (2048, "constexpr long FR_GRID_CAP = 2048;              // workgroups of a launch: pairs past it are walked by a grid-stride loop"),
    "DETECT_LDS": (4212, "constexpr int AD_Y = DT_S + REACH - 1;          // samples of a tile: 4212"),
    "LINES_THREADS": (256, "constexpr int LN_T = 256;"),
    "LINES_GRID_CAP": (1024, "constexpr long LN_GRID_CAP = 1024;              // workgroups of a launch: lines past it are walked by a grid-stride loop"),
}
# the launches and loops the constants size, as the source states them
LINES = (
    "hipLaunchKernelGGL(k_apt_front, dim3((unsigned)(n_pairs < FR_GRID_CAP ? n_pairs : FR_GRID_CAP)), dim3(FR_T), 0, PSS_STREAM(ctx),",
    "for (long p = blockIdx.x; p < n_pairs; p += gridDim.x) {",
    "hipLaunchKernelGGL(k_apt_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), d_env, e_stride, buf_index0,",
    "for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {",
    "const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;",
    "const dim3 lane_grid(PssStartList::list_grid(n_surv, LS_T));",
    "hipLaunchKernelGGL(k_apt_score, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_env, e_stride, buf_index0, surv, n_surv, tpr, w.e0, sync_errors, mism, score);",
    "hipLaunchKernelGGL(k_apt_keep, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, s_begin, s_end, mism, score, keep);",
    "hipLaunchKernelGGL(k_apt_emit, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, keep, rank, mism, score, max_syncs, d_row, d_pos, d_meta,",
    "hipLaunchKernelGGL(k_apt_lines, dim3((unsigned)(n_lines < LN_GRID_CAP ? n_lines : LN_GRID_CAP)), dim3(LN_T), 0, PSS_STREAM(ctx), d_env, n_rows, e_stride, n_row,",
    "for (long l = blockIdx.x; l < n_lines; l += gridDim.x) {",
    # the detect workgroup's way past a tile without survivors, tile_at's division, the rank cut, buffer 1's layout
    "if (__syncthreads_count(any) == 0) {",
    "row = tile / tpr;",
    "if (r >= max_syncs) continue;",
    "const size_t o_score = sizeof(long) * n, o_rank = o_score + sizeof(float) * n, o_mism = o_rank + sizeof(int) * n, o_keep = o_mism + n;",
    "r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + n, \"pss_apt_syncs list\");",
    # the front's own staging and task walk
    "const int q0 = tid / L, r0 = tid - q0 * L, dq = FR_T / L, dr = FR_T - dq * L;",
    "const int pos = r * ROW + q;",
    "const int G = (cnt + 63) >> 6;",
    "for (int t = wave; t < n_tasks; t += FR_WAVES) {",
)
# pss_ddc.h's lines behind front_tile
DDC_LINES = (
    "inline int tile_row(int M, int D, int T) { return (M - 1 + (T + D - 1) / D) | 1; }",
    "int M = PART_CAP / n_blocks(T);",
    "while (M > 1 && (long)D * tile_row(M, D, T) > STAGE_CAP) M--;",
)
# the header's lines the figures follow from
HEADER_LINES = (
    "constexpr int REACH = 117;                       // a start s reads env[s + 1 .. s + 115] and exists where s + 116 < n",
    "constexpr long NEAR = LINE_ENV / 2;              // 3120: the one-record rule's distance",
    "constexpr int LINE_WORDS = 2080, LINE_ENV = LINE_WORDS * ENV_SPW;",
)
# RECEIVER_CAPS rows of tests/launch_caps.py whose pss_starts.h lines state the shared constants
SHARED_ROWS = ("adsb_detect", "starts_scan", "starts_gather", "adsb_list")

TILE, DETECT_GRID_CAP, SCAN_STEP = L.DETECT_TILE, L.DETECT_GRID_CAP, L.SCAN_STEP
LANE_PASS = L.LS_T * L.LS_GRID_CAP          # survivors one pass of the lane-per-survivor kernels (k_apt_score, k_apt_keep, k_apt_emit) covers: 524 288
GATHER_GRID_CAP = L.GATHER_GRID_CAP         # tiles one pass of k_starts_gather covers: 2048
LIST_BYTES = 8 + 4 + 4 + 1 + 1              # buffer 1 of the start list, a survivor: the start, its score, rank, mismatches and keep flag
FRONT_WAVES = PINS["FRONT_THREADS"][0] // 64
FRONT_GRID_CAP = PINS["FRONT_GRID_CAP"][0]
LINES_GRID_CAP = PINS["LINES_GRID_CAP"][0]
WAVE = 64
REACH, NEAR, LINE_ENV, LINE_WORDS = 117, 3120, 6240, 2080
STAGE_CAP, PART_CAP, BLOCK = 8192, 1792, 64  # pss_ddc.h's tile, which the front shares


def front_tile(decim, n_taps):
    """pss_ddc.h's tile_outputs: the outputs of one (row, tile) pair of k_apt_front."""
    m = PART_CAP // -(-n_taps // BLOCK)
    while m > 1 and decim * ((m - 1 + -(-n_taps // decim)) | 1) > STAGE_CAP:
        m -= 1
    return m

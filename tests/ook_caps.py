"""The tile sizes, grid caps and list steps that tests/test_gpu_ook.py and tests/ook_cases.py size their cases by, restated from the source.

pss_ook.hip takes the tile, the detect grid cap, the scan step and the list kernels' threads and grid cap from the start list it shares with
the other receivers (pss_starts.h); tests/launch_caps.py pins them there and this module imports them.  What is pinned here are pss_ook.hip's
own constants and the lines that USE the shared ones: the detect tile's LDS, the launches and the loops.  tests/test_ook_caps.py fails, naming
the line, as soon as a pinned line no longer reads as below: a GPU case sized by a stale constant would pass without walking the loop it is
there for."""
import launch_caps as L

PINS = {
    "DETECT_HALO": (4161, "constexpr int OD_HALO = MAX_R + MAX_P;           // samples in front of a tile at the largest R and P: 4161"),
    "DETECT_LDS": (8257, "constexpr int OD_M = DT_S + OD_HALO;             // 8257 floats of m"),
    "SCAN_PER": (9, "constexpr int OD_PER = (DT_S + MAX_R + 1 + DT_T - 1) / DT_T;   // scan positions of a lane at the largest R: 9"),
    "LEVELS_T": (256, "constexpr int LV_T = 256;                        // threads of a levels workgroup"),
    "ENVELOPE_T": (256, "constexpr int EV_T = 256;                        // threads of an envelope workgroup"),
    "GRID_CAPS": ((4096, 65536), "constexpr long EV_GRID_CAP = 4096, LV_GRID_CAP = 65536;"),
}
# the launches and loops the constants size, as the source states them
LINES = (
    "hipLaunchKernelGGL(k_ook_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx),",
    "const dim3 lane_grid(PssStartList::list_grid(n_edges, LS_T)), wave_grid(PssStartList::list_grid((long)nm, LS_T / 64));",
    "hipLaunchKernelGGL(k_ook_heads, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), idx, n_edges, tpr, w.e0, t.off, tile_first, s_begin, s_end, gap_limit, epos, erow, head);",
    "hipLaunchKernelGGL(k_ook_list, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), head, rank, n_edges, heads);",
    "hipLaunchKernelGGL(k_ook_walk, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), epos, erow, n_edges, heads, n_heads, (long)nm, n_row, gap_limit, span, sl, pbits,",
    "hipLaunchKernelGGL(k_ook_emit, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), epos, erow, heads, n_heads, keep, rank2, pbits, pn_bits, pspan, pmeta, max_msgs,",
    "hipLaunchKernelGGL(k_ook_envelope, dim3((unsigned)(blocks < EV_GRID_CAP ? blocks : EV_GRID_CAP)), dim3(EV_T), 0, PSS_STREAM(ctx),",
    "hipLaunchKernelGGL(k_ook_levels, dim3((unsigned)(total < LV_GRID_CAP ? total : LV_GRID_CAP)), dim3(LV_T), 0, PSS_STREAM(ctx),",
    "for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {",
    "const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;",
    # the detect workgroup's two ways past a tile, the scan's share of a lane, the walk's steps, the rank cut, the room for messages
    "if (__syncthreads_count(high) == 0) {",
    "if (__syncthreads_count(any) == 0) {",
    "const int nq = cnt + R + 1, per = (nq + DT_T - 1) / DT_T;   // per <= OD_PER",
    "for (int step = 0; step < 2 * MAX_PULSES / 64; step++) {",
    "if (r >= max_msgs) continue;",
    "const size_t n = (size_t)n_edges, nm = (n + (size_t)n_rows) / 2 < n ? (n + (size_t)n_rows) / 2 : n;",
)
# the header's lines the figures follow from
HEADER_LINES = (
    "constexpr int MAX_P = 65, MAX_R = 4096;",
    "constexpr int BLOCK = 4096;                      // samples of a level block",
    "constexpr int MAX_PULSES = 1024, MAX_BITS = 256, BITS_BYTES = MAX_BITS / 8;",
)
# RECEIVER_CAPS rows of tests/launch_caps.py whose pss_starts.h lines state the shared constants
SHARED_ROWS = ("adsb_detect", "starts_scan", "starts_gather", "adsb_list")

TILE, DETECT_GRID_CAP, SCAN_STEP = L.DETECT_TILE, L.DETECT_GRID_CAP, L.SCAN_STEP
LANE_PASS = L.LS_T * L.LS_GRID_CAP          # edges one pass of the lane-per-edge kernels (k_ook_heads, k_ook_list) covers: 524 288
WAVE_PASS = (L.LS_T // 64) * L.LS_GRID_CAP  # messages one pass of the wavefront-per-message kernels (k_ook_walk, k_ook_emit) covers: 8192
GATHER_GRID_CAP = L.GATHER_GRID_CAP         # tiles one pass of k_starts_gather covers: 2048
EDGE_BYTES = 8 + 8 + 4 + 4 + 1              # buffer 1 of the start list, an edge: list index, position, row, rank, head flag
MESSAGE_BYTES = 4 + 4 + 4 + 4 + 4 + 32 + 1  # and a possible message (every other edge and one more a row): place in the list, n_bits, span, meta, rank, bits, keep flag
MAX_P, MAX_R, BLOCK, MAX_PULSES, MAX_BITS = 65, 4096, 4096, 1024, 256

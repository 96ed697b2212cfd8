"""The tile sizes, grid caps and list steps that tests/test_gpu_pocsag.py sizes its cases by, restated from the source.

pss_pocsag.hip states no launch constant of its own: the tile, the detect grid cap, the scan step and the list kernels' threads and grid cap
are those of the start list it shares with pss_adsb.hip and pss_ais.hip (pss_starts.h); tests/launch_caps.py pins them there and this module
imports them.  What is pinned here are pss_pocsag.hip's own lines that USE them: the detect tile's LDS, the launches and the loops.
tests/test_pocsag_caps.py fails, naming the line, as soon as a pinned line no longer reads as below: a GPU case sized by a stale constant
would pass without walking the loop it is there for."""
import launch_caps as L

PINS = {
    "DETECT_LDS": (8064, "constexpr int PD_Y = DT_S + HEAD_K * MAX_SPB;    // samples of a tile at the largest spb: 8064"),
}
# the launches and loops the constants size, as the source states them
LINES = (
    "hipLaunchKernelGGL(k_pocsag_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0,",
    "const dim3 lane_grid(PssStartList::list_grid(n_surv, LS_T)), wave_grid(PssStartList::list_grid(n_surv, LS_T / 64));",
    "hipLaunchKernelGGL(k_pocsag_walk, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0, surv, n_surv, tpr, w.e0, spb, sync_errors, fix, max_bad,",
    "hipLaunchKernelGGL(k_pocsag_keep, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, s_begin, s_end, spb, ok, score, cw, keep);",
    "hipLaunchKernelGGL(k_pocsag_emit, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, keep, rank, cw, fixb, meta, score, max_batches, d_cw,",
    "for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {",
    "const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;",
    # the detect workgroup's way past a tile without survivors, tile_at's division, the rank cut, buffer 1's layout
    "if (__syncthreads_count(any) == 0) {",
    "row = tile / tpr;",
    "if (r >= max_batches) continue;",
    "const size_t o_cw = sizeof(long) * n, o_meta = o_cw + sizeof(uint32_t) * N_CW * n, o_score = o_meta + sizeof(uint32_t) * n,",
    "o_rank = o_score + sizeof(float) * n, o_fix = o_rank + sizeof(int) * n, o_ok = o_fix + (size_t)N_CW * n, o_keep = o_ok + n;",
    "r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + n, \"pss_pocsag_batches list\");",
)
# the header's lines the LDS figure follows from
HEADER_LINES = (
    "constexpr int MIN_SPB = 2, MAX_SPB = 128;",
    "constexpr int HEAD_K = SYNC_BITS - 1;            // 31: the candidate test's last strobe",
)
# RECEIVER_CAPS rows of tests/launch_caps.py whose pss_starts.h lines state the shared constants
SHARED_ROWS = ("adsb_detect", "starts_scan", "starts_gather", "adsb_list")

TILE, DETECT_GRID_CAP, SCAN_STEP = L.DETECT_TILE, L.DETECT_GRID_CAP, L.SCAN_STEP
LANE_PASS = L.LS_T * L.LS_GRID_CAP          # survivors one pass of the lane-per-survivor kernel (k_pocsag_keep) covers: 524 288
WAVE_PASS = (L.LS_T // 64) * L.LS_GRID_CAP  # survivors one pass of the wavefront-per-survivor kernels (k_pocsag_walk, k_pocsag_emit) covers: 8192
GATHER_GRID_CAP = L.GATHER_GRID_CAP         # tiles one pass of k_starts_gather covers: 2048
LIST_BYTES = 8 + 4 * 16 + 4 + 4 + 4 + 16 + 1 + 1   # buffer 1 of the start list, a survivor: the start, 16 codewords, meta, score, rank, 16 fix bytes, ok, keep
WAVE = 64
MAX_SPB = 128

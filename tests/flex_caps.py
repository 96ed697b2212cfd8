"""The tile sizes, grid caps and list steps that tests/test_gpu_flex.py sizes its cases by, restated from the source.

The tile, the detect grid cap, the scan step and the list kernels' threads and workgroup-grid cap are those of the start list
(pss_starts.h); tests/launch_caps.py pins them there and this module imports them.  pss_flex.hip states two launch constants of its own:
the detect tile's LDS and the grid cap of its two lane-per-survivor kernels.  What is pinned here are those and the lines that USE the
shared ones.  tests/test_flex_caps.py fails, naming the line, as soon as a pinned line no longer reads as below."""
import launch_caps as L

PINS = {
    "DETECT_LDS": (12160, "constexpr int FD_V = DT_S + HEAD_V * MAX_H;      // values of a tile at the largest h: 12160"),
    "LANE_GRID_CAP": (32, "constexpr long FL_LANE_GRID_CAP = 32;            // workgroups of k_flex_head and k_flex_keep: 8192 survivors a pass (about 340 frames' at h = 12)"),
}
LINES = (
    "hipLaunchKernelGGL(k_flex_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0,",
    "const long lane_blocks = (n_surv + LS_T - 1) / LS_T;",
    "const dim3 lane_grid((unsigned)(lane_blocks < FL_LANE_GRID_CAP ? lane_blocks : FL_LANE_GRID_CAP)), group_grid(PssStartList::list_grid(n_surv, 1));",
    "hipLaunchKernelGGL(k_flex_head, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0, n_surv, tpr, w.e0, h, sync_errors, fix, L);",
    "hipLaunchKernelGGL(k_flex_keep, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), n_surv, tpr, w.e0, s_begin, s_end, h, L);",
    "hipLaunchKernelGGL(k_flex_walk, group_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0, n_surv, tpr, w.e0, h, fix, max_bad, L);",
    "hipLaunchKernelGGL(k_flex_compact, group_grid, dim3(LS_T), 0, PSS_STREAM(ctx), n_surv, tpr, w.e0, L, max_frames, d_words, d_fix, d_fiw, d_row, d_pos,",
    "for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {",
    "const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;",
    "if (__syncthreads_count(any) == 0) {",
    "row = tile / tpr;",
    "if (r >= max_frames) continue;",
    "static_assert(LS_T == 256, \"a block of 256 symbols is one symbol a thread, and a wavefront's ballot one byte of each of its words\");",
    "r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_fix + (size_t)REC_W * n, \"pss_flex_frames list\");",
)
# the header's lines the LDS figure and the reach follow from
HEADER_LINES = (
    "constexpr int MIN_H = 1, MAX_H = 64;",
    "constexpr int HEAD_V = 2 * (SYNC_BITS - 1);      // 126: the last sync value's offset in units of h",
    "constexpr long FRAME_H = 2l * DATA_BIT + 2l * N_SYM;   // 5936: the samples of a frame in units of h",
)

TILE, DETECT_GRID_CAP, SCAN_STEP = L.DETECT_TILE, L.DETECT_GRID_CAP, L.SCAN_STEP
LANE_PASS = L.LS_T * PINS["LANE_GRID_CAP"][0]   # survivors one pass of k_flex_head and k_flex_keep covers: 8192
GROUP_PASS = L.LS_GRID_CAP                       # survivors one pass of k_flex_walk and k_flex_compact covers: 2048
LIST_BYTES = 8 + 6 * 4 + 4 * 352 + 4 + 352       # buffer 1 of the start list, a survivor
MAX_H = 64

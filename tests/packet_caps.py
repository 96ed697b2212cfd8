"""The tile sizes, grid caps and list steps that tests/test_gpu_packet.py sizes its cases by, restated from the source.

k_packet_front's constants are pss_packet.hip's own and are pinned here: each entry gives the constant's value and the exact source line
(pyspecsdr_amd/csrc/pss_packet.hip) it restates.  The tile, the detect grid cap, the scan step and the list kernels' threads and grid cap
are those of the start list pss_packet.hip shares with the other receivers (pss_starts.h): tests/launch_caps.py pins them there and this
module imports them.  tests/test_packet_caps.py fails, naming the line, as soon as a pinned line no longer reads as below: a GPU case sized
by a stale constant would pass without walking the loop it is there for."""
import launch_caps as L

PINS = {
    "FRONT_TILE": (2048, "constexpr int FR_S = 2048;                       // outputs of a tile"),
    "FRONT_GRID_CAP": (2048, "constexpr long FR_GRID_CAP = 2048;               // workgroups of a launch: pairs past it are walked by a grid-stride loop"),
    "FRONT_THREADS": (256, "constexpr int FR_T = 256;                        // threads of a workgroup"),
}
# the launches the constants size, as the source states them
LAUNCHES = (
    "hipLaunchKernelGGL(k_packet_front, dim3((unsigned)(n_pairs < FR_GRID_CAP ? n_pairs : FR_GRID_CAP)), dim3(FR_T), 0, PSS_STREAM(ctx),",
    "hipLaunchKernelGGL(k_packet_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), dev_z, z_stride, buf_index0,",
    "const dim3 lane_grid(PssStartList::list_grid(n_surv, LS_T)), wave_grid(PssStartList::list_grid(n_surv, LS_T / 64));",
    # the detect workgroup's way past a tile without survivors, tile_at's division, the record's words, buffer 1's layout
    "if (__syncthreads_count(any) == 0) {",
    "row = tile / tpr;",
    "constexpr int REC_WORDS = REC_BYTES / 4;         // a survivor's payload in scratch: 83 words",
    "const size_t o_words = sizeof(long) * n, o_len = o_words + sizeof(uint32_t) * REC_WORDS * n, o_score = o_len + sizeof(int) * n,",
    "o_rank = o_score + sizeof(float) * n, o_keep = o_rank + sizeof(int) * n;",
    "r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + n, \"pss_packet_frames list\");",
)
# RECEIVER_CAPS rows of tests/launch_caps.py whose pss_starts.h lines state the shared constants
SHARED_ROWS = ("adsb_detect", "starts_scan", "starts_gather", "adsb_list")

FRONT_TILE, FRONT_GRID_CAP = PINS["FRONT_TILE"][0], PINS["FRONT_GRID_CAP"][0]
TILE, DETECT_GRID_CAP, SCAN_STEP = L.DETECT_TILE, L.DETECT_GRID_CAP, L.SCAN_STEP
LIST_PASS = L.LS_T * L.LS_GRID_CAP          # survivors one pass of a lane-per-survivor kernel covers: 524 288
GATHER_GRID_CAP = L.GATHER_GRID_CAP         # tiles one pass of k_starts_gather covers: 2048
LIST_BYTES = 8 + 4 * 83 + 4 + 4 + 4 + 1     # buffer 1 of the start list, a survivor: the start, 83 record words, length, score, rank, keep
WAVE = 64

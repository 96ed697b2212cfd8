"""The capped launch grids of the batched entry points outside compute_fft and the bench.py paths, restated from the launch code.

Each row gives the entry point, its kernel(s), a function (n, options) -> how many frames (rows, bits or elements: `unit`) one pass
of the grid covers, and the exact source lines (pyspecsdr_amd/csrc) the function restates.  Past that count a workgroup (or thread)
walks its grid-stride loop a second time; tests/test_gpu_grid_caps.py runs every row one step past it and checks every output
against the CPU oracle, and tests/test_launch_caps.py fails, naming the line, as soon as a pinned line no longer reads as below.
Where a row has several capped kernels, `cover` is the largest of their counts, so that a batch past it walks every one of them.

Not rows here:
- the compute_fft families, with test_gpu_spectrum_accuracy.py's GRID_CAPS, and the bench.py paths of test_gpu_full_batch.py;
- k_slide_extremes (its cap covers 1 M frames) and k_rows_f64_to_f32 (already walked at 65 536 x 1024 frames).
hilbert_long's own `grid` sizes nothing at 2^17 .. 2^20 samples (there the scratch is [n_rows][N]); those rows go through the Bluestein
pass kernels k_huge_p1_g / k_huge_p2_g with the Hilbert loaders and stores (row "hilbert_huge").
"""
from collections import namedtuple

Cap = namedtuple("Cap", "entry kernels unit cover source")

HIL_EXACT_LONG_SCRATCH = 1 << 30          # hilbert_pf_long: at most 1 GiB of per-workgroup scratch


def r16_cfg(n):
    """pss_r16::Cfg<log2(n / 256)> (pss_fft_r16.h, product layout): threads per frame T, frames per workgroup FPW, EX and TW2 in
    complex elements."""
    r3 = n // 256
    T = 16 * r3
    e1 = T + (4 if r3 == 1 else r3 % 16)
    e2 = 256 + (2 if r3 == 1 else 8 // r3 if r3 <= 8 else 1)
    return T, 256 // T, max(16 * e1, r3 * e2), r3 * 17


def r16_f64_cap(n):
    """launch_r16_f64: LDS-limited per_cu capped by vgpr_cap, 256 * per_cu * 2 workgroups of fpw frames (256 points: split, float64
    exchange; 2048 points: one frame per workgroup)."""
    T, FPW, EX, TW2 = r16_cfg(n)
    split, fpw = n == 256, (1 if n == 2048 else FPW)
    lds = FPW * EX * 8 + TW2 * 16 if split else fpw * EX * 16 + TW2 * 16
    per_cu = max(1, min((160 * 1024) // (lds + 256), (4 if split else 2) * 256 // (fpw * T)))
    return 256 * per_cu * 2 * fpw


def hil_r16_cap(n):
    """HIL_R16: per_cu = 160 KiB / (Cfg::LDS + 256) capped at 2; 256 * per_cu * 2 workgroups of FPW rows."""
    T, FPW, EX, TW2 = r16_cfg(n)
    per_cu = min(2, (160 * 1024) // (FPW * EX * 16 + TW2 * 16 + 256))
    return 256 * per_cu * 2 * FPW


def generic_cap(n):
    """The plain LDS transform (k_spectrum) behind grid_for: 2^min(log2 n, LOG_NSUB_MAX = 12) complex doubles of LDS, per_cu at most 8,
    256 * per_cu * 4 workgroups of one frame."""
    lds = 16 * min(n, 4096)
    return 256 * min(8, (160 * 1024) // (lds + 64)) * 4


def huge_cap(n):
    """Rows of 2^17 .. 2^20 samples (NS = n / 256 columns): k_huge_p1_g on at most 8192 workgroups of 16 columns, k_huge_p2_g on at
    most 8192 workgroups of Cfg<log2(NS / 256)>::FPW of the 256 sub-rows per row."""
    ns = n >> 8
    return max(8192 * 16 // ns, 8192 * r16_cfg(ns)[1] // 256)


R16_CFG = {"pss_fft_r16.h": [
    "static constexpr int T = 16 * R3;",
    "static constexpr int FPW = 256 / T;",
    "static constexpr int E1_STRIDE = T + (R3 == 1 ? 4 : R3 % 16);",
    "static constexpr int E2_STRIDE = 256 + (R3 == 1 ? 2 : R3 <= 8 ? 8 / R3 : 1);",
    "static constexpr int TW2S = 17;",
    "static constexpr int TW2 = R3 * TW2S;",
    "static constexpr int EX = (16 * E1_STRIDE > R3 * E2_STRIDE) ? 16 * E1_STRIDE : R3 * E2_STRIDE;",
    "static constexpr size_t LDS = (size_t)FPW * EX * sizeof(double2) + (size_t)TW2 * sizeof(double2);",
]}


def _pf_cap(n):
    """k_hilbert_pf: per_cu = 160 KiB / (n float64 of LDS + 512) clamped to 1 .. 8; 256 * per_cu workgroups of one row each."""
    return 256 * max(1, min(8, (160 * 1024) // (n * 8 + 512)))


CAPS = {
    "classify": Cap(
        "pss_classify (n >= 1024)", "k_cls_modidx, k_cls_welch", "frames", lambda n, o=None: 16384,
        {"pss_demod.hip": [
            "const int np = n < CLS_NP ? n : CLS_NP;",
            "const long g = n_frames < 16384 ? n_frames : 16384;\n    PssTimeScope timed(ctx);\n    pss_kernel_begin(ctx, \"k_cls_modidx\");",
            "hipLaunchKernelGGL(k_cls_modidx, dim3((unsigned)g), dim3(256), lds1,",
            "hipLaunchKernelGGL(k_cls_welch, dim3((unsigned)g), dim3(256), lds2,",
        ]}),
    "classify_short": Cap(
        "pss_classify (n < 1024)", "k_cls_modidx, k_cls_welch_short", "frames", lambda n, o=None: 16384,
        {"pss_demod.hip": [
            "const long g = n_frames < 16384 ? n_frames : 16384;\n    PssTimeScope timed(ctx);\n    pss_kernel_begin(ctx, \"k_cls_modidx\");",
            "hipLaunchKernelGGL(k_cls_welch_short, dim3((unsigned)g), dim3(256), lds3,",
        ]}),
    "morse": Cap(
        "pss_morse_edges", "k_morse_edges", "frames", lambda n, o=None: 16384,
        {"pss_demod.hip": [
            "const long g = n_frames < 16384 ? n_frames : 16384;\n    pss_kernel_begin(ctx, \"k_morse_edges\");",
            "hipLaunchKernelGGL(k_morse_edges, dim3((unsigned)g), dim3(256), 0,",
        ]}),
    "afsk": Cap(
        "pss_afsk_bits", "k_afsk_bits", "bits", lambda n, o=None: 4096 * 256,
        {"pss_demod.hip": [
            "const long total = n_rows * n_bits;",
            "hipLaunchKernelGGL(k_afsk_bits, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256), 0,",
        ]}),
    "row_normalise": Cap(
        "pss_row_normalise", "k_row_normalise", "rows", lambda n, o=None: 8192,
        {"pss_demod.hip": [
            "hipLaunchKernelGGL(k_row_normalise, dim3((unsigned)(n_rows < 8192 ? n_rows : 8192)), dim3(256), 0,",
        ]}),
    "am_c128": Cap(
        "pss_demod_am_c128", "k_am_env_c128, k_norm_rows_f64", "frames", lambda n, o=None: 4096,
        {"pss_demod.hip": [
            "hipLaunchKernelGGL(k_am_env_c128, dim3((unsigned)(n_frames < 4096 ? n_frames : 4096)), dim3(256), 0,",
            "hipLaunchKernelGGL(k_norm_rows_f64, dim3((unsigned)(n_frames < 4096 ? n_frames : 4096)), dim3(256), 0,",
        ]}),
    "power_c128": Cap(
        "pss_mean_power_c128", "k_power_c128", "frames", lambda n, o=None: 4096,
        {"pss_demod.hip": [
            "hipLaunchKernelGGL(k_power_c128, dim3((unsigned)(n_frames < 4096 ? n_frames : 4096)), dim3(256), 0,",
        ]}),
    # frames that are not a power of two (no hilbert() round trip): k_ssb_fir walks n_frames * cpf chunks of 1024 samples on at most
    # 16384 workgroups, k_finalize n_frames * n samples on at most 16384 x 256 threads
    "ssb_c128": Cap(
        "pss_demod_ssb_c128 (n not a power of two)", "k_ssb_fir<double2>, k_finalize", "frames",
        lambda n, o=None: max(16384 // ((n + 1023) // 1024), 16384 * 256 // n),
        {"pss_demod.hip": [
            "const int cpf = (n + 1023) / 1024;\n    long total = n_frames * cpf;\n    long g = total < 16384 ? total : 16384;",
            "hipLaunchKernelGGL(k_ssb_fir<double2>, dim3((unsigned)g), dim3(TPB), 0,",
            "size_t tot = (size_t)n_frames * n;\n    size_t g2 = (tot + TPB - 1) / TPB;\n    if (g2 > 16384) g2 = 16384;\n"
            "    pss_kernel_begin(ctx, \"k_finalize\");\n    hipLaunchKernelGGL(k_finalize, dim3((unsigned)g2), dim3(TPB), 0, PSS_STREAM(ctx), Yf,",
            "constexpr int TPB = 256;",
        ]}),
    "np_f32": Cap(
        "pss_np_f32", "k_np_f32", "elements", lambda n, o=None: 4096 * 256,
        {"pss_demod.hip": [
            "const long blocks = (n + 255) / 256;",
            "hipLaunchKernelGGL(k_np_f32, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,",
            "for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {",
        ]}),
    "spectrogram": Cap(
        "pss_spectrogram_cells / pss_spectrogram_cells_f64", "k_spectrogram<float>, k_spectrogram<double>", "rows", lambda n, o=None: 4096,
        {"pss_fft.hip": [
            "hipLaunchKernelGGL(k_spectrogram<T>, dim3((unsigned)(n_rows < 4096 ? n_rows : 4096)), dim3(len <= 4096 ? 256 : 1024), 0,",
        ]}),
    "vector": Cap(
        "pss_vector_cells", "k_vector", "elements", lambda n, o=None: 1024 * 256,
        {"pss_fft.hip": [
            "hipLaunchKernelGGL(k_vector, dim3((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0,",
            "for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {",
        ]}),
    "scan": Cap(
        "pss_scan / pss_scan_threshold (n not a power of two)", "k_scan_reduce", "rows", lambda n, o=None: 16384,
        {"pss_fft.hip": [
            "hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)(n_rows < 16384 ? n_rows : 16384)), dim3(256), 0,",
        ]}),
    # N = 32768 / 65536: k_big_g<3> / <4> on `grid` workgroups, each with a pre-pass scratch row S[blockIdx.x] reused for every row it owns
    "hilbert_long": Cap(
        "pss_hilbert (32768, 65536 samples)", "k_big_g<3>, k_big_g<4>", "rows", lambda n, o=None: 512,
        {"pss_fft.hip": [
            "const int grid = (int)(n_rows < 512 ? n_rows : 512);",
            "szS = (n <= 65536 ? (size_t)grid : (size_t)n_rows) * N * sizeof(double2);",
            "r = big_pass<3>(ctx, lx, sz, tw, n_rows, S, grid);",
            "r = big_pass<4>(ctx, lx, sz, tw, n_rows, S, grid);",
        ]}),
    "hilbert_exact_long": Cap(
        "pss_hilbert, option hilbert_exact (32768 .. 2^20 samples)", "k_hilbert_pf_long", "rows",
        lambda n, o=None: max(1, min(256, HIL_EXACT_LONG_SCRATCH // (n * 2 * 16))),
        {"pss_fft.hip": [
            "const size_t per_wg = (size_t)n * 2 * sizeof(double2);",
            "long grid = (long)(((size_t)1 << 30) / per_wg);",
            "grid = grid < 1 ? 1 : (grid > 256 ? 256 : grid);",
            "hipLaunchKernelGGL(pss_pf::k_hilbert_pf_long, dim3((unsigned)grid), dim3(1024), 0,",
        ]}),
    "hilbert_exact": Cap(
        "pss_hilbert, option hilbert_exact (256 .. 16384 samples)", "k_hilbert_pf", "rows", lambda n, o=None: _pf_cap(n),
        {"pss_fft.hip": [
            "const size_t lds = (size_t)n * sizeof(double);\n    const int ept = n >= 1024 ? 16 : 8;",
            "int per_cu = (int)((160 * 1024) / (lds + 512));\n    per_cu = per_cu > 8 ? 8 : (per_cu < 1 ? 1 : per_cu);\n    const long cap = 256L * per_cu;",
            "hipLaunchKernelGGL(kern, dim3((unsigned)(n_rows < cap ? n_rows : cap)), dim3(n / ept), lds,",
        ]}),
    "hilbert_xl": Cap(
        "pss_hilbert (8192, 16384 samples)", "k_hilbert_xl<1>, k_hilbert_xl<2>", "rows", lambda n, o=None: 512 if n == 8192 else 256,
        {"pss_fft.hip": [
            "hipLaunchKernelGGL(kern, dim3((unsigned)(n_rows < cap ? n_rows : cap)), dim3(threads), lds, PSS_STREAM(ctx), d_x, d_out, tw, n_rows,\n"
            "                           d_maxbits, reinterpret_cast<unsigned *>(d_pcm), out_mode);",
            "case 8192: return go_xl(pss_hil::k_hilbert_xl<1>, pss_xl::CfgX<1>::LDS, 512, 512);",
            "default: return go_xl(pss_hil::k_hilbert_xl<2>, pss_xl::CfgX<2>::LDS, 1024, 256);",
        ]}),
    "spectrum_f64_r16": Cap(
        "pss_spectrum_db_f64 (256 .. 4096 points)", "k_spectrum_r16<0..4, D64>", "frames", lambda n, o=None: r16_f64_cap(n),
        dict(R16_CFG, **{"pss_fft.hip": [
            "case 256: return launch_r16_f64<0>(ctx, d_iq, n_frames, d_db, tw, win);",
            "case 4096: return launch_r16_f64<4>(ctx, d_iq, n_frames, d_db, tw, win);",
            "constexpr bool split = LOG_R3 == 0, prefetch = LOG_R3 >= 1, one = LOG_R3 == 3;\n"
            "    auto kern = pss_r16::k_spectrum_r16<LOG_R3, false, split, prefetch, true, one, true>;\n"
            "    const int fpw = one ? 1 : C::FPW;\n"
            "    const size_t lds = split ? (size_t)C::FPW * C::EX * sizeof(double) + (size_t)C::TW2 * sizeof(double2)\n"
            "                             : (size_t)fpw * C::EX * sizeof(double2) + (size_t)C::TW2 * sizeof(double2);",
            "    const long groups = (n_frames + fpw - 1) / fpw;\n    const int wg_threads = fpw * C::T;\n"
            "    int per_cu = (int)((160 * 1024) / (lds + 256));\n    const int vgpr_cap = (split ? 4 : 2) * 256 / wg_threads;\n"
            "    if (per_cu > vgpr_cap) per_cu = vgpr_cap;\n    if (per_cu < 1) per_cu = 1;\n    const long cap = 256L * per_cu * 2;\n"
            "    PssTimeScope timed(ctx);\n    pss_kernel_begin(ctx, \"k_spectrum\");\n"
            "    hipLaunchKernelGGL(kern, dim3((unsigned)(groups < cap ? groups : cap)), dim3(wg_threads), lds,",
        ]})),
    # float64 rows of the other lengths (or option f64_plain = 1) and complex128 frames: the plain LDS transform, one frame per workgroup
    "spectrum_f64_plain": Cap(
        "pss_spectrum_db_f64 (16 .. 128 and 8192 .. 65536 points, or option f64_plain)", "k_spectrum<false, false, true>", "frames",
        lambda n, o=None: generic_cap(n),
        {"pss_fft.hip": [
            "constexpr int LOG_NSUB_MAX = 12;",
            "long cap = 256L * per_cu * 4;",
            "const int logn = ilog2(n_fft), logNsub = logn < LOG_NSUB_MAX ? logn : LOG_NSUB_MAX;\n"
            "    const size_t lds = ((size_t)1 << logNsub) * sizeof(double2);\n    auto kern = k_spectrum<false, false, true>;",
            "    int per_cu = (int)((160 * 1024) / (lds + 64));\n    per_cu = per_cu > 8 ? 8 : per_cu;\n    PssTimeScope timed(ctx);\n"
            "    pss_kernel_begin(ctx, \"k_spectrum_f64\");\n    hipLaunchKernelGGL(kern, dim3(grid_for(n_frames, per_cu)), dim3(TPB), lds,",
        ]}),
    "spectrum_c128": Cap(
        "pss_spectrum_db_c128", "k_spectrum<false, false, true, true>", "frames", lambda n, o=None: generic_cap(n),
        {"pss_fft.hip": [
            "constexpr int LOG_NSUB_MAX = 12;",
            "long cap = 256L * per_cu * 4;",
            "const int logn = ilog2(n_fft), logNsub = logn < LOG_NSUB_MAX ? logn : LOG_NSUB_MAX;\n"
            "    const size_t lds = ((size_t)1 << logNsub) * sizeof(double2);\n    auto kern = k_spectrum<false, false, true, true>;",
            "    int per_cu = (int)((160 * 1024) / (lds + 64));\n    per_cu = per_cu > 8 ? 8 : per_cu;\n    PssTimeScope timed(ctx);\n"
            "    pss_kernel_begin(ctx, \"k_spectrum_c128\");\n    hipLaunchKernelGGL(kern, dim3(grid_for(n_frames, per_cu)), dim3(TPB), lds,",
        ]}),
    # option f64_plain = 1, or a length the register select does not serve
    "post_f64": Cap(
        "pss_spectrum_post_f64 (option f64_plain)", "k_post_f64", "frames", lambda n, o=None: 2048,
        {"pss_fft.hip": [
            "hipLaunchKernelGGL(k_post_f64, dim3((unsigned)(n_frames < 2048 ? n_frames : 2048)), dim3(256), 0,",
        ]}),
    "hilbert_r16": Cap(
        "pss_hilbert (256 .. 4096 samples)", "k_hilbert_r16<0..4, 0>", "rows", lambda n, o=None: hil_r16_cap(n),
        dict(R16_CFG, **{"pss_fft.hip": [
            "const long groups = (n_rows + C::FPW - 1) / C::FPW;",
            "int per_cu = (int)((160 * 1024) / (C::LDS + 256));",
            "if (per_cu > 2) per_cu = 2;",
            "return out_mode == 0 ? go(pss_hil::k_hilbert_r16<L, 0>, C::LDS, 256, groups, 256L * per_cu * 2)",
            "hipLaunchKernelGGL(kern, dim3((unsigned)(groups < cap ? groups : cap)), dim3(threads), lds, PSS_STREAM(ctx), d_x, d_out, tw, n_rows,\n"
            "                           d_maxbits, reinterpret_cast<unsigned *>(d_pcm));",
            "case 256: HIL_R16(0)",
            "case 4096: HIL_R16(4)",
        ]})),
    "hilbert_huge": Cap(
        "pss_hilbert (2^17 .. 2^20 samples)", "k_huge_p1_g<HilLoadReal / HilLoadZ>, k_huge_p2_g<BsStoreC / HilStoreOut>", "rows",
        lambda n, o=None: huge_cap(n),
        dict(R16_CFG, **{"pss_fft.hip": [
            "const int NS = n >> 8;\n        r = bs_pass1(ctx, lx, tw, S, NS, n_rows);",
            "const long total1 = n_frames * (NS / 16);\n"
            "    hipLaunchKernelGGL(kern, dim3((unsigned)(total1 < 8192 ? total1 : 8192)), dim3(256), lds1,",
            "const long rows = n_frames * 256;\n    auto go = [&](auto kern, size_t lds2, int fpw) -> int {",
            "const long groups = rows / fpw;\n        hipLaunchKernelGGL(kern, dim3((unsigned)(groups < 8192 ? groups : 8192)), dim3(256), lds2,",
            "case 512: return go(pss_r16::k_huge_p2_g<1, Store>, pss_r16::Cfg<1>::LDS, pss_r16::Cfg<1>::FPW);",
            "default: return go(pss_r16::k_huge_p2_g<4, Store>, pss_r16::Cfg<4>::LDS, pss_r16::Cfg<4>::FPW);",
        ]})),
    # decimation factor 1: the left and right channels are rows of their own (rows = 2 n_frames), four rows per workgroup
    "wfm_q1": Cap(
        "pss_demod WFM, decimation factor 1", "k_wfm_rows_q1", "frames", lambda n, o=None: 8192 * 4 // 2,
        {"pss_demod.hip": [
            "const long rows = 2 * n_frames, tiles2 = (rows + TILE - 1) / TILE;",
            "hipLaunchKernelGGL(k_wfm_rows_q1, dim3((unsigned)((rows + 3) / 4 < 8192 ? (rows + 3) / 4 : 8192)), dim3(256), 0,",
            "for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_rows; g += (long)gridDim.x * 4) {",
        ]}),
}


# ---- the receivers (pss_rds.hip, pss_adsb.hip, and the start list pss_adsb.hip shares with pss_ais.hip: pss_starts.h).  Not rows of CAPS:
# tests/test_gpu_grid_caps.py iterates that table, and these units have their past-the-cap tests in tests/test_gpu_rds.py,
# tests/test_gpu_adsb.py and tests/test_gpu_ais.py, which import the numbers below (the last through tests/ais_caps.py) instead of restating
# them.  Every number stands in a pinned line, so a changed cap fails tests/test_launch_caps.py before it can turn those tests into tests of
# nothing.
FR_T, FR_GRID_CAP = 1024, 2048            # k_rds_front: (row, tile) pairs
EN_T, EN_GRID_CAP = 256, 16384            # k_rds_energy: tiles of EN_T / 16 segments of 1024 samples
BT_T, BT_GRID_CAP = 256, 4096             # k_rds_bits: rows; BT_T segments a pass of its scan
GR_T, GR_GRID_CAP = 256, 4096             # k_rds_groups: rows
DT_T, DT_S, DT_GRID_CAP = 1024, 4096, 1024    # k_adsb_detect, k_ais_detect: tiles of DT_S starts
SC_T, SC_PER = 1024, 4                    # k_starts_scan: SC_PER * SC_T counts a step
LS_T, LS_GRID_CAP = 256, 2048             # k_starts_gather: tiles; k_adsb_keep, k_adsb_emit: LS_T / 64 accepted starts a workgroup

RDS_SEGMENT = 1024                        # pss_rds.h: SEG_BITS * SPB samples of a row
FRONT_GRID_CAP = FR_GRID_CAP
ENERGY_TILE_SEGMENTS = EN_T // 16
BITS_SCAN_PASS = BT_T
DETECT_TILE, DETECT_GRID_CAP = DT_S, DT_GRID_CAP
SCAN_STEP = SC_PER * SC_T
LIST_PASS = LS_GRID_CAP * (LS_T // 64)    # accepted starts one pass of k_adsb_keep / k_adsb_emit covers
GATHER_GRID_CAP = LS_GRID_CAP             # tiles one pass of k_starts_gather covers
ADSB_LIST_BYTES = 4 + 4 + 1               # buffer 1 of the start list, a listed start of pss_adsb_frames: the start, its rank, its keep flag

RECEIVER_CAPS = {
    "rds_front": Cap(
        "pss_rds_front", "k_rds_front", "(row, tile) pairs", lambda n=None, o=None: FR_GRID_CAP,
        {"pss_rds.hip": [
            f"constexpr int FR_T = {FR_T};",
            f"constexpr long FR_GRID_CAP = {FR_GRID_CAP};",
            "hipLaunchKernelGGL(k_rds_front, dim3((unsigned)(n_pairs < FR_GRID_CAP ? n_pairs : FR_GRID_CAP)), dim3(FR_T), 0,",
            "for (long p = blockIdx.x; p < n_pairs; p += gridDim.x) {",
        ]}),
    # n samples a row: one tile covers EN_T / SPB segments of a row, and a tile never spans two rows
    "rds_energy": Cap(
        "pss_rds_bits", "k_rds_energy", "rows",
        lambda n, o=None: EN_GRID_CAP // max(1, -(-(-(-n // RDS_SEGMENT)) // ENERGY_TILE_SEGMENTS)),
        {"pss_rds.hip": [
            f"constexpr int EN_T = {EN_T};",
            "constexpr int EN_SEGS = EN_T / SPB;",
            f"constexpr long EN_GRID_CAP = {EN_GRID_CAP};",
            "const long tiles_per_row = (n_seg + EN_SEGS - 1) / EN_SEGS, n_tiles = tiles_per_row * n_rows;",
            "hipLaunchKernelGGL(k_rds_energy, dim3((unsigned)(n_tiles < EN_GRID_CAP ? n_tiles : EN_GRID_CAP)), dim3(EN_T), 0,",
            "for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {",
        ], "pss_rds.h": [
            "constexpr int SPB = 16;",
            "constexpr int SEG_BITS = 64, SEG = SEG_BITS * SPB;",
            "PSS_DDC_HD inline int n_segments(long n) { return (int)((n + SEG - 1) / SEG); }",
        ]}),
    "rds_bits": Cap(
        "pss_rds_bits", "k_rds_bits", "rows", lambda n=None, o=None: BT_GRID_CAP,
        {"pss_rds.hip": [
            f"constexpr int BT_T = {BT_T};",
            f"constexpr long BT_GRID_CAP = {BT_GRID_CAP};",
            "hipLaunchKernelGGL(k_rds_bits, dim3((unsigned)(n_rows < BT_GRID_CAP ? n_rows : BT_GRID_CAP)), dim3(BT_T), 0,",
            "for (long row = blockIdx.x; row < n_rows; row += gridDim.x) {\n        const float2 *x = bb + (size_t)row * row_stride;",
            "for (int s0 = 0; s0 < n_seg; s0 += BT_T) {",
        ]}),
    "rds_groups": Cap(
        "pss_rds_groups", "k_rds_groups", "rows", lambda n=None, o=None: GR_GRID_CAP,
        {"pss_rds.hip": [
            f"constexpr int GR_T = {GR_T};",
            f"constexpr long GR_GRID_CAP = {GR_GRID_CAP};",
            "hipLaunchKernelGGL(k_rds_groups, dim3((unsigned)(n_rows < GR_GRID_CAP ? n_rows : GR_GRID_CAP)), dim3(GR_T), 0,",
            "for (long row = blockIdx.x; row < n_rows; row += gridDim.x) {\n        const uint8_t *b = bits + (size_t)row * max_bits;",
        ]}),
    "adsb_detect": Cap(
        "pss_adsb_frames", "k_adsb_detect", "tiles of DT_S starts", lambda n=None, o=None: DT_GRID_CAP,
        {"pss_starts.h": [
            f"constexpr int DT_T = {DT_T};",
            f"constexpr int DT_S = {DT_S};",
            f"constexpr long DT_GRID_CAP = {DT_GRID_CAP};",
        ], "pss_adsb.hip": [
            "const long n_ext = w.e1 - w.e0, n_tiles = (n_ext + DT_S - 1) / DT_S;",
            "hipLaunchKernelGGL(k_adsb_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0,",
            "for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {\n        const long g0 = e0 + tile * DT_S;",
        ]}),
    "starts_scan": Cap(
        "pss_adsb_frames, pss_ais_frames", "k_starts_scan<int>, k_starts_scan<uint8_t>", "counts a step of the one workgroup",
        lambda n=None, o=None: SC_PER * SC_T,
        {"pss_starts.h": [
            f"constexpr int SC_T = {SC_T}, SC_PER = {SC_PER};",
            "for (long b0 = 0; b0 < n; b0 += (long)SC_PER * SC_T) {",
            "int run = (int)carry + before + inc - mine;",
            "carry += all;",
            "hipLaunchKernelGGL(k_starts_scan<int>, dim3(1), dim3(SC_T), 0,",
            "hipLaunchKernelGGL(k_starts_scan<uint8_t>, dim3(1), dim3(SC_T), 0,",
        ]}),
    "starts_gather": Cap(
        "pss_adsb_frames, pss_ais_frames", "k_starts_gather<int>, k_starts_gather<long>", "tiles", lambda n=None, o=None: LS_GRID_CAP,
        {"pss_starts.h": [
            f"constexpr int LS_T = {LS_T};",
            f"constexpr long LS_GRID_CAP = {LS_GRID_CAP};",
            "hipLaunchKernelGGL(k_starts_gather<I>, dim3((unsigned)(n_tiles < LS_GRID_CAP ? n_tiles : LS_GRID_CAP)), dim3(LS_T), 0,",
            "for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {\n        const int c = tile_count[tile], o = tile_off[tile];",
        ]}),
    "adsb_list": Cap(
        "pss_adsb_frames", "k_adsb_keep, k_adsb_emit", "accepted starts", lambda n=None, o=None: LS_GRID_CAP * (LS_T // 64),
        {"pss_starts.h": [
            f"constexpr int LS_T = {LS_T};",
            f"constexpr long LS_GRID_CAP = {LS_GRID_CAP};",
            "const long blocks = (n + per - 1) / per;",
            "return (unsigned)(blocks < pss_starts::LS_GRID_CAP ? blocks : pss_starts::LS_GRID_CAP);",
        ], "pss_adsb.hip": [
            "const dim3 wave_grid(PssStartList::list_grid(n_acc, LS_T / 64));",
            "const size_t o_rank = sizeof(int) * (size_t)n_acc, o_keep = 2 * o_rank;",
            "r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + (size_t)n_acc, \"pss_adsb_frames list\");",
            "hipLaunchKernelGGL(k_adsb_keep, wave_grid, dim3(LS_T), 0,",
            "hipLaunchKernelGGL(k_adsb_emit, wave_grid, dim3(LS_T), 0,",
            "const long wave = (long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6), n_waves = (long)gridDim.x * (LS_T / 64);\n"
            "    for (long k = wave; k < n_acc; k += n_waves) {\n        const int a = acc[k];",
            "const long wave = (long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6), n_waves = (long)gridDim.x * (LS_T / 64);\n"
            "    for (long k = wave; k < n_acc; k += n_waves) {\n        if (!keep[k]) continue;",
        ]}),
}

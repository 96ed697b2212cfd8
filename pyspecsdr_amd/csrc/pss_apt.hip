// pss_apt.hip — NOAA APT: from complex64 rows at 62 400 S/s to the image's lines.  The arithmetic is pss_apt.h's; this unit places it.
//   k_apt_front    discriminator + 2400 Hz mixer + decimating FIR + magnitude, shaped like k_rds_front (pss_rds.hip): a workgroup walks
//                  (row, tile) pairs; the discriminator (float32) and the mix (float64) run ONCE per sample and the mixed sample goes to LDS
//                  by phase; every wavefront takes (tap block, 64 outputs) tasks; one lane per output adds the block sums, takes the
//                  magnitude and stores ONE float32: the complex baseband never reaches HBM.
//   k_apt_detect   a workgroup walks tiles of DT_S start positions of one row.  The tile's samples and the 116 ahead of them go to LDS once
//                  (4212 floats); every lane tests sync A at four starts (39 LDS reads each, consecutive lanes on consecutive words at every
//                  k; the 39 bits in one 64-bit word, one popcount against the pattern); a tile without a survivor ends at one
//                  __syncthreads_count; otherwise tile_slots compacts the survivors in ascending order into the tile's own list.
//   pss_starts.h   k_starts_scan and k_starts_gather, shared with pss_adsb.hip, pss_ais.hip and pss_pocsag.hip.
//   k_apt_score    one lane per survivor: mismatches and score again, from global memory, into the receiver's scratch.  (Storing them in
//                  the detect pass would cost 5 bytes for each of the 4096 starts of every tile; a real line leaves two or three survivors.)
//   k_apt_keep     one lane per survivor: the accepted starts less than 3120 away in the same row are its neighbours in the list.
//   k_apt_emit     one lane per kept start below max_syncs: the record.
//   k_apt_lines    one workgroup per line: the line's 6240 envelope samples go to LDS with coalesced reads (+0 outside the row), then lane j
//                  reads word 3 j + 1 (a stride of 3 words: no two lanes of a wavefront's half on one bank) and the stores are coalesced.
// Compiled without contraction and with correctly rounded float32 division and square root (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_apt.h"
#include "pss_chan.h"
#include "pss_ctx.h"
#include "pss_device.h"
#define PSS_STARTS_KERNELS   // this unit launches the list's kernels
#include "pss_starts.h"

namespace {

using namespace pss_apt;
using pss_dc::B;
using pss_dc::KNOTS;
using pss_dc::PART_CAP;
using pss_dc::STAGE_CAP;

// ---- front ------------------------------------------------------------------------------------------------------------------------------------
constexpr int FR_T = 1024;                      // threads of a workgroup: 16 wavefronts beside the one LDS image of a CU
constexpr int FR_WAVES = FR_T / 64;
constexpr long FR_GRID_CAP = 2048;              // workgroups of a launch: pairs past it are walked by a grid-stride loop

// iq: the caller's buffer, rows x_stride samples apart, holding row indices [lo, hi) of every row; elements 0 and 1 are readable even where
// [lo, hi) is empty.  The discriminator sample of row index i exists where i >= 1 and both i - 1 and i lie in [lo, hi); every other one
// is zero (the host has checked that no output needs one that the buffer does not hold).  first0, n_m, M, L, ROW: as k_ddc.
__global__ __launch_bounds__(FR_T) void k_apt_front(const float2 *__restrict__ iq, long x_stride, long lo, long hi, const double *__restrict__ knots,
                                                    const double *__restrict__ taps, uint64_t nw, int D, int T, long first0, long n_m, int M, int L,
                                                    int ROW, long n_tiles, long n_pairs, float *__restrict__ out, long out_stride)
{
    __shared__ double zr[STAGE_CAP], zi[STAGE_CAP];
    __shared__ double pr[PART_CAP], pi[PART_CAP];
    __shared__ uint2 rcp[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 64) rcp[tid] = pss::RCP14_AB[tid];
    __syncthreads();
    const int NB = pss_dc::n_blocks(T);
    const int q0 = tid / L, r0 = tid - q0 * L, dq = FR_T / L, dr = FR_T - dq * L;
    for (long p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const long row = p / n_tiles, tile = p - row * n_tiles;
        const long m0 = tile * M;
        const int cnt = n_m - m0 < M ? (int)(n_m - m0) : M;       // >= 1
        const int span = (cnt - 1) * D + T;                       // <= L * ROW <= STAGE_CAP
        const long first = first0 + m0 * D;
        uint64_t ph = nw * (uint64_t)(first + tid);
        const uint64_t dph = nw * (uint64_t)FR_T;
        int q = q0, r = r0;
#pragma unroll 2
        for (int j = tid; j < span; j += FR_T) {
            // the loads, the discriminator and the rotor are unconditional: a sample that is zero reads element 0 and drops the result
            const long i = first + j;
            const bool in = i - 1 >= lo && i < hi;                // lo >= 0: i >= 1
            const size_t at = in ? (size_t)row * x_stride + (i - lo) : 1;
            const float2 c = iq[at], b = iq[at - 1];
            const float d = pss_rds::disc(c.x, c.y, b.x, b.y, [&](float im, float re) { return pss::atan2f_svml(im, re, rcp); });
            double a, e;
            pss_rds::mixed(d, ph, knots, a, e);
            const int pos = r * ROW + q;
            zr[pos] = in ? a : 0.0;
            zi[pos] = in ? e : 0.0;
            ph += dph;
            q += dq;
            r += dr;
            if (r >= L) { r -= L; q++; }
        }
        __syncthreads();
        // ---- (tap block, 64 outputs) tasks, k_ddc's loop: output m of the tile and tap k read span sample m D + (T - 1 - k); a task's 64
        // taps come in with one vector load a task ahead of their use and are read back lane by lane as scalars
        const int G = (cnt + 63) >> 6;
        const int n_tasks = NB * G;
        int b = 0, g = wave;   // task t = b G + g, stepped without a division
        while (g >= G) { g -= G; b++; }
        auto block_taps = [&](int bb) { const int k = bb * B + lane; return k < T ? taps[k] : 0.0; };
        double hv = block_taps(b);   // b <= NB where the wavefront has no task: k >= T, nothing is read
        for (int t = wave; t < n_tasks; t += FR_WAVES) {
            int bn = b, gn = g + FR_WAVES;
            while (gn >= G) { gn -= G; bn++; }
            const double hn = block_taps(bn);
            const int m = g * 64 + lane;
            const int k0 = b * B, nk = T - k0 < B ? T - k0 : B;
            const int c0 = T - 1 - k0;
            int cq = c0 / L, cr = c0 - cq * L;   // wave-uniform: the row and the column offset of the block's first tap
            if (m < cnt) {
                double sr, si;
                pss_dc::block_sum([&](int kk) {
                    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(hv), kk), __builtin_amdgcn_readlane(__double2loint(hv), kk));
                }, nk, [&](int, double &vr, double &vi) {
                    const int pos = cr * ROW + cq + m;
                    vr = zr[pos];
                    vi = zi[pos];
                    if (--cr < 0) { cr = L - 1; cq--; }
                }, sr, si);
                pr[b * M + m] = sr;
                pi[b * M + m] = si;
            }
            hv = hn;
            b = bn;
            g = gn;
        }
        __syncthreads();
        // ---- one lane per output: the block sums in ascending order, the magnitude, one rounding, one float32 store.  The next pair's
        // staging writes zr / zi only, and its tasks write pr / pi behind the barrier above, which every lane reaches after this loop.
        for (int m = tid; m < cnt; m += FR_T)
            out[(size_t)row * out_stride + (m0 + m)] = envelope(NB, [&](int bb, double &sr, double &si) { sr = pr[bb * M + m]; si = pi[bb * M + m]; });
    }
}

int front_check(pss_ctx *ctx, const char *who, const void *iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, double fs, int decim,
                const double *taps, int n_taps, int lead, long m_begin, long m_end, const void *out, long out_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (!std::isfinite(fs) || !(fs > 2.0 * SUBCARRIER_HZ)) return bad("fs must be finite and above 4800 (the 2400 Hz subcarrier below the discriminator's Nyquist)");
    if (decim < 1 || decim > pss_dc::MAX_DECIM) return bad("decim outside [1, 4096]");
    if (n_taps < 1 || n_taps > pss_dc::MAX_TAPS) return bad("n_taps outside [1, 4097]");
    if (n_rows < 1) return bad("n_rows < 1");
    if (!taps) return bad("null taps");
    if (x_stride < n_buf) return bad("x_stride < n_buf");
    const int r = pss_chan_window_check(ctx, who, false, iq, n_buf, buf_index0, n_row, decim, taps, n_taps, lead, m_begin, m_end, out, out_stride);
    if (r || m_begin == m_end) return r;
    // the discriminator of the first needed sample reads the sample before it
    long need_lo = m_begin * decim + lead - (n_taps - 1), need_hi = (m_end - 1) * decim + lead + 1;
    if (need_lo < 1) need_lo = 1;
    if (need_hi > n_row) need_hi = n_row;
    if (need_lo < need_hi && need_lo - 1 < buf_index0) return bad("an output needs a sample of the capture that the buffer does not hold");
    return PSS_OK;
}

// ---- syncs ------------------------------------------------------------------------------------------------------------------------------------
constexpr int AD_Y = DT_S + REACH - 1;          // samples of a tile: 4212
static_assert(AD_Y == 4212, "the detect tile's LDS");

// where tile `tile` lies: its row and the row index of its first start
__device__ __forceinline__ void tile_at(long tile, long tpr, long e0, long &row, long &g0)
{
    row = tile / tpr;
    g0 = e0 + (tile - row * tpr) * DT_S;
}

__global__ __launch_bounds__(DT_T) void k_apt_detect(const float *__restrict__ env, long e_stride, long buf_lo, long buf_hi, long n_row, int sync_errors,
                                                     long e0, long n_ext, long tpr, long n_tiles, int *__restrict__ tile_count,
                                                     uint16_t *__restrict__ tile_list)
{
    __shared__ float es[AD_Y];
    __shared__ int wcount[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        long row, g0;
        tile_at(tile, tpr, e0, row, g0);
        const int cnt = e0 + n_ext - g0 < DT_S ? (int)(e0 + n_ext - g0) : DT_S;   // >= 1
        const int ny = cnt + REACH - 1;                                            // <= AD_Y
        // es[j] = env of row index g0 + j; a sample the buffer does not hold is a zero, and only starts that do not exist read one (the
        // host has checked that the buffer holds [e0, min(n_row, e1 - 1 + 117)))
        for (int j = tid; j < ny; j += DT_T) {
            const long i = g0 + j;
            es[j] = i >= buf_lo && i < buf_hi ? env[(size_t)row * e_stride + (i - buf_lo)] : 0.0f;
        }
        __syncthreads();
        bool oks[DT_S / DT_T];
        bool any = false;
#pragma unroll
        for (int k = 0; k < DT_S / DT_T; k++) {
            const int j = k * DT_T + tid;
            oks[k] = false;
            if (j < cnt && exists(g0 + j, n_row)) {
                int mism;
                float q;
                oks[k] = candidate([&](int kk) { return es[j + ENV_SPW * kk + 1]; }, sync_errors, mism, q);
            }
            any |= oks[k];
        }
        // (this barrier also orders the reads of es above before the next tile's staging)
        if (__syncthreads_count(any) == 0) {
            if (tid == 0) tile_count[tile] = 0;
            continue;
        }
        // ---- the survivors in ascending order into the tile's own list
        const int total = tile_slots(oks, wcount, lane, wave, [&](int k, size_t slot) { tile_list[(size_t)tile * DT_S + slot] = (uint16_t)(k * DT_T + tid); });
        if (tid == 0) tile_count[tile] = total;
        __syncthreads();   // wcount is read before the next tile with survivors writes it
    }
}

// surv[k] = the k-th survivor as tile * DT_S + its offset in the tile: ascending in (row, s)
__device__ __forceinline__ void start_at(long idx, long tpr, long e0, long &row, long &s)
{
    long g0;
    tile_at(idx / DT_S, tpr, e0, row, g0);
    s = g0 + idx % DT_S;
}

// mism[k], score[k] of survivor k: the detect kernel's test again (every survivor exists and lies in the buffer with its 117 samples)
__global__ __launch_bounds__(LS_T) void k_apt_score(const float *__restrict__ env, long e_stride, long buf_lo, const long *__restrict__ surv, long n_surv,
                                                    long tpr, long e0, int sync_errors, uint8_t *__restrict__ mism, float *__restrict__ score)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        long row, s;
        start_at(surv[k], tpr, e0, row, s);
        const float *er = env + (size_t)row * e_stride + (s - buf_lo);
        int m;
        float q;
        candidate([&](int kk) { return er[ENV_SPW * kk + 1]; }, sync_errors, m, q);
        mism[k] = (uint8_t)m;
        score[k] = q;
    }
}

__global__ __launch_bounds__(LS_T) void k_apt_keep(const long *__restrict__ surv, long n_surv, long tpr, long e0, long s_begin, long s_end,
                                                   const uint8_t *__restrict__ mism, const float *__restrict__ score, uint8_t *__restrict__ keep)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        long row_a, s_a;
        start_at(surv[k], tpr, e0, row_a, s_a);
        bool kept = s_a >= s_begin && s_a < s_end;
        if (kept) {
            const float q_a = score[k];
            const int m_a = mism[k];
            for (long q = k - 1; kept && q >= 0; q--) {
                long row_b, s_b;
                start_at(surv[q], tpr, e0, row_b, s_b);
                if (row_b != row_a || s_a - s_b >= NEAR) break;
                if (drops(s_b, mism[q], score[q], s_a, m_a, q_a)) kept = false;
            }
            for (long q = k + 1; kept && q < n_surv; q++) {
                long row_b, s_b;
                start_at(surv[q], tpr, e0, row_b, s_b);
                if (row_b != row_a || s_b - s_a >= NEAR) break;
                if (drops(s_b, mism[q], score[q], s_a, m_a, q_a)) kept = false;
            }
        }
        keep[k] = kept ? 1 : 0;
    }
}

__global__ __launch_bounds__(LS_T) void k_apt_emit(const long *__restrict__ surv, long n_surv, long tpr, long e0, const uint8_t *__restrict__ keep,
                                                   const int *__restrict__ rank, const uint8_t *__restrict__ mism, const float *__restrict__ score,
                                                   int max_syncs, int32_t *__restrict__ d_row, int64_t *__restrict__ d_pos, uint32_t *__restrict__ d_meta,
                                                   float *__restrict__ d_score)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        if (!keep[k]) continue;
        const int r = rank[k];
        if (r >= max_syncs) continue;
        long row, s;
        start_at(surv[k], tpr, e0, row, s);
        d_row[r] = (int32_t)row;
        d_pos[r] = s;
        d_meta[r] = mism[k];
        d_score[r] = score[k];
    }
}

int syncs_check(pss_ctx *ctx, const void *env, long n_rows, long e_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                int sync_errors, const void *row, const void *pos, const void *meta, const void *score, const void *count, int max_syncs)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_apt_syncs: ") + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (n_rows < 1 || n_rows > (1l << 20)) return bad("n_rows outside [1, 2^20]");
    if (sync_errors < 0 || sync_errors > MAX_SYNC_ERRORS) return bad("sync_errors outside [0, 4]");
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 's', s_begin, s_end, "starts")) return r;
    if (e_stride < n_buf) return bad("e_stride < n_buf");
    if ((s_end - s_begin + 2 * NEAR) > (1l << 31) / n_rows) return bad("more than 2^31 starts in the rows of one call");
    if (max_syncs < 0) return bad("max_syncs < 0");
    if (!count || (n_buf > 0 && !env) || (max_syncs > 0 && (!row || !pos || !meta || !score))) return bad("null buffer");
    if (off(env, 4) || off(pos, 8) || off(row, 4) || off(meta, 4) || off(score, 4) || off(count, 4)) return bad("a misaligned pointer");
    if (s_begin < s_end) {
        const Reach r = reach_of(s_begin, s_end, n_row);
        if (buf_index0 > r.need_lo || buf_index0 + n_buf < r.need_hi)
            return bad("the buffer does not cover the window's reach (3119 starts either side, 117 samples forward)");
    }
    return PSS_OK;
}

// ---- lines ------------------------------------------------------------------------------------------------------------------------------------
constexpr int LN_T = 256;
constexpr long LN_GRID_CAP = 1024;              // workgroups of a launch: lines past it are walked by a grid-stride loop
constexpr long MAX_LINES = 1l << 24;

__global__ __launch_bounds__(LN_T) void k_apt_lines(const float *__restrict__ env, long n_rows, long e_stride, long n_row, const int32_t *__restrict__ line_row,
                                                    const int64_t *__restrict__ line_pos, long n_lines, float *__restrict__ words, long words_stride)
{
    __shared__ float es[LINE_ENV];
    for (long l = blockIdx.x; l < n_lines; l += gridDim.x) {
        const long row = line_row[l], p = line_pos[l];
        const bool row_ok = row >= 0 && row < n_rows;
        const float *er = env + (size_t)(row_ok ? row : 0) * e_stride;
        for (int t = threadIdx.x; t < LINE_ENV; t += LN_T) es[t] = row_ok && line_in(p, t, n_row) ? er[p + t] : 0.0f;
        __syncthreads();
        for (int j = threadIdx.x; j < LINE_WORDS; j += LN_T) words[(size_t)l * words_stride + j] = es[ENV_SPW * j + 1];
        __syncthreads();   // es is read before the next line's staging writes it
    }
}

int lines_check(pss_ctx *ctx, const void *env, long n_rows, long e_stride, long n_row, const void *line_row, const void *line_pos, long n_lines,
                const void *words, long words_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_apt_lines: ") + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (n_rows < 1 || n_rows > (1l << 20)) return bad("n_rows outside [1, 2^20]");
    if (n_row < 0 || n_row > (1l << 60)) return bad("n_row outside [0, 2^60]");
    if (e_stride < n_row) return bad("e_stride < n_row");
    if (n_lines < 0 || n_lines > MAX_LINES) return bad("n_lines outside [0, 2^24]");
    if (words_stride < LINE_WORDS) return bad("words_stride < 2080");
    if ((n_row > 0 && !env) || (n_lines > 0 && (!line_row || !line_pos || !words))) return bad("null buffer");
    if (off(env, 4) || off(line_row, 4) || off(line_pos, 8) || off(words, 4)) return bad("a misaligned pointer");
    return PSS_OK;
}

}  // namespace

// ---- plan, taps -------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_apt_plan(double fs, int *decim, int *up, int *down)
{
    auto bad = [&](const char *why) { return pss_fail(nullptr, PSS_E_ARG, std::string("pss_apt: ") + why); };
    if (!decim || !up || !down) return bad("null argument");
    if (!std::isfinite(fs) || fs != floor(fs) || fs > 0x1p52) return bad("fs must be an integer number of Hz");
    if (!(fs >= (double)RATE)) return bad("fs must be at least 62 400");
    if (!plan((long)fs, *decim, *up, *down)) return bad("62 400 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take");
    return PSS_OK;
}

extern "C" int pss_apt_default_taps(double *taps, int *n_taps)
{
    if (!n_taps) return pss_fail(nullptr, PSS_E_ARG, "pss_apt_default_taps: null n_taps");
    *n_taps = N_DEFAULT_TAPS;
    if (!taps) return PSS_OK;
    return pss_design_firwin(N_DEFAULT_TAPS, DEFAULT_CUTOFF, taps);
}

// ---- front ------------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_apt_front(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, double fs, int decim,
                               const double *taps, int n_taps, int lead, long m_begin, long m_end, float *h_env, long env_stride)
{
    const int r = front_check(nullptr, "pss_h_apt_front", h_iq, n_rows, x_stride, n_buf, buf_index0, n_row, fs, decim, taps, n_taps, lead, m_begin, m_end,
                              h_env, env_stride);
    if (r || m_begin == m_end) return r;
    const double *knots = pss_host_knots();
    const uint64_t w = pss_dc::word_of(SUBCARRIER_HZ, fs);
    const long lo = buf_index0, hi = buf_index0 + n_buf;
    const long run = 4096;
    std::vector<double> z;
    for (long row = 0; row < n_rows; row++) {
        const float *x = h_iq + 2 * (size_t)row * x_stride;
        for (long a = m_begin; a < m_end; a += run) {
            const long e = a + run < m_end ? a + run : m_end;
            const long first = a * decim + lead - (n_taps - 1), span = (e - 1 - a) * decim + n_taps;
            z.assign((size_t)span * 2, 0.0);
            for (long j = 0; j < span; j++) {
                const long i = first + j;
                if (!(i - 1 >= lo && i < hi)) continue;
                const float *c = x + 2 * (i - lo), *b = c - 2;
                pss_rds::mixed(pss_rds::disc(c[0], c[1], b[0], b[1], pss_h_atan2f_model), pss_dc::phase_of(w, i), knots, z[2 * j], z[2 * j + 1]);
            }
            for (long m = a; m < e; m++)
                h_env[(size_t)row * env_stride + (m - m_begin)] =
                    output(m, decim, taps, n_taps, lead, [&](long i, double &vr, double &vi) { vr = z[2 * (i - first)]; vi = z[2 * (i - first) + 1]; });
        }
    }
    return PSS_OK;
}

extern "C" int pss_apt_front(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, double fs, int decim,
                             const double *taps, int n_taps, int lead, long m_begin, long m_end, float *d_env, long env_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = front_check(ctx, "pss_apt_front", d_iq, n_rows, x_stride, n_buf, buf_index0, n_row, fs, decim, taps, n_taps, lead, m_begin, m_end, d_env,
                        env_stride);
    if (r || m_begin == m_end) return r;
    if ((reinterpret_cast<uintptr_t>(d_iq) & 7) || (reinterpret_cast<uintptr_t>(d_env) & 3))
        return pss_fail(ctx, PSS_E_ARG, "pss_apt_front: d_iq must be 8-byte and d_env 4-byte aligned");
    // the host tables, back to back: knots, taps (pss_table_sync: uploaded when they differ from the device copy)
    const size_t o_taps = sizeof(double) * 2 * KNOTS, bytes = o_taps + sizeof(double) * (size_t)n_taps;
    std::vector<unsigned char> tab(bytes);
    memcpy(tab.data(), pss_host_knots(), o_taps);
    memcpy(tab.data() + o_taps, taps, bytes - o_taps);
    r = pss_table_sync(ctx, &ctx->apt_tab, tab.data(), bytes, "pss_apt_front tables");
    if (r) return r;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(ctx->apt_tab.dev);
    const int M = pss_dc::tile_outputs(decim, n_taps);
    const int L = M == 1 ? 1 : decim, ROW = pss_dc::tile_row(M, decim, n_taps);
    const long n_tiles = (m_end - m_begin + M - 1) / M;
    if (n_tiles > INT64_MAX / n_rows) return pss_fail(ctx, PSS_E_ARG, "pss_apt_front: too many (row, tile) pairs");
    const long n_pairs = n_tiles * n_rows;
    const uint64_t nw = 0 - pss_dc::word_of(SUBCARRIER_HZ, fs);
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_apt_front");
    hipLaunchKernelGGL(k_apt_front, dim3((unsigned)(n_pairs < FR_GRID_CAP ? n_pairs : FR_GRID_CAP)), dim3(FR_T), 0, PSS_STREAM(ctx),
                       // (a buffer of fewer than two samples holds no discriminator sample: the idle lanes' reads go to the table)
                       n_buf > 1 ? reinterpret_cast<const float2 *>(d_iq) : reinterpret_cast<const float2 *>(base), x_stride, buf_index0, buf_index0 + n_buf,
                       reinterpret_cast<const double *>(base), reinterpret_cast<const double *>(base + o_taps), nw, decim, n_taps,
                       m_begin * decim + lead - (n_taps - 1), m_end - m_begin, M, L, ROW, n_tiles, n_pairs, d_env, env_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_apt_front launch");
}

// ---- syncs ------------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_apt_syncs(const float *h_env, long n_rows, long e_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                               int sync_errors, int32_t *h_row, int64_t *h_pos, uint32_t *h_meta, float *h_score, int32_t *h_count, int max_syncs)
{
    const int r = syncs_check(nullptr, h_env, n_rows, e_stride, n_buf, buf_index0, n_row, s_begin, s_end, sync_errors, h_row, h_pos, h_meta, h_score, h_count,
                              max_syncs);
    if (r) return r;
    struct Rec { long s; float q; int mism; };
    int total = 0;
    std::vector<Rec> acc;
    for (long row = 0; row < n_rows && s_begin < s_end; row++) {
        const Reach w = reach_of(s_begin, s_end, n_row);
        const float *er = h_env + (size_t)row * e_stride;
        acc.clear();
        for (long s = w.e0; s < w.e1; s++) {
            if (!exists(s, n_row)) continue;
            Rec c;
            if (!candidate([&](int k) { return er[s + ENV_SPW * k + 1 - buf_index0]; }, sync_errors, c.mism, c.q)) continue;
            c.s = s;
            acc.push_back(c);
        }
        keep_starts(acc.data(), acc.size(), s_begin, s_end, NEAR,
            [&](const Rec &b, const Rec &a) { return drops(b.s, b.mism, b.q, a.s, a.mism, a.q); },
            [&](const Rec &a) {
                if (total < max_syncs) {
                    h_row[total] = (int32_t)row;
                    h_pos[total] = a.s;
                    h_meta[total] = (uint32_t)a.mism;
                    h_score[total] = a.q;
                }
                total++;
            });
    }
    *h_count = total;
    return PSS_OK;
}

extern "C" int pss_apt_syncs(pss_ctx *ctx, const float *d_env, long n_rows, long e_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                             int sync_errors, int32_t *d_row, int64_t *d_pos, uint32_t *d_meta, float *d_score, int32_t *d_count, int max_syncs)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = syncs_check(ctx, d_env, n_rows, e_stride, n_buf, buf_index0, n_row, s_begin, s_end, sync_errors, d_row, d_pos, d_meta, d_score, d_count, max_syncs);
    if (r) return r;
    if (s_begin == s_end) {
        PSS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), PSS_STREAM(ctx)));
        return PSS_OK;
    }
    const Reach w = reach_of(s_begin, s_end, n_row);
    const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;
    PssStartList &starts = ctx->starts;   // buffer 0: the tiles' counts, offsets and lists
    PssStartList::Tiles t;
    r = starts.tiles(ctx, n_tiles, "pss_apt_syncs tiles", t);
    if (r) return r;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_apt_detect");
    hipLaunchKernelGGL(k_apt_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), d_env, e_stride, buf_index0,
                       buf_index0 + n_buf, n_row, sync_errors, w.e0, n_ext, tpr, n_tiles, t.count, t.list);
    pss_kernel_end(ctx);
    long n_surv;
    r = starts.total(ctx, t, n_tiles, "k_apt_detect launch", d_count, n_surv);
    if (r || n_surv == 0) return r;
    // buffer 1: the survivors, their scores and ranks, their mismatches and keep flags: 18 bytes a survivor
    const size_t n = (size_t)n_surv;
    const size_t o_score = sizeof(long) * n, o_rank = o_score + sizeof(float) * n, o_mism = o_rank + sizeof(int) * n, o_keep = o_mism + n;
    r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + n, "pss_apt_syncs list");
    if (r) return r;
    char *b1 = reinterpret_cast<char *>(starts.buf[1]);
    long *surv = reinterpret_cast<long *>(b1);
    float *score = reinterpret_cast<float *>(b1 + o_score);
    int *rank = reinterpret_cast<int *>(b1 + o_rank);
    uint8_t *mism = reinterpret_cast<uint8_t *>(b1 + o_mism), *keep = reinterpret_cast<uint8_t *>(b1 + o_keep);
    const dim3 lane_grid(PssStartList::list_grid(n_surv, LS_T));
    starts.gather(ctx, t, n_tiles, surv);   // surv[k] = the k-th survivor as tile * DT_S + its offset in the tile: ascending in (row, s)
    pss_kernel_begin(ctx, "k_apt_score");
    hipLaunchKernelGGL(k_apt_score, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_env, e_stride, buf_index0, surv, n_surv, tpr, w.e0, sync_errors, mism, score);
    pss_kernel_end(ctx);
    pss_kernel_begin(ctx, "k_apt_keep");
    hipLaunchKernelGGL(k_apt_keep, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, s_begin, s_end, mism, score, keep);
    pss_kernel_end(ctx);
    starts.rank(ctx, keep, rank, n_surv, d_count);   // the ranks of the kept starts, and the true count
    if (max_syncs > 0) {
        pss_kernel_begin(ctx, "k_apt_emit");
        hipLaunchKernelGGL(k_apt_emit, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, keep, rank, mism, score, max_syncs, d_row, d_pos, d_meta,
                           d_score);
        pss_kernel_end(ctx);
    }
    return pss_hip_check(ctx, hipGetLastError(), "k_apt_emit launch");
}

// ---- lines ------------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_apt_lines(const float *h_env, long n_rows, long e_stride, long n_row, const int32_t *h_line_row, const int64_t *h_line_pos, long n_lines,
                               float *h_words, long words_stride)
{
    const int r = lines_check(nullptr, h_env, n_rows, e_stride, n_row, h_line_row, h_line_pos, n_lines, h_words, words_stride);
    if (r) return r;
    for (long l = 0; l < n_lines; l++) {
        const long row = h_line_row[l], p = h_line_pos[l];
        const bool row_ok = row >= 0 && row < n_rows;
        const float *er = h_env + (size_t)(row_ok ? row : 0) * e_stride;
        for (int j = 0; j < LINE_WORDS; j++)
            h_words[(size_t)l * words_stride + j] = row_ok ? line_word([&](long i) { return er[i]; }, p, j, n_row) : 0.0f;
    }
    return PSS_OK;
}

extern "C" int pss_apt_lines(pss_ctx *ctx, const float *d_env, long n_rows, long e_stride, long n_row, const int32_t *d_line_row, const int64_t *d_line_pos,
                             long n_lines, float *d_words, long words_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    const int r = lines_check(ctx, d_env, n_rows, e_stride, n_row, d_line_row, d_line_pos, n_lines, d_words, words_stride);
    if (r || n_lines == 0) return r;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_apt_lines");
    hipLaunchKernelGGL(k_apt_lines, dim3((unsigned)(n_lines < LN_GRID_CAP ? n_lines : LN_GRID_CAP)), dim3(LN_T), 0, PSS_STREAM(ctx), d_env, n_rows, e_stride, n_row,
                       d_line_row, d_line_pos, n_lines, d_words, words_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_apt_lines launch");
}

// pss_packet.hip — packet radio: from rows of IQ at 26.4 kS/s to the AX.25 frames that pass their check.  The arithmetic is pss_packet.h's;
// this unit places it.
//   k_packet_front   a workgroup walks (row, tile) pairs.  Per pair the discriminator runs ONCE per sample of the tile and its halo (11
//                    discriminator samples in front, 10 behind: 12 and 10 input samples), d goes to LDS as float32, the 4 x 22 tone table
//                    as float64, and one lane per output runs the four float64 chains from there, then the division.
//   k_packet_detect  a workgroup walks tiles of DT_S start positions of one row.  The tile's samples and the 22 + 154 around them go to LDS
//                    once; every lane tests the flag of consecutive starts (nine LDS reads 22 apart, consecutive lanes on consecutive words
//                    at every k; a tile without a survivor ends there); ballots and the wavefronts' counts compact the survivors in ascending
//                    order into the tile's own list.
//   pss_starts.h     k_starts_scan and k_starts_gather, shared with the other receivers: the ascending list of survivors, and behind the
//                    keep pass the ranks of the kept starts and the true count.
//   k_packet_walk    one lane per survivor: the score again, then the HDLC walk with its moving strobes from global memory; the payload goes
//                    to the survivor's 83 words of scratch.
//   k_packet_keep    one lane per survivor: the accepted starts less than 22 away in the same row are its neighbours in the list: the
//                    one-record-per-frame rule.
//   k_packet_emit    one wavefront per kept start below max_frames: the record.
// Compiled without contraction and with correctly rounded float32 division (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_packet.h"
#include "pss_ctx.h"
#include "pss_device.h"
#define PSS_STARTS_KERNELS   // this unit launches the list's kernels
#include "pss_starts.h"

namespace {

using namespace pss_packet;

// ---- front --------------------------------------------------------------------------------------------------------------------------------
constexpr int FR_T = 256;                        // threads of a workgroup
constexpr int FR_S = 2048;                       // outputs of a tile
constexpr long FR_GRID_CAP = 2048;               // workgroups of a launch: pairs past it are walked by a grid-stride loop
constexpr int FR_D = FR_S + WIN - 1;             // discriminator samples under a tile: 2069

// iq: the caller's buffer, rows x_stride samples apart, holding row indices [lo, hi) of every row.  d of row index i exists where
// 1 <= i < n_row; the host has checked that the buffer holds i - 1 and i for every one an output reads.
__global__ __launch_bounds__(FR_T) void k_packet_front(const float2 *__restrict__ iq, long x_stride, long lo, long hi, long n_row, const double *__restrict__ tones,
                                                       double gain, long i_begin, long n_out, long n_tiles, long n_pairs, float *__restrict__ out, long z_stride)
{
    __shared__ float ds[FR_D];
    __shared__ double ts[N_TONES * WIN];
    __shared__ uint2 rcp[64];
    const int tid = threadIdx.x;
    if (tid < 64) rcp[tid] = pss::RCP14_AB[tid];
    if (tid < N_TONES * WIN) ts[tid] = tones[tid];
    for (long p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const long row = p / n_tiles, tile = p - row * n_tiles;
        const long m0 = tile * FR_S;
        const int cnt = n_out - m0 < FR_S ? (int)(n_out - m0) : FR_S;   // >= 1
        const int span = cnt + WIN - 1;                                  // <= FR_D
        const long first = i_begin + m0 - WIN_BACK;
        __syncthreads();   // the tables are in place; the previous pair's readers of ds are done
        for (int j = tid; j < span; j += FR_T) {
            const long i = first + j;
            float d = 0.0f;
            if (i >= 1 && i < n_row && i - 1 >= lo && i < hi) {
                const size_t at = (size_t)row * x_stride + (i - lo);
                const float2 cur = iq[at], prev = iq[at - 1];
                d = disc(cur.x, cur.y, prev.x, prev.y, [&](float im, float re) { return pss::atan2f_svml(im, re, rcp); });
            }
            ds[j] = d;
        }
        __syncthreads();
        for (int m = tid; m < cnt; m += FR_T)
            out[(size_t)row * z_stride + (m0 + m)] = tone_balance([&](long i) { return ds[i - first]; }, ts, gain, i_begin + m0 + m);
    }
}

int front_check(pss_ctx *ctx, const void *iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *tones, double space_gain,
                long i_begin, long i_end, const void *z, long z_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_packet_front: ") + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (n_rows < 1) return bad("n_rows < 1");
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 'i', i_begin, i_end, "samples")) return r;
    if (x_stride < n_buf) return bad("x_stride < n_buf");
    if (z_stride < i_end - i_begin) return bad("z_stride < i_end - i_begin");
    if (!tones) return bad("null tone table");
    for (int u = 0; u < N_TONES * WIN; u++)
        if (!std::isfinite(tones[u])) return bad("a table entry that is not finite");
    if (!std::isfinite(space_gain) || !(space_gain > 0.0)) return bad("space_gain must be finite and > 0");
    if ((n_buf > 0 && !iq) || (i_end > i_begin && !z)) return bad("null buffer");
    if (off(iq, 8) || off(z, 4)) return bad("a misaligned pointer");
    if (i_begin < i_end) {
        const Span s = front_span(i_begin, i_end, n_row);
        if (buf_index0 > s.lo || buf_index0 + n_buf < s.hi) return bad("the buffer does not cover the window's halo (12 samples in front, 10 behind)");
    }
    return PSS_OK;
}

// ---- frames -------------------------------------------------------------------------------------------------------------------------------
constexpr int DT_Z = DT_S + BACK + HEAD;         // samples of a tile: 4272
constexpr int REC_WORDS = REC_BYTES / 4;         // a survivor's payload in scratch: 83 words

// where tile `tile` lies: its row and the row index of its first start
__device__ __forceinline__ void tile_at(long tile, long tpr, long e0, long &row, long &g0)
{
    row = tile / tpr;
    g0 = e0 + (tile - row * tpr) * DT_S;
}

__global__ __launch_bounds__(DT_T) void k_packet_detect(const float *__restrict__ z, long z_stride, long buf_lo, long buf_hi, long n_row, long e0, long n_ext,
                                                        long tpr, long n_tiles, float q_min, int *__restrict__ tile_count, uint16_t *__restrict__ tile_list)
{
    __shared__ float zs[DT_Z];
    __shared__ int wcount[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        long row, g0;
        tile_at(tile, tpr, e0, row, g0);
        const int cnt = e0 + n_ext - g0 < DT_S ? (int)(e0 + n_ext - g0) : DT_S;   // >= 1
        const int nz = cnt + BACK + HEAD;                                          // <= DT_Z
        // zs[j] = z of row index g0 - 22 + j; a sample the buffer does not hold is a zero, and only starts that do not exist read one
        // (the host has checked that the buffer holds [max(0, e0 - 22), min(n_row, e1 - 1 + REACH)))
        for (int j = tid; j < nz; j += DT_T) {
            const long i = g0 - BACK + j;
            zs[j] = i >= buf_lo && i < buf_hi ? z[(size_t)row * z_stride + (i - buf_lo)] : 0.0f;
        }
        __syncthreads();
        bool oks[DT_S / DT_T];
        bool any = false;
#pragma unroll
        for (int k = 0; k < DT_S / DT_T; k++) {
            const int j = k * DT_T + tid;
            oks[k] = false;
            if (j < cnt && exists(g0 + j, n_row)) {
                float q;
                oks[k] = candidate([&](int kk) { return zs[j + BACK + SPB * kk]; }, q_min, q);
            }
            any |= oks[k];
        }
        // (this barrier also orders the reads of zs above before the next tile's staging)
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

// len[k]: the bytes of survivor k's frame, 0 where the walk or the check rejects it; score[k] = q; words[83 k ...]: the payload, zero-padded
// where len > 0
__global__ __launch_bounds__(LS_T) void k_packet_walk(const float *__restrict__ z, long z_stride, long buf_lo, long n_row, const long *__restrict__ surv,
                                                      long n_surv, long tpr, long e0, float q_min, int *__restrict__ len, float *__restrict__ score,
                                                      uint32_t *__restrict__ words)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        long row, s;
        start_at(surv[k], tpr, e0, row, s);
        const float *zr = z + (size_t)row * z_stride + (s - buf_lo);
        float q;
        candidate([&](int kk) { return zr[SPB * kk]; }, q_min, q);
        uint32_t *w = words + (size_t)k * REC_WORDS;
        const int nb = walk([&](long j) { return zr[j]; }, n_row - s, [&](int i, uint32_t v) { w[i] = v; });
        if (nb > 0)
            for (int i = (nb + 3) / 4; i < REC_WORDS; i++) w[i] = 0u;
        len[k] = nb;
        score[k] = q;
    }
}

__device__ __forceinline__ bool same_words(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int nb)
{
    for (int i = 0; i < (nb + 3) / 4; i++)
        if (a[i] != b[i]) return false;
    return true;
}

__global__ __launch_bounds__(LS_T) void k_packet_keep(const long *__restrict__ surv, long n_surv, long tpr, long e0, long s_begin, long s_end,
                                                      const int *__restrict__ len, const float *__restrict__ score, const uint32_t *__restrict__ words,
                                                      uint8_t *__restrict__ keep)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        long row_a, s_a;
        start_at(surv[k], tpr, e0, row_a, s_a);
        const int n_a = len[k];
        bool kept = n_a > 0 && s_a >= s_begin && s_a < s_end;
        if (kept) {
            const float q_a = score[k];
            const uint32_t *w_a = words + (size_t)k * REC_WORDS;
            auto same_as = [&](long q) {
                return len[q] == n_a && same_words(words + (size_t)q * REC_WORDS, w_a, n_a);
            };
            for (long q = k - 1; kept && q >= 0; q--) {
                long row_b, s_b;
                start_at(surv[q], tpr, e0, row_b, s_b);
                if (row_b != row_a || s_a - s_b >= NEAR) break;
                if (drops(same_as(q), s_b, score[q], s_a, q_a)) kept = false;
            }
            for (long q = k + 1; kept && q < n_surv; q++) {
                long row_b, s_b;
                start_at(surv[q], tpr, e0, row_b, s_b);
                if (row_b != row_a || s_b - s_a >= NEAR) break;
                if (drops(same_as(q), s_b, score[q], s_a, q_a)) kept = false;
            }
        }
        keep[k] = kept ? 1 : 0;
    }
}

__global__ __launch_bounds__(LS_T) void k_packet_emit(const long *__restrict__ surv, long n_surv, long tpr, long e0, const uint8_t *__restrict__ keep,
                                                      const int *__restrict__ rank, const int *__restrict__ len, const float *__restrict__ score,
                                                      const uint32_t *__restrict__ words, int max_frames, uint8_t *__restrict__ d_msg, int32_t *__restrict__ d_len,
                                                      int32_t *__restrict__ d_row, int64_t *__restrict__ d_pos, float *__restrict__ d_score)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6), n_waves = (long)gridDim.x * (LS_T / 64);
    for (long k = wave; k < n_surv; k += n_waves) {
        if (!keep[k]) continue;
        const int r = rank[k];
        if (r >= max_frames) continue;
        const uint8_t *src = reinterpret_cast<const uint8_t *>(words + (size_t)k * REC_WORDS);
        uint8_t *dst = d_msg + (size_t)r * REC_BYTES;
        for (int j = lane; j < REC_BYTES; j += 64) dst[j] = src[j];
        if (lane == 0) {
            long row, s;
            start_at(surv[k], tpr, e0, row, s);
            d_len[r] = len[k];
            d_row[r] = (int32_t)row;
            d_pos[r] = s;
            d_score[r] = score[k];
        }
    }
}

int frames_check(pss_ctx *ctx, const void *z, long n_rows, long z_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, float q_min,
                 const void *msg, const void *len, const void *row, const void *pos, const void *score, const void *count, int max_frames)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_packet_frames: ") + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (n_rows < 1 || n_rows > (1l << 20)) return bad("n_rows outside [1, 2^20]");
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 's', s_begin, s_end, "starts")) return r;
    if (z_stride < n_buf) return bad("z_stride < n_buf");
    if ((s_end - s_begin + 2 * NEAR) > (1l << 31) / n_rows) return bad("more than 2^31 starts in the rows of one call");
    if (!std::isfinite(q_min) || q_min < 0.0f) return bad("q_min must be finite and >= 0");
    if (max_frames < 0) return bad("max_frames < 0");
    if (!count || (n_buf > 0 && !z) || (max_frames > 0 && (!msg || !len || !row || !pos || !score))) return bad("null buffer");
    if (off(z, 4) || off(pos, 8) || off(len, 4) || off(row, 4) || off(score, 4) || off(count, 4)) return bad("a misaligned pointer");
    if (s_begin < s_end) {
        const Reach r = reach_of(s_begin, s_end, n_row);
        if (buf_index0 > r.need_lo || buf_index0 + n_buf < r.need_hi)
            return bad("the buffer does not cover the window's reach (21 starts either side, 22 samples back, 73203 samples forward)");
    }
    return PSS_OK;
}

}  // namespace

// ---- plan, tones ------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_packet_plan(double fs, int *decim, int *up, int *down)
{
    auto bad = [&](const char *why) { return pss_fail(nullptr, PSS_E_ARG, std::string("pss_packet: ") + why); };
    if (!decim || !up || !down) return bad("null argument");
    if (!std::isfinite(fs) || fs != floor(fs) || fs > 0x1p52) return bad("fs must be an integer number of Hz");
    if (!(fs >= (double)RATE)) return bad("fs must be at least 26 400");
    if (!plan((long)fs, *decim, *up, *down)) return bad("26 400 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take");
    return PSS_OK;
}

extern "C" int pss_packet_default_tones(double *tones)
{
    if (!tones) return pss_fail(nullptr, PSS_E_ARG, "pss_packet_default_tones: null table");
    default_tones(tones);
    return PSS_OK;
}

// ---- front ------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_packet_front(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *tones, double space_gain,
                                  long i_begin, long i_end, float *h_z, long z_stride)
{
    const int r = front_check(nullptr, h_iq, n_rows, x_stride, n_buf, buf_index0, n_row, tones, space_gain, i_begin, i_end, h_z, z_stride);
    if (r || i_begin == i_end) return r;
    const long first = i_begin - WIN_BACK, span = i_end - i_begin + WIN - 1;
    std::vector<float> d((size_t)span);
    for (long row = 0; row < n_rows; row++) {
        const float *x = h_iq + 2 * (size_t)row * x_stride;
        for (long j = 0; j < span; j++) {
            const long i = first + j;
            d[j] = 0.0f;
            if (i >= 1 && i < n_row) {
                const float *cur = x + 2 * (i - buf_index0), *prev = cur - 2;
                d[j] = disc(cur[0], cur[1], prev[0], prev[1], pss_h_atan2f_model);
            }
        }
        for (long i = i_begin; i < i_end; i++)
            h_z[(size_t)row * z_stride + (i - i_begin)] = tone_balance([&](long q) { return d[q - first]; }, tones, space_gain, i);
    }
    return PSS_OK;
}

extern "C" int pss_packet_front(pss_ctx *ctx, const float *dev_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *tones,
                                double space_gain, long i_begin, long i_end, float *dev_z, long z_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = front_check(ctx, dev_iq, n_rows, x_stride, n_buf, buf_index0, n_row, tones, space_gain, i_begin, i_end, dev_z, z_stride);
    if (r || i_begin == i_end) return r;
    r = pss_table_sync(ctx, &ctx->packet_tones, tones, sizeof(double) * N_TONES * WIN, "pss_packet_front tones");
    if (r) return r;
    const long n_out = i_end - i_begin, n_tiles = (n_out + FR_S - 1) / FR_S;
    if (n_tiles > INT64_MAX / n_rows) return pss_fail(ctx, PSS_E_ARG, "pss_packet_front: too many (row, tile) pairs");
    const long n_pairs = n_tiles * n_rows;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_packet_front");
    hipLaunchKernelGGL(k_packet_front, dim3((unsigned)(n_pairs < FR_GRID_CAP ? n_pairs : FR_GRID_CAP)), dim3(FR_T), 0, PSS_STREAM(ctx),
                       reinterpret_cast<const float2 *>(dev_iq), x_stride, buf_index0, buf_index0 + n_buf, n_row,
                       reinterpret_cast<const double *>(ctx->packet_tones.dev), space_gain, i_begin, n_out, n_tiles, n_pairs, dev_z, z_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_packet_front launch");
}

// ---- frames -------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_packet_frames(const float *h_z, long n_rows, long z_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, float q_min,
                                   uint8_t *h_msg, int32_t *h_len, int32_t *h_row, int64_t *h_pos, float *h_score, int32_t *h_count, int max_frames)
{
    const int r = frames_check(nullptr, h_z, n_rows, z_stride, n_buf, buf_index0, n_row, s_begin, s_end, q_min, h_msg, h_len, h_row, h_pos, h_score, h_count,
                               max_frames);
    if (r) return r;
    struct Rec { long s; int len; float q; uint8_t msg[REC_BYTES]; };
    int total = 0;
    std::vector<Rec> acc;
    for (long row = 0; row < n_rows && s_begin < s_end; row++) {
        const Reach w = reach_of(s_begin, s_end, n_row);
        const float *zr = h_z + (size_t)row * z_stride;
        acc.clear();
        for (long s = w.e0; s < w.e1; s++) {
            if (!exists(s, n_row)) continue;
            Rec c;
            if (!candidate([&](int k) { return zr[s + SPB * k - buf_index0]; }, q_min, c.q)) continue;
            memset(c.msg, 0, REC_BYTES);
            c.s = s;
            c.len = walk([&](long j) { return zr[s + j - buf_index0]; }, n_row - s, [&](int i, uint32_t v) {
                for (int b = 0; b < 4; b++) c.msg[4 * i + b] = (uint8_t)(v >> (8 * b));
            });
            if (c.len > 0) acc.push_back(c);
        }
        keep_starts(acc.data(), acc.size(), s_begin, s_end, NEAR,
            [&](const Rec &b, const Rec &a) { return drops(b.len == a.len && memcmp(b.msg, a.msg, REC_BYTES) == 0, b.s, b.q, a.s, a.q); },
            [&](const Rec &a) {
                if (total < max_frames) {
                    memcpy(h_msg + (size_t)total * REC_BYTES, a.msg, REC_BYTES);
                    h_len[total] = a.len;
                    h_row[total] = (int32_t)row;
                    h_pos[total] = a.s;
                    h_score[total] = a.q;
                }
                total++;
            });
    }
    *h_count = total;
    return PSS_OK;
}

extern "C" int pss_packet_frames(pss_ctx *ctx, const float *dev_z, long n_rows, long z_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                                 float q_min, uint8_t *dev_msg, int32_t *dev_len, int32_t *dev_row, int64_t *dev_pos, float *dev_score, int32_t *dev_count,
                                 int max_frames)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = frames_check(ctx, dev_z, n_rows, z_stride, n_buf, buf_index0, n_row, s_begin, s_end, q_min, dev_msg, dev_len, dev_row, dev_pos, dev_score, dev_count,
                         max_frames);
    if (r) return r;
    if (s_begin == s_end) {
        PSS_HIP(ctx, hipMemsetAsync(dev_count, 0, sizeof(int32_t), PSS_STREAM(ctx)));
        return PSS_OK;
    }
    const Reach w = reach_of(s_begin, s_end, n_row);
    const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;
    PssStartList &starts = ctx->starts;   // buffer 0: the tiles' counts, offsets and lists
    PssStartList::Tiles t;
    r = starts.tiles(ctx, n_tiles, "pss_packet_frames tiles", t);
    if (r) return r;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_packet_detect");
    hipLaunchKernelGGL(k_packet_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), dev_z, z_stride, buf_index0,
                       buf_index0 + n_buf, n_row, w.e0, n_ext, tpr, n_tiles, q_min, t.count, t.list);
    pss_kernel_end(ctx);
    long n_surv;
    r = starts.total(ctx, t, n_tiles, "k_packet_detect launch", dev_count, n_surv);
    if (r || n_surv == 0) return r;
    // buffer 1: the survivors, their payload words, lengths, scores and ranks, their keep flags
    const size_t n = (size_t)n_surv;
    const size_t o_words = sizeof(long) * n, o_len = o_words + sizeof(uint32_t) * REC_WORDS * n, o_score = o_len + sizeof(int) * n,
                 o_rank = o_score + sizeof(float) * n, o_keep = o_rank + sizeof(int) * n;
    r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + n, "pss_packet_frames list");
    if (r) return r;
    char *b1 = reinterpret_cast<char *>(starts.buf[1]);
    long *surv = reinterpret_cast<long *>(b1);
    uint32_t *words = reinterpret_cast<uint32_t *>(b1 + o_words);
    int *len = reinterpret_cast<int *>(b1 + o_len), *rank = reinterpret_cast<int *>(b1 + o_rank);
    float *score = reinterpret_cast<float *>(b1 + o_score);
    uint8_t *keep = reinterpret_cast<uint8_t *>(b1 + o_keep);
    const dim3 lane_grid(PssStartList::list_grid(n_surv, LS_T)), wave_grid(PssStartList::list_grid(n_surv, LS_T / 64));
    starts.gather(ctx, t, n_tiles, surv);   // surv[k] = the k-th survivor as tile * DT_S + its offset in the tile: ascending in (row, s)
    pss_kernel_begin(ctx, "k_packet_walk");
    hipLaunchKernelGGL(k_packet_walk, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), dev_z, z_stride, buf_index0, n_row, surv, n_surv, tpr, w.e0, q_min, len, score, words);
    pss_kernel_end(ctx);
    pss_kernel_begin(ctx, "k_packet_keep");
    hipLaunchKernelGGL(k_packet_keep, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, s_begin, s_end, len, score, words, keep);
    pss_kernel_end(ctx);
    starts.rank(ctx, keep, rank, n_surv, dev_count);   // the ranks of the kept starts, and the true count
    if (max_frames > 0) {
        pss_kernel_begin(ctx, "k_packet_emit");
        hipLaunchKernelGGL(k_packet_emit, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, keep, rank, len, score, words, max_frames, dev_msg,
                           dev_len, dev_row, dev_pos, dev_score);
        pss_kernel_end(ctx);
    }
    return pss_hip_check(ctx, hipGetLastError(), "k_packet_emit launch");
}

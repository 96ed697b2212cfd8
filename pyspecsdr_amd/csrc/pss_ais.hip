// pss_ais.hip — AIS: from rows of IQ at 48 kS/s to the frames that pass their check.  The arithmetic is pss_ais.h's; this unit places it.
//   k_ais_front   a workgroup walks (row, tile) pairs.  Per pair the discriminator runs ONCE per sample of the tile and its halo of c
//                 samples either side, d goes to LDS, and one lane per output runs the float64 tap loop from there.
//   k_ais_detect  a workgroup walks tiles of DT_S start positions of one row.  The tile's samples and the 45 + 35 around them go to LDS
//                 once; every lane tests the training sequence and the flag of consecutive starts (17 LDS reads, consecutive lanes on
//                 consecutive words at every k; a tile without a survivor ends there); ballots and the wavefronts' counts compact the
//                 survivors in ascending order into the tile's own list.
//   pss_starts.h  k_starts_scan and k_starts_gather, shared with pss_adsb.hip: the tiles' counts become offsets and a total, the tiles'
//                 lists are laid back to back (the ascending list of survivors as long tile * DT_S + offset: no atomics, no cap), and
//                 behind the keep pass the same scan ranks the kept starts and writes the true count.
//   k_ais_walk    one lane per survivor: threshold and score again, then the HDLC walk with its strobes from global memory; the payload
//                 goes to the survivor's 32 words of scratch.
//   k_ais_keep    one lane per survivor: the accepted starts less than 5 away in the same row are its neighbours in the list: the
//                 one-record-per-burst rule.
//   k_ais_emit    one wavefront per kept start below max_frames: the record.
// Compiled without contraction and with correctly rounded float32 division (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_ais.h"
#include "pss_ctx.h"
#include "pss_device.h"
#define PSS_STARTS_KERNELS   // this unit launches the list's kernels
#include "pss_starts.h"

namespace {

using namespace pss_ais;

// ---- front --------------------------------------------------------------------------------------------------------------------------------
constexpr int FR_T = 256;                        // threads of a workgroup
constexpr int FR_S = 2048;                       // outputs of a tile
constexpr long FR_GRID_CAP = 2048;               // workgroups of a launch: pairs past it are walked by a grid-stride loop
constexpr int FR_D = FR_S + MAX_PULSE - 1;       // discriminator samples under a tile: 2112

// iq: the caller's buffer, rows x_stride samples apart, holding row indices [lo, hi) of every row.  d of row index i exists where
// 1 <= i < n_row; the host has checked that the buffer holds i - 1 and i for every one an output reads.
__global__ __launch_bounds__(FR_T) void k_ais_front(const float2 *__restrict__ iq, long x_stride, long lo, long hi, long n_row, const double *__restrict__ pulse,
                                                    int P, long i_begin, long n_out, long n_tiles, long n_pairs, float *__restrict__ out, long y_stride)
{
    __shared__ float ds[FR_D];
    __shared__ double gs[MAX_PULSE];
    __shared__ uint2 rcp[64];
    const int tid = threadIdx.x;
    if (tid < 64) rcp[tid] = pss::RCP14_AB[tid];
    if (tid < P) gs[tid] = pulse[tid];
    const int c = (P - 1) / 2;
    for (long p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const long row = p / n_tiles, tile = p - row * n_tiles;
        const long m0 = tile * FR_S;
        const int cnt = n_out - m0 < FR_S ? (int)(n_out - m0) : FR_S;   // >= 1
        const int span = cnt + P - 1;                                    // <= FR_D
        const long first = i_begin + m0 - c;
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
            out[(size_t)row * y_stride + (m0 + m)] = filtered([&](long i) { return ds[i - first]; }, gs, P, i_begin + m0 + m);
    }
}

int pulse_check(pss_ctx *ctx, const char *who, const double *pulse, int n_pulse)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (!pulse || n_pulse < 1 || n_pulse > MAX_PULSE || !(n_pulse & 1)) return bad("n_pulse must be odd and in [1, 65]");
    for (int u = 0; u < n_pulse; u++)
        if (!std::isfinite(pulse[u])) return bad("a pulse tap that is not finite");
    return PSS_OK;
}

int front_check(pss_ctx *ctx, const char *who, const void *iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *pulse,
                int n_pulse, long i_begin, long i_end, const void *y, long y_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (n_rows < 1) return bad("n_rows < 1");
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 'i', i_begin, i_end, "samples")) return r;
    if (x_stride < n_buf) return bad("x_stride < n_buf");
    if (y_stride < i_end - i_begin) return bad("y_stride < i_end - i_begin");
    const int r = pulse_check(ctx, who, pulse, n_pulse);
    if (r) return r;
    if ((n_buf > 0 && !iq) || (i_end > i_begin && !y)) return bad("null buffer");
    if (off(iq, 8) || off(y, 4)) return bad("a misaligned pointer");
    if (i_begin < i_end) {
        const Span s = front_span(i_begin, i_end, n_pulse, n_row);
        if (buf_index0 > s.lo || buf_index0 + n_buf < s.hi) return bad("the buffer does not cover the window's halo ((P - 1) / 2 + 1 samples in front, (P - 1) / 2 behind)");
    }
    return PSS_OK;
}

// ---- frames -------------------------------------------------------------------------------------------------------------------------------
constexpr int DT_Y = DT_S + BACK + HEAD;         // samples of a tile: 4176
constexpr int REC_WORDS = MAX_BYTES / 4;         // a survivor's payload in scratch: 32 words

// where tile `tile` lies: its row and the row index of its first start
__device__ __forceinline__ void tile_at(long tile, long tpr, long e0, long &row, long &g0)
{
    row = tile / tpr;
    g0 = e0 + (tile - row * tpr) * DT_S;
}

__global__ __launch_bounds__(DT_T) void k_ais_detect(const float *__restrict__ y, long y_stride, long buf_lo, long buf_hi, long n_row, long e0, long n_ext,
                                                     long tpr, long n_tiles, int *__restrict__ tile_count, uint16_t *__restrict__ tile_list)
{
    __shared__ float ys[DT_Y];
    __shared__ int wcount[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        long row, g0;
        tile_at(tile, tpr, e0, row, g0);
        const int cnt = e0 + n_ext - g0 < DT_S ? (int)(e0 + n_ext - g0) : DT_S;   // >= 1
        const int ny = cnt + BACK + HEAD;                                          // <= DT_Y
        // ys[j] = y of row index g0 - 45 + j; a sample the buffer does not hold is a zero, and only starts that do not exist read one
        // (the host has checked that the buffer holds [max(0, e0 - 45), min(n_row, e1 - 1 + REACH)))
        for (int j = tid; j < ny; j += DT_T) {
            const long i = g0 - BACK + j;
            ys[j] = i >= buf_lo && i < buf_hi ? y[(size_t)row * y_stride + (i - buf_lo)] : 0.0f;
        }
        __syncthreads();
        bool oks[DT_S / DT_T];
        bool any = false;
#pragma unroll
        for (int k = 0; k < DT_S / DT_T; k++) {
            const int j = k * DT_T + tid;
            oks[k] = false;
            if (j < cnt && exists(g0 + j, n_row)) {
                float thr, q;
                oks[k] = candidate([&](int kk) { return ys[j + BACK + SPB * kk]; }, thr, q);
            }
            any |= oks[k];
        }
        // (this barrier also orders the reads of ys above before the next tile's staging)
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

// len[k]: the bytes of survivor k's frame, 0 where the walk or the check rejects it; score[k] = q; words[32 k ...]: the payload, zero-padded
// where len > 0
__global__ __launch_bounds__(LS_T) void k_ais_walk(const float *__restrict__ y, long y_stride, long buf_lo, long n_row, const long *__restrict__ surv, long n_surv,
                                                   long tpr, long e0, int *__restrict__ len, float *__restrict__ score, uint32_t *__restrict__ words)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        long row, s;
        start_at(surv[k], tpr, e0, row, s);
        const float *yr = y + (size_t)row * y_stride + (s - buf_lo);
        auto Y = [&](int kk) { return yr[SPB * kk]; };
        float thr, q;
        candidate(Y, thr, q);
        uint32_t *w = words + (size_t)k * REC_WORDS;
        const int nb = walk(Y, thr, (n_row - s + SPB - 1) / SPB, [&](int i, uint32_t v) { w[i] = v; });
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

__global__ __launch_bounds__(LS_T) void k_ais_keep(const long *__restrict__ surv, long n_surv, long tpr, long e0, long s_begin, long s_end,
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

__global__ __launch_bounds__(LS_T) void k_ais_emit(const long *__restrict__ surv, long n_surv, long tpr, long e0, const uint8_t *__restrict__ keep,
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
        uint8_t *dst = d_msg + (size_t)r * MAX_BYTES;
        dst[lane] = src[lane];
        dst[lane + 64] = src[lane + 64];
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

int frames_check(pss_ctx *ctx, const char *who, const void *y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                 const void *msg, const void *len, const void *row, const void *pos, const void *score, const void *count, int max_frames)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (n_rows < 1 || n_rows > (1l << 20)) return bad("n_rows outside [1, 2^20]");
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 's', s_begin, s_end, "starts")) return r;
    if (y_stride < n_buf) return bad("y_stride < n_buf");
    if ((s_end - s_begin + 2 * NEAR) > (1l << 31) / n_rows) return bad("more than 2^31 starts in the rows of one call");
    if (max_frames < 0) return bad("max_frames < 0");
    if (!count || (n_buf > 0 && !y) || (max_frames > 0 && (!msg || !len || !row || !pos || !score))) return bad("null buffer");
    if (off(y, 4) || off(pos, 8) || off(len, 4) || off(row, 4) || off(score, 4) || off(count, 4)) return bad("a misaligned pointer");
    if (s_begin < s_end) {
        const Reach r = reach_of(s_begin, s_end, n_row);
        if (buf_index0 > r.need_lo || buf_index0 + n_buf < r.need_hi)
            return bad("the buffer does not cover the window's reach (4 starts either side, 45 samples back, 6221 samples forward)");
    }
    return PSS_OK;
}

}  // namespace

// ---- plan, pulse, crc -----------------------------------------------------------------------------------------------------------------------
extern "C" int pss_ais_plan(double fs, int *decim, int *up, int *down)
{
    auto bad = [&](const char *why) { return pss_fail(nullptr, PSS_E_ARG, std::string("pss_ais: ") + why); };
    if (!decim || !up || !down) return bad("null argument");
    if (!std::isfinite(fs) || fs != floor(fs) || fs > 0x1p52) return bad("fs must be an integer number of Hz");
    if (!(fs >= (double)RATE)) return bad("fs must be at least 48 000");
    if (!plan((long)fs, *decim, *up, *down)) return bad("48 000 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take");
    return PSS_OK;
}

extern "C" int pss_ais_default_pulse(int span_bits, double *pulse, int *n_pulse)
{
    if (!n_pulse || span_bits < 1 || span_bits > MAX_SPAN)
        return pss_fail(nullptr, PSS_E_ARG, "pss_ais_default_pulse: span_bits outside [1, 12] (5 span_bits + 1 taps, at most 61)");
    *n_pulse = pulse_len(span_bits);
    if (pulse) default_pulse(span_bits, pulse);
    return PSS_OK;
}

extern "C" uint32_t pss_ais_crc(const uint8_t *bytes, long n)
{
    if (!bytes || n < 0) return 0xFFFFFFFFu;
    return crc_reg(bytes, n) ^ 0xFFFFu;
}

// ---- front ------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_ais_front(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *pulse, int n_pulse,
                               long i_begin, long i_end, float *h_y, long y_stride)
{
    const int r = front_check(nullptr, "pss_h_ais_front", h_iq, n_rows, x_stride, n_buf, buf_index0, n_row, pulse, n_pulse, i_begin, i_end, h_y, y_stride);
    if (r || i_begin == i_end) return r;
    const int c = (n_pulse - 1) / 2;
    const long first = i_begin - c, span = i_end - i_begin + 2 * c;
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
            h_y[(size_t)row * y_stride + (i - i_begin)] = filtered([&](long q) { return d[q - first]; }, pulse, n_pulse, i);
    }
    return PSS_OK;
}

extern "C" int pss_ais_front(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *pulse,
                             int n_pulse, long i_begin, long i_end, float *d_y, long y_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = front_check(ctx, "pss_ais_front", d_iq, n_rows, x_stride, n_buf, buf_index0, n_row, pulse, n_pulse, i_begin, i_end, d_y, y_stride);
    if (r || i_begin == i_end) return r;
    r = pss_table_sync(ctx, &ctx->ais_pulse, pulse, sizeof(double) * (size_t)n_pulse, "pss_ais_front pulse");
    if (r) return r;
    const long n_out = i_end - i_begin, n_tiles = (n_out + FR_S - 1) / FR_S;
    if (n_tiles > INT64_MAX / n_rows) return pss_fail(ctx, PSS_E_ARG, "pss_ais_front: too many (row, tile) pairs");
    const long n_pairs = n_tiles * n_rows;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_ais_front");
    hipLaunchKernelGGL(k_ais_front, dim3((unsigned)(n_pairs < FR_GRID_CAP ? n_pairs : FR_GRID_CAP)), dim3(FR_T), 0, PSS_STREAM(ctx),
                       reinterpret_cast<const float2 *>(d_iq), x_stride, buf_index0, buf_index0 + n_buf, n_row,
                       reinterpret_cast<const double *>(ctx->ais_pulse.dev), n_pulse, i_begin, n_out, n_tiles, n_pairs, d_y, y_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_ais_front launch");
}

// ---- frames -------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_ais_frames(const float *h_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                                uint8_t *h_msg, int32_t *h_len, int32_t *h_row, int64_t *h_pos, float *h_score, int32_t *h_count, int max_frames)
{
    const int r = frames_check(nullptr, "pss_ais_frames", h_y, n_rows, y_stride, n_buf, buf_index0, n_row, s_begin, s_end, h_msg, h_len, h_row, h_pos, h_score,
                               h_count, max_frames);
    if (r) return r;
    struct Rec { long s; int len; float q; uint8_t msg[MAX_BYTES]; };
    int total = 0;
    std::vector<Rec> acc;
    for (long row = 0; row < n_rows && s_begin < s_end; row++) {
        const Reach w = reach_of(s_begin, s_end, n_row);
        const float *yr = h_y + (size_t)row * y_stride;
        acc.clear();
        for (long s = w.e0; s < w.e1; s++) {
            if (!exists(s, n_row)) continue;
            auto Y = [&](int k) { return yr[s + SPB * k - buf_index0]; };
            float thr;
            Rec c;
            if (!candidate(Y, thr, c.q)) continue;
            memset(c.msg, 0, MAX_BYTES);
            c.s = s;
            c.len = walk(Y, thr, (n_row - s + SPB - 1) / SPB, [&](int i, uint32_t v) {
                for (int b = 0; b < 4; b++) c.msg[4 * i + b] = (uint8_t)(v >> (8 * b));
            });
            if (c.len > 0) acc.push_back(c);
        }
        keep_starts(acc.data(), acc.size(), s_begin, s_end, NEAR,
            [&](const Rec &b, const Rec &a) { return drops(b.len == a.len && memcmp(b.msg, a.msg, MAX_BYTES) == 0, b.s, b.q, a.s, a.q); },
            [&](const Rec &a) {
                if (total < max_frames) {
                    memcpy(h_msg + (size_t)total * MAX_BYTES, a.msg, MAX_BYTES);
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

extern "C" int pss_ais_frames(pss_ctx *ctx, const float *d_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                              uint8_t *d_msg, int32_t *d_len, int32_t *d_row, int64_t *d_pos, float *d_score, int32_t *d_count, int max_frames)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = frames_check(ctx, "pss_ais_frames", d_y, n_rows, y_stride, n_buf, buf_index0, n_row, s_begin, s_end, d_msg, d_len, d_row, d_pos, d_score, d_count,
                         max_frames);
    if (r) return r;
    if (s_begin == s_end) {
        PSS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), PSS_STREAM(ctx)));
        return PSS_OK;
    }
    const Reach w = reach_of(s_begin, s_end, n_row);
    const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;
    PssStartList &starts = ctx->starts;   // buffer 0: the tiles' counts, offsets and lists
    PssStartList::Tiles t;
    r = starts.tiles(ctx, n_tiles, "pss_ais_frames tiles", t);
    if (r) return r;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_ais_detect");
    hipLaunchKernelGGL(k_ais_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0,
                       buf_index0 + n_buf, n_row, w.e0, n_ext, tpr, n_tiles, t.count, t.list);
    pss_kernel_end(ctx);
    long n_surv;
    r = starts.total(ctx, t, n_tiles, "k_ais_detect launch", d_count, n_surv);
    if (r || n_surv == 0) return r;
    // buffer 1: the survivors, their payload words, lengths, scores and ranks, their keep flags
    const size_t n = (size_t)n_surv;
    const size_t o_words = sizeof(long) * n, o_len = o_words + sizeof(uint32_t) * REC_WORDS * n, o_score = o_len + sizeof(int) * n,
                 o_rank = o_score + sizeof(float) * n, o_keep = o_rank + sizeof(int) * n;
    r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + n, "pss_ais_frames list");
    if (r) return r;
    char *b1 = reinterpret_cast<char *>(starts.buf[1]);
    long *surv = reinterpret_cast<long *>(b1);
    uint32_t *words = reinterpret_cast<uint32_t *>(b1 + o_words);
    int *len = reinterpret_cast<int *>(b1 + o_len), *rank = reinterpret_cast<int *>(b1 + o_rank);
    float *score = reinterpret_cast<float *>(b1 + o_score);
    uint8_t *keep = reinterpret_cast<uint8_t *>(b1 + o_keep);
    const dim3 lane_grid(PssStartList::list_grid(n_surv, LS_T)), wave_grid(PssStartList::list_grid(n_surv, LS_T / 64));
    starts.gather(ctx, t, n_tiles, surv);   // surv[k] = the k-th survivor as tile * DT_S + its offset in the tile: ascending in (row, s)
    pss_kernel_begin(ctx, "k_ais_walk");
    hipLaunchKernelGGL(k_ais_walk, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0, n_row, surv, n_surv, tpr, w.e0, len, score, words);
    pss_kernel_end(ctx);
    pss_kernel_begin(ctx, "k_ais_keep");
    hipLaunchKernelGGL(k_ais_keep, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, s_begin, s_end, len, score, words, keep);
    pss_kernel_end(ctx);
    starts.rank(ctx, keep, rank, n_surv, d_count);   // the ranks of the kept starts, and the true count
    if (max_frames > 0) {
        pss_kernel_begin(ctx, "k_ais_emit");
        hipLaunchKernelGGL(k_ais_emit, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, keep, rank, len, score, words, max_frames, d_msg, d_len,
                           d_row, d_pos, d_score);
        pss_kernel_end(ctx);
    }
    return pss_hip_check(ctx, hipGetLastError(), "k_ais_emit launch");
}

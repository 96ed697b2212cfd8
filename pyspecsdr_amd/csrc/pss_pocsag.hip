// pss_pocsag.hip — POCSAG: from float32 discriminator rows at 38 400 S/s to the batches whose codewords pass their check.  The arithmetic is
// pss_pocsag.h's; this unit places it.  The front is pss_ais_front's (pss_ais.hip) with a boxcar.
//   k_pocsag_detect  a workgroup walks tiles of DT_S start positions of one row.  The tile's samples and the 31 spb ahead of them go to LDS
//                    once (at most 8064 floats); every lane tests the sync word of consecutive starts (32 LDS reads, consecutive lanes on
//                    consecutive words at every k; a tile without a survivor ends there); ballots and the wavefronts' counts compact the
//                    survivors in ascending order into the tile's own list.
//   pss_starts.h     k_starts_scan and k_starts_gather, shared with pss_adsb.hip and pss_ais.hip: the tiles' counts become offsets and a
//                    total, the tiles' lists are laid back to back, and behind the keep pass the same scan ranks the kept starts and writes
//                    the true count.
//   k_pocsag_walk    one wavefront per survivor: threshold and score again, then the 512 strobes of the 16 codewords, eight a lane; each
//                    ballot hands over two codewords; 16 lanes run the check, and ballots count the bad words and the fixed bits.
//   k_pocsag_keep    one lane per survivor: the accepted starts less than spb away in the same row are its neighbours in the list: the
//                    one-record-per-batch rule.
//   k_pocsag_emit    one wavefront per kept start below max_batches: the record.
// Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_pocsag.h"
#include "pss_ctx.h"
#include "pss_device.h"
#define PSS_STARTS_KERNELS   // this unit launches the list's kernels
#include "pss_starts.h"

namespace {

using namespace pss_pocsag;

constexpr int PD_Y = DT_S + HEAD_K * MAX_SPB;    // samples of a tile at the largest spb: 8064
static_assert(PD_Y == 8064, "the detect tile's LDS");

// where tile `tile` lies: its row and the row index of its first start
__device__ __forceinline__ void tile_at(long tile, long tpr, long e0, long &row, long &g0)
{
    row = tile / tpr;
    g0 = e0 + (tile - row * tpr) * DT_S;
}

__global__ __launch_bounds__(DT_T) void k_pocsag_detect(const float *__restrict__ y, long y_stride, long buf_lo, long buf_hi, long n_row, int spb, int sync_errors,
                                                        long e0, long n_ext, long tpr, long n_tiles, int *__restrict__ tile_count,
                                                        uint16_t *__restrict__ tile_list)
{
    __shared__ float ys[PD_Y];
    __shared__ int wcount[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        long row, g0;
        tile_at(tile, tpr, e0, row, g0);
        const int cnt = e0 + n_ext - g0 < DT_S ? (int)(e0 + n_ext - g0) : DT_S;   // >= 1
        const int ny = cnt + HEAD_K * spb;                                         // <= PD_Y
        // ys[j] = y of row index g0 + j; a sample the buffer does not hold is a zero, and only starts that do not exist read one (the
        // host has checked that the buffer holds [e0, min(n_row, e1 - 1 + 543 spb + 1)))
        for (int j = tid; j < ny; j += DT_T) {
            const long i = g0 + j;
            ys[j] = i >= buf_lo && i < buf_hi ? y[(size_t)row * y_stride + (i - buf_lo)] : 0.0f;
        }
        __syncthreads();
        bool oks[DT_S / DT_T];
        bool any = false;
#pragma unroll
        for (int k = 0; k < DT_S / DT_T; k++) {
            const int j = k * DT_T + tid;
            oks[k] = false;
            if (j < cnt && exists(g0 + j, n_row, spb)) {
                float thr, q;
                int mism;
                bool inv;
                oks[k] = candidate([&](int kk) { return ys[j + spb * kk]; }, sync_errors, thr, q, mism, inv);
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

// cw[16 k ...], fixb[16 k ...]: survivor k's corrected codewords and fixed counts; meta[k], score[k]; ok[k]: accepted
__global__ __launch_bounds__(LS_T) void k_pocsag_walk(const float *__restrict__ y, long y_stride, long buf_lo, const long *__restrict__ surv, long n_surv, long tpr,
                                                      long e0, int spb, int sync_errors, int fix, int max_bad, uint32_t *__restrict__ cw,
                                                      uint8_t *__restrict__ fixb, uint32_t *__restrict__ meta, float *__restrict__ score, uint8_t *__restrict__ ok)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6), n_waves = (long)gridDim.x * (LS_T / 64);
    for (long k = wave; k < n_surv; k += n_waves) {
        long row, s;
        start_at(surv[k], tpr, e0, row, s);
        const float *yr = y + (size_t)row * y_stride + (s - buf_lo);
        float thr, q;
        int mism;
        bool inv;
        candidate([&](int kk) { return yr[(long)spb * kk]; }, sync_errors, thr, q, mism, inv);   // the same in every lane
        // strobe 32 + 64 t + lane: the ballot's low half is codeword 2 t, first strobe first; its high half codeword 2 t + 1
        uint32_t mine = 0;
#pragma unroll
        for (int t = 0; t < N_CW / 2; t++) {
            const unsigned long long high = __ballot(yr[(long)spb * (SYNC_BITS + 64 * t + lane)] > thr);
            const uint32_t half = (lane & 1) ? (uint32_t)(high >> 32) : (uint32_t)high;
            if ((lane >> 1) == t) mine = half;
        }
        // bit l of `mine` is L of the codeword's strobe l: data bit = !L at bit 31 - l
        uint32_t word = __brev(~mine);
        if (inv) word = ~word;
        uint32_t out = 0;
        int n = 0;
        if (lane < N_CW) {
            n = check(word, fix, out);
            cw[(size_t)k * N_CW + lane] = out;
            fixb[(size_t)k * N_CW + lane] = (uint8_t)(n < 0 ? UNCORRECTABLE : n);
        }
        const int n_bad = __popcll(__ballot(n < 0));
        const int n_fixed = __popcll(__ballot(n >= 1)) + __popcll(__ballot(n == 2));
        if (lane == 0) {
            meta[k] = meta_of(mism, inv, n_bad, n_fixed);
            score[k] = q;
            ok[k] = n_bad <= max_bad ? 1 : 0;
        }
    }
}

__device__ __forceinline__ bool same_words(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b)
{
    for (int i = 0; i < N_CW; i++)
        if (a[i] != b[i]) return false;
    return true;
}

__global__ __launch_bounds__(LS_T) void k_pocsag_keep(const long *__restrict__ surv, long n_surv, long tpr, long e0, long s_begin, long s_end, int spb,
                                                      const uint8_t *__restrict__ ok, const float *__restrict__ score, const uint32_t *__restrict__ cw,
                                                      uint8_t *__restrict__ keep)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        long row_a, s_a;
        start_at(surv[k], tpr, e0, row_a, s_a);
        bool kept = ok[k] && s_a >= s_begin && s_a < s_end;
        if (kept) {
            const float q_a = score[k];
            const uint32_t *w_a = cw + (size_t)k * N_CW;
            auto same_as = [&](long q) { return ok[q] && same_words(cw + (size_t)q * N_CW, w_a); };
            for (long q = k - 1; kept && q >= 0; q--) {
                long row_b, s_b;
                start_at(surv[q], tpr, e0, row_b, s_b);
                if (row_b != row_a || s_a - s_b >= spb) break;
                if (drops(same_as(q), s_b, score[q], s_a, q_a, spb)) kept = false;
            }
            for (long q = k + 1; kept && q < n_surv; q++) {
                long row_b, s_b;
                start_at(surv[q], tpr, e0, row_b, s_b);
                if (row_b != row_a || s_b - s_a >= spb) break;
                if (drops(same_as(q), s_b, score[q], s_a, q_a, spb)) kept = false;
            }
        }
        keep[k] = kept ? 1 : 0;
    }
}

__global__ __launch_bounds__(LS_T) void k_pocsag_emit(const long *__restrict__ surv, long n_surv, long tpr, long e0, const uint8_t *__restrict__ keep,
                                                      const int *__restrict__ rank, const uint32_t *__restrict__ cw, const uint8_t *__restrict__ fixb,
                                                      const uint32_t *__restrict__ meta, const float *__restrict__ score, int max_batches,
                                                      uint32_t *__restrict__ d_cw, uint8_t *__restrict__ d_fix, int32_t *__restrict__ d_row,
                                                      int64_t *__restrict__ d_pos, uint32_t *__restrict__ d_meta, float *__restrict__ d_score)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6), n_waves = (long)gridDim.x * (LS_T / 64);
    for (long k = wave; k < n_surv; k += n_waves) {
        if (!keep[k]) continue;
        const int r = rank[k];
        if (r >= max_batches) continue;
        if (lane < N_CW) {
            d_cw[(size_t)r * N_CW + lane] = cw[(size_t)k * N_CW + lane];
            d_fix[(size_t)r * N_CW + lane] = fixb[(size_t)k * N_CW + lane];
        }
        if (lane == 0) {
            long row, s;
            start_at(surv[k], tpr, e0, row, s);
            d_row[r] = (int32_t)row;
            d_pos[r] = s;
            d_meta[r] = meta[k];
            d_score[r] = score[k];
        }
    }
}

int batches_check(pss_ctx *ctx, const void *y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, int spb,
                  int sync_errors, int fix, int max_bad, const void *cw, const void *fixb, const void *row, const void *pos, const void *meta,
                  const void *score, const void *count, int max_batches)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_pocsag_batches: ") + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (n_rows < 1 || n_rows > (1l << 20)) return bad("n_rows outside [1, 2^20]");
    if (spb < MIN_SPB || spb > MAX_SPB) return bad("spb outside [2, 128]");
    if (sync_errors < 0 || sync_errors > MAX_SYNC_ERRORS) return bad("sync_errors outside [0, 2]");
    if (fix < 0 || fix > MAX_FIX) return bad("fix outside [0, 2]");
    if (max_bad < 0 || max_bad > N_CW) return bad("max_bad outside [0, 16]");
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 's', s_begin, s_end, "starts")) return r;
    if (y_stride < n_buf) return bad("y_stride < n_buf");
    if ((s_end - s_begin + 2 * (long)spb) > (1l << 31) / n_rows) return bad("more than 2^31 starts in the rows of one call");
    if (max_batches < 0) return bad("max_batches < 0");
    if (!count || (n_buf > 0 && !y) || (max_batches > 0 && (!cw || !fixb || !row || !pos || !meta || !score))) return bad("null buffer");
    if (off(y, 4) || off(pos, 8) || off(cw, 4) || off(row, 4) || off(meta, 4) || off(score, 4) || off(count, 4)) return bad("a misaligned pointer");
    if (s_begin < s_end) {
        const Reach r = reach_of(s_begin, s_end, n_row, spb);
        if (buf_index0 > r.need_lo || buf_index0 + n_buf < r.need_hi)
            return bad("the buffer does not cover the window's reach (spb - 1 starts either side, 543 spb + 1 samples forward)");
    }
    return PSS_OK;
}

}  // namespace

// ---- plan, pulse, code ------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_pocsag_plan(double fs, int *decim, int *up, int *down)
{
    auto bad = [&](const char *why) { return pss_fail(nullptr, PSS_E_ARG, std::string("pss_pocsag: ") + why); };
    if (!decim || !up || !down) return bad("null argument");
    if (!std::isfinite(fs) || fs != floor(fs) || fs > 0x1p52) return bad("fs must be an integer number of Hz");
    if (!(fs >= (double)RATE)) return bad("fs must be at least 38 400");
    if (!plan((long)fs, *decim, *up, *down)) return bad("38 400 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take");
    return PSS_OK;
}

extern "C" int pss_pocsag_default_pulse(int spb, double *pulse, int *n_pulse)
{
    if (!n_pulse || spb < MIN_SPB || spb > MAX_SPB) return pss_fail(nullptr, PSS_E_ARG, "pss_pocsag_default_pulse: spb outside [2, 128]");
    *n_pulse = pulse_len(spb);
    if (pulse) default_pulse(spb, pulse);
    return PSS_OK;
}

extern "C" uint32_t pss_pocsag_codeword(uint32_t data21) { return codeword(data21); }

extern "C" int pss_pocsag_check(uint32_t cw, int fix, uint32_t *fixed)
{
    uint32_t out = 0;
    const int n = fix < 0 || fix > MAX_FIX ? -1 : check(cw, fix, out);
    if (fixed) *fixed = out;
    return n;
}

// ---- batches ----------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_pocsag_batches(const float *h_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, int spb,
                                    int sync_errors, int fix, int max_bad, uint32_t *h_cw, uint8_t *h_fix, int32_t *h_row, int64_t *h_pos, uint32_t *h_meta,
                                    float *h_score, int32_t *h_count, int max_batches)
{
    const int r = batches_check(nullptr, h_y, n_rows, y_stride, n_buf, buf_index0, n_row, s_begin, s_end, spb, sync_errors, fix, max_bad, h_cw, h_fix, h_row,
                                h_pos, h_meta, h_score, h_count, max_batches);
    if (r) return r;
    struct Rec { long s; float q; uint32_t meta; uint32_t cw[N_CW]; uint8_t fix[N_CW]; };
    int total = 0;
    std::vector<Rec> acc;
    for (long row = 0; row < n_rows && s_begin < s_end; row++) {
        const Reach w = reach_of(s_begin, s_end, n_row, spb);
        const float *yr = h_y + (size_t)row * y_stride;
        acc.clear();
        for (long s = w.e0; s < w.e1; s++) {
            if (!exists(s, n_row, spb)) continue;
            auto Y = [&](int k) { return yr[s + (long)spb * k - buf_index0]; };
            float thr;
            int mism;
            bool inv;
            Rec c;
            if (!candidate(Y, sync_errors, thr, c.q, mism, inv)) continue;
            c.s = s;
            int n_bad = 0, n_fixed = 0;
            for (int j = 0; j < N_CW; j++) {
                const int n = check(received(Y, thr, inv, j), fix, c.cw[j]);
                c.fix[j] = (uint8_t)(n < 0 ? UNCORRECTABLE : n);
                if (n < 0) n_bad++;
                else n_fixed += n;
            }
            c.meta = meta_of(mism, inv, n_bad, n_fixed);
            if (n_bad <= max_bad) acc.push_back(c);
        }
        keep_starts(acc.data(), acc.size(), s_begin, s_end, spb,
            [&](const Rec &b, const Rec &a) { return drops(memcmp(b.cw, a.cw, sizeof(a.cw)) == 0, b.s, b.q, a.s, a.q, spb); },
            [&](const Rec &a) {
                if (total < max_batches) {
                    memcpy(h_cw + (size_t)total * N_CW, a.cw, sizeof(a.cw));
                    memcpy(h_fix + (size_t)total * N_CW, a.fix, sizeof(a.fix));
                    h_row[total] = (int32_t)row;
                    h_pos[total] = a.s;
                    h_meta[total] = a.meta;
                    h_score[total] = a.q;
                }
                total++;
            });
    }
    *h_count = total;
    return PSS_OK;
}

extern "C" int pss_pocsag_batches(pss_ctx *ctx, const float *d_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                                  int spb, int sync_errors, int fix, int max_bad, uint32_t *d_cw, uint8_t *d_fix, int32_t *d_row, int64_t *d_pos,
                                  uint32_t *d_meta, float *d_score, int32_t *d_count, int max_batches)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = batches_check(ctx, d_y, n_rows, y_stride, n_buf, buf_index0, n_row, s_begin, s_end, spb, sync_errors, fix, max_bad, d_cw, d_fix, d_row, d_pos,
                          d_meta, d_score, d_count, max_batches);
    if (r) return r;
    if (s_begin == s_end) {
        PSS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), PSS_STREAM(ctx)));
        return PSS_OK;
    }
    const Reach w = reach_of(s_begin, s_end, n_row, spb);
    const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;
    PssStartList &starts = ctx->starts;   // buffer 0: the tiles' counts, offsets and lists
    PssStartList::Tiles t;
    r = starts.tiles(ctx, n_tiles, "pss_pocsag_batches tiles", t);
    if (r) return r;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_pocsag_detect");
    hipLaunchKernelGGL(k_pocsag_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0,
                       buf_index0 + n_buf, n_row, spb, sync_errors, w.e0, n_ext, tpr, n_tiles, t.count, t.list);
    pss_kernel_end(ctx);
    long n_surv;
    r = starts.total(ctx, t, n_tiles, "k_pocsag_detect launch", d_count, n_surv);
    if (r || n_surv == 0) return r;
    // buffer 1: the survivors, their codewords, metas, scores and ranks, their fixed counts, accept and keep flags
    const size_t n = (size_t)n_surv;
    const size_t o_cw = sizeof(long) * n, o_meta = o_cw + sizeof(uint32_t) * N_CW * n, o_score = o_meta + sizeof(uint32_t) * n,
                 o_rank = o_score + sizeof(float) * n, o_fix = o_rank + sizeof(int) * n, o_ok = o_fix + (size_t)N_CW * n, o_keep = o_ok + n;
    r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + n, "pss_pocsag_batches list");
    if (r) return r;
    char *b1 = reinterpret_cast<char *>(starts.buf[1]);
    long *surv = reinterpret_cast<long *>(b1);
    uint32_t *cw = reinterpret_cast<uint32_t *>(b1 + o_cw), *meta = reinterpret_cast<uint32_t *>(b1 + o_meta);
    float *score = reinterpret_cast<float *>(b1 + o_score);
    int *rank = reinterpret_cast<int *>(b1 + o_rank);
    uint8_t *fixb = reinterpret_cast<uint8_t *>(b1 + o_fix), *ok = reinterpret_cast<uint8_t *>(b1 + o_ok), *keep = reinterpret_cast<uint8_t *>(b1 + o_keep);
    const dim3 lane_grid(PssStartList::list_grid(n_surv, LS_T)), wave_grid(PssStartList::list_grid(n_surv, LS_T / 64));
    starts.gather(ctx, t, n_tiles, surv);   // surv[k] = the k-th survivor as tile * DT_S + its offset in the tile: ascending in (row, s)
    pss_kernel_begin(ctx, "k_pocsag_walk");
    hipLaunchKernelGGL(k_pocsag_walk, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0, surv, n_surv, tpr, w.e0, spb, sync_errors, fix, max_bad,
                       cw, fixb, meta, score, ok);
    pss_kernel_end(ctx);
    pss_kernel_begin(ctx, "k_pocsag_keep");
    hipLaunchKernelGGL(k_pocsag_keep, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, s_begin, s_end, spb, ok, score, cw, keep);
    pss_kernel_end(ctx);
    starts.rank(ctx, keep, rank, n_surv, d_count);   // the ranks of the kept starts, and the true count
    if (max_batches > 0) {
        pss_kernel_begin(ctx, "k_pocsag_emit");
        hipLaunchKernelGGL(k_pocsag_emit, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), surv, n_surv, tpr, w.e0, keep, rank, cw, fixb, meta, score, max_batches, d_cw,
                           d_fix, d_row, d_pos, d_meta, d_score);
        pss_kernel_end(ctx);
    }
    return pss_hip_check(ctx, hipGetLastError(), "k_pocsag_emit launch");
}

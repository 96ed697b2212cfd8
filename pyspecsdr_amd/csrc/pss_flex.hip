// pss_flex.hip — FLEX: from float32 discriminator rows at 38 400 S/s to the frames whose words pass their check.  The arithmetic is
// pss_flex.h's; this unit places it.  The front is pss_ais_front's (pss_ais.hip) with a boxcar.
//   k_flex_detect   a workgroup walks tiles of DT_S start positions of one row.  The values v = y[i] + y[i + h] of the tile and of the
//                   126 h ahead of it go to LDS once, formed as they are staged (12 160 floats at h = 64, the cap: the whole reach is staged,
//                   48 640 bytes, and two workgroups still share a compute unit's LDS); every lane tests the 64 sync bits of consecutive
//                   starts (marker in either polarity, outer code against its complement; a tile without a survivor ends there); ballots
//                   and the wavefronts' counts compact the survivors in ascending order into the tile's own list.
//   pss_starts.h    k_starts_scan and k_starts_gather, unchanged.
//   k_flex_head     one lane per survivor: c, a, the mode, the FIW with its check and its sum, into the list's scratch.
//   k_flex_keep     one lane per survivor, BEFORE the walk: the one-record rule over the accepted neighbours less than 2 h away.  About 2 h
//                   survivors share a frame of 5632 symbols; only the kept one is walked.
//   k_flex_walk     one workgroup per kept start.  Per block of 256 symbols every wavefront's ballot of bit_a / bit_b holds 8 bits of each of
//                   the block's 8 words: 16 lanes pick them by mask, shift and one multiply and store them as a byte of the word in LDS (no
//                   atomics: every byte has one writer).  Then the lanes run the check, ballots count the bad words and the fixed bits,
//                   and the record goes to the list's scratch with an `accepted` byte: n_bad <= max_bad.
//   k_flex_compact  k_starts_scan ranks the accepted bytes and writes the true count; a workgroup per accepted start below max_frames copies
//                   the record to its rank.  (The second of the two ways a frame over max_bad leaves no record: a byte and a compaction.)
// Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_flex.h"
#include "pss_ctx.h"
#include "pss_device.h"
#define PSS_STARTS_KERNELS   // this unit launches the list's kernels
#include "pss_starts.h"

namespace {

using namespace pss_flex;

constexpr int FD_V = DT_S + HEAD_V * MAX_H;      // values of a tile at the largest h: 12160
static_assert(FD_V == 12160 && FD_V * sizeof(float) + 64 * sizeof(int) <= 64 * 1024, "the detect tile's LDS");
constexpr int REC_W = N_PHASES * N_WORDS;        // words of a record: 352
constexpr long FL_LANE_GRID_CAP = 32;            // workgroups of k_flex_head and k_flex_keep: 8192 survivors a pass (about 340 frames' at h = 12)

// where tile `tile` lies: its row and the row index of its first start
__device__ __forceinline__ void tile_at(long tile, long tpr, long e0, long &row, long &g0)
{
    row = tile / tpr;
    g0 = e0 + (tile - row * tpr) * DT_S;
}

__global__ __launch_bounds__(DT_T) void k_flex_detect(const float *__restrict__ y, long y_stride, long buf_lo, long buf_hi, long n_row, int h, int sync_errors,
                                                      long e0, long n_ext, long tpr, long n_tiles, int *__restrict__ tile_count,
                                                      uint16_t *__restrict__ tile_list)
{
    __shared__ float vs[FD_V];
    __shared__ int wcount[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        long row, g0;
        tile_at(tile, tpr, e0, row, g0);
        const int cnt = e0 + n_ext - g0 < DT_S ? (int)(e0 + n_ext - g0) : DT_S;   // >= 1
        const int nv = cnt + HEAD_V * h;                                           // <= FD_V
        // vs[j] = v of row index g0 + j; a sample the buffer does not hold is a zero, and only starts that do not exist read one (the
        // host has checked that the buffer holds [e0, min(n_row, e1 - 1 + 5936 h)))
        const float *yr = y + (size_t)row * y_stride;
        for (int j = tid; j < nv; j += DT_T) {
            const long i = g0 + j, i2 = i + h;
            const float p = i >= buf_lo && i < buf_hi ? yr[i - buf_lo] : 0.0f;
            const float q = i2 >= buf_lo && i2 < buf_hi ? yr[i2 - buf_lo] : 0.0f;
            vs[j] = p + q;
        }
        __syncthreads();
        bool oks[DT_S / DT_T];
        bool any = false;
#pragma unroll
        for (int k = 0; k < DT_S / DT_T; k++) {
            const int j = k * DT_T + tid;
            oks[k] = false;
            if (j < cnt && exists(g0 + j, n_row, h)) {
                float c, a;
                uint32_t A;
                int mark, outer;
                bool inv;
                oks[k] = candidate([&](int kk) { return vs[j + 2 * h * kk]; }, sync_errors, c, a, A, mark, outer, inv);
            }
            any |= oks[k];
        }
        // (this barrier also orders the reads of vs above before the next tile's staging)
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

// the list's scratch, an array per field, n entries each
struct List {
    long *surv;
    float *c, *a;
    uint32_t *fiw, *meta0, *meta1, *words;
    int *rank;
    uint8_t *err, *ok, *keep, *acc, *fix;
};

__global__ __launch_bounds__(LS_T) void k_flex_head(const float *__restrict__ y, long y_stride, long buf_lo, long n_surv, long tpr, long e0, int h, int sync_errors,
                                                    int fix, List L)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        long row, s;
        start_at(L.surv[k], tpr, e0, row, s);
        const float *yr = y + (size_t)row * y_stride + (s - buf_lo);
        Head hd;
        const bool ok = head([&](int o) { return yr[(long)o * h] + yr[(long)o * h + h]; }, sync_errors, fix, hd);
        L.c[k] = hd.c;
        L.a[k] = hd.a;
        L.fiw[k] = hd.fiw;
        L.meta0[k] = meta0_of(hd);
        L.err[k] = (uint8_t)errors_of(hd);
        L.ok[k] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(LS_T) void k_flex_keep(long n_surv, long tpr, long e0, long s_begin, long s_end, int h, List L)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_surv; k += n_lanes) {
        long row_a, s_a;
        start_at(L.surv[k], tpr, e0, row_a, s_a);
        bool kept = L.ok[k] && s_a >= s_begin && s_a < s_end;
        if (kept) {
            const float a_a = L.a[k];
            const int e_a = L.err[k];
            for (long q = k - 1; kept && q >= 0; q--) {
                long row_b, s_b;
                start_at(L.surv[q], tpr, e0, row_b, s_b);
                if (row_b != row_a || s_a - s_b >= 2l * h) break;
                if (L.ok[q] && drops(s_b, L.err[q], L.a[q], s_a, e_a, a_a, h)) kept = false;
            }
            for (long q = k + 1; kept && q < n_surv; q++) {
                long row_b, s_b;
                start_at(L.surv[q], tpr, e0, row_b, s_b);
                if (row_b != row_a || s_b - s_a >= 2l * h) break;
                if (L.ok[q] && drops(s_b, L.err[q], L.a[q], s_a, e_a, a_a, h)) kept = false;
            }
        }
        L.keep[k] = kept ? 1 : 0;
    }
}

// the 8 bits of a ballot that lie 8 lanes apart from lane w on, as a byte: bit i = the ballot's bit w + 8 i
__device__ __forceinline__ uint32_t every_eighth(unsigned long long ballot, int w)
{
    const unsigned long long x = (ballot >> w) & 0x0101010101010101ull;
    return (uint32_t)((x * 0x0102040810204080ull) >> 56);
}

__global__ __launch_bounds__(LS_T) void k_flex_walk(const float *__restrict__ y, long y_stride, long buf_lo, long n_surv, long tpr, long e0, int h, int fix,
                                                    int max_bad, List L)
{
    __shared__ __attribute__((aligned(4))) uint8_t wb[REC_W * 4];   // the record's words, byte q of a word = its bits 8 q .. 8 q + 7
    __shared__ int wsum[LS_T / 64][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    static_assert(LS_T == 256, "a block of 256 symbols is one symbol a thread, and a wavefront's ballot one byte of each of its words");
    for (long k = blockIdx.x; k < n_surv; k += gridDim.x) {
        if (!L.keep[k]) {   // the same in every thread
            if (tid == 0) L.acc[k] = 0;
            continue;
        }
        long row, s;
        start_at(L.surv[k], tpr, e0, row, s);
        const float *yr = y + (size_t)row * y_stride + (s - buf_lo);
        const uint32_t m0 = L.meta0[k];
        Head hd;
        hd.c = L.c[k], hd.a = L.a[k], hd.mode = (int)(m0 >> 12 & 15u), hd.inverted = (m0 >> 8 & 1u) != 0;
        const Slicer z = slicer_of(hd);
        for (int i = tid; i < REC_W; i += LS_T) reinterpret_cast<uint32_t *>(wb)[i] = 0;
        __syncthreads();
        const int n_streams = z.fast ? 2 : 1;
        for (int p = 0; p < n_streams; p++)
            for (int blk = 0; blk < N_BLOCKS; blk++) {
                bool ba, bb;
                symbol([&](long o) { return yr[o]; }, h, z, blk * 256 + tid, p, ba, bb);
                const unsigned long long ma = __ballot(ba), mb = __ballot(bb);
                // lanes 0 .. 7: word `lane` of phase 2 p from bit_a; lanes 8 .. 15: word `lane - 8` of phase 2 p + 1 from bit_b
                if (lane < 8 || (lane < 16 && z.four)) {
                    const int w = lane & 7, phase = 2 * p + (lane >> 3);
                    wb[(phase * N_WORDS + blk * 8 + w) * 4 + wave] = (uint8_t)every_eighth(lane < 8 ? ma : mb, w);
                }
            }
        __syncthreads();
        int n_bad = 0, n_fixed = 0;
#pragma unroll
        for (int u = 0; u < (REC_W + LS_T - 1) / LS_T; u++) {
            const int i = u * LS_T + tid;
            int n = 0;
            if (i < REC_W) {
                uint32_t out = 0;
                if (active(hd.mode, i / N_WORDS)) n = check(reinterpret_cast<const uint32_t *>(wb)[i], fix, out);
                L.words[(size_t)k * REC_W + i] = out;
                L.fix[(size_t)k * REC_W + i] = (uint8_t)(n < 0 ? UNCORRECTABLE : n);
            }
            n_bad += __popcll(__ballot(n < 0));
            n_fixed += __popcll(__ballot(n >= 1)) + __popcll(__ballot(n == 2));
        }
        if (lane == 0) wsum[wave][0] = n_bad, wsum[wave][1] = n_fixed;
        __syncthreads();
        if (tid == 0) {
            int bad = 0, fixed = 0;
            for (int w = 0; w < LS_T / 64; w++) bad += wsum[w][0], fixed += wsum[w][1];
            L.meta1[k] = meta1_of(bad, fixed);
            L.acc[k] = bad <= max_bad ? 1 : 0;
        }
        __syncthreads();   // wb and wsum are read before the next kept start writes them
    }
}

__global__ __launch_bounds__(LS_T) void k_flex_compact(long n_surv, long tpr, long e0, List L, int max_frames, uint32_t *__restrict__ d_words,
                                                       uint8_t *__restrict__ d_fix, uint32_t *__restrict__ d_fiw, int32_t *__restrict__ d_row,
                                                       int64_t *__restrict__ d_pos, uint32_t *__restrict__ d_meta, float *__restrict__ d_score)
{
    for (long k = blockIdx.x; k < n_surv; k += gridDim.x) {
        if (!L.acc[k]) continue;
        const int r = L.rank[k];
        if (r >= max_frames) continue;
        for (int i = threadIdx.x; i < REC_W; i += LS_T) {
            d_words[(size_t)r * REC_W + i] = L.words[(size_t)k * REC_W + i];
            d_fix[(size_t)r * REC_W + i] = L.fix[(size_t)k * REC_W + i];
        }
        if (threadIdx.x == 0) {
            long row, s;
            start_at(L.surv[k], tpr, e0, row, s);
            d_fiw[r] = L.fiw[k];
            d_row[r] = (int32_t)row;
            d_pos[r] = s;
            d_meta[2 * (size_t)r] = L.meta0[k];
            d_meta[2 * (size_t)r + 1] = L.meta1[k];
            d_score[r] = L.a[k];
        }
    }
}

int frames_check(pss_ctx *ctx, const void *y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, int h,
                 int sync_errors, int fix, int max_bad, const void *words, const void *fixb, const void *fiw, const void *row, const void *pos,
                 const void *meta, const void *score, const void *count, int max_frames)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_flex_frames: ") + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (n_rows < 1 || n_rows > (1l << 20)) return bad("n_rows outside [1, 2^20]");
    if (h < MIN_H || h > MAX_H) return bad("h outside [1, 64]");
    if (sync_errors < 0 || sync_errors > MAX_SYNC_ERRORS) return bad("sync_errors outside [0, 3]");
    if (fix < 0 || fix > MAX_FIX) return bad("fix outside [0, 2]");
    if (max_bad < 0 || max_bad > MAX_BAD) return bad("max_bad outside [0, 352]");
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 's', s_begin, s_end, "starts")) return r;
    if (y_stride < n_buf) return bad("y_stride < n_buf");
    if ((s_end - s_begin + 4 * (long)h) > (1l << 31) / n_rows) return bad("more than 2^31 starts in the rows of one call");
    if (max_frames < 0) return bad("max_frames < 0");
    if (!count || (n_buf > 0 && !y) || (max_frames > 0 && (!words || !fixb || !fiw || !row || !pos || !meta || !score))) return bad("null buffer");
    if (off(y, 4) || off(pos, 8) || off(words, 4) || off(fiw, 4) || off(row, 4) || off(meta, 4) || off(score, 4) || off(count, 4))
        return bad("a misaligned pointer");
    if (s_begin < s_end) {
        const Reach r = reach_of(s_begin, s_end, n_row, h);
        if (buf_index0 > r.need_lo || buf_index0 + n_buf < r.need_hi)
            return bad("the buffer does not cover the window's reach (2 h - 1 starts either side, 5936 h samples forward)");
    }
    return PSS_OK;
}

}  // namespace

// ---- pulse, word ------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_flex_default_pulse(int h, double *pulse, int *n_pulse)
{
    if (!n_pulse || h < MIN_H || h > MAX_H) return pss_fail(nullptr, PSS_E_ARG, "pss_flex_default_pulse: h outside [1, 64]");
    *n_pulse = pulse_len(h);
    if (pulse) default_pulse(h, pulse);
    return PSS_OK;
}

extern "C" uint32_t pss_flex_word(uint32_t data21) { return word(data21); }

// ---- frames -----------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_flex_frames(const float *h_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, int h,
                                 int sync_errors, int fix, int max_bad, uint32_t *h_words, uint8_t *h_fix, uint32_t *h_fiw, int32_t *h_row, int64_t *h_pos,
                                 uint32_t *h_meta, float *h_score, int32_t *h_count, int max_frames)
{
    const int r = frames_check(nullptr, h_y, n_rows, y_stride, n_buf, buf_index0, n_row, s_begin, s_end, h, sync_errors, fix, max_bad, h_words, h_fix, h_fiw,
                               h_row, h_pos, h_meta, h_score, h_count, max_frames);
    if (r) return r;
    struct Rec { long s; Head hd; };
    int total = 0;
    std::vector<Rec> acc;
    std::vector<uint32_t> words(REC_W);
    std::vector<uint8_t> fixes(REC_W);
    for (long row = 0; row < n_rows && s_begin < s_end; row++) {
        const Reach w = reach_of(s_begin, s_end, n_row, h);
        const float *yr = h_y + (size_t)row * y_stride;
        acc.clear();
        for (long s = w.e0; s < w.e1; s++) {
            if (!exists(s, n_row, h)) continue;
            Rec c;
            c.s = s;
            if (head([&](int o) { return yr[s + (long)o * h - buf_index0] + yr[s + (long)o * h + h - buf_index0]; }, sync_errors, fix, c.hd)) acc.push_back(c);
        }
        keep_starts(acc.data(), acc.size(), s_begin, s_end, 2l * h,
            [&](const Rec &b, const Rec &a) { return drops(b.s, errors_of(b.hd), b.hd.a, a.s, errors_of(a.hd), a.hd.a, h); },
            [&](const Rec &a) {
                const Slicer z = slicer_of(a.hd);
                std::fill(words.begin(), words.end(), 0u);
                for (int p = 0; p < (z.fast ? 2 : 1); p++)
                    for (int i = 0; i < N_SYM; i++) {
                        bool ba, bb;
                        symbol([&](long o) { return yr[a.s + o - buf_index0]; }, h, z, i, p, ba, bb);
                        const int at = 8 * (i >> 8) + (i & 7), bit = (i & 255) >> 3;
                        if (ba) words[(size_t)(2 * p) * N_WORDS + at] |= 1u << bit;
                        if (bb && z.four) words[(size_t)(2 * p + 1) * N_WORDS + at] |= 1u << bit;
                    }
                int n_bad = 0, n_fixed = 0;
                for (int i = 0; i < REC_W; i++) {
                    int n = 0;
                    uint32_t out = 0;
                    if (active(a.hd.mode, i / N_WORDS)) n = check(words[i], fix, out);
                    words[i] = out;
                    fixes[i] = (uint8_t)(n < 0 ? UNCORRECTABLE : n);
                    if (n < 0) n_bad++;
                    else n_fixed += n;
                }
                if (n_bad > max_bad) return;
                if (total < max_frames) {
                    memcpy(h_words + (size_t)total * REC_W, words.data(), sizeof(uint32_t) * REC_W);
                    memcpy(h_fix + (size_t)total * REC_W, fixes.data(), REC_W);
                    h_fiw[total] = a.hd.fiw;
                    h_row[total] = (int32_t)row;
                    h_pos[total] = a.s;
                    h_meta[2 * (size_t)total] = meta0_of(a.hd);
                    h_meta[2 * (size_t)total + 1] = meta1_of(n_bad, n_fixed);
                    h_score[total] = a.hd.a;
                }
                total++;
            });
    }
    *h_count = total;
    return PSS_OK;
}

extern "C" int pss_flex_frames(pss_ctx *ctx, const float *d_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                               int h, int sync_errors, int fix, int max_bad, uint32_t *d_words, uint8_t *d_fix, uint32_t *d_fiw, int32_t *d_row,
                               int64_t *d_pos, uint32_t *d_meta, float *d_score, int32_t *d_count, int max_frames)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = frames_check(ctx, d_y, n_rows, y_stride, n_buf, buf_index0, n_row, s_begin, s_end, h, sync_errors, fix, max_bad, d_words, d_fix, d_fiw, d_row, d_pos,
                         d_meta, d_score, d_count, max_frames);
    if (r) return r;
    if (s_begin == s_end) {
        PSS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), PSS_STREAM(ctx)));
        return PSS_OK;
    }
    const Reach w = reach_of(s_begin, s_end, n_row, h);
    const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;
    PssStartList &starts = ctx->starts;   // buffer 0: the tiles' counts, offsets and lists
    PssStartList::Tiles t;
    r = starts.tiles(ctx, n_tiles, "pss_flex_frames tiles", t);
    if (r) return r;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_flex_detect");
    hipLaunchKernelGGL(k_flex_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0,
                       buf_index0 + n_buf, n_row, h, sync_errors, w.e0, n_ext, tpr, n_tiles, t.count, t.list);
    pss_kernel_end(ctx);
    long n_surv;
    r = starts.total(ctx, t, n_tiles, "k_flex_detect launch", d_count, n_surv);
    if (r || n_surv == 0) return r;
    // buffer 1, an array per field: the survivors, c, a, FIW, the two meta words, the ranks, the records' words; then the bytes: errors,
    // accepted head, keep, accepted frame, the records' fix bytes
    const size_t n = (size_t)n_surv;
    const size_t o_c = sizeof(long) * n, o_a = o_c + 4 * n, o_fiw = o_a + 4 * n, o_m0 = o_fiw + 4 * n, o_m1 = o_m0 + 4 * n, o_rank = o_m1 + 4 * n,
                 o_words = o_rank + 4 * n, o_err = o_words + 4 * (size_t)REC_W * n, o_ok = o_err + n, o_keep = o_ok + n, o_acc = o_keep + n, o_fix = o_acc + n;
    r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_fix + (size_t)REC_W * n, "pss_flex_frames list");
    if (r) return r;
    char *b1 = reinterpret_cast<char *>(starts.buf[1]);
    List L;
    L.surv = reinterpret_cast<long *>(b1);
    L.c = reinterpret_cast<float *>(b1 + o_c), L.a = reinterpret_cast<float *>(b1 + o_a);
    L.fiw = reinterpret_cast<uint32_t *>(b1 + o_fiw), L.meta0 = reinterpret_cast<uint32_t *>(b1 + o_m0), L.meta1 = reinterpret_cast<uint32_t *>(b1 + o_m1);
    L.rank = reinterpret_cast<int *>(b1 + o_rank);
    L.words = reinterpret_cast<uint32_t *>(b1 + o_words);
    L.err = reinterpret_cast<uint8_t *>(b1 + o_err), L.ok = reinterpret_cast<uint8_t *>(b1 + o_ok), L.keep = reinterpret_cast<uint8_t *>(b1 + o_keep);
    L.acc = reinterpret_cast<uint8_t *>(b1 + o_acc), L.fix = reinterpret_cast<uint8_t *>(b1 + o_fix);
    const long lane_blocks = (n_surv + LS_T - 1) / LS_T;
    const dim3 lane_grid((unsigned)(lane_blocks < FL_LANE_GRID_CAP ? lane_blocks : FL_LANE_GRID_CAP)), group_grid(PssStartList::list_grid(n_surv, 1));
    starts.gather(ctx, t, n_tiles, L.surv);   // surv[k] = the k-th survivor as tile * DT_S + its offset in the tile: ascending in (row, s)
    pss_kernel_begin(ctx, "k_flex_head");
    hipLaunchKernelGGL(k_flex_head, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0, n_surv, tpr, w.e0, h, sync_errors, fix, L);
    pss_kernel_end(ctx);
    pss_kernel_begin(ctx, "k_flex_keep");
    hipLaunchKernelGGL(k_flex_keep, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), n_surv, tpr, w.e0, s_begin, s_end, h, L);
    pss_kernel_end(ctx);
    pss_kernel_begin(ctx, "k_flex_walk");
    hipLaunchKernelGGL(k_flex_walk, group_grid, dim3(LS_T), 0, PSS_STREAM(ctx), d_y, y_stride, buf_index0, n_surv, tpr, w.e0, h, fix, max_bad, L);
    pss_kernel_end(ctx);
    starts.rank(ctx, L.acc, L.rank, n_surv, d_count);   // the ranks of the accepted frames, and the true count
    if (max_frames > 0) {
        pss_kernel_begin(ctx, "k_flex_compact");
        hipLaunchKernelGGL(k_flex_compact, group_grid, dim3(LS_T), 0, PSS_STREAM(ctx), n_surv, tpr, w.e0, L, max_frames, d_words, d_fix, d_fiw, d_row, d_pos,
                           d_meta, d_score);
        pss_kernel_end(ctx);
    }
    return pss_hip_check(ctx, hipGetLastError(), "k_flex_compact launch");
}

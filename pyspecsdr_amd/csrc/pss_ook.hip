// pss_ook.hip — OOK devices: from complex64 rows to the sliced messages of amplitude-keyed bursts.  The arithmetic is pss_ook.h's; this unit
// places it.
//   k_ook_envelope   the stage dump: one lane a sample, m formed on the fly.
//   k_ook_levels     a workgroup a block of 4096 samples: m to LDS once, lane 0 adds it up in ascending order.
//   k_ook_detect     a workgroup walks tiles of DT_S edge positions of one row.  The tile's m and the R + P samples in front of it go to LDS
//                    once (at most 8257 floats); every lane forms e for consecutive positions from there and its scan words; a tile without
//                    a decisive-high sample ends at one __syncthreads_count; otherwise a workgroup max-scan leaves the last decisive
//                    position and its class at every position (uint16 in LDS), on(n) and on(n - 1) follow, and tile_slots compacts the
//                    edges into the tile's ascending list.  A byte per tile keeps the polarity of its first edge: edges alternate.
//   pss_starts.h     k_starts_scan and k_starts_gather, shared with the other receivers: the ordered edge list.
//   k_ook_heads      one lane per listed edge: its row, position and polarity, and whether it starts a message.
//   k_ook_list       the message starts, ranked, as indices into the edge list.
//   k_ook_walk       one wavefront per message, 64 edges a step: the chain of pulses first (one ballot finds where it ends), then the
//                    slicer; bits are placed by a ballot and a popcount prefix, the Manchester half-bit positions by a wavefront prefix sum
//                    carried from step to step.
//   k_ook_emit       one wavefront per reported message below max_msgs: the record.
// Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_ook.h"
#include "pss_ctx.h"
#include "pss_device.h"
#define PSS_STARTS_KERNELS   // this unit launches the list's kernels
#include "pss_starts.h"

namespace {

using namespace pss_ook;

constexpr int OD_HALO = MAX_R + MAX_P;           // samples in front of a tile at the largest R and P: 4161
constexpr int OD_M = DT_S + OD_HALO;             // 8257 floats of m
constexpr int OD_PER = (DT_S + MAX_R + 1 + DT_T - 1) / DT_T;   // scan positions of a lane at the largest R: 9
constexpr int OD_Q = OD_PER * DT_T;              // 9216 scan words
constexpr int LV_T = 256;                        // threads of a levels workgroup
constexpr int EV_T = 256;                        // threads of an envelope workgroup
constexpr long EV_GRID_CAP = 4096, LV_GRID_CAP = 65536;
static_assert(OD_M == 8257 && OD_PER == 9, "the detect tile's LDS");
static_assert(((OD_Q - 1) << 1 | 1) + 1 <= UINT16_MAX, "a scan word is a uint16");

// m of sample i of a row: 0 outside the row and outside the buffer (the host has checked that the buffer holds what is read)
__device__ __forceinline__ float m_at(const float2 *__restrict__ x, long i, long buf_lo, long buf_hi)
{
    if (i < buf_lo || i >= buf_hi) return 0.0f;
    const float2 v = x[i - buf_lo];
    return magnitude(v.x, v.y);
}

__global__ __launch_bounds__(EV_T) void k_ook_envelope(const float2 *__restrict__ iq, long x_stride, long buf_lo, long buf_hi, long n_rows, int P, long i_begin,
                                                       long n_out, float *__restrict__ env, long env_stride)
{
    const long total = n_rows * n_out, n_lanes = (long)gridDim.x * EV_T;
    for (long g = (long)blockIdx.x * EV_T + threadIdx.x; g < total; g += n_lanes) {
        const long row = g / n_out, j = g - row * n_out, n = i_begin + j;
        const float2 *x = iq + (size_t)row * x_stride;
        env[(size_t)row * env_stride + j] = envelope([&](int k) { return m_at(x, n - k, buf_lo, buf_hi); }, P);
    }
}

__global__ __launch_bounds__(LV_T) void k_ook_levels(const float2 *__restrict__ iq, long x_stride, long buf_lo, long n_rows, long b_begin, long n_blocks,
                                                     double *__restrict__ means, long means_stride)
{
    __shared__ float ms[BLOCK];
    const long total = n_rows * n_blocks;
    for (long g = blockIdx.x; g < total; g += gridDim.x) {
        const long row = g / n_blocks, b = g - row * n_blocks;
        const float2 *x = iq + (size_t)row * x_stride + ((b_begin + b) * BLOCK - buf_lo);
        for (int j = threadIdx.x; j < BLOCK; j += LV_T) {
            const float2 v = x[j];
            ms[j] = magnitude(v.x, v.y);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int j = 0; j < BLOCK; j++) s = s + (double)ms[j];
            means[(size_t)row * means_stride + b] = s / (double)BLOCK;
        }
        __syncthreads();
    }
}

// where tile `tile` lies: its row and the row index of its first edge position
__device__ __forceinline__ void tile_at(long tile, long tpr, long e0, long &row, long &g0)
{
    row = tile / tpr;
    g0 = e0 + (tile - row * tpr) * DT_S;
}

// (two workgroups a CU: eight wavefronts a SIMD, so at most 64 VGPRs)
__global__ __launch_bounds__(DT_T, 8) void k_ook_detect(const float2 *__restrict__ iq, long x_stride, long buf_lo, long buf_hi, long n_row, int P, float hi, float lo,
                                                     int R, long e0, long n_ext, long tpr, long n_tiles, int *__restrict__ tile_count,
                                                     uint16_t *__restrict__ tile_list, uint8_t *__restrict__ tile_first)
{
    __shared__ float ms[OD_M];
    __shared__ uint16_t last[OD_Q];
    __shared__ uint32_t wmax[DT_WAVES];
    __shared__ int wcount[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int halo = R + P;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        long row, g0;
        tile_at(tile, tpr, e0, row, g0);
        const int cnt = e0 + n_ext - g0 < DT_S ? (int)(e0 + n_ext - g0) : DT_S;   // >= 1
        // ms[j] = m of row index g0 - halo + j
        const float2 *x = iq + (size_t)row * x_stride;
        const long hi_i = buf_hi < n_row ? buf_hi : n_row;
        for (int j = tid; j < halo + cnt; j += DT_T) ms[j] = m_at(x, g0 - halo + j, buf_lo, hi_i);
        __syncthreads();
        // scan position q is row index g0 - 1 - R + q, whose m is ms[P - 1 + q]; nq = cnt + R + 1 of them, `per` consecutive ones a lane
        const int nq = cnt + R + 1, per = (nq + DT_T - 1) / DT_T;   // per <= OD_PER
        uint32_t run = 0;
        bool high = false;
#pragma unroll
        for (int u = 0; u < OD_PER; u++) {
            const int q = tid * per + u;
            if (u < per && q < nq) {
                const long n = g0 - 1 - R + q;
                if (n >= 0 && n < n_row) {
                    const int code = decisive(envelope([&](int k) { return ms[P - 1 + q - k]; }, P), hi, lo);
                    high |= code == 3;
                    const uint32_t w = scan_word(q, code);
                    run = w > run ? w : run;
                }
                last[q] = (uint16_t)run;   // the lane's own running maximum; the lanes before it are folded in below
            }
        }
        // (this barrier also orders the reads of ms above before the next tile's staging)
        if (__syncthreads_count(high) == 0) {
            if (tid == 0) tile_count[tile] = 0;
            continue;
        }
        // ---- the running maximum over the workgroup: lanes by shuffles, wavefronts through LDS
        uint32_t inc = run;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d);
            if (lane >= d && t > inc) inc = t;
        }
        if (lane == 63) wmax[wave] = inc;
        uint32_t before = __shfl_up(inc, 1);
        if (lane == 0) before = 0;
        __syncthreads();
        for (int w = 0; w < wave; w++) before = wmax[w] > before ? wmax[w] : before;
#pragma unroll
        for (int u = 0; u < OD_PER; u++) {
            const int q = tid * per + u;
            if (u < per && q < nq && before > last[q]) last[q] = (uint16_t)before;
        }
        __syncthreads();
        // ---- the edges
        bool oks[DT_S / DT_T], rises[DT_S / DT_T];
        bool any = false;
#pragma unroll
        for (int k = 0; k < DT_S / DT_T; k++) {
            const int j = k * DT_T + tid;
            oks[k] = rises[k] = false;
            if (j < cnt) {
                const int q = j + R + 1;
                const bool on = g0 + j < n_row && state(last[q], q, R), prev = state(last[q - 1], q - 1, R);
                oks[k] = on != prev;
                rises[k] = on;
            }
            any |= oks[k];
        }
        // (this barrier also orders the reads of `last` above before the next tile's scan)
        if (__syncthreads_count(any) == 0) {
            if (tid == 0) tile_count[tile] = 0;
            continue;
        }
        const int total = tile_slots(oks, wcount, lane, wave, [&](int k, size_t slot) {
            tile_list[(size_t)tile * DT_S + slot] = (uint16_t)(k * DT_T + tid);
            if (slot == 0) tile_first[tile] = rises[k] ? 1 : 0;
        });
        if (tid == 0) tile_count[tile] = total;
        __syncthreads();   // wcount and wmax are read before the next tile with edges writes them
    }
}

// edge k of the list: its row, its position in the row, its polarity (1: a rise)
__device__ __forceinline__ void edge_at(long idx, long k, long tpr, long e0, const int *__restrict__ tile_off, const uint8_t *__restrict__ tile_first, long &row,
                                        long &pos, bool &rise)
{
    const long tile = idx / DT_S;
    long g0;
    tile_at(tile, tpr, e0, row, g0);
    pos = g0 + idx % DT_S;
    rise = (tile_first[tile] ^ (int)((k - tile_off[tile]) & 1)) != 0;
}

__global__ __launch_bounds__(LS_T) void k_ook_heads(const long *__restrict__ idx, long n_edges, long tpr, long e0, const int *__restrict__ tile_off,
                                                    const uint8_t *__restrict__ tile_first, long s_begin, long s_end, long gap_limit,
                                                    long *__restrict__ epos, int *__restrict__ erow, uint8_t *__restrict__ head)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_edges; k += n_lanes) {
        long row, pos;
        bool rise;
        edge_at(idx[k], k, tpr, e0, tile_off, tile_first, row, pos, rise);
        epos[k] = pos;
        erow[k] = (int)row;
        bool h = rise && pos >= s_begin && pos < s_end;
        if (h && k > 0) {
            // the edge before a rise of the same row is a fall
            long row_b, pos_b;
            bool rise_b;
            edge_at(idx[k - 1], k - 1, tpr, e0, tile_off, tile_first, row_b, pos_b, rise_b);
            if (row_b == row && pos - pos_b <= gap_limit) h = false;
        }
        head[k] = h ? 1 : 0;
    }
}

__global__ __launch_bounds__(LS_T) void k_ook_list(const uint8_t *__restrict__ head, const int *__restrict__ rank, long n_edges, int *__restrict__ heads)
{
    const long n_lanes = (long)gridDim.x * LS_T;
    for (long k = (long)blockIdx.x * LS_T + threadIdx.x; k < n_edges; k += n_lanes)
        if (head[k]) heads[rank[k]] = (int)k;
}

// the value of the lane d lanes up, the step's last d lanes taking the next step's first ones from `seam` (held by lanes 0 and 1)
__device__ __forceinline__ long down(long v, long seam, int d, int lane)
{
    const long a = __shfl_down(v, d), b = __shfl(seam, (lane + d) & 63);
    return lane + d < 64 ? a : b;
}

// pbits[32 m ...], pn_bits[m], pspan[m], pmeta[m]: message m's provisional record; keep[m]: reported.  keep is written for every m < n_up.
__global__ __launch_bounds__(LS_T) void k_ook_walk(const long *__restrict__ epos, const int *__restrict__ erow, long n_edges, const int *__restrict__ heads,
                                                   const int32_t *__restrict__ n_heads_p, long n_up, long n_row, long gap_limit, long span, Slicer sl,
                                                   uint8_t *__restrict__ pbits, int32_t *__restrict__ pn_bits, int32_t *__restrict__ pspan,
                                                   uint32_t *__restrict__ pmeta, uint8_t *__restrict__ keep)
{
    __shared__ uint8_t wbit[LS_T / 64][MAX_BITS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long wave = (long)blockIdx.x * (LS_T / 64) + w, n_waves = (long)gridDim.x * (LS_T / 64);
    const long n_heads = *n_heads_p;
    for (long m = wave; m < n_up; m += n_waves) {
        if (m >= n_heads) {
            if (lane == 0) keep[m] = 0;
            continue;
        }
        const long i0 = heads[m];
        const int row = erow[i0];
        const long pos = epos[i0], lim = pos + span;
        auto at = [&](long a) { return a < n_edges && erow[a] == row ? epos[a] : NO_EDGE; };
        // ---- the chain: pulse p has its rise at edge 2 p; an even lane looks at one pulse
        int n = MAX_PULSES;
        uint32_t flags = F_MANY;
        for (int step = 0; step < 2 * MAX_PULSES / 64; step++) {
            const long a = i0 + 64l * step + lane;
            const long v0 = at(a), seam = lane < 2 ? at(a + 64) : 0;
            const long v1 = down(v0, seam, 1, lane), v2 = down(v0, seam, 2, lane);
            const bool fits = v1 < lim, cont = fits && v2 < lim && v2 - v1 <= gap_limit;
            const unsigned long long ends = __ballot(!(lane & 1) && !cont);
            if (ends) {
                const int fl = __ffsll((long long)ends) - 1;
                const int f = __shfl((int)fits, fl);
                n = 32 * step + fl / 2 + f;
                flags = f ? 0u : F_LONG;
                break;
            }
        }
        long last_fall = pos;
        if (n > 0) {
            last_fall = at(i0 + 2l * n - 1);
            if (last_fall == n_row) flags |= F_OPEN;
        }
        // ---- the slicer
        long total = 0, n_odd = 0;   // the same in every lane
        auto place = [&](bool gives, bool bit) {
            const unsigned long long g = __ballot(gives);
            const long q = total + __popcll(g & below);
            if (gives && q < MAX_BITS) wbit[w][q] = (uint8_t)((bit ? 1 : 0) ^ sl.invert);
            total += __popcll(g);
        };
        if (sl.mode == MC) {
            long carry = 0;   // the half-bits before this step
            const long n_sym = 2l * n - 1;
            for (long s0 = 0; s0 < n_sym; s0 += 64) {
                const long s = s0 + lane, a = i0 + s;
                const long v0 = at(a), seam = lane < 2 ? at(a + 64) : 0;
                const long v1 = down(v0, seam, 1, lane), v2 = down(v0, seam, 2, lane);
                const bool in = s < n_sym;
                const int hv = in ? halves(v1 - v0, sl) : 0;
                const unsigned long long bad = __ballot(in && hv == 0);
                const int fb = bad ? __ffsll((long long)bad) - 1 : 64;
                const int k = in && lane < fb ? hv : 0;
                int inc = k;
                for (int d = 1; d < 64; d <<= 1) {
                    const int t = __shfl_up(inc, d);
                    if (lane >= d) inc += t;
                }
                const long c = carry + inc - k;   // this symbol's first half-bit
                const bool next = s + 1 < n_sym && halves(v2 - v1, sl) != 0;   // a symbol follows in the list
                // the one half-bit of this symbol that is the first of a pair
                const long x0 = ((c - sl.phase) & 1) ? c + 1 : c;
                const bool has = k > 0 && x0 < c + k;
                const bool split = has && x0 == c + k - 1;   // the pair's second half-bit is the next symbol's: the levels differ
                place(split && next, !(s & 1));
                n_odd += __popcll(__ballot(has && !split));   // both halves in one symbol: an equal pair
                carry += __shfl(inc, 63);
                if (bad) {
                    n_odd++;
                    break;
                }
            }
        } else {
            const long cnt = sl.mode == PWM ? n : n - 1;
            for (long p0 = 0; p0 < cnt; p0 += 32) {
                const long a = i0 + 2 * p0 + lane;
                const long v0 = at(a), seam = lane < 2 ? at(a + 64) : 0;
                const long v1 = down(v0, seam, 1, lane), v2 = down(v0, seam, 2, lane);
                const bool in = !(lane & 1) && p0 + lane / 2 < cnt;
                const int c = cls(sl.mode == PWM ? v1 - v0 : v2 - v1, sl);
                place(in && (c == C_SHORT || c == C_LONG), sl.mode == PWM ? c == C_SHORT : c == C_LONG);
                n_odd += __popcll(__ballot(in && c == C_ODD));
            }
        }
        if (total > MAX_BITS) flags |= F_FULL;
        const int n_bits = (int)(total < MAX_BITS ? total : MAX_BITS);
        // the wavefront's own bytes in LDS: written above, read below by other lanes of the same wavefront
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < BITS_BYTES) {
            uint32_t byte = 0;
            for (int u = 0; u < 8; u++)
                if (8 * lane + u < n_bits && wbit[w][8 * lane + u]) byte |= 0x80u >> u;
            pbits[(size_t)m * BITS_BYTES + lane] = (uint8_t)byte;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();   // read before the next message's bits are written
        if (lane == 0) {
            pn_bits[m] = n_bits;
            pspan[m] = (int32_t)(last_fall - pos);
            pmeta[m] = meta_of(n, n_odd, flags);
            keep[m] = reported(n_bits, n_odd, sl) ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(LS_T) void k_ook_emit(const long *__restrict__ epos, const int *__restrict__ erow, const int *__restrict__ heads,
                                                   const int32_t *__restrict__ n_heads_p, const uint8_t *__restrict__ keep, const int *__restrict__ rank,
                                                   const uint8_t *__restrict__ pbits, const int32_t *__restrict__ pn_bits, const int32_t *__restrict__ pspan,
                                                   const uint32_t *__restrict__ pmeta, int max_msgs, uint8_t *__restrict__ d_bits, int32_t *__restrict__ d_n_bits,
                                                   int32_t *__restrict__ d_row, int64_t *__restrict__ d_pos, int32_t *__restrict__ d_span,
                                                   uint32_t *__restrict__ d_meta)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6), n_waves = (long)gridDim.x * (LS_T / 64);
    const long n_heads = *n_heads_p;
    for (long m = wave; m < n_heads; m += n_waves) {
        if (!keep[m]) continue;
        const int r = rank[m];
        if (r >= max_msgs) continue;
        if (lane < BITS_BYTES) d_bits[(size_t)r * BITS_BYTES + lane] = pbits[(size_t)m * BITS_BYTES + lane];
        if (lane == 0) {
            const long i0 = heads[m];
            d_n_bits[r] = pn_bits[m];
            d_row[r] = erow[i0];
            d_pos[r] = epos[i0];
            d_span[r] = pspan[m];
            d_meta[r] = pmeta[m];
        }
    }
}

// ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
bool off(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

int rows_check(pss_ctx *ctx, const char *entry, const void *iq, long n_rows, long x_stride, long n_buf)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(entry) + ": " + why); };
    if (n_rows < 1 || n_rows > (1l << 20)) return bad("n_rows outside [1, 2^20]");
    if (x_stride < n_buf) return bad("x_stride < n_buf");
    if (n_buf > 0 && !iq) return bad("null buffer");
    if (off(iq, 8)) return bad("a misaligned pointer");
    return PSS_OK;
}

int envelope_check(pss_ctx *ctx, const void *iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, int P, long i_begin, long i_end,
                   const void *env, long env_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_ook_envelope: ") + why); };
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 'i', i_begin, i_end, "samples")) return r;
    if (P < 1 || P > MAX_P) return bad("P outside [1, 65]");
    if (const int r = rows_check(ctx, "pss_ook_envelope", iq, n_rows, x_stride, n_buf)) return r;
    if (env_stride < i_end - i_begin) return bad("env_stride < i_end - i_begin");
    if (i_begin < i_end && !env) return bad("null buffer");
    if (off(env, 4)) return bad("a misaligned pointer");
    if (i_begin < i_end && (buf_index0 > (i_begin - (P - 1) < 0 ? 0 : i_begin - (P - 1)) || buf_index0 + n_buf < i_end))
        return bad("the buffer does not cover the window's reach (P - 1 samples back)");
    return PSS_OK;
}

int levels_check(pss_ctx *ctx, const void *iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long b_begin, long b_end,
                 const void *means, long means_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_ook_levels: ") + why); };
    if (n_row < 0 || n_row > (1l << 60)) return bad("n_row outside [0, 2^60]");
    if (n_buf < 0 || buf_index0 < 0 || buf_index0 > n_row || n_buf > n_row - buf_index0) return bad("the buffer does not lie inside the row");
    if (b_end < b_begin) return bad("b_end < b_begin");
    if (b_begin < 0 || b_end > n_row / BLOCK) return bad("the window does not lie inside the row's whole blocks");
    if (const int r = rows_check(ctx, "pss_ook_levels", iq, n_rows, x_stride, n_buf)) return r;
    if (means_stride < b_end - b_begin) return bad("means_stride < b_end - b_begin");
    if (b_begin < b_end && !means) return bad("null buffer");
    if (off(means, 8)) return bad("a misaligned pointer");
    if (b_begin < b_end && (buf_index0 > b_begin * BLOCK || buf_index0 + n_buf < b_end * BLOCK)) return bad("the buffer does not cover the window's blocks");
    return PSS_OK;
}

struct Detect { int P; float hi, lo; int R; long gap_limit, span; };

int messages_check(pss_ctx *ctx, const void *iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, const Detect &d,
                   const Slicer &sl, const void *bits, const void *n_bits, const void *row, const void *pos, const void *span, const void *meta,
                   const void *count, int max_msgs)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string("pss_ook_messages: ") + why); };
    if (const int r = window_refusals(bad, "row", n_row, n_buf, buf_index0, 's', s_begin, s_end, "starts")) return r;
    if (const int r = rows_check(ctx, "pss_ook_messages", iq, n_rows, x_stride, n_buf)) return r;
    if (d.P < 1 || d.P > MAX_P) return bad("P outside [1, 65]");
    if (d.R < 0 || d.R > MAX_R) return bad("R outside [0, 4096]");
    if (!(d.hi >= d.lo && d.lo > 0.0f)) return bad("the thresholds must satisfy hi >= lo > 0");
    if (d.gap_limit < 1 || d.gap_limit > MAX_GAP) return bad("gap_limit outside [1, 2^20]");
    if (d.span < 1 || d.span > MAX_SPAN) return bad("span outside [1, 2^24]");
    if (const char *why = slicer_refusal(sl)) return bad(why);
    if ((s_end - s_begin + d.gap_limit + d.span) > (1l << 31) / n_rows) return bad("more than 2^31 edge positions in the rows of one call");
    if (max_msgs < 0) return bad("max_msgs < 0");
    if (!count || (max_msgs > 0 && (!bits || !n_bits || !row || !pos || !span || !meta))) return bad("null buffer");
    if (off(pos, 8) || off(n_bits, 4) || off(row, 4) || off(span, 4) || off(meta, 4) || off(count, 4)) return bad("a misaligned pointer");
    if (s_begin < s_end) {
        const Reach r = reach_of(s_begin, s_end, n_row, d.P, d.R, d.gap_limit, d.span);
        if (buf_index0 > r.need_lo || buf_index0 + n_buf < r.need_hi)
            return bad("the buffer does not cover the window's reach (gap_limit + R + P samples back, span samples forward)");
    }
    return PSS_OK;
}

}  // namespace

// ---- halo -------------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_ook_halo(int P, int R, long gap_limit, long span, long *before, long *after)
{
    auto bad = [&](const char *why) { return pss_fail(nullptr, PSS_E_ARG, std::string("pss_ook_halo: ") + why); };
    if (!before || !after) return bad("null argument");
    if (P < 1 || P > MAX_P) return bad("P outside [1, 65]");
    if (R < 0 || R > MAX_R) return bad("R outside [0, 4096]");
    if (gap_limit < 1 || gap_limit > MAX_GAP) return bad("gap_limit outside [1, 2^20]");
    if (span < 1 || span > MAX_SPAN) return bad("span outside [1, 2^24]");
    *before = halo_before(P, R, gap_limit);
    *after = halo_after(span);
    return PSS_OK;
}

// ---- envelope ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_ook_envelope(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, int P, long i_begin, long i_end,
                                  float *h_env, long env_stride)
{
    const int r = envelope_check(nullptr, h_iq, n_rows, x_stride, n_buf, buf_index0, n_row, P, i_begin, i_end, h_env, env_stride);
    if (r) return r;
    for (long row = 0; row < n_rows; row++) {
        const float *x = h_iq + 2 * (size_t)row * x_stride;
        for (long n = i_begin; n < i_end; n++)
            h_env[(size_t)row * env_stride + (n - i_begin)] = envelope(
                [&](int k) { return n - k >= 0 ? magnitude(x[2 * (n - k - buf_index0)], x[2 * (n - k - buf_index0) + 1]) : 0.0f; }, P);
    }
    return PSS_OK;
}

extern "C" int pss_ook_envelope(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, int P, long i_begin,
                                long i_end, float *d_env, long env_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    const int r = envelope_check(ctx, d_iq, n_rows, x_stride, n_buf, buf_index0, n_row, P, i_begin, i_end, d_env, env_stride);
    if (r) return r;
    if (i_begin == i_end) return PSS_OK;
    const long total = n_rows * (i_end - i_begin), blocks = (total + EV_T - 1) / EV_T;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_ook_envelope");
    hipLaunchKernelGGL(k_ook_envelope, dim3((unsigned)(blocks < EV_GRID_CAP ? blocks : EV_GRID_CAP)), dim3(EV_T), 0, PSS_STREAM(ctx),
                       reinterpret_cast<const float2 *>(d_iq), x_stride, buf_index0, buf_index0 + n_buf, n_rows, P, i_begin, i_end - i_begin, d_env, env_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_ook_envelope launch");
}

// ---- levels -----------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_ook_levels(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long b_begin, long b_end,
                                double *h_means, long means_stride)
{
    const int r = levels_check(nullptr, h_iq, n_rows, x_stride, n_buf, buf_index0, n_row, b_begin, b_end, h_means, means_stride);
    if (r) return r;
    for (long row = 0; row < n_rows; row++)
        for (long b = b_begin; b < b_end; b++) {
            const float *x = h_iq + 2 * ((size_t)row * x_stride + (b * BLOCK - buf_index0));
            double s = 0.0;
            for (int j = 0; j < BLOCK; j++) s = s + (double)magnitude(x[2 * j], x[2 * j + 1]);
            h_means[(size_t)row * means_stride + (b - b_begin)] = s / (double)BLOCK;
        }
    return PSS_OK;
}

extern "C" int pss_ook_levels(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long b_begin, long b_end,
                              double *d_means, long means_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    const int r = levels_check(ctx, d_iq, n_rows, x_stride, n_buf, buf_index0, n_row, b_begin, b_end, d_means, means_stride);
    if (r) return r;
    if (b_begin == b_end) return PSS_OK;
    const long total = n_rows * (b_end - b_begin);
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_ook_levels");
    hipLaunchKernelGGL(k_ook_levels, dim3((unsigned)(total < LV_GRID_CAP ? total : LV_GRID_CAP)), dim3(LV_T), 0, PSS_STREAM(ctx),
                       reinterpret_cast<const float2 *>(d_iq), x_stride, buf_index0, n_rows, b_begin, b_end - b_begin, d_means, means_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_ook_levels launch");
}

// ---- messages ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_ook_messages(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, int P,
                                  float hi, float lo, int R, long gap_limit, long span, int mode, int w_short, int w_long, int w_sync, int tol, int phase,
                                  int invert, int min_bits, int max_odd, uint8_t *h_bits, int32_t *h_n_bits, int32_t *h_row, int64_t *h_pos, int32_t *h_span,
                                  uint32_t *h_meta, int32_t *h_count, int max_msgs)
{
    const Detect d = {P, hi, lo, R, gap_limit, span};
    const Slicer sl = {mode, w_short, w_long, w_sync, tol, phase, invert, min_bits, max_odd};
    const int r = messages_check(nullptr, h_iq, n_rows, x_stride, n_buf, buf_index0, n_row, s_begin, s_end, d, sl, h_bits, h_n_bits, h_row, h_pos, h_span,
                                 h_meta, h_count, max_msgs);
    if (r) return r;
    int total = 0;
    std::vector<long> edges;   // a row's edges in [e0, e1), alternating
    for (long row = 0; row < n_rows && s_begin < s_end; row++) {
        const Reach w = reach_of(s_begin, s_end, n_row, P, R, gap_limit, span);
        const float *x = h_iq + 2 * (size_t)row * x_stride;
        edges.clear();
        bool first_rise = false;
        row_edges([&](long i) { return magnitude(x[2 * (i - buf_index0)], x[2 * (i - buf_index0) + 1]); }, n_row, w.e0, w.e1, P, hi, lo, R,
                  [&](long n, bool rise) {
                      if (edges.empty()) first_rise = rise;
                      edges.push_back(n);
                  });
        const long n_edges = (long)edges.size();
        for (long k = first_rise ? 0 : 1; k < n_edges; k += 2) {
            const long pos = edges[k];
            if (pos < s_begin || pos >= s_end) continue;
            if (k > 0 && pos - edges[k - 1] <= gap_limit) continue;
            const Message msg = walk([&](long a) { return k + a < n_edges ? edges[k + a] : NO_EDGE; }, pos, span, gap_limit, n_row, sl);
            if (!reported(msg.n_bits, msg.n_odd, sl)) continue;
            if (total < max_msgs) {
                memcpy(h_bits + (size_t)total * BITS_BYTES, msg.bits, BITS_BYTES);
                h_n_bits[total] = msg.n_bits;
                h_row[total] = (int32_t)row;
                h_pos[total] = pos;
                h_span[total] = (int32_t)msg.span;
                h_meta[total] = meta_of(msg.n_pulses, msg.n_odd, msg.flags);
            }
            total++;
        }
    }
    *h_count = total;
    return PSS_OK;
}

extern "C" int pss_ook_messages(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                                int P, float hi, float lo, int R, long gap_limit, long span, int mode, int w_short, int w_long, int w_sync, int tol, int phase,
                                int invert, int min_bits, int max_odd, uint8_t *d_bits, int32_t *d_n_bits, int32_t *d_row, int64_t *d_pos, int32_t *d_span,
                                uint32_t *d_meta, int32_t *d_count, int max_msgs)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    const Detect d = {P, hi, lo, R, gap_limit, span};
    const Slicer sl = {mode, w_short, w_long, w_sync, tol, phase, invert, min_bits, max_odd};
    int r = messages_check(ctx, d_iq, n_rows, x_stride, n_buf, buf_index0, n_row, s_begin, s_end, d, sl, d_bits, d_n_bits, d_row, d_pos, d_span, d_meta, d_count,
                           max_msgs);
    if (r) return r;
    if (s_begin == s_end) {
        PSS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), PSS_STREAM(ctx)));
        return PSS_OK;
    }
    const Reach w = reach_of(s_begin, s_end, n_row, P, R, gap_limit, span);
    const long n_ext = w.e1 - w.e0, tpr = (n_ext + DT_S - 1) / DT_S, n_tiles = tpr * n_rows;
    PssStartList &starts = ctx->starts;   // buffer 0: the tiles' counts, offsets and lists
    PssStartList::Tiles t;
    r = starts.tiles(ctx, n_tiles, "pss_ook_messages tiles", t);
    if (r) return r;
    r = pss_ensure_buffer(ctx, &ctx->ook_first, &ctx->ook_first_bytes, (size_t)n_tiles, "pss_ook_messages tile polarities");
    if (r) return r;
    uint8_t *tile_first = reinterpret_cast<uint8_t *>(ctx->ook_first);
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_ook_detect");
    hipLaunchKernelGGL(k_ook_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx),
                       reinterpret_cast<const float2 *>(d_iq), x_stride, buf_index0, buf_index0 + n_buf, n_row, P, hi, lo, R, w.e0, n_ext, tpr, n_tiles, t.count, t.list,
                       tile_first);
    pss_kernel_end(ctx);
    long n_edges;
    r = starts.total(ctx, t, n_tiles, "k_ook_detect launch", d_count, n_edges);
    if (r || n_edges == 0) return r;
    // buffer 1: per edge its list index, position, row, rank and head flag; per possible message its place in the edge list, its provisional
    // record, its rank and keep flag; the count of messages.  A row's listed edges alternate, so at most every other one and one more a row
    // is a rise (a row's list may end on a rise whose fall lies past the listed range): that many messages there can be, never more than edges.
    const size_t n = (size_t)n_edges, nm = (n + (size_t)n_rows) / 2 < n ? (n + (size_t)n_rows) / 2 : n;
    const size_t o_epos = sizeof(long) * n, o_erow = o_epos + sizeof(long) * n, o_rank = o_erow + sizeof(int) * n, o_heads = o_rank + sizeof(int) * n,
                 o_nbits = o_heads + sizeof(int) * nm, o_span = o_nbits + sizeof(int32_t) * nm, o_meta = o_span + sizeof(int32_t) * nm,
                 o_rank2 = o_meta + sizeof(uint32_t) * nm, o_nheads = o_rank2 + sizeof(int) * nm, o_pbits = o_nheads + 16, o_head = o_pbits + BITS_BYTES * nm,
                 o_keep = o_head + n;
    r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + nm, "pss_ook_messages list");
    if (r) return r;
    char *b1 = reinterpret_cast<char *>(starts.buf[1]);
    long *idx = reinterpret_cast<long *>(b1), *epos = reinterpret_cast<long *>(b1 + o_epos);
    int *erow = reinterpret_cast<int *>(b1 + o_erow), *rank = reinterpret_cast<int *>(b1 + o_rank), *heads = reinterpret_cast<int *>(b1 + o_heads);
    int32_t *pn_bits = reinterpret_cast<int32_t *>(b1 + o_nbits), *pspan = reinterpret_cast<int32_t *>(b1 + o_span);
    uint32_t *pmeta = reinterpret_cast<uint32_t *>(b1 + o_meta);
    int *rank2 = reinterpret_cast<int *>(b1 + o_rank2);
    int32_t *n_heads = reinterpret_cast<int32_t *>(b1 + o_nheads);
    uint8_t *pbits = reinterpret_cast<uint8_t *>(b1 + o_pbits), *head = reinterpret_cast<uint8_t *>(b1 + o_head), *keep = reinterpret_cast<uint8_t *>(b1 + o_keep);
    const dim3 lane_grid(PssStartList::list_grid(n_edges, LS_T)), wave_grid(PssStartList::list_grid((long)nm, LS_T / 64));
    starts.gather(ctx, t, n_tiles, idx);   // idx[k] = the k-th edge as tile * DT_S + its offset in the tile: ascending in (row, position)
    pss_kernel_begin(ctx, "k_ook_heads");
    hipLaunchKernelGGL(k_ook_heads, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), idx, n_edges, tpr, w.e0, t.off, tile_first, s_begin, s_end, gap_limit, epos, erow, head);
    pss_kernel_end(ctx);
    starts.rank(ctx, head, rank, n_edges, n_heads);   // the ranks of the message starts, and their count
    pss_kernel_begin(ctx, "k_ook_list");
    hipLaunchKernelGGL(k_ook_list, lane_grid, dim3(LS_T), 0, PSS_STREAM(ctx), head, rank, n_edges, heads);
    pss_kernel_end(ctx);
    pss_kernel_begin(ctx, "k_ook_walk");
    hipLaunchKernelGGL(k_ook_walk, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), epos, erow, n_edges, heads, n_heads, (long)nm, n_row, gap_limit, span, sl, pbits,
                       pn_bits, pspan, pmeta, keep);
    pss_kernel_end(ctx);
    starts.rank(ctx, keep, rank2, (long)nm, d_count);   // the ranks of the reported messages, and the true count
    if (max_msgs > 0) {
        pss_kernel_begin(ctx, "k_ook_emit");
        hipLaunchKernelGGL(k_ook_emit, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), epos, erow, heads, n_heads, keep, rank2, pbits, pn_bits, pspan, pmeta, max_msgs,
                           d_bits, d_n_bits, d_row, d_pos, d_span, d_meta);
        pss_kernel_end(ctx);
    }
    return pss_hip_check(ctx, hipGetLastError(), "k_ook_emit launch");
}

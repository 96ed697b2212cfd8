// pss_squelch.h — device code of the squelch path (pss_squelch.hip): the header's Peak / Avg meter over float64 rows, the squelch gate
// over the rows' peaks, and the gather of the open frames in front of the demodulator; and the scanner's gate, built the same way.
//
// Reference: draw_header sets PEAK_POWER = np.max(freq_data) and prints np.mean(freq_data) beside it (pyspecsdr.py:388-392), on every
// third loop iteration (:2288-2291); the loop demodulates a read buffer only if PEAK_POWER >= SQUELCH (:2261-2263); PEAK_POWER starts at
// 0, SQUELCH at -60 (:171-172).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "pss_npsum.h"

namespace pss_sq {

// ---- row meter ------------------------------------------------------------------------------------------------------------------------
// np.mean of a float64 row is add.reduce / len: NumPy's pairwise sum (pss_npsum.h states the rule and builds the tables).  Every addition
// is fixed; what is free is WHO performs it.  Here 8 lanes share a leaf block, lane j holding accumulator j (a wave reads 8 segments of
// 64 contiguous bytes per load instruction) and taking np.max in the same walk, the fold is three xor shuffles, the leaf sums go to LDS
// and the tree above them is added level by level.
// The tree of one chunk length is the same for every row, so the host builds it once per call (MeterPlan, passed by value).
using pss_np::CHUNK;            // NumPy's reduction buffer, in elements
using pss_np::LEAF;             // PW_BLOCKSIZE
constexpr int MAX_LEAVES = 128; // a chunk of <= 8192 elements has at most 128 leaf blocks (depth <= 7, no leaf below depth-6 blocks of > 128)

struct MeterPlan {
    uint16_t leaf_off[MAX_LEAVES];   // leaf blocks in element order: offset inside the chunk, length (1 .. 128)
    uint8_t leaf_len[MAX_LEAVES];
    uint8_t node_l[MAX_LEAVES];      // inner node k (value slot n_leaves + k) = slot node_l[k] + slot node_r[k]; sorted by height
    uint8_t node_r[MAX_LEAVES];
    uint8_t level_start[12];         // inner nodes of height h + 1: [level_start[h], level_start[h + 1])
    int n_leaves, n_levels, root;    // root: value slot of the chunk's sum
};
struct MeterPlans {
    MeterPlan full;   // a chunk of 8192 elements (rows longer than 8192)
    MeterPlan tail;   // the last, shorter chunk — or the whole row when len <= 8192
    int n_full;       // chunks that use `full`
    int n_chunks;
};

// host side: the pairwise tree of one chunk of n <= 8192 elements, pss_np::build_forest's tables in the compact by-value form
inline void fill_plan(int n, MeterPlan &p)
{
    const pss_np::Forest f = pss_np::build_forest(n);
    p = MeterPlan{};
    std::copy(f.leaf_off.begin(), f.leaf_off.end(), p.leaf_off);
    std::copy(f.leaf_len.begin(), f.leaf_len.end(), p.leaf_len);
    std::copy(f.node_l.begin(), f.node_l.end(), p.node_l);
    std::copy(f.node_r.begin(), f.node_r.end(), p.node_r);
    std::copy(f.level_start.begin(), f.level_start.end(), p.level_start);
    p.n_leaves = f.n_leaves();
    p.n_levels = f.n_levels;
    p.root = f.roots[0];
}

__device__ __forceinline__ double nan_max(double a, double b)   // np.max's step: a NaN wins
{
    return (b > a || b != b) ? b : a;
}

// G lanes per row: 64 (one wavefront per row, four rows per workgroup) or 256 (one workgroup per row)
template <int G>
__global__ __launch_bounds__(256) void k_row_meter(const double *__restrict__ rows, long n_rows, int len, const MeterPlans plans,
                                                   double *__restrict__ peak, double *__restrict__ avg)
{
    constexpr int RPW = 256 / G, SLOTS = G / 8;
    constexpr int PLAN_WORDS = (int)(sizeof(MeterPlan) / 4);
    static_assert(sizeof(MeterPlan) % 4 == 0, "copied word by word");
    __shared__ int pl_words[2][PLAN_WORDS];
    __shared__ double val[RPW][2 * MAX_LEAVES];
    __shared__ double red[256];
    {
        const int *src = reinterpret_cast<const int *>(&plans);   // `full` then `tail`, contiguous
        for (int i = threadIdx.x; i < 2 * PLAN_WORDS; i += 256) (&pl_words[0][0])[i] = src[i];
    }
    __syncthreads();
    const int slot = threadIdx.x / G, t = threadIdx.x % G, j = t & 7, ls = t >> 3;
    for (long base = (long)blockIdx.x * RPW; base < n_rows; base += (long)gridDim.x * RPW) {
        const long row = base + slot;
        const bool live = row < n_rows;
        const double *x = rows + (size_t)(live ? row : 0) * len;
        double m = -__builtin_inf(), acc = 0.0;
        for (int c = 0; c < plans.n_chunks; c++) {
            const MeterPlan &p = *reinterpret_cast<const MeterPlan *>(pl_words[c < plans.n_full ? 0 : 1]);
            const double *xc = x + (size_t)c * CHUNK;
            for (int l0 = 0; l0 < p.n_leaves; l0 += SLOTS) {
                const int l = l0 + ls;
                const bool has = live && l < p.n_leaves;
                const int ll = has ? p.leaf_len[l] : 0;
                const double *xl = xc + (has ? p.leaf_off[l] : 0);
                const int n8 = ll - (ll & 7);
                double v[LEAF / 8];
#pragma unroll
                for (int k = 0; k < LEAF / 8; k++) v[k] = 8 * k < n8 ? xl[8 * k + j] : 0.0;
                double r = v[0];
                if (n8 > 0) m = nan_max(m, r);
#pragma unroll
                for (int k = 1; k < LEAF / 8; k++)
                    if (8 * k < n8) {
                        r = __dadd_rn(r, v[k]);
                        m = nan_max(m, v[k]);
                    }
                // the leaf's fold ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) of pss_npsum.h (fold_acc), accumulator j in lane j: three xor shuffles
                r = __dadd_rn(r, __shfl_xor(r, 1));
                r = __dadd_rn(r, __shfl_xor(r, 2));
                r = __dadd_rn(r, __shfl_xor(r, 4));
                if (n8 == 0) r = 0.0;
                for (int i = n8; i < ll; i++) {   // the last len % 8 elements (or all of a block shorter than 8), one by one
                    const double e = xl[i];
                    r = __dadd_rn(r, e);
                    m = nan_max(m, e);
                }
                if (has && j == 0) val[slot][l] = r;
            }
            __syncthreads();
            for (int lv = 0; lv < p.n_levels; lv++) {
                for (int k = p.level_start[lv] + t; k < p.level_start[lv + 1]; k += G)
                    val[slot][p.n_leaves + k] = __dadd_rn(val[slot][p.node_l[k]], val[slot][p.node_r[k]]);
                __syncthreads();
            }
            if (t == 0) acc = c == 0 ? val[slot][p.root] : __dadd_rn(acc, val[slot][p.root]);
            __syncthreads();
        }
        red[threadIdx.x] = m;
        __syncthreads();
        for (int st = G / 2; st > 0; st >>= 1) {
            if (t < st) red[threadIdx.x] = nan_max(red[threadIdx.x], red[threadIdx.x + st]);
            __syncthreads();
        }
        if (t == 0 && live) {
            if (peak) peak[row] = red[threadIdx.x];
            if (avg) avg[row] = __ddiv_rn(acc, (double)len);
        }
        __syncthreads();
    }
}

// ---- gate -----------------------------------------------------------------------------------------------------------------------------
// Frame i of a batch is loop iteration i; the counter (ui_update_counter modulo `every`) stands at `phase` before frame 0.  A frame is
// metered if the incremented counter is a multiple of `every`, i.e. frame j with (phase + j + 1) % every == 0, and the value the gate of
// frame i compares is the peak of the last metered frame before i, or held_in if there is none: no serial scan.
__device__ __forceinline__ double gate_held(const double *__restrict__ peak, long i, long phase, int every, double held_in)
{
    if (every <= 0) return held_in;
    const long j = i - (phase + i) % every - 1;
    return j >= 0 ? peak[j] : held_in;
}

constexpr int GATE_TILE = 256;   // frames per workgroup pass

struct GateResult {   // what pss_squelch_gate hands to the host
    long n_open;
    double held_out;
};

// flags of every frame (d_open, nullable) and the number of open frames per tile of 256
__global__ __launch_bounds__(256) void k_gate_flags(const double *__restrict__ peak, long n_frames, double squelch, int every, long phase, double held_in,
                                                    uint8_t *__restrict__ d_open, int *__restrict__ tile_count, long n_tiles)
{
    __shared__ int wcount[4];
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long i = tile * GATE_TILE + threadIdx.x;
        const bool open = i < n_frames && gate_held(peak, i, phase, every, held_in) >= squelch;   // a NaN compares false: closed
        if (i < n_frames && d_open) d_open[i] = open ? 1 : 0;
        const unsigned long long b = __ballot(open);
        if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = __popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) tile_count[tile] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
}

// exclusive prefix sum of the tile counts in place (one workgroup, 256 tiles per step with a carry), the total and the carry-out
__global__ __launch_bounds__(256) void k_gate_scan(int *__restrict__ tile_count, long n_tiles, const double *__restrict__ peak, long n_frames, int every,
                                                   long phase, double held_in, GateResult *__restrict__ res)
{
    __shared__ int s[256];
    __shared__ long carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (long b0 = 0; b0 < n_tiles; b0 += 256) {
        const long k = b0 + threadIdx.x;
        const int mine = k < n_tiles ? tile_count[k] : 0;
        s[threadIdx.x] = mine;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int add = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        const long carry = carry_s;
        if (k < n_tiles) tile_count[k] = (int)(carry + s[threadIdx.x] - mine);
        __syncthreads();
        if (threadIdx.x == 255) carry_s = carry + s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        res->n_open = carry_s;
        res->held_out = gate_held(peak, n_frames, phase, every, held_in);
    }
}

// the ascending list of open frames: tile offset + the wavefronts in front + the open lanes below (ballot and popcount); no atomics
__global__ __launch_bounds__(256) void k_gate_index(const double *__restrict__ peak, long n_frames, double squelch, int every, long phase, double held_in,
                                                    const int *__restrict__ tile_off, long n_tiles, int *__restrict__ d_open_idx)
{
    __shared__ int wcount[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long i = tile * GATE_TILE + threadIdx.x;
        const bool open = i < n_frames && gate_held(peak, i, phase, every, held_in) >= squelch;
        const unsigned long long b = __ballot(open);
        if (lane == 0) wcount[w] = __popcll(b);
        __syncthreads();
        int before = 0;
        for (int q = 0; q < w; q++) before += wcount[q];
        if (open) d_open_idx[(long)tile_off[tile] + before + __popcll(b & ((1ull << lane) - 1ull))] = (int)i;
        __syncthreads();
    }
}

// ---- the scanner's gate ------------------------------------------------------------------------------------------------------------------
// Both sweeps keep a slice as a detection if `peak_power > threshold` and then `bandwidth > MIN_SIGNAL_BANDWIDTH` (pyspecsdr.py:2549 / :2555,
// :1054 / :1059).  peak_power is an np.float32 and the threshold a Python float, a weak scalar under NEP 50: the comparison runs in float32
// against the threshold ROUNDED to float32.  The bandwidth is float64 on both sides.  A NaN on either side compares false: no hit.
// Same three steps as the squelch gate above — flags and tile counts, k_gate_scan over the counts (every = 0: it reads no peak), the
// ascending list from ballot and popcount; no atomics.
__device__ __forceinline__ bool scan_hit(const float *__restrict__ peak, const double *__restrict__ bw, long i, float threshold, double min_bw)
{
    return peak[i] > threshold && bw[i] > min_bw;
}

__global__ __launch_bounds__(256) void k_scan_flags(const float *__restrict__ peak, const double *__restrict__ bw, long n_slices, float threshold,
                                                    double min_bw, uint8_t *__restrict__ d_hit, int *__restrict__ tile_count, long n_tiles)
{
    __shared__ int wcount[4];
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long i = tile * GATE_TILE + threadIdx.x;
        const bool hit = i < n_slices && scan_hit(peak, bw, i, threshold, min_bw);
        if (i < n_slices && d_hit) d_hit[i] = hit ? 1 : 0;
        const unsigned long long b = __ballot(hit);
        if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = __popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) tile_count[tile] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_scan_index(const float *__restrict__ peak, const double *__restrict__ bw, long n_slices, float threshold,
                                                    double min_bw, const int *__restrict__ tile_off, long n_tiles, int *__restrict__ d_hit_idx)
{
    __shared__ int wcount[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long i = tile * GATE_TILE + threadIdx.x;
        const bool hit = i < n_slices && scan_hit(peak, bw, i, threshold, min_bw);
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wcount[w] = __popcll(b);
        __syncthreads();
        int before = 0;
        for (int q = 0; q < w; q++) before += wcount[q];
        if (hit) d_hit_idx[(long)tile_off[tile] + before + __popcll(b & ((1ull << lane) - 1ull))] = (int)i;   // < n_hit <= n_slices
        __syncthreads();
    }
}

// ---- dead reads --------------------------------------------------------------------------------------------------------------------------
// The loop skips a read buffer whose samples are all zero before anything else sees it (pyspecsdr.py:2237: np.all(samples == 0), the
// zero-filled array of a read that timed out, :1887).  live[f] = some word of frame f has a bit set below the sign, NumPy's `== 0` decided on
// the bits (-0.0 is zero; a NaN and a denormal are not, in any denormal mode).
// G lanes per frame: 64 (one wavefront per frame, four frames per workgroup) or 256 (one workgroup per frame, its four wavefronts on
// interleaved tiles).  A tile is 64 lanes x 16 bytes; a wavefront votes after its first tile and then after every four, and leaves at the
// first vote that saw a set bit: a live frame costs its first tile, only a dead one is read to the end.  The frame's pointer is 8-byte
// aligned and no more (d_iq + f * 2n words, n may be odd): two words in front of the first 16-byte boundary and two behind the last whole
// group go to single lanes.  No atomics; the flags do not depend on the schedule.
constexpr int LIVE_WAVE_MAX_N = 2048;   // frames of up to this many samples (16 KB, the meter's boundary in bytes): one wavefront per frame

template <int G>
__global__ __launch_bounds__(256) void k_live_flags(const uint32_t *__restrict__ iq, long n_frames, int n, uint8_t *__restrict__ live)
{
    constexpr int FPB = 256 / G;   // frames per workgroup pass
    __shared__ int any_s[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = threadIdx.x / G, t = threadIdx.x % G;
    const size_t words = 2 * (size_t)n;
    const size_t first = G == 256 ? (size_t)wave * 64 : 0;   // this wavefront's first group of 16 bytes
    for (long base = (long)blockIdx.x * FPB; base < n_frames; base += (long)gridDim.x * FPB) {
        const long f = base + slot;
        const bool has = f < n_frames;   // the same for every lane of a wavefront
        const uint32_t *p = iq + (size_t)(has ? f : 0) * words;
        const unsigned head = (reinterpret_cast<uintptr_t>(p) & 15) ? 2u : 0u;   // words >= 2
        const size_t n_groups = (words - head) >> 2, tail0 = (size_t)head + (n_groups << 2);
        const uint4 *v = reinterpret_cast<const uint4 *>(p + head);
        bool nz = false;
        if (has) {
            if ((unsigned)t < head) nz = (p[t] & 0x7fffffffu) != 0;
            else if (tail0 + ((unsigned)t - head) < words) nz = (p[tail0 + ((unsigned)t - head)] & 0x7fffffffu) != 0;
        }
        unsigned long long b = __ballot(nz);
        size_t g0 = first;
        if (!b && has && g0 < n_groups) {   // the first tile alone: what a live frame costs
            const size_t g = g0 + lane;
            bool z = false;
            if (g < n_groups) {
                const uint4 q = v[g];
                z = ((q.x | q.y | q.z | q.w) & 0x7fffffffu) != 0;
            }
            b = __ballot(z);
            g0 += G;
        }
        while (!b && has && g0 < n_groups) {   // four tiles in flight per vote
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const size_t g = g0 + (size_t)u * G + lane;
                q[u] = g < n_groups ? v[g] : make_uint4(0u, 0u, 0u, 0u);
            }
            const uint32_t m = (q[0].x | q[0].y | q[0].z | q[0].w) | (q[1].x | q[1].y | q[1].z | q[1].w) | (q[2].x | q[2].y | q[2].z | q[2].w) |
                               (q[3].x | q[3].y | q[3].z | q[3].w);
            b = __ballot((m & 0x7fffffffu) != 0);
            g0 += 4 * (size_t)G;
        }
        if (G == 64) {
            if (has && lane == 0) live[f] = b ? 1 : 0;
        } else {
            if (lane == 0) any_s[wave] = b ? 1 : 0;
            __syncthreads();
            if (threadIdx.x == 0 && has) live[f] = (any_s[0] | any_s[1] | any_s[2] | any_s[3]) ? 1 : 0;
            __syncthreads();
        }
    }
}

// the gate's two list steps over flags that are already bytes: counts per tile of 256 for k_gate_scan, then the ascending list
__global__ __launch_bounds__(256) void k_flag_count(const uint8_t *__restrict__ flag, long n_frames, int *__restrict__ tile_count, long n_tiles)
{
    __shared__ int wcount[4];
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long i = tile * GATE_TILE + threadIdx.x;
        const bool on = i < n_frames && flag[i] != 0;
        const unsigned long long b = __ballot(on);
        if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = __popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) tile_count[tile] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_flag_index(const uint8_t *__restrict__ flag, long n_frames, const int *__restrict__ tile_off, long n_tiles,
                                                    int *__restrict__ d_idx)
{
    __shared__ int wcount[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long i = tile * GATE_TILE + threadIdx.x;
        const bool on = i < n_frames && flag[i] != 0;
        const unsigned long long b = __ballot(on);
        if (lane == 0) wcount[w] = __popcll(b);
        __syncthreads();
        int before = 0;
        for (int q = 0; q < w; q++) before += wcount[q];
        if (on) d_idx[(long)tile_off[tile] + before + __popcll(b & ((1ull << lane) - 1ull))] = (int)i;   // < n_live <= n_frames
        __syncthreads();
    }
}

// ---- gather of the open frames ---------------------------------------------------------------------------------------------------------
// dst[k] = src[idx[k]] for frames of `per_frame` elements of V (uint4: 16 bytes per lane; uint2 for an odd frame length or a batch that
// starts 8 bytes off a 16-byte boundary).  An index outside [0, n_frames) is clamped:
// a caller's own list cannot make the copy read outside the batch.
template <class V>
__global__ __launch_bounds__(256) void k_gather_frames(const V *__restrict__ src, const int *__restrict__ idx, long n_open, long n_frames, long per_frame,
                                                       V *__restrict__ dst)
{
    for (long k = blockIdx.x; k < n_open; k += gridDim.x) {
        long f = idx[k];
        f = f < 0 ? 0 : (f >= n_frames ? n_frames - 1 : f);
        const V *s = src + (size_t)f * per_frame;
        V *d = dst + (size_t)k * per_frame;
        for (long i = threadIdx.x; i < per_frame; i += 256) d[i] = s[i];
    }
}

}  // namespace pss_sq

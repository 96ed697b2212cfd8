// pss_views.h — the two views without a history, the surface plot (draw_surface_plot, pyspecsdr.py:1567-1616) and the constellation
// (draw_vector_display, :1719-1752), in their compact forms for whole batches (include/pss.h, "surface magnitudes" / "constellation masks").
// Included by pss_fft.hip after pss_post.h.
//
// Surface: every '#' of a column follows from magnitude = int(value * 20) (:1593) and the screen size, so a batch returns one int8 per column
// (k_surface_mags) and the screen grid is an expansion of those (k_mags_cells / pss_h_mags_cells).  surface_mag() is what k_cells<T, 3> calls
// for its columns as well: the magnitudes ARE that kernel's.
// Constellation: one bit per screen cell (k_vector_masks), built in LDS; vector_cell() is what k_vector calls for its samples as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#pragma clang fp contract(off)     // the reference's statements hold no fused multiply-adds (host expansion included)

namespace pss_views {

constexpr double COS45 = 0x1.6a09e667f3bcdp-1, SIN45 = 0x1.6a09e667f3bccp-1;  // np.cos / np.sin(np.radians(45))

// int(value * 20) of column x (:1580-1593): each sample is normalised in float64 BEFORE np.interp ((row - min_val) / db_range is an array
// statement), w = max_w - 8 columns; -1 where the resampled value is not finite (:1592).  range: max_val - min_val with the == 0 -> 1 guard.
template <class Row>
__device__ __forceinline__ int surface_mag(const Row &row, int len, int w, int x, double lo, double range)
{
    const auto normalised = [&](int j) { return ((double)row[j] - lo) / range; };
    const double value = pss_post::interp_at(pss_post::fn_row(normalised), len, w, x);
    if (!isfinite(value)) return -1;
    return (int)(value * 20);
}

// the screen cell step y of column x marks (:1595-1598); false: off the plot area
__host__ __device__ inline bool surface_hit(int x, int y, int max_h, int max_w, int &sx, int &sy)
{
    sx = (int)((double)x - (double)y * COS45) + 8;
    sy = (int)((double)(max_h - 2) - (double)y * SIN45);
    return sx >= 0 && sx < max_w && sy >= 2 && sy < max_h - 1;
}

// Cell (sy, sx) of the grid from the row's magnitudes: 1 + y % 5 of the LAST (x, y) of the reference's loops (x outer, y inner, y < mag[x])
// that hits it, 0 if none does.  The cell looks for its own winner: sy = int(max_h - 2 - y sin45) holds for at most two y (sin45 < 1), and for
// such a y, sx - 8 = int(x - y cos45) for at most two x (truncation toward zero: two only around 0).  The candidates around the real-valued
// solutions are tested with surface_hit itself, so rounding cannot move a hit: no atomics, no order of execution.
__host__ __device__ inline int surface_cell(const int8_t *mag, int w, int max_h, int max_w, int sy, int sx)
{
    if (sy < 2 || sy >= max_h - 1) return 0;
    const int y0 = (int)((double)(max_h - 2 - sy) / SIN45);
    int best_x = -1, best_y = 0;
    for (int y = y0 - 2 < 0 ? 0 : y0 - 2; y <= y0 + 1 && y < 127; y++) {
        const int x0 = (int)((double)(sx - 8) + (double)y * COS45);
        for (int x = x0 - 2 < 0 ? 0 : x0 - 2; x <= x0 + 2 && x < w; x++) {
            int hx, hy;
            if (mag[x] <= y || !surface_hit(x, y, max_h, max_w, hx, hy) || hx != sx || hy != sy) continue;
            if (x > best_x || (x == best_x && y > best_y)) { best_x = x; best_y = y; }
        }
    }
    return best_x < 0 ? 0 : 1 + best_y % 5;
}

// Many rows per launch: a row is owned by W wavefronts (W = 1: four independent rows per 256-thread workgroup and no workgroup barrier), its
// finite extremes and its columns come out of the same kernel.  STAGED: the row is parked in LDS while the extremes are formed (one read of the
// row from HBM), and the columns interpolate from there; otherwise (rows too long for LDS) the columns read the row again.
// Extremes with k_row_extremes' bits, down to the sign of a zero minimum present with both signs: lane l sees the elements l, l + 64, ... in
// that kernel's order and with its compares (a tie keeps the earlier element) — with W wavefronts each takes a contiguous stretch of that
// sequence and the W partial results of a lane are folded in order —, then the same butterfly.  A row without a finite value gives
// (+inf, -inf), and (v - inf) / -inf is NaN for every v: all columns -1.
template <class T, int W, bool STAGED>
__global__ __launch_bounds__(W == 1 ? 256 : 64 * W) void k_surface_mags(const T *__restrict__ rows, long n_rows, int len, int disp_w,
                                                                        int8_t *__restrict__ mag, double *__restrict__ range_out)
{
    constexpr int TT = 64 * W, RPW = W == 1 ? 4 : 1;
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ T part_lo[W > 1 ? TT : 1], part_hi[W > 1 ? TT : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = W == 1 ? lane : tid;
    T *buf = reinterpret_cast<T *>(smem) + (size_t)(W == 1 ? wave : 0) * (STAGED ? len : 0);
    const int steps = (len + 63) / 64, seg = (steps + W - 1) / W;                 // 64-element steps of the row; steps per wavefront
    const int i0 = W == 1 ? lane : lane + 64 * seg * wave;
    const int i1 = W == 1 ? len : (64 * seg * (wave + 1) < len ? 64 * seg * (wave + 1) : len);
    const long groups = (n_rows + RPW - 1) / RPW;
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long f = g * RPW + (W == 1 ? wave : 0);
        if (W == 1 && f >= n_rows) continue;     // whole wavefront (rows are wavefront-private when W = 1)
        const T *row = rows + (size_t)f * len;
        T lo = (T)INFINITY, hi = (T)-INFINITY;
#pragma unroll 4
        for (int i = i0; i < i1; i += 64) {
            const T v = row[i];
            if constexpr (STAGED) buf[i] = v;
            if (isfinite(v)) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        }
        if constexpr (W > 1) {
            part_lo[tid] = lo;
            part_hi[tid] = hi;
            __syncthreads();                     // (the staged row is complete as well)
            lo = part_lo[lane]; hi = part_hi[lane];
#pragma unroll
            for (int w = 1; w < W; w++) {
                const T a = part_lo[64 * w + lane], b = part_hi[64 * w + lane];
                lo = a < lo ? a : lo;
                hi = b > hi ? b : hi;
            }
        } else {
            pss_post::row_sync<true>();          // the row is in LDS
        }
        for (int off = 32; off > 0; off >>= 1) {
            const T a = __shfl_xor(lo, off), b = __shfl_xor(hi, off);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        // (k_row_extremes stores lane 0's result; broadcast, so that every column is normalised with those bits)
        lo = __shfl(lo, 0);
        hi = __shfl(hi, 0);
        if (range_out && t == 0) { range_out[2 * f] = (double)lo; range_out[2 * f + 1] = (double)hi; }
        double range = (double)hi - (double)lo;
        if (range == 0) range = 1;
        int8_t *mp = mag + (size_t)f * disp_w;
        for (int x = t; x < disp_w; x += TT)
            mp[x] = (int8_t)surface_mag(STAGED ? (const T *)buf : row, len, disp_w, x, (double)lo, range);
        pss_post::row_sync<W == 1>();            // the LDS row and the partial extremes may be overwritten now
    }
}

// pss_surface_cells' grids from the magnitudes: one thread per cell
__global__ __launch_bounds__(256) void k_mags_cells(const int8_t *__restrict__ mag, long n_rows, int max_h, int max_w, int8_t *__restrict__ colour)
{
    const long total = n_rows * max_h * max_w;
    const int w = max_w - 8;
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
        const long q = c / max_w, f = q / max_h;
        colour[c] = (int8_t)surface_cell(mag + f * w, w, max_h, max_w, (int)(q - f * max_h), (int)(c - q * max_w));
    }
}

// One IQ sample's '.' (:1744-1748): float32 arithmetic as NumPy evaluates it (complex64 parts times a Python int stay float32), truncation
// toward zero; false: not on the screen, or a coordinate that is not finite (the reference raises there; documented difference).
__device__ __forceinline__ bool vector_cell(float2 v, int cx, int cy, int scale, int max_h, int max_w, int &x, int &y)
{
    const float fx = __fadd_rn((float)cx, __fmul_rn(v.x, (float)scale)), fy = __fsub_rn((float)cy, __fmul_rn(v.y, (float)scale));
    if (!isfinite(fx) || !isfinite(fy)) return false;
    x = (int)fx;
    y = (int)fy;
    return x >= 0 && x < max_w && y >= 0 && y < max_h;
}

// One frame per W wavefronts (W = 1: four frames per 256-thread workgroup, wavefront-private masks, no workgroup barrier).  The frame's mask
// [max_h][words] is cleared and filled in LDS (atomicOr on LDS words; a bit already seen set is not set again — the peek may be stale, which
// costs one redundant atomic and never a bit), then copied out with coalesced stores: the result does not depend on the schedule.
// IQ is read 16 bytes (two samples) per lane; a frame that starts on an odd sample takes its first sample alone.
template <int W>
__global__ __launch_bounds__(W == 1 ? 256 : 64 * W) void k_vector_masks(const float2 *__restrict__ iq, long n_frames, int n, int max_h, int max_w,
                                                                        unsigned *__restrict__ mask)
{
    constexpr int TT = 64 * W, RPW = W == 1 ? 4 : 1;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = W == 1 ? lane : tid;
    const int words = (max_w + 31) >> 5, mw = max_h * words;
    unsigned *m = reinterpret_cast<unsigned *>(smem) + (size_t)(W == 1 ? wave : 0) * mw;
    const int cx = max_w / 2, cy = max_h / 2, scale = (max_w < max_h ? max_w : max_h) / 4;
    const auto put = [&](float2 v) {
        int x, y;
        if (!vector_cell(v, cx, cy, scale, max_h, max_w, x, y)) return;
        unsigned *wp = m + y * words + (x >> 5);
        const unsigned bit = 1u << (x & 31);
        if (!(*(volatile unsigned *)wp & bit)) atomicOr(wp, bit);
    };
    const long groups = (n_frames + RPW - 1) / RPW;
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long f = g * RPW + (W == 1 ? wave : 0);
        if (W == 1 && f >= n_frames) continue;   // whole wavefront
        for (int i = t; i < mw; i += TT) m[i] = 0;
        pss_post::row_sync<W == 1>();
        const float2 *fr = iq + (size_t)f * n;
        const int head = n > 0 ? (int)((reinterpret_cast<uintptr_t>(fr) >> 3) & 1) : 0;    // samples in front of the first 16-byte boundary
        const int pairs = (n - head) >> 1;
        const float4 *p4 = reinterpret_cast<const float4 *>(fr + head);
#pragma unroll 4
        for (int i = t; i < pairs; i += TT) {
            const float4 q = p4[i];
            put(make_float2(q.x, q.y));
            put(make_float2(q.z, q.w));
        }
        if (t == 0 && head) put(fr[0]);
        if (t == 1 && ((n - head) & 1)) put(fr[n - 1]);
        pss_post::row_sync<W == 1>();
        unsigned *out = mask + (size_t)f * mw;
        for (int i = t; i < mw; i += TT) out[i] = m[i];
        pss_post::row_sync<W == 1>();            // the mask may be cleared now
    }
}

// pss_vector_cells' grids from the masks: one thread per cell
__global__ __launch_bounds__(256) void k_masks_cells(const unsigned *__restrict__ mask, long n_frames, int max_h, int max_w, int8_t *__restrict__ grid)
{
    const long total = n_frames * max_h * max_w;
    const int words = (max_w + 31) >> 5;
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (long)gridDim.x * blockDim.x) {
        const long q = c / max_w;                // frame * max_h + y
        const int x = (int)(c - q * max_w);
        grid[c] = (int8_t)((mask[q * words + (x >> 5)] >> (x & 31)) & 1u);
    }
}

}  // namespace pss_views

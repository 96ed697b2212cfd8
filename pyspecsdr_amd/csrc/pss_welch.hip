// pss_welch.hip — the capture survey: Welch's averaged periodogram and the max-hold row of n_rows rows in one pass (scipy.signal.welch /
// spectrogram(mode='psd').max(-1), two-sided, float64).  The arithmetic is pss_welch.h's; this unit places it.
//   k_welch<LOG_R3, MAXROW, PREFETCH, REGS, OCC>   k_spectrum_r16's frame layout (pss_fft_r16.h): T = N / 16 threads per segment, 16 samples per thread, r16_core
//           with an emit that accumulates.  A work item is one block of a row (BLOCK consecutive segments); the 256 / T segment slots of a
//           workgroup take consecutive items, the items of the whole batch are numbered flat and walked under a capped grid.  A thread's 16
//           bins are the same for every segment, so its 16 sums (and 16 maxima) stay in its registers across the block and are never
//           exchanged; the item's partial rows [N] go to context-owned scratch with coalesced stores.  One wavefront per SIMD: the kernel
//           takes 254 to 334 registers, the accumulators and what the allocator moves out of its way in AGPRs, and with that budget the next
//           segment of the block is prefetched (PREFETCH; REGS: bit 0 the window, bit 1 the stage-1 twiddles stay in registers, else
//           they are read again for every segment from the vector cache; OCC: wavefronts per SIMD the compiler plans for) — the
//           measurements are in DESIGN 4.12.  Overlapping segments (S < N) are re-read through the caches.
//   k_welch_fold   adds the block partials of a row in the header's order (FOLD_Q chunks, then the chunk sums), applies 1 / L and scale and
//           writes the two rows.  Up to 1024 threads a workgroup: bins x chunks.
// No floating-point atomics; nothing depends on the grid.  Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pss_ctx.h"
// pss_fft_r16.h defines one kernel that is not a template, k_huge_p1 (pss_fft.hip launches it); a second unit that includes the header
// would define the symbol again, so this unit's unused copy gets a name of its own.
#define k_huge_p1 k_huge_p1_copy_of_pss_welch
#include "pss_fft_r16.h"
#undef k_huge_p1
#include "pss_welch.h"

namespace {

using namespace pss_wl;

constexpr long WELCH_GRID_CAP = 1024;   // workgroups of a launch: items past it are walked by a grid-stride loop

struct WelchGeom {
    long row_stride, L, nb, n_items;
    int S, detrend;
};

template <int LOG_R3, bool MAXROW, bool PREFETCH, int REGS, int OCC>
__global__ __launch_bounds__(256, OCC) void k_welch(const float2 *__restrict__ iq, const double2 *__restrict__ tw, const double *__restrict__ win,
                                               const WelchGeom G, double *__restrict__ part)
{
    using C = pss_r16::Cfg<LOG_R3>;
    constexpr int R3 = C::R3, T = C::T, N = C::N, FPW = C::FPW;
    constexpr bool WL = T <= 64;      // a segment's threads are lanes of one wavefront: no workgroup barriers in the transform
    constexpr int WAVES = T / 64;     // wavefronts of a segment (T > 64)
    constexpr bool WREG = (REGS & 1) != 0, TREG = (REGS & 2) != 0;
    // the thread's 16 window values and 15 stage-1 twiddles stay in registers beside the accumulators, except in the one instance where
    // they no longer fit (4096 points with the max row: 6 spilled VGPRs): there they are read again for every segment, from the vector cache
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *ex_all = reinterpret_cast<double2 *>(smem);
    double2 *tw2 = ex_all + (size_t)FPW * C::EX;
    __shared__ double2 red[4];        // the detrend mean across a segment's wavefronts (T > 64)
    const int tid = threadIdx.x, fl = tid / T, t = tid % T;
    double2 *ex = ex_all + (size_t)fl * C::EX;
    double2 tw1[16];
    double w[16];
    tw1[0] = make_double2(1.0, 0.0);
#pragma unroll
    for (int k2 = 1; k2 < 16; k2++) tw1[k2] = tw[(size_t)t * k2];
#pragma unroll
    for (int n2 = 0; n2 < 16; n2++) w[n2] = WREG ? win[t + T * n2] : 0.0;
    if (tid < R3 * 16) {
        const int m1 = tid / 16, j2 = tid % 16;
        tw2[C::tw2_slot(tid)] = tw[(size_t)(m1 * j2) * 16];
    }
    __syncthreads();
    const long groups = (G.n_items + FPW - 1) / FPW;
    const int nseg = G.L < BLOCK ? (int)G.L : BLOCK;   // uniform over the grid: the barriers below are met by every thread
    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long item = g * FPW + fl;
        const bool live = item < G.n_items;
        const long it = live ? item : 0;
        const long row = it / G.nb, blk = it - row * G.nb;
        const long s0 = blk * BLOCK;
        const float2 *xr = iq + (size_t)row * G.row_stride;
        double sum[16], mx[16];
#pragma unroll
        for (int i = 0; i < 16; i++) sum[i] = 0.0, mx[i] = -INFINITY;
        float2 nx[16];
        auto fetch = [&](int j) {   // a row's last block may be short: its spare turns read segment s0 and add nothing
            const float2 *x = xr + (size_t)(s0 + j < G.L ? s0 + j : s0) * G.S;
#pragma unroll
            for (int n2 = 0; n2 < 16; n2++) nx[n2] = x[t + T * n2];
        };
        if constexpr (PREFETCH) fetch(0);
        for (int j = 0; j < nseg; j++) {
            const bool valid = s0 + j < G.L;
            if constexpr (!PREFETCH) fetch(j);
            double mr = 0.0, mi = 0.0;
            if (G.detrend) {
                double sr = 0.0, si = 0.0;
#pragma unroll
                for (int n2 = 0; n2 < 16; n2++) sr += (double)nx[n2].x, si += (double)nx[n2].y;
#pragma unroll
                for (int off = (T < 64 ? T : 64) / 2; off >= 1; off >>= 1) sr += __shfl_xor(sr, off), si += __shfl_xor(si, off);
                if constexpr (WAVES > 1) {
                    if ((tid & 63) == 0) red[tid >> 6] = make_double2(sr, si);
                    __syncthreads();
                    const int w0 = fl * WAVES;
                    sr = red[w0].x, si = red[w0].y;
#pragma unroll
                    for (int wv = 1; wv < WAVES; wv++) sr += red[w0 + wv].x, si += red[w0 + wv].y;
                }
                mr = sr * (1.0 / N), mi = si * (1.0 / N);
            }
            double2 v[16];
            const double *wl = win + t;
            if constexpr (!WREG) asm volatile("" : "+v"(wl));   // a fresh address every turn: the loads stay inside the loop
            if constexpr (!TREG) {
                const double2 *tl = tw;
                asm volatile("" : "+v"(tl));
#pragma unroll
                for (int k2 = 1; k2 < 16; k2++) tw1[k2] = tl[(size_t)t * k2];
            }
#pragma unroll
            for (int n2 = 0; n2 < 16; n2++) {
                const double wv = WREG ? w[n2] : wl[T * n2];
                v[n2] = make_double2(((double)nx[n2].x - mr) * wv, ((double)nx[n2].y - mi) * wv);
            }
            if (PREFETCH && j + 1 < nseg) fetch(j + 1);   // the next segment's samples travel while this one is transformed
            pss_r16::r16_core<LOG_R3, WL>(v, ex, tw1, tw2, t, [&](int i, int, double2 X) {
                const double p = power(X.x, X.y);
                if (valid) {
                    sum[i] += p;
                    if constexpr (MAXROW) mx[i] = nan_max(mx[i], p);
                }
            });
            pss_r16::frame_sync<WL>();   // the next segment overwrites this one's exchange buffer (and `red`)
        }
        if (live) {
            double *ps = part + (size_t)item * (MAXROW ? 2 : 1) * N;
#pragma unroll
            for (int c = 0; c < 16 / R3; c++)
#pragma unroll
                for (int j1 = 0; j1 < R3; j1++) {
                    const int k = 256 * j1 + t + T * c;   // r16_core's bin of result c R3 + j1
                    ps[k] = sum[c * R3 + j1];
                    if constexpr (MAXROW) ps[N + k] = mx[c * R3 + j1];
                }
        }
    }
}

// part: [n_rows][nb][planes][N].  A workgroup of bins x qt threads folds `bins` bins of one row: thread (chunk c, bin b) adds its chunk's
// partials in ascending order (eight loads in flight, the additions in order), thread (0, b) then adds the chunk sums in ascending order.
// qt: the chunks that hold a partial, rounded up to a power of two (the tree's other chunks are empty and add nothing); bins = 1024 / qt, at
// most N: a row of few blocks is folded by wide workgroups, a row of many by 16 bins x 64 chunks.  The (row, bins) pieces are walked flat.
__global__ __launch_bounds__(1024) void k_welch_fold(const double *__restrict__ part, long n_rows, int N, long nb, long L, double scale, int planes,
                                                     int bins, int n_chunks, double *__restrict__ mean, double *__restrict__ max)
{
    __shared__ double ls[1024], lm[1024];
    const int tid = threadIdx.x, b = tid % bins, c = tid / bins;
    const long cl = chunk_len(nb);
    const long j0 = c * cl < nb ? c * cl : nb, j1 = j0 + cl < nb ? j0 + cl : nb;
    const long pieces = n_rows * (N / bins);
    const size_t step = (size_t)planes * N;
    for (long pc = blockIdx.x; pc < pieces; pc += gridDim.x) {
        const long row = pc / (N / bins);
        const int k = (int)(pc - row * (N / bins)) * bins + b;
        const double *p = part + ((size_t)row * nb * planes) * N + k;
        double s = 0.0, m = -INFINITY;
        long j = j0;
        for (; j + 8 <= j1; j += 8) {
            double a[8], x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) a[u] = p[(size_t)(j + u) * step], x[u] = planes == 2 ? p[(size_t)(j + u) * step + N] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; u++) s += a[u], m = nan_max(m, x[u]);
        }
        for (; j < j1; j++) {
            s += p[(size_t)j * step];
            if (planes == 2) m = nan_max(m, p[(size_t)j * step + N]);
        }
        if (n_chunks > 1) {
            ls[tid] = s, lm[tid] = m;
            __syncthreads();
        }
        if (c == 0) {
            for (int q = 1; q < n_chunks; q++) s += ls[q * bins + b], m = nan_max(m, lm[q * bins + b]);
            mean[(size_t)row * N + k] = (s / (double)L) * scale;
            if (planes == 2) max[(size_t)row * N + k] = m * scale;
        }
        if (n_chunks > 1) __syncthreads();
    }
}

template <int LOG_R3>
int launch(pss_ctx *ctx, const float *d_iq, const WelchGeom &G, const double2 *tw, const double *d_win, bool maxrow, double *d_part)
{
    using C = pss_r16::Cfg<LOG_R3>;
    // what stays in registers beside the accumulators was measured per instance: without the max row the stage-1 twiddles alone,
    // with it the window too, except at 4096 points, where window and twiddles together spill (6 VGPRs) and the window alone does not
    auto kern = maxrow ? k_welch<LOG_R3, true, true, (LOG_R3 == 4 ? 1 : 3), 1> : k_welch<LOG_R3, false, true, 2, 1>;
    const size_t lds = (size_t)C::FPW * C::EX * sizeof(double2) + (size_t)C::TW2 * sizeof(double2);
    if (lds > 64 * 1024)
        PSS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long groups = (G.n_items + C::FPW - 1) / C::FPW;
    pss_kernel_begin(ctx, "k_welch");
    hipLaunchKernelGGL(kern, dim3((unsigned)(groups < WELCH_GRID_CAP ? groups : WELCH_GRID_CAP)), dim3(256), lds, PSS_STREAM(ctx),
                       reinterpret_cast<const float2 *>(d_iq), tw, d_win, G, d_part);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_welch launch");
}

}  // namespace

extern "C" long pss_welch_segments(long n, int nperseg, int step)
{
    if (!nperseg_ok(nperseg) || step < 1 || step > nperseg) return PSS_E_ARG;
    return segments(n, nperseg, step);
}

extern "C" int pss_welch_default_window(int nperseg, double *h_win)
{
    if (!nperseg_ok(nperseg)) return pss_fail(nullptr, PSS_E_ARG, "pss_welch_default_window: nperseg not in {256, 512, 1024, 2048, 4096}");
    if (!h_win) return pss_fail(nullptr, PSS_E_ARG, "pss_welch_default_window: null window");
    default_window(nperseg, h_win);
    return PSS_OK;
}

extern "C" int pss_h_welch(const float *iq, long n_rows, long n, long row_stride, int nperseg, int step, const double *win, int detrend, double scale,
                           double *mean, double *max)
{
    if (const char *why = check(iq, n_rows, n, row_stride, nperseg, step, win, detrend, scale, mean))
        return pss_fail(nullptr, PSS_E_ARG, std::string("pss_h_welch: ") + why);
    HostPlan P(nperseg);
    for (long r = 0; r < n_rows; r++)
        host_row(P, iq + 2 * (size_t)r * row_stride, n, step, win, detrend, scale, mean + (size_t)r * nperseg, max ? max + (size_t)r * nperseg : nullptr);
    return PSS_OK;
}

extern "C" int pss_welch(pss_ctx *ctx, const float *d_iq, long n_rows, long n, long row_stride, int nperseg, int step, const double *h_win,
                         int detrend, double scale, double *d_mean, double *d_max)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (const char *why = check(d_iq, n_rows, n, row_stride, nperseg, step, h_win, detrend, scale, d_mean))
        return pss_fail(ctx, PSS_E_ARG, std::string("pss_welch: ") + why);
    if ((reinterpret_cast<uintptr_t>(d_iq) | reinterpret_cast<uintptr_t>(d_mean) | reinterpret_cast<uintptr_t>(d_max)) & 7)
        return pss_fail(ctx, PSS_E_ARG, "pss_welch: a pointer that is not aligned to 8 bytes");
    WelchGeom G;
    G.row_stride = row_stride, G.S = step, G.detrend = detrend;
    G.L = segments(n, nperseg, step), G.nb = n_blocks(G.L);
    if (n_rows > INT64_MAX / 32 / nperseg / G.nb) return pss_fail(ctx, PSS_E_ARG, "pss_welch: n_rows times the blocks of a row overflows");
    G.n_items = n_rows * G.nb;
    const int planes = d_max ? 2 : 1;
    // the window (pss_table_sync: uploaded when its bytes differ from the device copy), in a buffer that holds the longest one
    int r = pss_table_sync(ctx, &ctx->welch_win, h_win, sizeof(double) * nperseg, "pss_welch window", sizeof(double) * MAX_N);
    if (r) return r;
    r = pss_ensure_buffer(ctx, &ctx->welch_part, &ctx->welch_part_bytes, sizeof(double) * (size_t)G.n_items * planes * nperseg, "pss_welch partials");
    if (r) return r;
    const double2 *tw;
    const double *hamming;
    r = pss_fft_tables(ctx, nperseg, &tw, &hamming);
    if (r) return r;
    const double *d_win = reinterpret_cast<const double *>(ctx->welch_win.dev);
    double *d_part = reinterpret_cast<double *>(ctx->welch_part);
    PssTimeScope timed(ctx);
    switch (nperseg) {
    case 256: r = launch<0>(ctx, d_iq, G, tw, d_win, d_max != nullptr, d_part); break;
    case 512: r = launch<1>(ctx, d_iq, G, tw, d_win, d_max != nullptr, d_part); break;
    case 1024: r = launch<2>(ctx, d_iq, G, tw, d_win, d_max != nullptr, d_part); break;
    case 2048: r = launch<3>(ctx, d_iq, G, tw, d_win, d_max != nullptr, d_part); break;
    default: r = launch<4>(ctx, d_iq, G, tw, d_win, d_max != nullptr, d_part); break;
    }
    if (r) return r;
    const long cl = chunk_len(G.nb);
    const int n_chunks = (int)((G.nb + cl - 1) / cl);   // chunks that hold a partial: at most FOLD_Q
    int qt = 1;
    while (qt < n_chunks) qt <<= 1;
    const int bins = 1024 / qt < nperseg ? 1024 / qt : nperseg;
    const long pieces = n_rows * (nperseg / bins);
    pss_kernel_begin(ctx, "k_welch_fold");
    hipLaunchKernelGGL(k_welch_fold, dim3((unsigned)(pieces < 4 * WELCH_GRID_CAP ? pieces : 4 * WELCH_GRID_CAP)), dim3(bins * qt), 0, PSS_STREAM(ctx), d_part,
                       n_rows, nperseg, G.nb, G.L, scale, planes, bins, n_chunks, d_mean, d_max);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_welch_fold launch");
}

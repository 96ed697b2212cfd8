// pss_pfb.hip — the polyphase channeliser: "every channel of this capture's uniform grid of M channels at fs / D" as one call.  The
// arithmetic is pss_pfb.h's; this unit places it.
//   k_pfb   float64.  A workgroup walks tiles of R = TILE_ELEMS / M consecutive output instants.  Per tile:
//           1. branch sums: the tile's (instant, branch) pairs go round the threads by their FIRST TAP, first tap fastest — the lanes of
//              a wavefront own consecutive first taps of one instant (64 / M instants where M < 64), that is consecutive branches in
//              descending order: they read consecutive samples and consecutive taps.  The workgroup's thread count is a multiple of M,
//              so the PFB_ITEMS pairs of a thread share their first tap and with it every tap: a step of the thread is one tap load,
//              PFB_ITEMS sample loads and 2 PFB_ITEMS fma, the chains in registers, taps walked M apart in ascending order.  The span
//              (up to 32 M samples) is never resident anywhere; samples and taps come through the vector cache, where the instants of
//              a tile and the tiles of neighbouring workgroups find each other's lines.  The sums land in LDS at the bit-reversed branch.
//           2. the DFT of every instant of the tile in LDS: log2 M stages, the tile's R M / 2 butterflies of a stage go round the
//              threads, one barrier a stage.
//           3. the R x M tile leaves LDS transposed, instant fastest: every channel row receives R contiguous complex64 values (64 bytes
//              at M = 1024).  Rows lie M + 1 slots apart in LDS from M = 32 on, so this column read meets no bank twice.
// Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_chan.h"
#include "pss_ctx.h"
#include "pss_pfb.h"

namespace {

using namespace pss_pf;

constexpr int PFB_T = 1024;                     // threads of a workgroup: 16 wavefronts beside the one 132 KiB LDS image of a CU
constexpr int PFB_ITEMS = TILE_ELEMS / PFB_T;   // (instant, branch) pairs of a tile a thread owns
static_assert(PFB_T % MAX_CHAN == 0 && PFB_ITEMS * PFB_T == TILE_ELEMS, "a thread's pairs share their first tap");
constexpr long PFB_GRID_CAP = 1024;             // workgroups of a launch: tiles past it are walked by a grid-stride loop

// iq: the caller's buffer, [lo, hi): the capture indices it holds (inside the capture: the host has checked) — everything else is zero (the
// host has checked that nothing else inside the capture is needed); element 0 of iq is readable even where [lo, hi) is empty.
// j00: m_begin D + lead, the own sample of the first output; n_m: m_end - m_begin; lb: log2 M; R, RS: tile_instants(M), tile_row(M).
__global__ __launch_bounds__(PFB_T) void k_pfb(const float2 *__restrict__ iq, long lo, long hi, const double *__restrict__ knots,
                                               const double *__restrict__ taps, int M, int lb, int D, int T, long j00, long n_m, int R, int RS,
                                               long n_tiles, float2 *__restrict__ out, long out_stride)
{
    __shared__ double vr[TILE_SLOTS], vi[TILE_SLOTS];
    const int tid = threadIdx.x;
    const int kap = tid & (M - 1), r0 = tid >> lb, dr = PFB_T >> lb;
    const int k_last = kap < T ? kap + (((T - 1 - kap) >> lb) << lb) : kap;   // the last tap of this thread's chains
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long m0 = tile * R;                                 // the tile's first output, counted from m_begin
        const int cnt = n_m - m0 < R ? (int)(n_m - m0) : R;       // >= 1
        // ---- 1. branch sums.  Thread item i is (instant r0 + i dr, first tap kap): PFB_T is a multiple of M, so the chains of a thread
        // share their first tap and with it every tap — a step is ONE tap load and PFB_ITEMS sample loads, all in flight together.
        // jt: the oldest sample any chain of the tile may touch; samples are addressed from there by a 32-bit offset (a tile's span is
        // below 2^16 samples): one scalar base and one vector subtraction a load.
        const long tb = j00 + m0 * D - (T - 1) - lo;
        unsigned o[PFB_ITEMS];
        bool fast = cnt == R;
#pragma unroll
        for (int i = 0; i < PFB_ITEMS; i++) {
            const int r = r0 + i * dr;
            const long j0 = j00 + (m0 + r) * D;
            o[i] = (unsigned)(r * D + (T - 1));                   // j0 - jt: no smaller than any k
            fast = fast && j0 - k_last >= lo && j0 - kap < hi;
        }
        double ur[PFB_ITEMS], ui[PFB_ITEMS];
        if (fast) {
            // a whole tile and every sample of every chain in the buffer (all but the chains at the capture's ends): no test per step
            branch_sums<PFB_ITEMS>(kap, M, T, [&](int k) { return taps[k]; }, [&](int i, int k, float &xr, float &xi) {
                const unsigned off = o[i] - (unsigned)k;
                __builtin_assume(off < (1u << 16));
                const float2 x = iq[tb + (long)off];              // = iq[j0_i - k - lo]
                xr = x.x;
                xi = x.y;
            }, ur, ui);
        } else {
            branch_sums<PFB_ITEMS>(kap, M, T, [&](int k) { return taps[k]; }, [&](int i, int k, float &xr, float &xi) {
                // the load is unconditional (a sample that is zero or an instant past the tile's count reads element 0 and drops it), so
                // that the loads of a step are in flight together
                const long j = tb + lo + (long)(o[i] - (unsigned)k);
                const bool in = j >= lo && j < hi && r0 + i * dr < cnt;
                const float2 x = iq[in ? j - lo : 0];
                xr = in ? x.x : 0.0f;
                xi = in ? x.y : 0.0f;
            }, ur, ui);
        }
#pragma unroll
        for (int i = 0; i < PFB_ITEMS; i++) {
            const int r = r0 + i * dr;
            if (r < cnt) {
                const int rho = (int)((uint64_t)(j00 + (m0 + r) * D - kap) & (uint64_t)(M - 1));   // the branch whose first tap is kap: first_tap(j0, rho, M) = kap
                const int pos = r * RS + (int)(__brev((unsigned)rho) >> (32 - lb));                 // = bitrev(rho, lb)
                vr[pos] = ur[i];
                vi[pos] = ui[i];
            }
        }
        __syncthreads();
        // ---- 2. the DFT of every instant: butterfly q of a stage is butterfly q mod (M / 2) of instant q / (M / 2)
        for (int ls = 0; ls < lb; ls++) {
            for (int q = tid; q < cnt * (M >> 1); q += PFB_T) {
                const int r = q >> (lb - 1), i = q & ((M >> 1) - 1);
                const int a = r * RS + fly_a(i, ls), b = a + (1 << ls), kn = fly_knot(i, ls);
                double ar = vr[a], ai = vi[a], br = vr[b], bi = vi[b];
                butterfly(ar, ai, br, bi, knots[2 * kn], knots[2 * kn + 1]);
                vr[a] = ar;
                vi[a] = ai;
                vr[b] = br;
                vi[b] = bi;
            }
            __syncthreads();
        }
        // ---- 3. one rounding, transposed store: element e is instant e mod R of channel e / R (R is a power of two)
        const int lr = TILE_LOG2 - lb;                            // log2 R: R M = TILE_ELEMS
        for (int e = tid; e < TILE_ELEMS; e += PFB_T) {
            const int c = e >> lr, r = e & (R - 1);
            if (r < cnt) out[(size_t)c * out_stride + (m0 + r)] = make_float2((float)vr[r * RS + c], (float)vi[r * RS + c]);
        }
        __syncthreads();   // the next tile's branch sums overwrite what this loop reads
    }
}

// The argument rules of pss_pfb and pss_h_pfb: the channelisers' shared ones (pss_chan.h) for a power-of-two channel count.
int pfb_check(pss_ctx *ctx, const char *who, const void *iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim, const double *taps,
              int n_taps, int lead, long m_begin, long m_end, const void *out, long out_stride)
{
    return pss_chan_args_check(ctx, who, chan_ok(n_chan), "n_chan is not a power of two in [2, 1024]", iq, n_buf, buf_index0, n_capture, n_chan, decim, taps,
                               n_taps, lead, m_begin, m_end, out, out_stride);
}

}  // namespace

extern "C" int pss_pfb_default_taps(int n_chan, double *taps, int *n_taps)
{
    if (!n_taps || !chan_ok(n_chan)) return pss_fail(nullptr, PSS_E_ARG, "pss_pfb_default_taps: n_chan is not a power of two in [2, 1024]");
    *n_taps = DEFAULT_TAPS_PER_CHAN * n_chan + 1;
    if (!taps) return PSS_OK;
    return pss_design_firwin(*n_taps, 1.0 / (double)n_chan, taps);
}

extern "C" int pss_h_pfb(const float *h_iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim, const double *taps, int n_taps, int lead,
                         long m_begin, long m_end, float *h_out, long out_stride)
{
    const int r = pfb_check(nullptr, "pss_h_pfb", h_iq, n_buf, buf_index0, n_capture, n_chan, decim, taps, n_taps, lead, m_begin, m_end, h_out, out_stride);
    if (r || m_begin == m_end) return r;
    const double *knots = pss_host_knots();
    pss_chan_host_loop(h_iq, n_buf, buf_index0, n_chan, m_begin, m_end, h_out, out_stride, [&](long m, auto x, double *vr, double *vi, float *y) {
        instant(m, n_chan, decim, taps, n_taps, lead, knots, x, vr, vi, y);
    });
    return PSS_OK;
}

extern "C" int pss_pfb(pss_ctx *ctx, const float *d_iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim, const double *taps, int n_taps,
                       int lead, long m_begin, long m_end, float *d_out, long out_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = pfb_check(ctx, "pss_pfb", d_iq, n_buf, buf_index0, n_capture, n_chan, decim, taps, n_taps, lead, m_begin, m_end, d_out, out_stride);
    if (r || m_begin == m_end) return r;
    // the host tables, back to back: knots, taps (pss_table_sync: uploaded when they differ from the device copy)
    const size_t o_taps = sizeof(double) * 2 * pss_dc::KNOTS, bytes = o_taps + sizeof(double) * (size_t)n_taps;
    std::vector<unsigned char> tab(bytes);
    memcpy(tab.data(), pss_host_knots(), o_taps);
    memcpy(tab.data() + o_taps, taps, bytes - o_taps);
    r = pss_table_sync(ctx, &ctx->pfb_tab, tab.data(), bytes, "pss_pfb tables");
    if (r) return r;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(ctx->pfb_tab.dev);
    const int R = tile_instants(n_chan);
    const long n_m = m_end - m_begin, n_tiles = (n_m + R - 1) / R;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_pfb");
    hipLaunchKernelGGL(k_pfb, dim3((unsigned)(n_tiles < PFB_GRID_CAP ? n_tiles : PFB_GRID_CAP)), dim3(PFB_T), 0, PSS_STREAM(ctx),
                       n_buf > 0 ? reinterpret_cast<const float2 *>(d_iq) : reinterpret_cast<const float2 *>(base), buf_index0, buf_index0 + n_buf,
                       reinterpret_cast<const double *>(base), reinterpret_cast<const double *>(base + o_taps), n_chan, log2_of(n_chan), decim, n_taps,
                       m_begin * decim + lead, n_m, R, tile_row(n_chan), n_tiles, reinterpret_cast<float2 *>(d_out), out_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_pfb launch");
}

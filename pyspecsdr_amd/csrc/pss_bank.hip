// pss_bank.hip — the channeliser for band plans: "every channel of this capture's uniform grid of M = 2^a 3^b 5^c channels at fs / D" as one
// call.  The arithmetic is pss_bank.h's; this unit places it.  A power-of-two M is handed to pss_pfb / pss_h_pfb / pss_pfb_default_taps
// after the arguments have passed this unit's own check, so its bytes are pss_pfb's by construction; k_bank runs every other M.
//   k_bank  float64, k_pfb's three phases for a channel count that does not divide the workgroup.  G = BANK_T / M (rounded down) instants
//           fit side by side; W = M G threads work in phases 1 and 2, the other BANK_T - W (fewer than M) wait at the barriers.  A
//           workgroup walks tiles of R = ITEMS G consecutive output instants.  Per tile:
//           1. branch sums: thread tid < W owns first tap tid mod M of the instants tid / M + i G, i < ITEMS.  The lanes of a wavefront own
//              consecutive first taps, that is consecutive branches in descending order: they read consecutive samples and consecutive
//              taps.  The items of a thread share their first tap and with it every tap: a step is one tap load, ITEMS sample loads and
//              2 ITEMS fma, the chains in registers.  The span (up to 32 M samples) is never resident; samples and taps come through the
//              vector cache.  The branch of an item is a remainder: (j00 mod M) comes from the host, (m0 D) mod M is one 64-bit remainder
//              a tile, and an item adds its small offset with one 32-bit remainder — none inside the tap loop.  The sum lands in LDS at
//              the digit-reversed branch, read from the uploaded permutation.
//           2. the DFT of every instant of the tile in LDS, one barrier a stage.  A stage of radix r has M / r butterflies an instant:
//              thread (first tap kap, instant slot r0) takes butterfly kap mod (M / r) of the instants (kap / (M / r) + p r) G + r0,
//              p = 0, 1, ... — the W threads cover r G instants a pass, and a thread's place in the stage (block, t, its twiddles'
//              step) is found once a stage, not once a butterfly.
//           3. the R x M tile leaves LDS transposed, instant fastest, through all BANK_T threads: every channel row receives R contiguous
//              complex64 values.  Rows lie M | 1 (odd) slots apart in LDS, so this column read meets no bank twice.
// Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_bank.h"
#include "pss_chan.h"
#include "pss_ctx.h"

namespace {

using namespace pss_bk;

constexpr long BANK_GRID_CAP = 1024;            // workgroups of a launch: tiles past it are walked by a grid-stride loop

// iq: the caller's buffer, [lo, hi): the capture indices it holds (inside the capture: the host has checked) — everything else is zero (the
// host has checked that nothing else inside the capture is needed); element 0 of iq is readable even where [lo, hi) is empty.
// tw, taps, rev: the uploaded tables (build_twiddles, the caller's taps, digit_reverse of 0 .. M - 1).  j00: m_begin D + lead, the own
// sample of the first output, jm = j00 mod M; n_m: m_end - m_begin; n3, n5, n_st: the 3s, the 5s and all stages of M; G, RS:
// tile_group(M), tile_row(M).
__global__ __launch_bounds__(BANK_T) void k_bank(const float2 *__restrict__ iq, long lo, long hi, const double *__restrict__ tw,
                                                 const double *__restrict__ taps, const int *__restrict__ rev, int M, int n3, int n5, int n_st, int D,
                                                 int T, long j00, int jm, long n_m, int G, int RS, long n_tiles, float2 *__restrict__ out,
                                                 long out_stride)
{
    __shared__ double vr[TILE_SLOTS], vi[TILE_SLOTS];
    const int tid = threadIdx.x;
    const int R = ITEMS * G;
    const bool act = tid < M * G;
    const int kap = tid % M, r0 = tid / M;
    const int k_last = kap < T ? kap + (T - 1 - kap) / M * M : kap;   // the last tap of this thread's chains
    // this thread's butterfly in a stage of each radix: butterfly f of the instants (sub + p r) G + r0
    const int f5 = kap % (n5 ? M / 5 : M), sub5 = kap / (n5 ? M / 5 : M);
    const int f3 = kap % (n3 ? M / 3 : M), sub3 = kap / (n3 ? M / 3 : M);
    const int f2 = kap % (n_st > n3 + n5 ? M / 2 : M), sub2 = kap / (n_st > n3 + n5 ? M / 2 : M);
    // the transposed store: element e = tid + n BANK_T is instant e mod R of channel e / R
    const int c_first = tid / R, r_first = tid % R, c_step = BANK_T / R, r_step = BANK_T % R;
    const int g_step = (int)((unsigned)(G * D) % (unsigned)M);       // the branch moves by this from one item to the next
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long m0 = tile * R;                                 // the tile's first output, counted from m_begin
        const int cnt = n_m - m0 < R ? (int)(n_m - m0) : R;       // >= 1
        if (act) {
            // ---- 1. branch sums.  Thread item i is (instant r0 + i G, first tap kap).  jt: the oldest sample any chain of the tile may
            // touch; samples are addressed from there by a 32-bit offset (a tile's span is below 2^16 samples).
            const long tb = j00 + m0 * D - (T - 1) - lo;
            unsigned o[ITEMS];
            bool fast = cnt == R;
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const int r = r0 + i * G;
                const long j0 = j00 + (m0 + r) * D;
                o[i] = (unsigned)(r * D + (T - 1));               // j0 - jt: no smaller than any k
                fast = fast && j0 - k_last >= lo && j0 - kap < hi;
            }
            double ur[ITEMS], ui[ITEMS];
            if (fast) {
                // a whole tile and every sample of every chain in the buffer (all but the chains at the capture's ends): no test per step
                pss_pf::branch_sums<ITEMS>(kap, M, T, [&](int k) { return taps[k]; }, [&](int i, int k, float &xr, float &xi) {
                    const unsigned off = o[i] - (unsigned)k;
                    __builtin_assume(off < (1u << 16));
                    const float2 x = iq[tb + (long)off];          // = iq[j0_i - k - lo]
                    xr = x.x;
                    xi = x.y;
                }, ur, ui);
            } else {
                pss_pf::branch_sums<ITEMS>(kap, M, T, [&](int k) { return taps[k]; }, [&](int i, int k, float &xr, float &xi) {
                    // the load is unconditional (a sample that is zero or an instant past the tile's count reads element 0 and drops
                    // it), so that the loads of a step are in flight together
                    const long j = tb + lo + (long)(o[i] - (unsigned)k);
                    const bool in = j >= lo && j < hi && r0 + i * G < cnt;
                    const float2 x = iq[in ? j - lo : 0];
                    xr = in ? x.x : 0.0f;
                    xi = in ? x.y : 0.0f;
                }, ur, ui);
            }
            // the branch whose first tap is kap at item i: (j00 + (m0 + r0 + i G) D - kap) mod M
            const int tm = (int)((uint64_t)(m0 * D) % (uint64_t)M);
            int rho = (int)((unsigned)(jm + tm + r0 * D + (M - kap)) % (unsigned)M);
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const int r = r0 + i * G;
                if (r < cnt) {
                    const int pos = r * RS + rev[rho];
                    vr[pos] = ur[i];
                    vi[pos] = ui[i];
                }
                rho += g_step;
                rho -= rho >= M ? M : 0;
            }
        }
        __syncthreads();
        // ---- 2. the DFT of every instant
        int Np = 1;
        for (int s = 0; s < n_st; s++) {
            const int r = stage_radix(s, n3, n5), N = r * Np;
            if (act) {
                const int f = r == 5 ? f5 : r == 3 ? f3 : f2, sub = r == 5 ? sub5 : r == 3 ? sub3 : sub2;
                const int b = f / Np, t = f - b * Np;
                const int a = b * N + t, u = t * (M / N);
                for (int row = sub * G + r0; row < cnt; row += r * G) fly(r, vr, vi, row * RS + a, Np, u, tw);
            }
            Np = N;
            __syncthreads();
        }
        // ---- 3. one rounding, transposed store
        for (int c = c_first, r = r_first; c < M; c += c_step, r += r_step) {
            if (r >= R) {
                r -= R;
                c++;
                if (c >= M) break;
            }
            if (r < cnt) out[(size_t)c * out_stride + (m0 + r)] = make_float2((float)vr[r * RS + c], (float)vi[r * RS + c]);
        }
        __syncthreads();   // the next tile's branch sums overwrite what this loop reads
    }
}

// the host tables of one M, back to back: twiddles (2 M float64), the digit reversal (M int32)
struct Tables {
    int M = 0;
    std::vector<double> tw;
    std::vector<int> rev;
};

const Tables &host_tables(int M)
{
    static thread_local Tables t;
    if (t.M != M) {
        int n2, n3, n5;
        factor(M, n2, n3, n5);
        t.tw.resize(2 * (size_t)M);
        t.rev.resize(M);
        build_twiddles(M, t.tw.data());
        for (int rho = 0; rho < M; rho++) t.rev[rho] = digit_reverse(rho, M, n2, n3, n5);
        t.M = M;
    }
    return t;
}

// The argument rules of pss_bank and pss_h_bank: the channelisers' shared ones (pss_chan.h) with bank_ok for the channel count.
int bank_check(pss_ctx *ctx, const char *who, const void *iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim, const double *taps,
               int n_taps, int lead, long m_begin, long m_end, const void *out, long out_stride)
{
    return pss_chan_args_check(ctx, who, bank_ok(n_chan), "n_chan is not of the form 2^a 3^b 5^c in [2, 1024]", iq, n_buf, buf_index0, n_capture, n_chan,
                               decim, taps, n_taps, lead, m_begin, m_end, out, out_stride);
}

}  // namespace

extern "C" int pss_bank_default_taps(int n_chan, double *taps, int *n_taps)
{
    if (!n_taps || !bank_ok(n_chan)) return pss_fail(nullptr, PSS_E_ARG, "pss_bank_default_taps: n_chan is not of the form 2^a 3^b 5^c in [2, 1024]");
    if (pow2(n_chan)) return pss_pfb_default_taps(n_chan, taps, n_taps);
    *n_taps = pss_pf::DEFAULT_TAPS_PER_CHAN * n_chan + 1;
    if (!taps) return PSS_OK;
    return pss_design_firwin(*n_taps, 1.0 / (double)n_chan, taps);
}

extern "C" int pss_h_bank(const float *h_iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim, const double *taps, int n_taps, int lead,
                          long m_begin, long m_end, float *h_out, long out_stride)
{
    const int r = bank_check(nullptr, "pss_h_bank", h_iq, n_buf, buf_index0, n_capture, n_chan, decim, taps, n_taps, lead, m_begin, m_end, h_out, out_stride);
    if (r || m_begin == m_end) return r;
    if (pow2(n_chan)) return pss_h_pfb(h_iq, n_buf, buf_index0, n_capture, n_chan, decim, taps, n_taps, lead, m_begin, m_end, h_out, out_stride);
    const Tables &tab = host_tables(n_chan);
    pss_chan_host_loop(h_iq, n_buf, buf_index0, n_chan, m_begin, m_end, h_out, out_stride, [&](long m, auto x, double *vr, double *vi, float *y) {
        instant(m, n_chan, decim, taps, n_taps, lead, tab.tw.data(), tab.rev.data(), x, vr, vi, y);
    });
    return PSS_OK;
}

extern "C" int pss_bank(pss_ctx *ctx, const float *d_iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim, const double *taps, int n_taps,
                        int lead, long m_begin, long m_end, float *d_out, long out_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = bank_check(ctx, "pss_bank", d_iq, n_buf, buf_index0, n_capture, n_chan, decim, taps, n_taps, lead, m_begin, m_end, d_out, out_stride);
    if (r || m_begin == m_end) return r;
    if (pow2(n_chan)) return pss_pfb(ctx, d_iq, n_buf, buf_index0, n_capture, n_chan, decim, taps, n_taps, lead, m_begin, m_end, d_out, out_stride);
    // the host tables, back to back: twiddles, taps, digit reversal (pss_table_sync: uploaded when they differ from the device copy)
    const Tables &tab = host_tables(n_chan);
    const size_t o_taps = sizeof(double) * 2 * (size_t)n_chan, o_rev = o_taps + sizeof(double) * (size_t)n_taps, bytes = o_rev + sizeof(int) * (size_t)n_chan;
    std::vector<unsigned char> img(bytes);
    memcpy(img.data(), tab.tw.data(), o_taps);
    memcpy(img.data() + o_taps, taps, o_rev - o_taps);
    memcpy(img.data() + o_rev, tab.rev.data(), bytes - o_rev);
    r = pss_table_sync(ctx, &ctx->bank_tab, img.data(), bytes, "pss_bank tables");
    if (r) return r;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(ctx->bank_tab.dev);
    int n2, n3, n5;
    factor(n_chan, n2, n3, n5);
    const int G = tile_group(n_chan), R = tile_instants(n_chan);
    const long n_m = m_end - m_begin, n_tiles = (n_m + R - 1) / R, j00 = m_begin * decim + lead;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_bank");
    hipLaunchKernelGGL(k_bank, dim3((unsigned)(n_tiles < BANK_GRID_CAP ? n_tiles : BANK_GRID_CAP)), dim3(BANK_T), 0, PSS_STREAM(ctx),
                       n_buf > 0 ? reinterpret_cast<const float2 *>(d_iq) : reinterpret_cast<const float2 *>(base), buf_index0, buf_index0 + n_buf,
                       reinterpret_cast<const double *>(base), reinterpret_cast<const double *>(base + o_taps), reinterpret_cast<const int *>(base + o_rev),
                       n_chan, n3, n5, n2 + n3 + n5, decim, n_taps, j00, (int)(j00 % n_chan), n_m, G, tile_row(n_chan), n_tiles,
                       reinterpret_cast<float2 *>(d_out), out_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_bank launch");
}

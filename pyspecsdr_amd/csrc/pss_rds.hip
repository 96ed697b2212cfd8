// pss_rds.hip — RDS for broadcast FM: from rows of IQ to the groups a station sends.  The arithmetic is pss_rds.h's; this unit places it.
//   k_rds_front    discriminator + 57 kHz mixer + decimating FIR.  A workgroup walks (row, tile) pairs.  A tile is M outputs (pss_ddc.h:
//                  tile_outputs).  Per pair the span's (M - 1) D + T input samples are read once; the discriminator (float32) and the mix
//                  (float64) run ONCE per sample and the mixed sample goes to LDS by phase (sample j of the span at row j % D, column j / D),
//                  as in k_ddc.  Then every wavefront takes (tap block, 64 outputs) tasks and one lane per output adds the block sums.
//   k_rds_energy   one lane per (segment, offset): the matched filter's energy of the 64 samples of a timing segment at one offset.
//   k_rds_bits     one workgroup per row: the segments' offsets, the strobe counts and their prefix, then one lane per strobe.
//   k_rds_groups   one workgroup per row: one lane per bit position checks four blocks; ballots and prefix counts compact the hits.
// Compiled without contraction and with correctly rounded float32 division (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_chan.h"
#include "pss_ctx.h"
#include "pss_device.h"
#include "pss_rds.h"

namespace {

using namespace pss_rds;
using pss_dc::B;
using pss_dc::KNOTS;
using pss_dc::PART_CAP;
using pss_dc::STAGE_CAP;

// ---- front ------------------------------------------------------------------------------------------------------------------------------
constexpr int FR_T = 1024;                      // threads of a workgroup: 16 wavefronts beside the one LDS image of a CU
constexpr int FR_WAVES = FR_T / 64;
constexpr long FR_GRID_CAP = 2048;              // workgroups of a launch: pairs past it are walked by a grid-stride loop

// iq: the caller's buffer, rows x_stride samples apart, holding row indices [lo, hi) of every row; elements 0 and 1 are readable even where
// [lo, hi) is empty.  The discriminator sample of row index i exists where i >= 1 and both i - 1 and i lie in [lo, hi); every other one
// is zero (the host has checked that no output needs one that the buffer does not hold).  first0, n_m, M, L, ROW: as k_ddc.
__global__ __launch_bounds__(FR_T) void k_rds_front(const float2 *__restrict__ iq, long x_stride, long lo, long hi, const double *__restrict__ knots,
                                                    const double *__restrict__ taps, uint64_t nw, int D, int T, long first0, long n_m, int M, int L,
                                                    int ROW, long n_tiles, long n_pairs, float2 *__restrict__ out, long out_stride)
{
    __shared__ double zr[STAGE_CAP], zi[STAGE_CAP];
    __shared__ double pr[PART_CAP], pi[PART_CAP];
    __shared__ uint2 rcp[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 64) rcp[tid] = pss::RCP14_AB[tid];
    __syncthreads();
    const int NB = pss_dc::n_blocks(T);
    const int q0 = tid / L, r0 = tid - q0 * L, dq = FR_T / L, dr = FR_T - dq * L;
    for (long p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const long row = p / n_tiles, tile = p - row * n_tiles;
        const long m0 = tile * M;
        const int cnt = n_m - m0 < M ? (int)(n_m - m0) : M;       // >= 1
        const int span = (cnt - 1) * D + T;                       // <= L * ROW <= STAGE_CAP
        const long first = first0 + m0 * D;
        uint64_t ph = nw * (uint64_t)(first + tid);
        const uint64_t dph = nw * (uint64_t)FR_T;
        int q = q0, r = r0;
#pragma unroll 2
        for (int j = tid; j < span; j += FR_T) {
            // the loads, the discriminator and the rotor are unconditional: a sample that is zero reads element 0 and drops the result
            const long i = first + j;
            const bool in = i - 1 >= lo && i < hi;                // lo >= 0: i >= 1
            const size_t at = in ? (size_t)row * x_stride + (i - lo) : 1;
            const float2 c = iq[at], b = iq[at - 1];
            const float d = disc(c.x, c.y, b.x, b.y, [&](float im, float re) { return pss::atan2f_svml(im, re, rcp); });
            double a, e;
            mixed(d, ph, knots, a, e);
            const int pos = r * ROW + q;
            zr[pos] = in ? a : 0.0;
            zi[pos] = in ? e : 0.0;
            ph += dph;
            q += dq;
            r += dr;
            if (r >= L) { r -= L; q++; }
        }
        __syncthreads();
        // ---- (tap block, 64 outputs) tasks, k_ddc's loop word for word (tests/test_gpu_ddc.py pins that kernel's text, so the two kernels
        // each carry it): output m of the tile and tap k read span sample m D + (T - 1 - k); a task's 64 taps come in with one vector load
        // a task ahead of their use and are read back lane by lane as scalars
        const int G = (cnt + 63) >> 6;
        const int n_tasks = NB * G;
        int b = 0, g = wave;   // task t = b G + g, stepped without a division
        while (g >= G) { g -= G; b++; }
        auto block_taps = [&](int bb) { const int k = bb * B + lane; return k < T ? taps[k] : 0.0; };
        double hv = block_taps(b);   // b <= NB where the wavefront has no task: k >= T, nothing is read
        for (int t = wave; t < n_tasks; t += FR_WAVES) {
            int bn = b, gn = g + FR_WAVES;
            while (gn >= G) { gn -= G; bn++; }
            const double hn = block_taps(bn);
            const int m = g * 64 + lane;
            const int k0 = b * B, nk = T - k0 < B ? T - k0 : B;
            const int c0 = T - 1 - k0;
            int cq = c0 / L, cr = c0 - cq * L;   // wave-uniform: the row and the column offset of the block's first tap
            if (m < cnt) {
                double sr, si;
                pss_dc::block_sum([&](int kk) {
                    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(hv), kk), __builtin_amdgcn_readlane(__double2loint(hv), kk));
                }, nk, [&](int, double &vr, double &vi) {
                    const int pos = cr * ROW + cq + m;
                    vr = zr[pos];
                    vi = zi[pos];
                    if (--cr < 0) { cr = L - 1; cq--; }
                }, sr, si);
                pr[b * M + m] = sr;
                pi[b * M + m] = si;
            }
            hv = hn;
            b = bn;
            g = gn;
        }
        __syncthreads();
        // ---- one lane per output: the block sums in ascending order, one rounding, one store.  The next pair's staging writes zr / zi only,
        // and its tasks write pr / pi behind the barrier above, which every lane reaches after this loop.
        for (int m = tid; m < cnt; m += FR_T) {
            float yr, yi;
            pss_dc::combine(NB, [&](int bb, double &sr, double &si) { sr = pr[bb * M + m]; si = pi[bb * M + m]; }, yr, yi);
            out[(size_t)row * out_stride + (m0 + m)] = make_float2(yr, yi);
        }
    }
}

int front_check(pss_ctx *ctx, const char *who, const void *iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_capture, double fs,
                int decim, const double *taps, int n_taps, int lead, long m_begin, long m_end, const void *out, long out_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (!std::isfinite(fs) || !(fs > 2.0 * SUBCARRIER_HZ)) return bad("fs must be finite and above 114 000 (the 57 kHz subcarrier below the discriminator's Nyquist)");
    if (decim < 1 || decim > pss_dc::MAX_DECIM) return bad("decim outside [1, 4096]");
    if (n_taps < 1 || n_taps > pss_dc::MAX_TAPS) return bad("n_taps outside [1, 4097]");
    if (n_rows < 1) return bad("n_rows < 1");
    if (!taps) return bad("null taps");
    if (x_stride < n_buf) return bad("x_stride < n_buf");
    const int r = pss_chan_window_check(ctx, who, false, iq, n_buf, buf_index0, n_capture, decim, taps, n_taps, lead, m_begin, m_end, out, out_stride);
    if (r || m_begin == m_end) return r;
    // the discriminator of the first needed sample reads the sample before it
    long need_lo = m_begin * decim + lead - (n_taps - 1), need_hi = (m_end - 1) * decim + lead + 1;
    if (need_lo < 1) need_lo = 1;
    if (need_hi > n_capture) need_hi = n_capture;
    if (need_lo < need_hi && need_lo - 1 < buf_index0) return bad("an output needs a sample of the capture that the buffer does not hold");
    return PSS_OK;
}

// ---- bits -------------------------------------------------------------------------------------------------------------------------------
constexpr int EN_T = 256;                       // k_rds_energy: 16 segments x 16 offsets
constexpr int EN_SEGS = EN_T / SPB;
constexpr long EN_GRID_CAP = 16384;
constexpr int BT_T = 256;
constexpr long BT_GRID_CAP = 4096;
constexpr int SEG_MAX_STROBES = SEG_BITS + 1;

__global__ __launch_bounds__(EN_T) void k_rds_energy(const float2 *__restrict__ bb, long row_stride, long n, const double *__restrict__ pulse, int P,
                                                     int n_seg, long tiles_per_row, long n_tiles, double *__restrict__ E)
{
    __shared__ double p[MAX_PULSE];
    for (int u = threadIdx.x; u < P; u += EN_T) p[u] = pulse[u];
    __syncthreads();
    const int o = threadIdx.x & (SPB - 1), ds = threadIdx.x >> 4;
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long row = t / tiles_per_row;
        const int s = (int)(t - row * tiles_per_row) * EN_SEGS + ds;
        if (s >= n_seg) continue;
        const float2 *x = bb + (size_t)row * row_stride;
        E[((size_t)row * n_seg + s) * SPB + o] = seg_energy([&](long i, float &br, float &bi) { const float2 v = x[i]; br = v.x; bi = v.y; }, n, p, P, s, o);
    }
}

// E [n_rows][n_seg][16] in; off, base: int32 [n_rows][n_seg] scratch
__global__ __launch_bounds__(BT_T) void k_rds_bits(const float2 *__restrict__ bb, long row_stride, long n, const double *__restrict__ pulse, int P,
                                                   int n_seg, long n_rows, const double *__restrict__ E, int32_t *__restrict__ off_all,
                                                   int32_t *__restrict__ base_all, uint8_t *__restrict__ bits, long max_bits, int32_t *__restrict__ n_bits)
{
    __shared__ double p[MAX_PULSE];
    __shared__ int scan[BT_T];
    __shared__ int carry;
    const int tid = threadIdx.x;
    for (int u = tid; u < P; u += BT_T) p[u] = pulse[u];
    for (long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const float2 *x = bb + (size_t)row * row_stride;
        const double *Er = E + (size_t)row * n_seg * SPB;
        int32_t *off = off_all + (size_t)row * n_seg, *base = base_all + (size_t)row * n_seg;
        auto Bx = [&](long i, float &br, float &bi) { const float2 v = x[i]; br = v.x; bi = v.y; };
        __syncthreads();   // the pulse is in place; the previous row's readers of `carry` are done
        for (int s = tid; s < n_seg; s += BT_T) off[s] = seg_offset(Er, n_seg, s);
        if (tid == 0) carry = 0;
        __syncthreads();
        // the strobe counts and their exclusive prefix, 256 segments a pass
        for (int s0 = 0; s0 < n_seg; s0 += BT_T) {
            const int s = s0 + tid;
            const int c = s < n_seg ? strobes_total(seg_strobes(s, s > 0 ? off[s - 1] : 0, off[s], n)) : 0;
            scan[tid] = c;
            __syncthreads();
            for (int d = 1; d < BT_T; d <<= 1) {
                const int v = tid >= d ? scan[tid - d] : 0;
                __syncthreads();
                scan[tid] += v;
                __syncthreads();
            }
            if (s < n_seg) base[s] = carry + scan[tid] - c;
            __syncthreads();
            if (tid == BT_T - 1) carry += scan[tid];
            __syncthreads();
        }
        const int total = carry;
        if (tid == 0) n_bits[row] = total > 0 ? total - 1 : 0;
        // one lane per strobe: strobe g of the row against strobe g - 1 gives bit g - 1
        const long n_work = (long)n_seg * SEG_MAX_STROBES;
        for (long w = tid; w < n_work; w += BT_T) {
            const int s = (int)(w / SEG_MAX_STROBES), k = (int)(w - (long)s * SEG_MAX_STROBES);
            const int o_prev = s > 0 ? off[s - 1] : 0;
            const Strobes st = seg_strobes(s, o_prev, off[s], n);
            if (k >= strobes_total(st)) continue;
            const long g = (long)base[s] + k;
            if (g == 0 || g - 1 >= max_bits) continue;
            const long t1 = strobe_at(st, k), t0 = k > 0 ? strobe_at(st, k - 1) : last_of_prev(s, o_prev);
            double ar, ai, yr, yi;
            matched(Bx, n, p, P, t0, ar, ai);
            matched(Bx, n, p, P, t1, yr, yi);
            bits[(size_t)row * max_bits + (g - 1)] = data_bit(ar, ai, yr, yi);
        }
    }
}

int bits_check(pss_ctx *ctx, const char *who, const void *bb, long n_rows, long row_stride, long n, const double *pulse, int n_pulse, const void *bits,
               long max_bits, const void *n_bits)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (n_rows < 1) return bad("n_rows < 1");
    if (n < 0 || n > MAX_ROW) return bad("n outside [0, 2^30]");
    if (row_stride < n) return bad("row_stride < n");
    if (max_bits < 0 || max_bits > MAX_ROW) return bad("max_bits outside [0, 2^30]");
    if (!pulse || n_pulse < 1 || n_pulse > MAX_PULSE || !(n_pulse & 1)) return bad("n_pulse must be odd and in [1, 257]");
    for (int u = 0; u < n_pulse; u++)
        if (!std::isfinite(pulse[u])) return bad("a pulse tap that is not finite");
    if (!n_bits || (n > 0 && !bb) || (max_bits > 0 && !bits)) return bad("null buffer");
    return PSS_OK;
}

// ---- groups -----------------------------------------------------------------------------------------------------------------------------
constexpr int GR_T = 256;
constexpr long GR_GRID_CAP = 4096;

__global__ __launch_bounds__(GR_T) void k_rds_groups(const uint8_t *__restrict__ bits, const int32_t *__restrict__ n_bits, long n_rows, long max_bits,
                                                     uint16_t *__restrict__ groups, int32_t *__restrict__ pos, int max_groups, int32_t *__restrict__ n_groups)
{
    __shared__ int wcount[GR_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const uint8_t *b = bits + (size_t)row * max_bits;
        long nb = n_bits[row];
        if (nb > max_bits) nb = max_bits;
        const long n_pos = nb - GROUP + 1;      // positions a whole group fits at
        int total = 0;                          // the same in every lane
        for (long i0 = 0; i0 < n_pos; i0 += GR_T) {
            const long i = i0 + tid;
            uint16_t g[4];
            const bool ok = i < n_pos && group_at(b, i, g);
            const unsigned long long mask = __ballot(ok);
            if (lane == 0) wcount[wave] = __popcll(mask);
            __syncthreads();
            int before = total, all = 0;
            for (int w = 0; w < GR_T / 64; w++) {
                if (w < wave) before += wcount[w];
                all += wcount[w];
            }
            __syncthreads();
            const int k = before + __popcll(mask & ((1ull << lane) - 1ull));
            if (ok && k < max_groups) {
                uint16_t *o = groups + ((size_t)row * max_groups + k) * 4;
                o[0] = g[0], o[1] = g[1], o[2] = g[2], o[3] = g[3];
                pos[(size_t)row * max_groups + k] = (int32_t)i;
            }
            total += all;
        }
        if (tid == 0) n_groups[row] = total;
    }
}

int groups_check(pss_ctx *ctx, const char *who, const void *bits, const void *n_bits, long n_rows, long max_bits, const void *groups, const void *pos,
                 int max_groups, const void *n_groups)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (n_rows < 1) return bad("n_rows < 1");
    if (max_bits < 0 || max_bits > MAX_ROW) return bad("max_bits outside [0, 2^30]");
    if (max_groups < 0) return bad("max_groups < 0");
    if (!n_bits || !n_groups || (max_bits > 0 && !bits) || (max_groups > 0 && (!groups || !pos))) return bad("null buffer");
    return PSS_OK;
}

}  // namespace

// ---- plan and pulse -----------------------------------------------------------------------------------------------------------------------
extern "C" int pss_rds_plan(double fs, int *decim, int *up, int *down)
{
    auto bad = [&](const char *why) { return pss_fail(nullptr, PSS_E_ARG, std::string("pss_rds: ") + why); };
    if (!decim || !up || !down) return bad("null argument");
    if (!std::isfinite(fs) || fs != floor(fs) || fs > 0x1p52) return bad("fs must be an integer number of Hz");
    if (!(fs > 120000.0)) return bad("fs must be above 120 000 (the discriminator's Nyquist must clear 59.4 kHz)");
    if (!plan((long)fs, *decim, *up, *down)) return bad("19 000 decim / fs reduces to factors outside [1, 4096], which pss_resample does not take");
    return PSS_OK;
}

extern "C" int pss_rds_default_pulse(int span_bits, double *pulse, int *n_pulse)
{
    if (!n_pulse || span_bits < 1 || span_bits > MAX_SPAN)
        return pss_fail(nullptr, PSS_E_ARG, "pss_rds_default_pulse: span_bits outside [1, 16] (16 span_bits + 1 taps, at most 257)");
    *n_pulse = pulse_len(span_bits);
    if (pulse) default_pulse(span_bits, pulse);
    return PSS_OK;
}

// ---- front ------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_rds_front(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_capture, double fs, int decim,
                               const double *taps, int n_taps, int lead, long m_begin, long m_end, float *h_out, long out_stride)
{
    const int r = front_check(nullptr, "pss_h_rds_front", h_iq, n_rows, x_stride, n_buf, buf_index0, n_capture, fs, decim, taps, n_taps, lead, m_begin,
                              m_end, h_out, out_stride);
    if (r || m_begin == m_end) return r;
    const double *knots = pss_host_knots();
    const uint64_t w = pss_dc::word_of(SUBCARRIER_HZ, fs);
    const long lo = buf_index0, hi = buf_index0 + n_buf;
    const long run = 4096;
    std::vector<double> z;
    for (long row = 0; row < n_rows; row++) {
        const float *x = h_iq + 2 * (size_t)row * x_stride;
        for (long a = m_begin; a < m_end; a += run) {
            const long e = a + run < m_end ? a + run : m_end;
            const long first = a * decim + lead - (n_taps - 1), span = (e - 1 - a) * decim + n_taps;
            z.assign((size_t)span * 2, 0.0);
            for (long j = 0; j < span; j++) {
                const long i = first + j;
                if (!(i - 1 >= lo && i < hi)) continue;
                const float *c = x + 2 * (i - lo), *b = c - 2;
                mixed(disc(c[0], c[1], b[0], b[1], pss_h_atan2f_model), pss_dc::phase_of(w, i), knots, z[2 * j], z[2 * j + 1]);
            }
            for (long m = a; m < e; m++) {
                float *o = h_out + 2 * ((size_t)row * out_stride + (m - m_begin));
                pss_dc::output(m, decim, taps, n_taps, lead, [&](long i, double &vr, double &vi) { vr = z[2 * (i - first)]; vi = z[2 * (i - first) + 1]; },
                               o[0], o[1]);
            }
        }
    }
    return PSS_OK;
}

extern "C" int pss_rds_front(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_capture, double fs,
                             int decim, const double *taps, int n_taps, int lead, long m_begin, long m_end, float *d_out, long out_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = front_check(ctx, "pss_rds_front", d_iq, n_rows, x_stride, n_buf, buf_index0, n_capture, fs, decim, taps, n_taps, lead, m_begin, m_end, d_out,
                        out_stride);
    if (r || m_begin == m_end) return r;
    if ((reinterpret_cast<uintptr_t>(d_iq) & 7) || (reinterpret_cast<uintptr_t>(d_out) & 7))
        return pss_fail(ctx, PSS_E_ARG, "pss_rds_front: d_iq and d_out must be 8-byte aligned");
    // the host tables, back to back: knots, taps (pss_table_sync: uploaded when they differ from the device copy)
    const size_t o_taps = sizeof(double) * 2 * KNOTS, bytes = o_taps + sizeof(double) * (size_t)n_taps;
    std::vector<unsigned char> tab(bytes);
    memcpy(tab.data(), pss_host_knots(), o_taps);
    memcpy(tab.data() + o_taps, taps, bytes - o_taps);
    r = pss_table_sync(ctx, &ctx->rds_tab, tab.data(), bytes, "pss_rds_front tables");
    if (r) return r;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(ctx->rds_tab.dev);
    const int M = pss_dc::tile_outputs(decim, n_taps);
    const int L = M == 1 ? 1 : decim, ROW = pss_dc::tile_row(M, decim, n_taps);
    const long n_tiles = (m_end - m_begin + M - 1) / M;
    if (n_tiles > INT64_MAX / n_rows) return pss_fail(ctx, PSS_E_ARG, "pss_rds_front: too many (row, tile) pairs");
    const long n_pairs = n_tiles * n_rows;
    const uint64_t nw = 0 - pss_dc::word_of(SUBCARRIER_HZ, fs);
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_rds_front");
    hipLaunchKernelGGL(k_rds_front, dim3((unsigned)(n_pairs < FR_GRID_CAP ? n_pairs : FR_GRID_CAP)), dim3(FR_T), 0, PSS_STREAM(ctx),
                       // (a buffer of fewer than two samples holds no discriminator sample: the idle lanes' reads go to the table)
                       n_buf > 1 ? reinterpret_cast<const float2 *>(d_iq) : reinterpret_cast<const float2 *>(base), x_stride, buf_index0, buf_index0 + n_buf,
                       reinterpret_cast<const double *>(base), reinterpret_cast<const double *>(base + o_taps), nw, decim, n_taps,
                       m_begin * decim + lead - (n_taps - 1), m_end - m_begin, M, L, ROW, n_tiles, n_pairs, reinterpret_cast<float2 *>(d_out), out_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_rds_front launch");
}

// ---- bits -------------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_rds_bits(const float *h_bb, long n_rows, long row_stride, long n, const double *pulse, int n_pulse, uint8_t *h_bits, long max_bits,
                              int32_t *h_n_bits)
{
    const int r = bits_check(nullptr, "pss_h_rds_bits", h_bb, n_rows, row_stride, n, pulse, n_pulse, h_bits, max_bits, h_n_bits);
    if (r) return r;
    const int n_seg = n_segments(n);
    std::vector<double> E((size_t)n_seg * SPB), yr, yi;
    std::vector<int> off(n_seg);
    for (long row = 0; row < n_rows; row++) {
        const float *x = h_bb + 2 * (size_t)row * row_stride;
        auto Bx = [&](long i, float &br, float &bi) { br = x[2 * i]; bi = x[2 * i + 1]; };
        for (int s = 0; s < n_seg; s++)
            for (int o = 0; o < SPB; o++) E[(size_t)s * SPB + o] = seg_energy(Bx, n, pulse, n_pulse, s, o);
        for (int s = 0; s < n_seg; s++) off[s] = seg_offset(E.data(), n_seg, s);
        long g = 0;
        double ar = 0.0, ai = 0.0;
        for (int s = 0; s < n_seg; s++) {
            const Strobes st = seg_strobes(s, s > 0 ? off[s - 1] : 0, off[s], n);
            for (int k = 0; k < strobes_total(st); k++, g++) {
                double vr, vi;
                matched(Bx, n, pulse, n_pulse, strobe_at(st, k), vr, vi);
                if (g > 0 && g - 1 < max_bits) h_bits[(size_t)row * max_bits + (g - 1)] = data_bit(ar, ai, vr, vi);
                ar = vr;
                ai = vi;
            }
        }
        h_n_bits[row] = (int32_t)(g > 0 ? g - 1 : 0);
    }
    return PSS_OK;
}

extern "C" int pss_rds_bits(pss_ctx *ctx, const float *d_bb, long n_rows, long row_stride, long n, const double *pulse, int n_pulse, uint8_t *d_bits,
                            long max_bits, int32_t *d_n_bits)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = bits_check(ctx, "pss_rds_bits", d_bb, n_rows, row_stride, n, pulse, n_pulse, d_bits, max_bits, d_n_bits);
    if (r) return r;
    if ((reinterpret_cast<uintptr_t>(d_bb) & 7) || (reinterpret_cast<uintptr_t>(d_n_bits) & 3))
        return pss_fail(ctx, PSS_E_ARG, "pss_rds_bits: d_bb must be 8-byte aligned, d_n_bits 4-byte aligned");
    r = pss_table_sync(ctx, &ctx->rds_pulse, pulse, sizeof(double) * (size_t)n_pulse, "pss_rds_bits pulse");
    if (r) return r;
    const double *d_pulse = reinterpret_cast<const double *>(ctx->rds_pulse.dev);
    const int n_seg = n_segments(n);
    // scratch: E [n_rows][n_seg][16] float64, then the offsets and the strobe prefix [n_rows][n_seg] int32 each (one element at least)
    const size_t cells = (size_t)n_rows * (n_seg > 0 ? n_seg : 1);
    const size_t o_off = cells * SPB * sizeof(double), o_base = o_off + cells * sizeof(int32_t);
    r = pss_ensure_scratch(ctx, o_base + cells * sizeof(int32_t));
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->scratch);
    double *E = reinterpret_cast<double *>(base);
    const float2 *bb = reinterpret_cast<const float2 *>(d_bb);
    PssTimeScope timed(ctx);
    if (n_seg > 0) {
        const long tiles_per_row = (n_seg + EN_SEGS - 1) / EN_SEGS, n_tiles = tiles_per_row * n_rows;
        pss_kernel_begin(ctx, "k_rds_energy");
        hipLaunchKernelGGL(k_rds_energy, dim3((unsigned)(n_tiles < EN_GRID_CAP ? n_tiles : EN_GRID_CAP)), dim3(EN_T), 0, PSS_STREAM(ctx), bb, row_stride, n,
                           d_pulse, n_pulse, n_seg, tiles_per_row, n_tiles, E);
        pss_kernel_end(ctx);
        r = pss_hip_check(ctx, hipGetLastError(), "k_rds_energy launch");
        if (r) return r;
    }
    pss_kernel_begin(ctx, "k_rds_bits");
    hipLaunchKernelGGL(k_rds_bits, dim3((unsigned)(n_rows < BT_GRID_CAP ? n_rows : BT_GRID_CAP)), dim3(BT_T), 0, PSS_STREAM(ctx), bb, row_stride, n, d_pulse,
                       n_pulse, n_seg, n_rows, E, reinterpret_cast<int32_t *>(base + o_off), reinterpret_cast<int32_t *>(base + o_base), d_bits, max_bits,
                       d_n_bits);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_rds_bits launch");
}

// ---- groups -----------------------------------------------------------------------------------------------------------------------------
extern "C" int pss_h_rds_groups(const uint8_t *h_bits, const int32_t *h_n_bits, long n_rows, long max_bits, uint16_t *h_groups, int32_t *h_pos,
                                int max_groups, int32_t *h_n_groups)
{
    const int r = groups_check(nullptr, "pss_h_rds_groups", h_bits, h_n_bits, n_rows, max_bits, h_groups, h_pos, max_groups, h_n_groups);
    if (r) return r;
    for (long row = 0; row < n_rows; row++) {
        const uint8_t *b = h_bits + (size_t)row * max_bits;
        long nb = h_n_bits[row];
        if (nb > max_bits) nb = max_bits;
        int total = 0;
        for (long i = 0; i + GROUP <= nb; i++) {
            uint16_t g[4];
            if (!group_at(b, i, g)) continue;
            if (total < max_groups) {
                memcpy(h_groups + ((size_t)row * max_groups + total) * 4, g, sizeof(g));
                h_pos[(size_t)row * max_groups + total] = (int32_t)i;
            }
            total++;
        }
        h_n_groups[row] = total;
    }
    return PSS_OK;
}

extern "C" int pss_rds_groups(pss_ctx *ctx, const uint8_t *d_bits, const int32_t *d_n_bits, long n_rows, long max_bits, uint16_t *d_groups,
                              int32_t *d_pos, int max_groups, int32_t *d_n_groups)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    const int r = groups_check(ctx, "pss_rds_groups", d_bits, d_n_bits, n_rows, max_bits, d_groups, d_pos, max_groups, d_n_groups);
    if (r) return r;
    if ((reinterpret_cast<uintptr_t>(d_groups) & 1) || ((reinterpret_cast<uintptr_t>(d_pos) | reinterpret_cast<uintptr_t>(d_n_bits) |
                                                         reinterpret_cast<uintptr_t>(d_n_groups)) & 3))
        return pss_fail(ctx, PSS_E_ARG, "pss_rds_groups: a misaligned device pointer");
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_rds_groups");
    hipLaunchKernelGGL(k_rds_groups, dim3((unsigned)(n_rows < GR_GRID_CAP ? n_rows : GR_GRID_CAP)), dim3(GR_T), 0, PSS_STREAM(ctx), d_bits, d_n_bits, n_rows,
                       max_bits, d_groups, d_pos, max_groups, d_n_groups);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_rds_groups launch");
}

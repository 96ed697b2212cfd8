// pss_ddc.hip — the K-channel digital down-converter: "these K channels of this capture at fs / D" as one call.  The arithmetic is
// pss_ddc.h's; this unit places it.
//   k_ddc   float64.  A workgroup walks (tile, channel) pairs, tile-major, so that the channels of one tile read the same IQ close together.
//           A tile is M outputs (pss_ddc.h: tile_outputs).  Per pair: the span's (M - 1) D + T samples are read once, mixed once (rotor and
//           product in float64) and stored to LDS by phase (sample j of the span at row j % D, column j / D) — lanes that own consecutive
//           outputs read consecutive float64 slots, whatever D is.  Then every wavefront takes (tap block, 64 outputs) tasks: the block's taps
//           are wave-uniform (one vector load a task, read back lane by lane as scalars), each lane runs the block's fma chain for its own
//           output and leaves the block sum in LDS.
//           After a barrier one lane per output adds the block sums in ascending order, rounds once and stores.
// Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_chan.h"
#include "pss_ctx.h"
#include "pss_ddc.h"

namespace {

using namespace pss_dc;

constexpr int DDC_T = 1024;                     // threads of a workgroup: 16 wavefronts, four per SIMD beside the one 156 KiB LDS image of a CU
constexpr int DDC_WAVES = DDC_T / 64;
constexpr long DDC_GRID_CAP = 2048;             // workgroups of a launch: pairs past it are walked by a grid-stride loop

// iq: the caller's buffer, [lo, hi): the capture indices it holds (inside the capture: the host has checked) — everything else is zero (the host has checked that nothing else inside the capture is needed); element 0 of iq is readable
// even where [lo, hi) is empty.  first0: the capture index of the first sample output m_begin needs, m_begin D + lead - (T - 1); n_m: m_end - m_begin.
// L: the phases of the LDS layout, D, or 1 where a tile is one output; ROW: float64 slots of a phase row.
__global__ __launch_bounds__(DDC_T) void k_ddc(const float2 *__restrict__ iq, long lo, long hi, const double *__restrict__ knots,
                                               const double *__restrict__ taps, const uint64_t *__restrict__ words, int K, int D, int T, long first0,
                                               long n_m, int M, int L, int ROW, long n_pairs, float2 *__restrict__ out, long out_stride)
{
    __shared__ double zr[STAGE_CAP], zi[STAGE_CAP];
    __shared__ double pr[PART_CAP], pi[PART_CAP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NB = n_blocks(T);
    // span sample j sits at (j % L) * ROW + j / L; a thread's samples are DDC_T apart, so it steps (row, column) instead of dividing
    const int q0 = tid / L, r0 = tid - q0 * L, dq = DDC_T / L, dr = DDC_T - dq * L;
    for (long p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const long tile = p / K;
        const int ch = (int)(p - tile * K);
        const long m0 = tile * M;                                 // the tile's first output, counted from m_begin
        const int cnt = n_m - m0 < M ? (int)(n_m - m0) : M;       // >= 1
        const int span = (cnt - 1) * D + T;                       // <= L * ROW <= STAGE_CAP
        const long first = first0 + m0 * D;                       // capture index of span sample 0 (may be negative)
        const uint64_t nw = 0 - words[ch];
        // ---- mix the span into LDS: the phase of sample i is nw * i in wrapping integers, stepped by nw * DDC_T
        uint64_t ph = nw * (uint64_t)(first + tid);
        const uint64_t dph = nw * (uint64_t)DDC_T;
        int q = q0, r = r0;
#pragma unroll 2
        for (int j = tid; j < span; j += DDC_T) {
            // the load and the rotor are unconditional (a sample that is zero reads element 0 and drops the product), so that the loads
            // of several samples are in flight together
            const long i = first + j;
            const bool in = i >= lo && i < hi;
            const float2 x = iq[in ? i - lo : 0];
            double c, s, a, b;
            rotor(ph, knots, c, s);
            mix(x.x, x.y, c, s, a, b);
            const int pos = r * ROW + q;
            zr[pos] = in ? a : 0.0;
            zi[pos] = in ? b : 0.0;
            ph += dph;
            q += dq;
            r += dr;
            if (r >= L) { r -= L; q++; }
        }
        __syncthreads();
        // ---- (tap block, 64 outputs) tasks: output m of the tile and tap k read span sample m D + (T - 1 - k)
        const int G = (cnt + 63) >> 6;
        const int n_tasks = NB * G;
        // A task's 64 taps come in with ONE vector load, lane l holding tap k0 + l, a task ahead of their use (the load of the next task's
        // taps is in flight while this one's chains run); the chain reads tap kk out of lane kk (two v_readlane: a scalar operand again).
        int b = 0, g = wave;   // task t = b G + g, stepped without a division
        while (g >= G) { g -= G; b++; }
        auto block_taps = [&](int bb) { const int k = bb * B + lane; return k < T ? taps[k] : 0.0; };
        double hv = block_taps(b);   // b <= NB where the wavefront has no task: k >= T, nothing is read
        for (int t = wave; t < n_tasks; t += DDC_WAVES) {
            int bn = b, gn = g + DDC_WAVES;
            while (gn >= G) { gn -= G; bn++; }
            const double hn = block_taps(bn);
            const int m = g * 64 + lane;
            const int k0 = b * B, nk = T - k0 < B ? T - k0 : B;
            const int c0 = T - 1 - k0;
            int cq = c0 / L, cr = c0 - cq * L;   // wave-uniform: the row and the column offset of the block's first tap
            if (m < cnt) {
                double sr, si;
                block_sum([&](int kk) {
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
        for (int m = tid; m < cnt; m += DDC_T) {
            float yr, yi;
            combine(NB, [&](int b, double &sr, double &si) { sr = pr[b * M + m]; si = pi[b * M + m]; }, yr, yi);
            out[(size_t)ch * out_stride + (m0 + m)] = make_float2(yr, yi);
        }
    }
}

// The argument rules of pss_ddc and pss_h_ddc.  ctx: where the reason goes (NULL: the library's own slot).
int ddc_check(pss_ctx *ctx, const char *who, const void *iq, long n_buf, long buf_index0, long n_capture, const uint64_t *words, int n_chan, int decim,
              const double *taps, int n_taps, int lead, long m_begin, long m_end, const void *out, long out_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (decim < 1 || decim > MAX_DECIM) return bad("decim outside [1, 4096]");
    if (n_taps < 1 || n_taps > MAX_TAPS) return bad("n_taps outside [1, 4097]");
    if (n_chan < 1) return bad("n_chan < 1");
    if (!words || !taps) return bad("null words or taps");
    return pss_chan_window_check(ctx, who, false, iq, n_buf, buf_index0, n_capture, decim, taps, n_taps, lead, m_begin, m_end, out, out_stride);
}

}  // namespace

extern "C" int pss_ddc_word(double offset_hz, double fs, uint64_t *word, double *effective_hz)
{
    if (!word || !std::isfinite(fs) || !(fs > 0.0) || !std::isfinite(offset_hz) || !(fabs(offset_hz) <= fs / 2.0))
        return pss_fail(nullptr, PSS_E_ARG, "pss_ddc_word: fs must be finite and > 0, |offset_hz| <= fs / 2");
    *word = word_of(offset_hz, fs);
    if (effective_hz) *effective_hz = pss_dc::effective_hz(*word, fs);
    return PSS_OK;
}

extern "C" long pss_ddc_out_len(long n_capture, int decim)
{
    if (n_capture < 0 || decim < 1 || decim > MAX_DECIM) return PSS_E_ARG;
    return out_len(n_capture, decim);
}

extern "C" int pss_ddc_default_taps(int decim, double *taps, int *n_taps)
{
    if (!n_taps || decim < 1 || decim > MAX_DEFAULT_DECIM)
        return pss_fail(nullptr, PSS_E_ARG, "pss_ddc_default_taps: decim outside [1, 204] (20 decim + 1 taps, at most 4097)");
    *n_taps = decim == 1 ? 1 : 20 * decim + 1;
    if (!taps) return PSS_OK;
    if (decim == 1) {
        taps[0] = 1.0;
        return PSS_OK;
    }
    return pss_design_firwin(*n_taps, 1.0 / (double)decim, taps);
}

extern "C" int pss_h_ddc_rotor(uint64_t word, long index0, long n, double *c, double *s)
{
    if (index0 < 0 || n < 0 || index0 > INT64_MAX - n || (n > 0 && (!c || !s)))
        return pss_fail(nullptr, PSS_E_ARG, "pss_h_ddc_rotor: index0, n >= 0 without overflow; c and s not null");
    const double *knots = pss_host_knots();
    for (long t = 0; t < n; t++) rotor(phase_of(word, index0 + t), knots, c[t], s[t]);
    return PSS_OK;
}

extern "C" int pss_h_ddc(const float *h_iq, long n_buf, long buf_index0, long n_capture, const uint64_t *words, int n_chan, int decim,
                         const double *taps, int n_taps, int lead, long m_begin, long m_end, float *h_out, long out_stride)
{
    const int r = ddc_check(nullptr, "pss_h_ddc", h_iq, n_buf, buf_index0, n_capture, words, n_chan, decim, taps, n_taps, lead, m_begin, m_end, h_out,
                            out_stride);
    if (r || m_begin == m_end) return r;
    const double *knots = pss_host_knots();
    // per channel and per run of outputs: the mixed samples once, then the outputs
    const long run = 4096;
    std::vector<double> z;
    for (int ch = 0; ch < n_chan; ch++) {
        for (long a = m_begin; a < m_end; a += run) {
            const long e = a + run < m_end ? a + run : m_end;
            const long first = a * decim + lead - (n_taps - 1), span = (e - 1 - a) * decim + n_taps;
            z.assign((size_t)span * 2, 0.0);
            for (long j = 0; j < span; j++) {
                const long i = first + j;
                if (i < 0 || i >= n_capture) continue;
                double c, s;
                rotor(phase_of(words[ch], i), knots, c, s);
                mix(h_iq[2 * (i - buf_index0)], h_iq[2 * (i - buf_index0) + 1], c, s, z[2 * j], z[2 * j + 1]);
            }
            for (long m = a; m < e; m++) {
                float *o = h_out + 2 * ((size_t)ch * out_stride + (m - m_begin));
                output(m, decim, taps, n_taps, lead, [&](long i, double &vr, double &vi) { vr = z[2 * (i - first)]; vi = z[2 * (i - first) + 1]; }, o[0], o[1]);
            }
        }
    }
    return PSS_OK;
}

extern "C" int pss_ddc(pss_ctx *ctx, const float *d_iq, long n_buf, long buf_index0, long n_capture, const uint64_t *words, int n_chan, int decim,
                       const double *taps, int n_taps, int lead, long m_begin, long m_end, float *d_out, long out_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = ddc_check(ctx, "pss_ddc", d_iq, n_buf, buf_index0, n_capture, words, n_chan, decim, taps, n_taps, lead, m_begin, m_end, d_out, out_stride);
    if (r || m_begin == m_end) return r;
    if ((reinterpret_cast<uintptr_t>(d_iq) & 7) || (reinterpret_cast<uintptr_t>(d_out) & 7))
        return pss_fail(ctx, PSS_E_ARG, "pss_ddc: d_iq and d_out must be 8-byte aligned");
    // the host tables, back to back: knots, taps, words (pss_table_sync: uploaded when they differ from the device copy)
    const size_t o_taps = sizeof(double) * 2 * KNOTS, o_words = o_taps + sizeof(double) * (size_t)n_taps;
    const size_t bytes = o_words + sizeof(uint64_t) * (size_t)n_chan;
    std::vector<unsigned char> tab(bytes);
    memcpy(tab.data(), pss_host_knots(), o_taps);
    memcpy(tab.data() + o_taps, taps, o_words - o_taps);
    memcpy(tab.data() + o_words, words, bytes - o_words);
    r = pss_table_sync(ctx, &ctx->ddc_tab, tab.data(), bytes, "pss_ddc tables");
    if (r) return r;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(ctx->ddc_tab.dev);
    const int M = tile_outputs(decim, n_taps);
    const int L = M == 1 ? 1 : decim, ROW = tile_row(M, decim, n_taps);
    const long n_tiles = (m_end - m_begin + M - 1) / M;
    if (n_tiles > INT64_MAX / n_chan) return pss_fail(ctx, PSS_E_ARG, "pss_ddc: too many (tile, channel) pairs");
    const long n_pairs = n_tiles * n_chan;
    const long lo = buf_index0, hi = buf_index0 + n_buf;   // inside the capture: ddc_check
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_ddc");
    hipLaunchKernelGGL(k_ddc, dim3((unsigned)(n_pairs < DDC_GRID_CAP ? n_pairs : DDC_GRID_CAP)), dim3(DDC_T), 0, PSS_STREAM(ctx),
                       n_buf > 0 ? reinterpret_cast<const float2 *>(d_iq) : reinterpret_cast<const float2 *>(base), lo, hi, reinterpret_cast<const double *>(base),
                       reinterpret_cast<const double *>(base + o_taps), reinterpret_cast<const uint64_t *>(base + o_words), n_chan, decim, n_taps,
                       m_begin * decim + lead - (n_taps - 1), m_end - m_begin, M, L, ROW, n_pairs, reinterpret_cast<float2 *>(d_out), out_stride);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_ddc launch");
}

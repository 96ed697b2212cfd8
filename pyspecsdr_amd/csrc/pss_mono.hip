// pss_mono.hip — the reference's decode_mono (signal_processing.py:331-359: broadcast FM to mono int16 at fs / 6) for batches of read
// buffers, and scipy.signal.lfilter for batches of rows (lowpass_filter, :28-31).  The arithmetic is pss_mono.h's; this unit places it.
//   k_mono_fwd   float32: discriminator -> 121-tap decimator by 6.  A workgroup takes a tile of up to FWD_TILE outputs of one frame,
//                computes each of the 6 T + 121 discriminator samples the tile needs ONCE into LDS and then walks the taps.
//   k_mono_bwd   float64: de-emphasis recurrence and mean.  One lane per frame, 64 frames per workgroup.
//   k_mono_out   float64: minus the mean, scale, int16 cast, element-wise.
//   k_lfilter    float64: one lane per row.
// Compiled without contraction and with correctly rounded float32 division (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pss_ctx.h"
#include "pss_device.h"
#include "pss_mono.h"

namespace {

using namespace pss_mono;

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
constexpr int FWD_T = 256;                      // threads of a workgroup
constexpr int FWD_TILE = 512;                   // outputs of a tile: two per lane
constexpr int FWD_PH = FWD_TILE + 24;           // floats of one phase row: output jr reads columns jr .. jr + 21
constexpr int FWD_SAMPLES = Q * (FWD_TILE - 1) + NHP;   // discriminator samples of a full tile
static_assert(FWD_SAMPLES <= Q * FWD_PH && FWD_TILE - 1 + (NHP - 1) / Q < FWD_PH, "a tile's samples fit the phase rows");
constexpr long FWD_GRID_CAP = 16384;            // workgroups of a launch: tiles past it are walked by a grid-stride loop

struct MonoTaps { float hp[NHP]; };             // by-value kernel argument: wave-uniform, read with scalar loads

// LDS: sample r of the tile (r = i - first sample index) sits at ph[r % 6][r / 6], so that the lanes of a wavefront, which read samples
// 6 apart, read consecutive words (a plain row would put lanes 6 dwords apart: two lanes on every bank).
__global__ __launch_bounds__(FWD_T) void k_mono_fwd(const float2 *__restrict__ iq, int n, long n_frames, int n_out, int tiles_per_frame, float gain,
                                                    MonoTaps taps, float *__restrict__ dec)
{
    __shared__ float ph[Q * FWD_PH];
    __shared__ uint2 rcp[64];
    const int tid = threadIdx.x;
    if (tid < 64) rcp[tid] = pss::RCP14_AB[tid];
    const int n_in = n - 1;
    const long n_tiles = n_frames * tiles_per_frame;
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long f = t / tiles_per_frame;
        const int j0 = (int)(t - f * tiles_per_frame) * FWD_TILE;
        const int cnt = n_out - j0 < FWD_TILE ? n_out - j0 : FWD_TILE;   // >= 1
        const long first = (long)Q * (j0 + DROP) - (NHP - 1);            // sample index of r = 0 (negative in the first tile)
        const int n_r = Q * (cnt - 1) + NHP;                             // <= FWD_SAMPLES
        const float2 *x = iq + (size_t)f * n;
        __syncthreads();   // the table is in place; the previous tile's readers are done
        for (int r = tid; r < n_r; r += FWD_T) {
            const long i = first + r;
            float v = 0.0f;
            if (i >= 0 && i < n_in) {
                const float2 a = x[i], b = x[i + 1];
                float re, im;
                disc_product(a.x, a.y, b.x, b.y, re, im);
                v = __fmul_rn(gain, pss::atan2f_svml(im, re, rcp));
            }
            ph[(r % Q) * FWD_PH + r / Q] = v;
        }
        __syncthreads();
        for (int jr = tid; jr < cnt; jr += FWD_T)
            dec[(size_t)f * n_out + j0 + jr] = fir_out([&](int m) { return ph[(m % Q) * FWD_PH + jr + m / Q]; }, taps.hp);
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
constexpr int BWD_F = 64;        // frames of a workgroup = its lanes (one wavefront)
constexpr int BWD_CH = 32;       // outputs of a staged chunk
constexpr int BWD_ROW = BWD_CH + 1;   // doubles of a staged row: lane f reads words 66 f + 2 k, the 32 lanes of a half on 64 different banks
constexpr long BWD_GRID_CAP = 2048;

// The de-emphasis recurrence and the mean of every frame, one lane per frame: Y [n_frames][n_out] (the caller's d_audio, scaled in place by
// k_mono_out, or scratch) and mean [n_frames].  Chunks of 64 rows x 32 outputs are staged through LDS, so that the loads of `dec` and the
// stores of Y run along the rows while every lane walks its own row.  The mean needs no second pass: np_sum (pss_npsum.h) asks for a row's
// elements in ascending order, each once, and every lane of the wavefront asks for the same index at the same time — the accessor stages the
// next chunk (wave-uniformly) when the index leaves the current one, runs the recurrence over it and hands the values out of LDS.
__global__ __launch_bounds__(BWD_F) void k_mono_bwd(const float *__restrict__ dec, long n_frames, int n_out, Deemph d, double *__restrict__ Y,
                                                    double *__restrict__ mean)
{
    __shared__ double buf[BWD_F * BWD_ROW];
    const int lane = threadIdx.x;
    const int col = lane & (BWD_CH - 1), row0 = lane >> 5;   // staging: two rows of a chunk per pass of the wavefront
    const long n_groups = (n_frames + BWD_F - 1) / BWD_F;
    for (long g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const long f0 = g * BWD_F;
        const int nf = n_frames - f0 < BWD_F ? (int)(n_frames - f0) : BWD_F;
        double z = 0.0;
        int cur = -1;
        auto stage = [&](int c) {   // chunks come in order 0, 1, 2, ...: z is the state behind chunk c - 1
            const int c0 = c * BWD_CH, cn = n_out - c0 < BWD_CH ? n_out - c0 : BWD_CH;
            float v[BWD_F / 2];
#pragma unroll
            for (int it = 0; it < BWD_F / 2; it++) {   // all loads of the chunk in flight before the first is used
                const int row = row0 + 2 * it;
                v[it] = row < nf && col < cn ? dec[(size_t)(f0 + row) * n_out + c0 + col] : 0.0f;
            }
            __syncthreads();   // the previous chunk's readers are done
#pragma unroll
            for (int it = 0; it < BWD_F / 2; it++) buf[(row0 + 2 * it) * BWD_ROW + col] = (double)v[it];
            __syncthreads();
            if (lane < nf)
                for (int k = 0; k < cn; k++) buf[lane * BWD_ROW + k] = deemph_step(d.b0, d.b1, d.a1, buf[lane * BWD_ROW + k], z);
            __syncthreads();
#pragma unroll
            for (int it = 0; it < BWD_F / 2; it++) {
                const int row = row0 + 2 * it;
                if (row < nf && col < cn) Y[(size_t)(f0 + row) * n_out + c0 + col] = buf[row * BWD_ROW + col];
            }
        };
        // every lane walks the sum, also those past the last frame (the staging is the wavefront's): their rows hold zeros
        const double m = row_mean([&](int i) {
            const int c = i / BWD_CH;
            if (c != cur) { stage(c); cur = c; }
            return buf[lane * BWD_ROW + (i - c * BWD_CH)];
        }, n_out);
        if (lane < nf) mean[f0 + lane] = m;
    }
}

// (y - mean) * 0.75 * 32768 and the cast, element-wise: a workgroup takes 256 outputs of one frame.  audio: NULL, or Y itself (in place).
constexpr int OUT_T = 256;
constexpr long OUT_GRID_CAP = 16384;
__global__ __launch_bounds__(OUT_T) void k_mono_out(const double *Y, const double *__restrict__ mean, long n_frames, int n_out, int tiles_per_frame,
                                                    double *audio, int16_t *__restrict__ pcm)
{
    const long n_tiles = n_frames * tiles_per_frame;
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long f = t / tiles_per_frame;
        const int k = (int)(t - f * tiles_per_frame) * OUT_T + threadIdx.x;
        if (k >= n_out) continue;
        const size_t o = (size_t)f * n_out + k;
        const double a = scale_audio(Y[o], mean[f]);
        if (audio) audio[o] = a;
        if (pcm) pcm[o] = pcm_cast(a);
    }
}

// ---- lfilter ---------------------------------------------------------------------------------------------------------------------------
constexpr int LF_T = 64;
constexpr long LF_GRID_CAP = 1024;
struct LfArg { double b[MAX_COEF], a[MAX_COEF]; };   // divided by a[0] on the host

template <int NC>
__global__ __launch_bounds__(LF_T) void k_lfilter(const double *__restrict__ x, double *__restrict__ y, int n, long n_rows, LfArg c)
{
    for (long r = (long)blockIdx.x * LF_T + threadIdx.x; r < n_rows; r += (long)gridDim.x * LF_T)
        lfilter_row<NC>(x + (size_t)r * n, n, c.b, c.a, y + (size_t)r * n);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// NumPy's float32 arctan2 on the host: pss_device.h's atan2f_svml, statement for statement (the same table through PSS_RCP14_ROWS), with
// fmaf for __fmaf_rn and memcpy for the bit casts.  The device routine is pinned against NumPy by the atan2f goldens; this one by the
// fm_mono goldens, whose decimated rows depend on every bit of it.
const uint32_t RCP14_HOST[64][2] = {PSS_RCP14_ROWS};

inline uint32_t hf2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline float hu2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

float h_rcp14f(float x)
{
    const uint32_t u = hf2u(x), sign = u & 0x80000000u, e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    const uint32_t idx = m >> 17, low = (m >> 7) & 1023u;
    const uint32_t v = (RCP14_HOST[idx][0] - RCP14_HOST[idx][1] * low) >> 9;
    const uint32_t r = sign | ((253u - e) << 23) | ((v & 0xffffu) << 7);
    const uint32_t r0 = sign | ((254u - e) << 23);
    return hu2f(m == 0 ? r0 : r);
}

float h_atan2f_svml(float y, float x)
{
    const float PIO2 = 0x1.921fb6p+0f, PI = 0x1.921fb6p+1f;
    const uint32_t xb = hf2u(x), yb = hf2u(y);
    const uint32_t axb = xb & 0x7fffffffu, ayb = yb & 0x7fffffffu;
    const uint32_t sx = xb & 0x80000000u, sy = yb & 0x80000000u;
    const float ax = hu2f(axb), ay = hu2f(ayb);
    const bool k1 = ay < ax;
    const float a = k1 ? ay : -ax;
    const float b = k1 ? ax : ay;
    if (!((fabsf(a) >= 0x1p-125f) && (b < 0x1p123f))) {   // atan2f_svml_rare
        if (x != x || y != y) return x + y;
        if (axb == 0 || ayb == 0) {
            float v = (!(ay < ax) && !(axb == 0 && ayb == 0)) ? PIO2 : 0.0f;
            v = hu2f(hf2u(v) | sx);
            if (sx) v = v + PI;
            return hu2f(hf2u(v) | sy);
        }
        return (float)atan2((double)y, (double)x);
    }
    const float base = k1 ? 0.0f : PIO2;
    const float r0 = h_rcp14f(b);
    const float e = fmaf(-b, r0, 1.0f);
    const float r1 = fmaf(r0, e, r0);
    const float q0 = a * r1;
    const float rem = fmaf(-b, q0, a);
    const float q = fmaf(rem, r1, q0);
    const float s = q * q;
    const float s2 = s * s;
    float pa = fmaf(s2, 0x1.64598p-9f, 0x1.578708p-5f);
    float pb = fmaf(s2, -0x1.fe4c62p-7f, -0x1.30ec52p-4f);
    pa = fmaf(pa, s2, 0x1.b2c8e8p-4f);
    pb = fmaf(pb, s2, -0x1.22c3fp-3f);
    pa = fmaf(pa, s2, 0x1.996f3ep-3f);
    pb = fmaf(pb, s2, -0x1.555492p-2f);
    pa = fmaf(pa, s2, 1.0f);
    const float p = fmaf(pb, s, pa);
    float r = fmaf(p, q, base);
    r = hu2f(hf2u(r) | sx);
    if (x <= 0.0f) r = r + PI;
    return hu2f(hf2u(r) | sy);
}

// the 127 padded taps: firwin(121, 1 / 6) behind resample_poly's 6 zeros, as float32 (independent of fs)
int mono_taps(float *hp)
{
    double t[NTAPS];
    const int r = pss_design_firwin(NTAPS, 1.0 / Q, t);
    if (r) return r;
    for (int k = 0; k < PRE; k++) hp[k] = 0.0f;
    for (int k = 0; k < NTAPS; k++) hp[PRE + k] = (float)t[k];
    return PSS_OK;
}

int mono_deemph(double fs, Deemph &d)
{
    double b[2], a[2];
    const int r = pss_design_deemph(75e-6, fs, b, a);
    if (r) return r;
    d = Deemph{b[0], b[1], a[1]};
    return PSS_OK;
}

bool lf_args_ok(const double *b, const double *a, int ncoef)
{
    return b && a && ncoef >= 2 && ncoef <= MAX_COEF && a[0] != 0.0 && std::isfinite(a[0]);
}

}  // namespace

// the host model of NumPy's float32 arctan2 for the other units' host twins (pss_rds.hip)
float pss_h_atan2f_model(float y, float x) { return h_atan2f_svml(y, x); }

// scipy.signal.bilinear([1], [tau, 1], fs): with M = 1 its loops leave bprime = [1, 1] and aprime = [1 + t, 1 - t], t = tau * (2 fs) (the
// products by the binomial coefficients 1.0 and by (-1) ** k are exact), and normalize() divides both by aprime[0].
extern "C" int pss_design_deemph(double tau, double fs, double b[2], double a[2])
{
    if (!b || !a || !(tau > 0.0) || !(fs > 0.0) || !std::isfinite(tau) || !std::isfinite(fs)) return PSS_E_ARG;
    const double t = tau * (2.0 * fs);
    const double a0 = 1.0 + t, a1 = 1.0 + -t;
    b[0] = 1.0 / a0;
    b[1] = 1.0 / a0;
    a[0] = a0 / a0;
    a[1] = a1 / a0;
    return PSS_OK;
}

extern "C" int pss_decode_mono_len(int n)
{
    return n < 0 ? PSS_E_ARG : out_len(n);
}

extern "C" int pss_h_decode_mono(const float *h_iq, int n, double fs, int16_t *h_pcm, double *h_audio, float *h_dec)
{
    if (n < 0 || (n > 0 && !h_iq) || !(fs > 0.0) || !std::isfinite(fs)) return pss_fail(nullptr, PSS_E_ARG, "pss_h_decode_mono: bad argument");
    if (out_len(n) == 0) return PSS_OK;
    float hp[NHP];
    Deemph d;
    int r = mono_taps(hp);
    if (!r) r = mono_deemph(fs, d);
    if (r) return r;
    std::vector<float> work((size_t)n - 1);
    std::vector<double> y((size_t)out_len(n));
    frame(h_iq, n, gain_of(fs), hp, d, h_atan2f_svml, work.data(), h_pcm, h_audio, h_dec, y.data());
    return PSS_OK;
}

extern "C" int pss_decode_mono(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, int16_t *d_pcm, double *d_audio, float *d_dec)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_frames < 0 || n < 0 || !(fs > 0.0) || !std::isfinite(fs)) return pss_fail(ctx, PSS_E_ARG, "pss_decode_mono: bad argument");
    const int n_out = out_len(n);
    if (n_frames == 0 || n_out == 0) return PSS_OK;
    if (!d_iq || (!d_pcm && !d_audio && !d_dec)) return pss_fail(ctx, PSS_E_ARG, "pss_decode_mono: null buffer");
    if (reinterpret_cast<uintptr_t>(d_iq) & 7) return pss_fail(ctx, PSS_E_ARG, "pss_decode_mono: d_iq must be 8-byte aligned");
    MonoTaps taps;
    Deemph d;
    int r = mono_taps(taps.hp);
    if (!r) r = mono_deemph(fs, d);
    if (r) return pss_fail(ctx, r, "pss_decode_mono: filter design failed");
    // scratch: the frames' means, the decimated rows unless the caller takes them, the de-emphasised rows unless the caller takes the audio
    const size_t rows = (size_t)n_frames * n_out;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t o_dec = up((size_t)n_frames * sizeof(double)), o_y = o_dec + (d_dec ? 0 : up(rows * sizeof(float)));
    r = pss_ensure_scratch(ctx, o_y + (d_audio ? 0 : rows * sizeof(double)));
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->scratch);
    double *mean = reinterpret_cast<double *>(base);
    float *dec = d_dec ? d_dec : reinterpret_cast<float *>(base + o_dec);
    double *Y = d_audio ? d_audio : reinterpret_cast<double *>(base + o_y);
    const int tiles_per_frame = (n_out + FWD_TILE - 1) / FWD_TILE;
    const long n_tiles = n_frames * tiles_per_frame;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_mono_fwd");
    hipLaunchKernelGGL(k_mono_fwd, dim3((unsigned)(n_tiles < FWD_GRID_CAP ? n_tiles : FWD_GRID_CAP)), dim3(FWD_T), 0, PSS_STREAM(ctx),
                       reinterpret_cast<const float2 *>(d_iq), n, n_frames, n_out, tiles_per_frame, gain_of(fs), taps, dec);
    pss_kernel_end(ctx);
    r = pss_hip_check(ctx, hipGetLastError(), "k_mono_fwd launch");
    if (r || (!d_pcm && !d_audio)) return r;
    const long n_groups = (n_frames + BWD_F - 1) / BWD_F;
    pss_kernel_begin(ctx, "k_mono_bwd");
    hipLaunchKernelGGL(k_mono_bwd, dim3((unsigned)(n_groups < BWD_GRID_CAP ? n_groups : BWD_GRID_CAP)), dim3(BWD_F), 0, PSS_STREAM(ctx), dec, n_frames,
                       n_out, d, Y, mean);
    pss_kernel_end(ctx);
    r = pss_hip_check(ctx, hipGetLastError(), "k_mono_bwd launch");
    if (r) return r;
    const int out_tiles = (n_out + OUT_T - 1) / OUT_T;
    const long n_out_tiles = n_frames * out_tiles;
    pss_kernel_begin(ctx, "k_mono_out");
    hipLaunchKernelGGL(k_mono_out, dim3((unsigned)(n_out_tiles < OUT_GRID_CAP ? n_out_tiles : OUT_GRID_CAP)), dim3(OUT_T), 0, PSS_STREAM(ctx), Y, mean,
                       n_frames, n_out, out_tiles, d_audio, d_pcm);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_mono_out launch");
}

extern "C" int pss_h_lfilter(const double *h_x, long n_rows, int n, const double *b, const double *a, int ncoef, double *h_y)
{
    if (n_rows < 0 || n < 0 || !lf_args_ok(b, a, ncoef)) return pss_fail(nullptr, PSS_E_ARG, "pss_h_lfilter: bad argument");
    if (n_rows == 0 || n == 0) return PSS_OK;
    if (!h_x || !h_y) return pss_fail(nullptr, PSS_E_ARG, "pss_h_lfilter: null buffer");
    double bn[MAX_COEF], an[MAX_COEF];
    lfilter_normalise(b, a, ncoef, bn, an);
    with_ncoef(ncoef, [&](auto nc) {
        for (long r = 0; r < n_rows; r++) lfilter_row<decltype(nc)::value>(h_x + (size_t)r * n, n, bn, an, h_y + (size_t)r * n);
    });
    return PSS_OK;
}

extern "C" int pss_lfilter(pss_ctx *ctx, const double *d_x, long n_rows, int n, const double *b, const double *a, int ncoef, double *d_y)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_rows < 0 || n < 0 || !lf_args_ok(b, a, ncoef)) return pss_fail(ctx, PSS_E_ARG, "pss_lfilter: bad argument");
    PSS_ALIGNED(ctx, "pss_lfilter", PSS_P(d_x, 8), PSS_P(d_y, 8));
    if (n_rows == 0 || n == 0) return PSS_OK;
    if (!d_x || !d_y) return pss_fail(ctx, PSS_E_ARG, "pss_lfilter: null buffer");
    LfArg c = {};
    lfilter_normalise(b, a, ncoef, c.b, c.a);
    const long blocks = (n_rows + LF_T - 1) / LF_T;
    const dim3 grid((unsigned)(blocks < LF_GRID_CAP ? blocks : LF_GRID_CAP));
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_lfilter");
    with_ncoef(ncoef, [&](auto nc) {
        hipLaunchKernelGGL(k_lfilter<decltype(nc)::value>, grid, dim3(LF_T), 0, PSS_STREAM(ctx), d_x, d_y, n, n_rows, c);
    });
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_lfilter launch");
}

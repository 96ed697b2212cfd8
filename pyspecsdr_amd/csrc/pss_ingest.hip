// pss_ingest.hip — read buffers as the radio's ADC delivers them: 8- and 16-bit integer codes widened to the complex64 buffer the driver
// would have handed the reference (SoapySDR CF32, pyspecsdr.py:1870-1891).  One flat HBM-bound pass; the arithmetic is either none (8-bit
// containers: a caller-supplied table of 256 float32 words, copied bit for bit) or one IEEE float32 division (int16 containers), which is
// why this unit is compiled without contraction and with correctly rounded division.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "pss_ctx.h"

namespace {

// The 8-bit table as a by-value kernel argument (1 KB of the kernarg segment: the call keeps nothing of the caller's and allocates nothing),
// indexed by the RAW byte: for PSS_IQ_S8 the host stores table[code + 128] at the code's two's-complement byte, w[b] = table[b ^ 0x80].
struct IqLut {
    uint32_t w[256];
};

// Output words [0, head) and [head + 4 * n_groups, n_words) are written one by one by two lanes of the first workgroup (head: 0 or 2 words
// up to the first 16-byte boundary of `out`; the tail: 0 or 2 words); between them every lane turns 4 codes into one 16-byte store, four such
// groups a grid stride apart in flight per lane.  VEC: the 4 codes of a group are one aligned load; otherwise (a code pointer that is not
// aligned like the output behind the head) four loads of the container's own width.
template <bool VEC>
__global__ __launch_bounds__(256) void k_unpack_iq(const uint8_t *__restrict__ codes, uint32_t *__restrict__ out, size_t n_words, unsigned head,
                                                   IqLut lut)
{
    __shared__ uint32_t t[256];
    t[threadIdx.x] = lut.w[threadIdx.x];
    __syncthreads();
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const size_t n_groups = (n_words - head) >> 2, tail0 = (size_t)head + (n_groups << 2);
    if (tid == 0)
        for (size_t w = 0; w < head; w++) out[w] = t[codes[w]];
    if (tid == 1)
        for (size_t w = tail0; w < n_words; w++) out[w] = t[codes[w]];
    const uint8_t *c = codes + head;
    uint4 *o = reinterpret_cast<uint4 *>(out + head);
    for (size_t g = tid; g < n_groups; g += 4 * stride) {
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t gi = g + (size_t)u * stride;
            if (gi >= n_groups) continue;
            if (VEC) v[u] = reinterpret_cast<const uint32_t *>(c)[gi];
            else v[u] = (uint32_t)c[4 * gi] | ((uint32_t)c[4 * gi + 1] << 8) | ((uint32_t)c[4 * gi + 2] << 16) | ((uint32_t)c[4 * gi + 3] << 24);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t gi = g + (size_t)u * stride;
            if (gi >= n_groups) continue;
            o[gi] = make_uint4(t[v[u] & 255u], t[(v[u] >> 8) & 255u], t[(v[u] >> 16) & 255u], t[v[u] >> 24]);
        }
    }
}

// word = (float)code / scale: one correctly rounded IEEE float32 division per word (this unit's compile flags).
template <bool VEC>
__global__ __launch_bounds__(256) void k_unpack_iq_s16(const int16_t *__restrict__ codes, float *__restrict__ out, size_t n_words, unsigned head,
                                                       float scale)
{
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const size_t n_groups = (n_words - head) >> 2, tail0 = (size_t)head + (n_groups << 2);
    if (tid == 0)
        for (size_t w = 0; w < head; w++) out[w] = (float)codes[w] / scale;
    if (tid == 1)
        for (size_t w = tail0; w < n_words; w++) out[w] = (float)codes[w] / scale;
    const int16_t *c = codes + head;
    float4 *o = reinterpret_cast<float4 *>(out + head);
    for (size_t g = tid; g < n_groups; g += 4 * stride) {
        short4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t gi = g + (size_t)u * stride;
            if (gi >= n_groups) continue;
            if (VEC) v[u] = reinterpret_cast<const short4 *>(c)[gi];
            else v[u] = make_short4(c[4 * gi], c[4 * gi + 1], c[4 * gi + 2], c[4 * gi + 3]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t gi = g + (size_t)u * stride;
            if (gi >= n_groups) continue;
            o[gi] = make_float4((float)v[u].x / scale, (float)v[u].y / scale, (float)v[u].z / scale, (float)v[u].w / scale);
        }
    }
}

const char *iq_check_msg(int container, double scale, const float *table256)
{
    if (container != PSS_IQ_U8 && container != PSS_IQ_S8 && container != PSS_IQ_S16) return "unknown IQ code container";
    if (container == PSS_IQ_S16) {
        if (table256) return "PSS_IQ_S16 takes a scale, not a table: table256 must be NULL";
        if (!(scale > 0.0) || !std::isfinite(scale)) return "PSS_IQ_S16: scale must be finite and > 0";
    } else if (!table256) {
        return "the 8-bit containers need the table of 256 float32 values";
    }
    return nullptr;
}

}  // namespace

int pss_iq_check(pss_ctx *ctx, int container, double scale, const float *h_table256)
{
    const char *msg = iq_check_msg(container, scale, h_table256);
    return msg ? pss_fail(ctx, PSS_E_ARG, msg) : PSS_OK;
}

extern "C" int pss_iq_code_bytes(int container)
{
    if (container == PSS_IQ_U8 || container == PSS_IQ_S8) return 2;
    if (container == PSS_IQ_S16) return 4;
    return -1;
}

extern "C" int pss_h_iq_table(int container, double scale, double offset, float *table256)
{
    if (container != PSS_IQ_U8 && container != PSS_IQ_S8) return pss_fail(nullptr, PSS_E_ARG, "pss_h_iq_table: an 8-bit container (PSS_IQ_U8 / PSS_IQ_S8)");
    if (!table256 || !(scale > 0.0) || !std::isfinite(scale) || !std::isfinite(offset))
        return pss_fail(nullptr, PSS_E_ARG, "pss_h_iq_table: table256 is null, or scale / offset is not finite, or scale <= 0");
    for (int i = 0; i < 256; i++) {
        const double code = container == PSS_IQ_U8 ? (double)i : (double)(i - 128);
        table256[i] = (float)((code - offset) / scale);
    }
    return PSS_OK;
}

extern "C" int pss_h_unpack_iq(int container, const void *codes, long n_samples, double scale, const float *table256, float *iq)
{
    int r = pss_iq_check(nullptr, container, scale, table256);
    if (r) return r;
    if (n_samples < 0 || (n_samples > 0 && (!codes || !iq))) return pss_fail(nullptr, PSS_E_ARG, "pss_h_unpack_iq: bad arguments");
    const size_t n_words = 2 * (size_t)n_samples;
    if (container == PSS_IQ_S16) {
        const float s = (float)scale;
        const unsigned char *c = static_cast<const unsigned char *>(codes);   // any address: the words are assembled from their bytes
        for (size_t w = 0; w < n_words; w++) iq[w] = (float)(int16_t)(uint16_t)(c[2 * w] | (c[2 * w + 1] << 8)) / s;
    } else {
        const uint8_t *c = static_cast<const uint8_t *>(codes);
        const unsigned flip = container == PSS_IQ_S8 ? 0x80u : 0u;
        for (size_t w = 0; w < n_words; w++) memcpy(iq + w, table256 + (c[w] ^ flip), sizeof(float));   // words, not values: a NaN keeps its payload
    }
    return PSS_OK;
}

extern "C" int pss_unpack_iq(pss_ctx *ctx, int container, const void *d_codes, long n_samples, double scale, const float *h_table256, float *d_iq)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = pss_iq_check(ctx, container, scale, h_table256);
    if (r) return r;
    if (n_samples < 0) return pss_fail(ctx, PSS_E_ARG, "pss_unpack_iq: n_samples < 0");
    if (n_samples == 0) return PSS_OK;
    if (!d_codes || !d_iq) return pss_fail(ctx, PSS_E_ARG, "pss_unpack_iq: null buffer");
    const uintptr_t a_in = reinterpret_cast<uintptr_t>(d_codes), a_out = reinterpret_cast<uintptr_t>(d_iq);
    if (a_out & 7) return pss_fail(ctx, PSS_E_ARG, "pss_unpack_iq: d_iq must be 8-byte aligned");
    if (container == PSS_IQ_S16 && (a_in & 1)) return pss_fail(ctx, PSS_E_ARG, "pss_unpack_iq: int16 codes must be 2-byte aligned");
    const size_t n_words = 2 * (size_t)n_samples;
    const unsigned head = (a_out & 15) ? 2u : 0u;   // words in front of the first 16-byte boundary of d_iq (n_words >= 2)
    const size_t n_groups = (n_words - head) >> 2;
    const size_t want = (n_groups + 1023) / 1024, cap = (size_t)(ctx->n_cus > 0 ? ctx->n_cus : 256) * 16;
    const dim3 grid((unsigned)(want < 1 ? 1 : (want < cap ? want : cap))), block(256);
    PssTimeScope timed(ctx);
    if (container == PSS_IQ_S16) {
        const int16_t *c = static_cast<const int16_t *>(d_codes);
        const bool vec = ((a_in + 2 * (uintptr_t)head) & 7) == 0;
        pss_kernel_begin(ctx, "k_unpack_iq_s16");
        if (vec) hipLaunchKernelGGL(k_unpack_iq_s16<true>, grid, block, 0, PSS_STREAM(ctx), c, d_iq, n_words, head, (float)scale);
        else hipLaunchKernelGGL(k_unpack_iq_s16<false>, grid, block, 0, PSS_STREAM(ctx), c, d_iq, n_words, head, (float)scale);
        pss_kernel_end(ctx);
    } else {
        IqLut lut;
        const unsigned flip = container == PSS_IQ_S8 ? 0x80u : 0u;
        for (unsigned b = 0; b < 256; b++) memcpy(&lut.w[b], h_table256 + (b ^ flip), sizeof(uint32_t));
        const uint8_t *c = static_cast<const uint8_t *>(d_codes);
        uint32_t *o = reinterpret_cast<uint32_t *>(d_iq);
        const bool vec = ((a_in + (uintptr_t)head) & 3) == 0;
        pss_kernel_begin(ctx, "k_unpack_iq");
        if (vec) hipLaunchKernelGGL(k_unpack_iq<true>, grid, block, 0, PSS_STREAM(ctx), c, o, n_words, head, lut);
        else hipLaunchKernelGGL(k_unpack_iq<false>, grid, block, 0, PSS_STREAM(ctx), c, o, n_words, head, lut);
        pss_kernel_end(ctx);
    }
    return pss_hip_check(ctx, hipGetLastError(), "k_unpack_iq launch");
}

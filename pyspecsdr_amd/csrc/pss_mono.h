// pss_mono.h — the arithmetic of the reference's decode_mono (signal_processing.py:331-359) and of scipy.signal.lfilter, stated ONCE for
// the kernels (pss_mono.hip), the host twins (pss_h_decode_mono, pss_h_lfilter) and the stand-alone host check (tests/mono_host.cpp).
//
// decode_mono(samples, fs), n complex64 samples, n_in = n - 1, n_out = ceil(n_in / 6):
//   product   samples[:-1] * samples.conj()[1:]: a = x[i], b = conj(x[i + 1]), NumPy's FMA form.  The operand roles are the reverse of
//             NFM's samples[1:] * conj(samples[:-1]), and NumPy swaps nothing at any length here (no temporary is elided: both operands
//             are views), so there is no `swapped` form.
//   angle     np.angle = float32 arctan2(im, re): the caller's model of NumPy's routine (device: pss_device.h atan2f_svml; host: the same
//             statements in pss_mono.hip).  This header takes it as a function argument.
//   gain      one float32 multiply by float32(fs / (2 pi pi 75e3)) — the second pi is the reference's.
//   decimate  scipy.signal.decimate(demod, 6, ftype="fir") in float32: resample_poly puts 6 zero taps in front of
//             firwin(121, 1 / 6, "hamming").astype(float32) and drops the first 11 outputs of upfirdn, whose loop is
//             out[j] = sum over i ascending of x[i] * hp[6 J - i], J = j + 11, from +0: one float32 multiply, then one float32 add.
//   deemph    bilinear([1], [75e-6, 1], fs) with the PRE-decimation fs (the reference's quirk), run by lfilter in float64 from z = 0.
//   mean      mono -= mono.mean(): np.add.reduce (pss_npsum.h) and a true division by n_out.
//   scale     *= 0.75, *= 32768, astype(int16).
// lfilter(b, a, x): direct form II transposed in float64 on coefficients divided by a[0].
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation; fmaf is the fused one.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "pss_npsum.h"

#if defined(__clang__)
#define PSS_MONO_UNROLL _Pragma("unroll")
#else
#define PSS_MONO_UNROLL
#endif

namespace pss_mono {

constexpr int Q = 6;              // decode_mono's decimation factor
constexpr int NTAPS = 121;        // decimate's FIR: 2 * 10 * Q + 1 taps
constexpr int PRE = 6;            // resample_poly's zero taps in front: Q - (NTAPS / 2) % Q
constexpr int NHP = NTAPS + PRE;  // 127: the padded filter
constexpr int DROP = 11;          // outputs of upfirdn dropped in front: (NTAPS / 2 + PRE) / Q
constexpr int MAX_COEF = 9;       // lfilter: at most 9 coefficients a side (butter of order 8)

PSS_NP_HD inline int out_len(int n) { return n <= 1 ? 0 : (n - 1 + Q - 1) / Q; }

// float32(fs / (2 pi pi 75e3)), in Python's order of operations
inline float gain_of(double fs) { return (float)(fs / (2.0 * M_PI * M_PI * 75e3)); }

// x[i] * conj(x[i + 1]) as NumPy's complex64 loop multiplies (a = x[i], b = conj(x[i + 1]))
PSS_NP_HD inline void disc_product(float ar, float ai, float xr, float xi, float &re, float &im)
{
    const float br = xr, bi = -xi;
    re = fmaf(ar, br, -(ai * bi));
    im = fmaf(ar, bi, ai * br);
}

// One decimated sample.  X(m), m = 0 .. 126: discriminator sample i = 6 (j + DROP) - 126 + m, +0 where i is outside 0 .. n_in - 1;
// hp: the 127 padded taps.  The terms run in upfirdn's order (i ascending, the tap index descending).  A sample outside the frame
// contributes x * h = +-0 to an accumulator that starts at +0 and can never become -0, which leaves every bit as it is: the loop needs no
// bounds.  The zero taps stay in: 0 * NaN is NaN, and a frame with a NaN must come out as the reference's does.
template <class FX>
PSS_NP_HD inline float fir_out(FX X, const float *hp)
{
    float acc = 0.0f;
    PSS_MONO_UNROLL
    for (int m = 0; m < NHP; m++) {
        const float t = X(m) * hp[NHP - 1 - m];
        acc = acc + t;
    }
    return acc;
}

// lfilter's step for two coefficients a side (b = [b0, b0] here, but nothing relies on it): y = z + b0 x; z = b1 x - a1 y
PSS_NP_HD inline double deemph_step(double b0, double b1, double a1, double x, double &z)
{
    const double y = z + b0 * x;
    z = b1 * x - a1 * y;
    return y;
}

// scipy.signal.lfilter's step (_linear_filter, direct form II transposed), NC = 2 .. MAX_COEF coefficients a side, already divided by a[0].
// NC is a template argument: the state stays in registers on the device.
template <int NC>
PSS_NP_HD inline double lfilter_step(const double *b, const double *a, double *z, double x)
{
    const double y = z[0] + b[0] * x;
    PSS_MONO_UNROLL
    for (int k = 0; k < NC - 2; k++) z[k] = (z[k + 1] + x * b[k + 1]) - y * a[k + 1];
    z[NC - 2] = x * b[NC - 1] - y * a[NC - 1];
    return y;
}

// mono.astype(np.int16) as this NumPy build converts float64: truncation toward zero to int32, then the low 16 bits (40000.5 -> -25536);
// NaN, +-inf and everything outside int32 give 0.  No step is undefined: the range is tested before the conversion.
PSS_NP_HD inline int16_t pcm_cast(double v)
{
    if (!(v > -2147483649.0 && v < 2147483648.0)) return 0;
    const uint32_t u = (uint32_t)(int32_t)v & 0xffffu;
    return (int16_t)(u >= 0x8000u ? (int32_t)u - 0x10000 : (int32_t)u);
}

// (y - mean) * 0.75 * 32768: the value the cast sees
PSS_NP_HD inline double scale_audio(double y, double mean) { return ((y - mean) * 0.75) * 32768.0; }

// mono.mean() of a row Y(i), i < n_out
template <class FY>
PSS_NP_HD inline double row_mean(FY Y, int n_out)
{
    return pss_np::np_sum<8, double>(Y, n_out) / (double)n_out;
}

struct Deemph { double b0, b1, a1; };

// One whole frame on one thread — the host twin and the stand-alone check.  x: n interleaved complex64 samples; angle(im, re): float32 arctan2;
// work: n - 1 floats.  pcm / audio / dec: n_out values each, any of them may be NULL.
template <class FA>
inline void frame(const float *x, int n, float gain, const float *hp, Deemph d, FA angle, float *work, int16_t *pcm, double *audio, float *dec,
                  double *ywork)
{
    const int n_in = n - 1, n_out = out_len(n);
    if (n_out == 0) return;
    for (int i = 0; i < n_in; i++) {
        float re, im;
        disc_product(x[2 * i], x[2 * i + 1], x[2 * i + 2], x[2 * i + 3], re, im);
        work[i] = gain * angle(im, re);
    }
    double z = 0.0;
    for (int j = 0; j < n_out; j++) {
        const int base = Q * (j + DROP) - (NHP - 1);
        const float v = fir_out([&](int m) { const int i = base + m; return i >= 0 && i < n_in ? work[i] : 0.0f; }, hp);
        if (dec) dec[j] = v;
        ywork[j] = deemph_step(d.b0, d.b1, d.a1, (double)v, z);
    }
    const double mean = row_mean([&](int i) { return ywork[i]; }, n_out);
    for (int j = 0; j < n_out; j++) {
        const double a = scale_audio(ywork[j], mean);
        if (audio) audio[j] = a;
        if (pcm) pcm[j] = pcm_cast(a);
    }
}

// lfilter divides both sides by a[0] first, whatever a[0] is
inline void lfilter_normalise(const double *b, const double *a, int nc, double *bn, double *an)
{
    for (int k = 0; k < nc; k++) { bn[k] = b[k] / a[0]; an[k] = a[k] / a[0]; }
}

// scipy.signal.lfilter(bn, an, x) on one row from a zero state
template <int NC>
PSS_NP_HD inline void lfilter_row(const double *x, int n, const double *bn, const double *an, double *y)
{
    double z[NC - 1];
    for (int k = 0; k < NC - 1; k++) z[k] = 0.0;
    for (int i = 0; i < n; i++) y[i] = lfilter_step<NC>(bn, an, z, x[i]);
}

// f(std::integral_constant<int, NC>{}) for the runtime coefficient count nc (2 .. MAX_COEF; the caller has checked it)
template <class F>
inline void with_ncoef(int nc, F f)
{
    switch (nc) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 9>{}); break;
    }
}

}  // namespace pss_mono

// pss_welch.h — the arithmetic of the capture survey (Welch's averaged periodogram and its max-hold row, scipy.signal.welch /
// spectrogram(mode='psd').max(-1) with return_onesided=False), stated ONCE for the kernels (pss_welch.hip: k_welch, k_welch_fold), the host
// twin (pss_h_welch) and the stand-alone host check (tests/welch_host.cpp).
//
//   input     n_rows rows of n complex64 samples, row_stride samples apart.
//   segments  length N = nperseg in {256, 512, 1024, 2048, 4096}, step S in [1, N] (SciPy's noverlap = N - S); segment s covers samples
//             [s S, s S + N); L = (n - N) / S + 1 by integer division (0 when n < N); no padding, no partial segment.
//   segment   all float64.  The samples widen exactly.  detrend: the segment's own mean is subtracted, summed in this order, with
//             T = N / 16 and W = min(T, 64), real and imaginary parts alike:
//               c[t] = ((0 + x[t]) + x[t + T]) + ... + x[t + 15 T]                               t < T
//               for off = W / 2, W / 4, ..., 1:  c[t] = c[t] + c[t xor off]   (all t at once)     -> c[64 w] is the sum of samples of wave w
//               sum = c[0] + c[64] + ... ascending over the T / W waves;  mean = sum * (1 / N)   (exact: N is a power of two)
//             then v[i] = (x[i] - mean) * win[i], X = DFT_N(v), p[k] = fma(re, re, im * im).
//   tree      the L segments of a row form consecutive blocks of BLOCK; a block's sum is 0 + p_s0 + p_s0+1 + ... ascending, its max
//             nan_max over the same (from -inf).  The nb = ceil(L / BLOCK) block partials form FOLD_Q consecutive chunks of
//             ceil(nb / FOLD_Q) (the last ones may be empty: sum 0, max -inf); a chunk's sum is 0 + its partials ascending, the row's sum
//             the chunk sums ascending from chunk 0's.  The tree depends on L alone: not on the grid, not on the batch.
//   outputs   FFT order.  mean[k] = (sum[k] / L) * scale, max[k] = max[k] * scale.
//   nan_max   pss_squelch.h's (np.max's step: a NaN wins), restated below: that header is device code and defines kernels, so neither the host
//             compiler nor a second unit can include it (tests/test_welch_golden.py holds the two statements together).
// The device takes its twiddles from pss_fft_tables and transforms with r16_core (pss_fft_r16.h); the host twin has the short radix-2
// transform below on a table built the same way.  The two transforms add in different orders, so device and host agree within the bound
// of tests/welch_bounds.py, not bit for bit; everything else above is the same sequence of operations on both sides.
// Every unit that includes this header is compiled with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PSS_WELCH_HD __host__ __device__
#else
#define PSS_WELCH_HD
#endif

namespace pss_wl {

constexpr int MIN_N = 256, MAX_N = 4096;   // the lengths r16_core<LOG_R3> transforms
constexpr int BLOCK = 32;                  // segments of a block
constexpr int FOLD_Q = 64;                 // chunks of block partials

PSS_WELCH_HD inline bool nperseg_ok(int N) { return N >= MIN_N && N <= MAX_N && (N & (N - 1)) == 0; }
PSS_WELCH_HD inline long segments(long n, int N, int S) { return n < N ? 0 : (n - N) / S + 1; }
PSS_WELCH_HD inline long n_blocks(long L) { return (L + BLOCK - 1) / BLOCK; }
PSS_WELCH_HD inline long chunk_len(long nb) { return (nb + FOLD_Q - 1) / FOLD_Q; }
PSS_WELCH_HD inline double power(double re, double im) { return fma(re, re, im * im); }
PSS_WELCH_HD inline double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }   // pss_squelch.h: nan_max

// The argument rules of pss_welch and pss_h_welch -> the reason of a refusal, or NULL
inline const char *check(const void *iq, long n_rows, long n, long row_stride, int nperseg, int step, const double *win, int detrend, double scale,
                         const double *mean)
{
    if (!nperseg_ok(nperseg)) return "nperseg not in {256, 512, 1024, 2048, 4096}";
    if (step < 1 || step > nperseg) return "step outside [1, nperseg]";
    if (n < nperseg) return "n < nperseg";
    if (n_rows < 1) return "n_rows < 1";
    if (row_stride < n) return "row_stride < n";
    if (n_rows > INT64_MAX / 16 / row_stride) return "n_rows times row_stride overflows";
    if (!win) return "null window";
    if (!mean) return "null mean";
    if (!iq) return "null iq";
    if (detrend != 0 && detrend != 1) return "detrend outside {0, 1}";
    if (!(scale > 0.0) || !std::isfinite(scale)) return "scale not finite and positive";
    return nullptr;
}

// periodic Hann, 0.5 - 0.5 cos(2 pi i / N), evaluated in the order of scipy.signal.get_window('hann', N) (general_cosine over
// linspace(-pi, pi, N + 1)[:N]): 0.5 + 0.5 cos(i (2 pi / N) - pi).  Written the first way it lies up to 2 units of 2^-53 from SciPy's table.
inline void default_window(int N, double *w)
{
    const double step = (2.0 * M_PI) / (double)N;
    for (int i = 0; i < N; i++) w[i] = 0.5 + 0.5 * std::cos((double)i * step + -M_PI);
}

// ---- the host twin -------------------------------------------------------------------------------------------------------------------
struct HostPlan {
    int N = 0, log2n = 0;
    std::vector<double> twr, twi;    // exp(-2 pi i k / N), k < N / 2, as pss_fft_tables builds it
    std::vector<int> rev;            // bit reversal
    std::vector<double> re, im, cr, ci, p;   // work: the segment, the mean's lanes, the segment's powers
    explicit HostPlan(int n) : N(n), twr(n / 2), twi(n / 2), rev(n), re(n), im(n), cr(n / 16), ci(n / 16), p(n)
    {
        while ((1 << log2n) < N) log2n++;
        for (int k = 0; k < N / 2; k++) {
            const double ang = -2.0 * M_PI * (double)k / (double)N;
            twr[k] = std::cos(ang), twi[k] = std::sin(ang);
        }
        twr[N / 4] = 0.0, twi[N / 4] = -1.0;
        for (int i = 0; i < N; i++) {
            int r = 0;
            for (int b = 0; b < log2n; b++) r |= ((i >> b) & 1) << (log2n - 1 - b);
            rev[i] = r;
        }
    }
};

// in place, decimation in time: N / 2 butterflies per level, each one complex product (4 multiplies, 2 adds) and two complex adds
inline void fft_radix2(HostPlan &P)
{
    const int N = P.N;
    for (int i = 0; i < N; i++) {
        const int r = P.rev[i];
        if (r > i) {
            const double a = P.re[i], b = P.im[i];
            P.re[i] = P.re[r], P.im[i] = P.im[r];
            P.re[r] = a, P.im[r] = b;
        }
    }
    for (int len = 2; len <= N; len <<= 1) {
        const int half = len / 2, stride = N / len;
        for (int base = 0; base < N; base += len)
            for (int j = 0; j < half; j++) {
                const double wr = P.twr[(size_t)j * stride], wi = P.twi[(size_t)j * stride];
                const double br = P.re[base + j + half], bi = P.im[base + j + half];
                const double tr = br * wr - bi * wi, ti = br * wi + bi * wr;
                const double ar = P.re[base + j], ai = P.im[base + j];
                P.re[base + j] = ar + tr, P.im[base + j] = ai + ti;
                P.re[base + j + half] = ar - tr, P.im[base + j + half] = ai - ti;
            }
    }
}

// the segment's mean in the stated order; x: N interleaved complex64 samples
inline void segment_mean(HostPlan &P, const float *x, double &mr, double &mi)
{
    const int N = P.N, T = N / 16, W = T < 64 ? T : 64;
    for (int t = 0; t < T; t++) {
        double sr = 0.0, si = 0.0;
        for (int n2 = 0; n2 < 16; n2++) sr += (double)x[2 * (t + T * n2)], si += (double)x[2 * (t + T * n2) + 1];
        P.cr[t] = sr, P.ci[t] = si;
    }
    for (int off = W / 2; off >= 1; off >>= 1)
        for (int t = 0; t < T; t++)
            if ((t & off) == 0) {   // both lanes of a pair take the same sum
                const double sr = P.cr[t] + P.cr[t ^ off], si = P.ci[t] + P.ci[t ^ off];
                P.cr[t] = P.cr[t ^ off] = sr, P.ci[t] = P.ci[t ^ off] = si;
            }
    double sr = P.cr[0], si = P.ci[0];
    for (int w = 1; w < T / W; w++) sr += P.cr[(size_t)W * w], si += P.ci[(size_t)W * w];
    mr = sr * (1.0 / (double)N), mi = si * (1.0 / (double)N);
}

// p[k] of one segment -> P.p
inline void segment_power(HostPlan &P, const float *x, const double *win, int detrend)
{
    const int N = P.N;
    double mr = 0.0, mi = 0.0;
    if (detrend) segment_mean(P, x, mr, mi);
    for (int i = 0; i < N; i++) {
        const double xr = (double)x[2 * i], xi = (double)x[2 * i + 1];
        P.re[i] = detrend ? (xr - mr) * win[i] : xr * win[i];
        P.im[i] = detrend ? (xi - mi) * win[i] : xi * win[i];
    }
    fft_radix2(P);
    for (int k = 0; k < N; k++) P.p[k] = power(P.re[k], P.im[k]);
}

// one row: the tree above, walked in order with one block, one chunk and one row accumulator.  max may be NULL.
inline void host_row(HostPlan &P, const float *x, long n, int S, const double *win, int detrend, double scale, double *mean, double *max)
{
    const int N = P.N;
    const long L = segments(n, N, S), nb = n_blocks(L), cl = chunk_len(nb);
    std::vector<double> bs(N), bm(N), cs(N), cm(N), rs(N), rm(N);
    for (long j = 0; j < nb; j++) {
        for (int k = 0; k < N; k++) bs[k] = 0.0, bm[k] = -INFINITY;
        const long s1 = (j + 1) * BLOCK < L ? (j + 1) * BLOCK : L;
        for (long s = j * BLOCK; s < s1; s++) {
            segment_power(P, x + 2 * s * S, win, detrend);
            for (int k = 0; k < N; k++) bs[k] += P.p[k], bm[k] = nan_max(bm[k], P.p[k]);
        }
        if (j % cl == 0)
            for (int k = 0; k < N; k++) cs[k] = 0.0, cm[k] = -INFINITY;
        for (int k = 0; k < N; k++) cs[k] += bs[k], cm[k] = nan_max(cm[k], bm[k]);
        if ((j + 1) % cl == 0 || j + 1 == nb) {
            const bool first = j / cl == 0;
            for (int k = 0; k < N; k++) rs[k] = first ? cs[k] : rs[k] + cs[k], rm[k] = first ? cm[k] : nan_max(rm[k], cm[k]);
        }
    }
    for (int k = 0; k < N; k++) {
        mean[k] = (rs[k] / (double)L) * scale;
        if (max) max[k] = rm[k] * scale;
    }
}

}  // namespace pss_wl

// pss_ddc.h — the arithmetic of the K-channel digital down-converter (mix by a numerically controlled oscillator, low-pass FIR, decimate),
// stated ONCE for the kernel (pss_ddc.hip: k_ddc), the host twins (pss_h_ddc, pss_h_ddc_rotor) and the stand-alone host check
// (tests/ddc_host.cpp).  The reference has no such arithmetic — its tuner chip retunes and resamples — so this statement is the project's own.
//
//   word      w = the integer nearest to (offset_hz / fs) 2^64 (ties to even), modulo 2^64; |offset_hz| <= fs / 2.
//   phase     of capture sample i (int64): p = (-w i) mod 2^64 in wrapping integers — exact, so no chunking of a capture changes a bit.
//   rotor     p' = p + 2^53, knot k = p' >> 54 (0 .. 1023), rem = (p' & (2^54 - 1)) - 2^53 (exact in float64), theta = rem C with
//             C = 2 pi 2^-64; sin(theta), cos(theta) by fixed polynomials in theta^2 (|theta| <= pi / 1024), Horner with fma;
//             c = fma(Ck, cos, -(Sk sin)), s = fma(Sk, cos, Ck sin).  (Ck, Sk): 1024 knots built from sin / cos on [0, pi / 4] only and
//             extended by octant symmetry (build_knots); host and device read the same bytes.
//   mix       zr = fma(xr, c, -(xi s)), zi = fma(xr, s, xi c) on the float32 parts widened exactly.
//   filter    y[m] = sum over k of h[k] z[m D + lead - k], z = 0 outside the capture.  Taps in blocks of B = 64: S_b a fma chain over
//             ascending k from +0 (block_sum), then y = (((S_0 + S_1) + S_2) + ...) in ascending b.  Real and imaginary part apart.
//   output    each part rounded once to float32.
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation; fma is the fused one.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PSS_DDC_HD __host__ __device__
#else
#define PSS_DDC_HD
#endif
#if defined(__clang__)
#define PSS_DDC_UNROLL _Pragma("unroll")
#else
#define PSS_DDC_UNROLL
#endif

namespace pss_dc {

constexpr int B = 64;               // taps of a block: the unit several lanes may share one output by
constexpr int KNOTS = 1024;         // rotor knots of a turn
constexpr int MAX_DECIM = 4096;
constexpr int MAX_TAPS = 4097;
constexpr int MAX_DEFAULT_DECIM = 204;   // firwin(20 D + 1, 1 / D) has at most MAX_TAPS taps up to here

// 2 pi 2^-64: float64(2 pi) scaled exactly
constexpr double C_THETA = 0x1.921fb54442d18p+2 * 0x1p-64;
// sin(t) = t + t t^2 (S3 + t^2 (S5 + t^2 S7)), cos(t) = 1 + t^2 (C2 + t^2 (C4 + t^2 C6)): the Taylor coefficients; at |t| <= pi / 1024 the
// first dropped terms are below 7e-29 and 2e-25
constexpr double S3 = -1.0 / 6.0, S5 = 1.0 / 120.0, S7 = -1.0 / 5040.0;
constexpr double C2 = -0.5, C4 = 1.0 / 24.0, C6 = -1.0 / 720.0;

// ceil(n / D) without an intermediate that can overflow
PSS_DDC_HD inline long out_len(long n, int D) { return n / D + (n % D != 0); }

// The frequency word of offset_hz at fs; the caller has checked fs > 0 and |offset_hz| <= fs / 2 (so |v| <= 2^63, exactly representable).
inline uint64_t word_of(double offset_hz, double fs)
{
    const double v = nearbyint((offset_hz / fs) * 0x1p64);   // the scaling is exact; ties to even in the default rounding mode
    return v < 0.0 ? (uint64_t)(int64_t)v : (uint64_t)v;
}

// w / 2^64 fs with w read as signed: the offset that results (+fs / 2 comes back as -fs / 2, the same oscillator)
inline double effective_hz(uint64_t w, double fs) { return ((double)(int64_t)w * 0x1p-64) * fs; }

// the phase of capture sample i
PSS_DDC_HD inline uint64_t phase_of(uint64_t w, int64_t i) { return (0 - w) * (uint64_t)i; }

// knots[2 k] = cos(2 pi k / 1024), knots[2 k + 1] = sin(2 pi k / 1024).  sin and cos are evaluated on [0, pi / 4] only; the other
// octants are reflections and sign changes, so that the quarter turns are exactly (1, 0), (0, 1), (-1, 0), (0, -1) (zeros +0).
inline void build_knots(double *knots)
{
    for (int k = 0; k < KNOTS; k++) {
        const int quad = k >> 8, r = k & 255;
        const int j = r <= 128 ? r : 256 - r;           // 0 .. 128: the angle pi j / 512 in [0, pi / 4]
        const double a = (double)j * (M_PI / 512.0);
        double c = cos(a), s = sin(a);
        if (j == 0) { c = 1.0; s = 0.0; }
        if (j == 128) c = s = M_SQRT1_2;                // one value for both at pi / 4: the table mirrors exactly about every axis and diagonal
        if (r > 128) { const double t = c; c = s; s = t; }
        double C, S;
        switch (quad) {
        case 0: C = c; S = s; break;
        case 1: C = -s; S = c; break;
        case 2: C = -c; S = -s; break;
        default: C = s; S = -c; break;
        }
        knots[2 * k] = C == 0.0 ? 0.0 : C;
        knots[2 * k + 1] = S == 0.0 ? 0.0 : S;
    }
}

// the rotor exp(i 2 pi p / 2^64) -> (c, s)
PSS_DDC_HD inline void rotor(uint64_t p, const double *knots, double &c, double &s)
{
    const uint64_t pp = p + (1ull << 53);
    const unsigned k = (unsigned)(pp >> 54);
    const int64_t rem = (int64_t)(pp & ((1ull << 54) - 1)) - ((int64_t)1 << 53);
    const double th = (double)rem * C_THETA;
    const double t2 = th * th;
    double ps = fma(t2, S7, S5);
    ps = fma(ps, t2, S3);
    const double sn = fma(th * t2, ps, th);
    double pc = fma(t2, C6, C4);
    pc = fma(pc, t2, C2);
    const double cs = fma(pc, t2, 1.0);
    const double Ck = knots[2 * k], Sk = knots[2 * k + 1];
    c = fma(Ck, cs, -(Sk * sn));
    s = fma(Sk, cs, Ck * sn);
}

// x (float32 parts) times the rotor
PSS_DDC_HD inline void mix(float xr32, float xi32, double c, double s, double &zr, double &zi)
{
    const double xr = (double)xr32, xi = (double)xi32;
    zr = fma(xr, c, -(xi * s));
    zi = fma(xr, s, xi * c);
}

// One block sum of both parts: taps H(kk), kk < nk, of the block (nk <= B) against Z(kk, zr, zi), called once per kk in ascending order — the
// caller's Z hands out z[m D + lead - (k0 + kk)].  A fma chain from +0.  The samples of CHUNK steps are fetched before their fma steps run
// (on the device: the LDS reads and the tap loads of a chunk are in flight together); the chain itself is the plain ascending one.
constexpr int CHUNK = 8;
template <class FH, class FZ>
PSS_DDC_HD inline void block_sum(FH H, int nk, FZ Z, double &sr, double &si)
{
    double ar = 0.0, ai = 0.0;
    int kk = 0;
    for (; kk + CHUNK <= nk; kk += CHUNK) {
        double zr[CHUNK], zi[CHUNK];
        PSS_DDC_UNROLL
        for (int u = 0; u < CHUNK; u++) Z(kk + u, zr[u], zi[u]);
        PSS_DDC_UNROLL
        for (int u = 0; u < CHUNK; u++) {
            const double h = H(kk + u);
            ar = fma(h, zr[u], ar);
            ai = fma(h, zi[u], ai);
        }
    }
    for (; kk < nk; kk++) {
        double zr, zi;
        Z(kk, zr, zi);
        const double h = H(kk);
        ar = fma(h, zr, ar);
        ai = fma(h, zi, ai);
    }
    sr = ar;
    si = ai;
}

// y = (((S_0 + S_1) + S_2) + ...): S(b, sr, si) hands out the block sums in ascending b; one rounding to float32 per part
template <class FS>
PSS_DDC_HD inline void combine(int n_blocks, FS S, float &yr, float &yi)
{
    double ar, ai;
    S(0, ar, ai);
    for (int b = 1; b < n_blocks; b++) {
        double sr, si;
        S(b, sr, si);
        ar = ar + sr;
        ai = ai + si;
    }
    yr = (float)ar;
    yi = (float)ai;
}

PSS_DDC_HD inline int n_blocks(int T) { return (T + B - 1) / B; }

// One output on one thread: Z(j, zr, zi) hands out the mixed sample of capture index j (zero outside the capture), j = m D + lead - k.
template <class FZ>
inline void output(long m, int D, const double *h, int T, int lead, FZ Z, float &yr, float &yi)
{
    const long j0 = m * D + lead;
    combine(n_blocks(T), [&](int b, double &sr, double &si) {
        const int k0 = b * B, nk = T - k0 < B ? T - k0 : B;
        block_sum([&](int kk) { return h[k0 + kk]; }, nk, [&](int kk, double &zr, double &zi) { Z(j0 - (k0 + kk), zr, zi); }, sr, si);
    }, yr, yi);
}

// ---- the kernel's tile, as a function of the launch's D and T (host code; tests/test_gpu_ddc.py restates it) ----------------------------------
constexpr int STAGE_CAP = 8192;     // mixed samples (float64 pairs) of the staging buffer
constexpr int PART_CAP = 1792;      // (output, block) sums of a tile

// doubles of one phase row for a tile of M outputs: M - 1 + ceil(T / D) columns, made odd (the staging stores of neighbouring lanes land
// an odd number of float64 slots apart)
inline int tile_row(int M, int D, int T) { return (M - 1 + (T + D - 1) / D) | 1; }

// Outputs of a tile: the most whose staged span fits STAGE_CAP in the phase-major layout and whose block sums fit PART_CAP.  One output
// needs no phases (its T samples are stored in a row), and T <= MAX_TAPS <= STAGE_CAP: at least 1.
inline int tile_outputs(int D, int T)
{
    int M = PART_CAP / n_blocks(T);
    while (M > 1 && (long)D * tile_row(M, D, T) > STAGE_CAP) M--;
    return M;
}

}  // namespace pss_dc

// pss_bank.h — the arithmetic of the channeliser for band plans: every channel of a uniform grid of M = 2^a 3^b 5^c channels (25 kHz,
// 12.5 kHz and 10 kHz grids at 2.4 and 10 MS/s are all of that form; none is a power of two), fs / M apart, at fs / D.  Stated ONCE for
// the kernel (pss_bank.hip: k_bank), the host twin (pss_h_bank) and the stand-alone host check (tests/bank_host.cpp).  The bank's first
// half is pss_pfb.h's, unchanged; only the DFT and the first tap (a true modulo) are new.  A power-of-two M never reaches this header:
// pss_bank / pss_h_bank / pss_bank_default_taps hand it to pss_pfb's code path, so its bytes are pss_pfb's by construction.
//
//   definition  output m of channel c is y_c[m] = sum over k of h[k] x[j] exp(-2 pi i c j / M), j = m D + lead - k, x = 0 outside
//               [0, n_capture).  j is the sample's index in the CAPTURE, so no chunking of a capture changes a bit.  Row c sits at c fs / M
//               for c <= (M - 1) / 2 and at (c - M) fs / M otherwise (even M: row M / 2 reads -fs / 2).
//   branch sums pss_pf::branch_sums, the same chains: branch rho owns the taps k = k_rho + p M, k_rho = (j0 - rho) mod M — the
//               non-negative remainder of a 64-bit integer (first_tap: a true modulo, not a mask), j0 = m D + lead.
//   DFT         Y_c = sum over rho of u_rho W_M^(c rho), W_N = exp(-2 pi i / N), in float64 by mixed-radix decimation in time.  The
//               factor order is fixed: stage 0, 1, ... are ALL THE 5s, THEN ALL THE 3s, THEN ALL THE 2s (stage_radix).  u_rho goes in at the
//               mixed-radix digit reversal of rho (digit_reverse).  Stage s joins sub-transforms of length N' into N = r N': the butterfly
//               at t < N' of block b takes the operands a_q at b N + q N' + t, q = 0 .. r - 1, multiplies a_q, q >= 1, by W_N^(t q) —
//               (C, S) = entry t q M / N of the table, pr = fma(br, C, bi * S), pi = fma(bi, C, -(br * S)) (twiddle) — and runs one fixed
//               r-point kernel (kernel2: pss_pf::butterfly's sum and difference; kernel3, kernel5: below, every operation written out);
//               result p goes to b N + p N' + t.
//   table       M entries, entry t = (cos, sin)(2 pi t / M), built on the host (build_twiddles) and uploaded, so host and device read the
//               same bytes.  The rule: quadrant q4 = floor(4 t / M) and r4 = 4 t - q4 M in integers; j = r4 if 2 r4 <= M, else M - r4
//               with cos and sin swapped: the angle pi j / (2 M) lies in [0, pi / 4]; libm cos / sin of ((double)j * M_PI) / (double)(2 M)
//               there; exactly (1, 0) at j = 0 and M_SQRT1_2 for both at 2 j = M; the quadrant's signs as pss_dc::build_knots; zeros +0.
//   output      each part rounded once to float32.  The sign of a zero is not part of the contract.
//   bound       |float64(y32) - truth| <= 1/2 ulp_float32 + units 2^-53 sum|h| max(|xr|, |xi|), units = ceil(T / M) + sum over stages of
//               u(r) + 8 (f64_units), u(r) the roundings on the longest input-to-output path of one stage, a table entry's or a
//               constant's rounding counted as one:
//                 u(2) = 4  the table entry, bi * S, the fma, the sum
//                 u(3) = 7  the twiddle's 3 as above; t = a1 + a2; m = fma(-0.5, t, a0) (0.5 is exact); the constant S3; fma(S3, d, m)
//                 u(5) = 9  the twiddle's 3; t1 = a1 + a4; fma(C1, t1, a0) and its constant; fma(C2, t2, .) and its constant; m -+ n
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation; fma is the fused one.
#pragma once
#include <cmath>
#include <cstdint>

#include "pss_pfb.h"

namespace pss_bk {

constexpr int MAX_CHAN = 1024;
constexpr int MAX_STAGES = 10;      // 2^10 = 1024: no 5-smooth M <= 1024 has more prime factors

// the constants of the 3- and 5-point kernels, correctly rounded
constexpr double K3_S = 0x1.bb67ae8584caap-1;     // sin(2 pi / 3) = sqrt(3) / 2
constexpr double K5_C1 = 0x1.3c6ef372fe950p-2;    // cos(2 pi / 5) = (sqrt(5) - 1) / 4
constexpr double K5_C2 = -0x1.9e3779b97f4a8p-1;   // cos(4 pi / 5) = -(sqrt(5) + 1) / 4
constexpr double K5_S1 = 0x1.e6f0e134454ffp-1;    // sin(2 pi / 5)
constexpr double K5_S2 = 0x1.2cf2304755a5ep-1;    // sin(4 pi / 5)

// M = 2^n2 3^n3 5^n5 -> the exponents; false where another prime is left
PSS_DDC_HD inline bool factor(int M, int &n2, int &n3, int &n5)
{
    n2 = n3 = n5 = 0;
    if (M < 1) return false;
    while (M % 5 == 0) { M /= 5; n5++; }
    while (M % 3 == 0) { M /= 3; n3++; }
    while (M % 2 == 0) { M /= 2; n2++; }
    return M == 1;
}

PSS_DDC_HD inline bool bank_ok(int M)
{
    int n2, n3, n5;
    return M >= 2 && M <= MAX_CHAN && factor(M, n2, n3, n5);
}

PSS_DDC_HD inline bool pow2(int M) { return (M & (M - 1)) == 0; }

// the radix of stage s: all the 5s, then all the 3s, then all the 2s
PSS_DDC_HD inline int stage_radix(int s, int n3, int n5) { return s < n5 ? 5 : s < n5 + n3 ? 3 : 2; }

// the first tap of branch rho at an output whose own sample is j0: (j0 - rho) mod M, non-negative
PSS_DDC_HD inline int first_tap(int64_t j0, int rho, int M)
{
    const int64_t v = (j0 - (int64_t)rho) % (int64_t)M;
    return (int)(v < 0 ? v + M : v);
}

// position of u_rho in the DFT's input.  The LAST stage splits the index by its radix first: its digit (rho mod r) carries the largest
// weight M / r, and so on down to stage 0 — the 2s take their digits first, then the 3s, then the 5s.
PSS_DDC_HD inline int digit_reverse(int rho, int M, int n2, int n3, int n5)
{
    int pos = 0, w = M;
    for (int i = 0; i < n2; i++) { w /= 2; pos += (rho % 2) * w; rho /= 2; }
    for (int i = 0; i < n3; i++) { w /= 3; pos += (rho % 3) * w; rho /= 3; }
    for (int i = 0; i < n5; i++) { w /= 5; pos += (rho % 5) * w; rho /= 5; }
    return pos;
}

// tw[2 t] = cos(2 pi t / M), tw[2 t + 1] = sin(2 pi t / M), t = 0 .. M - 1, by the rule in the head of this file.  Host code.
inline void build_twiddles(int M, double *tw)
{
    for (int t = 0; t < M; t++) {
        const int quad = 4 * t / M, r4 = 4 * t - quad * M;      // the angle inside the quadrant: 2 pi r4 / (4 M), 0 <= r4 < M
        const bool mirror = 2 * r4 > M;
        const int j = mirror ? M - r4 : r4;                     // 0 <= 2 j <= M: the angle pi j / (2 M) in [0, pi / 4]
        const double a = ((double)j * M_PI) / (double)(2 * M);
        double c = cos(a), s = sin(a);
        if (j == 0) { c = 1.0; s = 0.0; }
        if (2 * j == M) c = s = M_SQRT1_2;                      // one value for both at pi / 4: the table mirrors exactly about every diagonal
        if (mirror) { const double x = c; c = s; s = x; }
        double C, S;
        switch (quad) {
        case 0: C = c; S = s; break;
        case 1: C = -s; S = c; break;
        case 2: C = -c; S = -s; break;
        default: C = s; S = -c; break;
        }
        tw[2 * t] = C == 0.0 ? 0.0 : C;
        tw[2 * t + 1] = S == 0.0 ? 0.0 : S;
    }
}

// b times W = C - i S, in the form pss_pf::butterfly uses
PSS_DDC_HD inline void twiddle(double &br, double &bi, double C, double S)
{
    const double pr = fma(br, C, bi * S);
    const double pi = fma(bi, C, -(br * S));
    br = pr;
    bi = pi;
}

// The 3-point DFT in place, W_3 = -1/2 - i S3: X0 = a0 + (a1 + a2); X1, X2 = (a0 - (a1 + a2) / 2) -+ i S3 (a1 - a2).
PSS_DDC_HD inline void kernel3(double (&xr)[3], double (&xi)[3])
{
    const double tr = xr[1] + xr[2], ti = xi[1] + xi[2];
    const double dr = xr[1] - xr[2], di = xi[1] - xi[2];
    const double mr = fma(-0.5, tr, xr[0]), mi = fma(-0.5, ti, xi[0]);
    xr[0] = xr[0] + tr;
    xi[0] = xi[0] + ti;
    xr[1] = fma(K3_S, di, mr);        // m - i S3 d
    xi[1] = fma(-K3_S, dr, mi);
    xr[2] = fma(-K3_S, di, mr);       // m + i S3 d
    xi[2] = fma(K3_S, dr, mi);
}

// The 5-point DFT in place, W_5^q = cos(2 pi q / 5) - i sin(2 pi q / 5): with t1 = a1 + a4, t2 = a2 + a3, d1 = a1 - a4, d2 = a2 - a3,
// X0 = a0 + (t1 + t2); X1, X4 = m1 -+ i n1, m1 = a0 + C1 t1 + C2 t2, n1 = S1 d1 + S2 d2; X2, X3 = m2 -+ i n2, m2 = a0 + C2 t1 + C1 t2,
// n2 = S2 d1 - S1 d2.
PSS_DDC_HD inline void kernel5(double (&xr)[5], double (&xi)[5])
{
    const double t1r = xr[1] + xr[4], t1i = xi[1] + xi[4], t2r = xr[2] + xr[3], t2i = xi[2] + xi[3];
    const double d1r = xr[1] - xr[4], d1i = xi[1] - xi[4], d2r = xr[2] - xr[3], d2i = xi[2] - xi[3];
    const double m1r = fma(K5_C2, t2r, fma(K5_C1, t1r, xr[0])), m1i = fma(K5_C2, t2i, fma(K5_C1, t1i, xi[0]));
    const double m2r = fma(K5_C1, t2r, fma(K5_C2, t1r, xr[0])), m2i = fma(K5_C1, t2i, fma(K5_C2, t1i, xi[0]));
    const double n1r = fma(K5_S2, d2r, K5_S1 * d1r), n1i = fma(K5_S2, d2i, K5_S1 * d1i);
    const double n2r = fma(-K5_S1, d2r, K5_S2 * d1r), n2i = fma(-K5_S1, d2i, K5_S2 * d1i);
    xr[0] = xr[0] + (t1r + t2r);
    xi[0] = xi[0] + (t1i + t2i);
    xr[1] = m1r + n1i;                // m - i n
    xi[1] = m1i - n1r;
    xr[4] = m1r - n1i;                // m + i n
    xi[4] = m1i + n1r;
    xr[2] = m2r + n2i;
    xi[2] = m2i - n2r;
    xr[3] = m2r - n2i;
    xi[3] = m2i + n2r;
}

// One butterfly of a stage of radix r in place: the operands at a, a + Np, ..., a + (r - 1) Np (a = b N + t); u = t M / N, so operand q
// takes table entry q u.
template <int R>
PSS_DDC_HD inline void fly_r(double *vr, double *vi, int a, int Np, int u, const double *tw)
{
    double xr[R], xi[R];
    PSS_DDC_UNROLL
    for (int q = 0; q < R; q++) {
        xr[q] = vr[a + q * Np];
        xi[q] = vi[a + q * Np];
    }
    PSS_DDC_UNROLL
    for (int q = 1; q < R; q++) twiddle(xr[q], xi[q], tw[2 * (q * u)], tw[2 * (q * u) + 1]);
    if constexpr (R == 3) kernel3(xr, xi);
    if constexpr (R == 5) kernel5(xr, xi);
    PSS_DDC_UNROLL
    for (int q = 0; q < R; q++) {
        vr[a + q * Np] = xr[q];
        vi[a + q * Np] = xi[q];
    }
}

PSS_DDC_HD inline void fly(int r, double *vr, double *vi, int a, int Np, int u, const double *tw)
{
    if (r == 5) fly_r<5>(vr, vi, a, Np, u, tw);
    else if (r == 3) fly_r<3>(vr, vi, a, Np, u, tw);
    else pss_pf::butterfly(vr[a], vi[a], vr[a + Np], vi[a + Np], tw[2 * u], tw[2 * u + 1]);   // radix 2, as pss_pfb.h has it
}

// The DFT of one output instant in place on one thread: vr / vi hold u in digit-reversed order on entry, Y_c at c on return.
inline void dft(int M, double *vr, double *vi, const double *tw)
{
    int n2, n3, n5;
    factor(M, n2, n3, n5);
    int Np = 1;
    for (int s = 0; s < n2 + n3 + n5; s++) {
        const int r = stage_radix(s, n3, n5), N = r * Np, step = M / N;
        for (int i = 0; i < M / r; i++) {
            const int b = i / Np, t = i % Np;
            fly(r, vr, vi, b * N + t, Np, t * step, tw);
        }
        Np = N;
    }
}

// One output instant on one thread: X(j, xr, xi) hands out capture sample j (zeros outside the capture); y: M complex64 values, channel c
// at y[2 c]; vr / vi: room for M doubles each; rev: digit_reverse of 0 .. M - 1.
template <class FX>
inline void instant(long m, int M, int D, const double *h, int T, int lead, const double *tw, const int *rev, FX X, double *vr, double *vi, float *y)
{
    const int64_t j0 = (int64_t)m * D + lead;
    for (int rho = 0; rho < M; rho++) {
        double ur[1], ui[1];
        pss_pf::branch_sums<1>(first_tap(j0, rho, M), M, T, [&](int k) { return h[k]; }, [&](int, int k, float &xr, float &xi) { X(j0 - k, xr, xi); }, ur, ui);
        vr[rev[rho]] = ur[0];
        vi[rev[rho]] = ui[0];
    }
    dft(M, vr, vi, tw);
    for (int c = 0; c < M; c++) {
        y[2 * c] = (float)vr[c];
        y[2 * c + 1] = (float)vi[c];
    }
}

// the float64 term of the output bound in units of 2^-53 sum|h| max(|xr|, |xi|) (the head of this file)
inline int f64_units(int M, int T)
{
    int n2, n3, n5;
    factor(M, n2, n3, n5);
    return (T + M - 1) / M + 4 * n2 + 7 * n3 + 9 * n5 + 8;
}

// ---- the kernel's tile (host code; tests/test_gpu_bank.py restates it) -------------------------------------------------------------------
// A workgroup of BANK_T threads uses W = M G of them, G = BANK_T / M (rounded down): thread tid < W has first tap tid mod M and instant
// tid / M; its ITEMS items lie G instants apart and share the first tap.  A tile holds R = ITEMS G instants, R M <= 8192 elements.
constexpr int BANK_T = 1024;
constexpr int ITEMS = 8;
PSS_DDC_HD inline int tile_group(int M) { return BANK_T / M; }
PSS_DDC_HD inline int tile_instants(int M) { return ITEMS * tile_group(M); }
// rows lie an ODD number of float64 slots apart in LDS: a column (one channel of every instant, what the transposed store reads) then
// falls on distinct banks
PSS_DDC_HD inline int tile_row(int M) { return M | 1; }
// float64 slots of each part of the tile: the largest R (M | 1) over the M the kernel runs (no power of two) is M = 6's, 1360 rows of 7
constexpr int TILE_SLOTS = 9520;

}  // namespace pss_bk

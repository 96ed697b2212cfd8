// pss_pfb.h — the arithmetic of the polyphase channeliser (every channel of a uniform grid of M channels, fs / M apart, at fs / D), stated
// ONCE for the kernel (pss_pfb.hip: k_pfb), the host twin (pss_h_pfb) and the stand-alone host check (tests/pfb_host.cpp).  The reference
// has a tuner chip instead, so this statement is the project's own.
//
//   definition  channel c sits at c fs / M for c < M / 2 and at (c - M) fs / M otherwise.  Output m of channel c is
//               y_c[m] = sum over k of h[k] x[j] exp(-2 pi i c j / M), j = m D + lead - k, x = 0 outside [0, n_capture): what pss_ddc
//               computes for the word c 2^64 / M.  j is the sample's index in the CAPTURE, so no chunking of a capture changes a bit.
//   branch sums j0 = m D + lead.  Branch rho in [0, M) owns the taps k = k_rho + p M, k_rho = (j0 - rho) mod M (the non-negative remainder
//               of a 64-bit integer), p = 0, 1, ... while k < T — the samples j = j0 - k with j mod M = rho.  u_rho is ONE fma chain from +0
//               over ascending p in each part: ur = fma(h[k], (double)xr[j], ur), ui alike (branch_sums).  A sample outside the capture is 0.
//   DFT         Y_c = sum over rho of u_rho W^(c rho), W = exp(-2 pi i / M), in float64 by radix-2 decimation in time: u_rho is loaded at
//               position bitrev(rho); log2 M stages of half-length hl = 1, 2, ..., M / 2; butterfly (a, b = a + hl), t = a mod hl, takes
//               (C, S) = knot t 1024 / (2 hl) of pss_dc::build_knots (cos and sin of 2 pi t / (2 hl): the same 1024-entry table, the same
//               bytes on host and device); pr = fma(br, C, bi * S), pi = fma(bi, C, -(br * S)), a' = a + p, b' = a - p (butterfly).
//   output      each part rounded once to float32.  The sign of a zero is not part of the contract.
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation; fma is the fused one.
#pragma once
#include <cstdint>

#include "pss_ddc.h"

namespace pss_pf {

constexpr int MAX_CHAN = 1024;      // = pss_dc::KNOTS: the twiddles of the last stage are the knots of the table's first half turn
constexpr int TAPS_PER_CHAN = 32;   // n_taps <= 32 n_chan: at most 32 steps in a branch's chain
constexpr int DEFAULT_TAPS_PER_CHAN = 20;   // firwin(20 M + 1, 1 / M)

PSS_DDC_HD inline bool chan_ok(int M) { return M >= 2 && M <= MAX_CHAN && (M & (M - 1)) == 0; }

PSS_DDC_HD inline int log2_of(int M)
{
    int l = 0;
    while ((1 << l) < M) l++;
    return l;
}

// the first tap of branch rho at an output whose own sample is j0: (j0 - rho) mod M, non-negative (M a power of two; j0 - rho may be
// negative, two's complement keeps the remainder)
PSS_DDC_HD inline int first_tap(int64_t j0, int rho, int M) { return (int)((uint64_t)(j0 - rho) & (uint64_t)(M - 1)); }

// position of u_rho in the DFT's input: the lb low bits of rho reversed
PSS_DDC_HD inline int bitrev(int rho, int lb)
{
    int r = 0;
    for (int b = 0; b < lb; b++) r |= ((rho >> b) & 1) << (lb - 1 - b);
    return r;
}

// N branch sums that share their taps — the branches of N output instants whose first tap is the same k0: taps H(k) for k = k0, k0 + M,
// ... < T against X(i, k, xr, xi), which hands out the float32 parts of chain i's sample x[j0_i - k] (zeros outside the capture), called
// once per (i, k), k ascending.  One fma chain from +0 in each part of each chain.  Every branch has T / M taps or one more (k0 < M), so
// the loop's trip count is the same for every branch — on the device a step's tap and N samples are in flight together and no lane leaves
// the loop early — and the odd tap follows; each chain is the plain ascending one.  The host twin runs N = 1.
template <int N, class FH, class FX>
PSS_DDC_HD inline void branch_sums(int k0, int M, int T, FH H, FX X, double (&ur)[N], double (&ui)[N])
{
    PSS_DDC_UNROLL
    for (int i = 0; i < N; i++) ur[i] = ui[i] = 0.0;
    auto step = [&](int k) {
        const double h = H(k);
        float xr[N], xi[N];
        PSS_DDC_UNROLL
        for (int i = 0; i < N; i++) X(i, k, xr[i], xi[i]);
        PSS_DDC_UNROLL
        for (int i = 0; i < N; i++) {
            ur[i] = fma(h, (double)xr[i], ur[i]);
            ui[i] = fma(h, (double)xi[i], ui[i]);
        }
    };
    const int n_full = T / M;
    int k = k0;
    for (int p = 0; p < n_full; p++, k += M) step(k);
    if (k < T) step(k);
}

// butterfly i (0 <= i < M / 2) of the stage of half-length hl = 1 << ls: its upper element a (the lower is a + hl) and its knot
PSS_DDC_HD inline int fly_a(int i, int ls) { return ((i >> ls) << (ls + 1)) | (i & ((1 << ls) - 1)); }
PSS_DDC_HD inline int fly_knot(int i, int ls) { return (i & ((1 << ls) - 1)) << (9 - ls); }   // t 1024 / (2 hl) = t 512 / hl

PSS_DDC_HD inline void butterfly(double &ar, double &ai, double &br, double &bi, double C, double S)
{
    const double pr = fma(br, C, bi * S);
    const double pi = fma(bi, C, -(br * S));
    br = ar - pr;
    bi = ai - pi;
    ar = ar + pr;
    ai = ai + pi;
}

// The DFT of one output instant in place on one thread: vr / vi hold u in bit-reversed order on entry, Y_c at c on return.
inline void dft(int M, double *vr, double *vi, const double *knots)
{
    const int lb = log2_of(M);
    for (int ls = 0; ls < lb; ls++)
        for (int i = 0; i < M / 2; i++) {
            const int a = fly_a(i, ls), b = a + (1 << ls), kn = fly_knot(i, ls);
            butterfly(vr[a], vi[a], vr[b], vi[b], knots[2 * kn], knots[2 * kn + 1]);
        }
}

// One output instant on one thread: X(j, xr, xi) hands out capture sample j (zeros outside the capture); y: M complex64 values, channel c
// at y[2 c]; vr / vi: room for M doubles each.
template <class FX>
inline void instant(long m, int M, int D, const double *h, int T, int lead, const double *knots, FX X, double *vr, double *vi, float *y)
{
    const int64_t j0 = (int64_t)m * D + lead;
    const int lb = log2_of(M);
    for (int rho = 0; rho < M; rho++) {
        const int q = bitrev(rho, lb);
        double ur[1], ui[1];
        branch_sums<1>(first_tap(j0, rho, M), M, T, [&](int k) { return h[k]; }, [&](int, int k, float &xr, float &xi) { X(j0 - k, xr, xi); }, ur, ui);
        vr[q] = ur[0];
        vi[q] = ui[0];
    }
    dft(M, vr, vi, knots);
    for (int c = 0; c < M; c++) {
        y[2 * c] = (float)vr[c];
        y[2 * c + 1] = (float)vi[c];
    }
}

// ---- the kernel's tile (host code; tests/test_gpu_pfb.py restates it) --------------------------------------------------------------------
constexpr int TILE_LOG2 = 13;
constexpr int TILE_ELEMS = 8192;    // = 1 << TILE_LOG2: (instant, branch) pairs of a tile: R = TILE_ELEMS / M consecutive output instants, at least 8
constexpr int PAD_FROM = 32;        // from M = 32 on a tile's rows lie M + 1 float64 slots apart in LDS: a column (one channel of every
                                    // instant, what the transposed store reads) then falls on distinct banks
constexpr int TILE_SLOTS = TILE_ELEMS + TILE_ELEMS / PAD_FROM;

PSS_DDC_HD inline int tile_instants(int M) { return TILE_ELEMS / M; }
PSS_DDC_HD inline int tile_row(int M) { return M >= PAD_FROM ? M + 1 : M; }

}  // namespace pss_pf

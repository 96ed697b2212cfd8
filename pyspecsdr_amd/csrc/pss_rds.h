// pss_rds.h — the arithmetic of the RDS receiver (the hooks extract_rds / demodulate_rds_bpsk that the reference's demodulate_wfm calls and
// never defines, signal_processing.py:165-174), stated ONCE for the kernels (pss_rds.hip: k_rds_front, k_rds_bits, k_rds_groups), the host
// twins (pss_h_rds_front, pss_h_rds_bits, pss_h_rds_groups) and the stand-alone host check (tests/rds_host.cpp).  The reference has no such
// arithmetic, so this statement is the project's own.  Every output follows from indices in the ROW, never from how the row was cut.
//
//   front   d[i] = float32 angle of the float32 product x[i] conj(x[i - 1]) (pss_mono.h's disc_product; the caller's model of NumPy's
//           arctan2), d[0] = 0, no gain.  z[i] = d[i] times the rotor of pss_ddc.h at word_of(57000, fs) and index i of the row: one float64
//           multiply per part.  y[m] = pss_ddc.h's output(m, D, h, T, lead, z): float64 fma chains in blocks of 64 taps, zero outside the
//           row, each part rounded once to float32.
//   pulse   the standard's biphase symbol at 16 samples a bit: p[u] = g(k + 4) - g(k - 4), k = u - c, c = 8 S, u = 0 .. 16 S, with
//           g(q) = cos(pi q / 4) / (1 - q^2 / 4) — the impulse response of H(f) = cos(pi f t_d / 4), |f| <= 2 / t_d, at t = q t_d / 16,
//           scaled to g(0) = 1; g(+-2) = pi / 4 (the limit).  cos(pi q / 4) comes from a table of eight exact entries: no libm call.
//   filter  y[j] = sum over u ascending of p[u] b[j + u - c], b = 0 outside the row: a float64 fma chain from +0 per part.
//   timing  segment s = samples [1024 s, 1024 s + 1024) cut to the row.  E[s][o] = sum over the segment's j = o (mod 16), ascending, of
//           fma(yr, yr, yi yi), from +0.  F[s][o] = the E of segments max(0, s - 4) .. min(S - 1, s + 4) added in ascending order from +0.
//           o_s: best = 0; for o = 1 .. 15: if F[s][o] > F[s][best] then best = o — a NaN is never greater and nothing is greater than a
//           NaN in slot 0.
//   strobe  the regular strobes of segment s are j = 1024 s + o_s + 16 k inside the segment and the row.  With L = 1024 s - 16 + o_(s-1)
//           the last strobe of the segment before and J the first regular one (s >= 1, J exists): J - L < 8 drops J; J - L > 24 inserts
//           one strobe at L + 16.  (J - L = 16 + o_s - o_(s-1) lies in 1 .. 31, so one step always settles it.)
//   bit     for consecutive strobes t', t: v = fma(yr[t'], yr[t], yi[t'] yi[t]); the data bit is 1 where v < 0.  n_bits = strobes - 1.
//   block   26 bits, first bit the most significant: 16 information bits and 10 check bits.  The checkword of the information word is
//           the remainder of m(x) x^10 by x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1; a block is valid as X when checkword XOR offset(X)
//           equals its check bits.  A group sits at bit i when the blocks at i, i + 26, i + 52, i + 78 are valid as A, B, C or C', D, the
//           third as C' exactly when bit 11 (B0) of the second information word is 1.
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation; fma is the fused one.
#pragma once
#include <cmath>
#include <cstdint>

#include "pss_ddc.h"
#include "pss_mono.h"

namespace pss_rds {

constexpr double SUBCARRIER_HZ = 57000.0;
constexpr long BASE_RATE = 19000;       // 16 samples a bit: 1187.5 bit/s = 57000 / 48
constexpr int SPB = 16;                 // samples per bit at BASE_RATE
constexpr int SEG_BITS = 64, SEG = SEG_BITS * SPB;   // a timing segment: 1024 samples
constexpr int SMOOTH = 4;               // segments either side whose energies are added
constexpr int MAX_SPAN = 16;            // bit periods of a pulse table: at most 16 MAX_SPAN + 1 = 257 taps
constexpr int MAX_PULSE = SPB * MAX_SPAN + 1;
constexpr long MAX_ROW = 1l << 30;      // samples of a baseband row (15 hours)
constexpr int BLOCK = 26, GROUP = 4 * BLOCK;
constexpr uint32_t POLY = 0x5B9;        // x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
constexpr uint32_t OFF_A = 0x0FC, OFF_B = 0x198, OFF_C = 0x168, OFF_CP = 0x350, OFF_D = 0x1B4;

// ---- front --------------------------------------------------------------------------------------------------------------------------------
// the discriminator sample of row index i >= 1: angle(im, re) of x[i] conj(x[i - 1])
template <class FA>
PSS_DDC_HD inline float disc(float cr, float ci, float pr, float pi, FA angle)
{
    float re, im;
    pss_mono::disc_product(cr, ci, pr, pi, re, im);
    return angle(im, re);
}

// d times the rotor at phase p
PSS_DDC_HD inline void mixed(float d, uint64_t p, const double *knots, double &zr, double &zi)
{
    double c, s;
    pss_dc::rotor(p, knots, c, s);
    zr = (double)d * c;
    zi = (double)d * s;
}

// D, up, down of a capture at fs Hz (the caller has checked that fs is an integer above 120 000): false where the reduced ratio leaves
// [1, 4096]
inline bool plan(long fs, int &D, int &up, int &down)
{
    long d = fs / BASE_RATE;
    if (d > pss_dc::MAX_DEFAULT_DECIM) d = pss_dc::MAX_DEFAULT_DECIM;
    long a = BASE_RATE * d, b = fs;
    long x = a, y = b;
    while (y) { const long t = x % y; x = y; y = t; }
    a /= x;
    b /= x;
    if (a < 1 || a > 4096 || b < 1 || b > 4096) return false;
    D = (int)d, up = (int)a, down = (int)b;
    return true;
}

// ---- pulse --------------------------------------------------------------------------------------------------------------------------------
inline double pulse_g(int q)
{
    static const double COS8[8] = {1.0, M_SQRT1_2, 0.0, -M_SQRT1_2, -1.0, -M_SQRT1_2, 0.0, M_SQRT1_2};
    if (q == 2 || q == -2) return M_PI / 4.0;
    return COS8[q & 7] / (1.0 - (double)q * (double)q / 4.0);
}
inline int pulse_len(int span_bits) { return SPB * span_bits + 1; }
inline void default_pulse(int span_bits, double *p)
{
    const int c = 8 * span_bits;
    for (int u = 0; u <= 2 * c; u++) p[u] = pulse_g(u - c + 4) - pulse_g(u - c - 4);
}

// ---- bits ---------------------------------------------------------------------------------------------------------------------------------
PSS_DDC_HD inline int n_segments(long n) { return (int)((n + SEG - 1) / SEG); }

// the matched filter at sample j: B(i, br, bi) hands out row sample i in [0, n)
template <class FB>
PSS_DDC_HD inline void matched(FB B, long n, const double *p, int P, long j, double &yr, double &yi)
{
    const int c = (P - 1) / 2;
    double ar = 0.0, ai = 0.0;
    for (int u = 0; u < P; u++) {
        const long i = j + u - c;
        float br = 0.0f, bi = 0.0f;
        if (i >= 0 && i < n) B(i, br, bi);
        ar = fma(p[u], (double)br, ar);
        ai = fma(p[u], (double)bi, ai);
    }
    yr = ar;
    yi = ai;
}

// E[s][o]
template <class FB>
PSS_DDC_HD inline double seg_energy(FB B, long n, const double *p, int P, int s, int o)
{
    const long j1 = (long)(s + 1) * SEG < n ? (long)(s + 1) * SEG : n;
    double e = 0.0;
    for (long j = (long)s * SEG + o; j < j1; j += SPB) {
        double yr, yi;
        matched(B, n, p, P, j, yr, yi);
        e = e + fma(yr, yr, yi * yi);
    }
    return e;
}

// o_s from E [n_seg][16]
PSS_DDC_HD inline int seg_offset(const double *E, int n_seg, int s)
{
    const int a = s - SMOOTH < 0 ? 0 : s - SMOOTH, b = s + SMOOTH > n_seg - 1 ? n_seg - 1 : s + SMOOTH;
    int best = 0;
    double fb = 0.0;
    for (int o = 0; o < SPB; o++) {
        double f = 0.0;
        for (int t = a; t <= b; t++) f = f + E[(size_t)t * SPB + o];
        if (o == 0) fb = f;
        else if (f > fb) { best = o; fb = f; }
    }
    return best;
}

// The strobes of segment s: an inserted one at `ins` (< 0: none), then `count` regular ones 16 apart from `first`.  o_prev: the offset of
// segment s - 1 (ignored for s = 0).
struct Strobes { long ins, first; int count; };
PSS_DDC_HD inline Strobes seg_strobes(int s, int o_prev, int o, long n)
{
    const long j0 = (long)s * SEG, j1 = j0 + SEG < n ? j0 + SEG : n;
    Strobes r;
    r.ins = -1;
    r.first = j0 + o;
    r.count = r.first < j1 ? (int)((j1 - 1 - r.first) / SPB) + 1 : 0;
    if (s > 0 && r.count > 0) {
        const long last = j0 - SPB + o_prev;
        const long gap = r.first - last;
        if (gap < 8) { r.first += SPB; r.count--; }
        else if (gap > 24) r.ins = last + SPB;
    }
    return r;
}
PSS_DDC_HD inline int strobes_total(const Strobes &r) { return r.count + (r.ins >= 0); }
// strobe k of the segment (k < strobes_total)
PSS_DDC_HD inline long strobe_at(const Strobes &r, int k)
{
    if (r.ins >= 0) return k == 0 ? r.ins : r.first + (long)(k - 1) * SPB;
    return r.first + (long)k * SPB;
}
// the last strobe of segment s - 1 as segment s sees it (s >= 1: the segment before is full)
PSS_DDC_HD inline long last_of_prev(int s, int o_prev) { return (long)s * SEG - SPB + o_prev; }

PSS_DDC_HD inline uint8_t data_bit(double pr, double pi, double yr, double yi) { return fma(pr, yr, pi * yi) < 0.0 ? 1 : 0; }

// ---- groups -------------------------------------------------------------------------------------------------------------------------------
// the checkword of a 16-bit information word
PSS_DDC_HD inline uint32_t checkword(uint32_t info)
{
    uint32_t r = info << 10;
    for (int b = 25; b >= 10; b--)
        if (r & (1u << b)) r ^= POLY << (b - 10);
    return r & 0x3FFu;
}
// the 26 bits at position i, first bit the most significant
PSS_DDC_HD inline uint32_t block_at(const uint8_t *bits, long i)
{
    uint32_t w = 0;
    for (int k = 0; k < BLOCK; k++) w = (w << 1) | (bits[i + k] & 1u);
    return w;
}
PSS_DDC_HD inline bool block_valid(uint32_t w, uint32_t offset) { return ((checkword(w >> 10) ^ offset) & 0x3FFu) == (w & 0x3FFu); }

// the group at bit i of a row of nb bits (i + GROUP <= nb): true and the four information words where all four blocks pass
PSS_DDC_HD inline bool group_at(const uint8_t *bits, long i, uint16_t *g)
{
    const uint32_t a = block_at(bits, i);
    if (!block_valid(a, OFF_A)) return false;
    const uint32_t b = block_at(bits, i + BLOCK);
    if (!block_valid(b, OFF_B)) return false;
    const uint32_t c = block_at(bits, i + 2 * BLOCK);
    if (!block_valid(c, ((b >> 10) >> 11) & 1u ? OFF_CP : OFF_C)) return false;
    const uint32_t d = block_at(bits, i + 3 * BLOCK);
    if (!block_valid(d, OFF_D)) return false;
    g[0] = (uint16_t)(a >> 10);
    g[1] = (uint16_t)(b >> 10);
    g[2] = (uint16_t)(c >> 10);
    g[3] = (uint16_t)(d >> 10);
    return true;
}

}  // namespace pss_rds

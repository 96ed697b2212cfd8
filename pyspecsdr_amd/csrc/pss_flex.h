// pss_flex.h — the arithmetic of the FLEX receiver (what the reference's command list hands to `rtl_fm ... | multimon-ng -a FLEX`,
// rtlcoms.json "Monitor Pager traffic (Def. 138M)"), stated ONCE for the kernels (pss_flex.hip: k_flex_detect, k_flex_head, k_flex_keep,
// k_flex_walk, k_flex_compact), the host twin (pss_h_flex_frames) and the stand-alone host check (tests/flex_host.cpp).  The reference has
// no such arithmetic, so this statement is the project's own (PARITY.md "FLEX").  The air-interface constants (marker, mode codes, the
// word layout, the interleave, the phase multiplex) are the published ones as multimon-ng's demod_flex.c reads them, written from memory:
// THEY HAVE NOT BEEN CHECKED AGAINST A TRANSMITTER.  Every output follows from indices in the ROW, never from how the row was cut.
//
//   rows       float32 discriminator rows from pss_ais_front with a boxcar: default_pulse(h): P = the largest odd number <= h (at least 1),
//              every tap 1.0 / P.  h = the samples of a 3200-baud symbol, in [1, 64]; 12 at 38 400 S/s.  Everything lies on the grid of h.
//   values     a 1600-baud symbol whose first strobe is the row index t has the value v(t) = y[t] + y[t + h], one float32 add; a 3200-baud
//              symbol at t has the value y[t].  One front pass serves both rates.
//   candidate  a start s of a row of n samples exists where s >= 0 and s + 5936 h <= n.  Its 64 sync bits are v_k = v(s + 2 h k), k = 0 .. 63.
//              c = (the float32 sum of the v_k, added one at a time in ascending order to +0) * 0.015625f.
//              bit k = v_k > c (a NaN is false); the first bit is the MSB of the 64-bit word AAAA MMMMMMMM CCCC.
//              mark = popcount(M ^ 0xA6C6AAAA).  The start passes iff mark <= sync_errors, or 32 - mark <= sync_errors: then the channel is
//              inverted, mark = 32 - mark, A and C are complemented here and every later bit_a is complemented;
//              and outer = popcount((A ^ ~C) & 0xFFFF) <= sync_errors (the caller's sync_errors, in [0, 3]).
//              a = (the float32 sum of |v_k - c|, ascending, to +0) * 0.015625f.
//   mode       dist = the smallest popcount(A ^ code) over the table, the lowest index winning a tie; more than sync_errors: no frame.
//              0: 0x870C 1600 baud / 2 levels   1: 0xB068 1600 / 4   2: 0x7B18 3200 / 2   3: 0xDEA0 3200 / 4   4: 0x4C7C 3200 / 4
//   FIW        32 bits at 1600 baud, two levels: bit k = v(s + 2 h (80 + k)) > c, complemented on an inverted channel, the first bit
//              is bit 0.  A FLEX word is a POCSAG codeword bit-reversed (data in bits 0 .. 20, check bits in 21 .. 30, even parity in bit
//              31): the check is pss_pocsag::check(brev32(w), fix) and its 1024-entry table is shared.  d = w & 0x1FFFFF;
//              nibble_sum(d) = (d & 15) + (d >> 4 & 15) + (d >> 8 & 15) + (d >> 12 & 15) + (d >> 16 & 15) + (d >> 20 & 1), & 15, must be 15.
//              cycle = d >> 4 & 15, frame = d >> 8 & 127.  Uncorrectable within fix, or a wrong sum: no frame.
//   accepted   a candidate with a mode and a FIW.  mism = mark + outer + dist; e = mism + the FIW's fixed bits.
//   one        an accepted A is dropped iff some accepted B of the same row has 0 < |s_B - s_A| < 2 h and
//   record     e_B < e_A, or e_B = e_A and (a_B > a_A, or a_B = a_A and s_B < s_A).  B's own fate does not matter, so the rule does not depend
//              on the order of evaluation; of two accepted starts less than 2 h apart exactly one drops the other.  The rule runs BEFORE
//              the data is read: a kept start whose data fails max_bad leaves no record and brings no neighbour back.
//   data       starts 304 h past s (112 sync bit times and 40 of Sync 2, which is not read).  Stream p (0 or 1) has 2816 symbols, symbol i
//              at t = s + 304 h + 2 h i + p h.  At 1600 baud only stream 0 exists, its value is v(t), centre = c, amp = a.  At 3200 baud
//              stream 0 is the even symbols and stream 1 the odd ones, the value is y[t], centre = c * 0.5f, amp = a * 0.5f (one float32
//              multiply each, exact unless the product is subnormal, where it rounds to nearest even on host and device alike).
//              T = 0.6666667f * amp; lo = centre - T; hi = centre + T (one float32 operation each).
//              bit_a = value > centre, complemented on an inverted channel.  bit_b = value > lo and not value > hi: the two inner levels,
//              the same on an inverted channel.  So +4800 / +1600 / -1600 / -4800 Hz read 10 / 11 / 01 / 00.
//   phases     A = stream 0's bit_a; B = stream 0's bit_b (four levels only); C = stream 1's bit_a; D = stream 1's bit_b (four levels).
//              Symbol i of a stream is bit (i & 255) >> 3 of word 8 (i >> 8) + (i & 7) of its phases: 11 blocks of 8 words, 88 a phase.
//   check      every word of an active phase through the FIW's check with the caller's fix in [0, 2].  n_bad = the uncorrectable words;
//              the frame is reported iff n_bad <= max_bad (the caller's, in [0, 352]).
//   record     words[4][88] corrected (0 where uncorrectable and in unused phases), fix[4][88] 0, 1, 2 or 255 (0 in unused phases), fiw,
//              row, pos = s, meta[0] = mism | inverted << 8 | mode << 12 | FIW fixed bits << 16, meta[1] = n_bad | total fixed bits of the
//              phase words << 16, score = a.
//   non-finite a NaN or an infinity among the 128 samples of the sync bits makes c non-finite or every comparison one-sided, and no marker
//              passes: no frame.  In the FIW and the data a NaN compares false everywhere: bit 0 before the polarity, bit_b 0; +inf reads as
//              the top level and -inf as the bottom one.
//   windows    a call reports the starts [s_begin, s_end); it evaluates [s_begin - (2 h - 1), s_end + 2 h - 1) clipped to the row, and the
//              buffer must hold the samples those starts read: 5936 h from each.
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation.
#pragma once
#include <cmath>
#include <cstdint>

#include "pss_pocsag.h"

#if defined(__HIPCC__)
#define PSS_FLEX_HD __host__ __device__
#else
#define PSS_FLEX_HD
#endif

namespace pss_flex {

constexpr int MIN_H = 1, MAX_H = 64;
constexpr uint32_t MARKER = 0xA6C6AAAAu;
constexpr int SYNC_BITS = 64;
constexpr int FIW_BIT = 80;                      // the FIW's first bit time behind the start
constexpr int DATA_BIT = 152;                    // 112 bit times of sync 1, FIW and the pause, 40 of sync 2
constexpr int N_PHASES = 4, N_BLOCKS = 11, N_WORDS = 8 * N_BLOCKS, N_SYM = 256 * N_BLOCKS;
constexpr long FRAME_H = 2l * DATA_BIT + 2l * N_SYM;   // 5936: the samples of a frame in units of h
constexpr int HEAD_V = 2 * (SYNC_BITS - 1);      // 126: the last sync value's offset in units of h
constexpr int MAX_SYNC_ERRORS = 3, MAX_FIX = 2, MAX_BAD = N_PHASES * N_WORDS;
constexpr int UNCORRECTABLE = 255;
constexpr int N_MODES = 5;
constexpr float TWO_THIRDS = 0.6666667f;
static_assert(FRAME_H == 5936 && N_WORDS == 88 && N_SYM == 2816 && MAX_BAD == 352, "the reach of a frame");

struct Mode { uint32_t code; bool fast, four; };
PSS_FLEX_HD inline Mode mode_of(int m)
{
    switch (m) {
    case 0: return {0x870Cu, false, false};
    case 1: return {0xB068u, false, true};
    case 2: return {0x7B18u, true, false};
    case 3: return {0xDEA0u, true, true};
    default: return {0x4C7Cu, true, true};
    }
}
// which of the phases A, B, C, D a mode fills
PSS_FLEX_HD inline bool active(int mode, int phase)
{
    const Mode m = mode_of(mode);
    return phase == 0 || (phase == 1 && m.four) || (phase == 2 && m.fast) || (phase == 3 && m.fast && m.four);
}

PSS_FLEX_HD inline uint32_t brev32(uint32_t v)
{
    v = (v >> 16) | (v << 16);
    v = ((v & 0xFF00FF00u) >> 8) | ((v & 0x00FF00FFu) << 8);
    v = ((v & 0xF0F0F0F0u) >> 4) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v & 0xCCCCCCCCu) >> 2) | ((v & 0x33333333u) << 2);
    return ((v & 0xAAAAAAAAu) >> 1) | ((v & 0x55555555u) << 1);
}

// ---- pulse ------------------------------------------------------------------------------------------------------------------------------------
inline int pulse_len(int h) { return (h & 1) ? h : (h > 1 ? h - 1 : 1); }
inline void default_pulse(int h, double *g)
{
    const int P = pulse_len(h);
    for (int u = 0; u < P; u++) g[u] = 1.0 / (double)P;
}

// ---- the code ---------------------------------------------------------------------------------------------------------------------------------
// the word of 21 data bits: the data in bits 0 .. 20, the BCH check bits in 21 .. 30, even parity in bit 31
inline uint32_t word(uint32_t data21) { return brev32(pss_pocsag::codeword(brev32(data21 & 0x1FFFFFu) >> 11)); }

// -> the bits fixed (0, 1, 2) with the corrected word in `out`, or -1: uncorrectable within `fix` (out = 0)
PSS_FLEX_HD inline int check(uint32_t w, int fix, uint32_t &out)
{
    uint32_t cw;
    const int n = pss_pocsag::check(brev32(w), fix, cw);
    out = n < 0 ? 0u : brev32(cw);
    return n;
}

PSS_FLEX_HD inline int nibble_sum(uint32_t d)
{
    return (int)(((d & 15u) + (d >> 4 & 15u) + (d >> 8 & 15u) + (d >> 12 & 15u) + (d >> 16 & 15u) + (d >> 20 & 1u)) & 15u);
}

// ---- candidate --------------------------------------------------------------------------------------------------------------------------------
PSS_FLEX_HD inline bool exists(long s, long n, int h) { return s >= 0 && s + FRAME_H * h <= n; }

// The sync test of a start: V(k) hands out the value v(s + 2 h k), k = 0 .. 63.  c, a, A (polarity undone), mark, outer and inverted are
// set either way.
template <class FV>
PSS_FLEX_HD inline bool candidate(FV V, int sync_errors, float &c, float &a, uint32_t &A, int &mark, int &outer, bool &inverted)
{
    // two passes that each ask for the 64 values, so that no caller holds them: with 64 live values k_flex_detect (1024 threads, 128
    // registers a lane at most) spilled 21; it reads its LDS twice instead
    float t = 0.0f;
    for (int k = 0; k < SYNC_BITS; k++) t = t + V(k);
    c = t * 0.015625f;
    uint32_t hi = 0, lo = 0;
    float d = 0.0f;
    for (int k = 0; k < SYNC_BITS; k++) {
        const float v = V(k);
        if (v > c) (k < 32 ? hi : lo) |= 0x80000000u >> (k & 31);
        d = d + fabsf(v - c);
    }
    a = d * 0.015625f;
    const uint32_t M = hi << 16 | lo >> 16;
    uint32_t Aw = hi >> 16, Cw = lo & 0xFFFFu;
    const int m = pss_pocsag::popcount32(M ^ MARKER);
    inverted = 32 - m <= sync_errors;
    mark = inverted ? 32 - m : m;
    if (inverted) Aw ^= 0xFFFFu, Cw ^= 0xFFFFu;
    A = Aw;
    outer = pss_pocsag::popcount32((Aw ^ ~Cw) & 0xFFFFu);
    return mark <= sync_errors && outer <= sync_errors;
}

// the mode of the outer code A, or -1; dist: its distance
PSS_FLEX_HD inline int nearest_mode(uint32_t A, int sync_errors, int &dist)
{
    int best = -1;
    dist = 17;
    for (int m = 0; m < N_MODES; m++) {
        const int d = pss_pocsag::popcount32((A ^ mode_of(m).code) & 0xFFFFu);
        if (d < dist) dist = d, best = m;
    }
    return dist <= sync_errors ? best : -1;
}

struct Head {
    float c, a;
    int mism, mode, fiw_fix;
    bool inverted;
    uint32_t fiw;
};

// Everything before the data of the start s: V(o) hands out the value v(s + o h).  -> accepted
template <class FV>
PSS_FLEX_HD inline bool head(FV V, int sync_errors, int fix, Head &hd)
{
    uint32_t A;
    int mark, outer, dist;
    hd.mism = 0, hd.mode = 0, hd.fiw_fix = 0, hd.fiw = 0;
    if (!candidate([&](int k) { return V(2 * k); }, sync_errors, hd.c, hd.a, A, mark, outer, hd.inverted)) return false;
    hd.mode = nearest_mode(A, sync_errors, dist);
    if (hd.mode < 0) return false;
    hd.mism = mark + outer + dist;
    uint32_t w = 0;
    for (int k = 0; k < 32; k++)
        if (V(2 * (FIW_BIT + k)) > hd.c) w |= 1u << k;
    if (hd.inverted) w = ~w;
    hd.fiw_fix = check(w, fix, hd.fiw);
    if (hd.fiw_fix < 0) return false;
    return nibble_sum(hd.fiw & 0x1FFFFFu) == 15;
}

PSS_FLEX_HD inline int errors_of(const Head &hd) { return hd.mism + hd.fiw_fix; }

// ---- data -------------------------------------------------------------------------------------------------------------------------------------
struct Slicer { float centre, lo, hi; bool fast, four, inverted; };
PSS_FLEX_HD inline Slicer slicer_of(const Head &hd)
{
    const Mode m = mode_of(hd.mode);
    Slicer z;
    z.fast = m.fast, z.four = m.four, z.inverted = hd.inverted;
    z.centre = m.fast ? hd.c * 0.5f : hd.c;
    const float amp = m.fast ? hd.a * 0.5f : hd.a;
    const float T = TWO_THIRDS * amp;
    z.lo = z.centre - T;
    z.hi = z.centre + T;
    return z;
}

// symbol i of stream p of the start s: R(o) hands out the sample y[s + o] (o in samples)
template <class FR>
PSS_FLEX_HD inline void symbol(FR R, int h, const Slicer &z, int i, int p, bool &bit_a, bool &bit_b)
{
    const long o = (long)(2 * DATA_BIT) * h + 2l * h * i + (long)p * h;
    const float val = z.fast ? R(o) : R(o) + R(o + h);
    bit_a = (val > z.centre) != z.inverted;
    bit_b = val > z.lo && !(val > z.hi);
}

PSS_FLEX_HD inline uint32_t meta0_of(const Head &hd)
{
    return (uint32_t)hd.mism | (hd.inverted ? 1u << 8 : 0u) | (uint32_t)hd.mode << 12 | (uint32_t)hd.fiw_fix << 16;
}
PSS_FLEX_HD inline uint32_t meta1_of(int n_bad, int n_fixed) { return (uint32_t)n_bad | (uint32_t)n_fixed << 16; }

// does accepted B drop accepted A?  (the same row is the caller's)
PSS_FLEX_HD inline bool drops(long s_b, int e_b, float a_b, long s_a, int e_a, float a_a, int h)
{
    const long d = s_b > s_a ? s_b - s_a : s_a - s_b;
    if (d == 0 || d >= 2l * h) return false;
    if (e_b != e_a) return e_b < e_a;
    return a_b > a_a || (a_b == a_a && s_b < s_a);
}

// ---- windows ----------------------------------------------------------------------------------------------------------------------------------
struct Reach { long e0, e1, need_lo, need_hi; };
PSS_FLEX_HD inline long reach(int h) { return FRAME_H * h; }
PSS_FLEX_HD inline Reach reach_of(long s_begin, long s_end, long n, int h)
{
    const long near = 2l * h - 1;
    Reach r;
    r.e0 = s_begin - near < 0 ? 0 : s_begin - near;
    r.e1 = s_end + near > n ? n : s_end + near;
    r.need_lo = r.e0;
    r.need_hi = r.e1 - 1 + reach(h) > n ? n : r.e1 - 1 + reach(h);
    return r;
}

}  // namespace pss_flex

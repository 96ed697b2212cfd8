// pss_pocsag.h — the arithmetic of the POCSAG receiver (what the reference's command list hands to `rtl_fm ... | multimon-ng -a POCSAG1200`,
// rtlcoms.json "Decode Pager", "Monitor Pager traffic"), stated ONCE for the kernels (pss_pocsag.hip: k_pocsag_detect, k_pocsag_walk,
// k_pocsag_keep, k_pocsag_emit), the host twin (pss_h_pocsag_batches) and the stand-alone host check (tests/pocsag_host.cpp).  The reference
// has no such arithmetic, so this statement is the project's own (PARITY.md "POCSAG").  Every output follows from indices in the ROW, never
// from how the row was cut.
//
//   rate       38 400 S/s: whole samples a bit at the three standard rates, spb = 75 (512 bit/s), 32 (1200), 16 (2400).  The kernels take
//              any spb in [2, 128].
//   front      none of its own: pss_ais_front (float32 discriminator, then the caller's odd pulse of at most 65 taps; it reads no rate) with
//              a boxcar.  default_pulse(spb): P = the largest odd number <= min(spb, 65), every tap 1.0 / P.
//   candidate  a start s of a row of n samples exists where s >= 0 and s + 543 spb < n: the sync word and all 16 codewords lie in the row.
//              Its strobes are y[s + spb k], k = 0 .. 543.
//              thr = the float32 sum of strobes 0 .. 31, added one at a time in ascending order from the first, times 0.03125f.  (The
//              sync word 0x7CD215D8 has exactly 16 ones: its own mean is the channel's frequency offset.  No preamble is needed, and a
//              batch in the middle of a transmission is a candidate like the first.)
//              L[k] = y > thr (a NaN is false).  The higher frequency is a 0: data bit = !L[k]; bit k of the word is its bit 31 - k.
//              e = popcount(word ^ 0x7CD215D8).  The start passes iff min(e, 32 - e) <= sync_errors (the caller's, in [0, 2]).
//              inverted = (32 - e < e): every later bit of the batch is complemented.
//              q = the smallest |y[s + spb k] - thr| over k = 0 .. 31, taken as a < q ? a : q in ascending order from q = |y[s] - thr|.
//   walk       codeword j (0 .. 15) takes strobes 32 + 32 j .. 63 + 32 j, the first strobe its bit 31, with the sync word's thr.
//   check      check(cw, fix): S = the remainder of bits 31 .. 1 under x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1 (0x769), P = popcount(cw) & 1.
//              S = 0, P = 0: good, 0 bits fixed.  S = 0, P = 1: bit 0 is wrong, 1 fixed.  S != 0: the error pattern E of weight 1 or 2 in
//              the 31 bits with that syndrome (the 31 + 465 patterns have 496 distinct non-zero syndromes, so a table of 1024 entries holds
//              them; static_assert below); none: uncorrectable.  With w = weight(E) the fixed count is w if P == (w & 1), else w + 1 (the
//              parity bit is wrong as well).  Corrected iff the fixed count <= fix (the caller's, in [0, 2]); otherwise uncorrectable.
//   accept     n_bad = the uncorrectable codewords of the 16; accepted iff n_bad <= max_bad (the caller's, in [0, 16]).
//   record     cw[16] the corrected codewords (0 where uncorrectable), fix[16] 0, 1, 2 or 255, row, pos = s,
//              meta = sync mismatches | inverted << 8 | n_bad << 16 | total fixed bits << 24, score = q.
//   one        an accepted A is dropped iff some accepted B of the same row has the same 16 cw words, 0 < |s_B - s_A| < spb, and
//   record     q_B > q_A or (q_B = q_A and s_B < s_A).  B's own fate does not matter, so the rule does not depend on the order of evaluation.
//   windows    a call reports the starts [s_begin, s_end); it evaluates [s_begin - (spb - 1), s_end + spb - 1) clipped to the row, and the
//              buffer must hold the samples those starts read: up to 543 spb + 1 past the last.
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PSS_POCSAG_HD __host__ __device__
#else
#define PSS_POCSAG_HD
#endif

namespace pss_pocsag {

constexpr long RATE = 38400;
constexpr int MIN_SPB = 2, MAX_SPB = 128;
constexpr int MAX_PULSE = 65;                    // pss_ais_front's
constexpr uint32_t SYNC = 0x7CD215D8u, IDLE = 0x7A89C197u;
constexpr uint32_t GEN = 0x769u;                 // x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
constexpr int SYNC_BITS = 32, N_CW = 16;
constexpr int N_STROBES = SYNC_BITS + 32 * N_CW; // 544: k = 0 .. 543
constexpr int LAST_K = N_STROBES - 1;
constexpr int HEAD_K = SYNC_BITS - 1;            // 31: the candidate test's last strobe
constexpr int MAX_SYNC_ERRORS = 2, MAX_FIX = 2;
constexpr int UNCORRECTABLE = 255;
constexpr int MAX_DEFAULT_DECIM = 204;           // pss_ddc.h's: firwin(20 D + 1, .) has at most 4097 taps up to here
static_assert(LAST_K == 543, "the reach of a batch");

PSS_POCSAG_HD inline int popcount32(uint32_t v)
{
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (int)((((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24);
}
constexpr int weight(uint32_t v)
{
    int n = 0;
    for (; v; v &= v - 1) n++;
    return n;
}

// ---- plan -------------------------------------------------------------------------------------------------------------------------------------
// decim, up, down of a capture at fs Hz (the caller has checked that fs is an integer >= 38 400): false where the reduced ratio leaves
// [1, 4096]
inline bool plan(long fs, int &D, int &up, int &down)
{
    long d = fs / RATE;
    if (d > MAX_DEFAULT_DECIM) d = MAX_DEFAULT_DECIM;
    long a = RATE * d, b = fs;
    long x = a, y = b;
    while (y) { const long t = x % y; x = y; y = t; }
    a /= x;
    b /= x;
    if (a < 1 || a > 4096 || b < 1 || b > 4096) return false;
    D = (int)d, up = (int)a, down = (int)b;
    return true;
}

// ---- pulse ------------------------------------------------------------------------------------------------------------------------------------
inline int pulse_len(int spb)
{
    const int m = spb < MAX_PULSE ? spb : MAX_PULSE;
    return (m & 1) ? m : m - 1;
}
inline void default_pulse(int spb, double *g)
{
    const int P = pulse_len(spb);
    for (int u = 0; u < P; u++) g[u] = 1.0 / (double)P;
}

// ---- the code ---------------------------------------------------------------------------------------------------------------------------------
// the remainder of the 31 bits v (bit 30 first) under GEN
constexpr uint32_t remainder31(uint32_t v)
{
    for (int i = 30; i >= 10; i--)
        if ((v >> i) & 1u) v ^= GEN << (i - 10);
    return v & 0x3FFu;
}
constexpr uint32_t syndrome(uint32_t cw) { return remainder31(cw >> 1); }

// the codeword of 21 data bits: the data in bits 31 .. 11, the BCH check bits in 10 .. 1, even parity in bit 0
constexpr uint32_t codeword(uint32_t data21)
{
    uint32_t cw = (data21 & 0x1FFFFFu) << 11;
    cw |= remainder31(cw >> 1) << 1;
    return cw | (uint32_t)(weight(cw) & 1);
}
static_assert(codeword(SYNC >> 11) == SYNC && codeword(IDLE >> 11) == IDLE, "the sync and idle words are codewords");

// e[S]: the error pattern of weight 1 or 2 in bits 31 .. 1 whose syndrome is S, 0 where there is none; distinct: how many entries are set
struct Table { uint32_t e[1024]; int distinct; };
constexpr Table make_table()
{
    Table t = {};
    for (int i = 1; i < 32; i++) {
        const uint32_t a = 1u << i;
        if (!t.e[syndrome(a)]) t.distinct++;
        t.e[syndrome(a)] = a;
    }
    for (int i = 1; i < 32; i++)
        for (int j = i + 1; j < 32; j++) {
            const uint32_t a = (1u << i) | (1u << j);
            if (!t.e[syndrome(a)]) t.distinct++;
            t.e[syndrome(a)] = a;
        }
    return t;
}
// (a constexpr variable of namespace scope: the host's copy and the device's come from the one initialiser)
#if defined(__HIPCC__)
__device__ constexpr Table D_TABLE = make_table();
#endif
constexpr Table TABLE = make_table();
static_assert(TABLE.distinct == 31 + 465 && TABLE.e[0] == 0, "every pattern of weight 1 or 2 has a non-zero syndrome of its own");

PSS_POCSAG_HD inline uint32_t pattern(uint32_t S)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return D_TABLE.e[S];
#else
    return TABLE.e[S];
#endif
}

// -> the bits fixed (0, 1, 2) with the corrected codeword in `out`, or -1: uncorrectable within `fix` (out = 0)
PSS_POCSAG_HD inline int check(uint32_t cw, int fix, uint32_t &out)
{
    const uint32_t S = syndrome(cw);
    const int P = popcount32(cw) & 1;
    int n;
    uint32_t E;
    if (S == 0) {
        n = P;
        E = (uint32_t)P;
    } else {
        E = pattern(S);
        if (!E) { out = 0; return -1; }
        const int w = popcount32(E);
        n = P == (w & 1) ? w : w + 1;
        if (n > w) E |= 1u;
    }
    if (n > fix) { out = 0; return -1; }
    out = cw ^ E;
    return n;
}

// ---- candidate --------------------------------------------------------------------------------------------------------------------------------
PSS_POCSAG_HD inline bool exists(long s, long n, int spb) { return s >= 0 && s + (long)LAST_K * spb < n; }

// The sync test of the start s: Y(k) hands out the strobe y[s + spb k], k = 0 .. 31.  thr, q, mism and inverted are set either way.
template <class FY>
PSS_POCSAG_HD inline bool candidate(FY Y, int sync_errors, float &thr, float &q, int &mism, bool &inverted)
{
    float v[SYNC_BITS];
    for (int k = 0; k < SYNC_BITS; k++) v[k] = Y(k);
    float t = v[0];
    for (int k = 1; k < SYNC_BITS; k++) t = t + v[k];
    t = t * 0.03125f;
    thr = t;
    uint32_t word = 0;
    float m = fabsf(v[0] - t);
    for (int k = 0; k < SYNC_BITS; k++) {
        if (!(v[k] > t)) word |= 1u << (31 - k);
        const float a = fabsf(v[k] - t);
        m = a < m ? a : m;
    }
    q = m;
    const int e = popcount32(word ^ SYNC);
    inverted = 32 - e < e;
    mism = inverted ? 32 - e : e;
    return mism <= sync_errors;
}

// codeword j of a start that passed, as received: Y(k) hands out the strobe y[s + spb k]
template <class FY>
PSS_POCSAG_HD inline uint32_t received(FY Y, float thr, bool inverted, int j)
{
    uint32_t word = 0;
    for (int k = 0; k < 32; k++)
        if (!(Y(SYNC_BITS + 32 * j + k) > thr)) word |= 1u << (31 - k);
    return inverted ? ~word : word;
}

PSS_POCSAG_HD inline uint32_t meta_of(int mism, bool inverted, int n_bad, int n_fixed)
{
    return (uint32_t)mism | (inverted ? 1u << 8 : 0u) | (uint32_t)n_bad << 16 | (uint32_t)n_fixed << 24;
}

// does accepted B drop accepted A?  (the word comparison is the caller's: same = the same row and the same 16 cw words)
PSS_POCSAG_HD inline bool drops(bool same, long s_b, float q_b, long s_a, float q_a, int spb)
{
    const long d = s_b > s_a ? s_b - s_a : s_a - s_b;
    return same && d > 0 && d < spb && (q_b > q_a || (q_b == q_a && s_b < s_a));
}

// ---- windows ----------------------------------------------------------------------------------------------------------------------------------
// A call reports the starts [s_begin, s_end) of every row.  Their possible suppressors lie spb - 1 starts to either side, clipped to the
// row: the starts [e0, e1) are evaluated, and they read the samples [need_lo, need_hi).
struct Reach { long e0, e1, need_lo, need_hi; };
PSS_POCSAG_HD inline long reach(int spb) { return (long)LAST_K * spb + 1; }
PSS_POCSAG_HD inline Reach reach_of(long s_begin, long s_end, long n, int spb)
{
    Reach r;
    r.e0 = s_begin - (spb - 1) < 0 ? 0 : s_begin - (spb - 1);
    r.e1 = s_end + (spb - 1) > n ? n : s_end + (spb - 1);
    r.need_lo = r.e0;
    r.need_hi = r.e1 - 1 + reach(spb) > n ? n : r.e1 - 1 + reach(spb);
    return r;
}

}  // namespace pss_pocsag

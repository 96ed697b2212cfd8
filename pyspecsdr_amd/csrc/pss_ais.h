// pss_ais.h — the arithmetic of the AIS receiver (what the reference's command list hands to `rtl_fm -M fm -s 48k | aisdecoder`, rtlcoms.json
// "Receive AIS"), stated ONCE for the kernels (pss_ais.hip: k_ais_front, k_ais_detect, k_ais_walk, k_ais_keep, k_ais_emit), the host twins
// (pss_h_ais_front, pss_h_ais_frames) and the stand-alone host check (tests/ais_host.cpp).  The reference has no such arithmetic, so this
// statement is the project's own (PARITY.md "AIS").  Every output follows from indices in the ROW, never from how the row was cut.
//
//   rate       48 000 S/s, SPB = 5 samples a bit (9600 bit/s).
//   front      d[i] = float32 angle of the float32 product x[i] conj(x[i - 1]) (pss_mono.h's disc_product; the caller's model of NumPy's
//              arctan2), d[0] = 0, no gain.  y[i] = sum over u ascending of g[u] d[i + u - c], c = (P - 1) / 2, d = 0 outside the row: one
//              float64 fma chain from +0, rounded once to float32.  g: the caller's table of an odd P in [1, 65].
//   pulse      default_pulse(span_bits): a Gaussian of BT = 0.4 at 5 samples a bit, g[u] = exp(-(2 pi^2 / ln 2) 0.16 ((u - c) / 5)^2),
//              P = 5 span_bits + 1, c = (P - 1) / 2 (an odd span_bits gives an even P centred between two samples, which the front
//              does not take), divided by its sum added ascending.
//   candidate  a start s of a row of n samples exists where s - 45 >= 0 and s + 35 < n; its strobes are y[s + 5 k].
//              thr = (y[s - 40] + y[s - 35] + ... + y[s - 5]) 0.125f, float32, added one at a time in ascending order.
//              L[k] = y[s + 5 k] > thr (a NaN is false), k >= -9; b[k] = (L[k] == L[k - 1]): the NRZI data bit, 1 for no change.
//              The start passes iff b[-8 .. -1] is 01010101 or 10101010 and b[0 .. 7] is 01111110.
//              q = the smallest |y[s + 5 k] - thr| over k = -8 .. 7, taken as a < q ? a : q in ascending order from k = -8.
//   walk       from k = 8, run counts consecutive ones.  A bit is appended, except after run == 5: the next bit, if 0, is dropped (run = 0);
//              if it is 1, one more bit e is read: e == 0 closes the frame (payload = appended bits minus the last 6), e == 1 rejects.
//              Rejected also when a 1031st bit would be appended, or when any strobe lies outside the row.  1030 appended bits hold 205
//              dropped ones before the last run of five, and two more strobes follow it: 1237 strobes, k = 8 .. 1244 (LAST_K).  A start
//              reads the samples [s - 45, s + REACH), REACH = 5 LAST_K + 1 = 6221.
//   check      accepted iff the payload length is a multiple of 8 in [56, 1024] and the CRC-16/X.25 register (reflected 0x8408, init 0xFFFF)
//              over all the bits leaves 0xF0B8.  Byte j holds bits 8 j .. 8 j + 7, the first received the LEAST significant.
//   one        an accepted A is dropped iff some accepted B of the same row has the same length and bytes, 0 < |s_B - s_A| < 5, and
//   record     q_B > q_A or (q_B = q_A and s_B < s_A).  B's own fate does not matter, so the rule does not depend on the order of evaluation.
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation; fma is the fused one.
#pragma once
#include <cmath>
#include <cstdint>

#include "pss_mono.h"

#if defined(__HIPCC__)
#define PSS_AIS_HD __host__ __device__
#else
#define PSS_AIS_HD
#endif

namespace pss_ais {

constexpr long RATE = 48000;
constexpr int SPB = 5;
constexpr int MAX_BYTES = 128;                   // 1008 payload bits and 16 check bits
constexpr int MIN_BITS = 56, MAX_BITS = 8 * MAX_BYTES;
constexpr int MAX_APPENDED = MAX_BITS + 6;       // the closing flag's 0 and five ones are appended before the walk knows them
constexpr int MAX_PULSE = 65, MAX_SPAN = 12;
constexpr int BACK = 9 * SPB;                    // 45: the samples in front of s that a start reads (k = -9)
constexpr int HEAD = 7 * SPB;                    // 35: the candidate test's last strobe (k = 7)
constexpr int LAST_K = 8 + MAX_APPENDED + (MAX_APPENDED / 5 - 1) + 2 - 1;   // 1244: the last strobe a walk can read
constexpr long REACH = (long)SPB * LAST_K + 1;   // 6221
constexpr int NEAR = SPB;                        // starts closer than this slice the same burst
constexpr uint32_t CRC_POLY = 0x8408u, CRC_INIT = 0xFFFFu, CRC_RESIDUE = 0xF0B8u;
constexpr int MAX_DEFAULT_DECIM = 204;           // pss_ddc.h's: firwin(20 D + 1, .) has at most 4097 taps up to here
static_assert(LAST_K == 1244, "the reach of a walk");

// ---- plan -------------------------------------------------------------------------------------------------------------------------------------
// decim, up, down of a capture at fs Hz (the caller has checked that fs is an integer >= 48 000): false where the reduced ratio leaves
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
inline int pulse_len(int span_bits) { return SPB * span_bits + 1; }
inline void default_pulse(int span_bits, double *g)
{
    const int P = pulse_len(span_bits);
    const double c = (P - 1) / 2.0;
    double sum = 0.0;
    for (int u = 0; u < P; u++) {
        const double t = ((double)u - c) / 5.0;
        g[u] = exp(-(2.0 * M_PI * M_PI / M_LN2) * 0.16 * (t * t));
        sum = sum + g[u];
    }
    for (int u = 0; u < P; u++) g[u] = g[u] / sum;
}

// ---- front ------------------------------------------------------------------------------------------------------------------------------------
// the discriminator sample of row index i >= 1: angle(im, re) of x[i] conj(x[i - 1])
template <class FA>
PSS_AIS_HD inline float disc(float cr, float ci, float pr, float pi, FA angle)
{
    float re, im;
    pss_mono::disc_product(cr, ci, pr, pi, re, im);
    return angle(im, re);
}

// y[i]: D(j) hands out d[j] for EVERY j in [i - c, i + c] (zero outside the row)
template <class FD>
PSS_AIS_HD inline float filtered(FD D, const double *g, int P, long i)
{
    const int c = (P - 1) / 2;
    double a = 0.0;
    for (int u = 0; u < P; u++) a = fma(g[u], (double)D(i + u - c), a);
    return (float)a;
}

// the input samples [lo, hi) of a row of n that the outputs [i_begin, i_end) read (i_begin < i_end)
struct Span { long lo, hi; };
PSS_AIS_HD inline Span front_span(long i_begin, long i_end, int P, long n)
{
    const int c = (P - 1) / 2;
    Span r;
    r.lo = i_begin - c - 1 < 0 ? 0 : i_begin - c - 1;
    r.hi = i_end + c > n ? n : i_end + c;
    return r;
}

// ---- candidate --------------------------------------------------------------------------------------------------------------------------------
PSS_AIS_HD inline bool exists(long s, long n) { return s - BACK >= 0 && s + HEAD < n; }

// The flag test of the start s: Y(k) hands out the strobe y[s + 5 k], k = -9 .. 7.  thr and q are set either way.
template <class FY>
PSS_AIS_HD inline bool candidate(FY Y, float &thr, float &q)
{
    float v[17];
    for (int k = -9; k <= 7; k++) v[k + 9] = Y(k);
    float t = v[1];
    for (int k = 2; k <= 8; k++) t = t + v[k];
    t = t * 0.125f;
    thr = t;
    uint32_t bits = 0;   // b[k] at bit k + 8, k = -8 .. 7
    float m = fabsf(v[1] - t);
    for (int k = 1; k < 17; k++) {
        const bool l1 = v[k] > t, l0 = v[k - 1] > t;
        if (l1 == l0) bits |= 1u << (k - 1);
        const float a = fabsf(v[k] - t);
        m = a < m ? a : m;
    }
    q = m;
    // b[-8 .. -1] = 01010101 (b[-8] = 0 at bit 0: 0xAA) or 10101010 (0x55); b[0 .. 7] = 01111110 (0x7E)
    return (bits >> 8) == 0x7Eu && ((bits & 0xFFu) == 0xAAu || (bits & 0xFFu) == 0x55u);
}

PSS_AIS_HD inline uint32_t crc_bit(uint32_t crc, uint32_t bit) { return ((crc ^ bit) & 1u) ? (crc >> 1) ^ CRC_POLY : crc >> 1; }
// the CRC register after n bytes, from CRC_INIT
PSS_AIS_HD inline uint32_t crc_reg(const uint8_t *p, long n)
{
    uint32_t crc = CRC_INIT;
    for (long j = 0; j < n; j++)
        for (int k = 0; k < 8; k++) crc = crc_bit(crc, (p[j] >> k) & 1u);
    return crc;
}

// The walk of a start that passed: Y(k) hands out the strobe y[s + 5 k] for k with s + 5 k < n (k_end = the first k outside the row).
// The payload's bits leave through W(w, word) as 32-bit words, bit p of the payload at bit p % 32 of word p / 32 (the payload runs six
// appended bits behind the walk, so the closing flag never reaches a word).  -> the payload's bytes, 0 where the start is rejected (words
// may have been written all the same).
template <class FY, class FW>
PSS_AIS_HD inline int walk(FY Y, float thr, long k_end, FW W)
{
    bool prev = Y(7) > thr;
    int run = 0, n_app = 0, n_pay = 0;
    uint32_t recent = 0, word = 0, crc = CRC_INIT;
    for (long k = 8;; k++) {
        if (k >= k_end) return 0;
        const bool lv = Y((int)k) > thr;
        const uint32_t b = lv == prev ? 1u : 0u;
        prev = lv;
        if (run == 5) {
            if (!b) { run = 0; continue; }
            if (k + 1 >= k_end) return 0;
            const bool le = Y((int)k + 1) > thr;
            if (le == lv) return 0;   // e = 1: seven ones
            break;
        }
        if (n_app == MAX_APPENDED) return 0;
        if (n_app >= 6) {
            const uint32_t old = (recent >> 5) & 1u;
            crc = crc_bit(crc, old);
            word |= old << (n_pay & 31);
            n_pay++;
            if ((n_pay & 31) == 0) { W(n_pay / 32 - 1, word); word = 0; }
        }
        recent = ((recent << 1) | b) & 0x3Fu;
        n_app++;
        run = b ? run + 1 : 0;
    }
    if (n_pay < MIN_BITS || n_pay > MAX_BITS || (n_pay & 7) || crc != CRC_RESIDUE) return 0;
    if (n_pay & 31) W(n_pay / 32, word);
    return n_pay / 8;
}

// does accepted B drop accepted A?  (the byte comparison is the caller's: same = the same row, equal length and bytes)
PSS_AIS_HD inline bool drops(bool same, long s_b, float q_b, long s_a, float q_a)
{
    const long d = s_b > s_a ? s_b - s_a : s_a - s_b;
    return same && d > 0 && d < NEAR && (q_b > q_a || (q_b == q_a && s_b < s_a));
}

// ---- windows ----------------------------------------------------------------------------------------------------------------------------------
// A call reports the starts [s_begin, s_end) of every row.  Their possible suppressors lie 4 starts to either side, clipped to the row: the
// starts [e0, e1) are evaluated, and they read the samples [need_lo, need_hi).
struct Reach { long e0, e1, need_lo, need_hi; };
PSS_AIS_HD inline Reach reach_of(long s_begin, long s_end, long n)
{
    Reach r;
    r.e0 = s_begin - (NEAR - 1) < 0 ? 0 : s_begin - (NEAR - 1);
    r.e1 = s_end + (NEAR - 1) > n ? n : s_end + (NEAR - 1);
    r.need_lo = r.e0 - BACK < 0 ? 0 : r.e0 - BACK;
    r.need_hi = r.e1 - 1 + REACH > n ? n : r.e1 - 1 + REACH;
    return r;
}

}  // namespace pss_ais

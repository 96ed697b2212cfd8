// pss_apt.h — the arithmetic of the NOAA APT receiver (what the reference's command list hands to `rtl_fm -f 137.62M -M fm -s 60k ... | sox ...
// && wxtoimg`, rtlcoms.json "Capture NOAA in .wav"; the band is pyspecconst.py's NOAA_SAT preset), stated ONCE for the kernels (pss_apt.hip:
// k_apt_front, k_apt_detect, k_apt_score, k_apt_keep, k_apt_emit, k_apt_lines), the host twins (pss_h_apt_front, pss_h_apt_syncs,
// pss_h_apt_lines) and the stand-alone host check (tests/apt_host.cpp).  The reference has no such arithmetic, so this statement is the
// project's own (PARITY.md "APT").  Every output follows from indices in the ROW, never from how the row was cut.
//
//   signal     a line lasts 0.5 s: 2080 words at 4160 words/s, amplitude-modulated on a 2400 Hz subcarrier that frequency-modulates the
//              carrier.  sync A (39 words), space A (47), image A (909), telemetry A (45), sync B (39), space B (47), image B (909),
//              telemetry B (45).  Sync A as words: 4 low, seven pulses `1100` (1040 Hz), 7 low.  Sync B: 4 low, seven pulses `11100`.
//   rates      rows are complex64 at 62 400 S/s: 15 samples a word, 26 a subcarrier cycle.  The envelope runs at 12 480 S/s (decimation 5):
//              ENV_SPW = 3 samples a word, LINE_ENV = 6240 a line.
//   front      d[i] = pss_rds.h's disc (float32 polar discriminator, no gain, d[0] = 0); z[i] = d[i] times pss_ddc.h's rotor at
//              word_of(2400, fs) and index i of the row; pss_ddc.h's filter in float64 (fma chains in blocks of 64 taps, zero outside the
//              row, the block sums added in ascending order): re, im.  env[m] = (float) sqrt(fma(re, re, im * im)): one float64 product,
//              one fused multiply-add, one correctly rounded square root, one rounding to float32 — the form host and device round alike.
//              The complex baseband is never stored.  Default taps: firwin(79, 1 / 15), a 2080 Hz low-pass at 62 400 S/s.
//   candidate  every envelope sample s of a row of n samples with s >= 0 and s + 116 < n.  Strobes e[k] = env[s + 3 k + 1], k = 0 .. 38 (the
//              middle sample of each of the 39 words).  thr = the float32 sum of e[4] .. e[31], added one at a time in ascending order from
//              e[4], divided by 28.0f: those 28 strobes are the pulse train's own, 14 high and 14 low, so no level is assumed.  bit k =
//              e[k] > thr (a NaN strobe compares false).  mism = popcount(bits ^ sync A); accepted iff mism <= sync_errors (the caller's,
//              in [0, 4]).  score = (the float32 sum of the 14 high strobes of k = 4 .. 31 in ascending order - that of the 14 low ones)
//              / 14.0f.  A NaN thr (a NaN among e[4 .. 31], or +inf and -inf) makes every comparison false: all 39 bits are 0, mism = 14,
//              never accepted.  An infinite thr does the same.  Sync B read against sync A differs in at least 12 words: never accepted.
//   one        among accepted starts of a row less than NEAR = 3120 (half a line) apart, B drops A where B has fewer mismatches; on equal
//   record     mismatches the higher score; on equal scores the earlier start.  Mismatches come first: a full-contrast 1040 Hz texture can
//              out-score the true sync with two mismatches.  B's own fate does not matter, so the order of evaluation does not either.
//   record     row, pos = s (the first envelope sample of sync A's first word), meta = mism, score.
//   windows    a call reports the starts [s_begin, s_end); it evaluates [s_begin - 3119, s_end + 3119) clipped to the row, and the buffer
//              must hold the samples those starts read: 117 from each start, clipped to the row.
//   lines      word[j] = env[p + 3 j + 1], j = 0 .. 2079, for a position p of the CALLER's (any int64) and a row; +0 where the sample lies
//              outside the row, and everywhere for a row index outside [0, n_rows).
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+`, `-` and `/` is one IEEE operation; fma is the fused one.
#pragma once
#include <cmath>
#include <cstdint>

#include "pss_ddc.h"
#include "pss_rds.h"

namespace pss_apt {

constexpr long RATE = 62400;                     // the rows
constexpr double SUBCARRIER_HZ = 2400.0;
constexpr int DECIM = 5;                         // the receiver's: the envelope at 12 480 S/s
constexpr int N_DEFAULT_TAPS = 79;
constexpr double DEFAULT_CUTOFF = 1.0 / 15.0;    // firwin's, of the Nyquist rate: 2080 Hz
constexpr int ENV_SPW = 3;                       // envelope samples a word
constexpr int LINE_WORDS = 2080, LINE_ENV = LINE_WORDS * ENV_SPW;
constexpr int SYNC_WORDS = 39;
constexpr int FIRST_K = 4, END_K = 32;           // the pulse train's strobes: k = 4 .. 31
constexpr int REACH = 117;                       // a start s reads env[s + 1 .. s + 115] and exists where s + 116 < n
constexpr long NEAR = LINE_ENV / 2;              // 3120: the one-record rule's distance
constexpr int MAX_SYNC_ERRORS = 4;
constexpr int FIELD_SYNC = 39, FIELD_SPACE = 47, FIELD_IMAGE = 909, FIELD_TELEMETRY = 45;
static_assert(2 * (FIELD_SYNC + FIELD_SPACE + FIELD_IMAGE + FIELD_TELEMETRY) == LINE_WORDS, "the fields of a line");
static_assert(ENV_SPW * (SYNC_WORDS - 1) + 1 + 1 < REACH && LINE_ENV == 6240 && NEAR == 3120, "the reach of a sync and of the rule");

// bit k: word k of sync A
constexpr uint64_t sync_a()
{
    uint64_t w = 0;
    for (int k = FIRST_K; k < END_K; k++)
        if (((k - FIRST_K) & 2) == 0) w |= 1ull << k;
    return w;
}
// bit k: word k of sync B (0000 + 7 x 11100)
constexpr uint64_t sync_b()
{
    uint64_t w = 0;
    for (int k = 4; k < SYNC_WORDS; k++)
        if ((k - 4) % 5 < 3) w |= 1ull << k;
    return w;
}
constexpr int weight64(uint64_t v)
{
    int n = 0;
    for (; v; v &= v - 1) n++;
    return n;
}
constexpr uint64_t SYNC_A = sync_a(), SYNC_B = sync_b();
static_assert(SYNC_A == 0x33333330ull && weight64(SYNC_A) == 14, "000011001100110011001100110011000000000, first word in bit 0");
static_assert(weight64(SYNC_A ^ SYNC_B) > 2 * MAX_SYNC_ERRORS, "sync B is never taken for sync A");

PSS_DDC_HD inline int popcount64(uint64_t v)
{
    v = v - ((v >> 1) & 0x5555555555555555ull);
    v = (v & 0x3333333333333333ull) + ((v >> 2) & 0x3333333333333333ull);
    return (int)((((v + (v >> 4)) & 0x0F0F0F0F0F0F0F0Full) * 0x0101010101010101ull) >> 56);
}

// ---- plan -------------------------------------------------------------------------------------------------------------------------------------
// decim, up, down of a capture at fs Hz (the caller has checked that fs is an integer >= 62 400): false where the reduced ratio leaves
// [1, 4096]
inline bool plan(long fs, int &D, int &up, int &down)
{
    long d = fs / RATE;
    if (d > pss_dc::MAX_DEFAULT_DECIM) d = pss_dc::MAX_DEFAULT_DECIM;
    long a = RATE * d, b = fs;
    long x = a, y = b;
    while (y) { const long t = x % y; x = y; y = t; }
    a /= x;
    b /= x;
    if (a < 1 || a > 4096 || b < 1 || b > 4096) return false;
    D = (int)d, up = (int)a, down = (int)b;
    return true;
}

// ---- front ------------------------------------------------------------------------------------------------------------------------------------
// pss_ddc.h's combine before its rounding, then the magnitude: S(b, sr, si) hands out the block sums in ascending b
template <class FS>
PSS_DDC_HD inline float envelope(int n_blocks, FS S)
{
    double ar, ai;
    S(0, ar, ai);
    for (int b = 1; b < n_blocks; b++) {
        double sr, si;
        S(b, sr, si);
        ar = ar + sr;
        ai = ai + si;
    }
    return (float)sqrt(fma(ar, ar, ai * ai));
}

// One output on one thread: Z(j, zr, zi) hands out the mixed sample of row index j (zero outside the row), j = m D + lead - k.
template <class FZ>
inline float output(long m, int D, const double *h, int T, int lead, FZ Z)
{
    const long j0 = m * D + lead;
    return envelope(pss_dc::n_blocks(T), [&](int b, double &sr, double &si) {
        const int k0 = b * pss_dc::B, nk = T - k0 < pss_dc::B ? T - k0 : pss_dc::B;
        pss_dc::block_sum([&](int kk) { return h[k0 + kk]; }, nk, [&](int kk, double &zr, double &zi) { Z(j0 - (k0 + kk), zr, zi); }, sr, si);
    });
}

// ---- candidate --------------------------------------------------------------------------------------------------------------------------------
PSS_DDC_HD inline bool exists(long s, long n) { return s >= 0 && s < n - (REACH - 1); }

// The sync test of the start s: E(k) hands out the strobe env[s + 3 k + 1], k = 0 .. 38.  mism and score are set either way.
template <class FE>
PSS_DDC_HD inline bool candidate(FE E, int sync_errors, int &mism, float &score)
{
    float v[SYNC_WORDS];
    for (int k = 0; k < SYNC_WORDS; k++) v[k] = E(k);
    float t = v[FIRST_K];
    for (int k = FIRST_K + 1; k < END_K; k++) t = t + v[k];
    t = t / 28.0f;
    uint64_t bits = 0;
    for (int k = 0; k < SYNC_WORDS; k++)
        if (v[k] > t) bits |= 1ull << k;
    // k = 4, 5, 8, 9, ... are the high ones; 6, 7, 10, 11, ... the low ones
    float hi = v[FIRST_K], lo = v[FIRST_K + 2];
    hi = hi + v[FIRST_K + 1];
    lo = lo + v[FIRST_K + 3];
    for (int k = FIRST_K + 4; k < END_K; k += 4) {
        hi = hi + v[k];
        hi = hi + v[k + 1];
        lo = lo + v[k + 2];
        lo = lo + v[k + 3];
    }
    score = (hi - lo) / 14.0f;
    mism = popcount64(bits ^ SYNC_A);
    return mism <= sync_errors;
}

// does accepted B drop accepted A of the same row?
PSS_DDC_HD inline bool drops(long s_b, int mism_b, float q_b, long s_a, int mism_a, float q_a)
{
    const long d = s_b > s_a ? s_b - s_a : s_a - s_b;
    if (d == 0 || d >= NEAR) return false;
    if (mism_b != mism_a) return mism_b < mism_a;
    return q_b > q_a || (q_b == q_a && s_b < s_a);
}

// ---- windows ----------------------------------------------------------------------------------------------------------------------------------
// A call reports the starts [s_begin, s_end) of every row.  Their possible suppressors lie NEAR - 1 starts to either side, clipped to the
// row: the starts [e0, e1) are evaluated, and they read the samples [need_lo, need_hi).
struct Reach { long e0, e1, need_lo, need_hi; };
PSS_DDC_HD inline Reach reach_of(long s_begin, long s_end, long n)
{
    Reach r;
    r.e0 = s_begin - (NEAR - 1) < 0 ? 0 : s_begin - (NEAR - 1);
    r.e1 = s_end + (NEAR - 1) > n ? n : s_end + (NEAR - 1);
    r.need_lo = r.e0;
    r.need_hi = r.e1 - 1 + REACH > n ? n : r.e1 - 1 + REACH;
    return r;
}

// ---- lines ------------------------------------------------------------------------------------------------------------------------------------
// does envelope index p + t (t in [0, LINE_ENV)) lie in a row of n samples?  No sum that can overflow.
PSS_DDC_HD inline bool line_in(long p, int t, long n) { return p > -(long)LINE_ENV && p < n && p + t >= 0 && p + t < n; }
// word j of the line at p: E(i) hands out env[i] of the row
template <class FE>
PSS_DDC_HD inline float line_word(FE E, long p, int j, long n)
{
    const int t = ENV_SPW * j + 1;
    return line_in(p, t, n) ? E(p + t) : 0.0f;
}

}  // namespace pss_apt

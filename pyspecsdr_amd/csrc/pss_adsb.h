// pss_adsb.h — the arithmetic of the Mode S / ADS-B receiver (what the reference's command list hands to dump1090, rtlcoms.json "Decode
// Aircraft Transmissions"), stated ONCE for the kernels (pss_adsb.hip: k_adsb_detect, k_adsb_keep, k_adsb_emit), the host twin
// (pss_h_adsb_frames; its walk over neighbouring starts is pss_starts.h's) and the stand-alone host check (tests/adsb_host.cpp).  The reference has no such arithmetic, so this statement is the
// project's own (PARITY.md "ADS-B").  Every output follows from indices in the CAPTURE, never from how the capture was cut.
//
//   rate      spc = fs / 2 000 000 samples per 0.5 us chip, an integer in [1, 8].
//   m[i]      = re re + im im in float32: two products and one add.
//   E(c)      the energy of chip c of a candidate that starts at capture sample s: m[s + spc c] + ... + m[s + spc c + spc - 1], float32, added
//             in ascending order starting from the first term.
//   preamble  16 chips, pulses at chips 0, 2, 7, 9.  hi = the minimum of those four energies, lo = the maximum of the other twelve, both
//             carrying a NaN through; the candidate passes iff hi > ratio lo (one float32 product, a strict comparison: a NaN fails).
//   bits      bit i = E(16 + 2 i) > E(17 + 2 i); 112 bits if bit 0 is 1, else 56.  The candidate exists only where its span of
//             spc (16 + 2 n_bits) samples lies inside the capture.  Byte j of the message holds bits 8 j .. 8 j + 7, the first the most
//             significant; a short frame's bytes 7 .. 13 are zero.
//   check     r = the 24-bit remainder of the whole message under 0x1FFF409; DF = bits 0 .. 4.  Accepted iff DF 17 / 18 and r = 0, or DF 11
//             and (r & 0xFFFF80) = 0, or DF 0 / 4 / 5 / 16 / 20 / 21 and r is in the caller's ascending address list (bisection).  Every
//             other format is rejected; there is no error correction.
//   one       an accepted A is dropped iff some accepted B has the same length and bytes, 0 < |s_B - s_A| < 2 spc, and hi_B > hi_A or
//   record    (hi_B = hi_A and s_B < s_A).  B's own fate does not matter, so the rule does not depend on the order of evaluation.
// Every unit that includes this header is compiled with -ffp-contract=off: each `*` and `+` is one IEEE operation.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PSS_ADSB_HD __host__ __device__
#else
#define PSS_ADSB_HD
#endif

namespace pss_adsb {

constexpr int MAX_SPC = 8;
constexpr double CHIP_RATE = 2000000.0;
constexpr int PRE_CHIPS = 16;                         // the preamble: 8 us
constexpr int LONG_BITS = 112, SHORT_BITS = 56;
constexpr int MSG_BYTES = 14;
constexpr int REACH_CHIPS = PRE_CHIPS + 2 * LONG_BITS;   // 240: what a start may read, in chips
constexpr uint32_t GENERATOR = 0x1FFF409u;
constexpr uint32_t MAX_ADDRESS = 1u << 24;

// spc of a capture at fs Hz, 0 where fs / 2 000 000 is no integer in [1, 8]
inline int plan(double fs)
{
    if (!(fs >= CHIP_RATE && fs <= CHIP_RATE * MAX_SPC)) return 0;
    const double q = fs / CHIP_RATE;
    const int spc = (int)q;
    return (double)spc == q && (double)spc * CHIP_RATE == fs ? spc : 0;
}

PSS_ADSB_HD inline float mag(float re, float im) { return re * re + im * im; }

// the sum of m[i .. i + spc), ascending from the first term; M(i) hands out m of capture sample i
template <class FM>
PSS_ADSB_HD inline float chip_sum(FM M, long i, int spc)
{
    float e = M(i);
    for (int k = 1; k < spc; k++) e = e + M(i + k);
    return e;
}

// minimum and maximum that hand a NaN on, whichever side it comes in from
PSS_ADSB_HD inline float min_nan(float a, float b) { return (a < b || a != a) ? a : b; }
PSS_ADSB_HD inline float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

// the preamble test on the sixteen chip energies e[0 .. 15]: true where it passes; hi is set either way
PSS_ADSB_HD inline bool preamble(const float *e, float ratio, float &hi)
{
    const float h = min_nan(min_nan(e[0], e[2]), min_nan(e[7], e[9]));
    float l = max_nan(e[1], e[3]);
    l = max_nan(l, e[4]);
    l = max_nan(l, e[5]);
    l = max_nan(l, e[6]);
    l = max_nan(l, e[8]);
    for (int c = 10; c < PRE_CHIPS; c++) l = max_nan(l, e[c]);
    hi = h;
    return h > ratio * l;
}

PSS_ADSB_HD inline int bits_of(bool bit0) { return bit0 ? LONG_BITS : SHORT_BITS; }
// the samples a frame of n_bits spans
PSS_ADSB_HD inline long span_of(int n_bits, int spc) { return (long)spc * (PRE_CHIPS + 2 * n_bits); }
PSS_ADSB_HD inline bool fits(long s, int n_bits, int spc, long n_capture) { return s >= 0 && s + span_of(n_bits, spc) <= n_capture; }

// the 24-bit remainder of the first n_bits bits of msg (a multiple of 8)
PSS_ADSB_HD inline uint32_t crc24(const uint8_t *msg, int n_bits)
{
    uint32_t r = 0;
    for (int j = 0; j < n_bits / 8; j++) {
        const uint32_t b = msg[j];
        for (int k = 7; k >= 0; k--) {
            r = (r << 1) | ((b >> k) & 1u);
            if (r & 0x1000000u) r ^= GENERATOR;
        }
    }
    return r;
}

PSS_ADSB_HD inline int df_of(const uint8_t *msg) { return msg[0] >> 3; }

// bisection in an ascending list
PSS_ADSB_HD inline bool listed(const uint32_t *icao, int n_icao, uint32_t a)
{
    int lo = 0, hi = n_icao;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (icao[mid] < a) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_icao && icao[lo] == a;
}

// the check of a message of format df whose remainder is r
PSS_ADSB_HD inline bool accepted_r(int df, uint32_t r, const uint32_t *icao, int n_icao)
{
    if (df == 17 || df == 18) return r == 0;
    if (df == 11) return (r & 0xFFFF80u) == 0;
    if (df == 0 || df == 4 || df == 5 || df == 16 || df == 20 || df == 21) return listed(icao, n_icao, r);
    return false;
}
PSS_ADSB_HD inline bool accepted(const uint8_t *msg, int n_bits, const uint32_t *icao, int n_icao)
{
    return accepted_r(df_of(msg), crc24(msg, n_bits), icao, n_icao);
}

// The remainder is linear over the message bits: r = XOR over the set bits i of x^(n_bits - 1 - i) mod the generator.  POWERS.t[k] = x^k
// mod the generator, k < 112: what one lane per bit folds by xor (pss_adsb.hip); crc24 above is the same integer function.
struct Powers {
    uint32_t t[LONG_BITS];
    constexpr Powers() : t()
    {
        uint32_t r = 1;
        for (int k = 0; k < LONG_BITS; k++) {
            t[k] = r;
            r <<= 1;
            if (r & 0x1000000u) r ^= GENERATOR;
        }
    }
};

// does accepted B drop accepted A?  (the byte comparison is the caller's: same = equal length and bytes)
PSS_ADSB_HD inline bool drops(bool same, long s_b, float hi_b, long s_a, float hi_a, int spc)
{
    const long d = s_b > s_a ? s_b - s_a : s_a - s_b;
    return same && d > 0 && d < 2 * (long)spc && (hi_b > hi_a || (hi_b == hi_a && s_b < s_a));
}

// A whole candidate on one thread: false where the start holds no accepted frame.  M(i): m of capture sample i, asked only inside the
// candidate's own span.  msg: MSG_BYTES bytes, written where the preamble passed.
template <class FM>
PSS_ADSB_HD inline bool candidate(FM M, long s, long n_capture, int spc, float ratio, const uint32_t *icao, int n_icao, uint8_t *msg, int &n_bits,
                                  float &hi)
{
    if (!fits(s, SHORT_BITS, spc, n_capture)) return false;
    float e[PRE_CHIPS];
    for (int c = 0; c < PRE_CHIPS; c++) e[c] = chip_sum(M, s + (long)spc * c, spc);
    if (!preamble(e, ratio, hi)) return false;
    auto bit = [&](int i) { return chip_sum(M, s + (long)spc * (PRE_CHIPS + 2 * i), spc) > chip_sum(M, s + (long)spc * (PRE_CHIPS + 2 * i + 1), spc); };
    const bool b0 = bit(0);
    n_bits = bits_of(b0);
    if (!fits(s, n_bits, spc, n_capture)) return false;
    for (int j = 0; j < MSG_BYTES; j++) msg[j] = 0;
    if (b0) msg[0] = 0x80;
    for (int i = 1; i < n_bits; i++)
        if (bit(i)) msg[i >> 3] |= (uint8_t)(0x80u >> (i & 7));
    return accepted(msg, n_bits, icao, n_icao);
}

// ---- windows ------------------------------------------------------------------------------------------------------------------------------
// A call reports the starts [s_begin, s_end).  Their possible suppressors lie 2 spc - 1 starts to either side, clipped to the capture: the
// starts [e0, e1) are evaluated, and they read the samples [e0, need_hi).
struct Reach { long e0, e1, need_hi; };
PSS_ADSB_HD inline Reach reach_of(long s_begin, long s_end, int spc, long n_capture)
{
    Reach r;
    r.e0 = s_begin - (2 * spc - 1) < 0 ? 0 : s_begin - (2 * spc - 1);
    r.e1 = s_end + (2 * spc - 1) > n_capture ? n_capture : s_end + (2 * spc - 1);
    r.need_hi = r.e1 - 1 + (long)REACH_CHIPS * spc > n_capture ? n_capture : r.e1 - 1 + (long)REACH_CHIPS * spc;
    return r;
}

// the meta word of a record: n_bits in the low half, DF above it
PSS_ADSB_HD inline uint32_t meta_of(int n_bits, int df) { return (uint32_t)n_bits | ((uint32_t)df << 16); }

}  // namespace pss_adsb

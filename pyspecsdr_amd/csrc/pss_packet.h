// pss_packet.h — the arithmetic of the packet-radio receiver (what the reference's command list hands to `rtl_fm -M fm -s 22050 | direwolf`,
// rtlcoms.json "Decode APRS"), stated ONCE for the kernels (pss_packet.hip: k_packet_front, k_packet_detect, k_packet_walk, k_packet_keep,
// k_packet_emit), the host twins (pss_h_packet_front, pss_h_packet_frames) and the stand-alone host check (tests/packet_host.cpp).  The
// reference has no such arithmetic, so this statement is the project's own (PARITY.md "Packet").  Every output follows from indices in the
// ROW, never from how the row was cut.
//
//   rate       26 400 S/s, SPB = 22 samples a bit (1200 bit/s).  Mark 1200 Hz: one cycle a window of 22; space 2200 Hz: 11 / 6 cycles.
//   tones      default_tones: t[0][u] = cos(2 pi u / 22), t[1][u] = sin(2 pi u / 22), t[2][u] = cos(2 pi u / 12), t[3][u] = sin(2 pi u / 12),
//              u = 0 .. 21, float64 from the host's libm: always a host table handed to the kernel and to the twin alike.
//   front      d[i] = pss_ais.h's discriminator (float32, d[0] = 0, no gain).  c_j = sum over u ascending of t[j][u] d[i - 11 + u], d = 0
//              outside the row: four float64 fma chains from +0.  E_m = c0 c0 + c1 c1; E_s = g (c2 c2 + c3 c3), g the caller's space_gain;
//              den = E_s + E_m; z[i] = (float)((E_s - E_m) / den), +0 where den == 0.  A NaN propagates.
//   candidate  a start s of a row of n samples exists where s - 22 >= 0 and s + 154 < n; its strobes are z[s + 22 k], k = -1 .. 7.
//              L[k] = z[s + 22 k] > 0 (a NaN is false); b[k] = (L[k] == L[k - 1]): the NRZI data bit, 1 for no change.
//              The start passes iff b[0 .. 7] is 01111110 and q >= q_min, q = the smallest |z[s + 22 k]| over k = -1 .. 7, taken as
//              a < q ? a : q in ascending order.  No preamble test: every flag of a TXDELAY run is a candidate, and all but the last end
//              in the walk as a frame of no bits.
//   walk       bits are appended as in pss_ais.h's walk (after a run of five ones the next bit, if 0, is dropped; if it is 1, one more
//              strobe is read: a change closes the frame, no change rejects; the payload runs six appended bits behind).  The strobes
//              move: p_7 = s + 154, p_k = p_(k-1) + 22 + a_(k-1), a_7 = 0.  After a strobe with L[k] != L[k - 1]: c = the smallest j in
//              (p_(k-1), p_k] with (z[j] > 0) == L[k]; e = 2 c - (p_(k-1) + p_k) - 1; a_k = +1 if e > 4, -1 if e < -4, else 0.  Without a
//              change a_k = 0 (so the closing look-ahead lies 22 behind its strobe).  Integer arithmetic on indices only.
//              Rejected where a strobe or the closing look-ahead lies outside the row, or where bit 2647 would be appended.  2646 appended
//              bits hold 528 dropped ones before the last run of five, and two more strobes follow it: k = 8 .. 3183 (LAST_K), each at most
//              23 behind the one before.  A start reads the samples [s - 22, s + REACH), REACH = 154 + 23 (LAST_K - 7) + 1 = 73 203.
//   check      accepted iff the payload length is a multiple of 8 in [136, 2640], the CRC-16/X.25 register over all the bits leaves 0xF0B8,
//              and the address field is well formed: the first byte with bit 0 set stands at index 7 m - 1 for some m in [2, 10], the frame
//              holds at least 7 m + 3 bytes, and bytes 0 .. 5 of each of the m addresses, shifted right by one, lie in A-Z, 0-9 or space.
//   one        an accepted A is dropped iff some accepted B of the same row has the same length and bytes, 0 < |s_B - s_A| < 22, and
//   record     q_B > q_A or (q_B = q_A and s_B < s_A).
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `-` is one IEEE operation; fma is the fused one.
#pragma once
#include <cmath>
#include <cstdint>

#include "pss_ais.h"

namespace pss_packet {

using pss_ais::crc_bit;
using pss_ais::disc;
using pss_ais::CRC_INIT;
using pss_ais::CRC_RESIDUE;

constexpr long RATE = 26400;
constexpr int SPB = 22;
constexpr int N_TONES = 4, WIN = SPB;            // the table: [4][22]
constexpr int WIN_BACK = 11, WIN_AHEAD = 10;     // z[i] reads d[i - 11 .. i + 10]
constexpr int MAX_BYTES = 330;                   // 70 address bytes, control, PID, 256 information bytes, 2 check bytes
constexpr int REC_BYTES = 332;                   // a record's bytes: MAX_BYTES up to a whole number of 32-bit words
constexpr int MIN_BITS = 136, MAX_BITS = 8 * MAX_BYTES;
constexpr int MAX_APPENDED = MAX_BITS + 6;       // the closing flag's 0 and five ones are appended before the walk knows them
constexpr int BACK = SPB;                        // 22: the samples in front of s that a start reads (k = -1)
constexpr int HEAD = 7 * SPB;                    // 154: the candidate test's last strobe (k = 7)
constexpr int LAST_K = 8 + MAX_APPENDED + (MAX_APPENDED / 5 - 1) + 2 - 1;   // 3183: the last strobe a walk can read
constexpr long REACH = HEAD + (long)(SPB + 1) * (LAST_K - 7) + 1;            // 73 203
constexpr int NEAR = SPB;                        // starts closer than this slice the same frame
constexpr int NUDGE_E = 4;                       // |e| above this moves the next strobe by one sample
constexpr int MIN_ADDR = 2, MAX_ADDR = 10;
static_assert(MAX_APPENDED == 2646 && LAST_K == 3183 && REACH == 73203, "the reach of a walk");
static_assert(REC_BYTES % 4 == 0 && REC_BYTES >= MAX_BYTES && REC_BYTES - MAX_BYTES < 4, "a record is whole words");
static_assert(7 * MAX_ADDR + 1 + 1 + 256 + 2 == MAX_BYTES && 8 * (7 * MIN_ADDR + 3) == MIN_BITS, "the frame's bounds");

// ---- plan -------------------------------------------------------------------------------------------------------------------------------------
// pss_ais.h's plan at this rate: decim = min(fs / 26 400, 204), up / down = 26 400 decim / fs reduced; false where they leave [1, 4096]
inline bool plan(long fs, int &D, int &up, int &down)
{
    long d = fs / RATE;
    if (d > pss_ais::MAX_DEFAULT_DECIM) d = pss_ais::MAX_DEFAULT_DECIM;
    long a = RATE * d, b = fs;
    long x = a, y = b;
    while (y) { const long t = x % y; x = y; y = t; }
    a /= x;
    b /= x;
    if (a < 1 || a > 4096 || b < 1 || b > 4096) return false;
    D = (int)d, up = (int)a, down = (int)b;
    return true;
}

// ---- tones ------------------------------------------------------------------------------------------------------------------------------------
inline void default_tones(double *t)
{
    for (int u = 0; u < WIN; u++) {
        t[0 * WIN + u] = cos(2.0 * M_PI * (double)u / 22.0);
        t[1 * WIN + u] = sin(2.0 * M_PI * (double)u / 22.0);
        t[2 * WIN + u] = cos(2.0 * M_PI * (double)u / 12.0);
        t[3 * WIN + u] = sin(2.0 * M_PI * (double)u / 12.0);
    }
}

// ---- front ------------------------------------------------------------------------------------------------------------------------------------
// z[i]: D(j) hands out d[j] for EVERY j in [i - 11, i + 10] (zero outside the row); t: the table [4][22]
template <class FD>
PSS_AIS_HD inline float tone_balance(FD D, const double *t, double g, long i)
{
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    for (int u = 0; u < WIN; u++) {
        const double d = (double)D(i - WIN_BACK + u);
        c0 = fma(t[0 * WIN + u], d, c0);
        c1 = fma(t[1 * WIN + u], d, c1);
        c2 = fma(t[2 * WIN + u], d, c2);
        c3 = fma(t[3 * WIN + u], d, c3);
    }
    const double em = c0 * c0 + c1 * c1;
    const double es = g * (c2 * c2 + c3 * c3);
    const double den = es + em;
    if (den == 0.0) return 0.0f;
    return (float)((es - em) / den);
}

// the input samples [lo, hi) of a row of n that the outputs [i_begin, i_end) read (i_begin < i_end)
struct Span { long lo, hi; };
PSS_AIS_HD inline Span front_span(long i_begin, long i_end, long n)
{
    Span r;
    r.lo = i_begin - WIN_BACK - 1 < 0 ? 0 : i_begin - WIN_BACK - 1;
    r.hi = i_end + WIN_AHEAD > n ? n : i_end + WIN_AHEAD;
    return r;
}

// ---- candidate --------------------------------------------------------------------------------------------------------------------------------
PSS_AIS_HD inline bool exists(long s, long n) { return s - BACK >= 0 && s + HEAD < n; }

// The flag test of the start s: Z(k) hands out the strobe z[s + 22 k], k = -1 .. 7.  q is set either way.
template <class FZ>
PSS_AIS_HD inline bool candidate(FZ Z, float q_min, float &q)
{
    float v = Z(-1);
    bool l0 = v > 0.0f;
    float m = fabsf(v);
    uint32_t bits = 0;   // b[k] at bit k
    for (int k = 0; k <= 7; k++) {
        v = Z(k);
        const bool l1 = v > 0.0f;
        if (l1 == l0) bits |= 1u << k;
        l0 = l1;
        const float a = fabsf(v);
        m = a < m ? a : m;
    }
    q = m;
    return bits == 0x7Eu && q >= q_min;
}

// the nudge behind a strobe at p (relative to s) whose level lv differs from the one at p_prev: Z(j) hands out z[s + j]
template <class FZ>
PSS_AIS_HD inline int nudge_of(FZ Z, long p_prev, long p, bool lv)
{
    // (p - p_prev is 21, 22 or 23.  Descending and without a way out, so that the reads do not wait for one another: a walk is a chain of
    // dependent reads, and an ascending scan that stops at c made it up to 22 reads longer at every change of level)
    long c = p;
    for (int u = SPB; u >= 1; u--) {
        const long j = p_prev + u;
        const float v = Z(j < p ? j : p);   // read whether or not it counts: a read under a condition waits for the one before it
        if (j < p && (v > 0.0f) == lv) c = j;
    }
    const long e = 2 * c - (p_prev + p) - 1;
    return e > NUDGE_E ? 1 : e < -NUDGE_E ? -1 : 0;
}

// The address rule, byte by byte: st < 0 while the field is open (-1), the index of its last byte once closed.  false: malformed.
PSS_AIS_HD inline bool address_byte(int j, uint32_t v, int &st)
{
    if (st >= 0) return true;
    const int in = j % 7;
    if (v & 1u) {
        if (in != 6 || j < 7 * MIN_ADDR - 1) return false;
        st = j;
        return true;
    }
    if (in == 6) return j < 7 * MAX_ADDR - 1;   // an 11th address would follow
    const uint32_t ch = v >> 1;
    return (ch >= 'A' && ch <= 'Z') || (ch >= '0' && ch <= '9') || ch == ' ';
}

// The walk of a start that passed: Z(j) hands out z[s + j] for j in [-22, end), end = n - s.  The payload's bits leave through W(w, word)
// as 32-bit words, bit p of the payload at bit p % 32 of word p / 32 (the payload runs six appended bits behind the walk, so the closing
// flag never reaches a word).  -> the payload's bytes, 0 where the start is rejected (words may have been written all the same).
template <class FZ, class FW>
PSS_AIS_HD inline int walk(FZ Z, long end, FW W)
{
    long p_prev = HEAD;
    bool prev = Z(p_prev) > 0.0f;
    int nudge = 0, run = 0, n_app = 0, n_pay = 0, addr = -1;
    bool addr_ok = true;   // judged with the check at the end, as the rule states it: a walk ends where its bits end, whatever they spell
    uint32_t recent = 0, word = 0, crc = CRC_INIT;
    for (;;) {
        const long p = p_prev + SPB + nudge;
        if (p >= end) return 0;
        const bool lv = Z(p) > 0.0f;
        const uint32_t b = lv == prev ? 1u : 0u;
        nudge = b ? 0 : nudge_of(Z, p_prev, p, lv);
        p_prev = p;
        prev = lv;
        if (run == 5) {
            if (!b) { run = 0; continue; }
            if (p + SPB >= end) return 0;
            const bool le = Z(p + SPB) > 0.0f;
            if (le == lv) return 0;   // seven ones
            break;
        }
        if (n_app == MAX_APPENDED) return 0;
        if (n_app >= 6) {
            const uint32_t old = (recent >> 5) & 1u;
            crc = crc_bit(crc, old);
            word |= old << (n_pay & 31);
            n_pay++;
            if ((n_pay & 7) == 0) addr_ok = address_byte(n_pay / 8 - 1, (word >> ((n_pay - 8) & 31)) & 0xFFu, addr) && addr_ok;
            if ((n_pay & 31) == 0) { W(n_pay / 32 - 1, word); word = 0; }
        }
        recent = ((recent << 1) | b) & 0x3Fu;
        n_app++;
        run = b ? run + 1 : 0;
    }
    if (n_pay < MIN_BITS || n_pay > MAX_BITS || (n_pay & 7) || crc != CRC_RESIDUE) return 0;
    if (!addr_ok || addr < 0 || n_pay / 8 < addr + 4) return 0;   // 7 m address bytes, control and the check bytes
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
// A call reports the starts [s_begin, s_end) of every row.  Their possible suppressors lie 21 starts to either side, clipped to the row: the
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

}  // namespace pss_packet

// pss_ook.h — the arithmetic of the OOK receiver (what the reference's command list hands to `rtl_433 -f {freq}M`, rtlcoms.json "Decode smart
// devices"), stated ONCE for the kernels (pss_ook.hip: k_ook_envelope, k_ook_levels, k_ook_detect, k_ook_heads, k_ook_list, k_ook_walk,
// k_ook_emit), the host twins (pss_h_ook_*) and the stand-alone host check (tests/ook_host.cpp).  The reference has no such arithmetic, so this
// statement is the project's own (PARITY.md "OOK").  Every output follows from indices in the ROW, never from how the row was cut.  Samples
// before index 0 of a row count as 0 + 0j.
//
//   magnitude  m[n] = fl32(fl32(re re) + fl32(im im)): two products and one sum, never contracted.
//   envelope   e[n] = fl32((m[n - P + 1] + ... + m[n], each widened to float64, added in that order from +0.0, one IEEE add a term) / P),
//              P in [1, 65].  No running sum.
//   levels     block b of a row is samples [4096 b, 4096 b + 4096); its mean is the float64 sum of its m, added in ascending order from
//              +0.0, divided by 4096.  (The thresholds hi, lo are the caller's: formats.ook_levels.)
//   state      sample n is decisive if e[n] >= hi (high) or e[n] < lo (low); a NaN is neither.  on(n) holds iff the last decisive sample
//              d <= n exists, is high, and n - d <= R, R in [0, 4096].  on(-1) is off, and so is every n past the row's end.  The state is a
//              function of e[n - R .. n], so of m[n - R - P + 1 .. n].
//   edges      a rise at n: on(n) && !on(n - 1); a fall at n: !on(n) && on(n - 1).  A pulse still on at the row's last sample falls at
//              n_row.  Edges alternate.  A pulse is a rise with the next fall of its row, its width their distance; its gap is the distance
//              from its fall to the next rise of the row.
//   messages   a rise at pos starts a message if no fall lies in [pos - gap_limit, pos): the row's first pulse, or a gap above gap_limit.
//              Edges at or past lim = pos + span are not read.  Pulse p = 0, 1, ... of the message has its rise at edge 2 p from the first
//              and its fall at the next.  With the rise of pulse p read: p = 1024 sets MANY and ends the message; a fall that is not read
//              sets LONG and ends it; otherwise the pulse belongs to the message, and the message goes on iff the next rise is read and
//              lies at most gap_limit behind the fall.  OPEN: the last pulse that belongs to the message falls at n_row.
//   slicers    integer rules on the n pulses that belong to the message (cls below; at most one class holds, the call refuses classes
//              less than 2 tol + 1 apart):
//              PWM  each pulse's width: short -> 1, long -> 0, sync -> nothing, else one odd symbol.
//              PPM  each pulse's gap but the last pulse's: short -> 0, long -> 1, sync -> nothing, else one odd symbol.
//              MC   the 2 n - 1 symbols pulse, gap, pulse, ..., pulse in time order: 1 half-bit within tol of short, 2 within tol of
//                   2 short; the first that is neither ends the list and counts as one odd.  h[0 .. H) the half-bit levels (pulse 1, gap
//                   0); pair i = (h[2 i + phase], h[2 i + phase + 1]) while inside H: (1, 0) -> 1, (0, 1) -> 0, equal -> one odd.
//              Bits go MSB first into bits[32]; the 257th and later are dropped (FULL); invert flips the bits kept.
//   records    reported iff n_bits >= min_bits and n_odd <= max_odd, in ascending (row, pos): bits, n_bits, row, pos, span (first rise to
//              the last fall of a pulse that belongs), meta = n | min(n_odd, 2047) << 11 | flags.
//   windows    a call reports the messages whose pos lies in [s_begin, s_end).  It lists the edges in [max(0, s_begin - gap_limit),
//              min(n_row + 1, s_end + span - 1)), and an edge at n reads m[n - 1 - R - (P - 1) .. n]: the buffer must hold
//              [max(0, s_begin - gap_limit - R - P), min(n_row, s_end + span)).
// Every unit that includes this header is compiled with -ffp-contract=off: each `*`, `+` and `/` is one IEEE operation.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PSS_OOK_HD __host__ __device__
#else
#define PSS_OOK_HD
#endif

namespace pss_ook {

constexpr int MAX_P = 65, MAX_R = 4096;
constexpr int BLOCK = 4096;                      // samples of a level block
constexpr long MAX_GAP = 1l << 20, MAX_SPAN = 1l << 24;
constexpr int MAX_WIDTH = 1 << 24;               // short, long, sync, tol
constexpr int MAX_PULSES = 1024, MAX_BITS = 256, BITS_BYTES = MAX_BITS / 8;
constexpr long NO_EDGE = 1l << 62;               // the position of an edge that does not exist: never read
enum Mode { PWM = 0, PPM = 1, MC = 2 };
constexpr int N_SHIFT_ODD = 11, MAX_ODD = 2047;
constexpr uint32_t F_OPEN = 1u << 22, F_LONG = 1u << 23, F_MANY = 1u << 24, F_FULL = 1u << 25;
static_assert(MAX_PULSES <= MAX_ODD && 2 * MAX_PULSES % 64 == 0, "meta's fields; the walk's 32 steps");

PSS_OOK_HD inline float magnitude(float re, float im)
{
    const float a = re * re, b = im * im;
    return a + b;
}

// M(k) hands out m[n - k], k = P - 1 .. 0
template <class FM>
PSS_OOK_HD inline float envelope(FM M, int P)
{
    double s = 0.0;
    for (int k = P - 1; k >= 0; k--) s = s + (double)M(k);
    return (float)(s / (double)P);
}

// 0: not decisive, 2: low, 3: high (bit 0 is the class)
PSS_OOK_HD inline int decisive(float e, float hi, float lo) { return e >= hi ? 3 : e < lo ? 2 : 0; }

// The scan's word of position q: 0 where q is not decisive, otherwise (q << 1 | class) + 1; the running maximum of the words up to q is the
// last decisive position and its class.
PSS_OOK_HD inline uint32_t scan_word(int q, int code) { return code ? (((uint32_t)q << 1) | (uint32_t)(code & 1)) + 1u : 0u; }
PSS_OOK_HD inline bool state(uint32_t last, int q, int R) { return last != 0 && ((last - 1u) & 1u) && q - (int)((last - 1u) >> 1) <= R; }

// ---- slicers ----------------------------------------------------------------------------------------------------------------------------------
struct Slicer { int mode, w_short, w_long, w_sync, tol, phase, invert, min_bits, max_odd; };
enum Cls { C_SHORT = 0, C_LONG = 1, C_SYNC = 2, C_ODD = 3 };
PSS_OOK_HD inline bool near_to(long w, long c, long tol) { return (w > c ? w - c : c - w) <= tol; }
PSS_OOK_HD inline int cls(long w, const Slicer &s)
{
    if (near_to(w, s.w_short, s.tol)) return C_SHORT;
    if (near_to(w, s.w_long, s.tol)) return C_LONG;
    if (s.w_sync != 0 && near_to(w, s.w_sync, s.tol)) return C_SYNC;
    return C_ODD;
}
// the half-bits of a Manchester symbol of length w: 1, 2, or 0 where it is neither
PSS_OOK_HD inline int halves(long w, const Slicer &s) { return near_to(w, s.w_short, s.tol) ? 1 : near_to(w, 2l * s.w_short, s.tol) ? 2 : 0; }

PSS_OOK_HD inline uint32_t meta_of(int n, long n_odd, uint32_t flags) { return (uint32_t)n | (uint32_t)(n_odd < MAX_ODD ? n_odd : MAX_ODD) << N_SHIFT_ODD | flags; }
PSS_OOK_HD inline bool reported(int n_bits, long n_odd, const Slicer &s) { return n_bits >= s.min_bits && n_odd <= s.max_odd; }

// nullptr, or what is wrong with the slicer
inline const char *slicer_refusal(const Slicer &s)
{
    if (s.mode != PWM && s.mode != PPM && s.mode != MC) return "mode is none of PSS_OOK_PWM, PSS_OOK_PPM, PSS_OOK_MC";
    if (s.tol < 0 || s.tol > MAX_WIDTH) return "tol outside [0, 2^24]";
    if (s.w_short < 1 || s.w_short > MAX_WIDTH) return "short outside [1, 2^24]";
    if (s.phase != 0 && s.phase != 1) return "phase outside {0, 1}";
    if (s.invert != 0 && s.invert != 1) return "invert outside {0, 1}";
    if (s.min_bits < 0 || s.min_bits > MAX_BITS) return "min_bits outside [0, 256]";
    if (s.max_odd < 0 || s.max_odd > MAX_ODD) return "max_odd outside [0, 2047]";
    auto apart = [&](long a, long b) { return (a > b ? a - b : b - a) > 2l * s.tol; };
    if (s.mode == MC) return apart(s.w_short, 2l * s.w_short) ? nullptr : "short and 2 short are not more than 2 tol apart";
    if (s.w_long < 1 || s.w_long > MAX_WIDTH) return "long outside [1, 2^24]";
    if (s.w_sync < 0 || s.w_sync > MAX_WIDTH) return "sync outside [0, 2^24]";
    if (!apart(s.w_short, s.w_long) || (s.w_sync != 0 && (!apart(s.w_short, s.w_sync) || !apart(s.w_long, s.w_sync))))
        return "short, long and sync are not more than 2 tol apart";
    return nullptr;
}

// ---- one message, sequentially: the host twin's walk (the kernel's is k_ook_walk: 64 edges a step) -------------------------------------------
struct Message { uint8_t bits[BITS_BYTES]; int n_bits, n_pulses; long n_odd, span; uint32_t flags; };

// E(a): the position of edge a of the row's list counted from the message's first rise (a = 0), NO_EDGE where the row has no such edge
template <class FE>
inline Message walk(FE E, long pos, long span, long gap_limit, long n_row, const Slicer &s)
{
    Message r = {};
    const long lim = pos + span;
    int n = 0;
    for (long p = 0;; p++) {
        if (p == MAX_PULSES) { r.flags |= F_MANY; break; }
        if (!(E(2 * p + 1) < lim)) { r.flags |= F_LONG; break; }
        n++;
        const long rise = E(2 * p + 2);
        if (!(rise < lim) || rise - E(2 * p + 1) > gap_limit) break;
    }
    r.n_pulses = n;
    if (n > 0) {
        r.span = E(2 * n - 1) - pos;
        if (E(2 * n - 1) == n_row) r.flags |= F_OPEN;
    }
    long total = 0;
    auto put = [&](int bit) {
        if (total < MAX_BITS) {
            if (bit ^ s.invert) r.bits[total >> 3] |= (uint8_t)(0x80u >> (total & 7));
        } else r.flags |= F_FULL;
        total++;
    };
    if (s.mode == MC) {
        // the half-bit levels, written out
        long H = 0;
        uint8_t h[4 * MAX_PULSES];
        for (long q = 0; q < 2l * n - 1; q++) {
            const int k = halves(E(q + 1) - E(q), s);
            if (!k) { r.n_odd++; break; }
            for (int u = 0; u < k; u++) h[H++] = (uint8_t)(1 - (q & 1));
        }
        for (long i = 0; 2 * i + s.phase + 1 < H; i++) {
            const int a = h[2 * i + s.phase], b = h[2 * i + s.phase + 1];
            if (a == b) r.n_odd++;
            else put(a);
        }
    } else {
        const long cnt = s.mode == PWM ? n : n - 1;
        for (long p = 0; p < cnt; p++) {
            const long w = s.mode == PWM ? E(2 * p + 1) - E(2 * p) : E(2 * p + 2) - E(2 * p + 1);
            const int c = cls(w, s);
            if (c == C_ODD) r.n_odd++;
            else if (c != C_SYNC) put(s.mode == PWM ? (c == C_SHORT) : (c == C_LONG));
        }
    }
    r.n_bits = (int)(total < MAX_BITS ? total : MAX_BITS);
    return r;
}

// ---- windows ----------------------------------------------------------------------------------------------------------------------------------
PSS_OOK_HD inline long halo_before(int P, int R, long gap_limit) { return gap_limit + R + P; }
PSS_OOK_HD inline long halo_after(long span) { return span; }
// the edges [e0, e1) a call lists, and the samples [need_lo, need_hi) it must be given
struct Reach { long e0, e1, need_lo, need_hi; };
PSS_OOK_HD inline Reach reach_of(long s_begin, long s_end, long n_row, int P, int R, long gap_limit, long span)
{
    Reach r;
    r.e0 = s_begin - gap_limit < 0 ? 0 : s_begin - gap_limit;
    r.e1 = s_end + span - 1 > n_row + 1 ? n_row + 1 : s_end + span - 1;
    r.need_lo = s_begin - halo_before(P, R, gap_limit) < 0 ? 0 : s_begin - halo_before(P, R, gap_limit);
    r.need_hi = s_end + halo_after(span) > n_row ? n_row : s_end + halo_after(span);
    return r;
}

// ---- a row's edges, sequentially: the host twin's detect --------------------------------------------------------------------------------------
// Mg(i) hands out m[i] of the row for i in [0, n_row) (the caller's zero outside its buffer is never asked for: the reach is checked first);
// edge(n, rise) is called for every edge in [e0, e1), ascending.
template <class FMg, class FEdge>
inline void row_edges(FMg Mg, long n_row, long e0, long e1, int P, float hi, float lo, int R, FEdge edge)
{
    long c0 = e0 - 1 - R;
    if (c0 < 0) c0 = 0;
    long last = -1;       // the last decisive sample seen
    bool last_high = false, prev = false;   // prev: on(n - 1)
    for (long n = c0; n < e1; n++) {
        bool on = false;
        if (n < n_row) {
            const float e = envelope([&](int k) { return n - k >= 0 ? Mg(n - k) : 0.0f; }, P);
            const int code = decisive(e, hi, lo);
            if (code) { last = n; last_high = code & 1; }
            on = last >= 0 && last_high && n - last <= R;
        }
        if (n >= e0 && on != prev) edge(n, on);
        prev = on;
    }
}

}  // namespace pss_ook

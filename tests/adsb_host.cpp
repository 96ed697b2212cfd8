// adsb_host.cpp — pss_adsb.h with the host compiler alone (the header must not need HIP), built with -fsanitize=address,undefined and run as
// a program of its own by tests/test_adsb_golden.py.  It walks the index arithmetic at the capture's ends and the window edges: every
// accessor checks its index against the capture AND against what reach_of says a window's call may read, the remainder is held against a
// division written out bit by bit, and the one-record rule against hand-made pairs and, through pss_starts.h's keep_starts (the neighbour
// loop of pss_h_adsb_frames), against hand-made lists in heap vectors of exactly their size.  Prints "adsb_host: ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pss_adsb.h"
#include "pss_starts.h"

using namespace pss_adsb;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            printf("adsb_host: FAILED %s (line %d)\n", #c, __LINE__);         \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static const uint8_t IDENT[14] = {0x8D, 0x48, 0x40, 0xD6, 0x20, 0x2C, 0xC3, 0x71, 0xC3, 0x2C, 0xE0, 0x57, 0x60, 0x98};
static const uint8_t ALL_CALL[14] = {0x5D, 0x48, 0x40, 0xD6, 0xF8, 0x74, 0x0F};
static const uint8_t ALT_REPLY[14] = {0x20, 0x00, 0x0B, 0x38, 0xAB, 0x0D, 0x0D};

// a frame at sample p of a zero capture of n samples, spc samples a chip
static std::vector<float> capture(long n, int spc, const uint8_t *msg, int n_bits, long p)
{
    std::vector<float> x(2 * (size_t)n, 0.0f);
    auto pulse = [&](int chip) {
        for (int k = 0; k < spc; k++) {
            const long i = p + (long)spc * chip + k;
            CHECK(i >= 0 && i < n);
            x[2 * (size_t)i] = 1.0f;
        }
    };
    for (int c : {0, 2, 7, 9}) pulse(c);
    for (int i = 0; i < n_bits; i++) pulse(16 + 2 * i + (((msg[i >> 3] >> (7 - (i & 7))) & 1) ? 0 : 1));
    return x;
}

// every start of a window through `candidate`, the accessor held to the capture and to the window's reach -> the accepted starts inside
// the window (neighbouring starts of one frame count one each: the one-record rule is not applied here); *want is set to -1 where it is one
static int count_window(const std::vector<float> &x, long n, int spc, long s_begin, long s_end, const uint32_t *icao, int n_icao, long *want)
{
    const Reach r = reach_of(s_begin, s_end, spc, n);
    CHECK(r.e0 >= 0 && r.e0 <= s_begin && r.e1 >= s_end && r.e1 <= n && r.need_hi <= n && r.need_hi >= r.e1);
    int found = 0;
    for (long s = r.e0; s < r.e1; s++) {
        uint8_t msg[MSG_BYTES];
        int n_bits;
        float hi;
        auto M = [&](long i) {
            CHECK(i >= 0 && i < n);
            CHECK(i >= r.e0 && i < r.need_hi);      // nothing outside what the caller was told to bring
            CHECK(i >= s && i < s + span_of(LONG_BITS, spc));
            return mag(x[2 * (size_t)i], x[2 * (size_t)i + 1]);
        };
        if (candidate(M, s, n, spc, 2.0f, icao, n_icao, msg, n_bits, hi)) {
            CHECK(fits(s, n_bits, spc, n));
            if (s >= s_begin && s < s_end) {
                found++;
                if (s == *want) *want = -1;   // the start the caller asked about is among them
            }
        }
    }
    return found;
}

static void test_crc()
{
    CHECK(crc24(IDENT, 112) == 0 && crc24(ALL_CALL, 56) == 0 && crc24(ALT_REPLY, 56) == 0x4840D6);
    // the division, one bit of the message at a time against a 25-bit register
    uint64_t r = 0;
    for (int i = 0; i < 112; i++) {
        r = (r << 1) | ((IDENT[i >> 3] >> (7 - (i & 7))) & 1);
        if (r >> 24) r ^= GENERATOR;
    }
    CHECK(r == 0);
    // the table the kernel folds: the remainder of a message is the xor of the powers of its set bits, at either length
    constexpr Powers P;
    for (int n_bits : {56, 112}) {
        const uint8_t *msg = n_bits == 56 ? ALT_REPLY : IDENT;
        uint32_t x = 0;
        for (int i = 0; i < n_bits; i++) {
            if ((msg[i >> 3] >> (7 - (i & 7))) & 1) x ^= P.t[n_bits - 1 - i];
            uint8_t one[14] = {};
            one[i >> 3] = (uint8_t)(0x80 >> (i & 7));
            CHECK(crc24(one, n_bits) == P.t[n_bits - 1 - i]);
        }
        CHECK(x == crc24(msg, n_bits));
    }
    uint8_t m[14];
    for (int i = 0; i < 112; i++) {
        memcpy(m, IDENT, 14);
        m[i >> 3] ^= (uint8_t)(0x80 >> (i & 7));
        CHECK(crc24(m, 112) != 0);
    }
    const uint32_t list[5] = {1, 7, 0x4840D6, 0x4840D7, 0xFFFFFF};
    for (int n = 0; n <= 5; n++)
        for (uint32_t a : {0u, 1u, 2u, 7u, 0x4840D6u, 0x4840D7u, 0xFFFFFFu}) {
            bool in = false;
            for (int k = 0; k < n; k++) in |= list[k] == a;
            CHECK(listed(list, n, a) == in);
        }
    CHECK(accepted(IDENT, 112, nullptr, 0) && accepted(ALL_CALL, 56, nullptr, 0) && !accepted(ALT_REPLY, 56, nullptr, 0));
    CHECK(accepted(ALT_REPLY, 56, list, 5) && !accepted(ALT_REPLY, 56, list, 2));
}

static void test_edges()
{
    const uint32_t addr[1] = {0x4840D6};
    for (int spc = 1; spc <= MAX_SPC; spc++) {
        const long span = span_of(LONG_BITS, spc), half = span_of(SHORT_BITS, spc);
        CHECK(span == 240l * spc && half == 128l * spc);
        long first = -1;
        // at sample 0 and ending on the last sample
        for (long p : {0l, 5l}) {
            const long n = p + span;
            auto x = capture(n, spc, IDENT, 112, p);
            CHECK(count_window(x, n, spc, 0, n, nullptr, 0, &(first = p)) >= 1 && first == -1);
            // one sample shorter: that start is gone (an earlier start of wide chips may still hold the frame)
            std::vector<float> y(x.begin(), x.end() - 2);
            count_window(y, n - 1, spc, 0, n - 1, nullptr, 0, &(first = p));
            CHECK(first == p);
        }
        // a short frame fits where a long one would not
        {
            const long p = 3, n = p + half;
            auto x = capture(n, spc, ALL_CALL, 56, p);
            CHECK(count_window(x, n, spc, 0, n, nullptr, 0, &(first = p)) >= 1 && first == -1);
            auto z = capture(n, spc, ALT_REPLY, 56, p);
            CHECK(count_window(z, n, spc, 0, n, nullptr, 0, &(first = -2)) == 0);
            CHECK(count_window(z, n, spc, 0, n, addr, 1, &(first = p)) >= 1 && first == -1);
        }
        // windows that cut the frame: every start is reported by exactly the window that holds it
        {
            const long p = 2l * spc + 1, n = p + span + 9;
            auto x = capture(n, spc, IDENT, 112, p);
            const int whole = count_window(x, n, spc, 0, n, nullptr, 0, &(first = p));
            CHECK(whole >= 1 && first == -1);
            for (long cut : {p - 1, p, p + 1, p + 3l * spc, p + 100l * spc, n - 1}) {
                long f2 = -2;
                CHECK(count_window(x, n, spc, 0, cut, nullptr, 0, &f2) + count_window(x, n, spc, cut, n, nullptr, 0, &f2) == whole);
            }
            CHECK(count_window(x, n, spc, p, p, nullptr, 0, &(first = -2)) == 0);   // an empty window
        }
        // captures too short for any frame
        for (long n : {0l, 1l, half - 1}) {
            std::vector<float> x(2 * (size_t)n + 2, 1.0f);
            CHECK(count_window(x, n, spc, 0, n, nullptr, 0, &(first = -2)) == 0);
        }
    }
}

static void test_rules()
{
    // the preamble: strict, and a NaN anywhere fails it
    float e[16] = {};
    for (int c : {0, 2, 7, 9}) e[c] = 4.0f;
    for (int c = 0; c < 16; c++)
        if (e[c] == 0.0f) e[c] = 2.0f;
    float hi;
    CHECK(!preamble(e, 2.0f, hi) && hi == 4.0f);          // hi == ratio lo exactly
    e[7] = 4.0000005f;
    CHECK(!preamble(e, 2.0f, hi) && hi == 4.0f);          // the minimum decides
    for (int c : {0, 2, 9}) e[c] = 4.0000005f;
    CHECK(preamble(e, 2.0f, hi));
    for (int c = 0; c < 16; c++) {
        float f[16];
        memcpy(f, e, sizeof(f));
        f[c] = NAN;
        CHECK(!preamble(f, 2.0f, hi));
        CHECK(!preamble(f, 0.0f, hi));
    }
    e[3] = INFINITY;
    CHECK(!preamble(e, 2.0f, hi) && !preamble(e, 0.0f, hi));   // 0 * inf is a NaN
    // one record per frame
    CHECK(drops(true, 10, 2.0f, 11, 1.0f, 2) && !drops(true, 10, 1.0f, 11, 2.0f, 2));
    CHECK(drops(true, 10, 1.0f, 11, 1.0f, 2) && !drops(true, 11, 1.0f, 10, 1.0f, 2));   // a tie: the earlier start stays
    CHECK(!drops(true, 10, 2.0f, 14, 1.0f, 2) && drops(true, 10, 2.0f, 13, 1.0f, 2) && !drops(false, 10, 2.0f, 11, 1.0f, 2));
    CHECK(!drops(true, 10, 2.0f, 10, 1.0f, 2));
    CHECK(plan(2e6) == 1 && plan(16e6) == 8 && plan(10e6) == 5 && plan(2.4e6) == 0 && plan(18e6) == 0 && plan(1e6) == 0 && plan(0.0) == 0);
}

// keep_starts over an ascending list of starts that all carry the same message, spc samples a chip -> the starts it emits, in its order
struct Start { long s; float hi; };
static std::vector<long> kept(const std::vector<Start> &list, long s_begin, long s_end, int spc)
{
    const std::vector<Start> heap(list.begin(), list.end());   // exactly list.size() records: a read past either end is the sanitizer's
    std::vector<long> out;
    pss_starts::keep_starts(
        heap.data(), heap.size(), s_begin, s_end, 2l * spc, [&](const Start &b, const Start &a) { return drops(true, b.s, b.hi, a.s, a.hi, spc); },
        [&](const Start &a) { out.push_back(a.s); });
    return out;
}

static void test_keep()
{
    using L = std::vector<long>;
    const int spc = 2;   // near = 4
    CHECK(kept({}, 0, 100, spc) == L{});
    CHECK(kept({{10, 1.0f}}, 0, 100, spc) == L{10} && kept({{10, 1.0f}}, 10, 11, spc) == L{10});
    CHECK(kept({{10, 1.0f}}, 11, 100, spc) == L{} && kept({{10, 1.0f}}, 0, 10, spc) == L{});
    // exactly near apart: no neighbours, both stay; near - 1 apart: the weaker one goes, whichever side it is on
    CHECK((kept({{10, 2.0f}, {14, 1.0f}}, 0, 100, spc) == L{10, 14}) && (kept({{10, 1.0f}, {14, 2.0f}}, 0, 100, spc) == L{10, 14}));
    CHECK(kept({{10, 2.0f}, {13, 1.0f}}, 0, 100, spc) == L{10} && kept({{10, 1.0f}, {13, 2.0f}}, 0, 100, spc) == L{13});
    // the stronger neighbour just outside the window still drops the one inside, and is not emitted itself
    CHECK(kept({{9, 2.0f}, {10, 1.0f}}, 10, 100, spc) == L{} && kept({{9, 1.0f}, {10, 2.0f}}, 0, 10, spc) == L{});
    CHECK(kept({{9, 1.0f}, {10, 2.0f}}, 10, 100, spc) == L{10} && kept({{9, 2.0f}, {10, 1.0f}}, 0, 10, spc) == L{9});
    // equal scores: the earlier start stays
    CHECK(kept({{10, 1.0f}, {11, 1.0f}}, 0, 100, spc) == L{10} && kept({{10, 1.0f}, {11, 1.0f}, {12, 1.0f}, {13, 1.0f}, {14, 1.0f}}, 0, 100, spc) == L{10});
    // a chain: each start is judged against every accepted neighbour, whatever that neighbour's own fate (12 goes to 14, and still drops 10)
    CHECK((kept({{10, 1.0f}, {12, 2.0f}, {14, 3.0f}, {30, 1.0f}}, 0, 100, spc) == L{14, 30}));
}

int main()
{
    test_crc();
    test_edges();
    test_rules();
    test_keep();
    printf("adsb_host: ok\n");
    return 0;
}

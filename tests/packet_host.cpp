// packet_host.cpp — pss_packet.h with the host compiler alone (no HIP), as a program of its own under AddressSanitizer and UBSan
// (tests/test_packet_golden.py builds and runs it).  Every row lives in a heap buffer of exactly its size and is read through at(), so a
// strobe, a look-ahead or a step of the clock tracking's scan outside the row ends the program.  It covers the reach of a walk (LAST_K and
// REACH, strobe by strobe), the nudge at e = +-3, +-4, +-5, +-6, every way the walk and the check refuse a start, the one-record rule
// through pss_starts.h's keep_starts, and the windows.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pss_packet.h"
#include "pss_starts.h"

using namespace pss_packet;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("packet_host: line %d: %s\n", __LINE__, #c);        \
            fails++;                                                    \
        }                                                               \
    } while (0)

using Bytes = std::vector<uint8_t>;
using Bits = std::vector<int>;

static Bits wire(const Bytes &bytes)
{
    Bits b;
    for (uint8_t v : bytes)
        for (int k = 0; k < 8; k++) b.push_back((v >> k) & 1);
    return b;
}

static Bits stuffed(const Bits &in)
{
    Bits out;
    int run = 0;
    for (int b : in) {
        out.push_back(b);
        run = b ? run + 1 : 0;
        if (run == 5) { out.push_back(0); run = 0; }
    }
    return out;
}

// flag, the bits between, flag
static Bits burst(const Bits &mid)
{
    const int flag[8] = {0, 1, 1, 1, 1, 1, 1, 0};
    Bits out(flag, flag + 8);
    out.insert(out.end(), mid.begin(), mid.end());
    out.insert(out.end(), flag, flag + 8);
    return out;
}

static Bytes with_crc(Bytes body)
{
    const uint32_t c = pss_ais::crc_reg(body.data(), (long)body.size()) ^ 0xFFFFu;
    body.push_back((uint8_t)(c & 0xFF));
    body.push_back((uint8_t)(c >> 8));
    return body;
}

static void put_address(Bytes &f, const char *call, int ssid, bool last)
{
    for (int j = 0; j < 6; j++) f.push_back((uint8_t)((j < (int)strlen(call) ? call[j] : ' ') << 1));
    f.push_back((uint8_t)(0x60 | (ssid << 1) | (last ? 1 : 0)));
}

// m addresses, control, PID and n_info bytes
static Bytes body_of(int m, int n_info)
{
    Bytes f;
    for (int a = 0; a < m; a++) put_address(f, a == 0 ? "APRS" : a == 1 ? "N0CALL" : "WIDE2", a, a == m - 1);
    f.push_back(0x03);
    f.push_back(0xF0);
    for (int i = 0; i < n_info; i++) f.push_back((uint8_t)(37 * i + 11));
    return f;
}

// a row of n samples: the level in front of the burst over one cell, then bit k over the 22 samples around its centre at + 22 k
static std::vector<float> row_of(const Bits &bits, long at, long n)
{
    std::vector<float> z((size_t)n, 0.0f);
    float level = -1.0f;
    for (long k = -1; k < (long)bits.size(); k++) {
        if (k >= 0) level = bits[(size_t)k] ? level : -level;
        for (long j = at + SPB * k - 11; j < at + SPB * k + 11; j++)
            if (j >= 0 && j < n) z[(size_t)j] = level;
    }
    return z;
}

struct Rec { long s; int len; float q; uint8_t msg[REC_BYTES]; };
// one start of the row on one thread
static bool one_start(const std::vector<float> &z, long s, float q_min, Rec &c)
{
    const long n = (long)z.size();
    if (!exists(s, n)) return false;
    if (!candidate([&](int k) { return z.at((size_t)(s + SPB * k)); }, q_min, c.q)) return false;
    uint32_t words[REC_BYTES / 4] = {};
    c.s = s;
    c.len = walk([&](long j) { return z.at((size_t)(s + j)); }, n - s, [&](int i, uint32_t v) { words[i] = v; });
    for (int j = 0; j < REC_BYTES; j++) c.msg[j] = (uint8_t)(words[j / 4] >> (8 * (j % 4)));
    return c.len > 0;
}

// the centred start of the row's first flag: the frame's bytes where it is accepted, empty otherwise
static Bytes centred(const Bits &mid, long cut = 0)
{
    const Bits bits = burst(mid);
    const long n = BACK + SPB * (long)(bits.size() - 1) + 1 - cut;   // the row ends on the closing look-ahead: the closing flag's last bit
    const std::vector<float> z = row_of(bits, BACK, n);
    Rec c;
    if (!one_start(z, BACK, 0.0f, c)) return {};
    return Bytes(c.msg, c.msg + c.len);
}

struct Start { long s; float q; };
static std::vector<long> kept(const std::vector<Start> &list, long s_begin, long s_end)
{
    const std::vector<Start> heap(list.begin(), list.end());
    std::vector<long> out;
    pss_starts::keep_starts(
        heap.data(), heap.size(), s_begin, s_end, NEAR, [](const Start &b, const Start &a) { return drops(true, b.s, b.q, a.s, a.q); },
        [&](const Start &a) { out.push_back(a.s); });
    return out;
}

int main()
{
    static_assert(SPB == 22 && BACK == 22 && HEAD == 154 && NEAR == 22 && MIN_BITS == 136 && MAX_BYTES == 330 && MAX_APPENDED == 2646, "the constants");
    static_assert(LAST_K == 3183 && REACH == 154 + 23l * (3183 - 7) + 1 && REACH == 73203, "the reach");
    // the plan
    int D, up, down;
    CHECK(plan(2400000, D, up, down) && D == 90 && up == 99 && down == 100);
    CHECK(plan(240000, D, up, down) && D == 9 && up == 99 && down == 100);
    CHECK(plan(264000, D, up, down) && D == 10 && up == 1 && down == 1);
    CHECK(plan(26400, D, up, down) && D == 1 && up == 1 && down == 1);
    CHECK(plan(250000, D, up, down) && D == 9 && up == 594 && down == 625);
    CHECK(!plan(1000003, D, up, down));
    // the tones and the front: a mark tone reads -1, a space tone +1, silence +0, a NaN a NaN; space_gain moves the balance
    {
        double t[N_TONES * WIN];
        default_tones(t);
        for (int u = 0; u < WIN; u++)
            CHECK(t[u] == cos(2.0 * M_PI * u / 22.0) && t[WIN + u] == sin(2.0 * M_PI * u / 22.0) && t[2 * WIN + u] == cos(2.0 * M_PI * u / 12.0) &&
                  t[3 * WIN + u] == sin(2.0 * M_PI * u / 12.0));
        const long n = 200;
        std::vector<float> mark((size_t)n), space((size_t)n), both((size_t)n), none((size_t)n, 0.0f);
        for (long i = 0; i < n; i++) {
            mark[(size_t)i] = (float)(0.7 * sin(2.0 * M_PI * 1200.0 * i / 26400.0));
            space[(size_t)i] = (float)(0.7 * sin(2.0 * M_PI * 2200.0 * i / 26400.0 + 0.4));
            both[(size_t)i] = mark[(size_t)i] + space[(size_t)i];
        }
        auto Z = [&](const std::vector<float> &d, double g, long i) {
            return tone_balance([&](long j) { return j >= 0 && j < n ? d.at((size_t)j) : 0.0f; }, t, g, i);
        };
        float mark_max = -1.0f, space_min = 1.0f;
        bool moved = true, zero = true;
        for (long i = 11; i < n - 10; i++) {
            mark_max = fmaxf(mark_max, Z(mark, 1.0, i));
            space_min = fminf(space_min, Z(space, 1.0, i));
            moved = moved && Z(both, 4.0, i) > Z(both, 1.0, i) && Z(both, 0.25, i) < Z(both, 1.0, i);
        }
        for (long i = 0; i < n; i++) {
            const float v = Z(none, 1.0, i);
            zero = zero && v == 0.0f && !std::signbit(v);
        }
        printf("packet_host: a mark tone reads at most %.4f, a space tone at least %.4f\n", mark_max, space_min);
        // a window of 22 holds one cycle of 1200 Hz exactly and 11 / 6 of 2200 Hz: the other correlator's leakage stays below a third of the energy
        CHECK(mark_max < -0.5f && space_min > 0.5f && moved && zero);
        both[50] = NAN;
        CHECK(std::isnan(Z(both, 1.0, 50 - 10)) && std::isnan(Z(both, 1.0, 50 + 11)) && !std::isnan(Z(both, 1.0, 50 - 11)) && !std::isnan(Z(both, 1.0, 50 + 12)));
        const Span a = front_span(100, 200, 1000), b = front_span(0, 1000, 1000), c = front_span(5, 6, 1000);
        CHECK(a.lo == 88 && a.hi == 210 && b.lo == 0 && b.hi == 1000 && c.lo == 0 && c.hi == 16);
    }
    // the nudge: p - p_prev = 22 gives odd e, 23 even e
    {
        auto nudge = [](long p_prev, long p, long c, bool lv) {
            std::vector<float> z((size_t)(p + 1));
            for (long j = 0; j <= p; j++) z[(size_t)j] = (j >= c) == lv ? 1.0f : -1.0f;
            return nudge_of([&](long j) { return z.at((size_t)j); }, p_prev, p, lv);
        };
        for (bool lv : {false, true}) {
            CHECK(nudge(100, 122, 114, lv) == 1 && nudge(100, 122, 113, lv) == 0 && nudge(100, 122, 109, lv) == -1 && nudge(100, 122, 110, lv) == 0);   // e = 5, 3, -5, -3
            CHECK(nudge(100, 123, 114, lv) == 0 && nudge(100, 123, 115, lv) == 1 && nudge(100, 123, 110, lv) == 0 && nudge(100, 123, 109, lv) == -1);   // e = 4, 6, -4, -6
            CHECK(nudge(100, 122, 101, lv) == -1 && nudge(100, 122, 122, lv) == 1 && nudge(100, 121, 111, lv) == 0);                                   // the ends of the scan; e = 0
        }
    }
    // frames: the shortest and the longest, the row ending on the closing look-ahead; one sample shorter: nothing
    for (int pick = 0; pick < 3; pick++) {
        Bytes body = pick == 0 ? body_of(2, 0) : pick == 1 ? body_of(3, 40) : body_of(10, 0);
        if (pick == 0) body.pop_back();                                  // two addresses and control: 15 bytes
        if (pick == 2) body.insert(body.end(), 256, (uint8_t)0xFF);      // every fifth bit of the information field stuffed
        const Bytes frame = with_crc(body);
        CHECK(pick != 0 || frame.size() == 17);
        CHECK(pick != 2 || frame.size() == 330);
        CHECK(centred(stuffed(wire(frame))) == frame);
        CHECK(centred(stuffed(wire(frame)), 1).empty());
        // every start of the row: the 22 of the cell pass the flag test and, the tracking pulling them in, read the same bytes
        const Bits bits = burst(stuffed(wire(frame)));
        const std::vector<float> z = row_of(bits, BACK + 11, BACK + 11 + SPB * (long)bits.size() + 40);
        int n_ok = 0;
        for (long s = 0; s < (long)z.size(); s++) {
            Rec c;
            if (!one_start(z, s, 0.0f, c)) continue;
            n_ok++;
            CHECK(s >= BACK && s < BACK + SPB && c.len == (int)frame.size() && memcmp(c.msg, frame.data(), frame.size()) == 0 && c.q == 1.0f);
            for (int j = c.len; j < REC_BYTES; j++) CHECK(c.msg[j] == 0);
        }
        CHECK(n_ok == SPB);
    }
    // what the walk and the check refuse
    {
        const Bytes good = with_crc(body_of(2, 10));
        CHECK(centred(stuffed(wire(good))) == good);
        Bytes bad = good;
        bad[16] ^= 0x10;
        CHECK(centred(stuffed(wire(bad))).empty());                                   // the check sequence
        Bits odd = stuffed(wire(good));
        odd.insert(odd.begin() + 120, 0);
        CHECK(centred(odd).empty());                                                  // no whole number of bytes
        Bytes two = body_of(2, 0);
        two.resize(14);
        CHECK(centred(stuffed(wire(with_crc(two)))).empty());                         // 16 bytes: below 136 bits
        Bytes big = body_of(10, 0);
        big.insert(big.end(), 257, (uint8_t)0x55);
        CHECK(with_crc(big).size() == 331 && centred(stuffed(wire(with_crc(big)))).empty());   // bit 2647
        Bits seven = stuffed(wire(good));
        seven.insert(seven.begin() + 60, {0, 1, 1, 1, 1, 1, 1, 1, 0});
        CHECK(centred(seven).empty());                                                // seven ones
        Bytes lower = body_of(2, 10);
        lower[8] = (uint8_t)('n' << 1);
        CHECK(centred(stuffed(wire(with_crc(lower)))).empty());                       // a character outside A-Z, 0-9, space
        Bytes ext = body_of(2, 10);
        ext[3] |= 1;
        CHECK(centred(stuffed(wire(with_crc(ext)))).empty());                         // the extension bit inside an address
        CHECK(centred(stuffed(wire(with_crc(body_of(1, 12))))).empty());              // one address
        Bytes eleven = body_of(11, 4);
        CHECK(centred(stuffed(wire(with_crc(eleven)))).empty());                      // eleven addresses
        Bytes none = body_of(2, 10);
        none[13] &= 0xFE;
        for (size_t j = 14; j < none.size(); j++) none[j] &= 0xFE;
        CHECK(centred(stuffed(wire(with_crc(none)))).size() == 0);                    // no extension bit at all (the check bytes may carry one: not at 7 m - 1 with the rest in place)
        Bytes three;                                                                  // 7 m + 2 bytes cannot be told from the length rule at m = 2 (136 bits); at m = 3 they can
        put_address(three, "APRS", 0, false);
        put_address(three, "N0CALL", 1, false);
        put_address(three, "WIDE2", 2, true);
        CHECK(with_crc(three).size() == 23 && centred(stuffed(wire(with_crc(three)))).empty());   // 7 m + 2 bytes: no control byte
        three.push_back(0x03);
        CHECK(centred(stuffed(wire(with_crc(three)))) == with_crc(three));            // 7 m + 3: accepted
        int st = -1;
        CHECK(address_byte(0, 'A' << 1, st) && address_byte(5, ' ' << 1, st) && address_byte(6, 0xE0, st) && st == -1);
        CHECK(!address_byte(6, 0xE1, st) && !address_byte(7, '*' << 1, st) && !address_byte(69, 0x60, st) && address_byte(13, 0x61, st) && st == 13);
        CHECK(address_byte(14, 0xFF, st) && st == 13);
        // the flag test: q_min, the level in front, a NaN
        const Bits bits = burst(stuffed(wire(good)));
        std::vector<float> z = row_of(bits, BACK, BACK + SPB * (long)bits.size());
        Rec c;
        CHECK(one_start(z, BACK, 1.0f, c) && !one_start(z, BACK, 1.5f, c) && !one_start(z, BACK - 1, 0.0f, c));   // s - 22 < 0: no such start
        z[BACK + 3 * SPB] = NAN;
        CHECK(!one_start(z, BACK, 0.0f, c));
    }
    // the reach: stuffed ones, every transition late enough for a nudge of +1, walked to strobe LAST_K and no further
    {
        const long n = BACK + REACH;
        std::vector<float> z((size_t)n, 0.0f);
        const int flag[8] = {0, 1, 1, 1, 1, 1, 1, 0};
        float level = -1.0f;
        for (long j = 0; j < BACK + 11; j++) z[(size_t)j] = level;
        for (int k = 0; k < 8; k++) {
            level = flag[k] ? level : -level;
            for (long j = BACK + SPB * k - 11; j < BACK + SPB * k + 11; j++) z[(size_t)j] = level;
        }
        long p_prev = BACK + HEAD, n_changes = 0;
        int a = 0;
        for (int k = 8; k <= LAST_K; k++) {
            const long p = p_prev + SPB + a;
            const int bit = (k - 8) % 6 == 5 ? 0 : 1;   // 11111 0 11111 0 ...
            a = 0;
            if (bit) {
                for (long j = p_prev + 1; j <= p; j++) z.at((size_t)j) = level;
            } else {
                const long c = p_prev + 16;              // e = 2 c - (p_prev + p) - 1 = 9 or 8
                for (long j = p_prev + 1; j < c; j++) z.at((size_t)j) = level;
                level = -level;
                for (long j = c; j <= p; j++) z.at((size_t)j) = level;
                a = 1;
                n_changes++;
            }
            p_prev = p;
        }
        const long last = p_prev - BACK;                 // strobe LAST_K, relative to s
        CHECK(last == HEAD + (long)SPB * (LAST_K - 7) + n_changes && n_changes == 529 && last < REACH);
        long far = 0;
        float q;
        CHECK(candidate([&](int k) { return z.at((size_t)(BACK + SPB * k)); }, 0.0f, q) && q == 1.0f);
        auto Z = [&](long j) { far = j > far ? j : far; return z.at((size_t)(BACK + j)); };
        CHECK(walk(Z, n - BACK, [](int, uint32_t) {}) == 0 && far == last);
        // the same row cut behind strobe LAST_K - 1: the walk ends there, inside the row
        far = 0;
        CHECK(walk(Z, last, [](int, uint32_t) {}) == 0 && far < last);
        // and the bound itself: a strobe 23 behind the one before, every time
        CHECK(REACH - 1 == HEAD + (long)(SPB + 1) * (LAST_K - 7));
    }
    // the one-record rule and the windows: NEAR = 22
    {
        using L = std::vector<long>;
        CHECK(kept({}, 0, 100) == L{} && kept({{50, 1.0f}}, 0, 100) == L{50} && kept({{50, 1.0f}}, 51, 100) == L{} && kept({{50, 1.0f}}, 0, 50) == L{});
        CHECK((kept({{50, 2.0f}, {72, 1.0f}}, 0, 100) == L{50, 72}) && kept({{50, 2.0f}, {71, 1.0f}}, 0, 100) == L{50} && kept({{50, 1.0f}, {71, 2.0f}}, 0, 100) == L{71});
        CHECK(kept({{49, 2.0f}, {50, 1.0f}}, 50, 100) == L{} && kept({{49, 1.0f}, {50, 2.0f}}, 50, 100) == L{50});
        CHECK(kept({{50, 1.0f}, {51, 1.0f}, {60, 1.0f}, {71, 1.0f}}, 0, 100) == L{50});
        CHECK((kept({{50, 1.0f}, {60, 2.0f}, {75, 3.0f}, {99, 1.0f}}, 0, 100) == L{75, 99}));
        CHECK(!drops(true, 11, 1.0f, 10, 1.0f) && drops(true, 9, 1.0f, 10, 1.0f) && drops(true, 31, 2.0f, 10, 1.0f) && !drops(true, 32, 2.0f, 10, 1.0f));
        CHECK(!drops(false, 9, 2.0f, 10, 1.0f) && !drops(true, 10, 2.0f, 10, 1.0f));
        const Reach w = reach_of(100, 200, 1000000), e = reach_of(0, 10, 10), t = reach_of(999990, 1000000, 1000000);
        CHECK(w.e0 == 79 && w.e1 == 221 && w.need_lo == 57 && w.need_hi == 220 + REACH);
        CHECK(e.e0 == 0 && e.e1 == 10 && e.need_lo == 0 && e.need_hi == 10 && t.e1 == 1000000 && t.need_hi == 1000000);
    }
    if (fails) return 1;
    printf("packet_host: ok\n");
    return 0;
}

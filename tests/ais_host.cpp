// ais_host.cpp — pss_ais.h with the host compiler alone (no HIP), as a program of its own under AddressSanitizer and UBSan
// (tests/test_ais_golden.py builds and runs it).  Every row lives in a heap buffer of exactly its size, so a strobe read outside the row is
// an error the sanitizer reports.  The one-record rule runs through pss_starts.h's keep_starts (the neighbour loop of pss_h_ais_frames) over
// hand-made lists, each in a heap vector of exactly its size as well.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pss_ais.h"
#include "pss_starts.h"

using namespace pss_ais;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("ais_host: line %d: %s\n", __LINE__, #c);           \
            fails++;                                                    \
        }                                                               \
    } while (0)

static std::vector<int> wire(const std::vector<uint8_t> &bytes)
{
    std::vector<int> b;
    for (uint8_t v : bytes)
        for (int k = 0; k < 8; k++) b.push_back((v >> k) & 1);
    return b;
}

// training, flag, the stuffed frame, flag
static std::vector<int> burst(const std::vector<uint8_t> &frame, int training)
{
    std::vector<int> out;
    for (int k = 0; k < training; k++) out.push_back(k & 1);
    const int flag[8] = {0, 1, 1, 1, 1, 1, 1, 0};
    out.insert(out.end(), flag, flag + 8);
    int run = 0;
    for (int b : wire(frame)) {
        out.push_back(b);
        run = b ? run + 1 : 0;
        if (run == 5) { out.push_back(0); run = 0; }
    }
    out.insert(out.end(), flag, flag + 8);
    return out;
}

static std::vector<uint8_t> with_crc(std::vector<uint8_t> body)
{
    const uint32_t c = crc_reg(body.data(), (long)body.size()) ^ 0xFFFFu;
    body.push_back((uint8_t)(c & 0xFF));
    body.push_back((uint8_t)(c >> 8));
    return body;
}

// a row of n samples with the burst's levels on the strobes, the first at `at`
static std::vector<float> row_of(const std::vector<int> &bits, long at, long n)
{
    std::vector<float> y((size_t)n, 0.0f);
    float level = 1.0f;
    for (size_t i = 0; i < bits.size(); i++) {
        level = bits[i] ? level : -level;
        const long j = at + SPB * (long)i;
        if (j >= 0 && j < n) y[(size_t)j] = level;
    }
    return y;
}

// every start of the row on one thread -> the accepted ones
struct Rec { long s; int len; float q; uint8_t msg[MAX_BYTES]; };
static std::vector<Rec> frames(const std::vector<float> &y)
{
    const long n = (long)y.size();
    std::vector<Rec> out;
    for (long s = 0; s < n; s++) {
        if (!exists(s, n)) continue;
        auto Y = [&](int k) { return y.at((size_t)(s + SPB * k)); };
        float thr;
        Rec c;
        if (!candidate(Y, thr, c.q)) continue;
        memset(c.msg, 0, MAX_BYTES);
        c.s = s;
        uint32_t words[MAX_BYTES / 4] = {};
        c.len = walk(Y, thr, (n - s + SPB - 1) / SPB, [&](int i, uint32_t v) { words[i] = v; });
        for (int j = 0; j < MAX_BYTES; j++) c.msg[j] = (uint8_t)(words[j / 4] >> (8 * (j % 4)));
        if (c.len > 0) out.push_back(c);
    }
    return out;
}

// keep_starts over an ascending list of starts of one row that all carry the same frame -> the starts it emits, in its order
struct Start { long s; float q; };
static std::vector<long> kept(const std::vector<Start> &list, long s_begin, long s_end)
{
    const std::vector<Start> heap(list.begin(), list.end());   // exactly list.size() records
    std::vector<long> out;
    pss_starts::keep_starts(
        heap.data(), heap.size(), s_begin, s_end, NEAR, [](const Start &b, const Start &a) { return drops(true, b.s, b.q, a.s, a.q); },
        [&](const Start &a) { out.push_back(a.s); });
    return out;
}

int main()
{
    // the neighbour rule over lists: NEAR = 5
    {
        using L = std::vector<long>;
        CHECK(NEAR == 5 && kept({}, 0, 100) == L{});
        CHECK(kept({{50, 1.0f}}, 0, 100) == L{50} && kept({{50, 1.0f}}, 50, 51) == L{50} && kept({{50, 1.0f}}, 51, 100) == L{} && kept({{50, 1.0f}}, 0, 50) == L{});
        // exactly NEAR apart: both stay; NEAR - 1 apart: the weaker one goes, whichever side it is on
        CHECK((kept({{50, 2.0f}, {55, 1.0f}}, 0, 100) == L{50, 55}) && (kept({{50, 1.0f}, {55, 2.0f}}, 0, 100) == L{50, 55}));
        CHECK(kept({{50, 2.0f}, {54, 1.0f}}, 0, 100) == L{50} && kept({{50, 1.0f}, {54, 2.0f}}, 0, 100) == L{54});
        // the stronger neighbour just outside the window still drops the one inside, and is not emitted itself
        CHECK(kept({{49, 2.0f}, {50, 1.0f}}, 50, 100) == L{} && kept({{49, 1.0f}, {50, 2.0f}}, 0, 50) == L{});
        CHECK(kept({{49, 1.0f}, {50, 2.0f}}, 50, 100) == L{50} && kept({{49, 2.0f}, {50, 1.0f}}, 0, 50) == L{49});
        // equal scores: the earlier start stays
        CHECK(kept({{50, 1.0f}, {51, 1.0f}}, 0, 100) == L{50} && kept({{50, 1.0f}, {51, 1.0f}, {52, 1.0f}, {53, 1.0f}, {54, 1.0f}, {55, 1.0f}}, 0, 100) == L{50});
        // a neighbour drops a start whatever its own fate: 53 goes to 56, and still drops 50
        CHECK((kept({{50, 1.0f}, {53, 2.0f}, {56, 3.0f}, {90, 1.0f}}, 0, 100) == L{56, 90}));
    }
    // the check value and the residue
    const uint8_t digits[] = "123456789";
    CHECK((crc_reg(digits, 9) ^ 0xFFFFu) == 0x906Eu);
    const uint8_t closed[] = {'1', '2', '3', '4', '5', '6', '7', '8', '9', 0x6E, 0x90};
    CHECK(crc_reg(closed, 11) == CRC_RESIDUE);
    // the pulse: symmetric, sum 1, its peak in the middle
    for (int span = 1; span <= MAX_SPAN; span++) {
        std::vector<double> g((size_t)pulse_len(span));
        default_pulse(span, g.data());
        double sum = 0.0;
        for (size_t u = 0; u < g.size(); u++) {
            sum += g[u];
            CHECK(g[u] == g[g.size() - 1 - u] && g[u] <= g[(g.size() - 1) / 2]);
        }
        CHECK(fabs(sum - 1.0) < 1e-15 && (int)g.size() <= MAX_PULSE);
    }
    // the plan
    int D, up, down;
    CHECK(plan(2400000, D, up, down) && D == 50 && up == 1 && down == 1);
    CHECK(plan(250000, D, up, down) && D == 5 && up == 24 && down == 25);
    CHECK(!plan(1000003, D, up, down));
    // the front on a row of exactly its size: a constant rotation gives a constant angle between the edges
    {
        const long n = 40;
        std::vector<float> x((size_t)(2 * n));
        for (long i = 0; i < n; i++) { x[2 * i] = (float)cos(0.3 * i); x[2 * i + 1] = (float)sin(0.3 * i); }
        std::vector<double> g((size_t)pulse_len(2));
        default_pulse(2, g.data());
        std::vector<float> d((size_t)n);
        for (long i = 0; i < n; i++)
            d[i] = i ? disc(x[2 * i], x[2 * i + 1], x[2 * i - 2], x[2 * i - 1], [](float im, float re) { return atan2f(im, re); }) : 0.0f;
        for (long i = 0; i < n; i++) {
            const float v = filtered([&](long j) { return j >= 0 && j < n ? d.at((size_t)j) : 0.0f; }, g.data(), (int)g.size(), i);
            if (i >= 6 && i < n - 5) CHECK(fabsf(v - 0.3f) < 1e-5f);
        }
        const Span sp = front_span(10, 20, 11, n);
        CHECK(sp.lo == 4 && sp.hi == 25 && front_span(0, n, 11, n).lo == 0 && front_span(0, n, 11, n).hi == n);
    }
    // frames: the shortest and the longest, at the row's first start and ending on its last sample
    for (int n_body : {5, 19, 126}) {
        std::vector<uint8_t> body;
        for (int i = 0; i < n_body; i++) body.push_back((uint8_t)(37 * i + 11 + n_body));
        const std::vector<uint8_t> frame = with_crc(body);
        const std::vector<int> bits = burst(frame, 9);
        const long last = SPB * (long)(bits.size() - 1);
        const std::vector<float> y = row_of(bits, 0, last + 1);
        const std::vector<Rec> r = frames(y);
        CHECK(r.size() == 1 && r[0].s == BACK && r[0].len == n_body + 2 && r[0].q == 1.0f);
        if (r.size() == 1) {
            CHECK(memcmp(r[0].msg, frame.data(), frame.size()) == 0);
            for (size_t j = frame.size(); j < MAX_BYTES; j++) CHECK(r[0].msg[j] == 0);
        }
        CHECK(frames(row_of(bits, 0, last)).empty());          // one sample shorter: the closing flag's last strobe lies outside
        CHECK(frames(row_of(bits, -SPB, last + 1)).empty());   // the first training bit is cut off: no start 45 samples into the row
    }
    // 127 message bytes do not fit; seven ones reject; every walk stops at LAST_K
    {
        std::vector<uint8_t> body(127, 0x55);
        const std::vector<int> bits = burst(with_crc(body), 9);
        CHECK(frames(row_of(bits, 0, SPB * (long)bits.size())).empty());
        std::vector<uint8_t> ones(200, 0xFF);
        const std::vector<int> stuffed = burst(ones, 9);        // 11111 0 11111 0 ...: the walk appends 1030 bits and stops
        const long n = BACK + REACH;
        std::vector<float> y = row_of(stuffed, 0, n);
        long reads = 0, far = 0;
        float thr, q;
        auto Y = [&](int k) { reads++; far = k > far ? k : far; return y.at((size_t)(BACK + SPB * k)); };
        CHECK(candidate(Y, thr, q));
        CHECK(walk(Y, thr, (n - BACK + SPB - 1) / SPB, [](int, uint32_t) {}) == 0 && far == LAST_K);
        CHECK(REACH == SPB * (long)LAST_K + 1);
    }
    // the one-record rule and the windows
    CHECK(drops(true, 11, 1.0f, 10, 1.0f) == false && drops(true, 9, 1.0f, 10, 1.0f) && drops(true, 14, 2.0f, 10, 1.0f));
    CHECK(!drops(true, 15, 2.0f, 10, 1.0f) && !drops(false, 9, 2.0f, 10, 1.0f) && !drops(true, 10, 2.0f, 10, 1.0f));
    const Reach w = reach_of(100, 200, 100000), e = reach_of(0, 10, 10), t = reach_of(99990, 100000, 100000);
    CHECK(w.e0 == 96 && w.e1 == 204 && w.need_lo == 51 && w.need_hi == 203 + REACH);
    CHECK(e.e0 == 0 && e.e1 == 10 && e.need_lo == 0 && e.need_hi == 10 && t.e1 == 100000 && t.need_hi == 100000);
    if (fails) return 1;
    printf("ais_host: ok\n");
    return 0;
}

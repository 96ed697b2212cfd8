// ook_host.cpp — pss_ook.h with the host compiler alone (no HIP), as a program of its own under AddressSanitizer and UBSan
// (tests/test_ook_golden.py builds and runs it).  Every row lives in a heap buffer of exactly its size and every window in one of exactly its
// stated reach, so a sample read outside the row or its halo is an error the sanitizer reports.  The slicers run on written-out edge lists:
// Manchester in both phases with the odd symbol first, last and nowhere, the chain's ends, the caps.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pss_ook.h"

using namespace pss_ook;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("ook_host: line %d: %s\n", __LINE__, #c);        \
            fails++;                                                 \
        }                                                            \
    } while (0)

struct Edge { long n; bool rise; };

// the edges [e0, e1) of a row of which the heap buffer holds exactly [lo, hi)
static std::vector<Edge> edges_of(const std::vector<float> &m, long lo, long n_row, long e0, long e1, int P, float hi_t, float lo_t, int R)
{
    std::vector<Edge> out;
    row_edges([&](long i) { return m.at((size_t)(i - lo)); }, n_row, e0, e1, P, hi_t, lo_t, R, [&](long n, bool rise) { out.push_back({n, rise}); });
    return out;
}

static Message walk_list(const std::vector<long> &e, long span, long gap_limit, long n_row, const Slicer &s)
{
    return walk([&](long a) { return a < (long)e.size() ? e.at((size_t)a) : NO_EDGE; }, e.at(0), span, gap_limit, n_row, s);
}

static std::vector<int> bits_of(const Message &r)
{
    std::vector<int> b;
    for (int k = 0; k < r.n_bits; k++) b.push_back((r.bits[k >> 3] >> (7 - (k & 7))) & 1);
    return b;
}

// the edge list of symbols (pulse, gap, pulse, ...) from position 100
static std::vector<long> list_of(const std::vector<long> &symbols)
{
    std::vector<long> e = {100};
    for (long w : symbols) e.push_back(e.back() + w);
    return e;
}

int main()
{
    // ---- magnitude, envelope, state on a written-out row
    CHECK(magnitude(3.0f, 4.0f) == 25.0f);
    {
        const float m[5] = {1.0f, 2.0f, 4.0f, 8.0f, 16.0f};
        CHECK(envelope([&](int k) { return m[4 - k]; }, 1) == 16.0f);
        CHECK(envelope([&](int k) { return m[4 - k]; }, 4) == 7.5f);
        CHECK(envelope([&](int k) { return 2 - k >= 0 ? m[2 - k] : 0.0f; }, 5) == 1.4f);
        CHECK(decisive(4.0f, 4.0f, 1.0f) == 3 && decisive(1.0f, 4.0f, 1.0f) == 0 && decisive(0.5f, 4.0f, 1.0f) == 2 && decisive(NAN, 4.0f, 1.0f) == 0);
        CHECK(decisive(INFINITY, 4.0f, 1.0f) == 3 && decisive(2.0f, 2.0f, 2.0f) == 3);
        CHECK(state(scan_word(7, 3), 7 + 64, 64) && !state(scan_word(7, 3), 7 + 65, 64) && !state(scan_word(7, 2), 7, 64) && !state(0, 0, 64));
    }
    // ---- a row in a buffer of exactly its size: high (16), neither (2), low (0.25); the reach R holds the state over `neither`
    {
        const long n_row = 300;
        std::vector<float> m((size_t)n_row, 0.25f);
        for (long i = 10; i < 20; i++) m[(size_t)i] = 16.0f;      // a pulse that low samples end: it falls at 20
        for (long i = 50; i < 60; i++) m[(size_t)i] = 16.0f;      // one that `neither` follows: it falls R + 1 behind its last high sample
        for (long i = 60; i < 200; i++) m[(size_t)i] = 2.0f;
        for (long i = 290; i < 300; i++) m[(size_t)i] = 16.0f;    // one still on at the row's end: it falls at n_row
        for (int R : {0, 1, 64}) {
            const std::vector<Edge> e = edges_of(m, 0, n_row, 0, n_row + 1, 1, 4.0f, 1.0f, R);
            CHECK(e.size() == 6);
            if (e.size() == 6) {
                CHECK(e[0].n == 10 && e[0].rise && e[1].n == 20 && !e[1].rise && e[2].n == 50 && e[3].n == 59 + R + 1 && !e[3].rise);
                CHECK(e[4].n == 290 && e[4].rise && e[5].n == n_row && !e[5].rise);
            }
            // windows: every split of the edge range, each buffer holding exactly what the rule states, gives the whole row's edges
            for (long cut = 1; cut < n_row; cut += 7) {
                std::vector<Edge> parts;
                const long ends[3] = {0, cut, n_row + 1};
                for (int w = 0; w < 2; w++) {
                    const long e0 = ends[w], e1 = ends[w + 1];
                    const long lo = e0 - 1 - R < 0 ? 0 : e0 - 1 - R, hi = e1 < n_row ? e1 : n_row;
                    const std::vector<float> buf(m.begin() + lo, m.begin() + hi);
                    for (const Edge &x : edges_of(buf, lo, n_row, e0, e1, 1, 4.0f, 1.0f, R)) parts.push_back(x);
                }
                CHECK(parts.size() == e.size());
                for (size_t k = 0; k < parts.size() && k < e.size(); k++) CHECK(parts[k].n == e[k].n && parts[k].rise == e[k].rise);
            }
        }
        // P = 9: the buffer reaches P - 1 further back
        const std::vector<Edge> whole = edges_of(m, 0, n_row, 0, n_row + 1, 9, 4.0f, 1.0f, 3);
        const long e0 = 40, lo = e0 - 1 - 3 - 8;
        const std::vector<float> buf(m.begin() + lo, m.end());
        const std::vector<Edge> part = edges_of(buf, lo, n_row, e0, n_row + 1, 9, 4.0f, 1.0f, 3);
        size_t skip = 0;
        while (skip < whole.size() && whole[skip].n < e0) skip++;
        CHECK(part.size() == whole.size() - skip && part.size() > 0);
        for (size_t k = 0; k < part.size() && skip + k < whole.size(); k++) CHECK(part[k].n == whole[skip + k].n && part[k].rise == whole[skip + k].rise);
    }
    // ---- the reach of a window
    {
        const Reach r = reach_of(5000, 6000, 100000, 9, 64, 750, 4096);
        CHECK(r.e0 == 4250 && r.e1 == 6000 + 4096 - 1 && r.need_lo == 5000 - (750 + 64 + 9) && r.need_hi == 6000 + 4096);
        const Reach c = reach_of(10, 90, 100, 65, 4096, 1 << 20, 1 << 24);
        CHECK(c.e0 == 0 && c.e1 == 101 && c.need_lo == 0 && c.need_hi == 100);
        CHECK(halo_before(9, 64, 750) == 823 && halo_after(4096) == 4096);
    }
    // ---- PWM and PPM on written-out lists
    const Slicer pwm = {PWM, 4, 8, 12, 1, 0, 0, 0, 0}, ppm = {PPM, 4, 8, 12, 1, 0, 0, 0, 0};
    {
        // pulses 4, 8, 12 (sync), 6 (odd), 5; gaps 8, 4, 4, 4
        const std::vector<long> e = list_of({4, 8, 8, 4, 12, 4, 6, 4, 5});
        Message r = walk_list(e, 1000, 10, 5000, pwm);
        CHECK(r.n_pulses == 5 && r.n_bits == 3 && r.n_odd == 1 && r.flags == 0 && r.span == 55 && bits_of(r) == std::vector<int>({1, 0, 1}));
        r = walk_list(e, 1000, 10, 5000, ppm);
        CHECK(r.n_pulses == 5 && r.n_bits == 4 && r.n_odd == 0 && bits_of(r) == std::vector<int>({1, 0, 0, 0}));
        Slicer inv = pwm;
        inv.invert = 1;
        CHECK(bits_of(walk_list(e, 1000, 10, 5000, inv)) == std::vector<int>({0, 1, 0}));
        // a gap above gap_limit ends the message behind its pulse; the span cuts it: a fall at lim is not read
        r = walk_list(e, 1000, 7, 5000, pwm);
        CHECK(r.n_pulses == 1 && r.n_bits == 1 && r.flags == 0 && r.span == 4);
        r = walk_list(e, 20, 10, 5000, pwm);        // lim = 120: pulse 1 rises at 112 and falls at 120
        CHECK(r.n_pulses == 1 && r.flags == F_LONG);
        r = walk_list(e, 21, 10, 5000, pwm);
        CHECK(r.n_pulses == 2 && r.flags == 0);     // and the next rise, at 124, is not read: nothing is cut short
        r = walk_list(e, 25, 10, 5000, pwm);        // lim = 125: the pulse that rises at 124 falls past it
        CHECK(r.n_pulses == 2 && r.flags == F_LONG);
        r = walk_list(e, 1000, 10, 155, pwm);       // the last pulse falls at the row's end
        CHECK(r.n_pulses == 5 && r.flags == F_OPEN);
    }
    {
        // 1025 pulses of 4 with gaps of 8: the 1025th is dropped (MANY), 256 bits are kept (FULL)
        std::vector<long> sym;
        for (int k = 0; k < 1025; k++) { sym.push_back(4); sym.push_back(8); }
        sym.pop_back();
        const Message r = walk_list(list_of(sym), 1 << 20, 10, 1 << 30, pwm);
        CHECK(r.n_pulses == 1024 && r.n_bits == 256 && r.flags == (F_MANY | F_FULL) && r.span == 1023 * 12 + 4);
        sym.resize(2 * 256 - 1);
        const Message q = walk_list(list_of(sym), 1 << 20, 10, 1 << 30, pwm);
        CHECK(q.n_pulses == 256 && q.n_bits == 256 && q.flags == 0);
        for (int k = 0; k < BITS_BYTES; k++) CHECK(q.bits[k] == 0xFF);
    }
    // ---- Manchester on written-out symbol lists: half-bit 5, both phases, the odd symbol first, last and nowhere
    {
        Slicer mc = {MC, 5, 0, 0, 1, 0, 0, 0, 0};
        // h = 1 0 | 0 1 | 1 0 | 1 0 | 0 1 | 1 : the symbols 5 10 10 5 5 10 10 -> phase 0: 1 0 1 1 0; phase 1: (0,0) (1,1) (0,1) (0,0) (1,1): four odd, 0
        const std::vector<long> clean = {5, 10, 10, 5, 5, 10, 10};
        Message r = walk_list(list_of(clean), 1000, 20, 5000, mc);
        CHECK(r.n_pulses == 4 && r.n_odd == 0 && bits_of(r) == std::vector<int>({1, 0, 1, 1, 0}));
        mc.phase = 1;
        r = walk_list(list_of(clean), 1000, 20, 5000, mc);
        CHECK(r.n_odd == 4 && bits_of(r) == std::vector<int>({0}));
        // 5 5 5 5 5: h = 1 0 1 0 1 -> phase 0: 1 1; phase 1: 0 0
        r = walk_list(list_of({5, 5, 5, 5, 5}), 1000, 20, 5000, mc);
        CHECK(r.n_odd == 0 && bits_of(r) == std::vector<int>({0, 0}));
        mc.phase = 0;
        r = walk_list(list_of({5, 5, 5, 5, 5}), 1000, 20, 5000, mc);
        CHECK(r.n_odd == 0 && bits_of(r) == std::vector<int>({1, 1}));
        // the odd symbol first: nothing but one odd
        r = walk_list(list_of({7, 5, 5}), 1000, 20, 5000, mc);
        CHECK(r.n_pulses == 2 && r.n_bits == 0 && r.n_odd == 1);
        // in the middle: the list ends there, the half-bit before it has no partner
        r = walk_list(list_of({5, 5, 5, 13, 5}), 1000, 20, 5000, mc);
        CHECK(r.n_odd == 1 && bits_of(r) == std::vector<int>({1}));
        // last
        r = walk_list(list_of({5, 5, 5, 5, 8}), 1000, 20, 5000, mc);
        CHECK(r.n_odd == 1 && bits_of(r) == std::vector<int>({1, 1}));
        mc.tol = 0;
        r = walk_list(list_of({5, 5, 6}), 1000, 20, 5000, mc);
        CHECK(r.n_odd == 1 && bits_of(r) == std::vector<int>({1}));
    }
    // ---- refusals of the slicer
    {
        CHECK(slicer_refusal(pwm) == nullptr && slicer_refusal(ppm) == nullptr);
        Slicer s = pwm;
        s.tol = 2;                                   // 4 and 8 are exactly 2 tol apart
        CHECK(slicer_refusal(s) != nullptr);
        s = pwm;
        s.w_sync = 10;                               // 8 and 10 at tol 1: exactly 2 tol apart
        CHECK(slicer_refusal(s) != nullptr);
        s.w_sync = 11;
        CHECK(slicer_refusal(s) == nullptr);
        s = {MC, 4, 0, 0, 2, 0, 0, 0, 0};            // 4 and 8 at tol 2
        CHECK(slicer_refusal(s) != nullptr);
        s.tol = 1;
        CHECK(slicer_refusal(s) == nullptr);
        s.mode = 3;
        CHECK(slicer_refusal(s) != nullptr);
        CHECK(meta_of(1024, 5000, F_MANY) == (1024u | 2047u << 11 | F_MANY));
    }
    if (fails) return 1;
    printf("ook_host: ok\n");
    return 0;
}

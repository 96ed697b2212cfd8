// flex_host.cpp — pss_flex.h with the host compiler alone (no HIP), as a program of its own under AddressSanitizer and UBSan
// (tests/test_flex_golden.py builds and runs it).  Every row lives in a heap buffer of exactly its size, so a sample read outside the row
// is an error the sanitizer reports.  It builds frames of every mode in both polarities, walks them with the header's statements as
// pss_h_flex_frames does, and runs the one-record rule through pss_starts.h's keep_starts over hand-made lists.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pss_flex.h"
#include "pss_starts.h"

using namespace pss_flex;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("flex_host: line %d: %s\n", __LINE__, #c);        \
            fails++;                                                  \
        }                                                             \
    } while (0)

static uint32_t with_sum(uint32_t d)
{
    d &= 0x1FFFF0u;
    return d | ((15u - (uint32_t)nibble_sum(d)) & 15u);
}

// the phase words of the test frames: word j of phase p
static uint32_t sent(int p, int j) { return word((uint32_t)(0x12345u * (uint32_t)(j + 1) + 0x777u * (uint32_t)p) & 0x1FFFFFu); }

// a frame of `mode` on the strobes of a row of exactly n samples, the first strobe at `at`, every level on one sample of its slot
static std::vector<float> row_of(int mode, int h, long at, long n, bool inverted, uint32_t fiw)
{
    const Mode m = mode_of(mode);
    std::vector<float> lv((size_t)FRAME_H, 0.0f);
    const uint64_t sync = (uint64_t)m.code << 48 | (uint64_t)MARKER << 16 | (uint64_t)(~m.code & 0xFFFFu);
    for (int k = 0; k < DATA_BIT; k++) {
        bool one = (k & 1) != 0;
        if (k < 64) one = ((sync >> (63 - k)) & 1u) != 0;
        else if (k >= FIW_BIT && k < FIW_BIT + 32) one = ((fiw >> (k - FIW_BIT)) & 1u) != 0;
        lv[(size_t)(2 * k)] = lv[(size_t)(2 * k + 1)] = one ? 1.0f : -1.0f;
    }
    for (int p = 0; p < (m.fast ? 2 : 1); p++)
        for (int i = 0; i < N_SYM; i++) {
            const int at_w = 8 * (i >> 8) + (i & 7), bit = (i & 255) >> 3;
            const bool a = ((sent(2 * p, at_w) >> bit) & 1u) != 0, b = ((sent(2 * p + 1, at_w) >> bit) & 1u) != 0;
            const float v = !m.four ? (a ? 1.0f : -1.0f) : a ? (b ? 1.0f / 3 : 1.0f) : (b ? -1.0f / 3 : -1.0f);
            if (m.fast) lv[(size_t)(2 * DATA_BIT + 2 * i + p)] = v;
            else lv[(size_t)(2 * DATA_BIT + 2 * i)] = lv[(size_t)(2 * DATA_BIT + 2 * i + 1)] = v;
        }
    std::vector<float> y((size_t)n, 0.0f);
    for (long g = 0; g < FRAME_H; g++) {
        const long j = at + g * h;
        if (j >= 0 && j < n) y[(size_t)j] = inverted ? -lv[(size_t)g] : lv[(size_t)g];
    }
    return y;
}

struct Rec { long s; Head hd; int n_bad, n_fixed; uint32_t words[N_PHASES * N_WORDS]; };
static std::vector<Rec> frames(const std::vector<float> &y, int h, int sync_errors, int fix, int max_bad)
{
    const long n = (long)y.size();
    std::vector<Rec> out;
    for (long s = 0; s < n; s++) {
        if (!exists(s, n, h)) continue;
        Rec c;
        c.s = s;
        if (!head([&](int o) { return y.at((size_t)(s + (long)o * h)) + y.at((size_t)(s + (long)o * h + h)); }, sync_errors, fix, c.hd)) continue;
        const Slicer z = slicer_of(c.hd);
        memset(c.words, 0, sizeof(c.words));
        for (int p = 0; p < (z.fast ? 2 : 1); p++)
            for (int i = 0; i < N_SYM; i++) {
                bool ba, bb;
                symbol([&](long o) { return y.at((size_t)(s + o)); }, h, z, i, p, ba, bb);
                const int at = 8 * (i >> 8) + (i & 7), bit = (i & 255) >> 3;
                if (ba) c.words[(2 * p) * N_WORDS + at] |= 1u << bit;
                if (bb && z.four) c.words[(2 * p + 1) * N_WORDS + at] |= 1u << bit;
            }
        c.n_bad = c.n_fixed = 0;
        for (int i = 0; i < N_PHASES * N_WORDS; i++) {
            if (!active(c.hd.mode, i / N_WORDS)) continue;
            uint32_t o;
            const int m = check(c.words[i], fix, o);
            c.words[i] = o;
            if (m < 0) c.n_bad++;
            else c.n_fixed += m;
        }
        if (c.n_bad <= max_bad) out.push_back(c);
    }
    return out;
}

struct Start { long s; int e; float a; };
static std::vector<long> kept(const std::vector<Start> &list, long s_begin, long s_end, int h)
{
    const std::vector<Start> heap(list.begin(), list.end());   // exactly list.size() records
    std::vector<long> out;
    pss_starts::keep_starts(
        heap.data(), heap.size(), s_begin, s_end, 2l * h, [&](const Start &b, const Start &a) { return drops(b.s, b.e, b.a, a.s, a.e, a.a, h); },
        [&](const Start &a) { out.push_back(a.s); });
    return out;
}

int main()
{
    // the word: a POCSAG codeword bit-reversed; the check undoes one and two wrong bits anywhere
    for (uint32_t d = 0; d < (1u << 21); d += 4093) {
        const uint32_t w = word(d);
        uint32_t out = 1;
        CHECK((w & 0x1FFFFFu) == d && brev32(w) == pss_pocsag::codeword(brev32(d) >> 11) && (pss_pocsag::popcount32(w) & 1) == 0);
        CHECK(check(w, 0, out) == 0 && out == w);
        CHECK(check(w ^ (1u << (d % 32)), 1, out) == 1 && out == w && check(w ^ (1u << (d % 32)), 0, out) == -1 && out == 0);
        CHECK(check(w ^ (1u << (d % 32)) ^ (1u << ((d + 7) % 32)), 2, out) == 2 && out == w);
    }
    CHECK(brev32(1u) == 0x80000000u && brev32(0x12345678u) == 0x1E6A2C48u);
    CHECK(nibble_sum(with_sum(0x7u << 4 | 0x64u << 8)) == 15 && nibble_sum(0) == 0 && nibble_sum(0x1FFFFFu) == ((5 * 15 + 1) & 15));
    // the pulse
    for (int h = MIN_H; h <= MAX_H; h++) {
        const int P = pulse_len(h);
        std::vector<double> g((size_t)P);
        default_pulse(h, g.data());
        CHECK((P & 1) && P <= h && P + 2 > h && g[0] == 1.0 / P && g[(size_t)P - 1] == g[0]);
    }
    // the modes: pairwise more than 2 * 3 apart, so a code within sync_errors of one is nearest to it alone
    for (int a = 0; a < N_MODES; a++)
        for (int b = a + 1; b < N_MODES; b++) CHECK(pss_pocsag::popcount32(mode_of(a).code ^ mode_of(b).code) > 2 * MAX_SYNC_ERRORS);
    CHECK(active(0, 0) && !active(0, 1) && !active(0, 2) && active(1, 1) && !active(1, 2) && active(2, 2) && !active(2, 1) && active(4, 3));
    // a frame at the row's first start and ending on its last sample; one sample shorter: no start
    const uint32_t fiw = word(with_sum(0x7u << 4 | 0x64u << 8));
    for (int h : {1, 2, 12, 64})
        for (int mode = 0; mode < N_MODES; mode++)
            for (bool inverted : {false, true}) {
                if (h == 64 && (mode == 1 || mode == 4)) continue;   // (time)
                const long n = reach(h);
                const std::vector<Rec> r = frames(row_of(mode, h, 0, n, inverted, fiw), h, 0, 0, 0);
                CHECK(r.size() == 1 && r[0].s == 0 && r[0].hd.a == 2.0f && r[0].hd.c == 0.0f && r[0].hd.mode == mode && r[0].hd.inverted == inverted);
                if (r.size() == 1) {
                    CHECK(r[0].hd.fiw == fiw && r[0].n_bad == 0 && r[0].n_fixed == 0 && meta0_of(r[0].hd) == ((inverted ? 1u << 8 : 0u) | (uint32_t)mode << 12));
                    for (int i = 0; i < N_PHASES * N_WORDS; i++) CHECK(r[0].words[i] == (active(mode, i / N_WORDS) ? sent(i / N_WORDS, i % N_WORDS) : 0u));
                }
                CHECK(frames(row_of(mode, h, 0, n - 1, inverted, fiw), h, 3, 2, MAX_BAD).empty());
            }
    // inside a longer row: a wrong FIW bit is fixed and counted; a NaN in the sync: no frame; a NaN in the data: one bit to fix
    {
        std::vector<float> y = row_of(3, 2, 37, 37 + reach(2) + 9, true, fiw ^ 0x400u);
        std::vector<Rec> r = frames(y, 2, 0, 1, 0);
        CHECK(r.size() == 1 && r[0].s == 37 && r[0].hd.fiw == fiw && r[0].hd.fiw_fix == 1 && errors_of(r[0].hd) == 1);
        CHECK(frames(y, 2, 3, 0, MAX_BAD).empty());
        y[37 + 2 * 2 * 10] = NAN;
        CHECK(frames(y, 2, 3, 2, MAX_BAD).empty());
        y = row_of(1, 2, 5, 5 + reach(2), false, fiw);
        y[5 + 304 * 2 + 4 * 99] = NAN;
        r = frames(y, 2, 0, 2, 0);
        CHECK(r.size() == 1 && r[0].n_bad == 0 && r[0].n_fixed <= 2);
    }
    // the neighbour rule over lists: near = 2 h
    {
        using L = std::vector<long>;
        CHECK(kept({}, 0, 100, 8) == L{} && kept({{50, 0, 1.0f}}, 50, 51, 8) == L{50} && kept({{50, 0, 1.0f}}, 51, 100, 8) == L{});
        CHECK((kept({{50, 0, 2.0f}, {66, 0, 1.0f}}, 0, 100, 8) == L{50, 66}) && kept({{50, 0, 2.0f}, {65, 0, 1.0f}}, 0, 100, 8) == L{50});
        CHECK(kept({{50, 0, 1.0f}, {65, 0, 2.0f}}, 0, 100, 8) == L{65} && kept({{50, 1, 9.0f}, {51, 0, 1.0f}, {52, 1, 9.0f}}, 0, 100, 8) == L{51});
        CHECK(kept({{50, 0, 1.0f}, {51, 0, 1.0f}, {52, 0, 1.0f}}, 0, 100, 1) == L{50} && (kept({{50, 0, 1.0f}, {52, 0, 1.0f}}, 0, 100, 1) == L{50, 52}));
        CHECK(kept({{49, 0, 2.0f}, {50, 0, 1.0f}}, 50, 100, 1) == L{} && (kept({{48, 0, 2.0f}, {50, 0, 1.0f}}, 50, 100, 1) == L{50}));
    }
    const Reach w = reach_of(100, 200, 10000000, 12), e = reach_of(0, 10, 10, 12), t = reach_of(99990, 100000, 100000, 1);
    CHECK(w.e0 == 77 && w.e1 == 223 && w.need_lo == 77 && w.need_hi == 222 + reach(12) && reach(12) == 71232);
    CHECK(e.e0 == 0 && e.e1 == 10 && e.need_hi == 10 && t.e0 == 99989 && t.e1 == 100000 && t.need_hi == 100000);
    if (fails) return 1;
    printf("flex_host: ok\n");
    return 0;
}

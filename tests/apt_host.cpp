// apt_host.cpp — pss_apt.h with the host compiler alone (no HIP), as a program of its own under AddressSanitizer and UBSan
// (tests/test_apt_golden.py builds and runs it).  Every row lives in a heap buffer of exactly its size, so a strobe or a word read outside
// the row is an error the sanitizer reports.  The candidate test, the one-record rule through pss_starts.h's keep_starts (the neighbour
// loop of pss_h_apt_syncs), the line gather at positions far outside the row, the plan and the front's output are run on hand-made rows.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "pss_apt.h"
#include "pss_starts.h"

using namespace pss_apt;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("apt_host: line %d: %s\n", __LINE__, #c);         \
            fails++;                                                 \
        }                                                            \
    } while (0)

// a row of exactly n samples at `low` with the 39-word pattern (bit k of `pattern`: word k) from `at`: a high word is high at its middle
// sample alone, so the starts one sample either side read 39 low words
static std::vector<float> row_of(long n, long at, uint64_t pattern, float high, float low)
{
    std::vector<float> e((size_t)n, low);
    for (int k = 0; k < SYNC_WORDS; k++)
        for (int u = 0; u < ENV_SPW; u++) {
            const long i = at + ENV_SPW * k + u;
            if (i >= 0 && i < n) e[(size_t)i] = ((pattern >> k) & 1u) && u == 1 ? high : low;
        }
    return e;
}

struct Rec { long s; float q; int mism; };
static std::vector<Rec> syncs(const std::vector<float> &e, int sync_errors, long s_begin, long s_end)
{
    const long n = (long)e.size();
    std::vector<Rec> acc, out;
    for (long s = 0; s < n; s++) {
        if (!exists(s, n)) continue;
        Rec c;
        if (!candidate([&](int k) { return e.at((size_t)(s + ENV_SPW * k + 1)); }, sync_errors, c.mism, c.q)) continue;
        c.s = s;
        acc.push_back(c);
    }
    pss_starts::keep_starts(acc.data(), acc.size(), s_begin, s_end, NEAR,
        [&](const Rec &b, const Rec &a) { return drops(b.s, b.mism, b.q, a.s, a.mism, a.q); }, [&](const Rec &a) { out.push_back(a); });
    return out;
}

int main()
{
    // ---- the patterns
    CHECK(SYNC_A == 0x33333330ull && popcount64(SYNC_A) == 14 && popcount64(SYNC_A ^ SYNC_B) == weight64(SYNC_A ^ SYNC_B));
    CHECK(popcount64(~0ull) == 64 && popcount64(0) == 0 && popcount64(1ull << 63) == 1);
    // ---- the plan
    int D, up, down;
    CHECK(plan(2400000, D, up, down) && D == 38 && up == 247 && down == 250);
    CHECK(plan(2048000, D, up, down) && D == 32 && up == 39 && down == 40);
    CHECK(plan(240000, D, up, down) && D == 3 && up == 39 && down == 50);
    CHECK(plan(10000000, D, up, down) && D == 160 && up == 624 && down == 625);
    CHECK(plan(62400, D, up, down) && D == 1 && up == 1 && down == 1);
    CHECK(!plan(1000003, D, up, down));
    // ---- one sync in a row that ends right behind its reach: the last candidate of the row
    {
        const long at = 50, n = at + REACH;
        const std::vector<float> e = row_of(n, at, SYNC_A, 1.0f, 0.25f);
        CHECK(exists(at, n) && !exists(at + 1, n) && !exists(-1, n) && !exists(0, REACH - 1) && exists(0, REACH));
        const std::vector<Rec> r = syncs(e, 0, 0, n);
        CHECK(r.size() == 1 && r[0].s == at && r[0].mism == 0 && r[0].q == 0.75f);
        CHECK(syncs(e, 4, 0, at).empty() && syncs(e, 4, at + 1, n).empty() && syncs(e, 4, at, at + 1).size() == 1);
        CHECK(syncs(row_of(n, at, SYNC_B, 1.0f, 0.25f), 4, 0, n).empty());
        CHECK(syncs(std::vector<float>(REACH - 1, 1.0f), 4, 0, REACH - 1).empty());
    }
    // ---- non-finite strobes: a NaN threshold and an infinite one leave 14 mismatches
    {
        const long at = 7, n = at + REACH + 9;
        std::vector<float> e = row_of(n, at, SYNC_A, 1.0f, 0.25f);
        int mism;
        float q;
        e[(size_t)(at + ENV_SPW * 10 + 1)] = std::numeric_limits<float>::quiet_NaN();
        CHECK(!candidate([&](int k) { return e.at((size_t)(at + ENV_SPW * k + 1)); }, 4, mism, q) && mism == 14);
        e[(size_t)(at + ENV_SPW * 10 + 1)] = std::numeric_limits<float>::infinity();
        CHECK(!candidate([&](int k) { return e.at((size_t)(at + ENV_SPW * k + 1)); }, 4, mism, q) && mism == 14);
        e = row_of(n, at, SYNC_A, 1.0f, 0.25f);
        e[(size_t)(at + ENV_SPW * 36 + 1)] = std::numeric_limits<float>::quiet_NaN();   // outside k = 4 .. 31: a low word, compares false
        CHECK(candidate([&](int k) { return e.at((size_t)(at + ENV_SPW * k + 1)); }, 0, mism, q) && mism == 0 && q == 0.75f);
        e[(size_t)(at + ENV_SPW * 2 + 1)] = std::numeric_limits<float>::infinity();      // a low word that reads high
        CHECK(candidate([&](int k) { return e.at((size_t)(at + ENV_SPW * k + 1)); }, 1, mism, q) && mism == 1);
    }
    // ---- the one-record rule: fewer mismatches first, then the score, then the earlier start; NEAR away is no neighbour
    {
        CHECK(drops(10, 0, 0.1f, 20, 2, 9.0f) && !drops(20, 2, 9.0f, 10, 0, 0.1f));
        CHECK(drops(10, 1, 0.5f, 20, 1, 0.25f) && !drops(20, 1, 0.25f, 10, 1, 0.5f));
        CHECK(drops(10, 1, 0.5f, 20, 1, 0.5f) && !drops(20, 1, 0.5f, 10, 1, 0.5f) && !drops(10, 1, 0.5f, 10, 1, 0.5f));
        CHECK(drops(10, 0, 1.0f, 10 + NEAR - 1, 0, 0.5f) && !drops(10, 0, 1.0f, 10 + NEAR, 0, 0.5f));
        const float nan = std::numeric_limits<float>::quiet_NaN();
        CHECK(!drops(10, 0, nan, 20, 0, 0.5f) && !drops(20, 0, 0.5f, 10, 0, nan));
        // two equal syncs 117 apart and a stronger one NEAR - 1 behind the second
        const long n = 6000;
        std::vector<float> e = row_of(n, 100, SYNC_A, 1.0f, 0.25f);
        for (long at : {217l, 217l + NEAR - 1})
            for (int k = 0; k < SYNC_WORDS; k++)
                e[(size_t)(at + ENV_SPW * k + 1)] = ((SYNC_A >> k) & 1u) ? (at == 217 ? 1.0f : 2.0f) : 0.25f;
        const std::vector<Rec> r = syncs(e, 0, 0, n);
        CHECK(r.size() == 2 && r[0].s == 100 && r[1].s == 217 + NEAR - 1);
        const std::vector<Rec> w = syncs(e, 0, 200, 300);   // the window holds the dropped one alone: its neighbours outside still count
        CHECK(w.empty());
    }
    // ---- lines: positions far outside the row read +0 and nothing else; no sum overflows
    {
        const long n = 7000;
        std::vector<float> e((size_t)n);
        for (long i = 0; i < n; i++) e[(size_t)i] = (float)(i + 1);
        auto E = [&](long i) { return e.at((size_t)i); };
        CHECK(line_word(E, 0, 0, n) == 2.0f && line_word(E, 0, LINE_WORDS - 1, n) == (float)(3 * 2079 + 2));
        CHECK(line_word(E, -1, 0, n) == 1.0f && line_word(E, -2, 0, n) == 0.0f && !std::signbit(line_word(E, -2, 0, n)));
        CHECK(line_word(E, n - 2, 0, n) == (float)n && line_word(E, n - 1, 0, n) == 0.0f && line_word(E, n, 0, n) == 0.0f);
        for (long p : {std::numeric_limits<long>::min(), std::numeric_limits<long>::max(), -(long)LINE_ENV, (long)-LINE_ENV + 1, n + 5})
            for (int j : {0, 1, LINE_WORDS - 1}) CHECK(line_word(E, p, j, n) == 0.0f);
        CHECK(line_word(E, -(long)LINE_ENV + 2, LINE_WORDS - 1, n) == 1.0f);
        CHECK(line_word(E, 0, 0, 0) == 0.0f);
    }
    // ---- the window's reach
    {
        const Reach r = reach_of(5000, 6000, 100000);
        CHECK(r.e0 == 5000 - 3119 && r.e1 == 6000 + 3119 && r.need_lo == r.e0 && r.need_hi == r.e1 - 1 + 117);
        const Reach c = reach_of(0, 50, 60);
        CHECK(c.e0 == 0 && c.e1 == 60 && c.need_hi == 60);
    }
    // ---- the front's output: one tap of 1 hands back |z|; 79 taps against a plain double loop
    {
        const int T = 79, lead = 39, Dd = 5;
        std::vector<double> h((size_t)T), zr(400), zi(400);
        for (int k = 0; k < T; k++) h[(size_t)k] = 1.0 / (1.0 + k);
        for (int i = 0; i < 400; i++) { zr[(size_t)i] = sin(0.1 * i); zi[(size_t)i] = cos(0.37 * i); }
        auto Z = [&](long i, double &vr, double &vi) {
            const bool in = i >= 0 && i < 400;
            vr = in ? zr.at((size_t)i) : 0.0;
            vi = in ? zi.at((size_t)i) : 0.0;
        };
        const double one = 1.0;
        CHECK(output(3, 1, &one, 1, 0, Z) == (float)sqrt(fma(zr[3], zr[3], zi[3] * zi[3])));
        for (long m : {0l, 1l, 40l, 79l}) {
            double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;   // the two blocks of 64 and 15 taps, each a chain from +0
            for (int k = 0; k < T; k++) {
                double vr, vi;
                Z(m * Dd + lead - k, vr, vi);
                if (k < 64) { ar = fma(h[(size_t)k], vr, ar); ai = fma(h[(size_t)k], vi, ai); }
                else { br = fma(h[(size_t)k], vr, br); bi = fma(h[(size_t)k], vi, bi); }
            }
            const double re = ar + br, im = ai + bi;
            CHECK(output(m, Dd, h.data(), T, lead, Z) == (float)sqrt(fma(re, re, im * im)));
        }
    }
    if (fails) return 1;
    printf("apt_host: ok\n");
    return 0;
}

// pocsag_host.cpp — pss_pocsag.h with the host compiler alone (no HIP), as a program of its own under AddressSanitizer and UBSan
// (tests/test_pocsag_golden.py builds and runs it).  Every row lives in a heap buffer of exactly its size, so a strobe read outside the row
// is an error the sanitizer reports.  The 1024-entry table is held to a brute-force search over every pattern of weight 1 and 2, and the
// one-record rule runs through pss_starts.h's keep_starts (the neighbour loop of pss_h_pocsag_batches) over hand-made lists.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pss_pocsag.h"
#include "pss_starts.h"

using namespace pss_pocsag;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("pocsag_host: line %d: %s\n", __LINE__, #c);        \
            fails++;                                                    \
        }                                                               \
    } while (0)

// the remainder by long division, one bit at a time, written again
static uint32_t slow_syndrome(uint32_t cw)
{
    uint32_t reg = 0;
    for (int i = 31; i >= 1; i--) {
        reg = (reg << 1) | ((cw >> i) & 1u);
        if (reg & 0x400u) reg ^= GEN;
    }
    return reg;
}

// sync word and 16 codewords at the strobes of a row of exactly n samples, the first strobe at `at`
static std::vector<float> row_of(const uint32_t *words17, int spb, long at, long n, bool inverted)
{
    std::vector<float> y((size_t)n, 0.0f);
    for (int w = 0; w < 17; w++)
        for (int k = 0; k < 32; k++) {
            const long j = at + (long)spb * (32 * w + k);
            const bool one = ((words17[w] >> (31 - k)) & 1u) != 0;
            if (j >= 0 && j < n) y[(size_t)j] = (one != inverted) ? -1.0f : 1.0f;
        }
    return y;
}

struct Rec { long s; float q; uint32_t meta; uint32_t cw[N_CW]; uint8_t fix[N_CW]; };
static std::vector<Rec> batches(const std::vector<float> &y, int spb, int sync_errors, int fix, int max_bad)
{
    const long n = (long)y.size();
    std::vector<Rec> out;
    for (long s = 0; s < n; s++) {
        if (!exists(s, n, spb)) continue;
        auto Y = [&](int k) { return y.at((size_t)(s + (long)spb * k)); };
        float thr;
        int mism;
        bool inv;
        Rec c;
        if (!candidate(Y, sync_errors, thr, c.q, mism, inv)) continue;
        c.s = s;
        int n_bad = 0, n_fixed = 0;
        for (int j = 0; j < N_CW; j++) {
            const int m = check(received(Y, thr, inv, j), fix, c.cw[j]);
            c.fix[j] = (uint8_t)(m < 0 ? UNCORRECTABLE : m);
            if (m < 0) n_bad++;
            else n_fixed += m;
        }
        c.meta = meta_of(mism, inv, n_bad, n_fixed);
        if (n_bad <= max_bad) out.push_back(c);
    }
    return out;
}

struct Start { long s; float q; };
static std::vector<long> kept(const std::vector<Start> &list, long s_begin, long s_end, int spb)
{
    const std::vector<Start> heap(list.begin(), list.end());   // exactly list.size() records
    std::vector<long> out;
    pss_starts::keep_starts(
        heap.data(), heap.size(), s_begin, s_end, spb, [&](const Start &b, const Start &a) { return drops(true, b.s, b.q, a.s, a.q, spb); },
        [&](const Start &a) { out.push_back(a.s); });
    return out;
}

int main()
{
    // the code: the sync and idle words, an address word, the syndrome against long division
    CHECK(codeword(SYNC >> 11) == SYNC && codeword(IDLE >> 11) == IDLE);
    CHECK(codeword((1234567u >> 3) << 2 | 3u) == 0x4B5A1A25u && (1234567u & 7u) == 7u);
    for (uint32_t d = 0; d < (1u << 21); d += 997) {
        const uint32_t cw = codeword(d);
        CHECK(syndrome(cw) == 0 && slow_syndrome(cw) == 0 && (popcount32(cw) & 1) == 0 && (cw >> 11) == d);
        CHECK(syndrome(cw ^ (d * 2654435761u)) == slow_syndrome(cw ^ (d * 2654435761u)));
    }
    // the table against brute force: every syndrome's entry is the one pattern of weight <= 2 in bits 31 .. 1 with that syndrome, or 0
    {
        int found = 0;
        for (uint32_t S = 0; S < 1024; S++) {
            uint32_t pat = 0;
            int hits = 0;
            for (int i = 1; i < 32; i++) {
                if (slow_syndrome(1u << i) == S) { pat = 1u << i; hits++; }
                for (int j = i + 1; j < 32; j++)
                    if (slow_syndrome((1u << i) | (1u << j)) == S) { pat = (1u << i) | (1u << j); hits++; }
            }
            CHECK(hits <= 1 && TABLE.e[S] == pat && pattern(S) == pat);
            found += hits;
        }
        CHECK(found == 31 + 465 && TABLE.distinct == found && TABLE.e[0] == 0);
    }
    // check: every error of weight 1 and 2 comes back with its count; fix below the count refuses; weight 3 never crashes
    for (uint32_t cw : {SYNC, IDLE, codeword(0x155555u)}) {
        uint32_t out = 1;
        CHECK(check(cw, 0, out) == 0 && out == cw);
        for (int i = 0; i < 32; i++) {
            CHECK(check(cw ^ (1u << i), 2, out) == 1 && out == cw && check(cw ^ (1u << i), 1, out) == 1 && out == cw);
            CHECK(check(cw ^ (1u << i), 0, out) == -1 && out == 0);
            for (int j = i + 1; j < 32; j++) {
                const uint32_t e2 = (1u << i) | (1u << j);
                CHECK(check(cw ^ e2, 2, out) == 2 && out == cw);
                CHECK(check(cw ^ e2, 1, out) == -1 && out == 0);
                for (int k = j + 1; k < 32; k++) {
                    const int n = check(cw ^ e2 ^ (1u << k), 2, out);
                    CHECK(n == -1 || (n >= 0 && out != cw && syndrome(out) == 0 && (popcount32(out) & 1) == 0));
                }
            }
        }
    }
    // the pulse and the plan
    for (int spb = MIN_SPB; spb <= MAX_SPB; spb++) {
        const int P = pulse_len(spb);
        std::vector<double> g((size_t)P);
        default_pulse(spb, g.data());
        CHECK((P & 1) && P <= spb && P <= MAX_PULSE && (P + 2 > spb || P == MAX_PULSE) && g[0] == 1.0 / P && g[(size_t)P - 1] == g[0]);
    }
    int D, up, down;
    CHECK(plan(2400000, D, up, down) && D == 62 && up == 124 && down == 125);
    CHECK(plan(250000, D, up, down) && D == 6 && up == 576 && down == 625);
    CHECK(plan(38400, D, up, down) && D == 1 && up == 1 && down == 1);
    CHECK(!plan(1000003, D, up, down));
    // a batch at the row's first start and ending on its last sample; one sample shorter: no start
    uint32_t words[17] = {SYNC};
    for (int j = 0; j < 16; j++) words[j + 1] = j & 1 ? IDLE : codeword(0x100000u | (uint32_t)(j * 0x1357u));
    for (int spb : {2, 16, 75, 128})
        for (bool inverted : {false, true}) {
            const long n = (long)LAST_K * spb + 1;
            CHECK(n == reach(spb));
            const std::vector<Rec> r = batches(row_of(words, spb, 0, n, inverted), spb, 0, 0, 0);
            CHECK(r.size() == 1 && r[0].s == 0 && r[0].q == 1.0f && r[0].meta == meta_of(0, inverted, 0, 0));
            if (r.size() == 1)
                for (int j = 0; j < 16; j++) CHECK(r[0].cw[j] == words[j + 1] && r[0].fix[j] == 0);
            CHECK(batches(row_of(words, spb, 0, n - 1, inverted), spb, 2, 2, 16).empty());
            // somewhere inside a longer row, with two wrong bits in one word, one in another and one in the sync word
            uint32_t hurt[17];
            memcpy(hurt, words, sizeof(hurt));
            hurt[0] ^= 0x00010000u;
            hurt[3] ^= 0x80000001u;
            hurt[9] ^= 0x00000400u;
            const std::vector<float> y = row_of(hurt, spb, 37, n + 50, inverted);
            const std::vector<Rec> h = batches(y, spb, 1, 2, 0);
            CHECK(h.size() == 1 && h[0].s == 37 && h[0].meta == meta_of(1, inverted, 0, 3) && h[0].fix[2] == 2 && h[0].fix[8] == 1 && h[0].cw[2] == words[3]);
            CHECK(batches(y, spb, 0, 2, 0).empty() && batches(y, spb, 1, 1, 0).empty());
            const std::vector<Rec> b = batches(y, spb, 1, 1, 1);
            CHECK(b.size() == 1 && b[0].fix[2] == UNCORRECTABLE && b[0].cw[2] == 0 && b[0].meta == meta_of(1, inverted, 1, 1));
        }
    // a NaN among the sync strobes fails the test; an inf as well
    {
        std::vector<float> y = row_of(words, 4, 0, reach(4), false);
        y[8] = NAN;
        CHECK(batches(y, 4, 2, 2, 16).empty());
        y[8] = INFINITY;
        CHECK(batches(y, 4, 2, 2, 16).empty());
    }
    // the neighbour rule over lists: near = spb
    {
        using L = std::vector<long>;
        CHECK(kept({}, 0, 100, 16) == L{} && kept({{50, 1.0f}}, 50, 51, 16) == L{50} && kept({{50, 1.0f}}, 51, 100, 16) == L{});
        CHECK((kept({{50, 2.0f}, {66, 1.0f}}, 0, 100, 16) == L{50, 66}) && kept({{50, 2.0f}, {65, 1.0f}}, 0, 100, 16) == L{50});
        CHECK(kept({{50, 1.0f}, {65, 2.0f}}, 0, 100, 16) == L{65} && kept({{50, 1.0f}, {51, 1.0f}, {52, 1.0f}}, 0, 100, 16) == L{50});
        CHECK(kept({{49, 2.0f}, {50, 1.0f}}, 50, 100, 2) == L{} && (kept({{49, 2.0f}, {51, 1.0f}}, 50, 100, 2) == L{51}));
    }
    CHECK(drops(true, 9, 1.0f, 10, 1.0f, 2) && !drops(true, 11, 1.0f, 10, 1.0f, 2) && !drops(true, 8, 2.0f, 10, 1.0f, 2) && !drops(false, 9, 2.0f, 10, 1.0f, 2));
    const Reach w = reach_of(100, 200, 1000000, 32), e = reach_of(0, 10, 10, 32), t = reach_of(99990, 100000, 100000, 2);
    CHECK(w.e0 == 69 && w.e1 == 231 && w.need_lo == 69 && w.need_hi == 230 + reach(32));
    CHECK(e.e0 == 0 && e.e1 == 10 && e.need_hi == 10 && t.e0 == 99989 && t.e1 == 100000 && t.need_hi == 100000);
    if (fails) return 1;
    printf("pocsag_host: ok\n");
    return 0;
}

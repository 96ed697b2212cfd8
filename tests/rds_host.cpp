// rds_host.cpp — pss_rds.h with the host compiler alone (the header must not need HIP), built with -fsanitize=address,undefined and run as a
// program of its own by tests/test_rds_golden.py.  It walks the index arithmetic of the three stages at the edge shapes: every accessor
// checks its index, the strobes of the closed form are held against the rule applied one strobe at a time, and the block check against
// hand-made rows.  Prints "rds_host: ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pss_rds.h"

using namespace pss_rds;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            printf("rds_host: FAILED %s (line %d)\n", #c, __LINE__);         \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static uint32_t rng_state = 12345;
static float rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((int32_t)rng_state) * (1.0f / 2147483648.0f);
}

// the front of one row, outputs [m0, m1), from a buffer that holds row samples [lo, hi)
static std::vector<float> front(const std::vector<float> &x, long n, long lo, long hi, uint64_t w, int D, const std::vector<double> &h, int lead, long m0, long m1,
                                const double *knots)
{
    const int T = (int)h.size();
    std::vector<float> y(2 * (size_t)(m1 - m0));
    for (long m = m0; m < m1; m++)
        pss_dc::output(m, D, h.data(), T, lead, [&](long i, double &zr, double &zi) {
            CHECK(i >= m * D + lead - (T - 1) && i <= m * D + lead);
            zr = zi = 0.0;
            if (i < 1 || i >= n) return;
            CHECK(i - 1 >= lo && i < hi);    // a window that holds its halo and one sample more is enough
            const float *c = &x[2 * (size_t)(i - lo)];
            mixed(disc(c[0], c[1], c[-2], c[-1], [](float im, float re) { return atan2f(im, re); }), pss_dc::phase_of(w, i), knots, zr, zi);
        }, y[2 * (m - m0)], y[2 * (m - m0) + 1]);
    return y;
}

static void test_front()
{
    std::vector<double> knots(2 * pss_dc::KNOTS);
    pss_dc::build_knots(knots.data());
    const uint64_t w = pss_dc::word_of(57000.0, 240000.0);
    const long n = 301;
    std::vector<float> x(2 * n);
    for (auto &v : x) v = rnd();
    for (int D : {1, 3, 12})
        for (int T : {1, D, 20 * D + 1}) {
            std::vector<double> h(T);
            for (auto &v : h) v = rnd();
            const int lead = (T - 1) / 2;
            const long n_out = pss_dc::out_len(n, D);
            const std::vector<float> whole = front(x, n, 0, n, w, D, h, lead, 0, n_out, knots.data());
            for (long m0 = 0; m0 < n_out; m0 += 7) {      // windows with exactly their halo and the discriminator's one sample more
                const long m1 = m0 + 7 < n_out ? m0 + 7 : n_out;
                long lo = m0 * D + lead - (T - 1) - 1, hi = (m1 - 1) * D + lead + 1;
                lo = lo < 0 ? 0 : lo;
                hi = hi > n ? n : hi;
                std::vector<float> part(x.begin() + 2 * lo, x.begin() + 2 * hi);
                const std::vector<float> y = front(part, n, lo, hi, w, D, h, lead, m0, m1, knots.data());
                for (size_t k = 0; k < y.size(); k++) CHECK(y[k] == whole[2 * m0 + k]);
            }
        }
    int D, up, down;
    CHECK(plan(240000, D, up, down) && D == 12 && up == 19 && down == 20);
    CHECK(plan(10000000, D, up, down) && D == 204 && up == 969 && down == 2500);
    CHECK(!plan(1000003, D, up, down));
}

static void test_bits()
{
    double p[MAX_PULSE];
    default_pulse(4, p);
    const int P = pulse_len(4);
    CHECK(P == 65 && p[32] == 0.0);
    for (int u = 0; u < P; u++) CHECK(p[u] == -p[P - 1 - u]);
    default_pulse(MAX_SPAN, p);
    default_pulse(4, p);
    for (long n : {0l, 1l, 15l, 16l, 17l, 40l, 1023l, 1024l, 1025l, 9l * 1024 - 1, 9l * 1024, 9l * 1024 + 1}) {
        std::vector<float> x(2 * (size_t)n + 2);
        for (auto &v : x) v = rnd();
        auto Bx = [&](long i, float &br, float &bi) {
            CHECK(i >= 0 && i < n);
            br = x[2 * i];
            bi = x[2 * i + 1];
        };
        const int n_seg = n_segments(n);
        CHECK((long)n_seg * SEG >= n && (long)(n_seg - 1) * SEG < n + (n == 0));
        std::vector<double> E((size_t)n_seg * SPB + 1);
        for (int s = 0; s < n_seg; s++)
            for (int o = 0; o < SPB; o++) E[(size_t)s * SPB + o] = seg_energy(Bx, n, p, P, s, o);
        for (int s = 0; s < n_seg; s++) {
            const int o = seg_offset(E.data(), n_seg, s);
            CHECK(o >= 0 && o < SPB);
        }
    }
    // a NaN never wins and never blocks: slot 0 holding one keeps offset 0, another slot holding one is passed over
    {
        std::vector<double> E(SPB, 1.0);
        E[5] = 3.0;
        E[7] = NAN;
        CHECK(seg_offset(E.data(), 1, 0) == 5);
        E[0] = NAN;
        CHECK(seg_offset(E.data(), 1, 0) == 0);
    }
    // the strobes of every pair of offsets against the rule applied one strobe at a time
    for (long n : {1024l + 1, 1024l + 9, 1024l + 16, 1024l + 40, 2048l, 2048l + 700})
        for (int a = 0; a < SPB; a++)
            for (int b = 0; b < SPB; b++) {
                std::vector<long> want;
                long last = -1;
                for (int s = 0; s < 2; s++) {
                    const int o = s ? b : a;
                    const long j1 = (long)(s + 1) * SEG < n ? (long)(s + 1) * SEG : n;
                    bool first = true;
                    for (long j = (long)s * SEG + o; j < j1; j += SPB) {
                        if (s && first) {
                            first = false;
                            if (j - last < 8) continue;
                            if (j - last > 24) want.push_back(last + 16);
                        }
                        want.push_back(j);
                        last = j;
                    }
                }
                std::vector<long> got;
                for (int s = 0; s < 2; s++) {
                    const Strobes st = seg_strobes(s, a, s ? b : a, n);
                    for (int k = 0; k < strobes_total(st); k++) got.push_back(strobe_at(st, k));
                    if (s) CHECK(last_of_prev(1, a) == SEG - SPB + a);
                }
                CHECK(got == want);
                for (size_t k = 0; k < got.size(); k++) {
                    CHECK(got[k] >= 0 && got[k] < n);
                    if (k) CHECK(got[k] - got[k - 1] >= 8 && got[k] - got[k - 1] <= 24);
                }
            }
    CHECK(data_bit(1.0, 0.0, -1.0, 0.0) == 1 && data_bit(1.0, 1.0, 1.0, 0.5) == 0 && data_bit(NAN, 0.0, 1.0, 0.0) == 0);
}

static void put_block(std::vector<uint8_t> &bits, size_t at, uint32_t info, uint32_t offset)
{
    const uint32_t w = (info << 10) | (checkword(info) ^ offset);
    for (int k = 0; k < BLOCK; k++) bits[at + k] = (w >> (25 - k)) & 1u;
}

static void test_groups()
{
    CHECK(checkword(0) == 0 && checkword(1) == (POLY & 0x3FF));
    const uint32_t a = 0x54A8, b_a = 0x0408, b_b = 0x2C10, c = 0xE0CD, d = 0x5053;
    for (int version_b = 0; version_b < 2; version_b++) {
        std::vector<uint8_t> bits(7 + GROUP, 0);
        const uint32_t b = version_b ? b_b : b_a;
        put_block(bits, 7, a, OFF_A);
        put_block(bits, 7 + BLOCK, b, OFF_B);
        put_block(bits, 7 + 2 * BLOCK, c, version_b ? OFF_CP : OFF_C);
        put_block(bits, 7 + 3 * BLOCK, d, OFF_D);
        uint16_t g[4];
        int hits = 0;
        for (long i = 0; i + GROUP <= (long)bits.size(); i++)
            if (group_at(bits.data(), i, g)) {
                hits++;
                CHECK(i == 7 && g[0] == a && g[1] == b && g[2] == c && g[3] == d);
            }
        CHECK(hits == 1);
        put_block(bits, 7 + 2 * BLOCK, c, version_b ? OFF_C : OFF_CP);   // the other offset word: wrong for this version bit
        CHECK(!group_at(bits.data(), 7, g));
    }
}

int main()
{
    test_front();
    test_bits();
    test_groups();
    printf("rds_host: ok\n");
    return 0;
}

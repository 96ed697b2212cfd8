// ddc_host.cpp — pss_ddc.h on the host, alone: compiled by tests/test_ddc_golden.py with the host compiler and
// -fsanitize=address,undefined, run as a program of its own (never loaded into Python, never on the GPU).  It checks the statement's exact
// identities — word 0 and the quarter turn, the knots at the quarter turns, the identity and quarter-turn filters, the word's rounding —
// walks the filter at the tap counts where an index could leave its array (1, 63, 64, 65, 129 taps; lead 0, middle, last), and checks the
// tile function's promises for every decimation at a sweep of tap counts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pss_ddc.h"

using namespace pss_dc;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

// the down-converter on one thread, exact sizes everywhere: the sanitizer sees the first element past any of them
static std::vector<float> ddc(const std::vector<float> &x, long index0, uint64_t w, int D, const std::vector<double> &h, int lead, const double *knots,
                              long m_begin = 0)
{
    // x holds samples [index0, n_cap) of a capture of n_cap samples; the caller's m_begin skips the outputs that need earlier ones
    const long n = (long)x.size() / 2, n_cap = index0 + n;
    const int T = (int)h.size();
    const long m_end = out_len(n_cap, D);
    std::vector<float> y(2 * (size_t)(m_end - m_begin));
    for (long m = m_begin; m < m_end; m++)
        output(m, D, h.data(), T, lead, [&](long i, double &zr, double &zi) {
            zr = zi = 0.0;
            if (i < 0 || i >= n_cap) return;
            double c, s;
            rotor(phase_of(w, i), knots, c, s);
            mix(x.at(2 * (size_t)(i - index0)), x.at(2 * (size_t)(i - index0) + 1), c, s, zr, zi);
        }, y[2 * (m - m_begin)], y[2 * (m - m_begin) + 1]);
    return y;
}

int main()
{
    std::vector<double> knots(2 * KNOTS);
    build_knots(knots.data());
    // the quarter turns are exact, every knot is on the unit circle to an ulp
    CHECK(knots[0] == 1.0 && knots[1] == 0.0 && knots[2 * 256] == 0.0 && knots[2 * 256 + 1] == 1.0);
    CHECK(knots[2 * 512] == -1.0 && knots[2 * 512 + 1] == 0.0 && knots[2 * 768] == 0.0 && knots[2 * 768 + 1] == -1.0);
    for (int k = 0; k < KNOTS; k++) {
        CHECK(std::fabs(knots[2 * k] * knots[2 * k] + knots[2 * k + 1] * knots[2 * k + 1] - 1.0) < 4e-16);
        CHECK(knots[2 * k] == knots[2 * ((KNOTS - k) % KNOTS)] && knots[2 * k + 1] == -knots[2 * ((KNOTS - k) % KNOTS) + 1]);
        CHECK(!std::signbit(knots[2 * k]) || knots[2 * k] != 0.0);
    }
    // word 0: (1, 0) at any index; word 2^62: (1, 0), (0, -1), (-1, 0), (0, 1)
    const long far[] = {0, 1, 2, 3, 4, 1000003, (1L << 40) + 12345, (1L << 62) - 1, 1L << 62, std::numeric_limits<long>::max()};
    const double qc[4] = {1, 0, -1, 0}, qs[4] = {0, -1, 0, 1};
    for (long i : far) {
        double c, s;
        rotor(phase_of(0, i), knots.data(), c, s);
        CHECK(c == 1.0 && s == 0.0);
        rotor(phase_of(1ull << 62, i), knots.data(), c, s);
        CHECK(c == qc[i & 3] && s == qs[i & 3]);
        rotor(phase_of(1, i), knots.data(), c, s);          // every word stays on the circle
        CHECK(std::fabs(c * c + s * s - 1.0) < 1e-15);
        rotor(phase_of(~0ull, i), knots.data(), c, s);
        CHECK(std::fabs(c * c + s * s - 1.0) < 1e-15);
    }
    // the word: exact fractions, the two ends, ties to even
    CHECK(word_of(0.0, 2.4e6) == 0 && word_of(600e3, 2.4e6) == 1ull << 62 && word_of(-600e3, 2.4e6) == 3ull << 62);
    CHECK(word_of(1.2e6, 2.4e6) == 1ull << 63 && word_of(-1.2e6, 2.4e6) == 1ull << 63);
    CHECK(word_of(0x1p-65, 1.0) == 0 && word_of(0x1.8p-64, 1.0) == 2 && word_of(-0x1p-64, 1.0) == ~0ull);
    CHECK(effective_hz(1ull << 62, 2.4e6) == 600e3 && effective_hz(3ull << 62, 2.4e6) == -600e3 && effective_hz(1ull << 63, 2.4e6) == -1.2e6);
    CHECK(out_len(0, 5) == 0 && out_len(1, 5) == 1 && out_len(5, 5) == 1 && out_len(6, 5) == 2 && out_len(std::numeric_limits<long>::max(), 1) > 0);

    // inputs: ordinary values, float32 subnormals, the largest float32
    const int n = 301;
    std::vector<float> x(2 * n);
    unsigned seed = 12345;
    for (auto &v : x) {
        seed = seed * 1664525u + 1013904223u;
        v = (float)((int)(seed >> 8) % 20001 - 10000) / 8192.0f;
    }
    const std::vector<float> plain = x;
    for (int i = 0; i < 2 * n; i += 7) x[i] = 1e-41f * (float)(1 + i);
    x[11] = std::numeric_limits<float>::max();
    x[14] = -std::numeric_limits<float>::min();
    const std::vector<double> one{1.0};
    for (long index0 : {0L, 1L, 2L, 3L, (1L << 40) + 12345}) {
        // identity: D = 1, taps {1}, lead 0, word 0
        auto y = ddc(x, index0, 0, 1, one, 0, knots.data(), index0);
        CHECK(y.size() == x.size());
        for (size_t i = 0; i < y.size() && i < x.size(); i++) CHECK(y[i] == x[i]);
        // quarter turn: output i = x[i] (-j)^i, i the index in the capture
        y = ddc(x, index0, 1ull << 62, 1, one, 0, knots.data(), index0);
        for (long i = 0; i < n; i++) {
            const float xr = x[2 * i], xi = x[2 * i + 1];
            const float er[4] = {xr, xi, -xr, -xi}, ei[4] = {xi, -xr, -xi, xr};
            CHECK(y[2 * i] == er[(index0 + i) & 3] && y[2 * i + 1] == ei[(index0 + i) & 3]);
        }
    }
    // the filter at the block edges against a plain long double sum (the error of a 129-term fma chain stays far below 1e-12 here)
    for (int T : {1, 2, 63, 64, 65, 128, 129})
        for (int D : {1, 2, 3, 7, 64})
            for (int lead : {0, (T - 1) / 2, T - 1}) {
                std::vector<double> h(T);
                for (int k = 0; k < T; k++) h[k] = std::cos(0.37 * k) / T;
                const uint64_t w = 0x243f6a8885a308d3ull;
                const auto y = ddc(plain, 0, w, D, h, lead, knots.data());
                CHECK((long)y.size() == 2 * out_len(n, D));
                for (long m = 0; m < (long)y.size() / 2; m++) {
                    long double ar = 0, ai = 0;
                    for (int k = 0; k < T; k++) {
                        const long i = m * D + lead - k;
                        if (i < 0 || i >= n) continue;
                        double c, s, zr, zi;
                        rotor(phase_of(w, i), knots.data(), c, s);
                        mix(plain[2 * i], plain[2 * i + 1], c, s, zr, zi);
                        ar += (long double)h[k] * zr;
                        ai += (long double)h[k] * zi;
                    }
                    CHECK(std::fabs(y[2 * m] - (double)ar) < 1e-5 && std::fabs(y[2 * m + 1] - (double)ai) < 1e-5);
                }
            }
    // the tile: at least one output, the staged span and the block sums fit, and one more output would not
    for (int D = 1; D <= MAX_DECIM; D++)
        for (int T : {1, 2, 63, 64, 65, 129, 1001, 4001, 4096, 4097, 20 * D + 1}) {
            if (T > MAX_TAPS) continue;
            const int M = tile_outputs(D, T);
            CHECK(M >= 1 && M * n_blocks(T) <= PART_CAP);
            CHECK(M == 1 ? T <= STAGE_CAP : (long)D * tile_row(M, D, T) <= STAGE_CAP && (M - 1 + (T + D - 1) / D) <= tile_row(M, D, T));
            CHECK((M + 1) * n_blocks(T) > PART_CAP || (long)D * tile_row(M + 1, D, T) > STAGE_CAP);
        }
    if (failures) return 1;
    std::printf("ddc_host: ok\n");
    return 0;
}

// pfb_host.cpp — pss_pfb.h on the host, alone: compiled by tests/test_pfb_golden.py with the host compiler and
// -fsanitize=address,undefined, run as a program of its own (never loaded into Python, never on the GPU).  It checks the statement's index
// functions (first tap, bit reversal, the butterflies of a stage and their knots, the tile), the exact identities (one tap: the DFT of M
// consecutive samples; M = 2 and 4: sums and differences), and walks the bank at the tap counts and decimations where an index could
// leave its array (T = 1, M - 1, M, M + 1, 32 M; D = 1, 3, M / 2, M; lead 0, middle, last; a buffer far into a long capture) against
// the definition in long double.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pss_pfb.h"

using namespace pss_pf;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

// the bank on one thread, exact sizes everywhere: the sanitizer sees the first element past any of them.  x holds samples
// [index0, n_cap) of a capture of n_cap samples; outputs [m_begin, out_len) -> [instant][channel] complex64
static std::vector<float> bank(const std::vector<float> &x, long index0, int M, int D, const std::vector<double> &h, int lead, const double *knots,
                               long m_begin = 0)
{
    const long n = (long)x.size() / 2, n_cap = index0 + n;
    const long m_end = pss_dc::out_len(n_cap, D);
    std::vector<float> y(2 * (size_t)M * (size_t)(m_end - m_begin));
    std::vector<double> vr(M), vi(M);
    for (long m = m_begin; m < m_end; m++)
        instant(m, M, D, h.data(), (int)h.size(), lead, knots, [&](long j, float &xr, float &xi) {
            xr = xi = 0.0f;
            if (j < index0 || j >= n_cap) return;
            xr = x.at(2 * (size_t)(j - index0));
            xi = x.at(2 * (size_t)(j - index0) + 1);
        }, vr.data(), vi.data(), y.data() + 2 * (size_t)M * (size_t)(m - m_begin));
    return y;
}

int main()
{
    std::vector<double> knots(2 * pss_dc::KNOTS);
    pss_dc::build_knots(knots.data());
    // the index functions
    CHECK(chan_ok(2) && chan_ok(1024) && !chan_ok(1) && !chan_ok(0) && !chan_ok(-4) && !chan_ok(48) && !chan_ok(2048));
    CHECK(log2_of(2) == 1 && log2_of(64) == 6 && log2_of(1024) == 10);
    CHECK(first_tap(0, 0, 8) == 0 && first_tap(0, 1, 8) == 7 && first_tap(13, 5, 8) == 0 && first_tap(13, 6, 8) == 7 && first_tap(5, 1023, 1024) == 6);
    CHECK(first_tap(((int64_t)1 << 40) + 12345, 7, 1024) == (12345 - 7) % 1024 && first_tap(std::numeric_limits<int64_t>::max(), 0, 1024) == 1023);
    for (int M = 2; M <= MAX_CHAN; M *= 2) {
        const int lb = log2_of(M);
        std::vector<int> seen(M, 0);
        for (int r = 0; r < M; r++) {
            const int q = bitrev(r, lb);
            CHECK(q >= 0 && q < M && bitrev(q, lb) == r);
            seen.at(q)++;
        }
        for (int v : seen) CHECK(v == 1);
        for (int ls = 0; ls < lb; ls++) {                       // every stage touches every element once, and its knots are in the table
            std::vector<int> hit(M, 0);
            for (int i = 0; i < M / 2; i++) {
                const int a = fly_a(i, ls), kn = fly_knot(i, ls);
                hit.at(a)++;
                hit.at(a + (1 << ls))++;
                CHECK(kn >= 0 && kn < pss_dc::KNOTS / 2 && kn * (2 << ls) == (a & ((1 << ls) - 1)) * pss_dc::KNOTS);
            }
            for (int v : hit) CHECK(v == 1);
        }
        CHECK(tile_instants(M) * M == TILE_ELEMS && tile_instants(M) >= 8 && tile_instants(M) * tile_row(M) <= TILE_SLOTS);
        CHECK(M < PAD_FROM || (tile_row(M) & 1));
    }
    // inputs: small integers over 256 (every sum below is exact), then ordinary values with float32 subnormals and the largest float32
    const int n = 301;
    std::vector<float> x(2 * n), plain(2 * n);
    unsigned seed = 12345;
    for (int i = 0; i < 2 * n; i++) {
        seed = seed * 1664525u + 1013904223u;
        x[i] = (float)((int)(seed >> 8) % 513 - 256) / 256.0f;
        seed = seed * 1664525u + 1013904223u;
        plain[i] = (float)((int)(seed >> 8) % 20001 - 10000) / 8192.0f;
    }
    // M = 2, one tap, D = 1: y_0[m] = x[m], y_1[m] = x[m] (-1)^m — whichever branch holds the sample
    {
        const auto y = bank(x, 0, 2, 1, {1.0}, 0, knots.data());
        CHECK((long)y.size() == 2 * 2 * n);
        for (long m = 0; m < n; m++) {
            const float s = m & 1 ? -1.0f : 1.0f;
            CHECK(y[4 * m] == x[2 * m] && y[4 * m + 1] == x[2 * m + 1] && y[4 * m + 2] == s * x[2 * m] && y[4 * m + 3] == s * x[2 * m + 1]);
        }
    }
    // M = 4, taps {1, 1, 1, 1}, D = 4, lead 3: the 4-point DFT of samples 4 m .. 4 m + 3, exact on these inputs (the twiddles are 1, -i, -1, i)
    {
        const auto y = bank(x, 0, 4, 4, {1.0, 1.0, 1.0, 1.0}, 3, knots.data());
        for (long m = 0; m + 1 < pss_dc::out_len(n, 4); m++)
            for (int c = 0; c < 4; c++) {
                double sr = 0, si = 0;
                const double wr[4] = {1, 0, -1, 0}, wi[4] = {0, -1, 0, 1};
                for (int t = 0; t < 4; t++) {
                    const double a = x[2 * (4 * m + t)], b = x[2 * (4 * m + t) + 1];
                    sr += a * wr[(c * t) & 3] - b * wi[(c * t) & 3];
                    si += a * wi[(c * t) & 3] + b * wr[(c * t) & 3];
                }
                CHECK(y[2 * (4 * m + c)] == (float)sr && y[2 * (4 * m + c) + 1] == (float)si);
            }
    }
    // the bank at the edges against the definition in long double (errors stay far below 1e-5 here)
    std::vector<float> odd = plain;
    for (int i = 0; i < 2 * n; i += 7) odd[i] = 1e-41f * (float)(1 + i);
    odd[11] = 1e30f;
    odd[14] = -std::numeric_limits<float>::min();
    const long double two_pi = 8.0L * std::atan(1.0L);
    for (int M : {2, 8, 64})
        for (int T : {1, M - 1, M, M + 1, 2 * M + 3, 32 * M})
            for (int D : {1, 3, M / 2, M}) {
                if (D > M || D < 1) continue;
                for (int lead : {0, (T - 1) / 2, T - 1})
                    for (long index0 : {0L, (1L << 40) + 12345}) {
                        if (index0 && (lead || M == 64)) continue;
                        std::vector<double> h(T);
                        for (int k = 0; k < T; k++) h[k] = std::cos(0.37 * k) / T;
                        const long m_begin = index0 ? (index0 + T - 1 - lead + D - 1) / D : 0;
                        const auto &src = T == M + 1 ? odd : plain;
                        const auto y = bank(src, index0, M, D, h, lead, knots.data(), m_begin);
                        const long n_m = pss_dc::out_len(index0 + n, D) - m_begin;
                        CHECK((long)y.size() == 2 * M * n_m && n_m > 0);
                        const long step = n_m > 40 ? n_m / 23 : 1;
                        for (long t = 0; t < n_m; t += step) {
                            const long m = m_begin + t;
                            for (int c = 0; c < M; c += (M > 8 ? 7 : 1)) {
                                long double ar = 0, ai = 0, scale = 1e-30L;
                                for (int k = 0; k < T; k++) {
                                    const long j = m * D + lead - k;
                                    if (j < index0 || j >= index0 + n) continue;
                                    const long double a = (long double)(((int64_t)c * (j % M)) % M) * two_pi / M;
                                    const long double xr = src[2 * (j - index0)], xi = src[2 * (j - index0) + 1];
                                    ar += (long double)h[k] * (xr * std::cos(a) + xi * std::sin(a));
                                    ai += (long double)h[k] * (xi * std::cos(a) - xr * std::sin(a));
                                    scale += std::fabs((long double)h[k]) * (std::fabs(xr) + std::fabs(xi));
                                }
                                const float *o = &y[2 * ((size_t)t * M + c)];
                                CHECK(std::fabs(o[0] - (double)ar) < 1e-5 * (double)scale + 1e-5 && std::fabs(o[1] - (double)ai) < 1e-5 * (double)scale + 1e-5);
                            }
                        }
                    }
            }
    if (failures) return 1;
    std::printf("pfb_host: ok\n");
    return 0;
}

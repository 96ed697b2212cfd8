// bank_host.cpp — pss_bank.h on the host, alone: compiled by tests/test_bank_golden.py with the host compiler and
// -fsanitize=address,undefined, run as a program of its own (never loaded into Python, never on the GPU).  It checks the statement's index
// functions for EVERY bank_ok M (the factors, the digit reversal as a permutation, every stage touching every element once with its
// twiddles inside the table, the tile inside its LDS image), the first tap as a true modulo for negative j0 - rho and far indices, the
// table's exact symmetries, the 3- and 5-point kernels and whole DFTs against direct sums in long double, and walks the bank at the tap
// counts and decimations where an index could leave its array against the definition in long double.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pss_bank.h"

using namespace pss_bk;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static std::vector<int> rev_of(int M)
{
    int n2, n3, n5;
    factor(M, n2, n3, n5);
    std::vector<int> rev(M);
    for (int r = 0; r < M; r++) rev[r] = digit_reverse(r, M, n2, n3, n5);
    return rev;
}

// the bank on one thread, exact sizes everywhere: the sanitizer sees the first element past any of them.  x holds samples
// [index0, n_cap) of a capture of n_cap samples; outputs [m_begin, out_len) -> [instant][channel] complex64
static std::vector<float> bank(const std::vector<float> &x, long index0, int M, int D, const std::vector<double> &h, int lead, long m_begin = 0)
{
    std::vector<double> tw(2 * (size_t)M);
    build_twiddles(M, tw.data());
    const std::vector<int> rev = rev_of(M);
    const long n = (long)x.size() / 2, n_cap = index0 + n;
    const long m_end = pss_dc::out_len(n_cap, D);
    std::vector<float> y(2 * (size_t)M * (size_t)(m_end - m_begin));
    std::vector<double> vr(M), vi(M);
    for (long m = m_begin; m < m_end; m++)
        instant(m, M, D, h.data(), (int)h.size(), lead, tw.data(), rev.data(), [&](long j, float &xr, float &xi) {
            xr = xi = 0.0f;
            if (j < index0 || j >= n_cap) return;
            xr = x.at(2 * (size_t)(j - index0));
            xi = x.at(2 * (size_t)(j - index0) + 1);
        }, vr.data(), vi.data(), y.data() + 2 * (size_t)M * (size_t)(m - m_begin));
    return y;
}

// the R-point kernel against the direct sum in long double
template <int R, class F>
static void check_kernel(F rnd)
{
    const long double two_pi = 8.0L * std::atan(1.0L);
    double xr[R], xi[R], yr[R], yi[R];
    long double scale = 0;
    for (int q = 0; q < R; q++) {
        xr[q] = yr[q] = rnd();
        xi[q] = yi[q] = rnd();
        scale += std::fabs(xr[q]) + std::fabs(xi[q]);
    }
    if constexpr (R == 3) kernel3(yr, yi);
    if constexpr (R == 5) kernel5(yr, yi);
    for (int p = 0; p < R; p++) {
        long double sr = 0, si = 0;
        for (int q = 0; q < R; q++) {
            const long double a = two_pi * ((p * q) % R) / R;
            sr += xr[q] * std::cos(a) + xi[q] * std::sin(a);
            si += xi[q] * std::cos(a) - xr[q] * std::sin(a);
        }
        CHECK(std::fabs(yr[p] - (double)sr) < 4e-16 * (double)scale && std::fabs(yi[p] - (double)si) < 4e-16 * (double)scale);
    }
}

int main()
{
    const long double two_pi = 8.0L * std::atan(1.0L);
    CHECK(bank_ok(2) && bank_ok(3) && bank_ok(5) && bank_ok(6) && bank_ok(15) && bank_ok(96) && bank_ok(1000) && bank_ok(1024) && bank_ok(729) && bank_ok(625));
    CHECK(!bank_ok(1) && !bank_ok(0) && !bank_ok(-6) && !bank_ok(7) && !bank_ok(14) && !bank_ok(49) && !bank_ok(343) && !bank_ok(1025) && !bank_ok(1080));
    // the first tap: a non-negative remainder whatever the sign of j0 - rho
    CHECK(first_tap(0, 0, 6) == 0 && first_tap(0, 1, 6) == 5 && first_tap(0, 5, 6) == 1 && first_tap(13, 5, 6) == 2 && first_tap(13, 14, 15) == 14);
    CHECK(first_tap(2, 999, 1000) == 3 && first_tap(0, 728, 729) == 1 && first_tap(5, 5, 45) == 0);
    CHECK(first_tap(((int64_t)1 << 40) + 12345, 7, 240) == (int)(((((int64_t)1 << 40) + 12345 - 7) % 240)));
    CHECK(first_tap(std::numeric_limits<int64_t>::max(), 0, 1000) == 807 && first_tap(-7, 0, 5) == 3);
    int n_ok = 0, worst_slots = 0;
    for (int M = 2; M <= MAX_CHAN; M++) {
        if (!bank_ok(M)) continue;
        n_ok++;
        int n2, n3, n5;
        CHECK(factor(M, n2, n3, n5) && n2 + n3 + n5 >= 1 && n2 + n3 + n5 <= MAX_STAGES);
        int prod = 1;
        for (int s = 0; s < n2 + n3 + n5; s++) {
            const int r = stage_radix(s, n3, n5);
            CHECK(r == (s < n5 ? 5 : s < n5 + n3 ? 3 : 2));
            prod *= r;
        }
        CHECK(prod == M);
        const std::vector<int> rev = rev_of(M);
        std::vector<int> seen(M, 0);
        for (int r = 0; r < M; r++) {
            CHECK(rev[r] >= 0 && rev[r] < M);
            seen.at(rev[r])++;
            for (int k = 0; k < M; k += 97) CHECK(first_tap(k + 3 * (int64_t)M, first_tap(k + 3 * (int64_t)M, r, M), M) == r);   // tap and branch are each other's
        }
        for (int v : seen) CHECK(v == 1);
        int Np = 1;
        for (int s = 0; s < n2 + n3 + n5; s++) {               // every stage touches every element once, and its twiddles are in the table
            const int r = stage_radix(s, n3, n5), N = r * Np, step = M / N;
            std::vector<int> hit(M, 0);
            for (int i = 0; i < M / r; i++) {
                const int b = i / Np, t = i % Np;
                for (int q = 0; q < r; q++) hit.at(b * N + t + q * Np)++;
                CHECK((r - 1) * t * step >= 0 && (r - 1) * t * step < M);
            }
            for (int v : hit) CHECK(v == 1);
            Np = N;
        }
        // the tile
        const int G = tile_group(M), R = tile_instants(M), RS = tile_row(M);
        CHECK(G >= 1 && M * G <= BANK_T && M * (G + 1) > BANK_T && R == ITEMS * G && R * M <= 8192 && (RS & 1) && RS >= M && RS <= M + 1);
        CHECK(R * M >= BANK_T);                                 // the transposed store gives every thread a first element inside the tile
        CHECK(R * 1 + 32 * M < (1 << 16) && R * M + 32 * M < (1 << 16));   // a tile's span, D <= M: the 32-bit sample offset
        if (!pow2(M)) {
            CHECK(R * RS <= TILE_SLOTS);
            if (R * RS > worst_slots) worst_slots = R * RS;
        }
        // the table: exact at the axes and the diagonals, mirrored exactly, close to the long double values
        std::vector<double> tw(2 * (size_t)M);
        build_twiddles(M, tw.data());
        CHECK(tw[0] == 1.0 && tw[1] == 0.0);
        for (int t = 0; t < M; t++) {
            const long double a = two_pi * t / M;
            CHECK(std::fabs(tw[2 * t] - (double)std::cos(a)) < 4e-16 && std::fabs(tw[2 * t + 1] - (double)std::sin(a)) < 4e-16);
            if (t) CHECK(tw[2 * (M - t)] == tw[2 * t] && tw[2 * (M - t) + 1] == -tw[2 * t + 1]);                 // conjugate
            if (M % 4 == 0) { const int u = (t + M / 4) % M; CHECK(tw[2 * u] == -tw[2 * t + 1] && tw[2 * u + 1] == tw[2 * t]); }   // a quarter turn on
            if (M % 8 == 0 && (t % (M / 8)) == 0 && (t / (M / 8)) % 2) CHECK(std::fabs(tw[2 * t]) == M_SQRT1_2 && std::fabs(tw[2 * t + 1]) == M_SQRT1_2);
        }
        if (M % 2 == 0) CHECK(tw[M] == -1.0 && tw[M + 1] == 0.0);
        if (M % 4 == 0) CHECK(tw[M / 2] == 0.0 && tw[M / 2 + 1] == 1.0 && tw[3 * M / 2] == 0.0 && tw[3 * M / 2 + 1] == -1.0);
    }
    CHECK(n_ok == 86 && worst_slots == TILE_SLOTS);            // 5-smooth numbers in [2, 1024]; the image is no larger than its largest tenant
    // the 3- and 5-point kernels against direct sums
    unsigned seed = 2024;
    auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return (double)((int)(seed >> 8) % 20001 - 10000) / 8192.0; };
    for (int trial = 0; trial < 50; trial++) {
        check_kernel<3>(rnd);
        check_kernel<5>(rnd);
    }
    // whole DFTs against the direct sum
    for (int M : {3, 5, 6, 9, 10, 12, 15, 25, 27, 30, 45, 96, 240, 625, 729, 1000}) {
        std::vector<double> tw(2 * (size_t)M), ur(M), ui(M), vr(M), vi(M);
        build_twiddles(M, tw.data());
        const std::vector<int> rev = rev_of(M);
        long double scale = 0;
        for (int r = 0; r < M; r++) {
            ur[r] = rnd();
            ui[r] = rnd();
            scale += std::fabs(ur[r]) + std::fabs(ui[r]);
            vr.at(rev[r]) = ur[r];
            vi.at(rev[r]) = ui[r];
        }
        dft(M, vr.data(), vi.data(), tw.data());
        for (int c = 0; c < M; c += (M > 100 ? 37 : 1)) {
            long double sr = 0, si = 0;
            for (int r = 0; r < M; r++) {
                const long double a = two_pi * (((int64_t)c * r) % M) / M;
                sr += ur[r] * std::cos(a) + ui[r] * std::sin(a);
                si += ui[r] * std::cos(a) - ur[r] * std::sin(a);
            }
            CHECK(std::fabs(vr[c] - (double)sr) < 1e-14 * (double)scale && std::fabs(vi[c] - (double)si) < 1e-14 * (double)scale);
        }
    }
    // inputs: small integers over 256, then ordinary values with float32 subnormals and a large float32
    const int n = 301;
    std::vector<float> x(2 * n), plain(2 * n);
    for (int i = 0; i < 2 * n; i++) {
        seed = seed * 1664525u + 1013904223u;
        x[i] = (float)((int)(seed >> 8) % 513 - 256) / 256.0f;
        seed = seed * 1664525u + 1013904223u;
        plain[i] = (float)((int)(seed >> 8) % 20001 - 10000) / 8192.0f;
    }
    // M = 3, one tap, D = 1: |y_c[m]| = |x[m]| and y_0[m] = x[m] exactly — whichever branch holds the sample
    {
        const auto y = bank(x, 0, 3, 1, {1.0}, 0);
        CHECK((long)y.size() == 2 * 3 * n);
        for (long m = 0; m < n; m++) CHECK(y[6 * m] == x[2 * m] && y[6 * m + 1] == x[2 * m + 1]);
    }
    // the bank at the edges against the definition in long double (errors stay far below 1e-5 here)
    std::vector<float> odd = plain;
    for (int i = 0; i < 2 * n; i += 7) odd[i] = 1e-41f * (float)(1 + i);
    odd[11] = 1e30f;
    odd[14] = -std::numeric_limits<float>::min();
    for (int M : {3, 6, 15, 45})
        for (int T : {1, M - 1, M, M + 1, 2 * M + 3, 32 * M})
            for (int D : {1, 2, M / 2, M}) {
                if (D > M || D < 1) continue;
                for (int lead : {0, (T - 1) / 2, T - 1})
                    for (long index0 : {0L, (1L << 40) + 12345}) {
                        if (index0 && (lead || M == 45 || T > 200)) continue;   // the far buffer holds n samples: its first whole span must fit
                        std::vector<double> h(T);
                        for (int k = 0; k < T; k++) h[k] = std::cos(0.37 * k) / T;
                        const long m_begin = index0 ? (index0 + T - 1 - lead + D - 1) / D : 0;
                        const auto &src = T == M + 1 ? odd : plain;
                        const auto y = bank(src, index0, M, D, h, lead, m_begin);
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
    std::printf("bank_host: ok\n");
    return 0;
}

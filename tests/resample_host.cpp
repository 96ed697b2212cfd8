// resample_host.cpp — pss_resample.h on the host, alone: compiled by tests/test_resample_golden.py with the host compiler and
// -fsanitize=address,undefined, run as a program of its own (never loaded into Python, never on the GPU).  It checks the plan against
// SciPy's own loop for the post pad, the two table layouts against each other, and walks the outputs at the lengths and ratios where an
// index could leave its array (rows of 1, 2, hpp - 1, hpp, hpp + 1 samples; up = 1, down = 1; 4096 either way; a window far into a row of
// 2^41 samples) against the definition in long double — every buffer has its exact size, so the sanitizer sees the first element past it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pss_resample.h"

using namespace pss_rs;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static std::vector<double> lowpass(int n_taps, int m)
{
    std::vector<double> h(n_taps);
    const double a = 0.5 * (n_taps - 1);
    for (int k = 0; k < n_taps; k++) {
        const double x = (k - a) / m;
        h[k] = (x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x)) * (0.54 + 0.46 * std::cos(M_PI * (k - a) / (a + 1))) / m;
    }
    return h;
}

template <class T>
static void walk(long n_in, int up, int down, int n_taps)
{
    const Plan p = make_plan(n_in, up, down, n_taps);
    const std::vector<double> taps = lowpass(n_taps, p.up > p.down ? p.up : p.down);
    // the post pad is SciPy's loop
    long post = 0;
    while (((n_in - 1) * p.up + n_taps + p.n_pre_pad + post - 1) / p.down + 1 < p.n_out + p.n_pre_remove) post++;
    CHECK(post == p.n_post_pad);
    CHECK((long)p.hpp * p.up >= p.n_pre_pad + n_taps + p.n_post_pad && (long)(p.hpp - 1) * p.up < p.n_pre_pad + n_taps + p.n_post_pad);
    std::vector<T> htf((size_t)table_len(p)), tab((size_t)table_len(p));
    build_htf(p, taps.data(), htf.data());
    build_visit(p, taps.data(), tab.data());
    for (int c = 0; c < p.up; c++)
        for (int m = 0; m < p.hpp; m++) CHECK(tab.at((size_t)m * p.up + c) == htf.at((size_t)(((long)c * p.down) % p.up) * p.hpp + m));
    std::vector<T> x((size_t)n_in);
    unsigned seed = 4321u + (unsigned)n_in;
    for (auto &v : x) {
        seed = seed * 1664525u + 1013904223u;
        v = (T)((int)(seed >> 8) % 2001 - 1000) / (T)512;
    }
    for (long j = 0; j < p.n_out; j++) {
        long first, last;
        needs(p, j, first, last);
        CHECK(first >= 0 && last <= n_in);
        const T y = output<T>(p, j, htf.data(), [&](long i) { return x.at((size_t)i); });
        // the definition: y[k] = sum over i of x[i] h[k down - i up - n_pre_pad] up
        long double acc = 0, scale = 1e-30L;
        const long k = j + p.n_pre_remove;
        for (long i = 0; i < n_in; i++) {
            const long idx = k * p.down - i * p.up - p.n_pre_pad;
            if (idx < 0 || idx >= n_taps) continue;
            acc += (long double)x[(size_t)i] * (long double)taps[(size_t)idx] * p.up;
            scale += std::fabs((long double)x[(size_t)i] * (long double)taps[(size_t)idx] * p.up);
        }
        CHECK(std::fabs((double)((long double)y - acc)) <= 1e-5 * (double)scale + 1e-6);
    }
}

int main()
{
    CHECK(gcd(12, 50) == 2 && gcd(7, 7) == 7 && gcd(441, 500) == 1 && gcd(1, 4096) == 1);
    CHECK(make_plan(10, 7, 7, 1).copy && make_plan(10, 7, 7, 1).n_out == 10 && table_len(make_plan(10, 7, 7, 1)) == 0);
    CHECK(make_plan(50000, 441, 500, 10001).n_out == 44100 && make_plan(50000, 882, 1000, 10001).up == 441);
    CHECK(make_plan(1, 5, 1, 101).n_out == 5 && make_plan(1, 1, 4, 81).n_out == 1 && make_plan(0, 3, 2, 61).n_out == 0);
    CHECK(max_taps(441, 500) == 16001 && max_taps(1, 1) == 33);
    const int ratios[][2] = {{2, 3}, {3, 2}, {1, 4}, {5, 1}, {24, 25}, {441, 500}, {147, 160}, {160, 147}, {12, 50}, {1, 4096}, {4096, 1}, {4095, 4096}};
    for (const auto &r : ratios) {
        const int g = gcd(r[0], r[1]), m = (r[0] > r[1] ? r[0] : r[1]) / g;
        const int big = m > 1000;
        const int n_taps = big ? 2 * m + 1 : 20 * m + 1;
        const int hpp = make_plan(4099, r[0], r[1], n_taps).hpp;
        for (long n : {1L, 2L, (long)hpp - 1, (long)hpp, (long)hpp + 1, 97L}) {
            if (n < 1 || (big && n > 3)) continue;
            walk<float>(n, r[0], r[1], n_taps);
            walk<double>(n, r[0], r[1], n_taps);
        }
        for (int n_taps2 : {1, 2, 3}) walk<double>(5, r[0], r[1], n_taps2);
    }
    // a window far into a row of 2^41 samples: the placement in 64-bit integers against 128-bit ones
    {
        const long n_in = (long)1 << 41;
        const Plan p = make_plan(n_in, 441, 500, 10001);
        CHECK(p.n_out == (long)(((__int128)n_in * 441 + 499) / 500));
        for (long j : {0L, 12345L, p.n_out / 2 + 17, p.n_out - 1}) {
            int t;
            long xi, lo;
            place(j, p.n_pre_remove, p.up, p.down, p.hpp, t, xi, lo);
            const __int128 q = ((__int128)j + p.n_pre_remove) * p.down;
            CHECK(xi == (long)(q / p.up) && t == (int)(q % p.up) && lo == xi - p.hpp + 1);
            long first, last;
            needs(p, j, first, last);
            CHECK(first >= 0 && last <= n_in && last - first <= p.hpp);
        }
        // complex rows: the same real tap on each part
        std::vector<double> taps = lowpass(10001, 500);
        std::vector<float> htf((size_t)table_len(p));
        build_htf(p, taps.data(), htf.data());
        const long j = p.n_out / 3;
        long first, last;
        needs(p, j, first, last);
        std::vector<cpx<float>> buf((size_t)(last - first));
        for (size_t i = 0; i < buf.size(); i++) buf[i] = {(float)i * 0.25f - 3.0f, 1.0f - (float)i * 0.125f};
        const cpx<float> y = output<cpx<float>>(p, j, htf.data(), [&](long i) { return buf.at((size_t)(i - first)); });
        const float yr = output<float>(p, j, htf.data(), [&](long i) { return buf.at((size_t)(i - first)).re; });
        const float yi = output<float>(p, j, htf.data(), [&](long i) { return buf.at((size_t)(i - first)).im; });
        CHECK(y.re == yr && y.im == yi);
    }
    if (failures) return 1;
    std::printf("resample_host: ok\n");
    return 0;
}

// welch_host.cpp — pss_welch.h on the host, alone: compiled by tests/test_welch_golden.py with the host compiler and
// -fsanitize=address,undefined, run as a program of its own (never loaded into Python, never on the GPU).  It checks the segment count,
// the argument rules, the window, the radix-2 transform against the definition in long double, and walks host_row at the segment counts
// where the tree changes shape (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 BLOCK + 3, more blocks than chunks, chunks of two blocks) with steps 1,
// N - 1 and N — every buffer has its exact size, so the sanitizer sees the first element past it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pss_welch.h"

using namespace pss_wl;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static std::vector<float> capture(long n, unsigned seed)
{
    std::vector<float> x((size_t)(2 * n));
    for (auto &v : x) {
        seed = seed * 1664525u + 1013904223u;
        v = (float)((int)(seed >> 8) % 2001 - 1000) / 512.0f + 0.25f;
    }
    return x;
}

// the definition, in long double: every segment's DFT by the sum, the mean and the max over the segments
static void direct(const std::vector<float> &x, long n, int N, int S, const std::vector<double> &w, int detrend, double scale, std::vector<double> &mean,
                   std::vector<double> &max)
{
    const long L = (n - N) / S + 1;
    std::vector<long double> sum((size_t)N, 0.0L), mx((size_t)N, 0.0L), cs((size_t)N), sn((size_t)N);
    for (int q = 0; q < N; q++) cs[(size_t)q] = cosl(2.0L * M_PIl * q / N), sn[(size_t)q] = sinl(2.0L * M_PIl * q / N);
    for (long s = 0; s < L; s++) {
        long double mr = 0, mi = 0;
        for (int i = 0; i < N; i++) mr += x.at((size_t)(2 * (s * S + i))), mi += x.at((size_t)(2 * (s * S + i) + 1));
        mr = detrend ? mr / N : 0, mi = detrend ? mi / N : 0;
        for (int k = 0; k < N; k++) {
            long double re = 0, im = 0;
            for (int i = 0; i < N; i++) {
                const long double vr = (x[(size_t)(2 * (s * S + i))] - mr) * w[(size_t)i], vi = (x[(size_t)(2 * (s * S + i) + 1)] - mi) * w[(size_t)i];
                const int q = (int)(((long)k * i) % N);
                re += vr * cs[(size_t)q] + vi * sn[(size_t)q];
                im += vi * cs[(size_t)q] - vr * sn[(size_t)q];
            }
            const long double p = re * re + im * im;
            sum[(size_t)k] += p;
            if (p > mx[(size_t)k]) mx[(size_t)k] = p;
        }
    }
    for (int k = 0; k < N; k++) mean[(size_t)k] = (double)(sum[(size_t)k] / L * scale), max[(size_t)k] = (double)(mx[(size_t)k] * scale);
}

static void walk(int N, int S, long L, long left, int detrend, bool with_definition)
{
    const long n = N + (L - 1) * S + left;
    CHECK(segments(n, N, S) == L);
    const std::vector<float> x = capture(n, 99u + (unsigned)(N + S + L));
    std::vector<double> w((size_t)N);
    default_window(N, w.data());
    for (int i = 0; i < N; i++) w[(size_t)i] += 0.05 * i / N;   // not symmetric
    const double scale = 1.0 / 3.0;
    HostPlan P(N);
    std::vector<double> mean((size_t)N), max((size_t)N), mean2((size_t)N);
    host_row(P, x.data(), n, S, w.data(), detrend, scale, mean.data(), max.data());
    host_row(P, x.data(), n, S, w.data(), detrend, scale, mean2.data(), nullptr);
    double top = 0;
    for (int k = 0; k < N; k++) {
        CHECK(mean[(size_t)k] == mean2[(size_t)k] && max[(size_t)k] >= mean[(size_t)k] * (1 - 1e-12) && std::isfinite(max[(size_t)k]));
        top = std::fmax(top, max[(size_t)k]);
    }
    if (with_definition) {
        std::vector<double> dm((size_t)N), dx((size_t)N);
        direct(x, n, N, S, w, detrend, scale, dm, dx);
        for (int k = 0; k < N; k++) CHECK(std::fabs(mean[(size_t)k] - dm[(size_t)k]) <= 1e-12 * top && std::fabs(max[(size_t)k] - dx[(size_t)k]) <= 1e-12 * top);
    }
}

int main()
{
    CHECK(segments(255, 256, 1) == 0 && segments(256, 256, 256) == 1 && segments(256 + 36 * 100 + 5, 256, 100) == 37 && segments(511, 256, 256) == 1);
    CHECK(n_blocks(1) == 1 && n_blocks(BLOCK) == 1 && n_blocks(BLOCK + 1) == 2 && chunk_len(1) == 1 && chunk_len(FOLD_Q) == 1 && chunk_len(FOLD_Q + 1) == 2);
    CHECK(nan_max(1.0, NAN) != nan_max(1.0, NAN) && nan_max(NAN, 1.0) != nan_max(NAN, 1.0) && nan_max(1.0, 2.0) == 2.0 && nan_max(-INFINITY, 0.0) == 0.0);
    {
        float x[2] = {0, 0};
        double w[1] = {1}, m[1];
        CHECK(check(x, 1, 256, 256, 256, 256, w, 1, 1.0, m) == nullptr && check(x, 3, 300, 307, 4096 / 16, 1, w, 0, 1e-300, m) == nullptr);
        CHECK(check(x, 1, 300, 300, 300, 1, w, 1, 1.0, m) && check(x, 1, 9000, 9000, 8192, 1, w, 1, 1.0, m) && check(x, 1, 300, 300, 128, 1, w, 1, 1.0, m));
        CHECK(check(x, 1, 300, 300, 256, 0, w, 1, 1.0, m) && check(x, 1, 300, 300, 256, 257, w, 1, 1.0, m) && check(x, 1, 255, 255, 256, 1, w, 1, 1.0, m));
        CHECK(check(x, 0, 300, 300, 256, 1, w, 1, 1.0, m) && check(x, 1, 300, 299, 256, 1, w, 1, 1.0, m) && check(x, 1, 300, 300, 256, 1, nullptr, 1, 1.0, m));
        CHECK(check(x, 1, 300, 300, 256, 1, w, 1, 1.0, nullptr) && check(nullptr, 1, 300, 300, 256, 1, w, 1, 1.0, m) && check(x, 1, 300, 300, 256, 1, w, 2, 1.0, m));
        CHECK(check(x, 1, 300, 300, 256, 1, w, -1, 1.0, m) && check(x, 1, 300, 300, 256, 1, w, 1, 0.0, m) && check(x, 1, 300, 300, 256, 1, w, 1, -1.0, m));
        CHECK(check(x, 1, 300, 300, 256, 1, w, 1, INFINITY, m) && check(x, 1, 300, 300, 256, 1, w, 1, NAN, m));
    }
    for (int N : {256, 512, 1024, 2048, 4096}) {
        std::vector<double> w((size_t)N);
        default_window(N, w.data());
        CHECK(w[0] == 0.0 && std::fabs(w[(size_t)N / 2] - 1.0) < 1e-15 && std::fabs(w[(size_t)N / 4] - 0.5) < 1e-15);
    }
    for (int detrend : {0, 1}) {
        walk(256, 256, 2, 5, detrend, true);
        walk(256, 97, 3, 0, detrend, true);
        for (long L : {1L, 2L, (long)BLOCK - 1, (long)BLOCK, (long)BLOCK + 1, 2L * BLOCK + 3, (long)BLOCK * FOLD_Q + 1, (long)BLOCK * (2 * FOLD_Q + 3)})
            for (int S : {1, 255, 256}) walk(256, S, L, S > 1 ? 1 : 0, detrend, false);
        for (int N : {512, 1024, 2048, 4096}) {
            walk(N, N, 2, 0, detrend, false);
            walk(N, N - 1, BLOCK + 1, 3, detrend, false);
            walk(N, 1, 3, 0, detrend, false);
        }
    }
    walk(512, 192, 2, 0, 1, true);
    if (failures) return 1;
    std::printf("welch_host: ok\n");
    return 0;
}

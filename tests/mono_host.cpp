// mono_host.cpp — pss_mono.h on the host, alone: compiled by tests/test_fm_mono_golden.py with the host compiler and
// -fsanitize=address,undefined, run as a program of its own (never loaded into Python, never on the GPU).  It walks the header's whole
// frame chain and lfilter at the lengths where an index could leave its array (0 .. 14 samples, 133, 1000), through a frame whose audio
// wraps the int16 cast and a frame with a NaN, and checks the cast's documented values.  The bits are the golden tests' business: the angle
// here is libm's atan2f and the taps a plain windowed sinc.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pss_mono.h"
#include "pss_npsum.h"

using namespace pss_mono;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

struct Out {
    std::vector<int16_t> pcm;
    std::vector<double> audio;
    std::vector<float> dec;
};

static Out run(const std::vector<float> &x, int n, double fs, const float *hp)
{
    const int n_out = out_len(n);
    Out o;
    // exact sizes: the sanitizer sees the first element past any of them
    o.pcm.resize(n_out), o.audio.resize(n_out), o.dec.resize(n_out);
    std::vector<float> work(n > 1 ? n - 1 : 0);
    std::vector<double> y(n_out);
    const double t = 75e-6 * (2.0 * fs);
    const Deemph d{1.0 / (1.0 + t), 1.0 / (1.0 + t), (1.0 - t) / (1.0 + t)};
    frame(x.data(), n, gain_of(fs), hp, d, [](float im, float re) { return std::atan2(im, re); }, work.data(), o.pcm.data(), o.audio.data(),
          o.dec.data(), y.data());
    return o;
}

int main()
{
    float hp[NHP];
    for (int k = 0; k < PRE; k++) hp[k] = 0.0f;
    for (int k = 0; k < NTAPS; k++) {
        const double m = k - 60.0, s = m == 0.0 ? 1.0 : std::sin(M_PI * m / 6.0) / (M_PI * m / 6.0);
        hp[PRE + k] = (float)(s / 6.0 * (0.54 - 0.46 * std::cos(2.0 * M_PI * k / 120.0)));
    }
    CHECK(out_len(0) == 0 && out_len(1) == 0 && out_len(2) == 1 && out_len(7) == 1 && out_len(8) == 2 && out_len(134) == 23);

    unsigned lcg = 12345u;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) / 16777216.0f - 0.5f; };
    std::vector<int> lengths;
    for (int n = 0; n <= 14; n++) lengths.push_back(n);
    lengths.push_back(133);
    lengths.push_back(1000);
    for (int n : lengths) {
        std::vector<float> x(2 * (size_t)n);
        for (float &v : x) v = rnd();
        for (double fs : {250e3, 2.4e6}) {
            const Out o = run(x, n, fs, hp);
            CHECK((int)o.pcm.size() == out_len(n));
            for (size_t j = 0; j < o.pcm.size(); j++) CHECK(std::isfinite(o.audio[j]) && std::isfinite(o.dec[j]) && o.pcm[j] == pcm_cast(o.audio[j]));
        }
    }
    {   // full deviation, +3 rad a sample then -3: wraps at 2.4 MS/s
        const int n = 1600;
        std::vector<float> x(2 * (size_t)n);
        double ph = 0.0;
        for (int i = 0; i < n; i++) { ph += i < n / 2 ? 3.0 : -3.0; x[2 * i] = (float)(0.5 * std::cos(ph)); x[2 * i + 1] = (float)(0.5 * std::sin(ph)); }
        const Out o = run(x, n, 2.4e6, hp);
        bool wraps = false;
        for (size_t j = 0; j < o.pcm.size(); j++) {
            const double a = o.audio[j];
            if (std::fabs(a) >= 32768.0) {
                wraps = true;
                CHECK(((long long)a & 0xffff) == ((long long)o.pcm[j] & 0xffff));
            }
        }
        CHECK(wraps);
        x[2 * 500] = std::numeric_limits<float>::quiet_NaN();   // one NaN: the mean is NaN, every sample 0
        const Out z = run(x, n, 2.4e6, hp);
        for (size_t j = 0; j < z.pcm.size(); j++) CHECK(z.pcm[j] == 0 && std::isnan(z.audio[j]));
    }
    // the cast: truncation to int32, low 16 bits; nothing outside int32 is converted
    CHECK(pcm_cast(40000.5) == -25536 && pcm_cast(1e9) == -13824 && pcm_cast(-1.9) == -1 && pcm_cast(32767.9) == 32767 && pcm_cast(-32768.5) == -32768);
    CHECK(pcm_cast(-40000.5) == 25536 && pcm_cast(2147483647.5) == -1 && pcm_cast(-2147483648.5) == 0);
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(pcm_cast(2147483648.0) == 0 && pcm_cast(-2147483649.0) == 0 && pcm_cast(1e300) == 0 && pcm_cast(inf) == 0 && pcm_cast(-inf) == 0 &&
          pcm_cast(std::numeric_limits<double>::quiet_NaN()) == 0);
    // lfilter at every coefficient count, rows of 0, 1 and 37 samples
    for (int nc = 2; nc <= MAX_COEF; nc++) {
        std::vector<double> b(nc), a(nc), bn(nc), an(nc);
        for (int k = 0; k < nc; k++) { b[k] = 0.1 * (k + 1); a[k] = k ? 0.05 / k : 2.0; }
        lfilter_normalise(b.data(), a.data(), nc, bn.data(), an.data());
        CHECK(an[0] == 1.0);
        for (int n : {0, 1, 37}) {
            std::vector<double> x(n), y(n);
            for (double &v : x) v = rnd();
            with_ncoef(nc, [&](auto c) { lfilter_row<decltype(c)::value>(x.data(), n, bn.data(), an.data(), y.data()); });
            for (int i = 0; i < n; i++) CHECK(std::isfinite(y[i]));
            if (n) CHECK(y[0] == bn[0] * x[0]);
        }
    }
    if (failures) return 1;
    std::puts("mono_host: ok");
    return 0;
}

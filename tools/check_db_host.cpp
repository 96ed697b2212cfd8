// The float64 dB evaluation (pyspecsdr_amd/csrc/pss_db_exact.h) measured against log10l as a stand-alone host program: the header is plain
// C++ and is compiled here as it is, next to the evaluation it replaced (97 centres on [0.75, 1.5), kept below as the yardstick).
//     g++ -std=c++17 -O2 -pthread tools/check_db_host.cpp -o check_db_host && ./check_db_host
// (or with -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all and a smaller first argument, the number of random mantissas).
// Inputs: for every exponent from that of 1e-10 to 2^296 both edges of every table interval of either evaluation +- 4 ulp; 1e8 seeded random
// mantissas over those exponents; 1e6 powers spaced evenly in 1 +- 1e-6; 1e-10 and 1; +inf and NaN.
// Per evaluation: the largest absolute error in dB, the largest relative error where |dB| < 1e-3, and the number of float32 roundings that
// differ from the float32 rounding of the long double value.  Verdict "ok" (exit status 0): none of the new figures exceeds the old one.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../pyspecsdr_amd/csrc/pss_db_exact.h"

namespace old_eval {
struct pair { double x, y; };
static const pair TAB[97] = {
    {0x1.5555555555555p+0, -0x1.ffbfc2bbc7802p-4},
    {0x1.51d07eae2f815p+0, -0x1.ed50a4a26eafbp-4},
    {0x1.4e5e0a72f0539p+0, -0x1.db11ed766abf2p-4},
    {0x1.4afd6a052bf5bp+0, -0x1.c902a19e65114p-4},
    {0x1.47ae147ae147bp+0, -0x1.b721cd17157e3p-4},
    {0x1.446f86562d9fbp+0, -0x1.a56e8325f5c87p-4},
    {0x1.4141414141414p+0, -0x1.93e7de0fc3e7fp-4},
    {0x1.3e22cbce4a902p+0, -0x1.828cfed29a212p-4},
    {0x1.3b13b13b13b14p+0, -0x1.715d0ce367afdp-4},
    {0x1.3813813813814p+0, -0x1.605735ee985f4p-4},
    {0x1.3521cfb2b78c1p+0, -0x1.4f7aad9bbcbaep-4},
    {0x1.323e34a2b10bfp+0, -0x1.3ec6ad5407866p-4},
    {0x1.2f684bda12f68p+0, -0x1.2e3a740b7800dp-4},
    {0x1.2c9fb4d812ca0p+0, -0x1.1dd5460c8b170p-4},
    {0x1.29e4129e4129ep+0, -0x1.0d966cc6500f8p-4},
    {0x1.27350b8812735p+0, -0x1.fafa6d397efdbp-5},
    {0x1.2492492492492p+0, -0x1.db11ed766abf1p-5},
    {0x1.21fb78121fb78p+0, -0x1.bb7209d1e24e4p-5},
    {0x1.1f7047dc11f70p+0, -0x1.9c197abf00dd3p-5},
    {0x1.1cf06ada2811dp+0, -0x1.7d070145f4fd8p-5},
    {0x1.1a7b9611a7b96p+0, -0x1.5e3966b7e9294p-5},
    {0x1.1811811811812p+0, -0x1.3faf7c6630614p-5},
    {0x1.15b1e5f75270dp+0, -0x1.21681b5c8c213p-5},
    {0x1.135c81135c811p+0, -0x1.0362241e638eap-5},
    {0x1.1111111111111p+0, -0x1.cb38fccd8bfdap-6},
    {0x1.0ecf56be69c90p+0, -0x1.902c31d62a847p-6},
    {0x1.0c9714fbcda3bp+0, -0x1.559bd2406c3c1p-6},
    {0x1.0a6810a6810a7p+0, -0x1.1b85d6044e9bbp-6},
    {0x1.0842108421084p+0, -0x1.c3d0837784c3ap-7},
    {0x1.0624dd2f1a9fcp+0, -0x1.51824c7587eb5p-7},
    {0x1.0410410410410p+0, -0x1.c03a80ae5e038p-8},
    {0x1.0204081020408p+0, -0x1.be76bd77b4fb5p-9},
    {0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.fc07f01fc07f0p-1, 0x1.bafd47221ed34p-9},
    {0x1.f81f81f81f820p-1, 0x1.b9476a4fcd0f3p-8},
    {0x1.f44659e4a4271p-1, 0x1.49b085144368ep-7},
    {0x1.f07c1f07c1f08p-1, 0x1.b5e908eb13789p-7},
    {0x1.ecc07b301ecc0p-1, 0x1.10a83a8446c7fp-6},
    {0x1.e9131abf0b767p-1, 0x1.45f4f5acb8be3p-6},
    {0x1.e573ac901e574p-1, 0x1.7adc3df3b1ff3p-6},
    {0x1.e1e1e1e1e1e1ep-1, 0x1.af5f92b00e611p-6},
    {0x1.de5d6e3f8868ap-1, 0x1.e3806acbd0593p-6},
    {0x1.dae6076b981dbp-1, 0x1.0ba01a816ffffp-5},
    {0x1.d77b654b82c34p-1, 0x1.25502c0fc3148p-5},
    {0x1.d41d41d41d41dp-1, 0x1.3ed1199a5e427p-5},
    {0x1.d0cb58f6ec074p-1, 0x1.58238eeb353dcp-5},
    {0x1.cd85689039b0bp-1, 0x1.71483427d2a97p-5},
    {0x1.ca4b3055ee191p-1, 0x1.8a3fadeb847f4p-5},
    {0x1.c71c71c71c71cp-1, 0x1.a30a9d609efedp-5},
    {0x1.c3f8f01c3f8f0p-1, 0x1.bba9a058dfd85p-5},
    {0x1.c0e070381c0e0p-1, 0x1.d41d5164facb7p-5},
    {0x1.bdd2b899406f7p-1, 0x1.ec6647eb5880bp-5},
    {0x1.bacf914c1bad0p-1, 0x1.02428c1f08014p-4},
    {0x1.b7d6c3dda338bp-1, 0x1.0e3d29d81165fp-4},
    {0x1.b4e81b4e81b4fp-1, 0x1.1a23445501814p-4},
    {0x1.b2036406c80d9p-1, 0x1.25f5215eb594ap-4},
    {0x1.af286bca1af28p-1, 0x1.31b3055c4711ap-4},
    {0x1.ac5701ac5701bp-1, 0x1.3d5d335c53178p-4},
    {0x1.a98ef606a63bep-1, 0x1.48f3ed1df48f9p-4},
    {0x1.a6d01a6d01a6dp-1, 0x1.5477731973e85p-4},
    {0x1.a41a41a41a41ap-1, 0x1.5fe80488af4fep-4},
    {0x1.a16d3f97a4b02p-1, 0x1.6b45df6f3e2c8p-4},
    {0x1.9ec8e951033d9p-1, 0x1.769140a2526fdp-4},
    {0x1.9c2d14ee4a102p-1, 0x1.81ca63d05a448p-4},
    {0x1.999999999999ap-1, 0x1.8cf183886480bp-4},
    {0x1.970e4f80cb872p-1, 0x1.9806d9414a20cp-4},
    {0x1.948b0fcd6e9e0p-1, 0x1.a30a9d609efebp-4},
    {0x1.920fb49d0e229p-1, 0x1.adfd07416be06p-4},
    {0x1.8f9c18f9c18fap-1, 0x1.b8de4d3ab3d97p-4},
    {0x1.8d3018d3018d3p-1, 0x1.c3aea4a5c6effp-4},
    {0x1.8acb90f6bf3aap-1, 0x1.ce6e41e463da3p-4},
    {0x1.886e5f0abb04ap-1, 0x1.d91d5866aa99ap-4},
    {0x1.8618618618618p-1, 0x1.e3bc1ab0e1a00p-4},
    {0x1.83c977ab2beddp-1, 0x1.ee4aba610f205p-4},
    {0x1.8181818181818p-1, 0x1.f8c9683468191p-4},
    {0x1.7f405fd017f40p-1, 0x1.019c2a064b487p-3},
    {0x1.7d05f417d05f4p-1, 0x1.06cbd67a6c3b7p-3},
    {0x1.7ad2208e0ecc3p-1, 0x1.0bf3d0937c41dp-3},
    {0x1.78a4c8178a4c8p-1, 0x1.11142f0811357p-3},
    {0x1.767dce434a9b1p-1, 0x1.162d082ac9d10p-3},
    {0x1.745d1745d1746p-1, 0x1.1b3e71ec94f7ap-3},
    {0x1.724287f46debcp-1, 0x1.204881dee8777p-3},
    {0x1.702e05c0b8170p-1, 0x1.254b4d35e7d3dp-3},
    {0x1.6e1f76b4337c7p-1, 0x1.2a46e8ca7ba29p-3},
    {0x1.6c16c16c16c17p-1, 0x1.2f3b691c5a000p-3},
    {0x1.6a13cd1537290p-1, 0x1.3428e2540096ep-3},
    {0x1.6816816816817p-1, 0x1.390f6844a0b82p-3},
    {0x1.661ec6a5122f9p-1, 0x1.3def0e6dfdf85p-3},
    {0x1.642c8590b2164p-1, 0x1.42c7e7fe3fc02p-3},
    {0x1.623fa77016240p-1, 0x1.479a07d3b6410p-3},
    {0x1.6058160581606p-1, 0x1.4c65807e93337p-3},
    {0x1.5e75bb8d015e7p-1, 0x1.512a644296c3ep-3},
    {0x1.5c9882b931057p-1, 0x1.55e8c518b10f9p-3},
    {0x1.5ac056b015ac0p-1, 0x1.5aa0b4b0988fap-3},
    {0x1.58ed2308158edp-1, 0x1.5f52447255c93p-3},
    {0x1.571ed3c506b3ap-1, 0x1.63fd857fc49bap-3},
    {0x1.5555555555555p-1, 0x1.68a288b60b7fdp-3}};

static double db64(double pw)
{
    uint64_t b;
    memcpy(&b, &pw, 8);
    const unsigned hi = (unsigned)(b >> 32), lo = (unsigned)b;
    const bool up = (hi & 0xfffffu) >= 0x80000u;
    const int e = (int)(hi >> 20) - 1023 + (up ? 1 : 0);
    const uint64_t zb = ((uint64_t)((hi & 0xfffffu) | (up ? 0x3fe00000u : 0x3ff00000u)) << 32) | lo;
    double z;
    memcpy(&z, &zb, 8);
    const int i = (int)std::fma(z, 128.0, -95.5);
    const pair tc = TAB[i];
    const double r = std::fma(z, tc.x, -1.0);
    double p = std::fma(r, -0x1.5555555555555p-3, 0x1.999999999999ap-3);
    p = std::fma(p, r, -0.25);
    p = std::fma(p, r, 0x1.5555555555555p-2);
    p = std::fma(p, r, -0.5);
    p = std::fma(p, r, 1.0);
    const double pr = p * r;
    double res = std::fma(pr, 0x1.bcb7b1526e50ep-2, tc.y);
    res = std::fma((double)e, 0x1.34413509f79ffp-2, res);
    return hi >= 0x7ff00000u ? pw : 10.0 * res;
}
}  // namespace old_eval

struct Figures {
    long double max_abs = 0, max_rel = 0;
    long f32_differ = 0, n = 0;
    void add(double pw, double got)
    {
        const long double want = 10.0L * log10l((long double)pw);
        const long double err = fabsl((long double)got - want);
        max_abs = std::max(max_abs, err);
        if (fabsl(want) < 1e-3L && want != 0) max_rel = std::max(max_rel, err / fabsl(want));
        if ((float)got != (float)want) f32_differ++;
        n++;
    }
    void merge(const Figures &o)
    {
        max_abs = std::max(max_abs, o.max_abs);
        max_rel = std::max(max_rel, o.max_rel);
        f32_differ += o.f32_differ;
        n += o.n;
    }
};

struct Both {
    Figures o, n;
    void add(double pw)
    {
        if (!(pw >= 1e-10)) return;                                  // the kernels' powers are |X|^2 + 1e-10
        o.add(pw, old_eval::db64(pw));
        n.add(pw, pss_r16::db64_of_exact(pw));
    }
};

static double from_bits(uint64_t b)
{
    double x;
    memcpy(&x, &b, 8);
    return x;
}
static uint64_t to_bits(double x)
{
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}
static uint64_t splitmix(uint64_t &s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

constexpr int E_LO = -34, E_HI = 296;                                // 1e-10 = 1.72 * 2^-34

int main(int argc, char **argv)
{
    const long n_random = argc > 1 ? atol(argv[1]) : 100000000L;
    Both tot;
    // interval edges of both evaluations, every exponent, +- 4 ulp
    std::vector<double> edges;
    for (int i = 0; i <= 128; i++) edges.push_back(1.0 + (2 * i - 1) / 256.0);         // new: centres 1 + i / 128, z in [1 - 1/256, 2 - 1/256)
    for (int i = 0; i <= 97; i++) edges.push_back(0.75 + (2 * i - 1) / 256.0);         // old: centres 0.75 + i / 128
    edges.push_back(1.0);
    edges.push_back(1.5);
    edges.push_back(2.0);
    for (int e = E_LO; e <= E_HI; e++)
        for (double m : edges) {
            const uint64_t b = to_bits(std::ldexp(m, e));
            for (int d = -4; d <= 4; d++) tot.add(from_bits(b + (uint64_t)(int64_t)d));
        }
    // random mantissas over the exponents: fixed chunks with their own seeds, so the figures do not depend on the thread count
    constexpr int CHUNKS = 64;
    std::vector<Both> part(CHUNKS);
    auto work = [&](int c) {
        uint64_t s = 0x5eedull * 1000003ull + (uint64_t)c;
        const long n0 = n_random * c / CHUNKS, n1 = n_random * (c + 1) / CHUNKS;
        for (long k = n0; k < n1; k++) {
            const uint64_t x = splitmix(s);
            const int e = E_LO + (int)((x >> 52) % (uint64_t)(E_HI - E_LO + 1));
            part[c].add(from_bits(((uint64_t)(e + 1023) << 52) | (x & 0xfffffffffffffull)));
        }
    };
    const int nt = (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int w = 0; w < nt; w++)
        th.emplace_back([&, w] { for (int c = w; c < CHUNKS; c += nt) work(c); });
    for (auto &t : th) t.join();
    for (auto &p : part) { tot.o.merge(p.o); tot.n.merge(p.n); }
    // the 0 dB crossing
    for (long k = 0; k <= 1000000; k++) tot.add(1.0 + (2e-6 * (double)k / 1e6 - 1e-6));
    tot.add(1e-10);
    tot.add(1.0);
    int failures = 0;
    if (pss_r16::db64_of_exact(1.0) != 0.0 || old_eval::db64(1.0) != 0.0) { printf("FAILED: 10 log10(1) != 0\n"); failures++; }
    const double inf = INFINITY, nan = NAN;
    for (double sign : {1.0, -1.0}) {
        const double q = std::copysign(nan, sign);
        if (!std::isnan(pss_r16::db64_of_exact(q)) || !std::isnan(pss_r16::db_of_exact(q)) || !std::isnan(old_eval::db64(q))) { printf("FAILED: NaN\n"); failures++; }
        // what k_spectrum_post's per-frame fix-up relies on
        if (std::fabs(pss_r16::db64_core(q)) < pss_r16::DB_FINITE_LIMIT || pss_r16::db64_core(q) == pss_r16::DB_NONFINITE_IMAGE) { printf("FAILED: image of NaN\n"); failures++; }
    }
    if (pss_r16::db64_of_exact(inf) != inf || pss_r16::db_of_exact(inf) != (float)inf || old_eval::db64(inf) != inf) { printf("FAILED: +inf\n"); failures++; }
    if (pss_r16::db64_core(inf) != pss_r16::DB_NONFINITE_IMAGE) { printf("FAILED: image of +inf\n"); failures++; }
    if (!(std::fabs(pss_r16::db64_core(std::ldexp(1.0, E_HI + 1))) < pss_r16::DB_FINITE_LIMIT) || !(std::fabs(pss_r16::db64_core(1e-10)) < pss_r16::DB_FINITE_LIMIT)) { printf("FAILED: finite range\n"); failures++; }
    printf("inputs: %ld (random mantissas: %ld)\n", tot.n.n, n_random);
    printf("old: max_abs_err_db %.4Le  max_rel_err_below_1e-3_db %.4Le  float32_roundings_differ %ld\n", tot.o.max_abs, tot.o.max_rel, tot.o.f32_differ);
    printf("new: max_abs_err_db %.4Le  max_rel_err_below_1e-3_db %.4Le  float32_roundings_differ %ld\n", tot.n.max_abs, tot.n.max_rel, tot.n.f32_differ);
    const bool ok = failures == 0 && tot.n.max_abs <= tot.o.max_abs && tot.n.max_rel <= tot.o.max_rel && tot.n.f32_differ <= tot.o.f32_differ;
    printf("verdict: %s\n", ok ? "ok" : "WORSE");
    return ok ? 0 : 1;
}

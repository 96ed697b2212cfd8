// pss_db_exact.h — 10 log10(pw) of a positive float64 power to float64 accuracy: the dB evaluation of the spectrum kernels (db_exact rows,
// float64 rows, the fused 1024-point kernel).  Plain C++ as well as HIP: tools/check_db_host.cpp compiles this file with the host compiler
// and measures the evaluation against log10l; the arithmetic is the same text in both.
//
//   pw = 2^e z with z in [1 - 1/256, 2 - 1/256): the mantissa is rounded to 7 bits IN the high word (+ 0x1000, the carry runs into the
//   exponent field), which yields e, the table index i and z from one add, one and, one subtract and one bit-field extract;
//   c_i = 1 + i / 128 (i = 0 .. 127) is the nearest centre, r = z / c_i - 1 with 1 / c_i from the table, |r| <= 2^-8;
//   10 log10 pw = e (10 log10 2) + 10 log10 c_i + r (A1 + r (A2 + ... r A6)),   Ak = (-1)^(k+1) (10 / ln 10) / k:
//   10 / ln 10 and the factor 10 live in the coefficients and in the table's second column, the truncation is (10 / ln 10) r^7 / 7 < 1e-17 dB.
// c_0 = 1 is a centre with the table entry {1, 0}, and the powers just below 1 fold onto it as well (e = 0, z < 1): near 0 dB the value is
// r (A1 + ...) alone and keeps its RELATIVE accuracy on both sides of the crossing (measured: profiles/db_eval.txt).
// DB_TAB[i] = {double(1 / c_i), 10 log10 of THAT double's reciprocal} (tools/make_db_table.py: extended precision), so the table's rounding cancels.
// Eight FMAs, one conversion, five integer instructions and the table read per value.
#pragma once

#if defined(__HIPCC__)
#define PSS_DB_FN __host__ __device__ __forceinline__
#define PSS_DB_TABLE static __constant__
namespace pss_r16 {
typedef double2 db_pair;
#else
#define PSS_DB_FN static inline
#define PSS_DB_TABLE static const
namespace pss_r16 {
struct db_pair { double x, y; };
#endif

PSS_DB_TABLE db_pair DB_TAB[128] = {
    {0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.fc07f01fc07f0p-1, 0x1.14de4c7553441p-5},
    {0x1.f81f81f81f820p-1, 0x1.13cca271e0298p-4},
    {0x1.f44659e4a4271p-1, 0x1.9c1ca65954431p-4},
    {0x1.f07c1f07c1f08p-1, 0x1.11b1a592ec2b6p-3},
    {0x1.ecc07b301ecc0p-1, 0x1.54d249255879ep-3},
    {0x1.e9131abf0b767p-1, 0x1.97723317e6edcp-3},
    {0x1.e573ac901e574p-1, 0x1.d9934d709e7f0p-3},
    {0x1.e1e1e1e1e1e1ep-1, 0x1.0d9bbbae08fcbp-2},
    {0x1.de5d6e3f8868ap-1, 0x1.2e3042bf6237cp-2},
    {0x1.dae6076b981dbp-1, 0x1.4e882121cbfffp-2},
    {0x1.d77b654b82c34p-1, 0x1.6ea43713b3d9ap-2},
    {0x1.d41d41d41d41dp-1, 0x1.8e856000f5d31p-2},
    {0x1.d0cb58f6ec074p-1, 0x1.ae2c72a6028d3p-2},
    {0x1.cd85689039b0bp-1, 0x1.cd9a4131c753dp-2},
    {0x1.ca4b3055ee191p-1, 0x1.eccf9966659f1p-2},
    {0x1.c71c71c71c71cp-1, 0x1.05e6a25c635f4p-1},
    {0x1.c3f8f01c3f8f0p-1, 0x1.154a04378be73p-1},
    {0x1.c0e070381c0e0p-1, 0x1.249252df1cbf2p-1},
    {0x1.bdd2b899406f7p-1, 0x1.33bfecf317507p-1},
    {0x1.bacf914c1bad0p-1, 0x1.42d32f26ca019p-1},
    {0x1.b7d6c3dda338bp-1, 0x1.51cc744e15bf7p-1},
    {0x1.b4e81b4e81b4fp-1, 0x1.60ac156a41e19p-1},
    {0x1.b2036406c80d9p-1, 0x1.6f7269b662f9cp-1},
    {0x1.af286bca1af28p-1, 0x1.7e1fc6b358d60p-1},
    {0x1.ac5701ac5701bp-1, 0x1.8cb4803367dd6p-1},
    {0x1.a98ef606a63bep-1, 0x1.9b30e86571b38p-1},
    {0x1.a6d01a6d01a6dp-1, 0x1.a9954fdfd0e26p-1},
    {0x1.a41a41a41a41ap-1, 0x1.b7e205aadb23dp-1},
    {0x1.a16d3f97a4b02p-1, 0x1.c617574b0db7ap-1},
    {0x1.9ec8e951033d9p-1, 0x1.d43590cae70bcp-1},
    {0x1.9c2d14ee4a102p-1, 0x1.e23cfcc470d5ap-1},
    {0x1.999999999999ap-1, 0x1.f02de46a7da0ep-1},
    {0x1.970e4f80cb872p-1, 0x1.fe088f919ca8ep-1},
    {0x1.948b0fcd6e9e0p-1, 0x1.05e6a25c635f3p+0},
    {0x1.920fb49d0e229p-1, 0x1.0cbe2488e36c4p+0},
    {0x1.8f9c18f9c18fap-1, 0x1.138af044b067ep+0},
    {0x1.8d3018d3018d3p-1, 0x1.1a4d26e79c55fp+0},
    {0x1.8acb90f6bf3aap-1, 0x1.2104e92ebe686p+0},
    {0x1.886e5f0abb04ap-1, 0x1.27b257402aa00p+0},
    {0x1.8618618618618p-1, 0x1.2e5590ae8d040p+0},
    {0x1.83c977ab2beddp-1, 0x1.34eeb47ca9743p+0},
    {0x1.8181818181818p-1, 0x1.3b7de120c10fbp+0},
    {0x1.7f405fd017f40p-1, 0x1.42033487de1a9p+0},
    {0x1.7d05f417d05f4p-1, 0x1.487ecc19074a4p+0},
    {0x1.7ad2208e0ecc3p-1, 0x1.4ef0c4b85b524p+0},
    {0x1.78a4c8178a4c8p-1, 0x1.55593aca1582dp+0},
    {0x1.767dce434a9b1p-1, 0x1.5bb84a357c453p+0},
    {0x1.745d1745d1746p-1, 0x1.620e0e67ba359p+0},
    {0x1.724287f46debcp-1, 0x1.685aa256a2955p+0},
    {0x1.702e05c0b8170p-1, 0x1.6e9e208361c8cp+0},
    {0x1.6e1f76b4337c7p-1, 0x1.74d8a2fd1a8b3p+0},
    {0x1.6c16c16c16c17p-1, 0x1.7b0a436370800p+0},
    {0x1.6a13cd1537290p-1, 0x1.81331ae900bc9p+0},
    {0x1.6816816816817p-1, 0x1.87534255c8e62p+0},
    {0x1.661ec6a5122f9p-1, 0x1.8d6ad2097d766p+0},
    {0x1.642c8590b2164p-1, 0x1.9379e1fdcfb03p+0},
    {0x1.623fa77016240p-1, 0x1.998089c8a3d14p+0},
    {0x1.6058160581606p-1, 0x1.9f7ee09e38005p+0},
    {0x1.5e75bb8d015e7p-1, 0x1.a574fd533c74dp+0},
    {0x1.5c9882b931057p-1, 0x1.ab62f65edd537p+0},
    {0x1.5ac056b015ac0p-1, 0x1.b148e1dcbeb39p+0},
    {0x1.58ed2308158edp-1, 0x1.b726d58eeb3b7p+0},
    {0x1.571ed3c506b3ap-1, 0x1.bcfce6dfb5c28p+0},
    {0x1.5555555555555p-1, 0x1.c2cb2ae38e5fcp+0},
    {0x1.5390948f40febp-1, 0x1.c891b65acb485p+0},
    {0x1.51d07eae2f815p-1, 0x1.ce509db365e20p+0},
    {0x1.5015015015015p-1, 0x1.d407f50aac626p+0},
    {0x1.4e5e0a72f0539p-1, 0x1.d9b7d02ee8586p+0},
    {0x1.4cab88725af6ep-1, 0x1.df6042a0fa749p+0},
    {0x1.4afd6a052bf5bp-1, 0x1.e5015f95ebe51p+0},
    {0x1.49539e3b2d067p-1, 0x1.ea9b39f87595ep+0},
    {0x1.47ae147ae147bp-1, 0x1.f02de46a7da0fp+0},
    {0x1.460cbc7f5cf9ap-1, 0x1.f5b971468b3d7p+0},
    {0x1.446f86562d9fbp-1, 0x1.fb3df2a131729p+0},
    {0x1.42d6625d51f87p-1, 0x1.005dbd25386b9p+1},
    {0x1.4141414141414p-1, 0x1.03190ce7884f7p+1},
    {0x1.3fb013fb013fbp-1, 0x1.05d0f13cf79c3p+1},
    {0x1.3e22cbce4a902p-1, 0x1.088572aaa55d9p+1},
    {0x1.3c995a47babe7p-1, 0x1.0b36999600afep+1},
    {0x1.3b13b13b13b14p-1, 0x1.0de46e456520fp+1},
    {0x1.3991c2c187f63p-1, 0x1.108ef8e0b3505p+1},
    {0x1.3813813813814p-1, 0x1.13364171e5ea3p+1},
    {0x1.3698df3de0748p-1, 0x1.15da4fe5a31a8p+1},
    {0x1.3521cfb2b78c1p-1, 0x1.187b2c0bca8d8p+1},
    {0x1.33ae45b57bcb2p-1, 0x1.1b18dd98001a5p+1},
    {0x1.323e34a2b10bfp-1, 0x1.1db36c22332dfp+1},
    {0x1.30d190130d190p-1, 0x1.204adf27230d6p+1},
    {0x1.2f684bda12f68p-1, 0x1.22df3e08e007bp+1},
    {0x1.2e025c04b8097p-1, 0x1.2570900f49aa6p+1},
    {0x1.2c9fb4d812ca0p-1, 0x1.27fedc688a10cp+1},
    {0x1.2b404ad012b40p-1, 0x1.2a8a2a298e5fap+1},
    {0x1.29e4129e4129ep-1, 0x1.2d12804e7c831p+1},
    {0x1.288b01288b013p-1, 0x1.2f97e5bb26408p+1},
    {0x1.27350b8812735p-1, 0x1.321a613b79b05p+1},
    {0x1.25e22708092f1p-1, 0x1.3499f983ef2eep+1},
    {0x1.2492492492492p-1, 0x1.3716b531f4da1p+1},
    {0x1.23456789abcdfp-1, 0x1.39909acc57a84p+1},
    {0x1.21fb78121fb78p-1, 0x1.3c07b0c3aa2bbp+1},
    {0x1.20b470c67c0d9p-1, 0x1.3e7bfd72a9105p+1},
    {0x1.1f7047dc11f70p-1, 0x1.40ed871e9d656p+1},
    {0x1.1e2ef3b3fb874p-1, 0x1.435c53f7bcbedp+1},
    {0x1.1cf06ada2811dp-1, 0x1.45c86a1987405p+1},
    {0x1.1bb4a4046ed29p-1, 0x1.4831cf8b239ccp+1},
    {0x1.1a7b9611a7b96p-1, 0x1.4a988a3fb9198p+1},
    {0x1.19453808ca29cp-1, 0x1.4cfca016c7a1fp+1},
    {0x1.1811811811812p-1, 0x1.4f5e16dc7df8cp+1},
    {0x1.16e0689427379p-1, 0x1.51bcf44a0e11fp+1},
    {0x1.15b1e5f75270dp-1, 0x1.54193e05ffa2cp+1},
    {0x1.1485f0e0acd3bp-1, 0x1.5672f9a480f2dp+1},
    {0x1.135c81135c811p-1, 0x1.58ca2ca7b5f9ap+1},
    {0x1.12358e75d3033p-1, 0x1.5b1edc8005d38p+1},
    {0x1.1111111111111p-1, 0x1.5d710e8c66982p+1},
    {0x1.0fef010fef011p-1, 0x1.5fc0c81aa79e6p+1},
    {0x1.0ecf56be69c90p-1, 0x1.620e0e67ba359p+1},
    {0x1.0db20a88f4696p-1, 0x1.6458e69ff8df6p+1},
    {0x1.0c9714fbcda3bp-1, 0x1.66a155df6d134p+1},
    {0x1.0b7e6ec259dc8p-1, 0x1.68e7613213945p+1},
    {0x1.0a6810a6810a7p-1, 0x1.6b2b0d941f63cp+1},
    {0x1.0953f39010954p-1, 0x1.6d6c5ff23b567p+1},
    {0x1.0842108421084p-1, 0x1.6fab5d29ca584p+1},
    {0x1.073260a47f7c6p-1, 0x1.71e80a0926642p+1},
    {0x1.0624dd2f1a9fcp-1, 0x1.74226b4fde38cp+1},
    {0x1.05197f7d73404p-1, 0x1.765a85aef1d2bp+1},
    {0x1.0410410410410p-1, 0x1.78905dc90db1ep+1},
    {0x1.03091b51f5e1ap-1, 0x1.7ac3f832c4f2ep+1},
    {0x1.0204081020408p-1, 0x1.7cf55972ca437p+1},
    {0x1.0101010101010p-1, 0x1.7f24860227b7bp+1}};

// bit fields of a double: the same text for the device (register halves) and the host
PSS_DB_FN unsigned db_hi32(double x) { return (unsigned)(__builtin_bit_cast(unsigned long long, x) >> 32); }
PSS_DB_FN unsigned db_lo32(double x) { return (unsigned)__builtin_bit_cast(unsigned long long, x); }
PSS_DB_FN double db_from_words(unsigned hi, unsigned lo) { return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo); }

// a power is +inf or NaN iff its high word, as an unsigned number, is at least +inf's (pw = |X|^2 + 1e-10 is never negative; a NaN of either sign qualifies)
constexpr unsigned DB_HI_NONFINITE = 0x7ff00000u;

// The evaluation for a FINITE pw > 0 (normal: pw >= 1e-10).  +inf / NaN come out as finite numbers beyond +-DB_FINITE_LIMIT (below); the
// callers put the power itself in their place (db64_of_exact per value, k_spectrum_post once per frame).
PSS_DB_FN double db64_core(double pw, const db_pair *tab = DB_TAB)
{
    const unsigned hi = db_hi32(pw);
    const unsigned u = hi + (0x1000u - 0x3ff00000u);                     // mantissa rounded to 7 bits, exponent unbiased
    const unsigned es = u & 0xfff00000u;                                 // e << 20 (two's complement)
    const double z = db_from_words(hi - es, db_lo32(pw));                // pw 2^-e
    const db_pair tc = tab[(u >> 13) & 127u];
    const double r = __builtin_fma(z, tc.x, -1.0);
    double p = __builtin_fma(r, -0x1.729913c4b1436p-1, 0x1.bcb7b1526e50ep-1);   // A6, A5
    p = __builtin_fma(p, r, -0x1.15f2ced384f29p+0);                      // A4
    p = __builtin_fma(p, r, 0x1.729913c4b1436p+0);                       // A3
    p = __builtin_fma(p, r, -0x1.15f2ced384f29p+1);                      // A2
    p = __builtin_fma(p, r, 0x1.15f2ced384f29p+2);                       // A1 = 10 / ln 10
    // the exponent term last: every rounding before it is at the scale of 10 log10 z (< 3 dB), one at the scale of the result
    return __builtin_fma((double)(int)es, 0x1.8151824c7587fp-19, __builtin_fma(p, r, tc.y));   // e 2^20 * (10 log10 2) 2^-20
}

// what db64_core makes of +inf (e = 1024, z = 1: exactly 1024 * 10 log10 2 = 3082.5 dB); of a quiet NaN (mantissa >= 1.5) with the sign bit clear
// at least 1.76 dB more, with the sign bit set (e = -1024) at most -3080.7 dB.  No finite power of a complex64 frame comes near either:
// 1e-10 <= |X|^2 + 1e-10 < 2^296 for frames of up to 2^20 points, -100 <= dB < 892.
constexpr double DB_NONFINITE_IMAGE = 1024.0 * 0x1.8151824c7587fp+1;
constexpr double DB_FINITE_LIMIT = 3000.0;

// the float64 value itself (the reference's own row type, pss_spectrum_db_f64), +inf and NaN as themselves.  Every caller but k_spectrum_post
// uses this per-value test (a compare and two selects): k_spectrum_r16 / k_spectrum_xl / the Bluestein and huge-length stores do not keep their
// 16 values (they store each as it is formed), so a per-frame fix-up would have to hold them — 16 to 32 registers in kernels at 226 .. 256 —
// and none of them is in the benchmarked step.
PSS_DB_FN double db64_of_exact(double pw, const db_pair *tab = DB_TAB)
{
    const double d = db64_core(pw, tab);
    return db_hi32(pw) >= DB_HI_NONFINITE ? pw : d;
}

// compute_fft's float64 value rounded ONCE to float32
PSS_DB_FN float db_of_exact(double pw, const db_pair *tab = DB_TAB) { return (float)db64_of_exact(pw, tab); }

}  // namespace pss_r16

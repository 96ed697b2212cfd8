// pss_resample.h — the arithmetic of the rational resampler for rows (scipy.signal.resample_poly: upfirdn behind a low-pass table),
// stated ONCE for the kernel (pss_resample.hip: k_resample), the host twin (pss_h_resample) and the stand-alone host check
// (tests/resample_host.cpp).
//
//   factors   up / down reduced by their gcd; both 1: the result is a copy of the row.
//   table     for a row of n_in samples of real type T (float32, float64; complex64 rows: float32) and a float64 low-pass table
//             taps[n_taps], half_len = (n_taps - 1) / 2:  h = (T)taps, then h = h * (T)up in T;  n_out = ceil(n_in up / down);
//             n_pre_pad = down - half_len % down;  n_pre_remove = (half_len + n_pre_pad) / down;  n_post_pad the smallest value >= 0 with
//             ((n_in - 1) up + n_taps + n_pre_pad + n_post_pad - 1) / down + 1 >= n_out + n_pre_remove;
//             hp = n_pre_pad zeros, h, n_post_pad zeros, zero-extended to a multiple of up;  hpp = len(hp) / up;
//             htf[t][m] = hp[(hpp - 1 - m) up + t]  (SciPy's _UpFIRDn: the table transposed and flipped).
//   output j  k = j + n_pre_remove, q = k down (64-bit), t = q mod up, xi = q div up, lo = xi - hpp + 1;  acc = +0;  for i from
//             max(lo, 0) to min(xi, n_in - 1) ascending: acc = acc + x[i] * htf[t][i - lo] — one IEEE multiply, then one IEEE add, in T;
//             a complex64 sample takes the same real tap on each part.  Terms outside the row are skipped, not added as zeros; the zero
//             pads are entries of the table and are executed (0 * NaN is NaN and reaches the outputs it reaches in SciPy).
//   complex64 the contract covers finite samples: SciPy multiplies by h + 0i there, which differs from the statement above on inf / NaN
//             samples only.  Such rows are computed as stated, never fault; their values are outside the contract.
//   kernel    the table in visit order, tap index major: tab[m up + p] = htf[(p down) mod up][m] — output k reads column k mod up.
// Every unit that includes this header is compiled with -ffp-contract=off: each `*` and `+` is one IEEE operation.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PSS_RS_HD __host__ __device__
#else
#define PSS_RS_HD
#endif

namespace pss_rs {

constexpr int MAX_FACTOR = 4096;                 // up and down as given
constexpr long MAX_ROW = (long)1 << 48;          // samples of a row: k down and n_in up stay far inside int64
constexpr int F32 = 0, F64 = 1, C64 = 2;         // row types (PSS_RS_* of include/pss.h)

template <class T>
struct cpx {
    T re, im;
};

inline int gcd(int a, int b)
{
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// most taps a table may have at the REDUCED factors
inline long max_taps(int up, int down) { return 32L * (up > down ? up : down) + 1; }

// What one row length, one pair of factors and one tap count fix.  up, down: reduced.  copy: both 1 (nothing else is used then).
struct Plan {
    int up = 1, down = 1;
    bool copy = true;
    long n_in = 0, n_out = 0;
    long n_pre_pad = 0, n_post_pad = 0, n_pre_remove = 0;
    int n_taps = 0;
    int hpp = 0;                                 // taps of a phase: the table is up x hpp
};

// the caller has checked 1 <= up, down <= MAX_FACTOR, 0 <= n_in <= MAX_ROW and 1 <= n_taps <= max_taps (reduced factors)
inline Plan make_plan(long n_in, int up, int down, int n_taps)
{
    Plan p;
    const int g = gcd(up, down);
    p.up = up / g;
    p.down = down / g;
    p.copy = p.up == 1 && p.down == 1;
    p.n_in = n_in;
    p.n_taps = n_taps;
    const long prod = n_in * p.up;
    p.n_out = prod / p.down + (prod % p.down != 0);
    if (p.copy) return p;
    const long half_len = (n_taps - 1) / 2;
    p.n_pre_pad = p.down - half_len % p.down;
    p.n_pre_remove = (half_len + p.n_pre_pad) / p.down;
    // floor((a + post) / down) >= b  <=>  post >= b down - a
    const long a = (n_in - 1) * p.up + n_taps + p.n_pre_pad - 1, b = p.n_out + p.n_pre_remove - 1;
    p.n_post_pad = b * p.down > a ? b * p.down - a : 0;
    const long len = p.n_pre_pad + n_taps + p.n_post_pad;
    p.hpp = (int)((len + p.up - 1) / p.up);
    return p;
}

inline long table_len(const Plan &p) { return p.copy ? 0 : (long)p.up * p.hpp; }

// hp[i]: the padded table, 0 <= i < up hpp
template <class T>
inline T padded_tap(const Plan &p, const double *taps, long i)
{
    const long k = i - p.n_pre_pad;
    if (k < 0 || k >= p.n_taps) return (T)0;
    const T h = (T)taps[k];
    return h * (T)p.up;
}

// htf[t * hpp + m]
template <class T>
inline void build_htf(const Plan &p, const double *taps, T *htf)
{
    for (int t = 0; t < p.up; t++)
        for (int m = 0; m < p.hpp; m++) htf[(long)t * p.hpp + m] = padded_tap<T>(p, taps, (long)(p.hpp - 1 - m) * p.up + t);
}

// tab[m * up + c] = htf[(c down) mod up][m]: the kernel's layout
template <class T>
inline void build_visit(const Plan &p, const double *taps, T *tab)
{
    for (int c = 0; c < p.up; c++) {
        const int t = (int)(((long)c * p.down) % p.up);
        for (int m = 0; m < p.hpp; m++) tab[(long)m * p.up + c] = padded_tap<T>(p, taps, (long)(p.hpp - 1 - m) * p.up + t);
    }
}

// one term of the chain
PSS_RS_HD inline void mac(float &acc, float x, float h) { acc = acc + x * h; }
PSS_RS_HD inline void mac(double &acc, double x, double h) { acc = acc + x * h; }
PSS_RS_HD inline void mac(cpx<float> &acc, cpx<float> x, float h)
{
    acc.re = acc.re + x.re * h;
    acc.im = acc.im + x.im * h;
}
PSS_RS_HD inline void zero(float &a) { a = 0.0f; }
PSS_RS_HD inline void zero(double &a) { a = 0.0; }
PSS_RS_HD inline void zero(cpx<float> &a) { a.re = a.im = 0.0f; }

// where output j of a row reads: the phase t, the last sample xi and the first one lo (may be negative; xi may pass the row's end)
PSS_RS_HD inline void place(long j, long n_pre_remove, int up, int down, int hpp, int &t, long &xi, long &lo)
{
    const long q = (j + n_pre_remove) * down;
    xi = q / up;
    t = (int)(q - xi * up);
    lo = xi - hpp + 1;
}

// the samples of the row output j needs, cut to the row: [first, last) (empty: first >= last)
inline void needs(const Plan &p, long j, long &first, long &last)
{
    int t;
    long xi, lo;
    place(j, p.n_pre_remove, p.up, p.down, p.hpp, t, xi, lo);
    first = lo < 0 ? 0 : lo;
    last = (xi < p.n_in - 1 ? xi : p.n_in - 1) + 1;
}

// One output on one thread.  X(i): sample i of the row, called for 0 <= i < n_in only, ascending; htf: [up][hpp].
template <class E, class T, class FX>
inline E output(const Plan &p, long j, const T *htf, FX X)
{
    int t;
    long xi, lo;
    place(j, p.n_pre_remove, p.up, p.down, p.hpp, t, xi, lo);
    const T *h = htf + (long)t * p.hpp;
    E acc;
    zero(acc);
    const long i0 = lo < 0 ? 0 : lo, i1 = xi < p.n_in - 1 ? xi : p.n_in - 1;
    for (long i = i0; i <= i1; i++) mac(acc, X(i), h[i - lo]);
    return acc;
}

}  // namespace pss_rs

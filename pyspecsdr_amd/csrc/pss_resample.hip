// pss_resample.hip — the rational resampler for batches of rows (scipy.signal.resample_poly, bit for bit).  The arithmetic is
// pss_resample.h's; this unit places it.
//   k_resample<E, T>   E: the row's element (float, double, complex64), T: its real type.  A thread owns R outputs of one row whose upfirdn
//           indices lie S apart, S a multiple of `up`: they share their phase, so a step of the chain is ONE tap load and R multiply-add
//           pairs, and their samples lie exactly (S / up) down apart.  Threads that follow each other own consecutive outputs: they read
//           consecutive words of the table (uploaded in visit order, tap index major) and samples down / up apart.  The (row, thread slot)
//           items of the whole batch are numbered flat and walked by a grid-stride loop, so 65 536 rows of 10 samples fill the device as
//           192 rows of 500 000 do.  An item whose outputs all read inside the row runs the chain without tests; the first and last hpp
//           outputs of a row, and a window's last items, test every term.  No LDS: the vector cache carries the sample span.
// Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_ctx.h"
#include "pss_resample.h"

namespace {

using namespace pss_rs;

constexpr int RS_T = 256;                       // threads of a workgroup
constexpr int RS_R = 4;                         // outputs of a thread
constexpr long RS_GRID_CAP = 4096;              // workgroups of a launch: items past it are walked by a grid-stride loop

struct RsGeom {       // the launch's numbers (host: geom())
    long x_stride, buf0, n_in, n_pre_remove, j_begin, n_w, ipr, n_items, y_stride;
    int up, down, hpp, copy, S, dx, p_base;
};

// x: the caller's buffer, element 0 = sample buf0 of row 0.  Every sample an output of the window needs inside its row is in the buffer (the
// host has checked).  Window offset w = j - j_begin; the items of a row: group g covers S R offsets, item (g, c) owns offsets
// g S R + c + r S, r < R; the last group has min(S, what is left) items.
template <class E, class T>
__global__ __launch_bounds__(RS_T) void k_resample(const E *__restrict__ x, const T *__restrict__ tab, const RsGeom G, E *__restrict__ y)
{
    const long step = (long)gridDim.x * RS_T;
    for (long id = (long)blockIdx.x * RS_T + threadIdx.x; id < G.n_items; id += step) {
        const long row = id / G.ipr, e = id - row * G.ipr;
        const long g = e / G.S;
        const int c = (int)(e - g * G.S);
        const long w0 = g * G.S * RS_R + c;
        const E *xr = x + row * G.x_stride;
        E *yr = y + row * G.y_stride;
        if (G.copy) {
            for (int r = 0; r < RS_R; r++) {
                const long w = w0 + (long)r * G.S;
                if (w < G.n_w) yr[w] = xr[G.j_begin + w - G.buf0];
            }
            continue;
        }
        int p = G.p_base + c % G.up;
        if (p >= G.up) p -= G.up;
        const T *h = tab + p;
        const long xi0 = ((G.j_begin + G.n_pre_remove + w0) * G.down) / G.up, lo0 = xi0 - G.hpp + 1;
        E acc[RS_R];
        for (int r = 0; r < RS_R; r++) zero(acc[r]);
        const bool full = w0 + (long)(RS_R - 1) * G.S < G.n_w;
        if (full && lo0 >= 0 && xi0 + (long)(RS_R - 1) * G.dx <= G.n_in - 1) {
            const E *s = xr + (lo0 - G.buf0);
#pragma unroll 4
            for (int m = 0; m < G.hpp; m++) {
                const T hv = h[(long)m * G.up];
#pragma unroll
                for (int r = 0; r < RS_R; r++) mac(acc[r], s[(long)r * G.dx + m], hv);
            }
#pragma unroll
            for (int r = 0; r < RS_R; r++) yr[w0 + (long)r * G.S] = acc[r];
        } else {
#pragma unroll
            for (int r = 0; r < RS_R; r++) {
                const long w = w0 + (long)r * G.S;
                if (w >= G.n_w) break;
                const long lo = lo0 + (long)r * G.dx, xi = xi0 + (long)r * G.dx;
                const int m0 = lo < 0 ? (int)-lo : 0;
                const int m1 = xi <= G.n_in - 1 ? G.hpp - 1 : (int)(G.n_in - 1 - lo);   // < m0 where the output reads nothing
                const E *s = xr + (lo - G.buf0);
                for (int m = m0; m <= m1; m++) mac(acc[r], s[m], h[(long)m * G.up]);
                yr[w] = acc[r];
            }
        }
    }
}

RsGeom geom(const Plan &p, long n_rows, long x_stride, long buf_index0, long j_begin, long j_end, long y_stride)
{
    RsGeom G;
    G.x_stride = x_stride, G.buf0 = buf_index0, G.n_in = p.n_in, G.n_pre_remove = p.n_pre_remove, G.j_begin = j_begin, G.n_w = j_end - j_begin;
    G.y_stride = y_stride;
    G.up = p.up, G.down = p.down, G.hpp = p.hpp, G.copy = p.copy;
    G.S = p.up * ((64 + p.up - 1) / p.up);
    G.dx = (G.S / p.up) * p.down;
    G.p_base = (int)((j_begin + p.n_pre_remove) % p.up);
    const long per = (long)G.S * RS_R, n_g = (G.n_w + per - 1) / per, left = G.n_w - (n_g - 1) * per;
    G.ipr = (n_g - 1) * G.S + (left < G.S ? left : G.S);
    G.n_items = n_rows * G.ipr;
    return G;
}

size_t elem_bytes(int dtype) { return dtype == F32 ? 4 : 8; }

// The argument rules of pss_resample and pss_h_resample.  ctx: where the reason goes (NULL: the library's own slot).  *plan is filled where
// the result is PSS_OK.
int rs_check(pss_ctx *ctx, const char *who, const void *x, int dtype, long n_rows, long x_stride, long n_buf, long buf_index0, long n_in, int up,
             int down, const double *taps, int n_taps, long j_begin, long j_end, const void *y, long y_stride, Plan *plan)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (up < 1 || up > MAX_FACTOR || down < 1 || down > MAX_FACTOR) return bad("up or down outside [1, 4096]");
    const int g = gcd(up, down);
    if (n_taps < 1 || n_taps > max_taps(up / g, down / g)) return bad("n_taps outside [1, 32 max(up, down) + 1] (the reduced factors)");
    if (!taps) return bad("null taps");
    for (int k = 0; k < n_taps; k++)
        if (!std::isfinite(taps[k])) return bad("a tap that is not finite");
    if (dtype != F32 && dtype != F64 && dtype != C64) return bad("unknown dtype");
    if (n_rows < 0) return bad("n_rows < 0");
    if (n_in < 0 || n_in > MAX_ROW) return bad("n_in outside [0, 2^48]");
    if (n_buf < 0 || buf_index0 < 0 || n_buf > n_in || buf_index0 > n_in - n_buf)
        return bad("the buffer [buf_index0, buf_index0 + n_buf) is not inside the row [0, n_in)");
    *plan = make_plan(n_in, up, down, n_taps);
    if (j_begin < 0 || j_end < j_begin || j_end > plan->n_out) return bad("[j_begin, j_end) outside [0, ceil(n_in up / down)]");
    if (y_stride < j_end - j_begin) return bad("y_stride < j_end - j_begin");
    if (x_stride < n_buf) return bad("x_stride < n_buf");
    if (n_rows == 0 || j_begin == j_end) return PSS_OK;
    const long widest = x_stride > y_stride ? x_stride : y_stride;   // >= 1: the window is not empty
    if (n_rows > INT64_MAX / 8 / widest) return bad("n_rows times a stride overflows");
    const uintptr_t mask = elem_bytes(dtype) - 1;
    if (!y) return bad("null output");
    if (reinterpret_cast<uintptr_t>(y) & mask) return bad("the output is not aligned to its element");
    // the samples the window's outputs need, cut to the row: they must lie in the buffer
    long need_lo, need_hi, t;
    if (plan->copy) {
        need_lo = j_begin, need_hi = j_end;
    } else {
        needs(*plan, j_begin, need_lo, t);
        needs(*plan, j_end - 1, t, need_hi);
    }
    if (need_lo < need_hi) {
        if (!x) return bad("null input");
        if (reinterpret_cast<uintptr_t>(x) & mask) return bad("the input is not aligned to its element");
        if (need_lo < buf_index0 || need_hi > buf_index0 + n_buf) return bad("an output needs a sample of the row that the buffer does not hold");
    }
    return PSS_OK;
}

template <class E, class T>
void host_rows(const Plan &p, const E *x, long n_rows, long x_stride, long buf_index0, const double *taps, long j_begin, long j_end, E *y,
               long y_stride)
{
    std::vector<T> htf((size_t)table_len(p));
    if (!p.copy) build_htf(p, taps, htf.data());
    for (long r = 0; r < n_rows; r++) {
        const E *xr = x + r * x_stride;
        E *yr = y + r * y_stride;
        for (long j = j_begin; j < j_end; j++)
            yr[j - j_begin] = p.copy ? xr[j - buf_index0] : output<E>(p, j, htf.data(), [&](long i) { return xr[i - buf_index0]; });
    }
}

template <class E, class T>
int launch(pss_ctx *ctx, const Plan &p, const void *d_x, long n_rows, long x_stride, long buf_index0, const double *taps, long j_begin, long j_end,
           void *d_y, long y_stride)
{
    // the plan's numbers and the table in visit order, back to back (pss_table_sync: uploaded when they differ from the device copy)
    const long n_tab = table_len(p);
    const long head[4] = {p.up, p.down, p.hpp, (long)sizeof(T)};
    const size_t bytes = sizeof(head) + sizeof(T) * (size_t)(n_tab > 0 ? n_tab : 1);
    std::vector<unsigned char> tab(bytes, 0);
    memcpy(tab.data(), head, sizeof(head));
    if (!p.copy) build_visit(p, taps, reinterpret_cast<T *>(tab.data() + sizeof(head)));
    const int r = pss_table_sync(ctx, &ctx->rs_tab, tab.data(), bytes, "pss_resample table");
    if (r) return r;
    const T *d_tab = reinterpret_cast<const T *>(reinterpret_cast<const unsigned char *>(ctx->rs_tab.dev) + sizeof(head));
    const RsGeom G = geom(p, n_rows, x_stride, buf_index0, j_begin, j_end, y_stride);
    const long n_groups = (G.n_items + RS_T - 1) / RS_T;
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_resample");
    hipLaunchKernelGGL((k_resample<E, T>), dim3((unsigned)(n_groups < RS_GRID_CAP ? n_groups : RS_GRID_CAP)), dim3(RS_T), 0, PSS_STREAM(ctx),
                       d_x ? reinterpret_cast<const E *>(d_x) : reinterpret_cast<const E *>(d_tab), d_tab, G, reinterpret_cast<E *>(d_y));
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_resample launch");
}

}  // namespace

extern "C" long pss_resample_out_len(long n_in, int up, int down)
{
    if (n_in < 0 || n_in > MAX_ROW || up < 1 || up > MAX_FACTOR || down < 1 || down > MAX_FACTOR) return PSS_E_ARG;
    return make_plan(n_in, up, down, 1).n_out;
}

extern "C" int pss_resample_default_taps(int up, int down, double *taps, int *n_taps)
{
    if (!n_taps || up < 1 || up > MAX_FACTOR || down < 1 || down > MAX_FACTOR)
        return pss_fail(nullptr, PSS_E_ARG, "pss_resample_default_taps: up or down outside [1, 4096]");
    const int g = gcd(up, down), mx = (up > down ? up : down) / g;
    *n_taps = mx == 1 ? 1 : 20 * mx + 1;
    if (!taps) return PSS_OK;
    if (mx == 1) {
        taps[0] = 1.0;   // a copy: the table is not used
        return PSS_OK;
    }
    return pss_design_firwin_kaiser(*n_taps, 1.0 / (double)mx, 5.0, taps);
}

extern "C" int pss_h_resample(const void *h_x, int dtype, long n_rows, long x_stride, long n_buf, long buf_index0, long n_in, int up, int down,
                              const double *taps, int n_taps, long j_begin, long j_end, void *h_y, long y_stride)
{
    Plan p;
    const int r = rs_check(nullptr, "pss_h_resample", h_x, dtype, n_rows, x_stride, n_buf, buf_index0, n_in, up, down, taps, n_taps, j_begin, j_end,
                           h_y, y_stride, &p);
    if (r || n_rows == 0 || j_begin == j_end) return r;
    if (dtype == F32)
        host_rows<float, float>(p, (const float *)h_x, n_rows, x_stride, buf_index0, taps, j_begin, j_end, (float *)h_y, y_stride);
    else if (dtype == F64)
        host_rows<double, double>(p, (const double *)h_x, n_rows, x_stride, buf_index0, taps, j_begin, j_end, (double *)h_y, y_stride);
    else
        host_rows<cpx<float>, float>(p, (const cpx<float> *)h_x, n_rows, x_stride, buf_index0, taps, j_begin, j_end, (cpx<float> *)h_y, y_stride);
    return PSS_OK;
}

extern "C" int pss_resample(pss_ctx *ctx, const void *d_x, int dtype, long n_rows, long x_stride, long n_buf, long buf_index0, long n_in, int up,
                            int down, const double *taps, int n_taps, long j_begin, long j_end, void *d_y, long y_stride)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    Plan p;
    const int r = rs_check(ctx, "pss_resample", d_x, dtype, n_rows, x_stride, n_buf, buf_index0, n_in, up, down, taps, n_taps, j_begin, j_end, d_y,
                           y_stride, &p);
    if (r || n_rows == 0 || j_begin == j_end) return r;
    if (dtype == F32) return launch<float, float>(ctx, p, d_x, n_rows, x_stride, buf_index0, taps, j_begin, j_end, d_y, y_stride);
    if (dtype == F64) return launch<double, double>(ctx, p, d_x, n_rows, x_stride, buf_index0, taps, j_begin, j_end, d_y, y_stride);
    return launch<cpx<float>, float>(ctx, p, d_x, n_rows, x_stride, buf_index0, taps, j_begin, j_end, d_y, y_stride);
}

// Host harness of tests/test_npsum_host.py: pss_npsum.h compiled WITHOUT HIP (g++ -std=c++17 -ffp-contract=off), behind a C ABI.
//   npsum_*   the header's plain sum (np_sum);
//   tabsum_*  the header's TABLES (build_forest) evaluated here: the leaf rule written out below, on its own, then the inner nodes level
//             by level and the roots in chunk order — what the kernels do with the same tables.
#include <vector>

#include "pss_npsum.h"

namespace {
// One leaf of `len` floats at a, every `stride`-th float from `c` on (stride 1: a real array; stride 2: component c of a complex one).
template <class T>
T leaf(const T *a, int len, int stride, int c)
{
    if (len < 8) {
        T res = 0;
        for (int i = c; i < len; i += stride) res += a[i];
        return res;
    }
    T r[8];
    for (int k = 0; k < 8; k++) r[k] = a[k];
    const int end = len - len % 8;
    for (int i = 8; i < end; i += 8)
        for (int k = 0; k < 8; k++) r[k] += a[i + k];
    T res = stride == 1 ? ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])) : (r[c] + r[c + 2]) + (r[c + 4] + r[c + 6]);
    for (int i = end + c; i < len; i += stride) res += a[i];
    return res;
}
template <class T>
void tabsum(const T *a, int n, bool cplx, T *out)
{
    const pss_np::Forest f = pss_np::build_forest(n, cplx);
    const int nl = f.n_leaves(), stride = cplx ? 2 : 1;
    for (int c = 0; c < stride; c++) {
        std::vector<T> val(nl + f.n_nodes());
        for (int l = 0; l < nl; l++) val[l] = leaf(a + f.leaf_off[l], f.leaf_len[l], stride, c);
        for (int lv = 0; lv < f.n_levels; lv++)
            for (int k = f.level_start[lv]; k < f.level_start[lv + 1]; k++) val[nl + k] = val[f.node_l[k]] + val[f.node_r[k]];
        T acc = val[f.roots[0]];
        for (size_t k = 1; k < f.roots.size(); k++) acc += val[f.roots[k]];
        out[c] = acc;
    }
}
}  // namespace

extern "C" {
float npsum_f32(const float *a, long n) { return pss_np::np_sum(a, n); }
double npsum_f64(const double *a, long n) { return pss_np::np_sum(a, n); }
void npsum_c64(const float *a, long n, float *out)   // a: n complex64 elements, interleaved
{
    const pss_np::Cx<float> s = pss_np::np_sum<4, pss_np::Cx<float>>([&](long i) { return pss_np::Cx<float>{a[2 * i], a[2 * i + 1]}; }, n);
    out[0] = s.re;
    out[1] = s.im;
}
float tabsum_f32(const float *a, int n) { float s; tabsum(a, n, false, &s); return s; }
double tabsum_f64(const double *a, int n) { double s; tabsum(a, n, false, &s); return s; }
void tabsum_c64(const float *a, int n, float *out) { tabsum(a, n, true, out); }
int wave_tree(int n, int cplx) { return pss_np::build_forest(n, cplx != 0).wave_tree ? 1 : 0; }
}

// pss_npsum.h — how np.add.reduce adds a contiguous array, stated ONCE for every host path and every kernel of this library.
//
// The rule (numpy/_core/src/umath/loops_utils.h.src, *_pairwise_sum, driven by the ufunc's 8192-element buffer):
//   * the array is taken in chunks of 8192 ELEMENTS, in order, and the chunk sums are added sequentially: ((S0 + S1) + S2) + ...;
//   * inside a chunk, a block of more than 128 FLOATS is split at n / 2 rounded down to a multiple of 8 and the two halves are added;
//   * a block of 8 .. 128 floats (a leaf) runs 8 strided accumulators r[j] += x[i + j], folds them as
//     ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and adds the last n % 8 floats one by one;
//   * fewer than 8 floats are added one by one, starting from 0.
// A complex array is reduced as its 2 n interleaved floats (chunks of 8192 complex elements): even and odd floats never meet, so the
// real part folds as (r0+r2)+(r4+r6) and the imaginary part as (r1+r3)+(r5+r7).  Counted in complex ELEMENTS that is the real rule with
// ACC = 4 accumulators instead of 8: leaves of at most 16 ACC elements, halves rounded down to multiples of ACC, sequential below ACC.
// Everything below is written in elements with ACC as a parameter, so the real and the complex case are one text.
// Every addition is thereby fixed; what is free is WHO performs it:
//   np_sum       one thread (host, or one device lane) walks the whole rule;
//   build_forest the host writes one group's trees down as tables (leaves, inner nodes by level, roots in chunk order);
//   wg_sum       a workgroup walks those tables: one lane per (leaf, accumulator), one per leaf fold, one per inner node.
// Every unit that includes this header is compiled with -ffp-contract=off: each `+` is one IEEE addition.
// (k_row_meter of pss_squelch.h keeps a leaf pass of its own — np.max taken in the same walk — over the tables built here;
//  oracle/ restates the rule independently: it is the checker.)
#pragma once
#include <cstddef>
#include <initializer_list>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PSS_NP_HD __host__ __device__
#else
#define PSS_NP_HD
#endif

namespace pss_np {

constexpr int CHUNK = 8192;   // NumPy's reduction buffer, in elements
constexpr int LEAF = 128;     // PW_BLOCKSIZE, in floats: a leaf holds at most LEAF / 8 * ACC = 16 ACC elements

// where a block of n > 16 ACC elements is split
template <int ACC = 8>
PSS_NP_HD inline int split_at(int n)
{
    int n2 = n / 2;
    n2 -= n2 % ACC;
    return n2;
}
// the fold of a leaf's accumulators
template <int ACC, class V, class Add>
PSS_NP_HD inline V fold_acc(const V *r, Add add)
{
    static_assert(ACC == 8 || ACC == 4, "8 float accumulators: 8 real or 4 complex elements");
    if constexpr (ACC == 8) return add(add(add(r[0], r[1]), add(r[2], r[3])), add(add(r[4], r[5]), add(r[6], r[7])));
    else return add(add(r[0], r[1]), add(r[2], r[3]));
}

// ---- one thread ------------------------------------------------------------------------------------------------------------------------
// V: the value type (needs V{} = zero and operator+); elem(i) -> element i.  A complex sum is np_sum<4, Cx<T>>.
template <class T>
struct Cx {
    T re, im;
    PSS_NP_HD Cx operator+(const Cx &o) const { return Cx{re + o.re, im + o.im}; }
};

template <int ACC, class V, class F>
PSS_NP_HD inline V leaf_sum(F elem, int a, int n)
{
    if (n < ACC) {
        V r{};
        for (int i = 0; i < n; i++) r = r + elem(a + i);
        return r;
    }
    V r[ACC];
    int i;
    for (int j = 0; j < ACC; j++) r[j] = elem(a + j);
    for (i = ACC; i < n - (n % ACC); i += ACC)
        for (int j = 0; j < ACC; j++) r[j] = r[j] + elem(a + i + j);
    V res = fold_acc<ACC>(r, [](const V &x, const V &y) { return x + y; });
    for (; i < n; i++) res = res + elem(a + i);
    return res;
}
// One chunk of n <= CHUNK elements from element a on.  The recursion sum(a, n) = sum(a, n2) + sum(a + n2, n - n2) as a post-order walk
// over an explicit stack (device code cannot recurse cheaply; a chunk splits at most 7 times): `pa / pn` hold the right halves still
// to be summed, `val` the sums of the left halves waiting for them.
template <int ACC, class V, class F>
PSS_NP_HD inline V chunk_sum(F elem, int a, int n)
{
    int pa[16], pn[16], depth_at[16], sp = 0, vp = 0, depth = 0;
    V val[16];
    int vdepth[16];
    V acc{};
    for (;;) {
        while (n > LEAF / 8 * ACC) {   // descend to the leftmost leaf, remembering the right halves
            const int n2 = split_at<ACC>(n);
            pa[sp] = a + n2, pn[sp] = n - n2, depth_at[sp] = depth + 1, sp++;
            n = n2;
            depth++;
        }
        acc = leaf_sum<ACC, V>(elem, a, n);
        // a right half just finished at `depth` joins the left half waiting at the same depth
        while (vp > 0 && vdepth[vp - 1] == depth) {
            acc = val[vp - 1] + acc;
            vp--;
            depth--;
        }
        if (sp == 0) return acc;
        // acc is a left half at `depth`: park it, go to its right sibling
        val[vp] = acc, vdepth[vp] = depth, vp++;
        sp--;
        a = pa[sp], n = pn[sp], depth = depth_at[sp];
    }
}
// np.add.reduce over n elements (I: int or long)
template <int ACC, class V, class F, class I>
PSS_NP_HD inline V np_sum(F elem, I n)
{
    const I B = CHUNK;
    V acc{};
    for (I st = 0; st < n; st += B) {
        const V c = chunk_sum<ACC, V>([&](int i) { return elem(st + i); }, 0, (int)((n - st) < B ? (n - st) : B));
        acc = st ? acc + c : c;   // the first chunk's sum is taken as it is, not added to a zero
    }
    return acc;
}
template <class T, class I>
PSS_NP_HD inline T np_sum(const T *a, I n)   // a contiguous real array
{
    return np_sum<8, T>([&](I i) { return a[i]; }, n);
}

// ---- the tables ------------------------------------------------------------------------------------------------------------------------
// The forest of ONE GROUP of `len` elements: one pairwise tree per chunk.  Value slots: the leaves in element order (0 .. n_leaves - 1),
// then the inner nodes stably sorted by height (slot n_leaves + k = slot node_l[k] + slot node_r[k]; height h + 1 occupies
// [level_start[h], level_start[h + 1])), so a level needs only the levels below it.  roots: the chunks' slots in chunk order.
// cplx: the tree of a complex reduce, built over the 2 len interleaved FLOATS — leaf offsets / lengths are then in floats (always
// even) and a walker with ACC = 4 halves them.
struct Forest {
    std::vector<int> leaf_off, leaf_len, node_l, node_r, level_start, roots;
    int n_levels = 0;
    // one wavefront can fold the tree with xor shuffles: 64 (leaf, accumulator) pairs over equal full leaves in order, and every node
    // joins two adjacent, equally sized halves (true for 1024 floats and for 1024 complex)
    bool wave_tree = false;
    int n_leaves() const { return (int)leaf_off.size(); }
    int n_nodes() const { return (int)node_l.size(); }
};

inline Forest build_forest(int len, bool cplx = false)
{
    struct Walk {
        std::vector<int> lo, ll, nl, nr, height;
        int go(int off, int n, int &h)   // -> leaf l as l, inner node k as -(k + 1)
        {
            if (n <= LEAF) {
                lo.push_back(off);
                ll.push_back(n);
                h = 0;
                return (int)lo.size() - 1;
            }
            const int n2 = split_at<8>(n);
            int hl, hr;
            const int l = go(off, n2, hl), r = go(off + n2, n - n2, hr);
            h = 1 + (hl > hr ? hl : hr);
            nl.push_back(l);
            nr.push_back(r);
            height.push_back(h);
            return -(int)nl.size();
        }
    } w;
    Forest f;
    const int n = cplx ? 2 * len : len, B = cplx ? 2 * CHUNK : CHUNK;
    for (int st = 0; st < n; st += B) {
        int h;
        f.roots.push_back(w.go(st, (n - st) < B ? (n - st) : B, h));
        f.n_levels = f.n_levels > h ? f.n_levels : h;
    }
    const int nleaf = (int)w.lo.size(), nnode = (int)w.nl.size();
    std::vector<int> order, pos(nnode);
    for (int h = 1; h <= f.n_levels; h++) {
        f.level_start.push_back((int)order.size());
        for (int k = 0; k < nnode; k++)
            if (w.height[k] == h) { pos[k] = (int)order.size(); order.push_back(k); }
    }
    f.level_start.push_back(nnode);
    auto slot = [&](int id) { return id >= 0 ? id : nleaf + pos[-id - 1]; };
    for (int k : order) { f.node_l.push_back(slot(w.nl[k])); f.node_r.push_back(slot(w.nr[k])); }
    for (int &r : f.roots) r = slot(r);
    f.leaf_off = std::move(w.lo);
    f.leaf_len = std::move(w.ll);
    // perfect: level h holds half as many nodes as the one below, node j of it joins slots 2 j and 2 j + 1 of the level below
    bool ok = f.roots.size() == 1 && nleaf * (cplx ? 4 : 8) == 64 && nnode == nleaf - 1 && f.roots[0] == nleaf + nnode - 1;
    for (int l = 0; ok && l < nleaf; l++) ok = f.leaf_len[l] == LEAF && f.leaf_off[l] == LEAF * l;
    for (int h = 0, below = 0, width = nleaf; ok && h < f.n_levels; h++) {
        width /= 2;
        ok = f.level_start[h + 1] - f.level_start[h] == width;
        for (int j = 0; ok && j < width; j++) {
            const int k = f.level_start[h] + j;
            ok = f.node_l[k] == below + 2 * j && f.node_r[k] == below + 2 * j + 1;
        }
        below = nleaf + f.level_start[h];
    }
    f.wave_tree = ok;
    return f;
}

// What a kernel gets: the tables (device pointers, or LDS after plan_to_lds) and their sizes.
struct PlanDev {
    const int *leaf_off, *leaf_len, *node_l, *node_r, *level_start, *roots;
    int n_leaves, n_levels, n_roots, n_nodes;
    int wave_tree;  // see Forest::wave_tree
};
// the tables back to back, in the order of the pointers above
PSS_NP_HD inline int plan_ints(const PlanDev &p)
{
    return p.n_leaves ? 2 * p.n_leaves + 2 * p.n_nodes + (p.n_levels + 1) + p.n_roots : 0;
}
// A frame is reduced in GROUPS of up to RED_K chunks: a group's plan is a forest whose roots are added in order onto the running sum.
// Frames up to RED_K chunks are one (tail) group; longer ones loop over full groups first — the LDS footprint does not grow with the
// frame (1 Mi-sample read buffers, pyspecsdr.py:2236 with SAMPLES = 12).
constexpr int RED_K = 8;
struct RedPlan {
    PlanDev full, tail;
    int n_full, glen;  // full groups of glen elements each, then the tail group (tail.n_leaves may be 0)
};

// Launch geometry of a kernel that walks some RedPlans with wg_sum.  A use: the plan, its accumulators per leaf and its value size.
// The kernel's LDS holds [part: part_slots][val: val_slots] slots of `slot_bytes` each, shared by its uses, then the plans' tables:
// part = ACC values per leaf, val = one per leaf and inner node plus one for the result, both the largest over the uses' groups.
// T: one lane per (leaf, accumulator) pair up to a workgroup of 256.  wave_tree: one wavefront folds every use with shuffles.
struct SumUse { const RedPlan *rp; int acc; size_t value_bytes; };
struct SumGeom {
    int part_slots = 0, val_slots = 0, T = 64;
    size_t plan_bytes = 0;
    bool wave_tree = true;
    size_t slot_bytes = 0;
    size_t lds_bytes() const { return slot_bytes * ((size_t)part_slots + val_slots) + plan_bytes; }
};
inline SumGeom sum_geometry(std::initializer_list<SumUse> uses, size_t slot_bytes)
{
    SumGeom g;
    g.slot_bytes = slot_bytes;
    int lanes = 0;
    for (const SumUse &u : uses) {
        for (const PlanDev *p : {&u.rp->full, &u.rp->tail}) {
            if (!p->n_leaves) continue;
            const int part = (int)((size_t)u.acc * p->n_leaves * u.value_bytes / slot_bytes), vals = p->n_leaves + p->n_nodes + 1;
            g.part_slots = part > g.part_slots ? part : g.part_slots;
            g.val_slots = vals > g.val_slots ? vals : g.val_slots;
            lanes = u.acc * p->n_leaves > lanes ? u.acc * p->n_leaves : lanes;
            g.plan_bytes += sizeof(int) * (size_t)plan_ints(*p);
        }
        g.wave_tree = g.wave_tree && !u.rp->n_full && u.rp->tail.wave_tree;
    }
    g.T = lanes <= 64 ? 64 : (lanes <= 128 ? 128 : 256);
    g.wave_tree = g.wave_tree && g.T == 64;
    return g;
}

#if defined(__HIPCC__)
// ---- one workgroup ---------------------------------------------------------------------------------------------------------------------
// The plan tables are walked with DEPENDENT loads several times per reduction (offsets -> elements, one round per tree level): read
// from global memory that was ~8 us per pass and dominated k_iqcorr (8 passes per frame).  Every workgroup copies the tables it needs
// into LDS once and works from there.
__device__ __forceinline__ void plan_to_lds(PlanDev &p, int *&cur)
{
    if (!p.n_leaves) return;
    const int tid = threadIdx.x, T = blockDim.x;
    int *lo = cur, *ll = lo + p.n_leaves, *nl = ll + p.n_leaves, *nr = nl + p.n_nodes, *ls = nr + p.n_nodes, *rt = ls + p.n_levels + 1;
    for (int i = tid; i < p.n_leaves; i += T) { lo[i] = p.leaf_off[i]; ll[i] = p.leaf_len[i]; }
    for (int i = tid; i < p.n_nodes; i += T) { nl[i] = p.node_l[i]; nr[i] = p.node_r[i]; }
    for (int i = tid; i <= p.n_levels; i += T) ls[i] = p.level_start[i];
    for (int i = tid; i < p.n_roots; i += T) rt[i] = p.roots[i];
    p.leaf_off = lo; p.leaf_len = ll; p.node_l = nl; p.node_r = nr; p.level_start = ls; p.roots = rt;
    cur = rt + p.n_roots;
}

// the value types: float, or a float2 added component-wise (a complex element, or two real sums over the same tree taken in one walk)
__device__ __forceinline__ float vadd(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float2 vadd(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ __forceinline__ float vshfl_xor(float a, int m) { return __shfl_xor(a, m); }
__device__ __forceinline__ float2 vshfl_xor(float2 a, int m) { return make_float2(__shfl_xor(a.x, m), __shfl_xor(a.y, m)); }

// One group.  elem(i) -> element i of the group as a V; ACC = 8: a real plan, ACC = 4: a complex plan.  The tables are in floats: the
// walk below counts floats as the rule does (8 per round of accumulators) and addresses element (float index >> SH).
// The ACC partial sums of a leaf are independent, so a lane owns one (leaf, accumulator) pair — at 1024 elements that is exactly
// one wavefront per frame — and one lane per leaf then folds them and adds the tail elements.  part: ACC values per leaf; val: one per
// slot plus one.  carry / have: the running sum of the groups before this one.
// PRELOAD = false leaves the 16-deep operand preload of full leaves out (the four-ahead form serves them too).  It is the default of the
// complex form: its sums sit between other register-heavy passes of k_iqcorr and the classifier, where the 32 operand registers of a
// float2 preload cost k_iqcorr two occupancy steps (78 -> 106 VGPRs).  The additions and their order are the same either way.
template <class V, int ACC, bool WT = false, bool PRELOAD = (ACC == 8), class F>
__device__ __forceinline__ V wg_sum(const PlanDev &p, V *part, V *val, F elem, V carry, bool have)
{
    constexpr int FULL = LEAF / 8 * ACC, LG = ACC == 8 ? 3 : 2, SH = 3 - LG;   // elements of a full leaf; log2 ACC; log2 floats per element
    const int tid = threadIdx.x, T = blockDim.x;
    if constexpr (WT) {  // the host guarantees: p.wave_tree, a single group (no carry)
        // 64 / ACC full leaves x ACC accumulators = the 64 lanes of a wavefront, and the tree is perfectly balanced — the fold inside a
        // leaf, adjacent halves above it.  IEEE addition is commutative, so an xor-butterfly computes exactly those sums (in every
        // lane): no LDS, no barriers.  (In a wider workgroup every wavefront computes the same sums redundantly.)
        const int lane = tid & 63;
        const int l = lane >> LG, k = lane & (ACC - 1), off = l * FULL;
        V r = elem(off + k);
#pragma unroll
        for (int i = ACC; i < FULL; i += ACC) r = vadd(r, elem(off + i + k));
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) r = vadd(r, vshfl_xor(r, m));
        return r;
    }
    for (int slot = tid; slot < p.n_leaves * ACC; slot += T) {
        const int l = slot >> LG, k = slot & (ACC - 1), off = p.leaf_off[l] >> SH, len = p.leaf_len[l];  // off: elements, len: floats
        if (PRELOAD && len == LEAF) {
            // a full leaf: all 16 operands of this accumulator requested before the dependent chain of additions starts (four ahead,
            // a CU's 2048 threads kept ~64 KB in flight and the pass ran at 3.7 TB/s)
            V v[16];
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = elem(off + ACC * j + k);
            V r = v[0];
#pragma unroll
            for (int j = 1; j < 16; j++) r = vadd(r, v[j]);
            part[slot] = r;
        } else if (len >= 8) {
            // the additions are a dependent chain in numpy's order; the operands are not: fetch four ahead of the chain
            V r = elem(off + k);
            const int end = len - (len % 8);
            int i = 8;
            for (; i + 24 < end; i += 32) {
                const V a = elem(off + (i >> SH) + k), b = elem(off + ((i + 8) >> SH) + k), c = elem(off + ((i + 16) >> SH) + k),
                        d = elem(off + ((i + 24) >> SH) + k);
                r = vadd(vadd(vadd(vadd(r, a), b), c), d);
            }
            for (; i < end; i += 8) r = vadd(r, elem(off + (i >> SH) + k));
            part[slot] = r;
        }
    }
    __syncthreads();
    for (int l = tid; l < p.n_leaves; l += T) {
        const int off = p.leaf_off[l] >> SH, len = p.leaf_len[l];
        V res;
        if (len < 8) {
            res = V{};
            for (int i = 0; i < len; i += 1 << SH) res = vadd(res, elem(off + (i >> SH)));
        } else {
            res = fold_acc<ACC>(part + ACC * l, [](V a, V b) { return vadd(a, b); });
            for (int i = len - (len % 8); i < len; i += 1 << SH) res = vadd(res, elem(off + (i >> SH)));
        }
        val[l] = res;
    }
    __syncthreads();
    for (int lv = 0; lv < p.n_levels; lv++) {
        for (int k = p.level_start[lv] + tid; k < p.level_start[lv + 1]; k += T)
            val[p.n_leaves + k] = vadd(val[p.node_l[k]], val[p.node_r[k]]);
        __syncthreads();
    }
    const int res = p.n_leaves + p.level_start[p.n_levels];  // free slot behind the nodes
    if (tid == 0) {
        V acc = have ? vadd(carry, val[p.roots[0]]) : val[p.roots[0]];
        for (int k = 1; k < p.n_roots; k++) acc = vadd(acc, val[p.roots[k]]);
        val[res] = acc;
    }
    __syncthreads();
    const V sum = val[res];
    __syncthreads();
    return sum;
}
// A whole frame: loop over the groups, elem(i) indexed from the start of the frame.
template <class V, int ACC, bool WT = false, bool PRELOAD = (ACC == 8), class F>
__device__ __forceinline__ V frame_sum(const RedPlan &rp, V *part, V *val, F elem)
{
    if constexpr (WT) return wg_sum<V, ACC, true>(rp.tail, part, val, elem, V{}, false);
    V acc{};
    bool have = false;
    for (int g = 0; g < rp.n_full; g++) {
        const int base = g * rp.glen;
        acc = wg_sum<V, ACC, false, PRELOAD>(rp.full, part, val, [&](int i) { return elem(base + i); }, acc, have);
        have = true;
    }
    if (rp.tail.n_leaves) {
        const int base = rp.n_full * rp.glen;
        acc = wg_sum<V, ACC, false, PRELOAD>(rp.tail, part, val, [&](int i) { return elem(base + i); }, acc, have);
    }
    return acc;
}
#endif  // __HIPCC__

}  // namespace pss_np

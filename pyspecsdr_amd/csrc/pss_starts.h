// pss_starts.h — the ordered start list behind the receivers in which every sample is a candidate start (pss_adsb.hip, pss_ais.hip), stated
// ONCE.  A detect kernel leaves each tile of DT_S starts its own ascending list of uint16 offsets and a count; k_starts_scan turns the
// tiles' counts into offsets and a total, which reaches the host through 8 pinned bytes and one stream synchronisation; k_starts_gather
// lays the lists back to back; a keep pass of the receiver's own applies its one-record rule to neighbours in that list; and the same scan
// ranks the kept starts and writes the true count.  Nothing here knows what a start is.
// The first part compiles with the host compiler alone (tests/adsb_host.cpp, tests/ais_host.cpp; pss_ctx.h takes PssStartList from it).
// The second, the device code and the launches, needs the whole context: a unit defines PSS_STARTS_KERNELS and includes this header
// again behind pss_ctx.h.  The kernels have internal linkage, so each such unit carries its own.
#ifndef PSS_STARTS_H
#define PSS_STARTS_H
#include <cstddef>
#include <cstdint>
#include <string>

namespace pss_starts {

constexpr int DT_T = 1024;                       // threads of a detect workgroup: 16 wavefronts
constexpr int DT_WAVES = DT_T / 64;
constexpr int DT_S = 4096;                       // start positions of a tile
constexpr long DT_GRID_CAP = 1024;               // workgroups of a detect launch: tiles past it are walked by a grid-stride loop
constexpr int SC_T = 1024, SC_PER = 4;           // the scan: 4096 counts a step
constexpr int LS_T = 256;                        // the list kernels
constexpr long LS_GRID_CAP = 2048;
static_assert(DT_S - 1 <= UINT16_MAX, "a tile's offsets are uint16");
static_assert(DT_S / DT_T * DT_WAVES == 64, "one lane per (pass, wavefront) count");

// The one-record rule over an ascending list: a record inside [s_begin, s_end) is kept unless drops(b, a) holds for some record b less
// than `near` away from it.  The list ascends, so those are a's neighbours in it; records outside the window still count as neighbours.
// emit(a) is called for the kept ones, in order.
template <class Rec, class Drops, class Emit>
void keep_starts(const Rec *acc, size_t n, long s_begin, long s_end, long near, Drops drops, Emit emit)
{
    for (size_t k = 0; k < n; k++) {
        const Rec &a = acc[k];
        if (a.s < s_begin || a.s >= s_end) continue;
        bool kept = true;
        size_t q = k;
        while (q > 0 && a.s - acc[q - 1].s < near) q--;
        for (; q < n && acc[q].s - a.s < near && kept; q++)
            if (drops(acc[q], a)) kept = false;
        if (kept) emit(a);
    }
}

// What every windowed call refuses first: n_<noun> samples, of which the buffer holds [buf_index0, buf_index0 + n_buf), and a window
// [begin, end) of `unit`s named <v>_begin, <v>_end.  bad(text) records the refusal and returns its code; 0: nothing to refuse.
template <class Bad>
int window_refusals(Bad bad, const char *noun, long n, long n_buf, long buf_index0, char v, long begin, long end, const char *unit)
{
    using S = std::string;
    if (n < 0 || n > (1l << 60)) return bad((S("n_") + noun + " outside [0, 2^60]").c_str());
    if (n_buf < 0 || buf_index0 < 0 || buf_index0 > n || n_buf > n - buf_index0) return bad((S("the buffer does not lie inside the ") + noun).c_str());
    if (end < begin) return bad((S(1, v) + "_end < " + v + "_begin").c_str());
    if (begin < 0 || end > n) return bad((S("the window does not lie inside the ") + noun).c_str());
    if (end - begin > (1l << 30)) return bad((S("a window of more than 2^30 ") + unit).c_str());
    return 0;
}

}  // namespace pss_starts

struct pss_ctx;

// The list's scratch in the context, grow-only, for whichever receiver ran last: both enqueue on the context's stream alone and synchronise
// it before they read the pin, so their calls on one context are ordered as the gates of pss_squelch.hip are on sq_buf and sq_pin.
struct PssStartList {
    void *buf[2] = {};     // [0] the count of listed starts, the tiles' counts and offsets, the tiles' lists; [1] the receiver's own arrays
    size_t cap[2] = {};
    void *pin = nullptr;   // 8 pinned bytes the count of listed starts lands in
    struct Tiles { long *d_total; int *count, *off; uint16_t *list; };   // list: DT_S slots a tile
    // buffer 0 for n_tiles tiles, and the pin on first use
    int tiles(pss_ctx *ctx, long n_tiles, const char *what, Tiles &t);
    // behind the detect launch (`launch` names it where it failed): the tiles' offsets, and their total n on the host.  Where that is 0
    // nothing follows: *d_count is set to 0.
    int total(pss_ctx *ctx, const Tiles &t, long n_tiles, const char *launch, int32_t *d_count, long &n);
    // out[k] = the k-th listed start as tile * DT_S + its offset in the tile
    template <class I>
    void gather(pss_ctx *ctx, const Tiles &t, long n_tiles, I *out);
    // out[k] = how many of keep[0 .. k) are set; *d_count = how many of all n
    void rank(pss_ctx *ctx, const uint8_t *keep, int *out, long n, int32_t *d_count);
    // the grid of a receiver's list kernel over n listed starts, `per` of them a workgroup: LS_T at a lane each, LS_T / 64 at a wavefront each
    static unsigned list_grid(long n, int per)
    {
        const long blocks = (n + per - 1) / per;
        return (unsigned)(blocks < pss_starts::LS_GRID_CAP ? blocks : pss_starts::LS_GRID_CAP);
    }
};

#endif  // PSS_STARTS_H

#if defined(PSS_STARTS_KERNELS) && !defined(PSS_STARTS_KERNELS_H)
#define PSS_STARTS_KERNELS_H

namespace {

using namespace pss_starts;

// The flagged starts of a tile in ascending order: where oks[k] is set, store(k, slot) is handed the slot of this lane's start of pass k
// (offset k * DT_T + tid) in the tile's list; the return value is the tile's count, the same in every lane.  The 64 counts (pass k,
// wavefront w) go through wcount at slot 16 k + w and every wavefront scans them for itself.  The store is the caller's (LDS or global: the
// slot is summed as a size_t, the form a global address takes it in), and so is the barrier before the next tile writes wcount.
template <class Store>
__device__ __forceinline__ int tile_slots(const bool (&oks)[DT_S / DT_T], int *wcount, int lane, int wave, Store store)
{
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long masks[DT_S / DT_T];
#pragma unroll
    for (int k = 0; k < DT_S / DT_T; k++) {
        masks[k] = __ballot(oks[k]);
        if (lane == 0) wcount[k * DT_WAVES + wave] = __popcll(masks[k]);
    }
    __syncthreads();
    const int own = wcount[lane];
    int inc = own;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    const int excl = inc - own;
    const int total = __shfl(inc, 63);
#pragma unroll
    for (int k = 0; k < DT_S / DT_T; k++) {
        const int before = __shfl(excl, k * DT_WAVES + wave);
        if (oks[k]) store(k, (size_t)before + __popcll(masks[k] & below));
    }
    return total;
}

// The exclusive prefix of n counts and their total, by one workgroup: SC_PER * SC_T counts a step with a carry, SC_PER consecutive counts a
// lane, the lanes' sums scanned by shuffles and the wavefronts' through LDS.  The tiles' counts (int32) and the keep flags (bytes) both go
// through it.
template <class T>
__global__ __launch_bounds__(SC_T) void k_starts_scan(const T *__restrict__ in, int *__restrict__ out, long n, long *__restrict__ total64,
                                                      int32_t *__restrict__ total32)
{
    __shared__ int wsum[SC_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long carry = 0;   // the same in every lane
    for (long b0 = 0; b0 < n; b0 += (long)SC_PER * SC_T) {
        const long k0 = b0 + (long)SC_PER * tid;
        int v[SC_PER], mine = 0;
#pragma unroll
        for (int u = 0; u < SC_PER; u++) {
            v[u] = k0 + u < n ? (int)in[k0 + u] : 0;
            mine += v[u];
        }
        int inc = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < SC_T / 64; w++) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        __syncthreads();
        int run = (int)carry + before + inc - mine;
#pragma unroll
        for (int u = 0; u < SC_PER; u++) {
            if (k0 + u < n) out[k0 + u] = run;
            run += v[u];
        }
        carry += all;
    }
    if (tid == 0) {
        if (total64) *total64 = carry;
        if (total32) *total32 = (int32_t)carry;
    }
}

// out[k] = the k-th listed start as tile * DT_S + its offset in the tile, in the receiver's index type
template <class I>
__global__ __launch_bounds__(LS_T) void k_starts_gather(const int *__restrict__ tile_count, const int *__restrict__ tile_off,
                                                        const uint16_t *__restrict__ tile_list, long n_tiles, I *__restrict__ out)
{
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int c = tile_count[tile], o = tile_off[tile];
        for (int q = threadIdx.x; q < c; q += LS_T) out[o + q] = (I)(tile * DT_S) + (I)tile_list[(size_t)tile * DT_S + q];
    }
}

}  // namespace

inline int PssStartList::tiles(pss_ctx *ctx, long n_tiles, const char *what, Tiles &t)
{
    const size_t o_count = 16, o_off = o_count + sizeof(int) * (size_t)n_tiles, o_list = (o_off + sizeof(int) * (size_t)n_tiles + 15) & ~(size_t)15;
    const int r = pss_ensure_buffer(ctx, &buf[0], &cap[0], o_list + sizeof(uint16_t) * (size_t)n_tiles * DT_S, what);
    if (r) return r;
    if (!pin) PSS_HIP(ctx, hipHostMalloc(&pin, sizeof(long), hipHostMallocDefault));
    char *b0 = reinterpret_cast<char *>(buf[0]);
    t = {reinterpret_cast<long *>(b0), reinterpret_cast<int *>(b0 + o_count), reinterpret_cast<int *>(b0 + o_off), reinterpret_cast<uint16_t *>(b0 + o_list)};
    return PSS_OK;
}

inline int PssStartList::total(pss_ctx *ctx, const Tiles &t, long n_tiles, const char *launch, int32_t *d_count, long &n)
{
    pss_kernel_begin(ctx, "k_starts_scan");
    hipLaunchKernelGGL(k_starts_scan<int>, dim3(1), dim3(SC_T), 0, PSS_STREAM(ctx), t.count, t.off, n_tiles, t.d_total, static_cast<int32_t *>(nullptr));
    pss_kernel_end(ctx);
    const int r = pss_hip_check(ctx, hipGetLastError(), launch);
    if (r) return r;
    // the list's length sizes what follows: it reaches the host through 8 pinned bytes and one stream synchronisation, as the gates' counts do
    PSS_HIP(ctx, hipMemcpyAsync(pin, t.d_total, sizeof(long), hipMemcpyDeviceToHost, PSS_STREAM(ctx)));
    PSS_HIP(ctx, hipStreamSynchronize(PSS_STREAM(ctx)));
    n = *reinterpret_cast<const long *>(pin);
    if (n == 0) PSS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), PSS_STREAM(ctx)));
    return PSS_OK;
}

template <class I>
inline void PssStartList::gather(pss_ctx *ctx, const Tiles &t, long n_tiles, I *out)
{
    pss_kernel_begin(ctx, "k_starts_gather");
    hipLaunchKernelGGL(k_starts_gather<I>, dim3((unsigned)(n_tiles < LS_GRID_CAP ? n_tiles : LS_GRID_CAP)), dim3(LS_T), 0, PSS_STREAM(ctx), t.count, t.off,
                       t.list, n_tiles, out);
    pss_kernel_end(ctx);
}

inline void PssStartList::rank(pss_ctx *ctx, const uint8_t *keep, int *out, long n, int32_t *d_count)
{
    pss_kernel_begin(ctx, "k_starts_scan");
    hipLaunchKernelGGL(k_starts_scan<uint8_t>, dim3(1), dim3(SC_T), 0, PSS_STREAM(ctx), keep, out, n, static_cast<long *>(nullptr), d_count);
    pss_kernel_end(ctx);
}

#endif  // PSS_STARTS_KERNELS

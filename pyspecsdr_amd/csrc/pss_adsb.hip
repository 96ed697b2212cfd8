// pss_adsb.hip — Mode S / ADS-B: from a 1090 MHz capture to the frames that pass their check.  The arithmetic is pss_adsb.h's; this unit
// places it.
//   k_adsb_detect  a workgroup walks tiles of DT_S start positions.  Per tile the magnitudes of the tile and its reach go to LDS once, the
//                  sliding sums B[i] = m[i] + ... + m[i + spc - 1] are built from them in the stated order (E(c) of start s is B[s + spc c]),
//                  every lane tests the preamble of consecutive starts (16 LDS reads at unit stride across lanes; a tile without a survivor
//                  ends there), ballots and the wavefront counts compact the survivors in ascending order, one wavefront per survivor reads
//                  the 112 bits out of two ballots and checks them, and the accepted starts of the tile are compacted again into the tile's
//                  own list.  The next tile's samples are fetched into registers while this one is worked on.
//   pss_starts.h   k_starts_scan and k_starts_gather, shared with pss_ais.hip: the tiles' counts become offsets and a total, the tiles' lists
//                  are laid back to back (the ascending list of accepted starts as int offsets from e0: no atomics, no cap), and behind
//                  the keep pass the same scan ranks the kept starts and writes the true count.
//   k_adsb_keep    one wavefront per accepted start inside the window: its message and score again from global memory, and those of the
//                  accepted starts less than 2 spc away (they are its neighbours in the list): the one-record-per-frame rule.
//   k_adsb_emit    one wavefront per kept start below max_frames: the record.
// Compiled without contraction (pyspecsdr_amd/build.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pss_adsb.h"
#include "pss_ctx.h"
#define PSS_STARTS_KERNELS   // this unit launches the list's kernels
#include "pss_starts.h"

namespace {

using namespace pss_adsb;

constexpr int DT_B = DT_S + REACH_CHIPS * MAX_SPC;   // sliding sums of a tile: 6016
constexpr int DT_M = DT_B + MAX_SPC;             // magnitudes under them: 6023, and one of padding
constexpr int DT_LOADS = (DT_M + DT_T - 1) / DT_T;   // samples a thread brings in for a tile: 6

// The message of two ballots (bit l of b0 = message bit l, bit l of b1 = message bit 64 + l): w0 holds message bits 0 .. 63 from its top
// bit down, w1 bits 64 .. 111 likewise; a short frame keeps its first 56.  false: the frame does not fit the capture.
__device__ __forceinline__ bool words_of(unsigned long long b0, unsigned long long b1, long s, int spc, long n_capture, uint64_t &w0, uint64_t &w1,
                                         int &n_bits)
{
    n_bits = bits_of((b0 & 1ull) != 0);
    if (!fits(s, n_bits, spc, n_capture)) return false;
    w0 = __brevll(b0);
    w1 = __brevll(b1);
    if (n_bits == SHORT_BITS) {
        w0 &= ~0xFFull;
        w1 = 0;
    }
    return true;
}
__device__ __forceinline__ uint8_t byte_of(uint64_t w0, uint64_t w1, int j) { return (uint8_t)((j < 8 ? w0 >> (56 - 8 * j) : w1 >> (56 - 8 * (j - 8))) & 0xFFu); }

__global__ __launch_bounds__(DT_T) void k_adsb_detect(const float2 *__restrict__ iq, long buf_lo, long buf_hi, long n_capture, int spc, float ratio,
                                                      const uint32_t *__restrict__ icao, int n_icao, long e0, long n_ext, long n_tiles,
                                                      int *__restrict__ tile_count, uint16_t *__restrict__ tile_list)
{
    __shared__ float ms[DT_M + 1];               // the magnitudes; once the sums stand, the survivors' list
    __shared__ float B[DT_B];
    __shared__ uint8_t acc_s[DT_S];
    __shared__ int wcount[64];
    __shared__ uint32_t pw[LONG_BITS];           // x^k mod the generator
    int *surv = reinterpret_cast<int *>(ms);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    {
        constexpr Powers P;
        if (tid < LONG_BITS) pw[tid] = P.t[tid];   // ordered before its first reader by the barriers of the first tile
    }
    // The samples of a tile and its reach, DT_LOADS a thread, all in flight at once.  A sample the buffer does not hold becomes a zero.  The
    // host has checked that the buffer reaches need_hi = min(n_capture, e1 - 1 + 240 spc).  Where need_hi = n_capture the zeros lie past the
    // capture, and only starts that do not fit read them.  Where need_hi lies inside the capture (a chunk with its halo and no more) the last
    // tile's zeros are ms[cnt - 1 + 240 spc ...]: they enter only the sums B[j], j >= cnt + 239 spc, and the last start of the tile reads no
    // further than B[cnt - 1 + 239 spc].
    float2 x[DT_LOADS];
    auto fetch = [&](long tile) {
        const long g0 = e0 + tile * DT_S;
        const int nm = (e0 + n_ext - g0 < DT_S ? (int)(e0 + n_ext - g0) : DT_S) + REACH_CHIPS * spc + spc - 1;
#pragma unroll
        for (int u = 0; u < DT_LOADS; u++) {
            const int j = tid + u * DT_T;
            const long i = g0 + j;
            x[u] = j < nm && i < buf_hi ? iq[i - buf_lo] : make_float2(0.0f, 0.0f);
        }
    };
    if ((long)blockIdx.x < n_tiles) fetch(blockIdx.x);
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long g0 = e0 + tile * DT_S;
        const int cnt = e0 + n_ext - g0 < DT_S ? (int)(e0 + n_ext - g0) : DT_S;   // >= 1
        const int nb = cnt + REACH_CHIPS * spc;   // <= DT_B: start j of the tile reads B[j + spc c], c < 240
        const int nm = nb + spc - 1;              // <= DT_M
#pragma unroll
        for (int u = 0; u < DT_LOADS; u++) {
            const int j = tid + u * DT_T;
            if (j < nm) ms[j] = mag(x[u].x, x[u].y);
        }
        __syncthreads();
        if (tile + gridDim.x < n_tiles) fetch(tile + gridDim.x);   // the next tile's samples travel while this one is worked on
        for (int j = tid; j < nb; j += DT_T) B[j] = chip_sum([&](long q) { return ms[q]; }, j, spc);
        __syncthreads();
        // ---- the preamble at consecutive starts.  In noise a few starts in a million pass: a tile without one ends here.
        bool oks[DT_S / DT_T];
        bool any = false;
#pragma unroll
        for (int k = 0; k < DT_S / DT_T; k++) {
            const int j = k * DT_T + tid;
            oks[k] = false;
            if (j < cnt && fits(g0 + j, SHORT_BITS, spc, n_capture)) {
                float e[PRE_CHIPS], hi;
#pragma unroll
                for (int c = 0; c < PRE_CHIPS; c++) e[c] = B[j + spc * c];
                oks[k] = preamble(e, ratio, hi);
            }
            any |= oks[k];
        }
        if (__syncthreads_count(any) == 0) {
            if (tid == 0) tile_count[tile] = 0;
            continue;
        }
        // ---- the survivors in ascending order
        const int total = tile_slots(oks, wcount, lane, wave, [&](int k, int slot) { surv[slot] = k * DT_T + tid; });
        __syncthreads();
        // ---- one wavefront per survivor: lane l holds bits l and 64 + l
        for (int q = wave; q < total; q += DT_WAVES) {
            const int j = surv[q];
            const int ca = j + spc * (PRE_CHIPS + 2 * lane), cb = ca + spc * 128;
            const bool bit_a = B[ca] > B[ca + spc];
            const bool bit_b = lane < LONG_BITS - 64 ? B[cb] > B[cb + spc] : false;   // cb + spc <= j + 239 spc < nb
            const unsigned long long b0 = __ballot(bit_a);
            const int n_bits = bits_of((b0 & 1ull) != 0);
            // the remainder: every lane brings the powers of its set bits, six xor shuffles fold them
            uint32_t r = bit_a && lane < n_bits ? pw[n_bits - 1 - lane] : 0u;
            if (bit_b && n_bits == LONG_BITS) r ^= pw[LONG_BITS - 65 - lane];   // bit 64 + lane, lane < 48
            for (int d = 32; d; d >>= 1) r ^= (uint32_t)__shfl_xor((int)r, d);
            const bool ok = fits(g0 + j, n_bits, spc, n_capture) && accepted_r((int)(__brevll(b0) >> 59), r, icao, n_icao);
            if (lane == 0) acc_s[q] = ok ? 1 : 0;
        }
        __syncthreads();
        // ---- the accepted survivors, still ascending, into the tile's list
        int n_acc = 0;
        for (int q0 = 0; q0 < total; q0 += DT_T) {
            const int q = q0 + tid;
            const bool on = q < total && acc_s[q] != 0;
            const unsigned long long mask = __ballot(on);
            if (lane == 0) wcount[wave] = __popcll(mask);
            __syncthreads();
            int before = n_acc, all = 0;
            for (int w = 0; w < DT_WAVES; w++) {
                if (w < wave) before += wcount[w];
                all += wcount[w];
            }
            __syncthreads();
            if (on) tile_list[(size_t)tile * DT_S + before + __popcll(mask & below)] = (uint16_t)surv[q];
            n_acc += all;
        }
        if (tid == 0) tile_count[tile] = n_acc;
        __syncthreads();   // the next tile's staging overwrites the survivors
    }
}

// The message and the score of the accepted start s, by one wavefront from global memory (the start fits the capture, so its preamble and
// its n_bits bits lie in the buffer; a chip past the capture is never asked for).
__device__ __forceinline__ void wave_slice(const float2 *__restrict__ iq, long buf_lo, long s, int spc, long n_capture, int lane, uint64_t &w0, uint64_t &w1,
                                           int &n_bits, float &hi)
{
    auto M = [&](long i) { const float2 x = iq[i - buf_lo]; return mag(x.x, x.y); };
    auto E = [&](int c) { return chip_sum(M, s + (long)spc * c, spc); };
    const long room = (n_capture - s) / spc;
    const int nc = room < REACH_CHIPS ? (int)room : REACH_CHIPS;   // the chips of this start that the capture holds: >= 128
    const float mine = E(lane & (PRE_CHIPS - 1));
    float e[PRE_CHIPS];
#pragma unroll
    for (int c = 0; c < PRE_CHIPS; c++) e[c] = __shfl(mine, c);
    preamble(e, 0.0f, hi);
    const int ca = PRE_CHIPS + 2 * lane, cb = ca + 128;
    const bool bit_a = ca + 1 < nc ? E(ca) > E(ca + 1) : false;
    const bool bit_b = lane < LONG_BITS - 64 && cb + 1 < nc ? E(cb) > E(cb + 1) : false;
    const unsigned long long b0 = __ballot(bit_a), b1 = __ballot(bit_b);
    words_of(b0, b1, s, spc, n_capture, w0, w1, n_bits);
}

__global__ __launch_bounds__(LS_T) void k_adsb_keep(const float2 *__restrict__ iq, long buf_lo, long n_capture, int spc, const int *__restrict__ acc, long n_acc,
                                                    long e0, long s_begin, long s_end, uint8_t *__restrict__ keep)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6), n_waves = (long)gridDim.x * (LS_T / 64);
    for (long k = wave; k < n_acc; k += n_waves) {
        const int a = acc[k];
        const long s_a = e0 + a;
        bool kept = s_a >= s_begin && s_a < s_end;
        if (kept) {
            uint64_t a0, a1, b0, b1;
            int n_a, n_b;
            float hi_a, hi_b;
            wave_slice(iq, buf_lo, s_a, spc, n_capture, lane, a0, a1, n_a, hi_a);
            for (long q = k - 1; kept && q >= 0 && a - acc[q] < 2 * spc; q--) {
                wave_slice(iq, buf_lo, e0 + acc[q], spc, n_capture, lane, b0, b1, n_b, hi_b);
                if (drops(n_b == n_a && b0 == a0 && b1 == a1, e0 + acc[q], hi_b, s_a, hi_a, spc)) kept = false;
            }
            for (long q = k + 1; kept && q < n_acc && acc[q] - a < 2 * spc; q++) {
                wave_slice(iq, buf_lo, e0 + acc[q], spc, n_capture, lane, b0, b1, n_b, hi_b);
                if (drops(n_b == n_a && b0 == a0 && b1 == a1, e0 + acc[q], hi_b, s_a, hi_a, spc)) kept = false;
            }
        }
        if (lane == 0) keep[k] = kept ? 1 : 0;
    }
}

__global__ __launch_bounds__(LS_T) void k_adsb_emit(const float2 *__restrict__ iq, long buf_lo, long n_capture, int spc, const int *__restrict__ acc, long n_acc,
                                                    long e0, const uint8_t *__restrict__ keep, const int *__restrict__ rank, int max_frames,
                                                    uint8_t *__restrict__ d_msg, int64_t *__restrict__ d_pos, uint32_t *__restrict__ d_meta,
                                                    float *__restrict__ d_score)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (LS_T / 64) + (threadIdx.x >> 6), n_waves = (long)gridDim.x * (LS_T / 64);
    for (long k = wave; k < n_acc; k += n_waves) {
        if (!keep[k]) continue;
        const int r = rank[k];
        if (r >= max_frames) continue;
        const long s = e0 + acc[k];
        uint64_t w0, w1;
        int n_bits;
        float hi;
        wave_slice(iq, buf_lo, s, spc, n_capture, lane, w0, w1, n_bits, hi);
        if (lane < MSG_BYTES) d_msg[(size_t)r * MSG_BYTES + lane] = byte_of(w0, w1, lane);
        if (lane == 0) {
            d_pos[r] = s;
            d_meta[r] = meta_of(n_bits, (int)(w0 >> 59));
            d_score[r] = hi;
        }
    }
}

int frames_check(pss_ctx *ctx, const char *who, bool host, const void *iq, long n_buf, long buf_index0, long n_capture, int spc, float ratio, const uint32_t *icao,
                 int n_icao, long s_begin, long s_end, const void *msg, const void *pos, const void *meta, const void *score, const void *count,
                 int max_frames)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    auto off = [](const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (spc < 1 || spc > MAX_SPC) return bad("spc outside [1, 8]");
    if (!std::isfinite(ratio) || ratio < 0.0f) return bad("ratio must be finite and not negative");
    if (const int r = window_refusals(bad, "capture", n_capture, n_buf, buf_index0, 's', s_begin, s_end, "starts")) return r;
    if (max_frames < 0) return bad("max_frames < 0");
    if (n_icao < 0 || n_icao > (int)MAX_ADDRESS) return bad("n_icao outside [0, 2^24]");
    if (!count || (n_buf > 0 && !iq) || (n_icao > 0 && !icao) || (max_frames > 0 && (!msg || !pos || !meta || !score))) return bad("null buffer");
    if (off(iq, 8) || off(pos, 8) || off(meta, 4) || off(score, 4) || off(count, 4) || off(icao, 4)) return bad("a misaligned pointer");
    if (host)
        for (int k = 0; k < n_icao; k++)
            if (icao[k] >= MAX_ADDRESS || (k > 0 && icao[k] <= icao[k - 1])) return bad("the address list must be ascending, unique and below 2^24");
    if (s_begin < s_end) {
        const Reach r = reach_of(s_begin, s_end, spc, n_capture);
        if (buf_index0 > r.e0 || buf_index0 + n_buf < r.need_hi) return bad("the buffer does not cover the window's reach (2 spc - 1 starts either side, 240 spc samples forward)");
    }
    return PSS_OK;
}

}  // namespace

extern "C" int pss_adsb_plan(double fs, int *spc)
{
    auto bad = [&](const char *why) { return pss_fail(nullptr, PSS_E_ARG, std::string("pss_adsb: ") + why); };
    if (!spc) return bad("null argument");
    const int v = std::isfinite(fs) ? plan(fs) : 0;
    if (!v) return bad("fs / 2 000 000 must be an integer in [1, 8] (2, 4, 6 ... 16 MS/s)");
    *spc = v;
    return PSS_OK;
}

extern "C" uint32_t pss_adsb_crc(const uint8_t *msg, int n_bits)
{
    if (!msg || n_bits < 0 || n_bits > LONG_BITS) return 0xFFFFFFFFu;
    return crc24(msg, n_bits & ~7);
}

extern "C" int pss_h_adsb_frames(const float *h_iq, long n_buf, long buf_index0, long n_capture, int spc, float ratio, const uint32_t *h_icao, int n_icao,
                                 long s_begin, long s_end, uint8_t *h_msg, int64_t *h_pos, uint32_t *h_meta, float *h_score, int32_t *h_count,
                                 int max_frames)
{
    const int r = frames_check(nullptr, "pss_adsb_frames", true, h_iq, n_buf, buf_index0, n_capture, spc, ratio, h_icao, n_icao, s_begin, s_end, h_msg, h_pos,
                               h_meta, h_score, h_count, max_frames);
    if (r) return r;
    struct Rec { long s; int n_bits; float hi; uint8_t msg[MSG_BYTES]; };
    std::vector<Rec> acc;
    if (s_begin < s_end) {
        const Reach w = reach_of(s_begin, s_end, spc, n_capture);
        auto M = [&](long i) { const float *x = h_iq + 2 * (size_t)(i - buf_index0); return mag(x[0], x[1]); };
        for (long s = w.e0; s < w.e1; s++) {
            Rec c;
            c.s = s;
            if (candidate(M, s, n_capture, spc, ratio, h_icao, n_icao, c.msg, c.n_bits, c.hi)) acc.push_back(c);
        }
    }
    int total = 0;
    keep_starts(acc.data(), acc.size(), s_begin, s_end, 2 * (long)spc,
        [&](const Rec &b, const Rec &a) { return drops(b.n_bits == a.n_bits && memcmp(b.msg, a.msg, MSG_BYTES) == 0, b.s, b.hi, a.s, a.hi, spc); },
        [&](const Rec &a) {
            if (total < max_frames) {
                memcpy(h_msg + (size_t)total * MSG_BYTES, a.msg, MSG_BYTES);
                h_pos[total] = a.s;
                h_meta[total] = meta_of(a.n_bits, df_of(a.msg));
                h_score[total] = a.hi;
            }
            total++;
        });
    *h_count = total;
    return PSS_OK;
}

extern "C" int pss_adsb_frames(pss_ctx *ctx, const float *d_iq, long n_buf, long buf_index0, long n_capture, int spc, float ratio, const uint32_t *d_icao,
                               int n_icao, long s_begin, long s_end, uint8_t *d_msg, int64_t *d_pos, uint32_t *d_meta, float *d_score, int32_t *d_count,
                               int max_frames)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    int r = frames_check(ctx, "pss_adsb_frames", false, d_iq, n_buf, buf_index0, n_capture, spc, ratio, d_icao, n_icao, s_begin, s_end, d_msg, d_pos, d_meta,
                         d_score, d_count, max_frames);
    if (r) return r;
    if (s_begin == s_end) {
        PSS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), PSS_STREAM(ctx)));
        return PSS_OK;
    }
    const Reach w = reach_of(s_begin, s_end, spc, n_capture);
    const long n_ext = w.e1 - w.e0, n_tiles = (n_ext + DT_S - 1) / DT_S;
    PssStartList &starts = ctx->starts;   // buffer 0: the tiles' counts, offsets and lists
    PssStartList::Tiles t;
    r = starts.tiles(ctx, n_tiles, "pss_adsb_frames tiles", t);
    if (r) return r;
    const float2 *iq = reinterpret_cast<const float2 *>(d_iq);
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_adsb_detect");
    hipLaunchKernelGGL(k_adsb_detect, dim3((unsigned)(n_tiles < DT_GRID_CAP ? n_tiles : DT_GRID_CAP)), dim3(DT_T), 0, PSS_STREAM(ctx), iq, buf_index0,
                       buf_index0 + n_buf, n_capture, spc, ratio, d_icao, n_icao, w.e0, n_ext, n_tiles, t.count, t.list);
    pss_kernel_end(ctx);
    long n_acc;
    r = starts.total(ctx, t, n_tiles, "k_adsb_detect launch", d_count, n_acc);
    if (r || n_acc == 0) return r;
    // buffer 1: the accepted starts, their ranks, their keep flags
    const size_t o_rank = sizeof(int) * (size_t)n_acc, o_keep = 2 * o_rank;
    r = pss_ensure_buffer(ctx, &starts.buf[1], &starts.cap[1], o_keep + (size_t)n_acc, "pss_adsb_frames list");
    if (r) return r;
    char *b1 = reinterpret_cast<char *>(starts.buf[1]);
    int *acc = reinterpret_cast<int *>(b1), *rank = reinterpret_cast<int *>(b1 + o_rank);
    uint8_t *keep = reinterpret_cast<uint8_t *>(b1 + o_keep);
    const dim3 wave_grid(PssStartList::list_grid(n_acc, LS_T / 64));
    starts.gather(ctx, t, n_tiles, acc);   // acc[k] = the k-th accepted start as an offset from e0
    pss_kernel_begin(ctx, "k_adsb_keep");
    hipLaunchKernelGGL(k_adsb_keep, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), iq, buf_index0, n_capture, spc, acc, n_acc, w.e0, s_begin, s_end, keep);
    pss_kernel_end(ctx);
    starts.rank(ctx, keep, rank, n_acc, d_count);   // the ranks of the kept starts, and the true count
    if (max_frames > 0) {
        pss_kernel_begin(ctx, "k_adsb_emit");
        hipLaunchKernelGGL(k_adsb_emit, wave_grid, dim3(LS_T), 0, PSS_STREAM(ctx), iq, buf_index0, n_capture, spc, acc, n_acc, w.e0, keep, rank, max_frames, d_msg,
                           d_pos, d_meta, d_score);
        pss_kernel_end(ctx);
    }
    return pss_hip_check(ctx, hipGetLastError(), "k_adsb_emit launch");
}

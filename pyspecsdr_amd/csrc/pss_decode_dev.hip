// pss_decode_dev.hip — the per-message halves of the reference's decoders (xqtr/PySpecSDR decoders.py) for BATCHES of read buffers, on the
// device (include/pss.h, "decoders for batches"): pss_morse_text, pss_ax25_frames, pss_real_normalise and the one-call entries built from
// them and from pss_morse_edges / pss_afsk_bits.  Each kernel restates its host twin of pss_decode.cpp (pss_h_morse_decode,
// pss_h_ax25_frame) and is compared with it byte for byte (tests/test_gpu_decode_batch.py).  Compiled with -ffp-contract=off: the class
// sums, the distance sums and the gap tree are sequences of single IEEE additions.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pss_ctx.h"
#include "pss_npsum.h"

namespace {

constexpr int MT_GRID_MAX = 4096;    // k_morse_text: one workgroup per frame, at most this many workgroups
constexpr int MT_STAGE = 4096;       // frames with at most this many pulses keep their pulse lengths (seconds) in LDS
constexpr int AX_GRID_MAX = 2048;    // k_ax25_frames: one wavefront per row, four rows per workgroup
constexpr int RN_GRID_MAX = 8192;    // k_real_normalise: one workgroup per row

// ---- decode_morse, back half (decoders.py:165-231) ----------------------------------------------------------------------------------------

// The application's table (pyspecconst.MORSE_CODE as pss_decode.cpp lists it): a symbol of L <= 9 elements is the key (1 << L) | bits,
// element j (0 = the first keyed) at bit L - 1 - j, 1 = dash.  53 entries; entry 52 is the prosign ...---..., three characters.
__device__ const uint16_t MORSE_KEY[53] = {
    0x05, 0x18, 0x1a, 0x0c, 0x02, 0x12, 0x0e, 0x10, 0x04, 0x17, 0x0d, 0x14, 0x07, 0x06, 0x0f, 0x16, 0x1d, 0x0a, 0x08, 0x03, 0x09, 0x11, 0x0b,
    0x19, 0x1b, 0x1c, 0x2f, 0x27, 0x23, 0x21, 0x20, 0x30, 0x38, 0x3c, 0x3e, 0x3f, 0x73, 0x55, 0x4c, 0x32, 0x61, 0x36, 0x6d, 0x28, 0x78, 0x6a,
    0x31, 0x2a, 0x52, 0x89, 0x5a, 0x4d, 0x238};
__device__ const char MORSE_CHR[53] = {'A', 'B', 'C', 'D', 'E', 'F', 'G', 'H', 'I', 'J', 'K', 'L', 'M', 'N', 'O', 'P', 'Q', 'R',
                                       'S', 'T', 'U', 'V', 'W', 'X', 'Y', 'Z', '1', '2', '3', '4', '5', '6', '7', '8', '9', '0',
                                       ',', '.', '?', '/', '-', '(', ')', '&', ':', ';', '=', '+', '"', '$', '@', '_', 'S'};

// One frame's edge lists as the reference trims them (decoders.py:169-172): pulse i runs from rise[i] to fall[off + i]
struct Pulses {
    const int32_t *rise, *fall;   // fall already advanced past a leading fall
    double fs;
    __device__ double dur(int i) const { return (double)((long long)fall[i] - (long long)rise[i]) / fs; }
    __device__ double gap(int i) const { return (double)((long long)rise[i + 1] - (long long)fall[i]) / fs; }
};

// np.add.reduce over the np_ - 1 gaps (pss_npsum.h; np.mean(gaps) of pss_decode.cpp).  One lane.
// (not inlined: one lane runs it once per frame, and inlined its 8 accumulators and divisions cost k_morse_text 52 spilled VGPRs and
// three quarters of its occupancy)
__device__ __attribute__((noinline)) double gap_sum(Pulses p, int n)   // by value: three registers, no stack object in the kernel
{
    return pss_np::np_sum<8, double>([&](int i) { return p.gap(i); }, n);
}

// (dist, threshold) order of two_classes: the smaller mean distance, equal distances keep the smaller threshold
__device__ __forceinline__ bool split_better(bool va, double da, double ta, bool vb, double db, double tb)
{
    if (!va) return false;
    if (!vb) return true;
    return da < db || (da == db && ta < tb);
}

// One workgroup per frame.  d_pulses: the number of complete pulses; 0 = the reference's early returns, -1 = an edge list that was truncated
// (counts > cap), -2 = edges that do not alternate (the host twin returns PSS_E_ARG, the reference's array subtraction raises).
__global__ __launch_bounds__(256) void k_morse_text(const int32_t *__restrict__ rise, const int32_t *__restrict__ fall,
                                                    const int32_t *__restrict__ counts, long n_frames, int cap, double fs, int text_cap,
                                                    uint8_t *__restrict__ text, int32_t *__restrict__ text_len, double *__restrict__ timing,
                                                    int32_t *__restrict__ pulses)
{
    __shared__ double sdur[MT_STAGE];
    __shared__ double tab[257];            // tab[0]: the distinct length below this round's first candidate; tab[1 ..]: the candidates
    __shared__ double red_d[4], red_t[4], red_c0[4], red_c1[4];
    __shared__ int red_v[4], scan_w[4];
    __shared__ double best_s[4];           // dist, threshold, c0, c1 of the best stable split so far
    __shared__ int best_v;
    __shared__ double gap_mean_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long f = blockIdx.x; f < n_frames; f += gridDim.x) {
        uint8_t *out = text + (size_t)f * text_cap;
        int nr = counts[2 * f], nf = counts[2 * f + 1];
        int status = 0, off = 0;
        if (nr > cap || nf > cap) status = -1;
        else if (nr > 0 && nf > 0) {
            off = fall[(size_t)f * cap] < rise[(size_t)f * cap] ? 1 : 0;
            nf -= off;
            if (nr > nf) nr--;
            status = nr != nf ? -2 : nr;
        }
        if (status <= 0) {                 // uniform over the workgroup
            for (int i = tid; i < text_cap; i += 256) out[i] = 0;
            if (tid == 0) {
                text_len[f] = 0;
                pulses[f] = status;
                timing[3 * f] = timing[3 * f + 1] = timing[3 * f + 2] = 0.0;
            }
            continue;
        }
        const int np_ = status;
        const Pulses p{rise + (size_t)f * cap, fall + (size_t)f * cap + off, fs};
        const bool staged = np_ <= MT_STAGE;
        if (staged)
            for (int i = tid; i < np_; i += 256) sdur[i] = p.dur(i);
        if (tid == 0) best_v = 0;
        if (tid == 255) gap_mean_s = np_ > 1 ? gap_sum(p, np_ - 1) / (double)(np_ - 1) : 0.0;
        __syncthreads();
        auto dur = [&](int i) { return staged ? sdur[i] : p.dur(i); };

        double dot, dash;
        if (np_ == 1) {
            dot = dur(0);
            dash = dot * 3;
        } else {
            // ---- two_classes: the candidate splits are the distinct lengths other than the smallest, 256 of them per round
            double below = 0.0;
            bool have_below = false;
            for (;;) {
                int cnt = 0;
                bool any = !have_below;    // the very first entry: the smallest length of all
                double prev = below;       // every lane carries the entry found last: the table is read only behind the barrier below
                if (have_below && tid == 0) tab[0] = below;
                for (int j = have_below ? 1 : 0; j <= 256; j++) {
                    // the smallest length above the previous entry
                    double m = INFINITY;
                    bool got = false;
                    for (int i = tid; i < np_; i += 256) {
                        const double d = dur(i);
                        if ((any || d > prev) && (!got || d < m)) { m = d; got = true; }
                    }
                    for (int o = 32; o > 0; o >>= 1) {
                        const double om = __shfl_xor(m, o);
                        const int og = __shfl_xor((int)got, o);
                        if (og && (!got || om < m)) { m = om; got = true; }
                    }
                    __syncthreads();       // the previous entry's readers are done with red_*
                    if (lane == 0) { red_d[wave] = m; red_v[wave] = got; }
                    __syncthreads();
                    got = false;
                    for (int w = 0; w < 4; w++)
                        if (red_v[w] && (!got || red_d[w] < m)) { m = red_d[w]; got = true; }
                    if (!got) break;       // uniform
                    if (tid == 0) tab[j] = m;
                    prev = m;
                    any = false;
                    cnt = j;
                }
                __syncthreads();
                // ---- one lane per candidate: class sums and the distance sum in observation order, one addition per pulse
                bool valid = false;
                double dist = 0.0, thr = 0.0, c0 = 0.0, c1 = 0.0;
                if (tid < cnt) {
                    thr = tab[tid + 1];
                    const double lo_max = tab[tid];
                    double s0 = 0.0, s1 = 0.0;
                    long k = 0;
                    for (int i = 0; i < np_; i++) {
                        const double d = dur(i);
                        if (d >= thr) s1 += d;
                        else { s0 += d; k++; }
                    }
                    c0 = s0 / (double)k;
                    c1 = s1 / (double)((long)np_ - k);
                    // stable under one Lloyd step: the largest member of the lower class no farther from c0 than from c1 (scipy's argmin
                    // gives a tie to the first centroid), the smallest member of the upper class strictly nearer to c1
                    if ((fabs(lo_max - c0) <= fabs(lo_max - c1)) && (fabs(thr - c1) < fabs(thr - c0))) {
                        for (int i = 0; i < np_; i++) {
                            const double d = dur(i);
                            dist += fabs(d - (d >= thr ? c1 : c0));
                        }
                        dist /= (double)np_;
                        valid = true;
                    }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const int ov = __shfl_xor((int)valid, o);
                    const double od = __shfl_xor(dist, o), ot = __shfl_xor(thr, o), o0 = __shfl_xor(c0, o), o1 = __shfl_xor(c1, o);
                    if (split_better(ov, od, ot, valid, dist, thr)) { valid = true; dist = od; thr = ot; c0 = o0; c1 = o1; }
                }
                if (lane == 0) { red_v[wave] = valid; red_d[wave] = dist; red_t[wave] = thr; red_c0[wave] = c0; red_c1[wave] = c1; }
                __syncthreads();
                if (tid == 0) {
                    bool bv = best_v;
                    double bd = best_s[0], bt = best_s[1], b0 = best_s[2], b1 = best_s[3];
                    for (int w = 0; w < 4; w++)
                        if (split_better(red_v[w], red_d[w], red_t[w], bv, bd, bt)) { bv = true; bd = red_d[w]; bt = red_t[w]; b0 = red_c0[w]; b1 = red_c1[w]; }
                    best_v = bv;
                    best_s[0] = bd, best_s[1] = bt, best_s[2] = b0, best_s[3] = b1;
                }
                if (cnt < 256) break;      // uniform: the lengths are exhausted
                below = tab[256];
                have_below = true;
                __syncthreads();           // tab[256] is read before the next round overwrites the table
            }
            __syncthreads();
            if (best_v) {
                dot = best_s[2];
                dash = best_s[3];
            } else {                       // no stable split: one centroid, the observation-order mean
                double s = 0.0;
                for (int i = 0; i < np_; i++) s += dur(i);
                dot = dash = s / (double)np_;
            }
        }

        // ---- symbols, letters, words: pulse i ends a letter when its gap exceeds 3 dots (the last pulse always does); the letter's
        // characters (+ a space past 7 dots) are that pulse's output, placed by a scan over the pulses
        const double mid = (dot + dash) / 2, g3 = dot * 3, g7 = dot * 7;
        int base = 0;
        for (int c = 0; c < np_; c += 256) {
            const int i = c + tid;
            int nb = 0;
            uint8_t ch[4] = {0, 0, 0, 0};
            if (i < np_) {
                const double g = i + 1 < np_ ? p.gap(i) : 0.0;
                if (i + 1 == np_ || g > g3) {
                    unsigned key = 0;
                    int len = 0;
                    for (int j = i; j >= 0 && len <= 9; j--) {     // back to the pulse behind the previous letter's end
                        if (j < i && p.gap(j) > g3) break;
                        key |= (dur(j) < mid ? 0u : 1u) << len;
                        len++;
                    }
                    int hit = -1;
                    if (len <= 9) {
                        key |= 1u << len;
                        for (int e = 0; e < 53; e++)
                            if (MORSE_KEY[e] == key) hit = e;
                    }
                    if (hit < 0) ch[nb++] = '?';
                    else if (hit == 52) { ch[0] = 'S'; ch[1] = 'O'; ch[2] = 'S'; nb = 3; }
                    else ch[nb++] = (uint8_t)MORSE_CHR[hit];
                    if (i + 1 < np_ && g > g7) ch[nb++] = ' ';
                }
            }
            int incl = nb;
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            __syncthreads();               // the previous chunk's readers are done with scan_w
            if (lane == 63) scan_w[wave] = incl;
            __syncthreads();
            int pos = base + incl - nb;
            for (int w = 0; w < wave; w++) pos += scan_w[w];
            for (int j = 0; j < nb; j++)
                if (pos + j < text_cap) out[pos + j] = ch[j];
            base += scan_w[0] + scan_w[1] + scan_w[2] + scan_w[3];
        }
        for (int i = (base < text_cap ? base : text_cap) + tid; i < text_cap; i += 256) out[i] = 0;
        if (tid == 0) {
            text_len[f] = base;
            pulses[f] = np_;
            timing[3 * f] = dot;
            timing[3 * f + 1] = dash;
            timing[3 * f + 2] = gap_mean_s;
        }
        __syncthreads();                   // the next frame reuses the shared state
    }
}

// ---- decode_ax25_frame + decode_aprs_payload (decoders.py:6-91) --------------------------------------------------------------------------

// the characters str.strip() removes, as far as 7-bit characters go
__device__ __forceinline__ bool py_space7(unsigned ch) { return ch == 0x20 || (ch >= 0x09 && ch <= 0x0d) || (ch >= 0x1c && ch <= 0x1f); }

// One wavefront per row.  The first flag is a parallel search over the raw bytes; the loop behind it runs on 64-bit masks of the row that the
// wavefront loads with one ballot per 64 bits, uniformly in every lane (one lane writes).  Bytes past the packet's length are not written.
__global__ __launch_bounds__(256) void k_ax25_frames(const uint8_t *__restrict__ bits, long n_rows, int n_bits, int out_cap,
                                                     uint8_t *__restrict__ out, int32_t *__restrict__ out_len)
{
    const int lane = threadIdx.x & 63;
    const long wave0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    for (long r = wave0; r < n_rows; r += nwaves) {
        const uint8_t *b = bits + (size_t)r * n_bits;
        uint8_t *o = out + (size_t)r * out_cap;
        // ---- first flag 01111110 in the raw values (a value other than 0 / 1 matches neither)
        int start = -1;
        for (int c = 0; c + 7 < n_bits && start < 0; c += 64) {
            const int i = c + lane;
            bool is = false;
            if (i + 7 < n_bits)
                is = b[i] == 0 && b[i + 1] == 1 && b[i + 2] == 1 && b[i + 3] == 1 && b[i + 4] == 1 && b[i + 5] == 1 && b[i + 6] == 1 && b[i + 7] == 0;
            const unsigned long long m = __ballot(is);
            if (m) start = c + __ffsll((long long)m) - 1 + 8;
        }
        if (start < 0) {
            if (lane == 0) out_len[r] = -1;
            continue;
        }
        // ---- the frame: kept bits up to the end flag in the KEPT stream, the zero after five ones dropped
        int cb = -64;                        // the 64 bits held in `nz` start here
        unsigned long long nz = 0;
        auto bit = [&](int i) -> unsigned {  // bits[i] != 0, i < n_bits, i never decreases by more than the window
            if (i < cb || i >= cb + 64) {
                cb = i & ~63;
                const int k = cb + lane;
                nz = __ballot(k < n_bits && b[k] != 0);
            }
            return (unsigned)((nz >> (i - cb)) & 1ull);
        };
        unsigned win = 0, cur = 0;           // the last 8 kept bits (newest at bit 7); the byte being assembled, LSB first
        int kept = 0, ones = 0, nby = 0;     // nby: completed bytes
        unsigned long long h0 = 0, h1 = 0;   // bytes 0..7 and 8..13 of the frame
        int pend = -1, hdr_len = 0;          // the completed byte not yet known to lie in front of the end flag
        bool found = false;
        int i = start;
        auto commit = [&](int k, unsigned v) {   // byte k of the frame is final
            if (k < 8) h0 |= (unsigned long long)v << (8 * k);
            else if (k < 14) h1 |= (unsigned long long)v << (8 * (k - 8));
            else if (k >= 15) {
                const int pos = hdr_len + (k - 15);
                if (lane == 0 && pos < out_cap) o[pos] = (uint8_t)v;
            }
        };
        auto hbyte = [&](int k) { return (unsigned)((k < 8 ? h0 >> (8 * k) : h1 >> (8 * (k - 8))) & 0xff); };
        auto addr = [&](int a, int e, int pos, bool write) {   // the stripped 7-bit characters of bytes [a, e) -> their count
            int lo = a, hi = e;
            while (lo < hi && py_space7((hbyte(lo) >> 1) & 0x7f)) lo++;
            while (hi > lo && py_space7((hbyte(hi - 1) >> 1) & 0x7f)) hi--;
            if (write && lane == 0)
                for (int k = lo; k < hi; k++)
                    if (pos + (k - lo) < out_cap) o[pos + (k - lo)] = (uint8_t)((hbyte(k) >> 1) & 0x7f);
            return hi - lo;
        };
        while (i < n_bits - 7) {
            const unsigned v = bit(i);
            win = (win >> 1) | (v << 7);
            cur |= v << (kept & 7);
            kept++;
            if ((kept & 7) == 0) {
                if (pend >= 0) commit(nby - 1, (unsigned)pend);
                pend = (int)cur;
                cur = 0;
                nby++;
                // byte 14 complete: bytes 0..13 are final, the header's length places the information field
                if (nby == 15) hdr_len = addr(7, 13, 0, false) + 1 + addr(0, 6, 0, false) + 1;
            }
            ones = v ? ones + 1 : 0;
            if (ones == 5 && i + 1 < n_bits && bit(i + 1) == 0) {   // the transmitter's stuffed zero: dropped, and no flag test on this turn
                i += 2;
                ones = 0;
                continue;
            }
            i += 1;
            if (kept >= 8 && win == 0x7eu) { found = true; break; }
        }
        // the end flag's 8 kept bits leave: exactly one completed byte less, the pending one
        const int n_bytes = found ? (kept - 8) / 8 : kept / 8;
        if (!found && pend >= 0) commit(nby - 1, (unsigned)pend);
        if (n_bytes < 14) {
            if (lane == 0) out_len[r] = -1;
            continue;
        }
        const int ls = addr(7, 13, 0, true);
        if (lane == 0 && ls < out_cap) o[ls] = '>';
        const int ld = addr(0, 6, ls + 1, true);
        if (lane == 0 && ls + 1 + ld < out_cap) o[ls + 1 + ld] = ':';
        if (lane == 0) out_len[r] = ls + 1 + ld + 1 + (n_bytes > 15 ? n_bytes - 15 : 0);
    }
}

// ---- decode_aprs's first lines for a complex64 buffer (decoders.py:121-125) ------------------------------------------------------------------
// np.real is float32, so is np.max(np.abs(.)) (a NaN propagates) and so is the division; sosfilt widens afterwards.  The imaginary parts
// are never read.  One workgroup per row.
__global__ __launch_bounds__(256) void k_real_normalise(const float2 *__restrict__ iq, long n_rows, int n, double *__restrict__ audio)
{
    __shared__ float red[4];
    const int tid = threadIdx.x;
    for (long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const float *a = reinterpret_cast<const float *>(iq + (size_t)r * n);
        float m = 0.0f;
        bool nan = false;
        for (int i = tid; i < n; i += 256) {
            const float v = fabsf(a[2 * (size_t)i]);
            nan = nan || v != v;
            m = v > m ? v : m;
        }
        if (nan) m = __builtin_nanf("");
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(m, off);
            m = (o != o || o > m) ? o : m;
        }
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        m = red[0];
        for (int w = 1; w < 4; w++) m = (red[w] != red[w] || red[w] > m) ? red[w] : m;
        double *o = audio + (size_t)r * n;
        for (int i = tid; i < n; i += 256) o[i] = (double)__fdiv_rn(a[2 * (size_t)i], m);
    }
}

}  // namespace

extern "C" int pss_morse_text(pss_ctx *ctx, const int32_t *d_rise, const int32_t *d_fall, const int32_t *d_counts, long n_frames, int cap,
                              double fs, int text_cap, uint8_t *d_text, int32_t *d_text_len, double *d_timing, int32_t *d_pulses)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_frames < 0 || cap < 0 || text_cap < 0 || !(fs > 0.0)) return pss_fail(ctx, PSS_E_ARG, "pss_morse_text: bad argument (n_frames, cap, text_cap >= 0, fs > 0)");
    PSS_ALIGNED(ctx, "pss_morse_text", PSS_P(d_rise, 4), PSS_P(d_fall, 4), PSS_P(d_counts, 4), PSS_P(d_text_len, 4), PSS_P(d_timing, 8), PSS_P(d_pulses, 4));
    if (n_frames == 0) return PSS_OK;
    if (!d_counts || !d_text_len || !d_timing || !d_pulses || (cap > 0 && (!d_rise || !d_fall)) || (text_cap > 0 && !d_text))
        return pss_fail(ctx, PSS_E_ARG, "pss_morse_text: null buffer");
    pss_kernel_begin(ctx, "k_morse_text");
    hipLaunchKernelGGL(k_morse_text, dim3((unsigned)(n_frames < MT_GRID_MAX ? n_frames : MT_GRID_MAX)), dim3(256), 0, PSS_STREAM(ctx), d_rise, d_fall,
                       d_counts, n_frames, cap, fs, text_cap, d_text, d_text_len, d_timing, d_pulses);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_morse_text launch");
}

extern "C" int pss_ax25_frames(pss_ctx *ctx, const uint8_t *d_bits, long n_rows, int n_bits, int out_cap, uint8_t *d_out, int32_t *d_out_len)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_rows < 0 || n_bits < 0 || out_cap < 0) return pss_fail(ctx, PSS_E_ARG, "pss_ax25_frames: bad argument (n_rows, n_bits, out_cap >= 0)");
    PSS_ALIGNED(ctx, "pss_ax25_frames", PSS_P(d_out_len, 4));
    if (n_rows == 0) return PSS_OK;
    if (!d_out_len || (n_bits > 0 && !d_bits) || (out_cap > 0 && !d_out)) return pss_fail(ctx, PSS_E_ARG, "pss_ax25_frames: null buffer");
    const long groups = (n_rows + 3) / 4;
    pss_kernel_begin(ctx, "k_ax25_frames");
    hipLaunchKernelGGL(k_ax25_frames, dim3((unsigned)(groups < AX_GRID_MAX ? groups : AX_GRID_MAX)), dim3(256), 0, PSS_STREAM(ctx), d_bits, n_rows, n_bits,
                       out_cap, d_out, d_out_len);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_ax25_frames launch");
}

extern "C" int pss_real_normalise(pss_ctx *ctx, const float *d_iq, long n_rows, int n, double *d_audio)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_rows < 0 || n < 0 || (n_rows > 0 && n > 0 && (!d_iq || !d_audio))) return pss_fail(ctx, PSS_E_ARG, "pss_real_normalise: bad argument");
    PSS_ALIGNED(ctx, "pss_real_normalise", PSS_P(d_iq, 8), PSS_P(d_audio, 8));
    if (n_rows == 0 || n == 0) return PSS_OK;
    pss_kernel_begin(ctx, "k_real_normalise");
    hipLaunchKernelGGL(k_real_normalise, dim3((unsigned)(n_rows < RN_GRID_MAX ? n_rows : RN_GRID_MAX)), dim3(256), 0, PSS_STREAM(ctx),
                       reinterpret_cast<const float2 *>(d_iq), n_rows, n, d_audio);
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_real_normalise launch");
}

// ---- one call per batch, from IQ: compositions of the calls above and of pss_morse_edges / pss_afsk_bits, no arithmetic of their own ---------

extern "C" int pss_decode_morse_batch(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, double threshold_db, int cap, int32_t *d_rise,
                                      int32_t *d_fall, int32_t *d_counts, int text_cap, uint8_t *d_text, int32_t *d_text_len, double *d_timing,
                                      int32_t *d_pulses)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_frames < 0 || n < 1 || cap < 0 || text_cap < 0 || !(fs > 0.0))
        return pss_fail(ctx, PSS_E_ARG, "pss_decode_morse_batch: bad argument (n_frames, cap, text_cap >= 0, n >= 1, fs > 0)");
    PSS_ALIGNED(ctx, "pss_decode_morse_batch", PSS_P(d_iq, 8), PSS_P(d_rise, 4), PSS_P(d_fall, 4), PSS_P(d_counts, 4), PSS_P(d_text_len, 4), PSS_P(d_timing, 8),
                PSS_P(d_pulses, 4));
    if (n_frames == 0) return PSS_OK;
    PssTimeScope timed(ctx);
    int r = pss_morse_edges(ctx, d_iq, n_frames, n, threshold_db, cap, d_rise, d_fall, d_counts);
    if (!r) r = pss_morse_text(ctx, d_rise, d_fall, d_counts, n_frames, cap, fs, text_cap, d_text, d_text_len, d_timing, d_pulses);
    return r;
}

extern "C" int pss_decode_aprs_batch(pss_ctx *ctx, const float *d_iq, long n_rows, int n, double fs, const double *sos1200, const double *sos2200,
                                     int nsec, double *d_audio, uint8_t *d_bits, int out_cap, uint8_t *d_out, int32_t *d_out_len)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_rows < 0 || n < 0 || out_cap < 0 || !(fs >= 1200.0))
        return pss_fail(ctx, PSS_E_ARG, "pss_decode_aprs_batch: bad argument (n_rows, n, out_cap >= 0, fs >= 1200)");
    PSS_ALIGNED(ctx, "pss_decode_aprs_batch", PSS_P(d_iq, 8), PSS_P(d_audio, 8), PSS_P(d_out_len, 4));
    if (n_rows == 0) return PSS_OK;
    PssTimeScope timed(ctx);
    int r = pss_real_normalise(ctx, d_iq, n_rows, n, d_audio);
    if (!r) r = pss_afsk_bits(ctx, d_audio, n_rows, n, fs, sos1200, sos2200, nsec, d_bits);
    if (!r) r = pss_ax25_frames(ctx, d_bits, n_rows, pss_afsk_n_bits(n, fs), out_cap, d_out, d_out_len);
    return r;
}

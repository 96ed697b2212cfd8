// pss_squelch.hip — squelch and the header's Peak / Avg meter for batches of read buffers (include/pss.h, "squelch"): the row meter,
// the gate with its host twin, the demodulator on the open frames only, and the one-call step built from them.  Everything here sits
// BEHIND the existing entry points (pss_spectrum_cells, pss_spectrum_post_f64, pss_demod_signal): none of their kernels or schedules
// changes.
// The scanner sweep report (include/pss.h, "scanner sweep report") is the same shape of work and lives here too: scan -> gate ->
// classifier on the detections only, behind pss_scan, pss_scan_threshold and pss_classify.
// The dead-read test (include/pss.h, "replaying a capture") is a third gate over a batch — flags, the same prefix sum, the ascending list —
// and shares the scratch and the pinned count with the other two.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <set>
#include <vector>

#include "pss_ctx.h"
#include "pss_live.h"
#include "pss_squelch.h"

namespace {
using namespace pss_sq;

constexpr int METER_WAVE_MAX_LEN = 2048;   // rows up to this length: one wavefront per row; longer rows: one workgroup per row

int sq_buffer(pss_ctx *ctx, int which, size_t bytes, const char *what, void **out)
{
    const int r = pss_ensure_buffer(ctx, &ctx->sq_buf[which], &ctx->sq_cap[which], bytes, what);
    *out = ctx->sq_buf[which];
    return r;
}

bool gate_args_ok(long n_frames, int every, int phase)
{
    return n_frames >= 0 && n_frames <= INT32_MAX && every >= 0 && phase >= 0 && (every == 0 ? phase == 0 : phase < every);
}
}  // namespace

extern "C" int pss_row_meter_f64(pss_ctx *ctx, const double *d_rows, long n_rows, int len, double *d_peak, double *d_avg)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_rows < 0 || len < 1 || (!d_peak && !d_avg) || (n_rows > 0 && !d_rows)) return pss_fail(ctx, PSS_E_ARG, "pss_row_meter_f64: bad argument");
    PSS_ALIGNED(ctx, "pss_row_meter_f64", PSS_P(d_rows, 8), PSS_P(d_peak, 8), PSS_P(d_avg, 8));
    if (n_rows == 0) return PSS_OK;
    MeterPlans pl{};
    pl.n_full = len > CHUNK ? len / CHUNK : 0;
    const int rem = len - pl.n_full * CHUNK;
    pl.n_chunks = pl.n_full + (rem > 0 ? 1 : 0);
    if (pl.n_full) fill_plan(CHUNK, pl.full);
    if (rem > 0) fill_plan(rem, pl.tail);
    PssTimeScope timed(ctx);
    pss_kernel_begin(ctx, "k_row_meter");
    if (len <= METER_WAVE_MAX_LEN) {
        const long groups = (n_rows + 3) / 4;
        hipLaunchKernelGGL(k_row_meter<64>, dim3((unsigned)(groups < 8192 ? groups : 8192)), dim3(256), 0, PSS_STREAM(ctx), d_rows, n_rows, len, pl, d_peak, d_avg);
    } else {
        hipLaunchKernelGGL(k_row_meter<256>, dim3((unsigned)(n_rows < 4096 ? n_rows : 4096)), dim3(256), 0, PSS_STREAM(ctx), d_rows, n_rows, len, pl, d_peak, d_avg);
    }
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_row_meter launch");
}

// The loop's gate as the loop runs it (pyspecsdr.py:2261, :2288-2291), one frame after the other: pure host code, no context.
extern "C" int pss_h_squelch_gate(const double *peak, long n_frames, double squelch, int every, int phase, double held_in, uint8_t *open, long *n_open,
                                  double *held_out)
{
    if (!gate_args_ok(n_frames, every, phase) || (n_frames > 0 && !peak)) return PSS_E_ARG;
    double held = held_in;
    long count = 0, counter = phase;
    for (long i = 0; i < n_frames; i++) {
        const bool o = held >= squelch;
        if (open) open[i] = o ? 1 : 0;
        count += o;
        counter++;
        if (every > 0 && counter % every == 0) held = peak[i];
    }
    if (n_open) *n_open = count;
    if (held_out) *held_out = held;
    return PSS_OK;
}

extern "C" int pss_squelch_gate(pss_ctx *ctx, const double *d_peak, long n_frames, double squelch, int every, int phase, double held_in, uint8_t *d_open,
                                int32_t *d_open_idx, long *n_open, double *held_out)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!gate_args_ok(n_frames, every, phase) || (n_frames > 0 && !d_peak))
        return pss_fail(ctx, PSS_E_ARG, "pss_squelch_gate: every < 0, phase outside [0, every), a frame count outside [0, 2^31) or a null peak array");
    PSS_ALIGNED(ctx, "pss_squelch_gate", PSS_P(d_peak, 8), PSS_P(d_open_idx, 4));
    if (n_frames == 0) {
        if (n_open) *n_open = 0;
        if (held_out) *held_out = held_in;
        return PSS_OK;
    }
    const long n_tiles = (n_frames + GATE_TILE - 1) / GATE_TILE;
    void *buf;
    int r = sq_buffer(ctx, 0, sizeof(GateResult) + (size_t)n_tiles * sizeof(int), "gate scratch", &buf);
    if (r) return r;
    if (!ctx->sq_pin) PSS_HIP(ctx, hipHostMalloc(&ctx->sq_pin, sizeof(GateResult), hipHostMallocDefault));
    GateResult *d_res = reinterpret_cast<GateResult *>(buf);
    int *tiles = reinterpret_cast<int *>(d_res + 1);
    const dim3 grid((unsigned)(n_tiles < 4096 ? n_tiles : 4096));
    {
        PssTimeScope timed(ctx);
        pss_kernel_begin(ctx, "k_gate_flags");
        hipLaunchKernelGGL(k_gate_flags, grid, dim3(256), 0, PSS_STREAM(ctx), d_peak, n_frames, squelch, every, (long)phase, held_in, d_open, tiles, n_tiles);
        pss_kernel_end(ctx);
        pss_kernel_begin(ctx, "k_gate_scan");
        hipLaunchKernelGGL(k_gate_scan, dim3(1), dim3(256), 0, PSS_STREAM(ctx), tiles, n_tiles, d_peak, n_frames, every, (long)phase, held_in, d_res);
        pss_kernel_end(ctx);
        if (d_open_idx) {
            pss_kernel_begin(ctx, "k_gate_index");
            hipLaunchKernelGGL(k_gate_index, grid, dim3(256), 0, PSS_STREAM(ctx), d_peak, n_frames, squelch, every, (long)phase, held_in, tiles, n_tiles, d_open_idx);
            pss_kernel_end(ctx);
        }
    }
    r = pss_hip_check(ctx, hipGetLastError(), "squelch gate launch");
    if (r) return r;
    // the one place where the count reaches the host: 16 bytes into pinned memory, one stream synchronisation
    PSS_HIP(ctx, hipMemcpyAsync(ctx->sq_pin, d_res, sizeof(GateResult), hipMemcpyDeviceToHost, PSS_STREAM(ctx)));
    PSS_HIP(ctx, hipStreamSynchronize(PSS_STREAM(ctx)));
    const GateResult *h = reinterpret_cast<const GateResult *>(ctx->sq_pin);
    if (n_open) *n_open = h->n_open;
    if (held_out) *held_out = h->held_out;
    return PSS_OK;
}

// dst[k] = frame idx[k] of the batch, k < n_idx (k_gather_frames: 16 bytes per lane, 8 for an odd frame length or a batch that starts 8 bytes off
// a 16-byte boundary).  d_iq aligned to one sample; dst from hipMalloc.  Stream-ordered.
int pss_gather_frames(pss_ctx *ctx, const float *d_iq, long n_frames, int n, const int32_t *d_idx, long n_idx, float *d_dst)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_iq);
    const dim3 grid((unsigned)(n_idx < 2048 ? n_idx : 2048));
    pss_kernel_begin(ctx, "k_gather_frames");
    if (n % 2 == 0 && a % 16 == 0)
        hipLaunchKernelGGL(k_gather_frames<uint4>, grid, dim3(256), 0, PSS_STREAM(ctx), reinterpret_cast<const uint4 *>(d_iq), d_idx, n_idx, n_frames,
                           (long)n / 2, reinterpret_cast<uint4 *>(d_dst));
    else
        hipLaunchKernelGGL(k_gather_frames<uint2>, grid, dim3(256), 0, PSS_STREAM(ctx), reinterpret_cast<const uint2 *>(d_iq), d_idx, n_idx, n_frames,
                           (long)n, reinterpret_cast<uint2 *>(d_dst));
    pss_kernel_end(ctx);
    return pss_hip_check(ctx, hipGetLastError(), "k_gather_frames launch");
}

extern "C" int pss_demod_gated(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, const int32_t *d_open_idx, long n_open,
                               int16_t *d_pcm, double *d_audio)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (mode < PSS_MODE_NFM || mode > PSS_MODE_WFM) return pss_fail(ctx, PSS_E_ARG, "unknown demodulation mode");
    if (n_frames < 0 || n < 1 || n_open < 0 || n_open > n_frames) return pss_fail(ctx, PSS_E_ARG, "pss_demod_gated: n_open outside [0, n_frames] or a bad size");
    if (n_open == 0) return PSS_OK;                 // squelch closed on every frame: nothing is launched, the outputs stay as they are
    if (!d_iq) return pss_fail(ctx, PSS_E_ARG, "pss_demod_gated: null IQ buffer");
    if (n_open == n_frames) return pss_demod_signal(ctx, mode, d_iq, n_frames, n, fs, d_pcm, d_audio);   // an ascending list of all frames: no copy
    if (!d_open_idx) return pss_fail(ctx, PSS_E_ARG, "pss_demod_gated: null index list");
    if (reinterpret_cast<uintptr_t>(d_iq) % 8) return pss_fail(ctx, PSS_E_ARG, "pss_demod_gated: d_iq is not aligned to one complex64 sample (8 bytes)");
    void *gathered;
    int r = sq_buffer(ctx, 1, (size_t)n_open * n * 2 * sizeof(float), "open frames", &gathered);
    if (r) return r;
    PssTimeScope timed(ctx);
    r = pss_gather_frames(ctx, d_iq, n_frames, n, d_open_idx, n_open, reinterpret_cast<float *>(gathered));
    if (!r) r = pss_demod_signal(ctx, mode, reinterpret_cast<const float *>(gathered), n_open, n, fs, d_pcm, d_audio);
    return r;
}

// ---- dead reads (include/pss.h, "replaying a capture") ----------------------------------------------------------------------------------
// The loop's first test on a read buffer (pyspecsdr.py:2237), one frame after the other: pure host code, no context.
extern "C" int pss_h_live_frames(const float *iq, long n_frames, int n, uint8_t *live, int32_t *live_idx, long *n_live)
{
    if (n < 1 || n_frames < 0 || n_frames > INT32_MAX || !n_live || (n_frames > 0 && !iq)) return PSS_E_ARG;
    *n_live = pss_live::live_frames(iq, n_frames, n, live, live_idx);
    return PSS_OK;
}

extern "C" int pss_live_frames(pss_ctx *ctx, const float *d_iq, long n_frames, int n, uint8_t *d_live, int32_t *d_live_idx, long *n_live)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n < 1 || n_frames < 0 || n_frames > INT32_MAX || !n_live || (n_frames > 0 && !d_iq))
        return pss_fail(ctx, PSS_E_ARG, "pss_live_frames: n < 1, a frame count outside [0, 2^31), or a null d_iq / n_live");
    if (n_frames == 0) {
        *n_live = 0;
        return PSS_OK;
    }
    if (reinterpret_cast<uintptr_t>(d_iq) % 8) return pss_fail(ctx, PSS_E_ARG, "pss_live_frames: d_iq is not aligned to one complex64 sample (8 bytes)");
    const long n_tiles = (n_frames + GATE_TILE - 1) / GATE_TILE;
    const size_t tiles_b = (sizeof(GateResult) + (size_t)n_tiles * sizeof(int) + 15) & ~(size_t)15;
    void *buf;
    int r = sq_buffer(ctx, 0, tiles_b + (d_live ? 0 : (size_t)n_frames), "gate scratch", &buf);   // the flags, if the caller keeps none
    if (r) return r;
    if (!ctx->sq_pin) PSS_HIP(ctx, hipHostMalloc(&ctx->sq_pin, sizeof(GateResult), hipHostMallocDefault));
    GateResult *d_res = reinterpret_cast<GateResult *>(buf);
    int *tiles = reinterpret_cast<int *>(d_res + 1);
    uint8_t *flags = d_live ? d_live : reinterpret_cast<uint8_t *>(buf) + tiles_b;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(d_iq);
    const dim3 grid((unsigned)(n_tiles < 4096 ? n_tiles : 4096));
    {
        PssTimeScope timed(ctx);
        pss_kernel_begin(ctx, "k_live_flags");
        if (n <= LIVE_WAVE_MAX_N) {
            const long groups = (n_frames + 3) / 4;
            hipLaunchKernelGGL(k_live_flags<64>, dim3((unsigned)(groups < 8192 ? groups : 8192)), dim3(256), 0, PSS_STREAM(ctx), words, n_frames, n, flags);
        } else {
            hipLaunchKernelGGL(k_live_flags<256>, dim3((unsigned)(n_frames < 4096 ? n_frames : 4096)), dim3(256), 0, PSS_STREAM(ctx), words, n_frames, n, flags);
        }
        pss_kernel_end(ctx);
        pss_kernel_begin(ctx, "k_flag_count");
        hipLaunchKernelGGL(k_flag_count, grid, dim3(256), 0, PSS_STREAM(ctx), flags, n_frames, tiles, n_tiles);
        pss_kernel_end(ctx);
        pss_kernel_begin(ctx, "k_gate_scan");   // the squelch gate's prefix sum; every = 0: it reads no peak
        hipLaunchKernelGGL(k_gate_scan, dim3(1), dim3(256), 0, PSS_STREAM(ctx), tiles, n_tiles, static_cast<const double *>(nullptr), n_frames, 0, 0L, 0.0, d_res);
        pss_kernel_end(ctx);
        if (d_live_idx) {
            pss_kernel_begin(ctx, "k_flag_index");
            hipLaunchKernelGGL(k_flag_index, grid, dim3(256), 0, PSS_STREAM(ctx), flags, n_frames, tiles, n_tiles, d_live_idx);
            pss_kernel_end(ctx);
        }
    }
    r = pss_hip_check(ctx, hipGetLastError(), "live frames launch");
    if (r) return r;
    // as in pss_squelch_gate: the count reaches the host through 16 pinned bytes and one stream synchronisation
    PSS_HIP(ctx, hipMemcpyAsync(ctx->sq_pin, d_res, sizeof(GateResult), hipMemcpyDeviceToHost, PSS_STREAM(ctx)));
    PSS_HIP(ctx, hipStreamSynchronize(PSS_STREAM(ctx)));
    *n_live = reinterpret_cast<const GateResult *>(ctx->sq_pin)->n_open;
    return PSS_OK;
}

// One loop iteration per read buffer WITH the squelch: the display half of pss_frame_pipeline_cells (pss_spectrum_cells: the same kernels), the
// post-processed float64 rows materialised in context scratch, meter -> gate -> demodulator on the open frames.  The gate waits for the count.
extern "C" int pss_frame_pipeline_squelch(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                                          double *d_row_lo, double *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w, int8_t *d_line_a,
                                          int8_t *d_line_b, int16_t *d_pcm, double squelch, int every, int phase, double held_in, double *d_peak,
                                          double *d_avg, uint8_t *d_open, long *n_open, double *held_out)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (mode < PSS_MODE_NFM || mode > PSS_MODE_WFM) return pss_fail(ctx, PSS_E_ARG, "unknown demodulation mode");
    if (!gate_args_ok(n_frames, every, phase)) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_squelch: every < 0 or phase outside [0, every)");
    if (n < 16 || n > 65536 || (n & (n - 1))) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_squelch: n must be a power of two in [16, 65536]");
    if (n_frames > 0 && (!d_db32 || !d_peak || !d_pcm)) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_squelch: null buffer");
    PSS_ALIGNED(ctx, "pss_frame_pipeline_squelch", PSS_P(d_iq, 8), PSS_P(d_db32, 4), PSS_P(d_db64, 8), PSS_P(d_row_lo, 8), PSS_P(d_row_hi, 8), PSS_P(d_pcm, 4), PSS_P(d_peak, 8),
                PSS_P(d_avg, 8));
    if (n_frames == 0) {
        const int r0 = pss_spectrum_cells(ctx, d_iq, 0, n, d_db32, d_db64, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w, d_line_a, d_line_b);
        if (r0) return r0;
        if (n_open) *n_open = 0;
        if (held_out) *held_out = held_in;
        return PSS_OK;
    }
    const size_t row_bytes = (size_t)n_frames * n * sizeof(double), post_bytes = (size_t)n_frames * (n - 4) * sizeof(double);
    void *buf;
    int r = sq_buffer(ctx, 2, (d_db64 ? 0 : row_bytes) + post_bytes + (size_t)n_frames * sizeof(int32_t), "squelch rows", &buf);
    if (r) return r;
    char *b = reinterpret_cast<char *>(buf);
    double *db64 = d_db64 ? d_db64 : reinterpret_cast<double *>(b);
    double *post = reinterpret_cast<double *>(b + (d_db64 ? 0 : row_bytes));
    int32_t *open_idx = reinterpret_cast<int32_t *>(b + (d_db64 ? 0 : row_bytes) + post_bytes);
    PssTimeScope timed(ctx);
    r = pss_spectrum_cells(ctx, d_iq, n_frames, n, d_db32, db64, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w, d_line_a, d_line_b);
    if (!r) r = pss_spectrum_post_f64(ctx, db64, n_frames, n, post, nullptr, nullptr);
    if (!r) r = pss_row_meter_f64(ctx, post, n_frames, n - 4, d_peak, d_avg);
    long count = 0;
    if (!r) r = pss_squelch_gate(ctx, d_peak, n_frames, squelch, every, phase, held_in, d_open, open_idx, &count, held_out);
    if (!r) r = pss_demod_gated(ctx, mode, d_iq, n_frames, n, fs, open_idx, count, d_pcm, nullptr);
    if (!r && n_open) *n_open = count;
    return r;
}

// ---- scanner sweep report ---------------------------------------------------------------------------------------------------------------
// The sweeps' gate as they run it (pyspecsdr.py:2549 / :2555, :1054 / :1059), one slice after the other: pure host code, no context.
extern "C" int pss_h_scan_gate(const float *peak, const double *bw, long n_slices, double threshold_db, double min_bw, uint8_t *hit, int32_t *hit_idx,
                               long *n_hit)
{
    if (n_slices < 0 || n_slices > INT32_MAX || (n_slices > 0 && (!peak || !bw))) return PSS_E_ARG;
    const float thr = (float)threshold_db;   // NEP 50: np.float32 > Python float compares in float32
    long count = 0;
    for (long i = 0; i < n_slices; i++) {
        bool h = false;
        if (peak[i] > thr) h = bw[i] > min_bw;
        if (hit) hit[i] = h ? 1 : 0;
        if (h && hit_idx) hit_idx[count] = (int32_t)i;
        count += h;
    }
    if (n_hit) *n_hit = count;
    return PSS_OK;
}

extern "C" int pss_scan_gate(pss_ctx *ctx, const float *d_peak, const double *d_bw, long n_slices, double threshold_db, double min_bw, uint8_t *d_hit,
                             int32_t *d_hit_idx, long *n_hit)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_slices < 0 || n_slices > INT32_MAX || (n_slices > 0 && (!d_peak || !d_bw)))
        return pss_fail(ctx, PSS_E_ARG, "pss_scan_gate: a slice count outside [0, 2^31) or a null peak / bandwidth array");
    PSS_ALIGNED(ctx, "pss_scan_gate", PSS_P(d_peak, 4), PSS_P(d_bw, 8), PSS_P(d_hit_idx, 4));
    if (n_slices == 0) {
        if (n_hit) *n_hit = 0;
        return PSS_OK;
    }
    const long n_tiles = (n_slices + GATE_TILE - 1) / GATE_TILE;
    void *buf;
    int r = sq_buffer(ctx, 0, sizeof(GateResult) + (size_t)n_tiles * sizeof(int), "gate scratch", &buf);
    if (r) return r;
    if (!ctx->sq_pin) PSS_HIP(ctx, hipHostMalloc(&ctx->sq_pin, sizeof(GateResult), hipHostMallocDefault));
    GateResult *d_res = reinterpret_cast<GateResult *>(buf);
    int *tiles = reinterpret_cast<int *>(d_res + 1);
    const float thr = (float)threshold_db;
    const dim3 grid((unsigned)(n_tiles < 4096 ? n_tiles : 4096));
    {
        PssTimeScope timed(ctx);
        pss_kernel_begin(ctx, "k_scan_flags");
        hipLaunchKernelGGL(k_scan_flags, grid, dim3(256), 0, PSS_STREAM(ctx), d_peak, d_bw, n_slices, thr, min_bw, d_hit, tiles, n_tiles);
        pss_kernel_end(ctx);
        pss_kernel_begin(ctx, "k_gate_scan");   // the squelch gate's prefix sum; every = 0: it reads no peak, held_out = 0
        hipLaunchKernelGGL(k_gate_scan, dim3(1), dim3(256), 0, PSS_STREAM(ctx), tiles, n_tiles, static_cast<const double *>(nullptr), n_slices, 0, 0L, 0.0, d_res);
        pss_kernel_end(ctx);
        if (d_hit_idx) {
            pss_kernel_begin(ctx, "k_scan_index");
            hipLaunchKernelGGL(k_scan_index, grid, dim3(256), 0, PSS_STREAM(ctx), d_peak, d_bw, n_slices, thr, min_bw, tiles, n_tiles, d_hit_idx);
            pss_kernel_end(ctx);
        }
    }
    r = pss_hip_check(ctx, hipGetLastError(), "scan gate launch");
    if (r) return r;
    // as in pss_squelch_gate: the count reaches the host through 16 pinned bytes and one stream synchronisation
    PSS_HIP(ctx, hipMemcpyAsync(ctx->sq_pin, d_res, sizeof(GateResult), hipMemcpyDeviceToHost, PSS_STREAM(ctx)));
    PSS_HIP(ctx, hipStreamSynchronize(PSS_STREAM(ctx)));
    if (n_hit) *n_hit = reinterpret_cast<const GateResult *>(ctx->sq_pin)->n_open;
    return PSS_OK;
}

// One sweep in one call: the chosen scan, the gate on its peaks and bandwidths, the classifier on the detections.  The gate waits for the count.
extern "C" int pss_sweep_report(pss_ctx *ctx, int kind, const float *d_iq, long n_slices, int n, double fs, double threshold_db, double min_bw, float *d_db,
                                float *d_peak, double *d_bw, int32_t *d_count, uint8_t *d_hit, int32_t *d_hit_idx, long *n_hit, int32_t *d_label,
                                double *d_cls_bw, float *d_mi, float *d_flat)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (kind != PSS_SWEEP_INLINE && kind != PSS_SWEEP_DRIVER) return pss_fail(ctx, PSS_E_ARG, "pss_sweep_report: unknown sweep kind");
    if (n_slices < 0 || n_slices > INT32_MAX || !(fs > 0.0)) return pss_fail(ctx, PSS_E_ARG, "pss_sweep_report: a slice count outside [0, 2^31) or fs <= 0");
    if (n_slices > 0 && (!d_iq || !d_peak || !d_bw || !d_hit_idx)) return pss_fail(ctx, PSS_E_ARG, "pss_sweep_report: null d_iq / d_peak / d_bw / d_hit_idx");
    PSS_ALIGNED(ctx, "pss_sweep_report", PSS_P(d_iq, 8), PSS_P(d_db, 4), PSS_P(d_peak, 4), PSS_P(d_bw, 8), PSS_P(d_count, 4), PSS_P(d_hit_idx, 4), PSS_P(d_label, 4),
                PSS_P(d_cls_bw, 8), PSS_P(d_mi, 4), PSS_P(d_flat, 4));
    if (n_slices == 0) {
        if (n_hit) *n_hit = 0;
        return PSS_OK;
    }
    PssTimeScope timed(ctx);
    int r = kind == PSS_SWEEP_INLINE ? pss_scan(ctx, d_iq, n_slices, n, fs, d_db, d_peak, d_bw, d_count)
                                     : pss_scan_threshold(ctx, d_iq, n_slices, n, fs, threshold_db, d_db, d_peak, d_bw, d_count);
    long count = 0;
    if (!r) r = pss_scan_gate(ctx, d_peak, d_bw, n_slices, threshold_db, min_bw, d_hit, d_hit_idx, &count);
    if (!r) r = pss_classify_gated(ctx, d_iq, n_slices, n, fs, d_hit_idx, count, d_label, d_cls_bw, d_mi, d_flat, nullptr);
    if (!r && n_hit) *n_hit = count;
    return r;
}

// scan_frequencies' last step (pyspecsdr.py:1084-1091): the records ordered by frequency (sorted() is stable), the first of every
// round(f / grid) * grid kept.  Python's round() of a float is half to even on the double = nearbyint in the default rounding mode.
extern "C" int pss_h_scan_dedupe(const double *freq, long n, double grid_hz, int32_t *keep, long *n_keep)
{
    if (n < 0 || n > INT32_MAX || !(grid_hz > 0.0) || (n > 0 && (!freq || !keep))) return PSS_E_ARG;
    std::vector<int32_t> order((size_t)n);
    for (long i = 0; i < n; i++) {
        if (!std::isfinite(freq[i])) return PSS_E_ARG;
        order[(size_t)i] = (int32_t)i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return freq[a] < freq[b]; });
    std::set<double> seen;
    long count = 0;
    for (long k = 0; k < n; k++) {
        const double key = std::nearbyint(freq[order[(size_t)k]] / grid_hz) * grid_hz;
        if (seen.insert(key).second) keep[count++] = order[(size_t)k];
    }
    if (n_keep) *n_keep = count;
    return PSS_OK;
}

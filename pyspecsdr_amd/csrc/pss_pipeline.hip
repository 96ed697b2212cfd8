// pss_pipeline.hip — one loop iteration per read buffer for whole batches: the demodulator (pss_demod.hip, through pss_demod_run) with the
// spectrum and the display chain (pss_fft.hip) beside it on the side stream.  Host code and one conversion kernel; compiled with
// pss_demod.hip's flags.
#include <hip/hip_runtime.h>

#include <string>

#include "pss_ctx.h"
#include "pss_rows.h"

extern "C" int pss_spectrum_nfm(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, float *d_db,
                                int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    PSS_ALIGNED(ctx, "pss_spectrum_nfm", PSS_P(d_iq, 8), PSS_P(d_db, 4), PSS_P(d_pcm, 4));
    // The backward IIR pass runs one wavefront per SIMD and is latency-bound; the spectrum kernel (HBM-bound, high
    // occupancy) is launched on a side stream right behind the forward kernel so that the two share the machine
    // (pss_side_*).  Only the fused large-batch NFM path honours PSS_FORK_AFTER_FWD, and reports it in `forked`.
    PssTimeScope timed(ctx);  // nested brackets inside the two calls are no-ops
    PssDemodCall call;
    call.after_fwd = PSS_FORK_AFTER_FWD;
    const int r2 = pss_demod_run(ctx, PSS_MODE_NFM, PssIq{d_iq}, n_frames, n, fs, d_pcm, nullptr, &call);
    int r;
    if (call.forked) {
        r = pss_side_wait(ctx);
        if (!r && !r2) r = pss_on_side(ctx, [&] { return pss_spectrum_db(ctx, d_iq, n_frames, n, d_db); });
        const int rj = pss_side_join(ctx);
        if (!r) r = rj;
    } else {
        r = r2 ? r2 : pss_spectrum_db(ctx, d_iq, n_frames, n, d_db);
    }
    return r2 ? r2 : r;
}

// One iteration of the reference's main loop for a whole batch of read buffers (pyspecsdr.py:2262-2283 + the display call):
// demodulate_signal(samples, fs, mode) -> int16; compute_fft -> dB row; smoothing + median clamp; display accumulator line.
// Rows of either type through the SAME schedule: TR = float (pss_frame_pipeline[_nfm]: float32 dB rows, the contract of the spectrum
// output) or TR = double (pss_frame_pipeline_nfm_f64: the reference's own row type from IQ to cells — compute_fft returns float64 and the
// caller smooths, clamps and draws float64: these are the reference's cells).
namespace {
template <class TR>
inline int pipe_lines(pss_ctx *ctx, int display, const TR *d_post, long nf, int len, const TR *lo, const TR *hi, int n_halo, int window, int disp_h,
                      int disp_w, int8_t *a, int8_t *b)
{
    return display == 2 ? pss_rows::gradient_rows(ctx, d_post, nf, len, lo, hi, n_halo, window, disp_w, a, b)
         : display ? pss_rows::persistence_rows(ctx, d_post, nf, len, lo, hi, n_halo, window, disp_h, disp_w, a)
                   : pss_rows::waterfall_rows(ctx, d_post, nf, len, lo, hi, n_halo, window, disp_w, a, b);
}
}  // namespace

// display: 0 = the waterfall accumulator's newest line (d_glyph, d_colour), 1 = the persistence accumulator's newest trace (d_glyph = row
// index per column, d_colour unused), 2 = the gradient view's newest line (d_glyph = index into ' ._-=+*#@', d_colour).
// d_post == NULL: the post-processed rows are not materialised.  Rows the register select serves (a multiple of 4 points, up to 32 772 /
// float64: 16 388): ONE pass over the dB rows leaves per row the extremes and the row resampled to the display width (disp_w float64
// values: what the accumulators normalise and quantise), and the lines are quantised from those — the same bytes as from materialised rows.
// Other lengths go through a context-owned scratch copy of the rows.
template <class TR>
static int frame_pipeline_impl(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, TR *d_db, TR *d_post,
                               TR *d_row_lo, TR *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w,
                               int8_t *d_glyph, int8_t *d_colour, int16_t *d_pcm, float *d_db32, bool demodulate);
// d_db32 (float64 rows only; NULL otherwise): the dB rows ALSO (or, with d_db == NULL, ONLY) as float32 — compute_fft's float64 value rounded once
// demodulate = false: the display half alone (pss_spectrum_cells): no demodulator, d_pcm unused
template <class TR>
static int frame_pipeline(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, TR *d_db, TR *d_post,
                          TR *d_row_lo, TR *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w,
                          int8_t *d_glyph, int8_t *d_colour, int16_t *d_pcm, float *d_db32 = nullptr, bool demodulate = true)
{
    PssTimeScope timed(ctx);     // one bracket around the whole call (the nested ones inside are no-ops)
    return frame_pipeline_impl<TR>(ctx, mode, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w,
                                   d_glyph, d_colour, d_pcm, d_db32, demodulate);
}

__global__ __launch_bounds__(256) void k_rows_f64_to_f32(const double *__restrict__ src, float *__restrict__ dst, long count)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x) dst[i] = (float)src[i];
}

template <class TR>
static int frame_pipeline_impl(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, TR *d_db, TR *d_post,
                               TR *d_row_lo, TR *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w,
                               int8_t *d_glyph, int8_t *d_colour, int16_t *d_pcm, float *d_db32, bool demodulate)
{
    constexpr bool F64 = sizeof(TR) == 8;
    if (n_frames < 0 || n_halo < 0 || window < 1 || disp_w < 1 || display < 0 || display > 2 || (display == 1 && (disp_h < 1 || disp_h > 127)))
        return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline: bad frame count, halo, window or display geometry");
    if (n < 8) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline: frames of fewer than 8 samples have no post-processed row to draw");
    if (n_frames > 0 && (!d_iq || (!d_db && !d_db32) || !d_row_lo || !d_row_hi || !d_glyph || (!d_colour && display != 1) || (!d_pcm && demodulate)))
        return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline: null buffer");
    double *d_vals = nullptr;
    if (n_frames > 0 && !d_post) {
        const bool direct = pss_post_sel_serves(n, F64) && !(F64 && ctx->f64_plain);
        const size_t need = direct ? (size_t)n_frames * disp_w * sizeof(double) : (size_t)n_frames * (n - 4) * sizeof(TR);
        int rq = pss_ensure_buffer(ctx, &ctx->scratch_post, &ctx->scratch_post_bytes, need, "post-process scratch");
        if (rq) return rq;
        if (direct) d_vals = reinterpret_cast<double *>(ctx->scratch_post);
        else d_post = reinterpret_cast<TR *>(ctx->scratch_post);
    }
    // 1024-point frames, float64 rows, rows not materialised: the transform and the post-process are ONE kernel (pss_spec_post.h; option
    // "fuse_post" = 0: the two kernels) — the float64 rows never go through HBM unless the caller asks for them (d_db)
    bool fused = false;
    if constexpr (F64) fused = ctx->fuse_post && d_vals && pss_spec_post_serves(ctx, n);
    if (n_frames > 0 && !d_db && !fused) {     // float32 rows only, but this path needs the float64 rows in memory: the context's scratch
        int rq = pss_ensure_buffer(ctx, &ctx->scratch_db64, &ctx->scratch_db64_bytes, (size_t)n_frames * n * sizeof(TR), "float64 dB rows");
        if (rq) return rq;
        d_db = reinterpret_cast<TR *>(ctx->scratch_db64);
    }
    // compute_fft of every frame and the display chain behind it, on whichever stream it is queued
    const PssBwdLaunch *beside_bwd = nullptr;      // the deferred backward launch the chain runs beside (NFM / WFM below): the fused kernel's grid allows for it
    auto spectrum_and_chain = [&]() -> int {
        if constexpr (F64) {
            if (fused)
                return pss_spec_post_chain(ctx, d_iq, n_frames, n, d_db32, d_db, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w, d_glyph,
                                           d_colour, d_vals, beside_bwd);
        }
        int q = pss_rows::spectrum_db(ctx, d_iq, n_frames, n, d_db);     // compute_fft sees the samples as read (pyspecsdr.py:2275), not the corrected ones
        if (q) return q;
        if (d_db32 && n_frames > 0) {
            const long count = n_frames * (long)n;
            pss_kernel_begin(ctx, "k_rows_f64_to_f32");
            hipLaunchKernelGGL(k_rows_f64_to_f32, dim3((unsigned)((count + 255) / 256 < 16384 ? (count + 255) / 256 : 16384)), dim3(256), 0, PSS_STREAM(ctx),
                               reinterpret_cast<const double *>(d_db), d_db32, count);
            pss_kernel_end(ctx);
            q = pss_hip_check(ctx, hipGetLastError(), "k_rows_f64_to_f32 launch");
            if (q) return q;
        }
        if (d_vals) return pss_rows::chain_vals(ctx, d_db, n_frames, n, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w, d_glyph, d_colour, d_vals);
        q = pss_rows::post(ctx, d_db, n_frames, n, d_post, d_row_lo + n_halo, d_row_hi + n_halo);
        if (!q) q = pipe_lines(ctx, display, d_post, n_frames, n - 4, d_row_lo, d_row_hi, n_halo, window, disp_h, disp_w, d_glyph, d_colour);
        return q;
    };
    if (!demodulate) return spectrum_and_chain();
    // WFM: demodulate_signal's dispatcher semantics — the frames are IQ-corrected first (signal_processing.py:222-225); the WFM
    // demodulator does it (PssDemodCall::correct): a scalars pre-pass in front of the forward kernel, alone on the machine
    PssDemodCall call;
    call.correct = mode == PSS_MODE_WFM && n_frames > 0;
    PssTimeScope timed(ctx);
    if (mode != PSS_MODE_NFM && mode != PSS_MODE_WFM) {
        // AM / USB / LSB: neither demodulator has the two-phase shape of the FM paths, so the display chain simply runs on the side stream
        // beside the whole demodulator (AM's recurrence kernel keeps two thirds of the SIMDs busy with one wavefront each — the HBM-bound
        // chain fits in beside it).
        const int r = pss_side_fork(ctx);
        if (r) return r;
        const int rd = pss_demod_run(ctx, mode, PssIq{d_iq}, n_frames, n, fs, d_pcm, nullptr, &call);   // main stream
        const int rc = pss_on_side(ctx, spectrum_and_chain);
        const int rj = pss_side_join(ctx);
        return rd ? rd : (rc ? rc : rj);
    }
    // NFM and WFM.  Schedule: forward kernel (VALU-bound, fills the machine) ->
    //   { backward pass (latency-bound, one wavefront per SIMD)  ||  spectrum -> post-process -> display lines }.
    // (WFM until round 4: the chain beside the whole demodulator.  k_wfm_fwd's four workgroups per CU hold 150 of a CU's 160 KB of LDS, so the
    // spectrum kernel's 70 KB workgroups only ran as forward workgroups retired: 1.2 ms for a 0.17 ms kernel, and the chain was the critical path.)
    // Measured alternatives (rounds 2 - 4, NOTEBOOK.md R4-08 and A5; the code of those experiments left the tree in round 5): the spectrum in
    // front of the fork (+2 %); the whole display chain on the side stream from the start (-5 % when the forward kernel reaches the dispatcher
    // first, +8 % when it does not); the two streams on disjoint CU masks (hipExtStreamCreateWithCUMask, 128..240 of 256 CUs for the forward
    // kernel: +5 % at best — both halves of the step scale with the CUs they get); the spectrum kernel handing discriminator rows to the
    // forward kernel (+2 %); everything in order on one stream; forward -> spectrum -> { backward || post-process -> lines }.
    call.after_fwd = PSS_DEFER_BWD;
    int r = pss_demod_run(ctx, mode, PssIq{d_iq}, n_frames, n, fs, d_pcm, nullptr, &call);
    if (call.bwd.flt) {
        // the side stream ALWAYS waits for the main stream here: the chain reads d_iq and writes d_db / the scratch, all ordered on ctx->stream
        beside_bwd = &call.bwd;
        if (!r) r = pss_side_fork(ctx);
        if (!r) r = pss_on_side(ctx, spectrum_and_chain);
        const int rb = call.bwd.launch(ctx);       // main stream; launched whatever happened above (the PCM must be produced)
        const int rj = pss_side_join(ctx);
        if (!r) r = rb ? rb : rj;
    } else if (!r) {
        r = spectrum_and_chain();                  // the demodulator took a path without a separate backward kernel
    }
    return r;
}

// The iteration with the reference's own row type: float64 dB rows, float64 post-processed rows (d_post may be NULL: not materialised) and
// extremes, the waterfall line quantised from those — the cells the reference draws from this IQ, not those of the float32 rows.  The same
// schedule and the same kernel families as the float32 call (register transform with a float64 dB evaluation and 8-byte stores, register
// select on 64-bit keys); option "f64_plain" = 1: the plain round-3 kernels.  n: a power of two in [16, 65536].
extern "C" int pss_frame_pipeline_nfm_f64(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, double *d_db, double *d_post,
                                          double *d_row_lo, double *d_row_hi, int n_halo, int window, int disp_w, int8_t *d_glyph,
                                          int8_t *d_colour, int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n < 16 || n > 65536 || (n & (n - 1))) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_nfm_f64: n must be a power of two in [16, 65536]");
    PSS_ALIGNED(ctx, "pss_frame_pipeline_nfm_f64", PSS_P(d_iq, 8), PSS_P(d_db, 8), PSS_P(d_post, 8), PSS_P(d_row_lo, 8), PSS_P(d_row_hi, 8), PSS_P(d_pcm, 4));
    return frame_pipeline<double>(ctx, PSS_MODE_NFM, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, n_halo, window, 0, 0, disp_w, d_glyph,
                                  d_colour, d_pcm);
}

// ... in ANY demodulation mode and for either batched display accumulator (pss_frame_pipeline's arguments, float64 rows)
extern "C" int pss_frame_pipeline_f64(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, double *d_db, double *d_post,
                                      double *d_row_lo, double *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w,
                                      int8_t *d_line_a, int8_t *d_line_b, int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (mode < PSS_MODE_NFM || mode > PSS_MODE_WFM) return pss_fail(ctx, PSS_E_ARG, "unknown demodulation mode");
    if (n < 16 || n > 65536 || (n & (n - 1))) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_f64: n must be a power of two in [16, 65536]");
    PSS_ALIGNED(ctx, "pss_frame_pipeline_f64", PSS_P(d_iq, 8), PSS_P(d_db, 8), PSS_P(d_post, 8), PSS_P(d_row_lo, 8), PSS_P(d_row_hi, 8), PSS_P(d_pcm, 4));
    return frame_pipeline<double>(ctx, mode, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w, d_line_a,
                                  d_line_b, d_pcm);
}

// The cell-exact iteration with the dB rows materialised as float32 (compute_fft's float64 value rounded once: the spectrum output's own contract),
// and as float64 too if d_db64 != NULL; float64 from the IQ to the cells either way.
extern "C" int pss_frame_pipeline_cells(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                                        double *d_row_lo, double *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w, int8_t *d_line_a,
                                        int8_t *d_line_b, int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (mode < PSS_MODE_NFM || mode > PSS_MODE_WFM) return pss_fail(ctx, PSS_E_ARG, "unknown demodulation mode");
    if (n < 16 || n > 65536 || (n & (n - 1))) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_cells: n must be a power of two in [16, 65536]");
    if (n_frames > 0 && !d_db32) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_cells: d_db32 is null");
    PSS_ALIGNED(ctx, "pss_frame_pipeline_cells", PSS_P(d_iq, 8), PSS_P(d_db32, 4), PSS_P(d_db64, 8), PSS_P(d_row_lo, 8), PSS_P(d_row_hi, 8), PSS_P(d_pcm, 4));
    return frame_pipeline<double>(ctx, mode, d_iq, n_frames, n, fs, d_db64, nullptr, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w, d_line_a,
                                  d_line_b, d_pcm, d_db32);
}

// ... and its display half alone: compute_fft -> post-process -> display line of every frame, no demodulator
extern "C" int pss_spectrum_cells(pss_ctx *ctx, const float *d_iq, long n_frames, int n, float *d_db32, double *d_db64, double *d_row_lo,
                                  double *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w, int8_t *d_line_a, int8_t *d_line_b)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n < 16 || n > 65536 || (n & (n - 1))) return pss_fail(ctx, PSS_E_ARG, "pss_spectrum_cells: n must be a power of two in [16, 65536]");
    if (n_frames > 0 && !d_db32 && !d_db64) return pss_fail(ctx, PSS_E_ARG, "pss_spectrum_cells: no row buffer");
    PSS_ALIGNED(ctx, "pss_spectrum_cells", PSS_P(d_iq, 8), PSS_P(d_db32, 4), PSS_P(d_db64, 8), PSS_P(d_row_lo, 8), PSS_P(d_row_hi, 8));
    return frame_pipeline<double>(ctx, PSS_MODE_NFM, d_iq, n_frames, n, 0.0, d_db64, nullptr, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w,
                                  d_line_a, d_line_b, nullptr, d_db32, false);
}

// One loop iteration per read buffer with a view that has no history (no halo, no window, no extremes): pss_frame_pipeline_cells' dB rows, the
// demodulator's PCM (d_pcm NULL: the display half alone) and what `view` queues behind the post-processed float64 rows.  Schedule: the
// demodulator on the main stream, compute_fft -> float32 rows -> post-process -> view on the side stream (the AM branch of
// frame_pipeline_impl).  The float64 rows go through memory here (d_db64 / d_post, or the context's scratch): these views need the whole
// post-processed row (the bars' percentile, the surface's extremes), and the header's meter reads it in every view.
template <class View>
static int view_pipeline(pss_ctx *ctx, const char *who, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                         double *d_post, int16_t *d_pcm, View view)
{
    if (mode < PSS_MODE_NFM || mode > PSS_MODE_WFM) return pss_fail(ctx, PSS_E_ARG, "unknown demodulation mode");
    if (n < 16 || n > 65536 || (n & (n - 1))) return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": n must be a power of two in [16, 65536]");
    if (n_frames > 0 && (!d_iq || !d_db32)) return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": null buffer");
    if (n_frames == 0) return PSS_OK;
    if (!d_db64) {
        int rq = pss_ensure_buffer(ctx, &ctx->scratch_db64, &ctx->scratch_db64_bytes, (size_t)n_frames * n * sizeof(double), "float64 dB rows");
        if (rq) return rq;
        d_db64 = reinterpret_cast<double *>(ctx->scratch_db64);
    }
    if (!d_post) {
        int rq = pss_ensure_buffer(ctx, &ctx->scratch_post, &ctx->scratch_post_bytes, (size_t)n_frames * (n - 4) * sizeof(double), "post-process scratch");
        if (rq) return rq;
        d_post = reinterpret_cast<double *>(ctx->scratch_post);
    }
    auto display_chain = [&]() -> int {
        int q = pss_spectrum_db_f64(ctx, d_iq, n_frames, n, d_db64);
        if (q) return q;
        const long count = n_frames * (long)n;
        pss_kernel_begin(ctx, "k_rows_f64_to_f32");
        hipLaunchKernelGGL(k_rows_f64_to_f32, dim3((unsigned)((count + 255) / 256 < 16384 ? (count + 255) / 256 : 16384)), dim3(256), 0, PSS_STREAM(ctx),
                           d_db64, d_db32, count);
        pss_kernel_end(ctx);
        q = pss_hip_check(ctx, hipGetLastError(), "k_rows_f64_to_f32 launch");
        if (!q) q = pss_spectrum_post_f64(ctx, d_db64, n_frames, n, d_post, nullptr, nullptr);
        if (!q) q = view(d_post);
        return q;
    };
    PssTimeScope timed(ctx);
    if (!d_pcm) return display_chain();
    const int r = pss_side_fork(ctx);
    if (r) return r;
    const int rd = pss_demod_signal(ctx, mode, d_iq, n_frames, n, fs, d_pcm, nullptr);   // main stream
    const int rc = pss_on_side(ctx, display_chain);
    const int rj = pss_side_join(ctx);
    return rd ? rd : (rc ? rc : rj);
}

// ... with the reference's DEFAULT view (draw_spectrogram): per frame the bars and the scale's range of the post-processed float64 row
// (k_spectrum_bars).
extern "C" int pss_frame_pipeline_bars(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                                       double *d_post, int disp_h, int disp_w, int8_t *d_height, int8_t *d_level, double *d_range, int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_frames < 0 || disp_h < 1 || disp_h > 127 || disp_w < 1) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_bars: bad frame count or display geometry");
    if (n_frames > 0 && (!d_height || !d_level)) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_bars: null buffer");
    PSS_ALIGNED(ctx, "pss_frame_pipeline_bars", PSS_P(d_iq, 8), PSS_P(d_db32, 4), PSS_P(d_db64, 8), PSS_P(d_post, 8), PSS_P(d_range, 8), PSS_P(d_pcm, 4));
    return view_pipeline(ctx, "pss_frame_pipeline_bars", mode, d_iq, n_frames, n, fs, d_db32, d_db64, d_post, d_pcm, [&](const double *post) {
        return pss_spectrum_bars_f64(ctx, post, n_frames, n - 4, disp_h, disp_w, d_height, d_level, d_range);
    });
}

// ... with the surface plot (draw_surface_plot): per frame the magnitudes and the finite extremes of the post-processed float64 row
// (k_surface_mags).
extern "C" int pss_frame_pipeline_surface(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                                          double *d_post, int disp_w, int8_t *d_mag, double *d_range, int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_frames < 0 || disp_w < 2) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_surface: bad frame count or display width");
    if (n_frames > 0 && !d_mag) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_surface: null buffer");
    PSS_ALIGNED(ctx, "pss_frame_pipeline_surface", PSS_P(d_iq, 8), PSS_P(d_db32, 4), PSS_P(d_db64, 8), PSS_P(d_post, 8), PSS_P(d_range, 8), PSS_P(d_pcm, 4));
    return view_pipeline(ctx, "pss_frame_pipeline_surface", mode, d_iq, n_frames, n, fs, d_db32, d_db64, d_post, d_pcm, [&](const double *post) {
        return pss_surface_mags_f64(ctx, post, n_frames, n - 4, disp_w, d_mag, d_range);
    });
}

// ... with the constellation (draw_vector_display): the masks of the read buffers AS READ (the reference hands `samples` to the view, not the
// corrected copy the WFM demodulator works on), and the rows all the same: the header's meter reads them in this view too.
extern "C" int pss_frame_pipeline_vector(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                                         double *d_post, int max_h, int max_w, uint32_t *d_mask, int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (n_frames < 0 || max_h < 1 || max_w < 1) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_vector: bad frame count or screen size");
    if (n_frames > 0 && !d_mask) return pss_fail(ctx, PSS_E_ARG, "pss_frame_pipeline_vector: null buffer");
    PSS_ALIGNED(ctx, "pss_frame_pipeline_vector", PSS_P(d_iq, 8), PSS_P(d_db32, 4), PSS_P(d_db64, 8), PSS_P(d_post, 8), PSS_P(d_mask, 4), PSS_P(d_pcm, 4));
    return view_pipeline(ctx, "pss_frame_pipeline_vector", mode, d_iq, n_frames, n, fs, d_db32, d_db64, d_post, d_pcm, [&](const double *) {
        return pss_vector_masks(ctx, d_iq, n_frames, n, max_h, max_w, d_mask);
    });
}

extern "C" int pss_frame_pipeline_nfm(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, float *d_db, float *d_post,
                                      float *d_row_lo, float *d_row_hi, int n_halo, int window, int disp_w, int8_t *d_glyph,
                                      int8_t *d_colour, int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    PSS_ALIGNED(ctx, "pss_frame_pipeline_nfm", PSS_P(d_iq, 8), PSS_P(d_db, 4), PSS_P(d_post, 4), PSS_P(d_row_lo, 4), PSS_P(d_row_hi, 4), PSS_P(d_pcm, 4));
    return frame_pipeline<float>(ctx, PSS_MODE_NFM, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, n_halo, window, 0, 0, disp_w, d_glyph,
                                 d_colour, d_pcm);
}

extern "C" int pss_frame_pipeline(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db, float *d_post,
                                  float *d_row_lo, float *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w,
                                  int8_t *d_line_a, int8_t *d_line_b, int16_t *d_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (mode < PSS_MODE_NFM || mode > PSS_MODE_WFM) return pss_fail(ctx, PSS_E_ARG, "unknown demodulation mode");
    PSS_ALIGNED(ctx, "pss_frame_pipeline", PSS_P(d_iq, 8), PSS_P(d_db, 4), PSS_P(d_post, 4), PSS_P(d_row_lo, 4), PSS_P(d_row_hi, 4), PSS_P(d_pcm, 4));
    return frame_pipeline<float>(ctx, mode, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, n_halo, window, display, disp_h, disp_w, d_line_a,
                                 d_line_b, d_pcm);
}

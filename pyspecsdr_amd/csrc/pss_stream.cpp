// pss_stream.cpp — the streamed entry points of the C ABI (include/pss.h): a capture in HOST memory goes through the GPU chunk by chunk, upload,
// compute and download overlapping on three streams and two buffer sets.  Host code only.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "pss_ctx.h"
#include "pss_live.h"
#include "pss_rows.h"

extern "C" void *pss_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) return nullptr;  // pinned for every device
    return p;
}

extern "C" void pss_host_free(void *p)
{
    if (p) hipHostFree(p);
}

int PssStreaming::open(pss_ctx *ctx)
{
    if (!up) PSS_HIP(ctx, hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    if (!dn) PSS_HIP(ctx, hipStreamCreateWithFlags(&dn, hipStreamNonBlocking));
    for (hipEvent_t *ev : {up_done, cmp_done, dn_done})
        for (int i = 0; i < 2; i++)
            if (!ev[i]) PSS_HIP(ctx, hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    return PSS_OK;
}

int PssStreaming::ensure(pss_ctx *ctx, int slot, size_t bytes, void **out)
{
    if (cap[slot] < bytes) {
        if (buf[slot]) { PSS_HIP(ctx, hipFree(buf[slot])); buf[slot] = nullptr; cap[slot] = 0; }
        PSS_HIP(ctx, hipMalloc(&buf[slot], bytes));
        cap[slot] = bytes;
    }
    *out = buf[slot];
    return PSS_OK;
}

// a step that reports through the context: on failure its code is the call's
#define PSS_TRY(call)          \
    do {                       \
        int _r = (call);       \
        if (_r) return _r;     \
    } while (0)

namespace {
// The chunk loop of a streamed capture, stated once.  Chunk k lives in buffer set k & 1.  Per chunk, in this order:
//   upload(k)      the HOST waits until chunk k - 2 has been downloaded (the set is free), then the copy on the upload stream, then up_done[b]
//   admit(k)       the compute stream waits for up_done[b] and, from the third chunk on, for dn_done[b]; ADC codes are unpacked behind that
//   ... the caller's step on the compute stream ...
//   computed(k)    cmp_done[b] on the compute stream; the download stream waits for it
//   down(...)      the chunk's results, on the download stream
//   downloaded(k)  dn_done[b]
// upload(j) is a step of its own because a caller whose step makes the host wait queues chunk k + 1's upload in front of chunk k's step.
// Why the host waits in upload(), not the upload stream: this is a synchronous call, the thread has nothing else to do, and so the upload
// itself carries no dependency — an upload behind a hipStreamWaitEvent becomes a barrier packet in whichever hardware queue the upload stream
// shares (the runtime multiplexes streams over a few queues), and sat behind chunk k - 1's kernels there: uploads and compute alternated
// instead of overlapping (21.4 ms per cfg 5 capture; 15 ms with the host-side wait).
// From its construction on — in front of the first queued copy — every way out of the caller's scope drains the three streams: no copy
// touches the caller's host buffers once the call has returned, whatever it returns.  The drain checks nothing, so the code and message of
// the first failure are what the caller sees.
class ChunkLoop {
public:
    struct Chunk { int b; long f0, cnt; };   // buffer set, first frame, frames (the last chunk is short)

    // h_in: the capture, frames of n samples in fmt; a chunk goes up into d_iq[b], or as ADC codes (fmt.codes) into d_codes[b]
    ChunkLoop(pss_ctx *ctx, long n_frames, long chunk, int n, const void *h_in, const PssIqFmt &fmt, void *const *d_iq, void *const *d_codes)
        : n_chunks((n_frames + chunk - 1) / chunk), ctx(ctx), st(ctx->st), n_frames(n_frames), chunk(chunk), n(n),
          h_in(static_cast<const char *>(h_in)), fmt(fmt), d_iq(d_iq), d_codes(d_codes) {}
    ~ChunkLoop() { drain(); }
    ChunkLoop(const ChunkLoop &) = delete;
    ChunkLoop &operator=(const ChunkLoop &) = delete;

    const long n_chunks;

    Chunk at(long k) const
    {
        const long f0 = k * chunk;
        return Chunk{(int)(k & 1), f0, (n_frames - f0) < chunk ? (n_frames - f0) : chunk};
    }
    int upload(long j)
    {
        const Chunk c = at(j);
        const size_t frame_b = (size_t)n * fmt.sample_bytes();
        if (j >= 2) PSS_HIP(ctx, hipEventSynchronize(st.dn_done[c.b]));
        PSS_HIP(ctx, hipMemcpyAsync(fmt.codes ? d_codes[c.b] : d_iq[c.b], h_in + (size_t)c.f0 * frame_b, (size_t)c.cnt * frame_b, hipMemcpyHostToDevice, st.up));
        PSS_HIP(ctx, hipEventRecord(st.up_done[c.b], st.up));
        return PSS_OK;
    }
    int admit(long k)
    {
        const Chunk c = at(k);
        PSS_HIP(ctx, hipStreamWaitEvent(ctx->stream, st.up_done[c.b], 0));
        if (k >= 2) PSS_HIP(ctx, hipStreamWaitEvent(ctx->stream, st.dn_done[c.b], 0));
        return fmt.codes ? pss_unpack_iq(ctx, fmt.container, d_codes[c.b], c.cnt * (long)n, fmt.scale, fmt.h_table256, (float *)d_iq[c.b]) : PSS_OK;
    }
    int computed(long k)
    {
        const int b = (int)(k & 1);
        PSS_HIP(ctx, hipEventRecord(st.cmp_done[b], ctx->stream));
        PSS_HIP(ctx, hipStreamWaitEvent(st.dn, st.cmp_done[b], 0));
        return PSS_OK;
    }
    // `count` items of `per` bytes from d_src to item `at` of the host array h_dst; nothing for an output the caller did not ask for
    int down(void *h_dst, long at, const void *d_src, long count, size_t per)
    {
        if (h_dst && count > 0)
            PSS_HIP(ctx, hipMemcpyAsync(static_cast<char *>(h_dst) + (size_t)at * per, d_src, (size_t)count * per, hipMemcpyDeviceToHost, st.dn));
        return PSS_OK;
    }
    int downloaded(long k) { return pss_hip_check(ctx, hipEventRecord(st.dn_done[k & 1], st.dn), "hipEventRecord(dn_done)"); }
    // every queued copy / kernel of the capture has finished
    void drain()
    {
        if (drained) return;
        drained = true;
        hipStreamSynchronize(ctx->stream);
        hipStreamSynchronize(st.up);
        hipStreamSynchronize(st.dn);
    }

private:
    pss_ctx *ctx;
    PssStreaming &st;
    const long n_frames, chunk;
    const int n;
    const char *h_in;
    const PssIqFmt fmt;
    void *const *d_iq, *const *d_codes;
    bool drained = false;
};
}  // namespace

extern "C" int pss_h_stream_spectrum_nfm(pss_ctx *ctx, const float *h_iq, long n_frames, int n, double fs, long chunk_frames,
                                         float *h_db, int16_t *h_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || !h_pcm || n_frames < 0 || n < 1 || chunk_frames < 1) return pss_fail(ctx, PSS_E_ARG, "bad stream arguments");
    const int n_out = pss_demod_out_len_ctx(ctx, PSS_MODE_NFM, n, fs);
    if (n_out < 0) return pss_fail(ctx, PSS_E_ARG, "sample rate below the target rate");
    if (n_frames == 0) return PSS_OK;
    if (chunk_frames > n_frames) chunk_frames = n_frames;
    const size_t iq_b = (size_t)chunk_frames * n * 2 * sizeof(float), db_b = (size_t)chunk_frames * n * sizeof(float),
                 pcm_b = (size_t)chunk_frames * n_out * 2 * sizeof(int16_t);
    PssStreaming &st = ctx->st;
    PSS_TRY(st.open(ctx));
    void *d_iq[2], *d_db[2], *d_pcm[2];
    for (int i = 0; i < 2; i++) {
        PSS_TRY(st.ensure(ctx, PssStreaming::IQ + i, iq_b, &d_iq[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::DB + i, db_b, &d_db[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::PCM + i, pcm_b, &d_pcm[i]));
    }
    ChunkLoop loop(ctx, n_frames, chunk_frames, n, h_iq, PssIqFmt{}, d_iq, nullptr);
    for (long k = 0; k < loop.n_chunks; k++) {
        const auto [b, f0, cnt] = loop.at(k);
        PSS_TRY(loop.upload(k));
        PSS_TRY(loop.admit(k));
        {
            // chunks of a stream are throughput work: keep them on the fused large-batch kernels, which also overlap the
            // spectrum kernel with the backward pass (the small-batch path measured 1.5x slower here)
            PssFlagScope keep(ctx->no_small_batch, true);
            PSS_TRY(pss_spectrum_nfm(ctx, (const float *)d_iq[b], cnt, n, fs, (float *)d_db[b], (int16_t *)d_pcm[b]));
        }
        PSS_TRY(loop.computed(k));
        PSS_TRY(loop.down(h_db, f0, d_db[b], cnt, (size_t)n * sizeof(float)));
        PSS_TRY(loop.down(h_pcm, f0, d_pcm[b], cnt, (size_t)n_out * 2 * sizeof(int16_t)));
        PSS_TRY(loop.downloaded(k));
    }
    return PSS_OK;
}

// BASELINE.json configs[4] as the host sees it: a long capture streamed through the GPU, and what comes back per frame is
// what the application consumes — the display accumulator's line (waterfall: glyph + colour, persistence: the newest trace's
// row indices) and the int16 PCM — not the dB rows (8 KB per frame of PCIe traffic nobody reads; still available: h_db).
// Per chunk: upload (copy stream) | spectrum + NFM, post-process + row extremes, display lines (compute stream) | download
// (copy stream), two buffer sets.  The row extremes of the whole capture stay in one device array, so a frame's history
// window reaches back across chunk boundaries; h_halo_lo / h_halo_hi (n_halo values each, may be NULL) are the extremes of
// the rows that precede this capture (previous capture, or the left neighbour's tail when the capture is sharded).
// TR = float: float32 dB / post-processed rows (the float32 pipeline's cells); TR = double: compute_fft's own float64 rows from the transform to the
// cells (pss_h_stream_display_nfm_f64: the reference's cells; the capture is PCIe-bound either way).
namespace {
inline int sd_spectrum_nfm(pss_ctx *ctx, const float *d_iq, long cnt, int n, double fs, float *d_db, int16_t *d_pcm) { return pss_spectrum_nfm(ctx, d_iq, cnt, n, fs, d_db, d_pcm); }
inline int sd_spectrum_nfm(pss_ctx *ctx, const float *d_iq, long cnt, int n, double fs, double *d_db, int16_t *d_pcm)
{
    int r = pss_demod(ctx, PSS_MODE_NFM, d_iq, cnt, n, fs, d_pcm, nullptr);
    return r ? r : pss_spectrum_db_f64(ctx, d_iq, cnt, n, d_db);
}
}  // namespace
template <class TR>
static int stream_display(pss_ctx *ctx, const void *h_in, const PssIqFmt &fmt, long n_frames, int n, double fs, long chunk_frames,
                          int mode, int window, int disp_h, int disp_w, const TR *h_halo_lo,
                          const TR *h_halo_hi, int n_halo, int8_t *h_line_a, int8_t *h_line_b, int16_t *h_pcm,
                          TR *h_db, TR *h_row_lo, TR *h_row_hi, int8_t *h_grid_a, int8_t *h_grid_b)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (h_grid_a && (window > 64 || (mode == 0 && !h_grid_b)))
        return pss_fail(ctx, PSS_E_ARG, "stream display grids: window <= 64, and both planes for the waterfall");
    if (fmt.codes) {
        const int rf = pss_iq_check(ctx, fmt.container, fmt.scale, fmt.h_table256);
        if (rf) return rf;
    }
    if (!h_in || !h_pcm || !h_line_a || n_frames < 0 || n < 8 || chunk_frames < 1 || window < 1 || disp_w < 1 || disp_h < 1 ||
        disp_h > 127 || n_halo < 0 || (mode != 0 && mode != 1) || (mode == 0 && !h_line_b) || (n_halo > 0 && (!h_halo_lo || !h_halo_hi)))
        return pss_fail(ctx, PSS_E_ARG, "bad stream-display arguments");
    const int n_out = pss_demod_out_len_ctx(ctx, PSS_MODE_NFM, n, fs);
    if (n_out < 0) return pss_fail(ctx, PSS_E_ARG, "sample rate below the target rate");
    if (n_frames == 0) return PSS_OK;
    if (chunk_frames > n_frames) chunk_frames = n_frames;
    const int m = n - 4;
    const size_t iq_b = (size_t)chunk_frames * n * 2 * sizeof(float), db_b = (size_t)chunk_frames * n * sizeof(TR),
                 post_b = (size_t)chunk_frames * m * sizeof(TR), pcm_b = (size_t)chunk_frames * n_out * 2 * sizeof(int16_t),
                 line_b = (size_t)chunk_frames * disp_w;
    PssStreaming &st = ctx->st;
    PSS_TRY(st.open(ctx));
    void *d_iq[2], *d_db[2], *d_pcm[2], *d_la[2], *d_lb[2] = {nullptr, nullptr}, *d_codes[2] = {nullptr, nullptr};
    void *d_post = nullptr, *d_ext = nullptr;   // post rows of the chunk in flight; [lo | hi] x (n_halo + n_frames)
    const size_t n_ext = (size_t)n_halo + (size_t)n_frames;
    for (int i = 0; i < 2; i++) {
        PSS_TRY(st.ensure(ctx, PssStreaming::IQ + i, iq_b, &d_iq[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::DB + i, db_b, &d_db[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::PCM + i, pcm_b, &d_pcm[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::PLANE_A + i, line_b, &d_la[i]));
        if (mode == 0) PSS_TRY(st.ensure(ctx, PssStreaming::PLANE_B + i, line_b, &d_lb[i]));
        if (fmt.codes) PSS_TRY(st.ensure(ctx, PssStreaming::CODES + i, (size_t)chunk_frames * n * fmt.sample_bytes(), &d_codes[i]));
    }
    PSS_TRY(st.ensure(ctx, PssStreaming::POST, post_b, &d_post));
    PSS_TRY(st.ensure(ctx, PssStreaming::EXTREMES, 2 * n_ext * sizeof(TR), &d_ext));
    // full screens (h_grid_a): after the LAST frame of every chunk the whole grid as the reference redraws it — all lines / traces of the
    // history normalised with the history's current extremes (pyspecsdr.py:1342-1406, :1512-1564) — from the last `window` post-processed
    // rows, which are carried from chunk to chunk in a small device buffer
    void *d_ga[2] = {nullptr, nullptr}, *d_gb[2] = {nullptr, nullptr}, *d_tail[2] = {nullptr, nullptr};
    const size_t grid_b = (size_t)disp_h * disp_w, tail_b = (size_t)window * m * sizeof(TR);
    if (h_grid_a) {
        for (int i = 0; i < 2; i++) {
            PSS_TRY(st.ensure(ctx, PssStreaming::GRID_A + i, grid_b, &d_ga[i]));
            if (mode == 0) PSS_TRY(st.ensure(ctx, PssStreaming::GRID_B + i, grid_b, &d_gb[i]));
            PSS_TRY(st.ensure(ctx, PssStreaming::TAIL + i, tail_b, &d_tail[i]));
        }
    }
    long tail_rows = 0;   // rows of the history held in d_tail[tail_cur], oldest first
    int tail_cur = 0;
    ChunkLoop loop(ctx, n_frames, chunk_frames, n, h_in, fmt, d_iq, d_codes);
    TR *d_lo = reinterpret_cast<TR *>(d_ext), *d_hi = d_lo + n_ext;
    if (n_halo) {
        PSS_HIP(ctx, hipMemcpyAsync(d_lo, h_halo_lo, sizeof(TR) * n_halo, hipMemcpyHostToDevice, ctx->stream));
        PSS_HIP(ctx, hipMemcpyAsync(d_hi, h_halo_hi, sizeof(TR) * n_halo, hipMemcpyHostToDevice, ctx->stream));
    }
    for (long k = 0; k < loop.n_chunks; k++) {
        const auto [b, f0, cnt] = loop.at(k);
        PSS_TRY(loop.upload(k));
        PSS_TRY(loop.admit(k));
        {
            PssFlagScope keep(ctx->no_small_batch, true);   // chunks of a stream are throughput work: fused large-batch kernels
            PSS_TRY(sd_spectrum_nfm(ctx, (const float *)d_iq[b], cnt, n, fs, (TR *)d_db[b], (int16_t *)d_pcm[b]));
        }
        // rows f0 .. f0+cnt-1 of the capture sit at positions n_halo + f0 .. of the extremes arrays; their history reaches
        // back over everything before them (previous chunks and the caller's halo)
        PSS_TRY(pss_rows::post(ctx, (const TR *)d_db[b], cnt, n, (TR *)d_post, d_lo + n_halo + f0, d_hi + n_halo + f0));
        const long before = (long)n_halo + f0;
        const int halo_k = (int)(before < (long)(window - 1) ? before : (long)(window - 1));
        const TR *lo_k = d_lo + n_halo + f0 - halo_k, *hi_k = d_hi + n_halo + f0 - halo_k;
        if (mode == 0) PSS_TRY(pss_rows::waterfall_rows(ctx, (const TR *)d_post, cnt, m, lo_k, hi_k, halo_k, window, disp_w, (int8_t *)d_la[b], (int8_t *)d_lb[b]));
        else PSS_TRY(pss_rows::persistence_rows(ctx, (const TR *)d_post, cnt, m, lo_k, hi_k, halo_k, window, disp_h, disp_w, (int8_t *)d_la[b]));
        if (h_grid_a) {
            // history after this chunk = the last `window` rows of (history before it ++ the chunk's rows)
            const long take = cnt < window ? cnt : window, keep = (tail_rows + take > window) ? window - take : tail_rows;
            TR *dst = (TR *)d_tail[tail_cur ^ 1];
            if (keep > 0)
                PSS_HIP(ctx, hipMemcpyAsync(dst, (const TR *)d_tail[tail_cur] + (size_t)(tail_rows - keep) * m, (size_t)keep * m * sizeof(TR),
                                            hipMemcpyDeviceToDevice, ctx->stream));
            PSS_HIP(ctx, hipMemcpyAsync(dst + (size_t)keep * m, (const TR *)d_post + (size_t)(cnt - take) * m, (size_t)take * m * sizeof(TR),
                                        hipMemcpyDeviceToDevice, ctx->stream));
            tail_cur ^= 1;
            tail_rows = keep + take;
            if (mode == 0) PSS_TRY(pss_rows::waterfall_cells(ctx, dst, (int)tail_rows, m, disp_h, disp_w, (int8_t *)d_ga[b], (int8_t *)d_gb[b]));
            else PSS_TRY(pss_rows::persistence_cells(ctx, dst, (int)tail_rows, m, disp_h, disp_w, (int8_t *)d_ga[b]));
        }
        PSS_TRY(loop.computed(k));
        if (h_grid_a) {
            PSS_TRY(loop.down(h_grid_a, k, d_ga[b], 1, grid_b));
            if (mode == 0) PSS_TRY(loop.down(h_grid_b, k, d_gb[b], 1, grid_b));
        }
        PSS_TRY(loop.down(h_db, f0, d_db[b], cnt, (size_t)n * sizeof(TR)));
        PSS_TRY(loop.down(h_line_a, f0, d_la[b], cnt, (size_t)disp_w));
        if (mode == 0) PSS_TRY(loop.down(h_line_b, f0, d_lb[b], cnt, (size_t)disp_w));
        PSS_TRY(loop.down(h_pcm, f0, d_pcm[b], cnt, (size_t)n_out * 2 * sizeof(int16_t)));
        PSS_TRY(loop.downloaded(k));
    }
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_row_lo) PSS_HIP(ctx, hipMemcpy(h_row_lo, d_lo + n_halo, sizeof(TR) * n_frames, hipMemcpyDeviceToHost));
    if (h_row_hi) PSS_HIP(ctx, hipMemcpy(h_row_hi, d_hi + n_halo, sizeof(TR) * n_frames, hipMemcpyDeviceToHost));
    return PSS_OK;
}

extern "C" int pss_h_stream_display_nfm(pss_ctx *ctx, const float *h_iq, long n_frames, int n, double fs, long chunk_frames,
                                        int mode, int window, int disp_h, int disp_w, const float *h_halo_lo,
                                        const float *h_halo_hi, int n_halo, int8_t *h_line_a, int8_t *h_line_b, int16_t *h_pcm,
                                        float *h_db, float *h_row_lo, float *h_row_hi)
{
    return stream_display<float>(ctx, h_iq, PssIqFmt{}, n_frames, n, fs, chunk_frames, mode, window, disp_h, disp_w, h_halo_lo, h_halo_hi, n_halo, h_line_a,
                                 h_line_b, h_pcm, h_db, h_row_lo, h_row_hi, nullptr, nullptr);
}

// ... with compute_fft's own float64 rows from the transform to the cells: the lines (and grids) the reference draws from this capture
extern "C" int pss_h_stream_display_nfm_f64(pss_ctx *ctx, const float *h_iq, long n_frames, int n, double fs, long chunk_frames,
                                            int mode, int window, int disp_h, int disp_w, const double *h_halo_lo,
                                            const double *h_halo_hi, int n_halo, int8_t *h_line_a, int8_t *h_line_b, int16_t *h_pcm,
                                            double *h_db, double *h_row_lo, double *h_row_hi, int8_t *h_grid_a, int8_t *h_grid_b)
{
    if (ctx && (n < 16 || n > 65536 || (n & (n - 1)))) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_display_nfm_f64: n must be a power of two in [16, 65536]");
    if (ctx && h_grid_a && n_halo > 0) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_display_nfm_f64: grids need a fresh history (no halo)");
    return stream_display<double>(ctx, h_iq, PssIqFmt{}, n_frames, n, fs, chunk_frames, mode, window, disp_h, disp_w, h_halo_lo, h_halo_hi, n_halo, h_line_a,
                                  h_line_b, h_pcm, h_db, h_row_lo, h_row_hi, h_grid_a, h_grid_b);
}

extern "C" int pss_h_stream_display_nfm_grids(pss_ctx *ctx, const float *h_iq, long n_frames, int n, double fs, long chunk_frames,
                                              int mode, int window, int disp_h, int disp_w, int8_t *h_line_a, int8_t *h_line_b,
                                              int16_t *h_pcm, float *h_row_lo, float *h_row_hi, int8_t *h_grid_a, int8_t *h_grid_b)
{
    if (ctx && !h_grid_a) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_display_nfm_grids: h_grid_a is null");
    return stream_display<float>(ctx, h_iq, PssIqFmt{}, n_frames, n, fs, chunk_frames, mode, window, disp_h, disp_w, nullptr, nullptr, 0, h_line_a, h_line_b,
                                 h_pcm, nullptr, h_row_lo, h_row_hi, h_grid_a, h_grid_b);
}

// ... and on captures of ADC codes (include/pss.h "ADC codes"): the same template, the codes uploaded and unpacked chunk by chunk
extern "C" int pss_h_stream_display_nfm_codes(pss_ctx *ctx, int container, double scale, const float *h_table256, const void *h_codes,
                                              long n_frames, int n, double fs, long chunk_frames, int mode, int window, int disp_h, int disp_w,
                                              const float *h_halo_lo, const float *h_halo_hi, int n_halo, int8_t *h_line_a, int8_t *h_line_b,
                                              int16_t *h_pcm, float *h_db, float *h_row_lo, float *h_row_hi)
{
    return stream_display<float>(ctx, h_codes, PssIqFmt::of_codes(container, scale, h_table256), n_frames, n, fs, chunk_frames, mode, window, disp_h, disp_w,
                                 h_halo_lo, h_halo_hi, n_halo, h_line_a, h_line_b, h_pcm, h_db, h_row_lo, h_row_hi, nullptr, nullptr);
}

extern "C" int pss_h_stream_display_nfm_codes_f64(pss_ctx *ctx, int container, double scale, const float *h_table256, const void *h_codes,
                                                  long n_frames, int n, double fs, long chunk_frames, int mode, int window, int disp_h,
                                                  int disp_w, const double *h_halo_lo, const double *h_halo_hi, int n_halo, int8_t *h_line_a,
                                                  int8_t *h_line_b, int16_t *h_pcm, double *h_db, double *h_row_lo, double *h_row_hi,
                                                  int8_t *h_grid_a, int8_t *h_grid_b)
{
    if (ctx && (n < 16 || n > 65536 || (n & (n - 1)))) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_display_nfm_codes_f64: n must be a power of two in [16, 65536]");
    if (ctx && h_grid_a && n_halo > 0) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_display_nfm_codes_f64: grids need a fresh history (no halo)");
    return stream_display<double>(ctx, h_codes, PssIqFmt::of_codes(container, scale, h_table256), n_frames, n, fs, chunk_frames, mode, window, disp_h, disp_w,
                                  h_halo_lo, h_halo_hi, n_halo, h_line_a, h_line_b, h_pcm, h_db, h_row_lo, h_row_hi, h_grid_a, h_grid_b);
}

// ---- replaying a capture (include/pss.h): the main loop on a host recording — any mode, any view, dead reads skipped, squelch ------------
// stream_display's chunk loop around the RESIDENT step of the view (pss_frame_pipeline_cells / _squelch / _bars / _surface / _vector, the
// squelch composition for the views without a history), run on the chunk's live frames.  What differs from stream_display: results land at
// the running live / open counts (pss_live::Cursor), and a chunk may make the host wait (the live count, the gate's count) — so in that
// case the upload of chunk k + 1 is queued BEFORE chunk k's step, and the link works through the waits.
extern "C" int pss_h_stream_frames(pss_ctx *ctx, const pss_stream_req *req, pss_stream_res *res)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!req || !res || req->size != sizeof(pss_stream_req) || res->size != sizeof(pss_stream_res))
        return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: null request / result, or a struct size this library does not know");
    const int n = req->n, view = req->view, mode = req->mode, window = req->window, disp_h = req->disp_h, disp_w = req->disp_w, n_halo = req->n_halo;
    const long n_frames = req->n_frames;
    const bool gated = !(req->squelch != req->squelch), skip = req->skip_dead != 0, history = view <= 2;
    if (view < 0 || view > 5) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: unknown view (0 waterfall .. 5 vector)");
    if (mode < PSS_MODE_NFM || mode > PSS_MODE_WFM) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: unknown demodulation mode");
    PssIqFmt fmt;
    if (req->container != -1) {
        const int rf = pss_iq_check(ctx, req->container, req->scale, req->h_table256);
        if (rf) return rf;
        fmt = PssIqFmt::of_codes(req->container, req->scale, req->h_table256);
    }
    if (n < 16 || n > 65536 || (n & (n - 1))) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: n must be a power of two in [16, 65536]");
    if (n_frames < 0 || n_frames > INT32_MAX || req->chunk_frames < 1 || (n_frames > 0 && !req->h_in))
        return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: a frame count outside [0, 2^31), chunk_frames < 1 or a null capture");
    if (!history && (n_halo != 0 || req->h_halo_lo || req->h_halo_hi))
        return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: a halo belongs to the views with a history (0 - 2)");
    if (history && (n_halo < 0 || (n_halo > 0 && (!req->h_halo_lo || !req->h_halo_hi)) || window < 1 || disp_w < 1 || (view == 1 && (disp_h < 1 || disp_h > 127))))
        return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: bad halo, window or display geometry");
    if (view == 3 && (disp_h < 1 || disp_h > 127 || disp_w < 1)) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: spectrum bars need disp_h in [1, 127] and disp_w >= 1");
    if (view == 4 && disp_w < 2) return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: the surface view needs disp_w >= 2");
    const size_t mask_words = view == 5 && disp_w >= 1 ? ((size_t)disp_w + 31) / 32 : 0;
    if (view == 5 && (disp_h < 1 || disp_w < 1 || (size_t)disp_h * mask_words > 16384))
        return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: the vector view needs max_h >= 1, max_w >= 1 and max_h * ((max_w + 31) / 32) <= 16384 (the mask in LDS)");
    if (gated && (req->every < 0 || req->phase < 0 || (req->every == 0 ? req->phase != 0 : req->phase >= req->every)))
        return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: every < 0 or phase outside [0, every)");
    if (!gated && (res->peak || res->avg || res->open))
        return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: peak / avg / open come with a squelch (no meter runs without one)");
    const bool two_lines = view == 0 || view == 2;
    if ((history && (!res->line_a || (two_lines && !res->line_b))) || (view == 3 && (!res->height || !res->level)) || (view == 4 && !res->mag) ||
        (view == 5 && !res->mask))
        return pss_fail(ctx, PSS_E_ARG, "pss_h_stream_frames: an output the view requires is null");
    const int n_out = pss_demod_out_len_ctx(ctx, mode, n, req->fs);
    if (n_out < 0) return pss_fail(ctx, PSS_E_ARG, "sample rate below the target rate");
    pss_live::Cursor cur;
    cur.held = gated ? req->held_in : 0.0;
    cur.phase = gated ? req->phase : 0;
    auto finish = [&]() {
        res->n_live = cur.n_live, res->n_open = cur.n_open, res->held_out = gated ? cur.held : req->held_in, res->phase_out = gated ? cur.phase : req->phase;
    };
    if (n_frames == 0) {
        finish();
        return PSS_OK;
    }
    const long chunk = req->chunk_frames > n_frames ? n_frames : req->chunk_frames;
    const int m = n - 4;
    // per frame of a chunk: the view's two byte planes (lines / bars / magnitudes / mask), and a set of small numbers
    const size_t per_a = view == 5 ? (size_t)disp_h * mask_words * sizeof(uint32_t) : (size_t)disp_w, per_b = (two_lines || view == 3) ? (size_t)disp_w : 0;
    const size_t iq_b = (size_t)chunk * n * 2 * sizeof(float);
    const size_t num_b = (size_t)chunk * (4 * sizeof(double) + 2);   // [range 2 | peak | avg] float64, [open | live] bytes
    const size_t n_ext = (size_t)n_halo + (size_t)n_frames;
    PssStreaming &st = ctx->st;
    PSS_TRY(st.open(ctx));
    void *d_iq[2], *d_db[2], *d_pcm[2], *d_a[2], *d_b[2] = {nullptr, nullptr}, *d_num[2], *d_codes[2] = {nullptr, nullptr};
    void *d_post = nullptr, *d_ext = nullptr, *d_work = nullptr;
    for (int i = 0; i < 2; i++) {
        PSS_TRY(st.ensure(ctx, PssStreaming::IQ + i, iq_b, &d_iq[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::DB + i, (size_t)chunk * n * sizeof(float), &d_db[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::PCM + i, (size_t)chunk * n_out * 2 * sizeof(int16_t), &d_pcm[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::PLANE_A + i, (size_t)chunk * per_a, &d_a[i]));
        if (per_b) PSS_TRY(st.ensure(ctx, PssStreaming::PLANE_B + i, (size_t)chunk * per_b, &d_b[i]));
        if (fmt.codes) PSS_TRY(st.ensure(ctx, PssStreaming::CODES + i, (size_t)chunk * n * fmt.sample_bytes(), &d_codes[i]));
        PSS_TRY(st.ensure(ctx, PssStreaming::NUMBERS + i, num_b, &d_num[i]));
    }
    if (!history && gated) PSS_TRY(st.ensure(ctx, PssStreaming::POST, (size_t)chunk * m * sizeof(double), &d_post));
    if (history) PSS_TRY(st.ensure(ctx, PssStreaming::EXTREMES, 2 * n_ext * sizeof(double), &d_ext));
    // the chunk's live frames gathered in front of its step, and the two index lists (live frames, open frames)
    const size_t gather_b = skip ? iq_b : 0;
    PSS_TRY(st.ensure(ctx, PssStreaming::WORK, gather_b + 2 * (size_t)chunk * sizeof(int32_t), &d_work));
    float *d_gather = reinterpret_cast<float *>(d_work);
    int32_t *d_live_idx = reinterpret_cast<int32_t *>(static_cast<char *>(d_work) + gather_b), *d_open_idx = d_live_idx + chunk;
    ChunkLoop loop(ctx, n_frames, chunk, n, req->h_in, fmt, d_iq, d_codes);
    double *d_lo = reinterpret_cast<double *>(d_ext), *d_hi = history ? d_lo + n_ext : nullptr;
    if (n_halo) {
        PSS_HIP(ctx, hipMemcpyAsync(d_lo, req->h_halo_lo, sizeof(double) * n_halo, hipMemcpyHostToDevice, ctx->stream));
        PSS_HIP(ctx, hipMemcpyAsync(d_hi, req->h_halo_hi, sizeof(double) * n_halo, hipMemcpyHostToDevice, ctx->stream));
    }
    const bool waits = skip || gated;   // a chunk's step makes the host wait: the next upload is queued in front of it
    for (long k = 0; k < loop.n_chunks; k++) {
        const auto [b, f0, cnt] = loop.at(k);
        if (k == 0 || !waits) PSS_TRY(loop.upload(k));
        if (waits && k + 1 < loop.n_chunks) PSS_TRY(loop.upload(k + 1));
        PSS_TRY(loop.admit(k));
        double *d_range = reinterpret_cast<double *>(d_num[b]), *d_peak = d_range + 2 * chunk, *d_avg = d_peak + chunk;
        uint8_t *d_open = reinterpret_cast<uint8_t *>(d_avg + chunk), *d_live = d_open + chunk;
        long nl = cnt, no = 0;
        double held_next = cur.held;
        const float *src = (const float *)d_iq[b];
        if (skip) {
            PSS_TRY(pss_live_frames(ctx, src, cnt, n, d_live, d_live_idx, &nl));   // waits for the count
            if (nl > 0 && nl < cnt) {
                PSS_TRY(pss_gather_frames(ctx, src, cnt, n, d_live_idx, nl, d_gather));
                src = d_gather;
            }
        }
        if (nl > 0) {
            PssFlagScope keep(ctx->no_small_batch, true);   // chunks of a stream are throughput work: fused large-batch kernels
            if (history) {
                // live frames cur.n_live .. of the capture sit at positions n_halo + cur.n_live .. of the extremes arrays: the history reaches back
                // over the live frames before them and the caller's halo, and skips dead reads as the reference's deque does
                const long before = (long)n_halo + cur.n_live;
                const int halo_k = (int)(before < (long)(window - 1) ? before : (long)(window - 1));
                double *lo_k = d_lo + before - halo_k, *hi_k = d_hi + before - halo_k;
                if (gated)
                    PSS_TRY(pss_frame_pipeline_squelch(ctx, mode, src, nl, n, req->fs, (float *)d_db[b], nullptr, lo_k, hi_k, halo_k, window, view, disp_h, disp_w,
                                                       (int8_t *)d_a[b], (int8_t *)d_b[b], (int16_t *)d_pcm[b], req->squelch, req->every, cur.phase, cur.held,
                                                       d_peak, d_avg, d_open, &no, &held_next));
                else
                    PSS_TRY(pss_frame_pipeline_cells(ctx, mode, src, nl, n, req->fs, (float *)d_db[b], nullptr, lo_k, hi_k, halo_k, window, view, disp_h, disp_w,
                                                     (int8_t *)d_a[b], (int8_t *)d_b[b], (int16_t *)d_pcm[b]));
            } else {
                // the views without a history; with a squelch the display half alone, then meter -> gate -> demodulator on the open frames
                int16_t *pcm_now = gated ? nullptr : (int16_t *)d_pcm[b];
                double *post = gated ? (double *)d_post : nullptr;
                if (view == 3)
                    PSS_TRY(pss_frame_pipeline_bars(ctx, mode, src, nl, n, req->fs, (float *)d_db[b], nullptr, post, disp_h, disp_w, (int8_t *)d_a[b], (int8_t *)d_b[b],
                                                    d_range, pcm_now));
                else if (view == 4)
                    PSS_TRY(pss_frame_pipeline_surface(ctx, mode, src, nl, n, req->fs, (float *)d_db[b], nullptr, post, disp_w, (int8_t *)d_a[b], d_range, pcm_now));
                else
                    PSS_TRY(pss_frame_pipeline_vector(ctx, mode, src, nl, n, req->fs, (float *)d_db[b], nullptr, post, disp_h, disp_w, (uint32_t *)d_a[b], pcm_now));
                if (gated) {
                    PSS_TRY(pss_row_meter_f64(ctx, post, nl, m, d_peak, d_avg));
                    PSS_TRY(pss_squelch_gate(ctx, d_peak, nl, req->squelch, req->every, cur.phase, cur.held, d_open, d_open_idx, &no, &held_next));
                    PSS_TRY(pss_demod_gated(ctx, mode, src, nl, n, req->fs, d_open_idx, no, (int16_t *)d_pcm[b], nullptr));
                }
            }
            if (!gated) no = nl;
        }
        PSS_TRY(loop.computed(k));
        // the live mask lands at the chunk's frames, everything else at the running live count, the PCM at the running open count
        if (skip) PSS_TRY(loop.down(res->live, f0, d_live, cnt, 1));
        const long at = cur.n_live;
        PSS_TRY(loop.down(res->db32, at, d_db[b], nl, (size_t)n * sizeof(float)));
        if (history) {
            PSS_TRY(loop.down(res->line_a, at, d_a[b], nl, per_a));
            if (two_lines) PSS_TRY(loop.down(res->line_b, at, d_b[b], nl, per_b));
        } else if (view == 3) {
            PSS_TRY(loop.down(res->height, at, d_a[b], nl, per_a));
            PSS_TRY(loop.down(res->level, at, d_b[b], nl, per_b));
        } else if (view == 4) {
            PSS_TRY(loop.down(res->mag, at, d_a[b], nl, per_a));
        } else {
            PSS_TRY(loop.down(res->mask, at, d_a[b], nl, per_a));
        }
        if (view == 3 || view == 4) PSS_TRY(loop.down(res->range, at, d_range, nl, 2 * sizeof(double)));
        if (gated) {
            PSS_TRY(loop.down(res->peak, at, d_peak, nl, sizeof(double)));
            PSS_TRY(loop.down(res->avg, at, d_avg, nl, sizeof(double)));
            PSS_TRY(loop.down(res->open, at, d_open, nl, 1));
        }
        PSS_TRY(loop.down(res->pcm, cur.n_open, d_pcm[b], no, (size_t)n_out * 2 * sizeof(int16_t)));
        PSS_TRY(loop.downloaded(k));
        cur.advance(nl, no, held_next, gated ? req->every : 0);
    }
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (history && cur.n_live > 0) {
        if (res->row_lo) PSS_HIP(ctx, hipMemcpy(res->row_lo, d_lo + n_halo, sizeof(double) * cur.n_live, hipMemcpyDeviceToHost));
        if (res->row_hi) PSS_HIP(ctx, hipMemcpy(res->row_hi, d_hi + n_halo, sizeof(double) * cur.n_live, hipMemcpyDeviceToHost));
    }
    loop.drain();   // what the host writes itself comes behind every copy
    if (!skip && res->live) memset(res->live, 1, (size_t)n_frames);   // every frame counts as live
    finish();
    return PSS_OK;
}

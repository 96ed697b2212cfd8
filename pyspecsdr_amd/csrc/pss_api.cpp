// pss_api.cpp — context management and the single-buffer host convenience calls of the C ABI (include/pss.h); the streamed captures
// are pss_stream.cpp.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pss_ctx.h"

static std::string g_create_err;

int pss_fail(pss_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    else g_create_err = msg;
    return code;
}

int pss_ptrs_aligned(pss_ctx *ctx, const char *entry, std::initializer_list<PssPtr> ptrs)
{
    for (const PssPtr &a : ptrs)
        if (reinterpret_cast<uintptr_t>(a.p) & (a.align - 1))
            return pss_fail(ctx, PSS_E_ARG, std::string(entry) + ": " + a.name + " must be " + std::to_string(a.align) + "-byte aligned");
    return PSS_OK;
}

int pss_hip_check(pss_ctx *ctx, hipError_t e, const char *what)
{
    if (e == hipSuccess) return PSS_OK;
    return pss_fail(ctx, PSS_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int pss_ensure_buffer(pss_ctx *ctx, void **buf, size_t *cap, size_t bytes, const char *what)
{
    if (bytes <= *cap) return PSS_OK;
    if (*buf) {
        // the old buffer may still be in use by work queued on either stream
        hipStreamSynchronize(ctx->stream);
        if (ctx->stream2) hipStreamSynchronize(ctx->stream2);
        hipFree(*buf);
        *buf = nullptr;
        *cap = 0;
    }
    hipError_t e = hipMalloc(buf, bytes);
    if (e != hipSuccess) return pss_fail(ctx, PSS_E_NOMEM, std::string(what) + " hipMalloc: " + hipGetErrorString(e));
    *cap = bytes;
    return PSS_OK;
}

int pss_table_sync(pss_ctx *ctx, PssDevTable *t, const void *img, size_t bytes, const char *what, size_t capacity)
{
    if (t->host.size() == bytes && memcmp(t->host.data(), img, bytes) == 0) return PSS_OK;
    t->host.clear();   // first: pss_ensure_buffer may free the buffer the mirror describes, and every step below may fail
    int r = pss_ensure_buffer(ctx, &t->dev, &t->cap, capacity > bytes ? capacity : bytes, what);
    if (r) return r;
    PSS_HIP(ctx, hipMemcpyAsync(t->dev, img, bytes, hipMemcpyHostToDevice, PSS_STREAM(ctx)));
    PSS_HIP(ctx, hipStreamSynchronize(PSS_STREAM(ctx)));   // img may be a local; the upload is ordered behind earlier launches reading the old tables
    const unsigned char *b = static_cast<const unsigned char *>(img);
    t->host.assign(b, b + bytes);
    return PSS_OK;
}

int pss_ensure_scratch(pss_ctx *ctx, size_t bytes)
{
    return pss_ensure_buffer(ctx, &ctx->scratch, &ctx->scratch_bytes, bytes, "scratch");
}

void pss_time_begin(pss_ctx *ctx)
{
    if (ctx->timing && ctx->tdepth++ == 0 && ctx->tfilter.empty()) hipEventRecord(ctx->ev0, ctx->stream);
}
void pss_kernel_begin(pss_ctx *ctx, const char *name)
{
    if (!ctx->timing) return;
    ctx->kskip = !ctx->tfilter.empty() && ctx->tfilter != name;
    if (ctx->kskip) return;
    if (ctx->kused == (int)ctx->krecs.size()) {
        pss_ctx::KRec r{name, nullptr, nullptr};
        hipEventCreate(&r.e0);
        hipEventCreate(&r.e1);
        ctx->krecs.push_back(r);
    }
    ctx->krecs[ctx->kused].name = name;
    hipEventRecord(ctx->krecs[ctx->kused].e0, PSS_STREAM(ctx));
}
void pss_kernel_end(pss_ctx *ctx)
{
    if (!ctx->timing || ctx->kskip) return;
    hipEventRecord(ctx->krecs[ctx->kused].e1, PSS_STREAM(ctx));
    ctx->kused++;
}
void pss_time_end(pss_ctx *ctx)
{
    if (ctx->timing && --ctx->tdepth == 0) {
        if (ctx->tfilter.empty()) hipEventRecord(ctx->ev1, ctx->stream);
        ctx->last_ms = 0.0f;
    }
}

int pss_side_mark(pss_ctx *ctx) { PSS_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream)); return PSS_OK; }
int pss_side_wait(pss_ctx *ctx) { return pss_hip_check(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0), "hipStreamWaitEvent(fork)"); }
int pss_side_fork(pss_ctx *ctx)
{
    const int r = pss_hip_check(ctx, hipEventRecord(ctx->ev_fork, ctx->stream), "hipEventRecord(fork)");
    return r ? r : pss_side_wait(ctx);
}
int pss_side_join(pss_ctx *ctx)
{
    const int r = pss_hip_check(ctx, hipEventRecord(ctx->ev_join, ctx->stream2), "hipEventRecord(join)");
    return r ? r : pss_hip_check(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0), "hipStreamWaitEvent(join)");
}

extern "C" int pss_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int pss_create(int device, pss_ctx **out)
{
    if (!out) return PSS_E_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return pss_fail(nullptr, PSS_E_HIP, std::string("no HIP device available (libpss has no CPU fallback): ") +
                                                (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device < 0 || device >= n) return pss_fail(nullptr, PSS_E_ARG, "device index out of range");
    int prev = -1;
    hipGetDevice(&prev);
    e = hipSetDevice(device);
    if (e != hipSuccess) return pss_fail(nullptr, PSS_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    struct Restore {  // the caller's current device is left as it was
        int prev, dev;
        ~Restore() { if (prev >= 0 && prev != dev) hipSetDevice(prev); }
    } restore{prev, device};
    pss_ctx *ctx = new pss_ctx();
    ctx->device = device;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) ctx->n_cus = cus; }
    { const char *e = getenv("PSS_NO_FUSED"); ctx->no_fused = e && e[0] == '1'; }
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) ctx->own_stream = true;
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) {
        const std::string msg = std::string("context stream / event creation: ") + hipGetErrorString(e);
        if (ctx->ev0) hipEventDestroy(ctx->ev0);
        if (ctx->ev1) hipEventDestroy(ctx->ev1);
        if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
        if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
        if (ctx->stream2) hipStreamDestroy(ctx->stream2);
        if (ctx->own_stream) hipStreamDestroy(ctx->stream);
        delete ctx;
        return pss_fail(nullptr, PSS_E_HIP, msg);
    }
    *out = ctx;
    return PSS_OK;
}

extern "C" void pss_destroy(pss_ctx *ctx)
{
    if (!ctx) return;
    PssDevGuard guard(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (ctx->comm) pss_comm_free(ctx);
    for (auto &kv : ctx->tw) hipFree(kv.second);
    for (auto &kv : ctx->tw_pf) hipFree(kv.second);
    for (auto &kv : ctx->win) hipFree(kv.second);
    for (auto &kv : ctx->bs) { hipFree(kv.second.d_chirp); hipFree(kv.second.d_B); hipFree(kv.second.d_win); }
    for (auto &kv : ctx->plans) {
        hipFree(kv.second.d_tab);
    }
    for (auto &kv : ctx->nfm) if (kv.second.d_rev) hipFree(kv.second.d_rev);
    if (ctx->scratch) hipFree(ctx->scratch);
    if (ctx->scratch_fft) hipFree(ctx->scratch_fft);
    if (ctx->scratch_hil) hipFree(ctx->scratch_hil);
    if (ctx->scratch_iqc) hipFree(ctx->scratch_iqc);
    if (ctx->d_hann) hipFree(ctx->d_hann);
    if (ctx->d_hann_short) hipFree(ctx->d_hann_short);
    ctx->st.release();
    if (ctx->scratch_scan) hipFree(ctx->scratch_scan);
    if (ctx->scratch_pk) hipFree(ctx->scratch_pk);
    if (ctx->scratch_win) hipFree(ctx->scratch_win);
    if (ctx->scratch_db64) hipFree(ctx->scratch_db64);
    if (ctx->scratch_post) hipFree(ctx->scratch_post);
    if (ctx->prog) hipFree(ctx->prog);
    if (ctx->stage) hipFree(ctx->stage);
    for (auto &b : ctx->sq_buf) if (b) hipFree(b);
    if (ctx->sq_pin) hipHostFree(ctx->sq_pin);
    for (PssDevTable *t : {&ctx->ddc_tab, &ctx->pfb_tab, &ctx->bank_tab, &ctx->rs_tab, &ctx->welch_win, &ctx->rds_tab, &ctx->rds_pulse, &ctx->ais_pulse, &ctx->apt_tab, &ctx->packet_tones}) t->release();
    if (ctx->welch_part) hipFree(ctx->welch_part);
    for (auto &b : ctx->starts.buf) if (b) hipFree(b);
    if (ctx->starts.pin) hipHostFree(ctx->starts.pin);
    if (ctx->ook_first) hipFree(ctx->ook_first);
    hipEventDestroy(ctx->ev0);
    hipEventDestroy(ctx->ev1);
    hipStreamSynchronize(ctx->stream2);
    hipStreamDestroy(ctx->stream2);
    hipEventDestroy(ctx->ev_fork);
    hipEventDestroy(ctx->ev_join);
    if (ctx->ev_in) hipEventDestroy(ctx->ev_in);
    if (ctx->ev_out) hipEventDestroy(ctx->ev_out);
    for (auto &k : ctx->krecs) { hipEventDestroy(k.e0); hipEventDestroy(k.e1); }
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int pss_set_stream(pss_ctx *ctx, void *hip_stream)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    hipStreamSynchronize(ctx->stream);
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    ctx->own_stream = false;
    return PSS_OK;
}

// Ordering against a caller's stream without giving up the context's own (non-blocking) stream: one event record + one stream wait each,
// nothing blocks the host.
extern "C" int pss_order_after(pss_ctx *ctx, void *hip_stream)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (s == ctx->stream) return PSS_OK;
    if (!ctx->ev_in) PSS_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming));
    PSS_HIP(ctx, hipEventRecord(ctx->ev_in, s));
    PSS_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
    return PSS_OK;
}

extern "C" int pss_order_before(pss_ctx *ctx, void *hip_stream)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (s == ctx->stream) return PSS_OK;
    if (!ctx->ev_out) PSS_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_out, hipEventDisableTiming));
    PSS_HIP(ctx, hipEventRecord(ctx->ev_out, ctx->stream));
    PSS_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_out, 0));
    return PSS_OK;
}

extern "C" void *pss_get_stream(pss_ctx *ctx) { return ctx ? reinterpret_cast<void *>(ctx->stream) : nullptr; }

extern "C" int pss_set_option(pss_ctx *ctx, const char *key, int value)
{
    if (!ctx || !key) return PSS_E_ARG;
    if (!strcmp(key, "nfm_fused")) { ctx->no_fused = (value == 0); return PSS_OK; }
    if (!strcmp(key, "wfm_fused")) { ctx->no_wfm_fused = (value == 0); return PSS_OK; }
    if (!strcmp(key, "small_batch")) { ctx->no_small_batch = (value == 0); return PSS_OK; }
    if (!strcmp(key, "small_batch_max")) { ctx->small_batch_max = value; return PSS_OK; }
    if (!strcmp(key, "wfm_small_batch_max")) { ctx->wfm_small_batch_max = value; return PSS_OK; }
    if (!strcmp(key, "fuse_post")) { ctx->fuse_post = value != 0; return PSS_OK; }
    if (!strcmp(key, "post_split")) { ctx->post_split = value < 0 ? -1 : value; return PSS_OK; }
    if (!strcmp(key, "ssb_rfft")) { ctx->ssb_rfft = value != 0; return PSS_OK; }
    if (!strcmp(key, "ssb_hilbert")) { ctx->ssb_hilbert = value != 0; return PSS_OK; }
    if (!strcmp(key, "hilbert_exact")) { ctx->hilbert_exact = value != 0; return PSS_OK; }
    if (!strcmp(key, "scan_exact")) { ctx->scan_exact = value != 0; return PSS_OK; }
    if (!strcmp(key, "db_exact")) { ctx->db_exact = value != 0; return PSS_OK; }
    if (!strcmp(key, "f64_plain")) { ctx->f64_plain = value != 0; return PSS_OK; }
    if (!strcmp(key, "wfm_corr_copy")) { ctx->wfm_corr_copy = value != 0; return PSS_OK; }
    return pss_fail(ctx, PSS_E_ARG, std::string("unknown option: ") + key);
}

extern "C" int pss_sync(pss_ctx *ctx)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    return pss_hip_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

extern "C" const char *pss_last_error(pss_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

extern "C" int pss_enable_timing(pss_ctx *ctx, int on)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    ctx->timing = on != 0;
    ctx->tdepth = 0;
    ctx->kused = 0;
    ctx->last_ms = -1.0f;
    return PSS_OK;
}

extern "C" int pss_timing_filter(pss_ctx *ctx, const char *kernel)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    ctx->tfilter = kernel ? kernel : "";
    ctx->kused = 0;
    ctx->last_ms = -1.0f;
    return PSS_OK;
}

extern "C" float pss_last_kernel_ms(pss_ctx *ctx)
{
    if (!ctx || !ctx->timing || ctx->last_ms < 0.0f || !ctx->tfilter.empty()) return -1.0f;
    PSS_GUARD(ctx);
    if (hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) != hipSuccess) return -1.0f;
    return ms;
}

extern "C" int pss_kernel_times(pss_ctx *ctx, char *buf, int buf_len)
{
    // "name=ms;name=ms;..." for every kernel launched since timing was enabled / since the previous read
    if (!ctx || !buf || buf_len < 1) return PSS_E_ARG;
    PSS_GUARD(ctx);
    std::string out;
    if (ctx->timing && ctx->last_ms >= 0.0f) {
        if (ctx->tfilter.empty()) hipEventSynchronize(ctx->ev1);
        else hipStreamSynchronize(ctx->stream);
        for (int i = 0; i < ctx->kused; i++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ctx->krecs[i].e0, ctx->krecs[i].e1) != hipSuccess) continue;
            out += ctx->krecs[i].name;
            out += "=" + std::to_string(ms) + ";";
        }
    }
    ctx->kused = 0;
    if ((int)out.size() + 1 > buf_len) return pss_fail(ctx, PSS_E_ARG, "buffer too small");
    memcpy(buf, out.c_str(), out.size() + 1);
    return PSS_OK;
}

// ---- host-buffer convenience: one frame, synchronous ------------------------------------------------
// Device staging comes from one grow-only buffer owned by the context (no hipMalloc per call: this is the path the
// drop-in module takes on every loop iteration of the host application).
namespace {
size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

extern "C" int pss_h_compute_fft(pss_ctx *ctx, const float *h_iq, int n, double *h_db)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || !h_db || n < 1) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_db = up256(sizeof(float) * 2 * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_db + up256(sizeof(float) * n), "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(float) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_spectrum_db(ctx, reinterpret_cast<const float *>(base), 1, n, reinterpret_cast<float *>(base + o_db));
    if (r) return r;
    std::vector<float> tmp(n);
    PSS_HIP(ctx, hipMemcpyAsync(tmp.data(), base + o_db, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; i++) h_db[i] = (double)tmp[i];
    return PSS_OK;
}

// complex128 read buffers (the reference computes these two functions in float64 then; tests/golden/c128.npz)
extern "C" int pss_h_compute_fft_c128(pss_ctx *ctx, const double *h_iq, int n, double *h_db)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || !h_db || n < 1) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_db = up256(sizeof(double) * 2 * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_db + up256(sizeof(double) * n), "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(double) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_spectrum_db_c128(ctx, reinterpret_cast<const double *>(base), 1, n, reinterpret_cast<double *>(base + o_db));
    if (r) return r;
    PSS_HIP(ctx, hipMemcpyAsync(h_db, base + o_db, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSS_OK;
}

extern "C" int pss_h_demodulate_am_c128(pss_ctx *ctx, const double *h_iq, int n, double *h_audio_stereo, int16_t *h_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || n < 1 || (!h_audio_stereo && !h_pcm)) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_pcm = up256(sizeof(double) * 2 * n), o_au = o_pcm + up256(sizeof(int16_t) * 2 * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_au + up256(sizeof(double) * n), "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(double) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_demod_am_c128(ctx, reinterpret_cast<const double *>(base), 1, n, reinterpret_cast<int16_t *>(base + o_pcm), reinterpret_cast<double *>(base + o_au));
    if (r) return r;
    std::vector<double> au(n);
    PSS_HIP(ctx, hipMemcpyAsync(au.data(), base + o_au, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (h_pcm) PSS_HIP(ctx, hipMemcpyAsync(h_pcm, base + o_pcm, sizeof(int16_t) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_audio_stereo)
        for (int i = 0; i < n; i++) h_audio_stereo[2 * i] = h_audio_stereo[2 * i + 1] = au[i];   // mono_to_stereo (:83-88)
    return PSS_OK;
}

extern "C" int pss_h_demodulate_ssb_c128(pss_ctx *ctx, int lower, const double *h_iq, int n, double fs, double *h_audio_stereo, int16_t *h_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || n < 1 || (!h_audio_stereo && !h_pcm)) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_pcm = up256(sizeof(double) * 2 * n), o_au = o_pcm + up256(sizeof(int16_t) * 2 * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_au + up256(sizeof(double) * n), "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(double) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_demod_ssb_c128(ctx, lower, reinterpret_cast<const double *>(base), 1, n, fs, reinterpret_cast<int16_t *>(base + o_pcm), reinterpret_cast<double *>(base + o_au));
    if (r) return r;
    std::vector<double> au(n);
    PSS_HIP(ctx, hipMemcpyAsync(au.data(), base + o_au, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (h_pcm) PSS_HIP(ctx, hipMemcpyAsync(h_pcm, base + o_pcm, sizeof(int16_t) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_audio_stereo)
        for (int i = 0; i < n; i++) h_audio_stereo[2 * i] = h_audio_stereo[2 * i + 1] = au[i];   // mono_to_stereo (:83-88)
    return PSS_OK;
}

extern "C" int pss_h_mean_power_c128(pss_ctx *ctx, const double *h_iq, int n, double *h_power)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || !h_power || n < 1) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_p = up256(sizeof(double) * 2 * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_p + 256, "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(double) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_mean_power_c128(ctx, reinterpret_cast<const double *>(base), 1, n, reinterpret_cast<double *>(base + o_p));
    if (r) return r;
    PSS_HIP(ctx, hipMemcpyAsync(h_power, base + o_p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSS_OK;
}

static int h_demod_impl(pss_ctx *ctx, int mode, const float *h_iq, int n, double fs, double *h_audio_stereo,
                        int16_t *h_pcm, bool dispatcher)
{
    if (!ctx) return PSS_E_ARG;
    if (!h_iq || n < 1 || (!h_audio_stereo && !h_pcm)) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    int n_out = pss_demod_out_len_ctx(ctx, mode, n, fs);
    if (n_out < 0) return pss_fail(ctx, PSS_E_ARG, "unknown mode or sample rate below the target rate");
    const bool stereo = mode == PSS_MODE_WFM;
    const size_t o_pcm = up256(sizeof(float) * 2 * n), o_au = o_pcm + up256(sizeof(int16_t) * 2 * n_out);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_au + up256(sizeof(double) * 2 * n_out), "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(float) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = (dispatcher ? pss_demod_signal : pss_demod)(ctx, mode, reinterpret_cast<const float *>(base), 1, n, fs,
                                                    reinterpret_cast<int16_t *>(base + o_pcm),
                                                    reinterpret_cast<double *>(base + o_au));
    if (r) return r;
    std::vector<double> au((size_t)n_out * (stereo ? 2 : 1));
    PSS_HIP(ctx, hipMemcpyAsync(au.data(), base + o_au, sizeof(double) * au.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (h_pcm) PSS_HIP(ctx, hipMemcpyAsync(h_pcm, base + o_pcm, sizeof(int16_t) * 2 * n_out, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_audio_stereo) {
        if (stereo) memcpy(h_audio_stereo, au.data(), sizeof(double) * au.size());  // np.column_stack((left, right))
        else
            for (int i = 0; i < n_out; i++) h_audio_stereo[2 * i] = h_audio_stereo[2 * i + 1] = au[i];  // mono_to_stereo
    }
    return PSS_OK;
}

extern "C" int pss_h_demodulate(pss_ctx *ctx, int mode, const float *h_iq, int n, double fs, double *h_audio_stereo,
                                int16_t *h_pcm)
{
    return h_demod_impl(ctx, mode, h_iq, n, fs, h_audio_stereo, h_pcm, false);
}

extern "C" int pss_h_demodulate_signal(pss_ctx *ctx, int mode, const float *h_iq, int n, double fs,
                                       double *h_audio_stereo, int16_t *h_pcm)
{
    return h_demod_impl(ctx, mode, h_iq, n, fs, h_audio_stereo, h_pcm, true);
}

// demodulate_signal over a batch of frames in HOST memory (a recording cut into read buffers, pyspecsdr.py:814-824 /
// :2236): chunks of frames go up, through pss_demod_signal, and the int16 PCM comes back — the byte stream
// audio_processing.write_audio_samples / io_manager.write_to_pipe would have produced buffer by buffer.
// fmt: the recording's sample format; ADC codes are uploaded as they are and unpacked in front of the demodulator (pss_ingest.hip)
static int h_demod_batch_impl(pss_ctx *ctx, int mode, const void *h_in, const PssIqFmt &fmt, long n_frames, int n, double fs,
                              long chunk_frames, int16_t *h_pcm)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (fmt.codes) {
        const int rf = pss_iq_check(ctx, fmt.container, fmt.scale, fmt.h_table256);
        if (rf) return rf;
    }
    if (!h_in || !h_pcm || n_frames < 0 || n < 1 || chunk_frames < 1) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const char *h_bytes = static_cast<const char *>(h_in);
    const size_t sample_b = fmt.sample_bytes();
    const int n_out = pss_demod_out_len_ctx(ctx, mode, n, fs);
    if (n_out < 0) return pss_fail(ctx, PSS_E_ARG, "unknown mode or sample rate below the target rate");
    if (chunk_frames > n_frames) chunk_frames = n_frames;
    if (n_frames == 0) return PSS_OK;
    const size_t iq_b = up256((size_t)chunk_frames * n * 2 * sizeof(float));
    const size_t pcm_b = up256((size_t)chunk_frames * n_out * 2 * sizeof(int16_t));
    const size_t codes_b = fmt.codes ? up256((size_t)chunk_frames * n * sample_b) : 0;
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, iq_b + pcm_b + codes_b, "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    char *d_in = fmt.codes ? base + iq_b + pcm_b : base;
    for (long f0 = 0; f0 < n_frames; f0 += chunk_frames) {
        const long cnt = (n_frames - f0) < chunk_frames ? (n_frames - f0) : chunk_frames;
        PSS_HIP(ctx, hipMemcpyAsync(d_in, h_bytes + (size_t)f0 * n * sample_b, (size_t)cnt * n * sample_b, hipMemcpyHostToDevice, ctx->stream));
        if (fmt.codes) {
            r = pss_unpack_iq(ctx, fmt.container, d_in, cnt * (long)n, fmt.scale, fmt.h_table256, reinterpret_cast<float *>(base));
            if (r) return r;
        }
        r = pss_demod_signal(ctx, mode, reinterpret_cast<const float *>(base), cnt, n, fs, reinterpret_cast<int16_t *>(base + iq_b),
                             nullptr);
        if (r) return r;
        PSS_HIP(ctx, hipMemcpyAsync(h_pcm + (size_t)f0 * n_out * 2, base + iq_b, (size_t)cnt * n_out * 2 * sizeof(int16_t),
                                    hipMemcpyDeviceToHost, ctx->stream));
        PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PSS_OK;
}

extern "C" int pss_h_demodulate_batch(pss_ctx *ctx, int mode, const float *h_iq, long n_frames, int n, double fs,
                                      long chunk_frames, int16_t *h_pcm)
{
    return h_demod_batch_impl(ctx, mode, h_iq, PssIqFmt{}, n_frames, n, fs, chunk_frames, h_pcm);
}

extern "C" int pss_h_demodulate_batch_codes(pss_ctx *ctx, int container, double scale, const float *h_table256, int mode, const void *h_codes,
                                            long n_frames, int n, double fs, long chunk_frames, int16_t *h_pcm)
{
    return h_demod_batch_impl(ctx, mode, h_codes, PssIqFmt::of_codes(container, scale, h_table256), n_frames, n, fs, chunk_frames, h_pcm);
}

extern "C" int pss_h_measure_power(pss_ctx *ctx, const float *h_iq, int n, float *h_power)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || !h_power || n < 1) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_p = up256(sizeof(float) * 2 * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_p + 256, "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(float) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_power_db(ctx, reinterpret_cast<const float *>(base), 1, n, reinterpret_cast<float *>(base + o_p));
    if (r) return r;
    PSS_HIP(ctx, hipMemcpyAsync(h_power, base + o_p, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSS_OK;
}

extern "C" int pss_h_morse_edges(pss_ctx *ctx, const float *h_iq, int n, double threshold_db, int cap, int32_t *h_rise,
                                 int32_t *h_fall, int *n_rise, int *n_fall)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || n < 1 || cap < 0 || (cap > 0 && (!h_rise || !h_fall))) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_r = up256(sizeof(float) * 2 * n), o_f = o_r + up256(sizeof(int32_t) * (size_t)cap), o_c = o_f + up256(sizeof(int32_t) * (size_t)cap);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_c + 256, "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(float) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_morse_edges(ctx, reinterpret_cast<const float *>(base), 1, n, threshold_db, cap, reinterpret_cast<int32_t *>(base + o_r),
                        reinterpret_cast<int32_t *>(base + o_f), reinterpret_cast<int32_t *>(base + o_c));
    if (r) return r;
    int32_t cnt[2];
    PSS_HIP(ctx, hipMemcpyAsync(cnt, base + o_c, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int kr = cnt[0] < cap ? cnt[0] : cap, kf = cnt[1] < cap ? cnt[1] : cap;
    if (kr) PSS_HIP(ctx, hipMemcpyAsync(h_rise, base + o_r, sizeof(int32_t) * kr, hipMemcpyDeviceToHost, ctx->stream));
    if (kf) PSS_HIP(ctx, hipMemcpyAsync(h_fall, base + o_f, sizeof(int32_t) * kf, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_rise) *n_rise = cnt[0];
    if (n_fall) *n_fall = cnt[1];
    return PSS_OK;
}

extern "C" int pss_h_classify_signal(pss_ctx *ctx, const float *h_iq, int n, double fs, int *label, double *bw, float *mi, float *flat)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || n < 1) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_out = up256(sizeof(float) * 2 * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_out + 256, "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(float) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    // results: [bw f64][label i32][mi f32][flat f32]
    double *d_bw = reinterpret_cast<double *>(base + o_out);
    int32_t *d_lab = reinterpret_cast<int32_t *>(base + o_out + 8);
    float *d_mi = reinterpret_cast<float *>(base + o_out + 12), *d_fl = reinterpret_cast<float *>(base + o_out + 16);
    r = pss_classify(ctx, reinterpret_cast<const float *>(base), 1, n, fs, d_lab, d_bw, d_mi, d_fl, nullptr);
    if (r) return r;
    unsigned char res[24];
    PSS_HIP(ctx, hipMemcpyAsync(res, base + o_out, sizeof res, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bw) memcpy(bw, res, 8);
    int32_t lab;
    memcpy(&lab, res + 8, 4);
    if (label) *label = lab;
    if (mi) memcpy(mi, res + 12, 4);
    if (flat) memcpy(flat, res + 16, 4);
    return PSS_OK;
}

extern "C" int pss_h_iq_correction(pss_ctx *ctx, const float *h_iq, int n, float *h_out_iq, float *h_raw)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_iq || (!h_out_iq && !h_raw) || n < 1) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    const size_t o_c = up256(sizeof(float) * 2 * n), o_r = o_c + up256(sizeof(float) * 2 * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, o_r + up256(sizeof(float) * n), "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_iq, sizeof(float) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_iq_correction(ctx, reinterpret_cast<const float *>(base), 1, n,
                          h_out_iq ? reinterpret_cast<float *>(base + o_c) : nullptr,
                          h_raw ? reinterpret_cast<float *>(base + o_r) : nullptr);
    if (r) return r;
    if (h_out_iq) PSS_HIP(ctx, hipMemcpyAsync(h_out_iq, base + o_c, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (h_raw) PSS_HIP(ctx, hipMemcpyAsync(h_raw, base + o_r, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSS_OK;
}

// bandpass_filter(data, lowcut, highcut, sample_rate) (signal_processing.py:34-42) on one host row of float64 samples.
// sos: caller-supplied table (nsec rows) or NULL to design butter(5, ...) natively.
extern "C" int pss_h_bandpass_filter(pss_ctx *ctx, const double *h_x, int n, double lowcut, double highcut, double fs,
                                     const double *sos, int nsec, double *h_y)
{
    if (!ctx) return PSS_E_ARG;
    PSS_GUARD(ctx);
    if (!h_x || !h_y || n < 0) return pss_fail(ctx, PSS_E_ARG, "bad arguments");
    double tbl[48];
    if (!sos) {
        int r = pss_design_butter_sos(5, lowcut <= 0 ? 0.0 : lowcut / (fs / 2.0), highcut / (fs / 2.0), tbl, &nsec);
        if (r) return pss_fail(ctx, r, "butter: digital filter critical frequencies must be 0 < Wn < 1");
        sos = tbl;
    }
    if (n == 0) return PSS_OK;
    const size_t o_y = up256(sizeof(double) * n);
    int r = pss_ensure_buffer(ctx, &ctx->stage, &ctx->stage_bytes, 2 * o_y, "staging");
    if (r) return r;
    char *base = reinterpret_cast<char *>(ctx->stage);
    PSS_HIP(ctx, hipMemcpyAsync(base, h_x, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    r = pss_sosfilt(ctx, reinterpret_cast<const double *>(base), 1, n, sos, nsec, reinterpret_cast<double *>(base + o_y));
    if (r) return r;
    PSS_HIP(ctx, hipMemcpyAsync(h_y, base + o_y, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    PSS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSS_OK;
}

// pss_ctx.h — the context object behind the C ABI (include/pss.h): device, stream, cached tables, scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/pss.h"
#include "pss_starts.h"

struct PssNfmFilt {
    double taps[65];
    double sos[24];
    double zi[8];
    double *d_rev = nullptr;   // device copy of the reversed taps (rev[j] = taps[64 - j], 65 doubles + 15 zeros): the fused NFM kernel's
                               // hand-scheduled FIR fetches its taps from here with scalar loads; made on first use, owned by the context
};

struct PssWfmFilt {
    double lp[18], pilot[30], lmr[30];  // butter(5) SOS rows: low-pass 15 kHz, pilot band-pass, L-R band-pass
    double alpha;                       // de-emphasis pole exp(-1/(75e-6 fs))
};

struct PssPairwisePlan {  // numpy pairwise-sum forest of one group length (pss_npsum.h: Forest; uploaded by get_plan of pss_demod.hip)
    int n_leaves = 0, n_nodes = 0, n_levels = 0, n_roots = 0;
    int wave_tree = 0;  // Forest::wave_tree: one wavefront can fold it with xor shuffles
    int *d_tab = nullptr;  // ONE device allocation: leaf_off, leaf_len, node_l, node_r, level_start, roots back to back (PlanDev points into it)
};

// The device copy of a call's host tables, grow-only, and the host bytes it mirrors: a call with the same tables as the last one uploads
// nothing (pss_table_sync below keeps the two in step)
struct PssDevTable {
    void *dev = nullptr;
    size_t cap = 0;
    std::vector<unsigned char> host;
    void release()
    {
        if (dev) hipFree(dev);
        dev = nullptr, cap = 0;
        host.clear();
    }
};

// What the streamed entry points (pss_h_stream_*, pss_stream.cpp) keep across calls: the two copy streams, the events of the two buffer
// sets and the device buffers, created on first use and grow-only (creating and freeing them per capture cost ~2 ms of a 17 ms capture).
// The three calls use the same slots for the same roles, so a context that alternates between them holds one set of chunk buffers.
struct PssStreaming {
    enum Slot {         // a pair is two slots, one per buffer set: ensure(ctx, SLOT + b, ...)
        IQ = 0,         // the chunk's samples as complex64 (pair)
        DB = 2,         // its dB rows (pair)
        PCM = 4,        // its int16 PCM (pair)
        PLANE_A = 6,    // the view's first byte plane per frame: glyphs / row indices, bar heights, magnitudes, the mask (pair)
        PLANE_B = 8,    // the second: colours, bar levels (pair)
        POST = 10,      // the post-processed rows of the chunk in flight
        EXTREMES = 11,  // [lo | hi] x (halo + frames): the row extremes of the whole capture
        GRID_A = 12,    // the full screen after a chunk, first plane (pair)
        GRID_B = 14,    // its second plane (pair)
        TAIL = 16,      // the last `window` post-processed rows, carried from chunk to chunk (ping-pong pair)
        CODES = 18,     // the chunk's ADC codes as uploaded (pair; pss_ingest.hip unpacks them into IQ)
        NUMBERS = 20,   // per frame: range, peak, avg as float64, open and live as bytes (pair)
        WORK = 22,      // the chunk's live frames gathered, then the index lists of its live and open frames
        N_SLOTS
    };
    hipStream_t up = nullptr, dn = nullptr;   // upload and download stream; compute is the context's own
    hipEvent_t up_done[2] = {}, cmp_done[2] = {}, dn_done[2] = {};   // per buffer set: uploaded, computed, downloaded
    void *buf[N_SLOTS] = {};
    size_t cap[N_SLOTS] = {};
    int open(pss_ctx *ctx);   // streams and events, on first use
    int ensure(pss_ctx *ctx, int slot, size_t bytes, void **out);   // *out = the slot's buffer, at least `bytes` long (a grow frees and reallocates)
    void release()
    {
        if (up) hipStreamDestroy(up);
        if (dn) hipStreamDestroy(dn);
        for (hipEvent_t *ev : {up_done, cmp_done, dn_done})
            for (int i = 0; i < 2; i++)
                if (ev[i]) hipEventDestroy(ev[i]);
        for (void *b : buf)
            if (b) hipFree(b);
        *this = PssStreaming{};
    }
};

struct pss_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t stream2 = nullptr;  // side stream: the spectrum / display chain runs beside the demodulator (pss_side_* below)
    hipStream_t cur = nullptr;      // stream the next launches go to (nullptr = `stream`)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // pss_side_* only
    hipEvent_t ev_in = nullptr, ev_out = nullptr;   // pss_order_after / pss_order_before (created on first use)
    int n_cus = 0;                                  // hipDeviceProp_t::multiProcessorCount
    int fuse_post = 1;              // option "fuse_post" (float64-row pipelines, 1024-point frames): 1 = transform + post-process in ONE kernel (pss_spec_post.h), 0 = two kernels (A/B reference)
    int post_split = -1;            // option "post_split" (k_spectrum_post's one-round grid, pss_post_split.h): how many groups more the early workgroups take than the late ones; -1 = decided at the launch (equal shares unless an NFM backward pass runs beside the chain: pss_spec_post_chain), >= 0 = forced (sweeps, tests)
    double target_rate = 22050.0;   // demodulate_nfm / _wfm's target_rate (pss_set_target_rate): decimation factor int(fs / target_rate)
    bool wfm_corr_copy = false;     // option "wfm_corr_copy": always materialise the corrected copy of the batch (the round-4 path; A/B reference)
    std::string err;
    std::map<int, double2 *> tw;       // exp(-2 pi i k / N), k < N
    std::map<int, double *> win;       // np.hamming(N)
    std::map<int, double2 *> tw_pf;    // exp(+2 pi i k / N) as pocketfft tabulates it (pss_hilbert_pf.h), k < N
    struct Bluestein { double2 *d_chirp; double2 *d_B; double *d_win; int M; };
    std::map<int, Bluestein> bs;       // per frame length that is not a power of two (pss_fft.hip)
    std::map<double, PssNfmFilt> nfm;  // per sample rate
    std::map<double, std::array<double, 65>> ssb;
    std::map<double, PssWfmFilt> wfm;
    std::map<int, PssPairwisePlan> plans;
    void *scratch = nullptr;       // demodulator scratch (main stream)
    size_t scratch_bytes = 0;
    void *scratch_iqc = nullptr;   // IQ-corrected frames for the WFM dispatcher path
    void *scratch_scan = nullptr;  // scanner dB rows when the caller asks only for the per-slice numbers
    size_t scratch_scan_bytes = 0;
    void *scratch_pk = nullptr;
    size_t scratch_pk_bytes = 0;
    void *prog = nullptr;          // k_nfm_fwd: per-CU progress words of its workgroups (priority balancing)
    unsigned prog_epoch = 0;       // launch counter stamped into those words (16 bits, never 0)
    void *scratch_post = nullptr;  // pss_frame_pipeline_nfm without materialised post-processed rows: the rows' clamp thresholds
    size_t scratch_post_bytes = 0;
    void *scratch_db64 = nullptr;  // pss_frame_pipeline_cells / pss_spectrum_cells with float32 rows only, on lengths the fused kernel does not serve: the float64 rows
    size_t scratch_db64_bytes = 0;
    void *scratch_win = nullptr;   // sliding-window extremes of the batched display accumulators
    size_t scratch_win_bytes = 0;
    float *d_hann = nullptr;       // pss_classify: scipy's periodic Hann window (1024, float32) and sum(win * win)
    float hann_sum = 0.0f;
    PssStreaming st;               // the streamed entry points' streams, events and chunk buffers (pss_stream.cpp)
    float *d_hann_short = nullptr;  // the same for reads shorter than 1024 samples (window length = read length hann_short_n)
    float hann_short_sum = 0.0f;
    int hann_short_n = 0;
    size_t scratch_iqc_bytes = 0;
    void *scratch_fft = nullptr;   // spectrum scratch: separate, the spectrum kernel may run on the side stream
    size_t scratch_fft_bytes = 0;
    void *scratch_hil = nullptr;   // hilbert() of rows longer than 16384 samples (spectrum Z + pre-pass scratch): the demodulator's, never shared with the side stream's spectrum
    size_t scratch_hil_bytes = 0;
    void *stage = nullptr;         // device staging of the host-buffer convenience calls (grow-only)
    size_t stage_bytes = 0;
    bool no_wfm_fused = false;  // option "wfm_fused" = 0: k_wfm_front + k_nfm_iir path (A/B testing)
    long small_batch_max = 8192;  // option "small_batch_max": largest frame count that takes the small-batch path (measured crossover ~12000)
    long wfm_small_batch_max = 6000;  // option "wfm_small_batch_max" (crossover with the fused kernels, 1024-sample frames: ~12000 frames in round 2, ~6000 since the small-batch path is one array: 0.58 / 1.13 ms at 4096 / 8192 frames against 0.83)
    bool hilbert_exact = false;   // option "hilbert_exact": scipy.signal.hilbert bit for bit (pocketfft's butterfly order, pss_hilbert_pf.h) for rows of 256..1048576 samples
    bool ssb_rfft = true;      // option "ssb_rfft": frames of 8192 / 16384 samples evaluate hilbert() as a real transform pair (k_ssb_rfft); 0: two full-length complex transforms (k_ssb_hilbert_xl)
    bool ssb_hilbert = true;   // option "ssb_hilbert": run the reference's hilbert() round trip inside demodulate_ssb where a register transform exists for the frame length
    bool db_exact = false;         // true: compute_fft's dB rows evaluated to float64 accuracy and rounded once (= float32 of the reference's float64 rows); false: float32 evaluation, 1-2 ulp off, 15-25 % faster kernels
    bool f64_plain = false;        // option "f64_plain": the float64-row entry points (pss_spectrum_db_f64, pss_spectrum_post_f64, pss_frame_pipeline_nfm_f64) on the plain round-3 kernels (generic LDS transform with hypot / log10, radix select) instead of the register kernels: A/B reference
    bool scan_exact = true;        // scanner slices: NumPy's float32 chain bit for bit (scan_db_np); false: the float64 / hardware-log2 dB of compute_fft
    bool no_small_batch = false;  // option "small_batch" = 0: never take the systolic small-batch NFM path (A/B testing)
    bool no_fused = false;  // PSS_NO_FUSED=1: use the three-kernel NFM path (A/B and fallback testing)
    void *comm = nullptr;          // pss_comm_init: the RCCL communicator (ncclComm_t) of this context's rank; collectives run on the context's stream
    int comm_rank = 0, comm_n = 1;
    // squelch path (pss_squelch.hip), grow-only: [0] the gate's tile counts and result, [1] the open frames gathered for the demodulator,
    // [2] pss_frame_pipeline_squelch's float64 rows and index list; sq_pin: 16 pinned bytes the gate's count and carry-out land in
    void *sq_buf[3] = {};
    size_t sq_cap[3] = {};
    void *sq_pin = nullptr;
    // the channel family's cached tables, one per unit so that alternating calls do not evict each other
    PssDevTable ddc_tab;     // pss_ddc.hip: rotor knots, taps, frequency words
    PssDevTable pfb_tab;     // pss_pfb.hip: rotor knots, taps
    PssDevTable bank_tab;    // pss_bank.hip: twiddles of M, taps, digit reversal
    PssDevTable rs_tab;      // pss_resample.hip: the plan's numbers, then the taps in visit order
    PssDevTable welch_win;   // pss_welch.hip: the caller's window
    PssDevTable rds_tab;     // pss_rds.hip, pss_rds_front: rotor knots, taps
    PssDevTable rds_pulse;   // pss_rds.hip, pss_rds_bits: the pulse table
    PssDevTable ais_pulse;   // pss_ais.hip, pss_ais_front: the pulse table
    PssDevTable apt_tab;     // pss_apt.hip, pss_apt_front: rotor knots, taps
    PssDevTable packet_tones;   // pss_packet.hip, pss_packet_front: the tone table
    // pss_adsb.hip and pss_ais.hip, grow-only, shared as the gates share sq_buf (pss_starts.h): [0] the tiles' counts, offsets and lists,
    // [1] the listed starts with what the receiver keeps beside them (ADS-B: ranks and keep flags; AIS: payloads, lengths, scores as well)
    PssStartList starts;
    void *ook_first = nullptr;    // pss_ook.hip: a byte per detect tile, the polarity of its first edge, grow-only
    size_t ook_first_bytes = 0;
    void *welch_part = nullptr;   // pss_welch.hip: the block partials, grow-only
    size_t welch_part_bytes = 0;
    bool timing = false;
    std::string tfilter;  // pss_timing_filter: only launches of this kernel get events (and no per-call events); empty = all
    bool kskip = false;
    int tdepth = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = -1.0f;
    // per-kernel timing of the most recent outermost call (timing mode only)
    struct KRec { const char *name; hipEvent_t e0, e1; };
    std::vector<KRec> krecs;   // event pool (grown on demand, reused)
    int kused = 0;
};

// Every entry point works on ITS context's device, whatever the calling thread's current device is, and leaves the
// caller's current device as it found it (HIP's current device is per thread and defaults to 0).
struct PssDevGuard {
    int prev = -1;
    bool switched = false;
    explicit PssDevGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~PssDevGuard()
    {
        if (switched) hipSetDevice(prev);
    }
    PssDevGuard(const PssDevGuard &) = delete;
    PssDevGuard &operator=(const PssDevGuard &) = delete;
};
#define PSS_GUARD(ctx) PssDevGuard _pss_dev_guard((ctx)->device)

// Temporarily override a context switch (restored on scope exit, also on early returns)
template <class T>
struct PssScoped {
    T &ref;
    T keep;
    PssScoped(T &r, T v) : ref(r), keep(r) { r = v; }
    ~PssScoped() { ref = keep; }
    PssScoped(const PssScoped &) = delete;
    PssScoped &operator=(const PssScoped &) = delete;
};
using PssFlagScope = PssScoped<bool>;
using PssStreamScope = PssScoped<hipStream_t>;

int pss_fail(pss_ctx *ctx, int code, const std::string &msg);
int pss_hip_check(pss_ctx *ctx, hipError_t e, const char *what);
// The core entry points' pointer contract (include/pss.h, "pointer alignment"): a device pointer is valid when it is aligned to one record
// of its buffer (complex64 sample 8, float32 4, float64 / complex128 value 8, int16 [L, R] pair 4, int32 4); anything below that is refused
// here, before the first launch, with a message that names the argument.  A null pointer passes (whether it may be null is the entry
// point's own rule).  Which wider accesses the kernels make on such pointers, and why they are served: PARITY.md, "Views of buffers".
struct PssPtr { const void *p; unsigned align; const char *name; };
int pss_ptrs_aligned(pss_ctx *ctx, const char *entry, std::initializer_list<PssPtr> ptrs);
#define PSS_P(x, bytes) PssPtr{(x), (bytes), #x}
#define PSS_ALIGNED(ctx, entry, ...)                                      \
    do {                                                                  \
        int _a = pss_ptrs_aligned((ctx), (entry), {__VA_ARGS__});         \
        if (_a) return _a;                                                \
    } while (0)
int pss_ensure_scratch(pss_ctx *ctx, size_t bytes);
int pss_ensure_buffer(pss_ctx *ctx, void **buf, size_t *cap, size_t bytes, const char *what);
// Make t's device copy hold the `bytes` bytes at `img`: nothing where the mirror already equals them, otherwise an upload on the context's
// stream that has finished on return (img may be a local).  capacity: what to allocate where the buffer must grow (0: bytes).
int pss_table_sync(pss_ctx *ctx, PssDevTable *t, const void *img, size_t bytes, const char *what, size_t capacity = 0);
void pss_time_begin(pss_ctx *ctx);
void pss_time_end(pss_ctx *ctx);
// The timing bracket of a call (pss_last_kernel_ms): nested brackets are no-ops, the outermost one closes on every way out of its scope
struct PssTimeScope {
    pss_ctx *ctx;
    explicit PssTimeScope(pss_ctx *c) : ctx(c) { pss_time_begin(c); }
    ~PssTimeScope() { pss_time_end(ctx); }
    PssTimeScope(const PssTimeScope &) = delete;
    PssTimeScope &operator=(const PssTimeScope &) = delete;
};
// bracket ONE kernel launch with events on the context's stream (no-ops unless timing is enabled)
void pss_kernel_begin(pss_ctx *ctx, const char *name);
void pss_kernel_end(pss_ctx *ctx);

#define PSS_STREAM(ctx) ((ctx)->cur ? (ctx)->cur : (ctx)->stream)

// "Run this on stream2 beside the main stream" (pss_api.cpp).  pss_side_fork: stream2 waits for everything queued on the main stream so far
// (pss_side_mark + pss_side_wait: the same in two steps, for a fork point inside the demodulator); pss_on_side: f's launches go to stream2;
// pss_side_join: the main stream waits for stream2 — to be attempted whatever happened in between, the main stream must never run ahead of
// the side stream.
int pss_side_mark(pss_ctx *ctx);
int pss_side_wait(pss_ctx *ctx);
int pss_side_fork(pss_ctx *ctx);
int pss_side_join(pss_ctx *ctx);
template <class F>
int pss_on_side(pss_ctx *ctx, F &&f)
{
    PssStreamScope side(ctx->cur, ctx->stream2);
    return f();
}

// ---- the demodulator's internal call (pss_demod.hip): what the public entry points and the pipelines (pss_pipeline.hip) build -----------------
struct PssIq {   // a batch of read buffers [n_frames][n]: complex64 (f32) or complex128 (f64, the SSB kernels' float64 loader), one of the two
    const float *f32 = nullptr;
    const double *f64 = nullptr;
};
// The backward launch of the fused NFM / WFM paths as data (k_nfm_bwd's arguments), for a caller that places it itself
struct PssBwdLaunch {
    const PssNfmFilt *flt = nullptr;   // the decimator (the context's cached design); NULL: nothing was handed back
    bool stereo = false;               // WFM: both channels of a tile, joint normalisation
    double *Yf = nullptr, *Af = nullptr;
    int n = 0, q = 0, n_out = 0;
    long n_frames = 0;
    int16_t *d_pcm = nullptr; double *d_audio = nullptr;
    int launch(pss_ctx *ctx) const;
};
enum PssAfterFwd { PSS_RUN_ALL = 0, PSS_FORK_AFTER_FWD, PSS_DEFER_BWD };
struct PssDemodCall {   // in: correct, d_power, after_fwd; out: forked, bwd
    bool correct = false;          // WFM: the frames are AS READ, iq_correction comes first (demodulate_signal's dispatcher)
    float *d_power = nullptr;      // AM: the power dB of the same frames, out of the mean pass
    PssAfterFwd after_fwd = PSS_RUN_ALL;   // fused NFM / WFM paths: PSS_FORK_AFTER_FWD marks the fork point behind the forward kernel (NFM),
                                           // PSS_DEFER_BWD launches the forward kernel only and hands the backward launch back
    bool forked = false;           // pss_side_mark was called: the caller owes pss_side_wait .. pss_side_join
    PssBwdLaunch bwd;              // bwd.flt != NULL: the caller owes bwd.launch(ctx)
};
// Checks its arguments as pss_demod does; call == NULL: a default PssDemodCall
int pss_demod_run(pss_ctx *ctx, int mode, PssIq iq, long n_frames, int n, double fs, int16_t *d_pcm, double *d_audio, PssDemodCall *call);

#define PSS_HIP(ctx, call)                                         \
    do {                                                           \
        int _r = pss_hip_check((ctx), (call), #call);              \
        if (_r) return _r;                                         \
    } while (0)

// implemented in pss_ingest.hip: the argument rules every *_codes entry point shares (container, scale, table); ctx may be NULL
int pss_iq_check(pss_ctx *ctx, int container, double scale, const float *h_table256);
// A host capture's sample format: complex64 as it is (the default), or ADC codes that are unpacked on the device.  `codes` is set by
// of_codes alone, never derived from the caller's container, so no container value can select the complex64 path.
struct PssIqFmt {
    bool codes = false;
    int container = 0;
    double scale = 0.0;
    const float *h_table256 = nullptr;
    static PssIqFmt of_codes(int container, double scale, const float *h_table256)
    {
        PssIqFmt f;
        f.codes = true, f.container = container, f.scale = scale, f.h_table256 = h_table256;
        return f;
    }
    size_t sample_bytes() const { return codes ? (size_t)pss_iq_code_bytes(container) : 2 * sizeof(float); }   // behind pss_iq_check
};

// implemented in pss_squelch.hip: d_dst[k] = frame d_idx[k] of the batch [n_frames][n], k < n_idx (indices outside the batch are clamped into it);
// d_iq aligned to one sample (8 bytes).  Stream-ordered.
int pss_gather_frames(pss_ctx *ctx, const float *d_iq, long n_frames, int n, const int32_t *d_idx, long n_idx, float *d_dst);

// implemented in pss_fft.hip
bool pss_hilbert_supported(int n);
int pss_hilbert_rows(pss_ctx *ctx, const double *d_x, long n_rows, int n, double *d_out, int out_mode, unsigned long long *d_maxbits,
                     int16_t *d_pcm);
int pss_fft_tables(pss_ctx *ctx, int n, const double2 **tw, const double **win);
// pss_frame_pipeline's display chain behind the dB rows (rows of either type): thresholds + extremes + the rows resampled to the display
// width in one pass (no post-processed rows in memory), sliding extremes, the line of every frame.  d_vals: n_frames x disp_w doubles.
bool pss_post_sel_serves(int n_fft, bool f64);
bool pss_spec_post_serves(const pss_ctx *ctx, int n_fft);
int pss_spec_post_chain(pss_ctx *ctx, const float *d_iq, long n_frames, int n_fft, float *d_db32, double *d_db64, double *d_lo, double *d_hi, int n_halo,
                        int window, int display, int disp_h, int disp_w, int8_t *d_a, int8_t *d_b, double *d_vals, const PssBwdLaunch *beside_bwd = nullptr);
int pss_chain_vals_f32(pss_ctx *ctx, const float *d_db, long n_frames, int n_fft, float *d_lo, float *d_hi, int n_halo, int window, int display,
                       int disp_h, int disp_w, int8_t *d_a, int8_t *d_b, double *d_vals);
int pss_chain_vals_f64(pss_ctx *ctx, const double *d_db, long n_frames, int n_fft, double *d_lo, double *d_hi, int n_halo, int window, int display,
                       int disp_h, int disp_w, int8_t *d_a, int8_t *d_b, double *d_vals);
bool pss_ssb_fused_supported(int n);
// NumPy's float32 arctan2 on the host, the statements of pss_device.h's atan2f_svml (pss_mono.hip)
float pss_h_atan2f_model(float y, float x);
// NumPy's float64 tan / exp under its AVX512_SKX dispatch (SVML's _ha routines restated, pss_design.cpp)
double pss_np_tan(double x);
double pss_np_exp(double x);
// scipy.signal.firwin(numtaps, cutoff, window=('kaiser', beta)) for an odd numtaps >= 3 and 0 <= beta <= 8 (pss_design.cpp)
int pss_design_firwin_kaiser(int numtaps, double cutoff, double beta, double *taps);
int pss_ssb_hilbert_fused(pss_ctx *ctx, const float *d_iq, long n_rows, int n, const double *taps65, double *d_audio, int16_t *d_pcm);

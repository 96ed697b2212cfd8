/*
 * pss.h — C ABI of libpss.so, the MI355X (gfx950) implementation of PySpecSDR's IQ -> spectrum + demod
 * hot path.  Plain C: pointers and sizes only, no torch / HIP types in any signature.
 *
 * What this replaces.  The reference (xqtr/PySpecSDR, pure Python) has no FFI; its hot path is the module
 * namespace `from signal_processing import *` (pyspecsdr.py:98).  Each entry point below names the
 * reference callable it replaces; pyspecsdr_amd/signal_processing.py is the ctypes binding that presents
 * those callables with their original Python signatures (INTEGRATION.md shows the two-line patch).
 *
 * Conventions
 *   - iq: interleaved complex64 (I0,Q0,I1,Q1,...) — the SoapySDR CF32 buffer of SDRDevice.read_samples
 *     (pyspecsdr.py:1885-1891).  Batched calls take n_frames contiguous frames of n samples each.
 *   - `d_` parameters are DEVICE pointers (hipMalloc / torch tensors' data_ptr); `h_` are host pointers.
 *   - All functions return 0 on success or a negative pss_status; pss_last_error() gives the text.
 *     Nothing aborts or throws.  A missing GPU is an error (PSS_E_HIP), never a CPU fallback.
 *   - A context is bound to one device and one stream; calls on a context are stream-ordered and must
 *     not be issued concurrently from several threads.  Batched calls are asynchronous w.r.t. the host
 *     unless stated; call pss_sync() (or sync the stream you supplied) before reading results.
 */
#ifndef PSS_H
#define PSS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pss_ctx pss_ctx;

typedef enum {
    PSS_OK = 0,
    PSS_E_ARG = -1,      /* bad argument (size not supported, null pointer, ...) */
    PSS_E_HIP = -2,      /* HIP runtime error / no device */
    PSS_E_PADLEN = -3,   /* NFM: n-1 <= 27 -> the reference raises ValueError (scipy sosfiltfilt padlen)   */
    PSS_E_CUTOFF = -4,   /* NFM/SSB: cutoff >= Nyquist -> the reference raises ValueError (scipy firwin)  */
    PSS_E_NOMEM = -5,
    PSS_E_COMM = -6      /* multi-GPU exchange: librccl not found, no communicator, or an RCCL error (text in pss_last_error) */
} pss_status;

typedef enum { PSS_MODE_NFM = 0, PSS_MODE_AM = 1, PSS_MODE_USB = 2, PSS_MODE_LSB = 3, PSS_MODE_WFM = 4 } pss_mode;

/* ---- context ------------------------------------------------------------------------------------ */
int pss_create(int device, pss_ctx **out);
void pss_destroy(pss_ctx *ctx);
/* Use an existing hipStream_t (passed as void*) instead of the context's own stream; NULL = default stream. */
int pss_set_stream(pss_ctx *ctx, void *hip_stream);
/* The hipStream_t (as void*) the context's work is queued on: lets a caller order its own streams / events against it
 * (e.g. torch.cuda.ExternalStream(pss_get_stream(ctx)) to overlap an RCCL gather with the next batch). */
void *pss_get_stream(pss_ctx *ctx);
/* Order the context's stream against a caller's stream (hipStream_t as void*, NULL = the default stream) WITHOUT adopting it — the context
 * keeps its own non-blocking stream, which the legacy default stream does not synchronise with:
 *   pss_order_after:  work queued on the context from now on starts after everything queued on the caller's stream so far (inputs the
 *                     caller produced, outputs it cleared);
 *   pss_order_before: work queued on the caller's stream from now on starts after everything the context has queued so far (results).
 * One event record + one stream wait each (~2 us), nothing blocks the host.  A single-threaded caller that fills buffers on its stream,
 * calls an entry point and reads the results on its stream — the call order of the reference's loop, pyspecsdr.py:2250-2283 — brackets every
 * call with the pair; pyspecsdr_amd.engine.Engine does so by default with torch's current stream. */
int pss_order_after(pss_ctx *ctx, void *hip_stream);
int pss_order_before(pss_ctx *ctx, void *hip_stream);
int pss_sync(pss_ctx *ctx);
const char *pss_last_error(pss_ctx *ctx); /* ctx may be NULL: error of the last failed pss_create */
int pss_device_count(void);
/* Switches.  Returns PSS_E_ARG for unknown keys.  Every alternative path produces the same int16 samples and float64 audio.
 *   "nfm_fused" (1)            0: lane-per-frame three-kernel NFM path (front, edge, iir) instead of the fused kernels (test fallback)
 *   "wfm_fused" (1)            0: k_wfm_front + lane-per-frame decimator instead of the fused WFM forward kernel (test fallback)
 *   "small_batch" (1)          0: never take the latency-oriented small-batch kernels (one lane per filter section)
 *   "small_batch_max" (8192)   largest NFM frame count that takes them;  "wfm_small_batch_max" (6000) likewise for WFM
 *   "ssb_hilbert" (1)          0: demodulate_ssb skips the reference's hilbert() FFT round trip (the identity on the real part it
 *                              keeps, up to ~1e-16); 1: executed for power-of-two frames of 256..1048576 samples
 *   "hilbert_exact" (0)        1: pss_hilbert and demodulate_ssb's hilbert() run pocketfft's own butterfly order for rows of 256..1048576
 *                              samples (real radix-4 / radix-2 forward passes, complex radix-8 / 4 / 2 inverse passes, its twiddle products):
 *                              the analytic signal and the SSB float64 audio then equal SciPy's on every bit.  0 (default): the register
 *                              transforms, within 2e-14 of it (int16 PCM equal either way) and about twice as fast
 *   "db_exact" (0)             1: compute_fft's dB rows (pss_spectrum_db and everything built on it) are evaluated to float64 accuracy and
 *                              rounded once: the float32 row then IS the float32 rounding of the reference's float64 row (all 69 490
 *                              golden values; measured on FM frames: 5 of 8.4 million bins off by one ulp, where the value lies within
 *                              ~1e-15 of a rounding boundary).  0 (default): float32 evaluation of the logarithm, 1-2 ulp from that
 *                              (the contract is 1e-4 relative); the exact evaluation costs the spectrum kernels 15-25 % (0.17 -> 0.20 ms
 *                              at cfg 2, 0.75 -> 0.91 ms at 8192 x 16384) and the bench step 3 %
 *   "scan_exact" (1)           0: scanner slices (pss_scan, pss_scan_threshold) get their dB values from compute_fft's float64 / hardware-log2
 *                              evaluation (1e-4 relative; 30 % faster at 8192 x 4096) instead of NumPy's float32 chain bit for bit
 * Any other key is refused with PSS_E_ARG ("unknown option").  The kernel-selection knobs of earlier rounds' A/B measurements are gone
 * with the kernels they selected; those experiments and the others that lost — the FIR on the matrix
 * pipe, discriminator rows handed from the spectrum kernel, the fused spectrum + post-process kernel, the 112-VGPR spectrum kernel, the
 * alternative pipeline schedules, CU-mask partitioning — are documented with their measurements in DESIGN.md and no longer compiled in. */
int pss_set_option(pss_ctx *ctx, const char *key, int value);

/* ---- filter design (host side, pure C++; replaces the per-call SciPy design work) --------------
 * The designers restate SciPy's / NumPy's arithmetic operation by operation (DESIGN.md par. 2): firwin, cheby1 as scipy.signal.decimate
 * calls it, sosfilt_zi and butter return SciPy 1.15's tables bit for bit at every cutoff / decimation factor / sample rate tried (the pre-warp
 * tan is NumPy's SVML routine restated, pss_h_np_f64). */
/* scipy.signal.firwin(numtaps, cutoff) low-pass, Hamming window, cutoff normalised to Nyquist
 * (signal_processing.py:107 and :203/:208).  Returns PSS_E_CUTOFF unless 0 < cutoff < 1. */
int pss_design_firwin(int numtaps, double cutoff, double *taps);
/* scipy.signal.cheby1(order, rp_db, wn, output='sos') low-pass, order even (decimate(): order 8, rp 0.05,
 * wn 0.8/q — signal_processing.py:112 via scipy _signaltools.py:4831).  sos[order/2][6]. */
int pss_design_cheby1_sos(int order, double rp_db, double wn, double *sos);
/* scipy.signal.butter(order, Wn, output='sos'): low-pass with cutoff wn_high when wn_low <= 0 (as bandpass_filter does,
 * signal_processing.py:37-39), else band-pass [wn_low, wn_high] (:41).  sos[ceil(order/2)][6] (low) / sos[order][6] (band);
 * *nsec (nullable) receives the row count.  PSS_E_CUTOFF where SciPy raises ValueError (Wn outside 0 < Wn < 1). */
int pss_design_butter_sos(int order, double wn_low, double wn_high, double *sos, int *nsec);
/* scipy.signal.sosfilt_zi(sos).  zi[nsec][2]. */
int pss_design_sosfilt_zi(const double *sos, int nsec, double *zi);
/* NumPy's float64 tan (op 0) / exp (op 1) as the reference's SciPy calls evaluate them (NumPy's AVX512_SKX dispatch: SVML, an ulp from libm
 * on 0.5 % / 5 % of arguments) — the two primitives the designers need beyond libm; host arrays. */
int pss_h_np_f64(int op, const double *x, long n, double *out);
/* butter(5, [300, 3000]/(22050/2), 'band', output='sos') — the fixed AM filter (signal_processing.py:188-191,
 * :39-41; pyspecconst.py:3,5).  sos[5][6]. */
int pss_am_bandpass_sos(double *sos);

/* Override the designed coefficients for a sample rate (e.g. with tables captured from SciPy). Optional. */
int pss_set_nfm_filters(pss_ctx *ctx, double fs, const double *taps65, const double *sos4x6, const double *zi4x2);
int pss_set_ssb_taps(pss_ctx *ctx, double fs, const double *taps65);
/* Read back the coefficients the context uses for fs (designing them on first use). */
int pss_get_nfm_filters(pss_ctx *ctx, double fs, double *taps65, double *sos4x6, double *zi4x2);
int pss_get_ssb_taps(pss_ctx *ctx, double fs, double *taps65);

/* ---- batched device entry points --------------------------------------------------------------- */
/* Pointer alignment.  A caller does not have to hand these entry points whole allocations: a capture resident on the device may be cut
 * into frames at any sample (d_capture + 2 * k floats), a float32 row may lie inside a larger grid, a PCM ring may be written at a running
 * offset.  A device pointer is valid when it is aligned to ONE RECORD of its documented layout:
 *     complex64 samples (d_iq, d_out_iq)            one sample            8 bytes
 *     float32 values (dB rows, extremes, power ...)  one value             4
 *     float64 values, complex128 (re, im) values     one float64           8
 *     int16 PCM [n_out][2]                           one [L, R] pair       4
 *     int32 / uint32 values (indices, counts, masks) one value             4
 *     int8 / uint8 grids, lines, bits, flags         one byte              1
 * Every entry point from here to pss_lfilter, and pss_afsk_bits, pss_np_f32 and pss_row_normalise further down, SERVES such a pointer
 * with the bytes it produces for a 256-byte-aligned one: where a kernel moves 8 or 16 bytes per lane on a caller's buffer it does so
 * with plain address arithmetic on the pointer as given (or aligns itself, as k_vector_masks does), and no atomic operation is ever made
 * on a caller's buffer.  A pointer BELOW its record's alignment (a d_pcm at 2 bytes, a float32 row at 2, a d_iq at 4) is refused before
 * anything is launched: PSS_E_ARG, "<entry point>: <argument> must be <n>-byte aligned", outputs untouched.  Either way a call touches
 * no byte outside its documented buffers and never writes its inputs.  (Serving a float32 row or a PCM pointer 4 bytes off a 16-byte boundary
 * relies on MEASURED behaviour of gfx950 under the driver's default memory configuration — multi-dword vector-memory accesses need dword
 * alignment only —, not on an architectural guarantee: a port re-runs tests/test_gpu_views_of_buffers.py.)  PARITY.md ("Views of buffers") lists every access wider than its
 * buffer's record with file and line; tests/test_gpu_views_of_buffers.py runs every entry point one record off, between guard bands.
 * The units further down that take strides and capture offsets (pss_ddc .. pss_apt_lines, pss_unpack_iq, pss_live_frames,
 * pss_demod_gated, pss_decode_mono) state their own alignment rules where they are declared. */
/* compute_fft (signal_processing.py:243-264) for n_frames frames: Hamming window, n_fft-point FFT (float64
 * butterflies), fftshift, 10*log10(|X|^2 + 1e-10).  d_db: float32 [n_frames][n_fft].
 * n_fft: a power of two in [16, 1048576] (register / LDS radix-16 kernels), or any other length in [2, 524288]
 * (Bluestein's algorithm over the two-pass 2^17..2^20-point transform: NumPy's fft takes any length too). */
int pss_spectrum_db(pss_ctx *ctx, const float *d_iq, long n_frames, int n_fft, float *d_db);
/* Caller-side post-process (pyspecsdr.py:2278-2283): 5-tap moving average ('valid') then clamp below
 * median-10.  d_post: float32 [n_frames][n_fft-4]. */
int pss_spectrum_post(pss_ctx *ctx, const float *d_db, long n_frames, int n_fft, float *d_post);
/* The same, and the finite minimum / maximum of every post-processed row (float32 [n_frames] each; (+inf, -inf) for a row
 * without a finite value): what the display accumulators below normalise with. */
int pss_spectrum_post_extremes(pss_ctx *ctx, const float *d_db, long n_frames, int n_fft, float *d_post, float *d_row_lo,
                               float *d_row_hi);
/* compute_fft and the post-process of the same frames in one call (d_db, d_post, and — both or neither — the row extremes): two launches. */
int pss_spectrum_db_post(pss_ctx *ctx, const float *d_iq, long n_frames, int n_fft, float *d_db, float *d_post, float *d_row_lo,
                         float *d_row_hi);
/* Finite extremes of arbitrary rows (np.min / np.max over all_data[np.isfinite(all_data)], pyspecsdr.py:1356-1358, per row). */
int pss_row_extremes(pss_ctx *ctx, const float *d_rows, long n_rows, int len, float *d_row_lo, float *d_row_hi);
int pss_row_extremes_f64(pss_ctx *ctx, const double *d_rows, long n_rows, int len, double *d_row_lo, double *d_row_hi);
/* Inline scanner slice (pyspecsdr.py:2542-2552): unwindowed FFT, dB, peak, 20-dB-down bin count,
 * bandwidth = count * fs / n_fft.  d_db float32 [n][n_fft] (may be NULL), d_peak float32 [n],
 * d_bw float64 [n], d_count int32 [n] (may be NULL).  n_fft: power of two in [16, 16384] (one kernel), or any other
 * length in [2, 524288] (Bluestein + a reduction kernel).  The dB values are the reference's float32 values bit for bit (so are
 * peak, count and bandwidth): np.fft.fft on complex64 is a double transform rounded to complex64 (NumPy 2.2), everything behind
 * it float32 arithmetic that is modelled exactly; a bin can differ only if a float64 component lies within the transform's ~1e-16 * max|X|
 * of a float32 rounding boundary (weak bins beside a strong carrier: ~1e-6 of the bins) (option "scan_exact" = 0: the 1e-4-relative evaluation of pss_spectrum_db, 30 % faster). */
int pss_scan(pss_ctx *ctx, const float *d_iq, long n_slices, int n_fft, double fs, float *d_db, float *d_peak,
             double *d_bw, int32_t *d_count);
/* The sweep driver's per-read arithmetic (scan_frequencies, pyspecsdr.py:1049-1057): unwindowed fft of a read of
 * n = int(0.1 * fs) samples (240 000 at 2.4 MS/s: not a power of two), dB, max_power, bins above the ABSOLUTE threshold,
 * bandwidth = count * fs / n.  Buffers as for pss_scan (d_db, d_peak, d_bw, d_count may each be NULL). */
int pss_scan_threshold(pss_ctx *ctx, const float *d_iq, long n_slices, int n, double fs, double threshold_db, float *d_db,
                       float *d_peak, double *d_bw, int32_t *d_count);
/* iq_correction — signal_processing.py:46-80, per frame: DC removal, IQ amplitude/phase balance, power restore; float32
 * throughout, bit-identical to the reference on NumPy 2.2.  d_out_iq: complex64 [n_frames][n] (nullable);
 * d_raw: float32 [n_frames][n] = real part = demodulate_signal(..., 'RAW') (signal_processing.py:222-238) (nullable). */
int pss_iq_correction(pss_ctx *ctx, const float *d_iq, long n_frames, int n, float *d_out_iq, float *d_raw);

/* scipy.signal.hilbert along n_rows float64 rows of n samples (the analytic signal demodulate_ssb builds,
 * signal_processing.py:205, :210): fft, one-sided mask, ifft.  n: a power of two in [256, 1048576] (PSS_E_ARG otherwise) — up to
 * 16384 both transforms in one kernel; longer rows (the reference's read buffers: 32768 by default, up to 2^20) through a complex
 * float64 spectrum in HBM.  d_analytic: complex128 [n_rows][n] (interleaved re, im). */
int pss_hilbert(pss_ctx *ctx, const double *d_x, long n_rows, int n, double *d_analytic);

/* measure_signal_power (signal_processing.py:325-328): float32 [n_frames]. */
int pss_power_db(pss_ctx *ctx, const float *d_iq, long n_frames, int n, float *d_power);
/* adjust_gain (pyspecsdr.py:898-919) run sequentially over a series of power readings:
 * d_idx_out[i] = gain index after reading i, starting from start_idx. */
int pss_agc_steps(pss_ctx *ctx, const float *d_power, long n, int start_idx, int n_gains, int32_t *d_idx_out);

/* demodulate_signal (signal_processing.py:220-240) for NFM / AM / USB / LSB, every frame independently
 * (filter state reset and peak normalisation per frame, exactly like the reference's per-buffer calls).
 *   n_out per frame = pss_demod_out_len(mode, n, fs): NFM ceil((n-1)/int(fs/22050)), AM/SSB n.
 *   d_pcm   int16  [n_frames][n_out][2]  — np.int16(audio*32767), L=R  (io_manager.py:25-26); may be NULL
 *   d_audio double [n_frames][n_out]     — the mono float64 audio before stereo duplication; may be NULL */
int pss_demod(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, int16_t *d_pcm,
              double *d_audio);
int pss_demod_out_len(int mode, int n, double fs);
/* demodulate_nfm / demodulate_wfm's `target_rate` argument (signal_processing.py:91, :119; default DEFAULT_SAMPLE_RATE = 22050): the decimation
 * factor is int(sample_rate / target_rate) (:111).  pss_set_target_rate changes it for the context (and drops the cached decimator designs);
 * pss_demod_out_len_ctx is pss_demod_out_len at the context's target rate, pss_demod_out_len_rate at an explicit one.
 * Every factor >= 1 is served: NFM runs decimate(x, 1) at factor 1 (as the reference does); WFM at factor 1 skips the decimate() stage as
 * the reference does (:152-155) and normalises the de-emphasised channels (n - 1 samples per channel; plain kernels). */
int pss_set_target_rate(pss_ctx *ctx, double target_rate);
int pss_demod_out_len_ctx(pss_ctx *ctx, int mode, int n, double fs);
int pss_demod_out_len_rate(int mode, int n, double fs, double target_rate);

/* PSS_MODE_WFM = demodulate_wfm (signal_processing.py:119-176): discriminator, L+R / pilot / L-R Butterworth branches,
 * 75 us de-emphasis, zero-phase decimation, joint peak normalisation.  n_out = ceil((n-1)/int(fs/22050)); here
 *   d_audio double [n_frames][n_out][2] holds np.column_stack((left, right)) and d_pcm its int16 image.
 * pss_demod() runs the demodulator on the samples as given; pss_demod_signal() is the reference's dispatcher
 * demodulate_signal (:220-240): identical for NFM/AM/USB/LSB, and for WFM it applies iq_correction first (:222-225). */
int pss_demod_signal(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, int16_t *d_pcm,
                     double *d_audio);
/* measure_signal_power (signal_processing.py:325-328) and demodulate of the same read buffers, as the main loop runs them back to back
 * (pyspecsdr.py:2251, :2262).  d_power float32 [n_frames]: pss_power_db's bits; d_pcm / d_audio: pss_demod's.  For AM the power and the
 * demodulator's mean of |x| are reduced in ONE pass over the IQ; for the other modes this is the two calls in order. */
int pss_demod_power(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, int16_t *d_pcm, double *d_audio,
                    float *d_power);
/* WFM filter set of one sample rate: lp = butter(5, 15000/(fs/2)) [3][6], pilot = butter(5, [18800,19200]/(fs/2), 'band')
 * [5][6], lmr = butter(5, [23000,53000]/(fs/2), 'band') [5][6], alpha = exp(-1/(75e-6 fs)).  Designed on first use
 * (pss_design_butter_sos and NumPy's exp restated: SciPy 1.15's / NumPy's bits); set_ lets a caller inject another SciPy build's tables. */
int pss_set_wfm_filters(pss_ctx *ctx, double fs, const double *lp3x6, const double *pilot5x6, const double *lmr5x6,
                        double alpha);
int pss_get_wfm_filters(pss_ctx *ctx, double fs, double *lp3x6, double *pilot5x6, double *lmr5x6, double *alpha);

/* Headline fused call: spectrum + NFM demod of the same frames (BASELINE.json metric). */
int pss_spectrum_nfm(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, float *d_db,
                     int16_t *d_pcm);

/* One iteration of the reference's main loop (pyspecsdr.py:2262-2283 and the waterfall draw) for a batch of read buffers:
 * NFM demod -> d_pcm; compute_fft -> d_db [n_frames][n]; post-process -> d_post [n_frames][n-4] and the row extremes
 * (d_row_lo / d_row_hi: [n_halo + n_frames], the first n_halo entries supplied by the caller as for pss_waterfall_rows);
 * waterfall line per frame -> d_glyph / d_colour [n_frames][disp_w].  The same results as the separate calls; part of the
 * display chain runs on a side stream beside the demodulator's backward pass and is joined before the call returns.
 * d_post may be NULL: the post-processed rows are then not written to memory at all (a third of the chain's HBM traffic) — the
 * display lines are the same bytes, rebuilt from the dB rows and the 12 bytes per row that pss_spectrum_post_thresholds leaves. */
int pss_frame_pipeline_nfm(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, float *d_db, float *d_post,
                           float *d_row_lo, float *d_row_hi, int n_halo, int window, int disp_w, int8_t *d_glyph,
                           int8_t *d_colour, int16_t *d_pcm);

/* The same iteration in ANY of the main loop's demodulation modes — demodulate_signal(samples, fs, CURRENT_DEMOD) (pyspecsdr.py:2262), whose
 * default is WFM (:2855) — and for either batched display accumulator.  mode: PSS_MODE_*, with demodulate_signal's dispatcher semantics (WFM
 * frames are IQ-corrected first, signal_processing.py:222-225; compute_fft sees the samples as read, pyspecsdr.py:2275).  d_pcm int16
 * [n_frames][pss_demod_out_len(mode, n, fs)][2].  display 0: waterfall line, d_line_a = glyph, d_line_b = colour (window: 30 in the reference);
 * display 1: persistence trace, d_line_a = row index per column, d_line_b unused (may be NULL), disp_h <= 127 (window: 10 in the reference);
 * display 2: gradient line (pss_gradient_rows), d_line_a = index into ' ._-=+*#@', d_line_b = colour (window: 30 in the reference) — here and
 * wherever `display` is an argument below (pss_frame_pipeline_f64, pss_frame_pipeline_cells, pss_spectrum_cells, pss_frame_pipeline_squelch).
 * The other arguments and the results are those of the separate calls (pss_demod_signal, pss_spectrum_db, pss_spectrum_post_extremes /
 * _thresholds, pss_waterfall_rows[_db] / pss_persistence_rows[_db]); NFM runs the schedule of pss_frame_pipeline_nfm, the other modes run the
 * display chain on the side stream beside the whole demodulator.  PSS_E_ARG for n < 8 (no post-processed row), n_halo < 0, window < 1. */
int pss_frame_pipeline(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db, float *d_post,
                       float *d_row_lo, float *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w, int8_t *d_line_a,
                       int8_t *d_line_b, int16_t *d_pcm);

/* The reference's own row type.  compute_fft returns float64 rows (signal_processing.py:243-264) and the caller smooths, clamps and
 * draws them in float64 (pyspecsdr.py:2278-2283, :1342-1406); the float32 rows above agree with them to 1e-7 relative, but a display cell
 * can differ where a value sits on a quantisation edge (<= 2e-3 of the cells).  These entry points keep float64 throughout, so the
 * display lines are the reference's cells.  Since round 5 they run on the register kernels of the float32 calls (float64 dB values stored from
 * the transform's registers for 256 .. 4096 points, register select on 64-bit keys up to 16 388 points; option "f64_plain" = 1: the plain
 * round-3 kernels) and pss_frame_pipeline_nfm_f64 is the step bench.py times.  n_fft: a power of two in [16, 65536].
 *   pss_spectrum_db_f64:   d_db float64 [n_frames][n_fft] = 10 log10(|fftshift(fft(iq * hamming))|^2 + 1e-10)
 *   pss_spectrum_post_f64: d_post float64 [n_frames][n_fft - 4]; d_row_lo / d_row_hi [n_frames] (both or neither): finite extremes
 *   pss_frame_pipeline_nfm_f64: pss_frame_pipeline_nfm with float64 rows, extremes (and halo) */
int pss_spectrum_db_f64(pss_ctx *ctx, const float *d_iq, long n_frames, int n_fft, double *d_db);
int pss_spectrum_post_f64(pss_ctx *ctx, const double *d_db, long n_frames, int n_fft, double *d_post, double *d_row_lo,
                          double *d_row_hi);
int pss_frame_pipeline_nfm_f64(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, double *d_db, double *d_post,
                               double *d_row_lo, double *d_row_hi, int n_halo, int window, int disp_w, int8_t *d_glyph,
                               int8_t *d_colour, int16_t *d_pcm);
/* pss_frame_pipeline (any demodulation mode, waterfall line or persistence trace) with float64 rows: the cells of either batched accumulator
 * as the reference draws them from this IQ.  d_post may be NULL (rows of up to 16 388 points are then never materialised). */
int pss_frame_pipeline_f64(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, double *d_db, double *d_post,
                           double *d_row_lo, double *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w, int8_t *d_line_a,
                           int8_t *d_line_b, int16_t *d_pcm);

/* The cell-exact iteration with the dB ROW materialised as float32.  Everything is computed in float64 from the IQ to the display cells, as
 * in pss_frame_pipeline_f64 (compute_fft signal_processing.py:243-264, the caller's smoothing + median clamp pyspecsdr.py:2278-2283, the
 * accumulators :1342-1406 / :1512-1564), but what is written per bin is compute_fft's float64 value ROUNDED ONCE to float32 — d_db32
 * [n_frames][n], the spectrum output's own contract (1e-4 relative; the rounding is ~6e-8) and SURVEY's 4 bytes per bin — and, only if
 * d_db64 != NULL, the float64 value as well.  1024-point frames: the transform and the post-process of a frame are ONE kernel
 * (k_spectrum_post: the frame's float64 dB values go from the transform's registers through LDS into the select; option "fuse_post" = 0:
 * two kernels) — the float64 rows never travel through HBM unless asked for.  Other lengths: the float64 rows go through d_db64 or a
 * context-owned scratch, and a conversion pass writes d_db32.  The float64 entry points above use the fused kernel too (their d_db = d_db64).
 *   pss_frame_pipeline_cells: pss_frame_pipeline_f64's arguments with (d_db32, d_db64) in place of d_db and no d_post; this is the step bench.py times
 *   pss_spectrum_cells:       its display half alone — compute_fft -> post-process -> display line of every frame, no demodulator
 *                             (d_db32 or d_db64 may be NULL, not both) */
int pss_frame_pipeline_cells(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                             double *d_row_lo, double *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w,
                             int8_t *d_line_a, int8_t *d_line_b, int16_t *d_pcm);
int pss_spectrum_cells(pss_ctx *ctx, const float *d_iq, long n_frames, int n, float *d_db32, double *d_db64, double *d_row_lo,
                       double *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w, int8_t *d_line_a, int8_t *d_line_b);

/* Squelch and the header's Peak / Avg meter.  The reference does not demodulate every read buffer: its loop gates the audio,
 *     if PEAK_POWER >= SQUELCH: audio = demodulate_signal(...); audio_buffer.append(audio)          (pyspecsdr.py:2261-2263)
 * where draw_header sets PEAK_POWER = np.max(freq_data) of the post-processed row and prints np.mean(freq_data) beside it ("Peak: x dB
 * Avg: y dB", :388-392).  draw_header runs on every third iteration only (ui_update_counter, :2288-2291); PEAK_POWER starts at 0 and
 * SQUELCH at -60 (:171-172).  Frames 0 .. n_frames-1 of a batch are successive iterations (VFO mode), with a counter that stands at
 * `phase` before frame 0:
 *     open[i]  = held >= squelch, `held` being the value BEFORE iteration i (a NaN compares false: closed; +inf opens);
 *     then the counter is incremented and, if counter % every == 0, frame i is METERED: held = np.max(row_i).
 * every = 3 in the reference; every = 0: never metered (its MR mode draws no header), phase must then be 0.  A batch cut into several
 * calls carries (held_out, (phase + n_frames) % every) from one call into the next.
 *
 *   pss_row_meter_f64   float64 rows [n_rows][len], len >= 1 -> d_peak [n_rows] = np.max (a NaN in the row gives NaN; otherwise NumPy's
 *                       bits, except that a maximum of zero may carry either sign) and d_avg [n_rows] = np.mean on every bit (NumPy's
 *                       pairwise tree in 8192-element chunks added in order, / len).  Either output may be NULL, not both.  One pass
 *                       over the rows; rows of up to 2048 values one wavefront each, longer rows one workgroup.
 *   pss_squelch_gate    d_peak [n_frames] -> d_open uint8 [n_frames] (nullable), d_open_idx int32 [n_frames] (nullable): the open
 *                       frames' indices in ascending order, *n_open their number, *held_out the carry.  THIS CALL WAITS: the count has
 *                       to reach the host to size the demodulator's launches — one asynchronous 16-byte copy (count, carry) into pinned
 *                       memory and one synchronisation of the context's stream.  It cannot be captured into a graph.
 *   pss_h_squelch_gate  the same on host arrays, pure C, no context and no GPU (open nullable).
 *   pss_demod_gated     pss_demod_signal (dispatcher semantics: WFM frames IQ-corrected) on the n_open frames d_open_idx names, the
 *                       results written COMPACTED in frame order — d_pcm int16 [n_open][n_out][2], d_audio as pss_demod_signal's with
 *                       n_open rows: the concatenation the reference appends to audio_buffer.  Stream-ordered, no host wait: n_open
 *                       and the list as pss_squelch_gate left them, or any ascending list of the caller's (PSS_E_ARG for n_open
 *                       outside [0, n_frames]; indices outside the batch are clamped into it).  n_open = n_frames: the demodulator
 *                       reads d_iq itself, nothing is copied; n_open = 0: nothing is launched, the outputs stay untouched; otherwise
 *                       the open frames are gathered into context scratch (never more than the batch) in front of the demodulator
 *                       (16 bytes per lane; d_iq aligned to one sample, 8 bytes: PSS_E_ARG otherwise).
 *   pss_frame_pipeline_squelch   pss_frame_pipeline_cells' arguments and display results (d_db32, d_db64, extremes, lines: the same
 *                       kernels), then d_peak / d_avg [n_frames] of every frame's post-processed row, the gate (d_open, *n_open,
 *                       *held_out) and d_pcm [n_open][n_out][2] of the open frames.  The post-processed float64 rows are materialised
 *                       in context scratch for the meter (one HBM round trip more than pss_frame_pipeline_cells, and the demodulator
 *                       starts behind the display half instead of beside it).  Contains the gate, hence its wait: not capturable.
 * PSS_E_ARG: every < 0, phase outside [0, every) (every = 0: phase != 0), null buffers, len < 1, n_frames >= 2^31. */
int pss_row_meter_f64(pss_ctx *ctx, const double *d_rows, long n_rows, int len, double *d_peak, double *d_avg);
int pss_squelch_gate(pss_ctx *ctx, const double *d_peak, long n_frames, double squelch, int every, int phase, double held_in, uint8_t *d_open,
                     int32_t *d_open_idx, long *n_open, double *held_out);
int pss_h_squelch_gate(const double *peak, long n_frames, double squelch, int every, int phase, double held_in, uint8_t *open, long *n_open,
                       double *held_out);
int pss_demod_gated(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, const int32_t *d_open_idx, long n_open,
                    int16_t *d_pcm, double *d_audio);
int pss_frame_pipeline_squelch(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                               double *d_row_lo, double *d_row_hi, int n_halo, int window, int display, int disp_h, int disp_w,
                               int8_t *d_line_a, int8_t *d_line_b, int16_t *d_pcm, double squelch, int every, int phase, double held_in,
                               double *d_peak, double *d_avg, uint8_t *d_open, long *n_open, double *held_out);

/* Scanner sweep report.  Neither sweep classifies every slice: the inline sweep (pyspecsdr.py:2539-2561) and the sweep driver
 * (scan_frequencies, :1054-1068) both run
 *     if peak_power > threshold:  ...bandwidth...  if bandwidth > MIN_SIGNAL_BANDWIDTH (50e3):  signals.append({..., 'type': classify_signal(...)})
 * on the numbers pss_scan / pss_scan_threshold return, and only the slices that pass reach the classifier.  The rule, exactly:
 *     hit[i] = (d_peak[i] > (float)threshold_db) && (d_bw[i] > min_bw)
 * peak_power is an np.float32 and the threshold a Python float, a weak scalar under NEP 50, so NumPy compares in FLOAT32 against the threshold
 * rounded to float32: np.float32(-30.05) > -30.05 is False although the float32 value is the larger real number.  The bandwidth is float64,
 * np.sum(mask) * (fs / len), compared with the float64 min_bw.  A NaN on either side: no hit.
 *
 *   pss_scan_gate       d_peak float32 [n_slices], d_bw float64 [n_slices] -> d_hit uint8 [n_slices] (nullable), d_hit_idx int32 [n_slices]
 *                       (nullable): the detections' indices in ascending order, entries behind the *n_hit-th stay untouched.  No atomics:
 *                       ballot and popcount inside a wavefront, a prefix sum over the counts of tiles of 256 above it (the squelch gate's).
 *                       THIS CALL WAITS like pss_squelch_gate: one asynchronous 16-byte copy of the count into pinned memory and one
 *                       synchronisation of the context's stream.  It cannot be captured into a graph.
 *   pss_h_scan_gate     the same on host arrays, pure C, no context and no GPU: the rule one slice after the other (hit, hit_idx nullable).
 *   pss_classify_gated  pss_classify on the n_idx frames d_idx names, every output (each nullable) COMPACTED to n_idx rows in list order:
 *                       d_label / d_bw / d_mi / d_flat [n_idx], d_psd [n_idx][1024].  The frames are read where they lie — a driver read is
 *                       240 000 samples, 1.9 MB: nothing is gathered — by the classifier's own kernels, whose frame pointer and output row
 *                       come from the list (one __device__ body per kernel, instantiated for both): a listed frame's results are
 *                       pss_classify's bytes.  The scratch is sized by n_idx.  Stream-ordered, no host wait.  n_idx outside [0, n_frames]:
 *                       PSS_E_ARG; n_idx = 0: nothing is launched, the outputs stay untouched; n_idx = n_frames: pss_classify itself (the list
 *                       is taken to be 0 .. n_frames - 1 and not read); indices outside the batch are clamped into it.
 *   pss_sweep_report    one sweep in one call: scan -> gate -> pss_classify_gated.
 *                         kind = PSS_SWEEP_INLINE   pss_scan (the mask is peak - 20 dB, :2542-2552); threshold_db is the gate only
 *                         kind = PSS_SWEEP_DRIVER   pss_scan_threshold (the absolute mask, :1049-1057); threshold_db is the mask and the gate
 *                       d_db [n_slices][n] and d_count (nullable), d_peak, d_bw: the scan's outputs, byte for byte; d_hit (nullable), d_hit_idx,
 *                       *n_hit: the gate's; d_label, d_cls_bw, d_mi, d_flat (each nullable): caller-sized [n_slices], filled [*n_hit], the
 *                       classifier's results of the detections in slice order (d_cls_bw is estimate_bandwidth's figure, not d_bw).  Lengths:
 *                       whatever the chosen scan accepts.  Contains the gate, hence its wait: not capturable.
 *   pss_h_scan_dedupe   scan_frequencies' last step (:1084-1091) on host arrays, pure C: the records ordered by frequency (a stable sort: ties keep
 *                       input order), key = round(f / grid_hz) * grid_hz with Python's round (half to even on the double: nearbyint), the first
 *                       record of every key kept -> keep int32 [n]: the kept INPUT indices in sorted order, *n_keep their number.  The
 *                       reference's grid_hz is 100e3.  PSS_E_ARG: grid_hz <= 0 or a frequency that is not finite (round() raises there).
 * Hit indices are local to a call: a caller that shards a sweep offsets them.  Thresholds below -100 dB are outside the contract (an all-zero
 * slice, -100 dB, would then be classified).  PSS_E_ARG: n_slices outside [0, 2^31), null d_peak / d_bw / d_iq / d_hit_idx, unknown kind, fs <= 0. */
enum { PSS_SWEEP_INLINE = 0, PSS_SWEEP_DRIVER = 1 };
int pss_scan_gate(pss_ctx *ctx, const float *d_peak, const double *d_bw, long n_slices, double threshold_db, double min_bw, uint8_t *d_hit,
                  int32_t *d_hit_idx, long *n_hit);
int pss_h_scan_gate(const float *peak, const double *bw, long n_slices, double threshold_db, double min_bw, uint8_t *hit, int32_t *hit_idx,
                    long *n_hit);
int pss_classify_gated(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, const int32_t *d_idx, long n_idx, int32_t *d_label,
                       double *d_bw, float *d_mi, float *d_flat, float *d_psd);
int pss_sweep_report(pss_ctx *ctx, int kind, const float *d_iq, long n_slices, int n, double fs, double threshold_db, double min_bw, float *d_db,
                     float *d_peak, double *d_bw, int32_t *d_count, uint8_t *d_hit, int32_t *d_hit_idx, long *n_hit, int32_t *d_label,
                     double *d_cls_bw, float *d_mi, float *d_flat);
int pss_h_scan_dedupe(const double *freq, long n, double grid_hz, int32_t *keep, long *n_keep);

/* complex128 read buffers.  The reference's SDR buffer is complex64 (pyspecsdr.py:1887), but its functions accept any array, and handed
 * complex128 they compute in float64 from the first statement on.  These entry points serve compute_fft (signal_processing.py:243-264: the
 * window product is float64 x float64) and demodulate_am (:179-195: np.abs / np.mean / the subtraction in float64 — the same scaled hypot and
 * pairwise tree as the complex64 loops, one type wider) for such buffers: float64 dB rows to ~1e-10 of NumPy's, AM audio and int16 PCM bit
 * for bit (tests/golden/c128.npz).  Plain kernels — a conformance path for callers that hold float64 samples, not a throughput path.
 * The other demodulators narrow complex128 input to complex64 (np.angle on complex128 is libm's float64 atan2: not restated).
 *   d_iq / h_iq: interleaved float64 (re, im); n_fft a power of two in [16, 65536] (PSS_E_ARG otherwise); demodulate_am: any n >= 1
 *   pss_demod_am_c128: d_pcm int16 [n_frames][n][2] and / or d_audio float64 [n_frames][n] (mono); pss_h_*: one buffer, host pointers,
 *   h_audio_stereo float64 [n][2] */
int pss_spectrum_db_c128(pss_ctx *ctx, const double *d_iq, long n_frames, int n_fft, double *d_db);
int pss_demod_am_c128(pss_ctx *ctx, const double *d_iq, long n_frames, int n, int16_t *d_pcm, double *d_audio);
int pss_h_compute_fft_c128(pss_ctx *ctx, const double *h_iq, int n, double *h_db);
int pss_h_demodulate_am_c128(pss_ctx *ctx, const double *h_iq, int n, double *h_audio_stereo, int16_t *h_pcm);
/* demodulate_ssb (signal_processing.py:198-217) of complex128 frames: lfilter's complex128 convolution on the samples as they are (a complex64 buffer is
 * widened first by the reference: the same kernels behind a float64 loader), hilbert() round trip, normalisation, int16 (tests/golden/c128.npz keys
 * ssb_*: int16 equal; float64 audio bit for bit with option "hilbert_exact" = 1 at power-of-two lengths, to ~1e-15 otherwise — as for complex64). */
int pss_demod_ssb_c128(pss_ctx *ctx, int lower, const double *d_iq, long n_frames, int n, double fs, int16_t *d_pcm, double *d_audio);
int pss_h_demodulate_ssb_c128(pss_ctx *ctx, int lower, const double *h_iq, int n, double fs, double *h_audio_stereo, int16_t *h_pcm);
/* measure_signal_power (signal_processing.py:325-328) of complex128 frames, the ARRAY part: d_power[f] = np.mean(np.abs(x) ** 2) in float64 (np.abs's
 * scaled hypot, x * x, NumPy's pairwise sum, / n — tests/golden/c128.npz keys mp_*).  The scalar the reference finishes with,
 * 10 * log10(power + 1e-10), is left to the caller: it is NumPy's float64 log10 of ONE number (the Python shim applies NumPy's own, which gives the
 * reference's bits on the host it runs on: keys pw_*). */
int pss_mean_power_c128(pss_ctx *ctx, const double *d_iq, long n_frames, int n, double *d_power);
int pss_h_mean_power_c128(pss_ctx *ctx, const double *h_iq, int n, double *h_power);

/* Waterfall / persistence quantisers over a ring of post-processed rows (pyspecsdr.py:1342-1406,
 * :1512-1564).  d_rows float32 [n_rows][len], oldest first (n_rows <= 30 / <= 10).
 * d_glyph/d_colour int8 [disp_h][disp_w] (-1 = not drawn; persistence: 0 = empty). */
int pss_waterfall_cells(pss_ctx *ctx, const float *d_rows, int n_rows, int len, int disp_h, int disp_w,
                        int8_t *d_glyph, int8_t *d_colour);
int pss_persistence_cells(pss_ctx *ctx, const float *d_rows, int n_rows, int len, int disp_h, int disp_w,
                          int8_t *d_colour);
/* Spectrum display quantiser — draw_spectrogram (pyspecsdr.py:398-498), one independent post-processed dB row per display:
 * 20th-percentile noise floor, display range, clip + x**0.7, resample to disp_w columns, bar height and the glyph / colour
 * of every cell.  d_rows [n_rows][len]; d_glyph / d_colour int8 [n_rows][disp_h][disp_w]: glyph 0 '.', 1 '-', 2 '=',
 * 3 '#', 4 ' '; colour = curses pair number (1 = cleared cell); -1 where the column was not drawn (non-finite value).
 * d_range (nullable) double [n_rows][2] = (display_min, display_max), the dB range of the scale labels (:424-436). */
int pss_spectrogram_cells(pss_ctx *ctx, const float *d_rows, long n_rows, int len, int disp_h, int disp_w, int8_t *d_glyph,
                          int8_t *d_colour, double *d_range);
int pss_spectrogram_cells_f64(pss_ctx *ctx, const double *d_rows, long n_rows, int len, int disp_h, int disp_w,
                              int8_t *d_glyph, int8_t *d_colour, double *d_range);

/* The spectrum display in its compact per-column form ("spectrum bars") — draw_spectrogram (pyspecsdr.py:399-499), the view the reference starts
 * in (:167, :2054), for BATCHES of rows.  Every cell the reference draws in a column follows from two small integers, so that is what a batch
 * returns per row instead of pss_spectrogram_cells' two disp_h x disp_w grids (2 disp_w + 16 bytes per row instead of 2 disp_h disp_w + 16):
 *   d_height int8 [n_rows][disp_w]  min(int(value * disp_h), disp_h), the bar's height in cells (:458); -1: column not drawn (value not finite, :456)
 *   d_level  int8 [n_rows][disp_w]  3 if value > 0.8, 2 if value > 0.4, 1 if value > 0.2, else 0 (:476-491); -1 with d_height
 *   d_range  double [n_rows][2]     (display_min, display_max) as pss_spectrogram_cells returns it (:424-436); nullable
 * `value` is pss_spectrogram_cells' own: the two kernels call the same __device__ functions behind their selects (percentile _lerp, range,
 * clip + x**0.7 at the knots, np.interp), so the bars ARE that kernel's grid, column by column.
 *   pss_spectrum_bars[_f64]  rows [n_rows][len], len >= 1, 1 <= disp_h <= 127, disp_w >= 1.  Rows of up to 4092 values stay in registers as
 *                            order-preserving 64-bit keys (one wavefront per row up to 2048 values, four above); the 20th percentile's two
 *                            order statistics come from exact counts over the finite values, one pass over the rows.  Longer rows: the radix
 *                            select of pss_spectrogram_cells.  A row without a finite value (the reference raises ValueError there): every
 *                            column -1, range (NaN, NaN).  PSS_E_ARG: len < 1, disp_h outside [1, 127], disp_w < 1, n_rows < 0, null buffers.
 *   pss_bars_cells           the expansion to pss_spectrogram_cells' grids, d_glyph / d_colour int8 [n_rows][disp_h][disp_w]: above the bar
 *                            (4, 1); for y >= disp_h - height, rel = (y - (disp_h - height)) / height (:473) and level 3 -> (rel > 0.5 ? 3 : 2,
 *                            14), 2 -> (rel > 0.5 ? 2 : 1, 13), 1 -> (rel > 0.5 ? 1 : 0, 12), 0 -> rel > 0.7 ? (0, 11) : (4, 10); height -1:
 *                            (-1, -1).  PSS_E_ARG: disp_h outside [1, 127], disp_w < 1, n_rows < 0, null buffers.
 *   pss_h_bars_cells         the same on host arrays, pure C, no context and no GPU: a curses front end draws from the 2 disp_w bytes it
 *                            downloaded.  PSS_E_ARG also for a height above disp_h.
 *   pss_frame_pipeline_bars  one loop iteration per read buffer with this view: pss_frame_pipeline_cells' dB rows (d_db32 [n_frames][n], d_db64
 *                            nullable: the same bytes), the demodulator's PCM in any mode with the dispatcher's semantics (d_pcm NULL: the
 *                            display half alone), the bars and range of every frame's post-processed row.  The view has no history: no halo,
 *                            no window, no extremes.  d_post (nullable) receives the float64 post-processed rows [n_frames][n - 4] — what
 *                            pss_row_meter_f64 -> pss_squelch_gate -> pss_demod_gated take for the squelch beside this view; NULL: context
 *                            scratch.  n: a power of two in [16, 65536].  The demodulator runs on the main stream, the display chain on the
 *                            side stream; joined before the call returns.  PSS_E_ARG: unknown mode, n, disp_h outside [1, 127], disp_w < 1,
 *                            null d_iq / d_db32 / d_height / d_level.
 * Not reproduced: the reference redraws only every third iteration and clears the screen itself. */
int pss_spectrum_bars(pss_ctx *ctx, const float *d_rows, long n_rows, int len, int disp_h, int disp_w, int8_t *d_height, int8_t *d_level,
                      double *d_range);
int pss_spectrum_bars_f64(pss_ctx *ctx, const double *d_rows, long n_rows, int len, int disp_h, int disp_w, int8_t *d_height, int8_t *d_level,
                          double *d_range);
int pss_bars_cells(pss_ctx *ctx, const int8_t *d_height, const int8_t *d_level, long n_rows, int disp_h, int disp_w, int8_t *d_glyph,
                   int8_t *d_colour);
int pss_h_bars_cells(const int8_t *height, const int8_t *level, long n_rows, int disp_h, int disp_w, int8_t *glyph, int8_t *colour);
int pss_frame_pipeline_bars(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                            double *d_post, int disp_h, int disp_w, int8_t *d_height, int8_t *d_level, double *d_range, int16_t *d_pcm);

/* Gradient waterfall — draw_gradient_waterfall (pyspecsdr.py:1640-1716) over the same ring of rows: glyph = index into
 * ' ._-=+*#@' (0..8), colour index 0..5, -1 = not drawn.  d_glyph / d_colour int8 [disp_h][disp_w], disp_w = max_width - 10. */
int pss_gradient_cells(pss_ctx *ctx, const float *d_rows, int n_rows, int len, int disp_h, int disp_w, int8_t *d_glyph,
                       int8_t *d_colour);
int pss_gradient_cells_f64(pss_ctx *ctx, const double *d_rows, int n_rows, int len, int disp_h, int disp_w, int8_t *d_glyph,
                           int8_t *d_colour);
/* Surface plot — draw_surface_plot (pyspecsdr.py:1567-1616) of one row on the whole screen: d_colour int8 [max_h][max_w],
 * 0 = empty, else the curses pair 1..5 of the '#' drawn there. */
int pss_surface_cells(pss_ctx *ctx, const float *d_row, int len, int max_h, int max_w, int8_t *d_colour);
int pss_surface_cells_f64(pss_ctx *ctx, const double *d_row, int len, int max_h, int max_w, int8_t *d_colour);

/* Constellation display — draw_vector_display (pyspecsdr.py:1718-1752): d_grid int8 [max_h][max_w], 1 where the '.' of
 * one of the n IQ samples lands (float32 arithmetic as in the reference). */
int pss_vector_cells(pss_ctx *ctx, const float *d_iq, int n, int max_h, int max_w, int8_t *d_grid);

/* The surface plot in its compact per-column form ("surface magnitudes") — draw_surface_plot (pyspecsdr.py:1567-1616) for BATCHES of rows.  Every
 * '#' the reference draws from a column follows from magnitude = int(value * 20) (:1593) and the screen size, so that is what a batch returns
 * per row instead of pss_surface_cells' max_h x max_w grid (disp_w + 16 bytes per row; disp_w = max_w - 8, :1571):
 *   d_mag    int8 [n_rows][disp_w]  int(value * 20), 0 .. 20; -1: the resampled value is not finite, column not drawn (:1592)
 *   d_range  double [n_rows][2]     the row's finite (min_val, max_val) (:1575-1576), bit-equal to pss_row_extremes[_f64]'s pair (float32 rows:
 *                                   widened); nullable.  The scale labels follow from it (formats.surface_scale_labels).
 * `value` is pss_surface_cells' own: both kernels call one __device__ function for the normaliser ((row - min_val) / db_range per sample in
 * float64, db_range == 0 -> 1, THEN np.interp) and the magnitude, so the magnitudes ARE that kernel's, column by column.
 *   pss_surface_mags[_f64]   rows [n_rows][len].  The row's extremes and its columns come out of one kernel, many rows per launch: one wavefront per
 *                            row up to 1024 values, four up to 4092, the row parked in LDS (one read from HBM); longer rows are read twice.  No
 *                            atomics; the output does not depend on the schedule.  A row without a finite value (the reference raises ValueError
 *                            there): range (+inf, -inf), every column -1, as pss_surface_cells draws nothing.  PSS_E_ARG: len < 2, disp_w < 2
 *                            (max_w >= 10), n_rows < 0, null d_rows / d_mag.
 *   pss_mags_cells           the expansion to pss_surface_cells' grids, d_colour int8 [n_rows][max_h][max_w] (disp_w = max_w - 8 magnitudes per row):
 *                            cell (sy, sx) holds 1 + y % 5 of the LAST (x, y), x = 0 .. disp_w - 1 outer, y = 0 .. mag[x] - 1 inner (:1591-1601),
 *                            with sx = int(x - y cos45) + 8 and sy = int(max_h - 2 - y sin45), 0 <= sx < max_w, 2 <= sy < max_h - 1; 0 where none
 *                            hits.  Every cell finds its own winner (at most two y map to one sy): no atomics.  PSS_E_ARG: max_h < 4, max_w < 10,
 *                            n_rows < 0, null buffers.  A magnitude below -1 cannot come from pss_surface_mags and is not checked on the device.
 *   pss_h_mags_cells         the same on host arrays, pure C, no context and no GPU.  PSS_E_ARG also for a magnitude outside [-1, 127].
 *   pss_frame_pipeline_surface  one loop iteration per read buffer with this view (current_display_mode SURFACE): pss_frame_pipeline_bars' rows
 *                            (d_db32 [n_frames][n]; d_db64, d_post nullable: context scratch) and PCM (d_pcm NULL: the display half alone), with
 *                            pss_surface_mags_f64 of the post-processed rows (len n - 4) as the chain's last link.  n: a power of two in
 *                            [16, 65536], any of the five modes.  PSS_E_ARG: unknown mode, n, disp_w < 2, n_frames < 0, null d_iq / d_db32 / d_mag. */
int pss_surface_mags(pss_ctx *ctx, const float *d_rows, long n_rows, int len, int disp_w, int8_t *d_mag, double *d_range);
int pss_surface_mags_f64(pss_ctx *ctx, const double *d_rows, long n_rows, int len, int disp_w, int8_t *d_mag, double *d_range);
int pss_mags_cells(pss_ctx *ctx, const int8_t *d_mag, long n_rows, int max_h, int max_w, int8_t *d_colour);
int pss_h_mags_cells(const int8_t *mag, long n_rows, int max_h, int max_w, int8_t *colour);
int pss_frame_pipeline_surface(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                               double *d_post, int disp_w, int8_t *d_mag, double *d_range, int16_t *d_pcm);

/* The constellation in its compact form ("constellation masks") — draw_vector_display (pyspecsdr.py:1719-1752) for BATCHES of read buffers: one
 * bit per screen cell instead of pss_vector_cells' byte grid.
 *   d_mask   uint32 [n_frames][max_h][words], words = (max_w + 31) / 32: bit (x & 31) of word (x >> 5) of line y is set where a '.' lands at
 *            (y, x); the unused bits of a line's last word are 0.
 *   pss_vector_masks         d_iq complex64 [n_frames][n].  Per sample pss_vector_cells' arithmetic (one shared __device__ function: float32
 *                            products and sums, truncation toward zero; a coordinate that is not finite draws nothing — the reference raises
 *                            there and abandons the rest of the buffer).  The frame's mask is built in LDS (LDS atomic OR) and stored once:
 *                            one wavefront per frame up to 4096 samples where four masks fit in 64 KB, else one 512-thread workgroup per frame; no
 *                            global atomics, no per-frame memset.  n = 0: empty masks.  LIMIT: max_h * words <= 16384 (the mask in 64 KB of
 *                            LDS; 130 x 1100 takes 4550 words, 6 x 32 767 takes 6144).  PSS_E_ARG: max_h < 1, max_w < 1, a screen above that
 *                            limit, n < 0, n_frames < 0, null buffers.
 *   pss_masks_cells          the expansion to pss_vector_cells' grids, d_grid int8 [n_frames][max_h][max_w] (1 = '.').  PSS_E_ARG: max_h < 1,
 *                            max_w < 1, n_frames < 0, null buffers.
 *   pss_h_masks_cells        the same on host arrays, pure C, no context and no GPU.
 *   pss_frame_pipeline_vector  one loop iteration per read buffer with this view (current_display_mode VECTOR): pss_frame_pipeline_bars' rows and
 *                            PCM — the header's meter needs the rows in this view too — and the masks of the read buffers AS READ (the reference
 *                            hands `samples` to the view, not the corrected copy).  PSS_E_ARG: unknown mode, n, the screen rules above,
 *                            n_frames < 0, null d_iq / d_db32 / d_mask.
 * Not reproduced: the axes ('-' / '|', drawn before the dots) and draw_frequency_labels, which are host text. */
int pss_vector_masks(pss_ctx *ctx, const float *d_iq, long n_frames, int n, int max_h, int max_w, uint32_t *d_mask);
int pss_masks_cells(pss_ctx *ctx, const uint32_t *d_mask, long n_frames, int max_h, int max_w, int8_t *d_grid);
int pss_h_masks_cells(const uint32_t *mask, long n_frames, int max_h, int max_w, int8_t *grid);
int pss_frame_pipeline_vector(pss_ctx *ctx, int mode, const float *d_iq, long n_frames, int n, double fs, float *d_db32, double *d_db64,
                              double *d_post, int max_h, int max_w, uint32_t *d_mask, int16_t *d_pcm);

/* decode_morse, front half (decoders.py:149-165): envelope = |x| / max|x| in float32, 20 log10(envelope + 1e-10) > threshold,
 * and the indices of the rising / falling transitions of that mask (np.diff + np.where), i.e. the arrays rise_times /
 * fall_times the timing logic of decode_morse (:167 ff., stays in the reference's own decoders.py) starts from.
 * d_iq: interleaved complex64 [n_frames][n]; d_rise / d_fall: int32 [n_frames][cap], in increasing order; d_counts: int32
 * [n_frames][2] = the TRUE numbers of rises and falls (entries beyond cap are dropped).  threshold_db: any value — the mask is
 * float32(20 log10(envelope + 1e-10)) > float32(threshold_db) with NumPy's float32 log10 bit for bit (the reference calls it with -20,
 * pyspecsdr.py:573: that case is one comparison against a precomputed float32 cut). */
int pss_morse_edges(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double threshold_db, int cap, int32_t *d_rise,
                    int32_t *d_fall, int32_t *d_counts);
int pss_h_morse_edges(pss_ctx *ctx, const float *h_iq, int n, double threshold_db, int cap, int32_t *h_rise, int32_t *h_fall,
                      int *n_rise, int *n_fall);

/* The decoders' per-message halves (host side; no GPU work, no context): what decode_morse does with its rise / fall indices
 * (decoders.py:167-231) and what decode_aprs does with its bit stream (decode_ax25_frame + decode_aprs_payload, decoders.py:6-88).
 *   pss_h_morse_decode: rise / fall = the int32 sample indices pss_morse_edges / pss_h_morse_edges return.  Pulse lengths and gaps in
 *       seconds, two pulse classes (the reference: scipy.cluster.vq.kmeans(durations, 2) from random starting points; here the partition
 *       Lloyd's iteration leaves unchanged with the smallest mean distance, class means summed in observation order — the reference's
 *       centroids wherever its answer does not depend on its random draw, i.e. for every keyed signal), symbols, letter gaps (> 3 dots),
 *       word gaps (> 7 dots), ITU table ('?' for an unknown symbol).  text: NUL-terminated ASCII, returns its length (0: no pulse);
 *       timing3 = (dot, dash, mean gap) in seconds.  PSS_E_ARG: bad arguments, text_cap too small, edges that do not alternate.
 *   pss_h_ax25_frame: bits = one 0/1 value per byte.  First flag 01111110, bits up to the next flag with stuffed zeros dropped, bytes LSB
 *       first, "SOURCE>DEST:info" (addresses: 7-bit characters shifted down by one, stripped of white space).  Returns 1 and the packet
 *       in out (*out_len bytes = the characters' code points 0..255, not NUL-terminated: info may hold NULs), 0 when there is no frame of
 *       at least 14 bytes (the reference returns None), PSS_E_ARG on bad arguments or out_cap too small.
 *   pss_h_decode_morse / pss_h_decode_aprs: the whole decoders on one host buffer — edges / normalisation + AFSK bit slicer on the GPU, the
 *       functions above behind them.  h_audio is real float64 (np.real of a complex buffer is the caller's, decoders.py:122-123). */
int pss_h_morse_decode(const int32_t *rise, long n_rise, const int32_t *fall, long n_fall, double fs, char *text, long text_cap,
                       double *timing3);
int pss_h_ax25_frame(const uint8_t *bits, long n_bits, char *out, long out_cap, long *out_len);
int pss_h_decode_morse(pss_ctx *ctx, const float *h_iq, int n, double fs, double threshold_db, char *text, long text_cap, double *timing3);
int pss_h_decode_aprs(pss_ctx *ctx, const double *h_audio, int n, double fs, const double *sos1200, const double *sos2200, int nsec,
                      char *out, long out_cap, long *out_len);

/* ---- decoders for batches: the per-message halves above on the DEVICE, for every read buffer of a batch (pss_decode_dev.hip).  Device
 * pointers, the context's stream, no host wait.  n_frames / n_rows == 0: PSS_OK, nothing is launched.  PSS_E_ARG: negative sizes, fs not
 * above 0, null buffers.
 *   pss_morse_text   pss_h_morse_decode for every frame of a pss_morse_edges result (d_rise / d_fall int32 [n_frames][cap], d_counts int32
 *       [n_frames][2]).  d_text uint8 [n_frames][text_cap]: the text's bytes, zeros behind them; d_text_len int32 [n_frames]: the TRUE
 *       length (bytes past text_cap are dropped; a text has at most 2 bytes per pulse); d_timing float64 [n_frames][3] = (dot, dash, mean
 *       gap) in seconds — text, length and timing are the host function's, bit for bit: the class sums and the distance sum of every
 *       candidate split are added up in observation order, the mean gap over NumPy's pairwise tree.  d_pulses int32 [n_frames]: the number
 *       of complete pulses; 0 = the reference's early returns (empty text, timing zeros: its {"dot": 0, "dash": 0, "gap": 0}); -1 = a
 *       truncated edge list (a count above cap): no text, zeros; -2 = edges that do not alternate (the host function returns PSS_E_ARG, the
 *       reference raises; pss_morse_edges never produces them): no text, zeros.
 *   pss_ax25_frames  pss_h_ax25_frame for n_rows rows of n_bits bits (one 0/1 value per byte).  d_out_len int32 [n_rows]: -1 where the host
 *       function returns 0 (no packet), else the packet's TRUE length; d_out uint8 [n_rows][out_cap]: its bytes (code points 0..255, not
 *       NUL-terminated), bytes past out_cap dropped, bytes behind the packet not written.
 *   pss_real_normalise  decode_aprs's first lines for complex64 read buffers (decoders.py:121-125), d_iq interleaved [n_rows][n]: the real
 *       parts divided by their largest magnitude IN FLOAT32 (np.real of a complex64 buffer is float32; one correctly rounded division; a
 *       NaN propagates through the maximum; a row of zeros gives NaN), widened to float64 d_audio [n_rows][n].  The imaginary parts are
 *       not read.  (pss_row_normalise is the same for a buffer that is float64 already.)
 *   pss_decode_morse_batch  pss_morse_edges + pss_morse_text: decode_morse for every read buffer.  d_rise / d_fall / d_counts are work
 *       buffers of pss_morse_edges' shapes, returned filled.
 *   pss_decode_aprs_batch   pss_real_normalise + pss_afsk_bits + pss_ax25_frames: decode_aprs for every complex64 read buffer.  d_audio
 *       float64 [n_rows][n] and d_bits uint8 [n_rows][pss_afsk_n_bits(n, fs)] are work buffers, returned filled (the filtered rows of
 *       pss_afsk_bits live in the context's scratch, so the normalised audio is the caller's).  sos1200 / sos2200 / nsec: as pss_afsk_bits. */
int pss_morse_text(pss_ctx *ctx, const int32_t *d_rise, const int32_t *d_fall, const int32_t *d_counts, long n_frames, int cap, double fs,
                   int text_cap, uint8_t *d_text, int32_t *d_text_len, double *d_timing, int32_t *d_pulses);
int pss_ax25_frames(pss_ctx *ctx, const uint8_t *d_bits, long n_rows, int n_bits, int out_cap, uint8_t *d_out, int32_t *d_out_len);
int pss_real_normalise(pss_ctx *ctx, const float *d_iq, long n_rows, int n, double *d_audio);
int pss_decode_morse_batch(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, double threshold_db, int cap, int32_t *d_rise,
                           int32_t *d_fall, int32_t *d_counts, int text_cap, uint8_t *d_text, int32_t *d_text_len, double *d_timing,
                           int32_t *d_pulses);
int pss_decode_aprs_batch(pss_ctx *ctx, const float *d_iq, long n_rows, int n, double fs, const double *sos1200, const double *sos2200, int nsec,
                          double *d_audio, uint8_t *d_bits, int out_cap, uint8_t *d_out, int32_t *d_out_len);

/* classify_signal (signal_processing.py:296-322; helpers estimate_bandwidth :267-280, estimate_modulation_index :283-293) for
 * a batch of scanner reads, as the function runs once its missing `welch` import is supplied (in the reference it raises
 * NameError on every call: SURVEY App. C2, §8(f) #3).  d_iq: interleaved complex64 [n_frames][n], n >= 1.  n >= 1024: Welch
 * segments of 1024 samples every 512; shorter reads: ONE segment of n samples (SciPy's nperseg = n fallback: Hann window and
 * transform of length n, n PSD bins — the first n entries of a d_psd row).  n < 1: PSS_E_ARG (welch raises).  Outputs (each may be
 * NULL): d_label int32 [n_frames] (PSS_CLASS_*), d_bw float64 (the "bandwidth" of estimate_bandwidth: last minus first bin
 * above max - 20 dB in FFT order, in Hz), d_mi float32 (modulation index, bit-exact with NumPy's float32 evaluation),
 * d_flat float32 (spectral flatness), d_psd float32 [n_frames][1024] (Welch PSD, FFT order).  The segment FFT runs in
 * float64 (the reference's is single precision): PSD and flatness agree to the reference's own float32 FFT noise. */
enum { PSS_CLASS_UNKNOWN = 0, PSS_CLASS_FM_BROADCAST = 1, PSS_CLASS_NARROW_FM = 2, PSS_CLASS_AM_BROADCAST = 3, PSS_CLASS_SSB = 4,
       PSS_CLASS_DIGITAL = 5 };
int pss_classify(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, int32_t *d_label, double *d_bw, float *d_mi,
                 float *d_flat, float *d_psd);
const char *pss_class_name(int label);
/* One read buffer in host memory (what pyspecsdr.py:1061 / :2560 hand over), synchronous. */
int pss_h_classify_signal(pss_ctx *ctx, const float *h_iq, int n, double fs, int *label, double *bw, float *mi, float *flat);

/* Same quantisers over float64 rows (the reference's rows are float64; used to check cell-exact parity). */
int pss_waterfall_cells_f64(pss_ctx *ctx, const double *d_rows, int n_rows, int len, int disp_h, int disp_w,
                            int8_t *d_glyph, int8_t *d_colour);
int pss_persistence_cells_f64(pss_ctx *ctx, const double *d_rows, int n_rows, int len, int disp_h, int disp_w,
                              int8_t *d_colour);

/* Stateful accumulators: a device ring of the last max_rows post-processed rows, the counterpart of the reference's
 * WATERFALL_HISTORY (30 rows, pyspecsdr.py:130-131,1351-1353) and PERSISTENCE_HISTORY (10 rows, :151-152,1521-1523).
 * push = history.append(row) + pop(0) when full; the two quantisers then work on the ring in place. */
typedef struct pss_ring pss_ring;
int pss_ring_create(pss_ctx *ctx, int max_rows, int len, pss_ring **out);
void pss_ring_destroy(pss_ring *ring);
int pss_ring_push(pss_ring *ring, const float *d_row);
int pss_ring_count(pss_ring *ring);
int pss_ring_waterfall(pss_ring *ring, int disp_h, int disp_w, int8_t *d_glyph, int8_t *d_colour);
int pss_ring_persistence(pss_ring *ring, int disp_h, int disp_w, int8_t *d_colour);

/* Batched accumulators: the display line the reference would draw for EVERY frame of a batch, in one call.
 * draw_waterfall / draw_persistence (pyspecsdr.py:1342-1406, :1512-1564) append the frame's post-processed row to a history
 * of `window` rows (30 / 10) and normalise with the finite extremes of that history; for frame i of a batch that is the
 * sliding-window minimum / maximum of the per-row extremes over rows i-window+1 .. i.
 *   d_post            [n_frames][len]        the batch's post-processed rows
 *   d_row_lo/d_row_hi [n_halo + n_frames]    per-row finite extremes (pss_spectrum_post_extremes / pss_row_extremes); the
 *                                            first n_halo entries belong to the rows that PRECEDE the batch (the previous
 *                                            batch's tail, or the left neighbour's when frames are sharded over GPUs:
 *                                            8 bytes per row cross the link instead of the rows) — 0 for a fresh history
 *   waterfall:   d_glyph / d_colour int8 [n_frames][disp_w] = line y = 0 (the newest row) of the reference's grid at frame i
 *                (glyph 0 '.', 1 '-', 2 '=', 3 '#'; colour 0..5; -1 where the value is not finite)
 *   persistence: d_y int8 [n_frames][disp_w] = row index int((1 - norm) * (disp_h - 1)) of the newest trace's '*' in every
 *                column (-1: not drawn); disp_h <= 127. */
int pss_waterfall_rows(pss_ctx *ctx, const float *d_post, long n_frames, int len, const float *d_row_lo, const float *d_row_hi,
                       int n_halo, int window, int disp_w, int8_t *d_glyph, int8_t *d_colour);
int pss_waterfall_rows_f64(pss_ctx *ctx, const double *d_post, long n_frames, int len, const double *d_row_lo,
                           const double *d_row_hi, int n_halo, int window, int disp_w, int8_t *d_glyph, int8_t *d_colour);
int pss_persistence_rows(pss_ctx *ctx, const float *d_post, long n_frames, int len, const float *d_row_lo, const float *d_row_hi,
                         int n_halo, int window, int disp_h, int disp_w, int8_t *d_y);
int pss_persistence_rows_f64(pss_ctx *ctx, const double *d_post, long n_frames, int len, const double *d_row_lo,
                             const double *d_row_hi, int n_halo, int window, int disp_h, int disp_w, int8_t *d_y);
/* The gradient view as a line per frame — draw_gradient_waterfall (pyspecsdr.py:1640-1716) is the waterfall accumulator with another
 * quantiser (the same history of 30 rows, the same window extremes, np.interp to max_width - 10 columns = disp_w): pss_waterfall_rows'
 * arguments; d_glyph int8 [n_frames][disp_w] = int(norm * 8), the index into ' ._-=+*#@', d_colour = int(norm * 5), -1 where the resampled
 * value is not finite; norm = (v - lo) / range over the window's finite extremes with range == 0 -> 1 (:1657-1659: this view has the guard
 * the plain waterfall lacks).  PSS_E_ARG as for pss_waterfall_rows (len < 2, disp_w < 1, window < 1, n_halo < 0, null buffers). */
int pss_gradient_rows(pss_ctx *ctx, const float *d_post, long n_frames, int len, const float *d_row_lo, const float *d_row_hi,
                      int n_halo, int window, int disp_w, int8_t *d_glyph, int8_t *d_colour);
int pss_gradient_rows_f64(pss_ctx *ctx, const double *d_post, long n_frames, int len, const double *d_row_lo,
                          const double *d_row_hi, int n_halo, int window, int disp_w, int8_t *d_glyph, int8_t *d_colour);
/* The same WITHOUT materialised post-processed rows (float32 path; n_fft a multiple of 4, n_fft - 4 <= 32768).
 * pss_spectrum_post_thresholds: the post-process of pyspecsdr.py:2278-2283 reduced to what the accumulators need of every row —
 * d_row_thr float32 [n_frames] (the clamp threshold float32(median - 10)) and the finite extremes of the clamped row.
 * pss_waterfall_rows_db / pss_persistence_rows_db: the display lines from the dB rows [n_frames][n_fft] and those thresholds; element j
 * of a post-processed row is rebuilt where a cell needs it — float32(sum of 5 dB values * 0.2 in np.convolve's order) clamped at the
 * threshold, bit for bit what pss_spectrum_post writes — so the lines are byte-identical to pss_waterfall_rows on materialised rows. */
int pss_spectrum_post_thresholds(pss_ctx *ctx, const float *d_db, long n_frames, int n_fft, float *d_row_thr, float *d_row_lo,
                                 float *d_row_hi);
int pss_waterfall_rows_db(pss_ctx *ctx, const float *d_db, long n_frames, int n_fft, const float *d_row_thr, const float *d_row_lo,
                          const float *d_row_hi, int n_halo, int window, int disp_w, int8_t *d_glyph, int8_t *d_colour);
int pss_persistence_rows_db(pss_ctx *ctx, const float *d_db, long n_frames, int n_fft, const float *d_row_thr, const float *d_row_lo,
                            const float *d_row_hi, int n_halo, int window, int disp_h, int disp_w, int8_t *d_y);

/* ---- host-buffer convenience (single frame, synchronous; what the drop-in Python module calls) --- */
int pss_h_compute_fft(pss_ctx *ctx, const float *h_iq, int n, double *h_db);
int pss_h_demodulate(pss_ctx *ctx, int mode, const float *h_iq, int n, double fs, double *h_audio_stereo,
                     int16_t *h_pcm);
/* scipy.signal.sosfilt(sos, x) with zero initial state on n_rows independent float64 rows of n samples (one lane per row);
 * sos: HOST pointer, nsec <= 8 rows of 6.  The building block behind bandpass_filter (signal_processing.py:34-42). */
int pss_sosfilt(pss_ctx *ctx, const double *d_x, long n_rows, int n, const double *sos, int nsec, double *d_y);
/* scipy.signal.lfilter(b, a, x) with zero initial state on n_rows independent float64 rows of n samples (one lane per row) — what the
 * reference's lowpass_filter (signal_processing.py:28-31) runs with butter_lowpass's (b, a).  b, a: HOST tables of ncoef values each,
 * 2 <= ncoef <= 9, a[0] finite and not 0; both are divided by a[0] first, as lfilter does.  Direct form II transposed, unfused:
 * y = z[0] + b[0] x; z[k] = (z[k + 1] + x b[k + 1]) - y a[k + 1]; the last z = x b[N] - y a[N].  pss_h_lfilter: the same on host rows, pure
 * host code (no context, no GPU). */
int pss_lfilter(pss_ctx *ctx, const double *d_x, long n_rows, int n, const double *b, const double *a, int ncoef, double *d_y);
int pss_h_lfilter(const double *h_x, long n_rows, int n, const double *b, const double *a, int ncoef, double *h_y);

/* ---- FM mono: decode_mono (signal_processing.py:331-359), broadcast FM to mono int16 at fs / 6, bit for bit ----
 * Per frame of n complex64 samples: angle(x[i] * conj(x[i + 1])) in float32 (NumPy's FMA product and arctan2) times
 * float32(fs / (2 pi pi 75e3)); scipy.signal.decimate(., 6, ftype="fir") in float32 (firwin(121, 1 / 6) as float32, zero phase, one
 * multiply and one add per tap in upfirdn's order); the 75 us de-emphasis bilinear([1], [75e-6, 1], fs) — designed for the rate BEFORE
 * the decimation, as the reference does — run by lfilter in float64; minus np.mean; * 0.75 * 32768; astype(int16), which truncates to
 * int32 and keeps the low 16 bits (a full-deviation signal at 2.4 MS/s wraps; NaN, inf and values outside int32 give 0).
 * n_out = pss_decode_mono_len(n) = ceil((n - 1) / 6), 0 for n = 0 and 1 (n < 0: PSS_E_ARG).
 * pss_decode_mono: d_iq [n_frames][n] complex64 (8-byte aligned); d_pcm int16 [n_frames][n_out]; d_audio (optional) float64, the value
 * the cast sees; d_dec (optional) float32, the decimated row before the de-emphasis — at least one of the three.  Any n >= 0; n <= 1
 * succeeds and writes nothing.  Kernels k_mono_fwd (float32, to the decimated rows), k_mono_bwd (float64 recurrence and mean, one lane per
 * frame) and k_mono_out (scale and cast).
 * pss_h_decode_mono: one host frame, pure host code (no context, no GPU): the same statements (pss_mono.h) on one thread.
 * pss_design_deemph: scipy.signal.bilinear([1], [tau, 1], fs) -> b[2], a[2] (a[0] = 1), every bit. */
int pss_decode_mono_len(int n);
int pss_decode_mono(pss_ctx *ctx, const float *d_iq, long n_frames, int n, double fs, int16_t *d_pcm, double *d_audio, float *d_dec);
int pss_h_decode_mono(const float *h_iq, int n, double fs, int16_t *h_pcm, double *h_audio, float *h_dec);
int pss_design_deemph(double tau, double fs, double b[2], double a[2]);

/* ---- digital down-converter: K channels of one capture at fs / decim (mix, low-pass FIR, decimate) ----
 * What the reference asks its radio for (sdr.set_center_freq, sdr.sample_rate = ...) done to a capture.  The arithmetic is the project's
 * own, stated once in csrc/pss_ddc.h (PARITY.md "down-converter"); the device and the host twin agree on every bit.
 * pss_ddc_word: the 64-bit frequency word of offset_hz at fs, w = the integer nearest to (offset_hz / fs) 2^64 modulo 2^64, and the offset
 *   that results, w / 2^64 fs with w read as signed (effective_hz may be NULL).  PSS_E_ARG unless fs is finite and > 0 and |offset_hz| <= fs / 2.
 *   A signal at +offset_hz lands at 0 Hz.
 * pss_ddc_out_len: ceil(n_capture / decim); < 0 on n_capture < 0 or decim outside [1, 4096].
 * pss_ddc_default_taps: scipy.signal.decimate's own FIR, firwin(20 decim + 1, 1 / decim) through pss_design_firwin; decim = 1: the single
 *   tap 1.0.  decim in [1, 204] (at most 4097 taps); *n_taps is set, taps (room for 20 decim + 1 values; NULL: only the count) is filled.
 * pss_h_ddc_rotor: the oscillator alone, (c, s)[t] = exp(-2 pi i w (index0 + t) / 2^64), t < n; host code.
 * pss_ddc: d_iq complex64, 8-byte aligned, holds samples [buf_index0, buf_index0 + n_buf) of a capture of n_capture samples; the phase of
 *   a sample follows from its index in the CAPTURE, so any chunking of a capture gives the same bits.  words [n_chan], taps [n_taps]: HOST
 *   tables, as for pss_lfilter.  Output m of channel c, y[m] = sum over k of taps[k] z[m decim + lead - k] with z the mixed capture and zero
 *   outside [0, n_capture), goes to complex64 element c out_stride + (m - m_begin) of d_out (8-byte aligned) for m in [m_begin, m_end);
 *   elements between rows are not touched.  lead = 0: lfilter(taps, 1, z)[::decim]; lead = (n_taps - 1) / 2 with the default taps:
 *   scipy.signal.decimate(z, decim, ftype='fir', zero_phase=True).  Every sample of the capture that an output needs must lie in the
 *   buffer.  PSS_E_ARG (reason in pss_last_error): decim outside [1, 4096], n_taps outside [1, 4097], n_chan < 1, lead outside
 *   [0, n_taps - 1], a tap that is not finite, a null pointer, a buffer that is not inside the capture, [m_begin, m_end) outside
 *   [0, ceil(n_capture / decim)], out_stride < m_end - m_begin, a needed sample outside the buffer, a misaligned device pointer.  A
 *   refused call writes nothing.  One kernel, k_ddc (float64, mixer and FIR staged in LDS).
 * pss_h_ddc: the same on host buffers, pure host code (no context, no GPU; the reason of a refusal: pss_last_error(NULL)). */
int pss_ddc_word(double offset_hz, double fs, uint64_t *word, double *effective_hz);
long pss_ddc_out_len(long n_capture, int decim);
int pss_ddc_default_taps(int decim, double *taps, int *n_taps);
int pss_h_ddc_rotor(uint64_t word, long index0, long n, double *c, double *s);
int pss_ddc(pss_ctx *ctx, const float *d_iq, long n_buf, long buf_index0, long n_capture, const uint64_t *words, int n_chan, int decim,
            const double *taps, int n_taps, int lead, long m_begin, long m_end, float *d_out, long out_stride);
int pss_h_ddc(const float *h_iq, long n_buf, long buf_index0, long n_capture, const uint64_t *words, int n_chan, int decim,
              const double *taps, int n_taps, int lead, long m_begin, long m_end, float *h_out, long out_stride);
/* ---- polyphase channeliser: EVERY channel of a uniform grid of n_chan channels, fs / n_chan apart, of one capture at fs / decim ----
 * What the reference's scan_frequencies and band sweep step their tuner through, done to a capture in one pass.  Row c of the output is
 * the channel at c fs / n_chan for c < n_chan / 2 and at (c - n_chan) fs / n_chan otherwise (row n_chan / 2: the band edge); output m of
 * row c is y_c[m] = sum over k of taps[k] x[j] exp(-2 pi i c j / n_chan), j = m decim + lead - k, x zero outside [0, n_capture) — what
 * pss_ddc computes for the word c 2^64 / n_chan, evaluated as n_chan branch sums and one n_chan-point DFT per output instant.  The
 * arithmetic is the project's own, stated once in csrc/pss_pfb.h (PARITY.md "channeliser"); the device and the host twin agree on every
 * bit of every finite sample (the sign of a zero is not part of the contract).
 * pss_pfb_default_taps: firwin(20 n_chan + 1, 1 / n_chan) through pss_design_firwin; *n_taps is set, taps (room for 20 n_chan + 1
 *   values; NULL: only the count) is filled.  PSS_E_ARG unless n_chan is a power of two in [2, 1024].
 * pss_pfb: buffer and output conventions are pss_ddc's: d_iq complex64, 8-byte aligned, holds samples [buf_index0, buf_index0 + n_buf) of
 *   a capture of n_capture samples; the phase of a sample follows from its index in the CAPTURE, so any chunking of a capture gives the same
 *   bits.  taps [n_taps]: a HOST table, uploaded when its bytes differ from the last call's.  Output m of row c goes to complex64 element
 *   c out_stride + (m - m_begin) of d_out (8-byte aligned) for m in [m_begin, m_end); n_out = pss_ddc_out_len(n_capture, decim).  decim
 *   need not divide n_chan.  PSS_E_ARG (reason in pss_last_error): n_chan not a power of two in [2, 1024], decim outside [1, n_chan],
 *   n_taps outside [1, 32 n_chan], lead outside [0, n_taps - 1], a tap that is not finite, a null or misaligned pointer, a buffer that is
 *   not inside the capture, [m_begin, m_end) outside [0, n_out], out_stride < m_end - m_begin, a needed sample outside the buffer.  A
 *   refused call writes nothing.  One kernel, k_pfb (float64: chains in registers, DFT and transpose in LDS).
 * pss_h_pfb: the same on host buffers, pure host code (no context, no GPU; the reason of a refusal: pss_last_error(NULL)). */
int pss_pfb_default_taps(int n_chan, double *taps, int *n_taps);
int pss_pfb(pss_ctx *ctx, const float *d_iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim,
            const double *taps, int n_taps, int lead, long m_begin, long m_end, float *d_out, long out_stride);
int pss_h_pfb(const float *h_iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim,
              const double *taps, int n_taps, int lead, long m_begin, long m_end, float *h_out, long out_stride);
/* ---- channeliser for band plans: the same for every n_chan = 2^a 3^b 5^c in [2, 1024] (25 kHz, 12.5 kHz and 10 kHz grids at 2.4 and
 * 10 MS/s: 96, 192, 240, 400, 800, 1000 channels) — what the reference's memory-channel mode steps its tuner through, done to a capture.
 * Row c of the output is the channel at c fs / n_chan for c <= (n_chan - 1) / 2 and at (c - n_chan) fs / n_chan otherwise (odd n_chan
 * has no band-edge row); output m of row c is the sum pss_pfb states, evaluated as n_chan branch sums (pss_pfb's, with a true modulo for
 * the first tap) and one mixed-radix n_chan-point DFT per output instant: radix 5, 3 and 2 stages in that order, twiddles from a table of
 * n_chan entries.  The arithmetic is stated once in csrc/pss_bank.h (PARITY.md "channeliser for band plans"); the device and the host
 * twin agree on every bit of every finite sample (the sign of a zero is not part of the contract).
 * A power-of-two n_chan is DELEGATED: after the arguments have passed the checks below, all three calls hand it to pss_pfb_default_taps /
 * pss_pfb / pss_h_pfb, so its bytes are pss_pfb's by construction.
 * pss_bank_default_taps: firwin(20 n_chan + 1, 1 / n_chan) through pss_design_firwin; *n_taps is set, taps (room for 20 n_chan + 1
 *   values; NULL: only the count) is filled.  PSS_E_ARG unless n_chan = 2^a 3^b 5^c in [2, 1024].
 * pss_bank: the arguments, the buffer and output conventions and the refusals are pss_pfb's, with "n_chan not of the form 2^a 3^b 5^c in
 *   [2, 1024]" in place of the power-of-two rule: decim in [1, n_chan] (it need not divide n_chan), at most 32 n_chan taps.  The reason of
 *   a refusal starts with "pss_bank: "; a refused call writes nothing.  One kernel, k_bank (float64: chains in registers, DFT and
 *   transpose in LDS); the device copy of the tables (twiddles, taps, digit reversal) is kept on the context.
 * pss_h_bank: the same on host buffers, pure host code (no context, no GPU; the reason of a refusal: pss_last_error(NULL), "pss_h_bank: "). */
int pss_bank_default_taps(int n_chan, double *taps, int *n_taps);
int pss_bank(pss_ctx *ctx, const float *d_iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim,
             const double *taps, int n_taps, int lead, long m_begin, long m_end, float *d_out, long out_stride);
int pss_h_bank(const float *h_iq, long n_buf, long buf_index0, long n_capture, int n_chan, int decim,
               const double *taps, int n_taps, int lead, long m_begin, long m_end, float *h_out, long out_stride);
/* ---- rational resampler for batches of rows: scipy.signal.resample_poly(x, up, down) bit for bit — the step between a channel row at
 * fs / D (50 kS/s on a 12.5 kHz plan) and the rates the demodulators turn into exactly DEFAULT_SAMPLE_RATE audio.  up / down is reduced by
 * its gcd; both 1: a copy.  Output j of a row of n_in samples is upfirdn's: one IEEE multiply and one IEEE add per tap in ascending sample
 * order from +0, in the row's real type, the float64 table cast to that type and scaled by up in it.  The arithmetic is stated once in
 * csrc/pss_resample.h (PARITY.md "Resampler"); the device and the host twin agree on every byte.  complex64 rows: the contract with SciPy
 * covers finite samples (SciPy multiplies by h + 0i there); rows with inf / NaN never fault, their values are those of the statement.
 * pss_resample_out_len: ceil(n_in up / down) at the reduced factors; PSS_E_ARG (negative) unless 1 <= up, down <= 4096 and
 *   0 <= n_in <= 2^48.
 * pss_resample_default_taps: firwin(20 max(u, d) + 1, 1 / max(u, d), window=('kaiser', 5.0)) at the reduced factors u, d, in float64 (before
 *   the cast and the scaling by up), through the library's designer with Cephes' i0; u = d = 1: the one tap 1.0 (not used).  *n_taps is
 *   set, taps (NULL: only the count) is filled.
 * pss_resample: each of the n_rows rows is n_in samples long; the buffer d_x holds samples [buf_index0, buf_index0 + n_buf) of every row,
 *   x_stride elements apart.  Outputs [j_begin, j_end) of row r go to element r y_stride + (j - j_begin) of d_y; elements between rows are
 *   not touched.  An output's index arithmetic follows from its index in the ROW, so any chunking gives the same bytes.  taps: a HOST
 *   float64 low-pass table; the device copy of the plan's table is kept on the context and uploaded when its bytes differ from the last
 *   call's.  One kernel, k_resample (three instances).  n_rows = 0 or an empty window succeeds and writes nothing.
 *   PSS_E_ARG (reason in pss_last_error, starting "pss_resample: "; a refused call writes nothing): up or down outside [1, 4096];
 *   n_taps outside [1, 32 max(u, d) + 1]; a tap that is not finite; an unknown dtype; a null or misaligned pointer; a buffer not inside
 *   the row; [j_begin, j_end) outside [0, n_out]; a stride shorter than its window (x_stride < n_buf, y_stride < j_end - j_begin); a
 *   needed sample outside the buffer; n_in above 2^48.
 * pss_h_resample: the same on host buffers, pure host code (no context, no GPU; the reason of a refusal: pss_last_error(NULL),
 *   "pss_h_resample: "). */
#define PSS_RS_F32 0   /* float32 rows */
#define PSS_RS_F64 1   /* float64 rows */
#define PSS_RS_C64 2   /* complex64 rows (float32 pairs) */
long pss_resample_out_len(long n_in, int up, int down);
int pss_resample_default_taps(int up, int down, double *taps, int *n_taps);
int pss_resample(pss_ctx *ctx, const void *d_x, int dtype, long n_rows, long x_stride, long n_buf, long buf_index0, long n_in, int up, int down,
                 const double *taps, int n_taps, long j_begin, long j_end, void *d_y, long y_stride);
int pss_h_resample(const void *h_x, int dtype, long n_rows, long x_stride, long n_buf, long buf_index0, long n_in, int up, int down,
                   const double *taps, int n_taps, long j_begin, long j_end, void *h_y, long y_stride);
/* ---- survey of a capture: Welch's averaged periodogram and its max-hold row (scipy.signal.welch and spectrogram(mode='psd').max(-1) with
 * return_onesided=False, float64), the step in front of plan_bank / tune_recording: what is in this capture, and where.  n_rows rows of n
 * complex64 samples, row_stride samples apart (a capture is one row, the output of pss_bank M rows).  Segment s of a row covers samples
 * [s step, s step + nperseg): SciPy's noverlap = nperseg - step, L = (n - nperseg) / step + 1 segments, no padding, no partial segment.
 * Per segment, in float64: the samples widened exactly, minus the segment's own mean where detrend = 1 (SciPy's 'constant'), times win, the
 * nperseg-point DFT, p[k] = re^2 + im^2.  mean[row][k] = (sum over segments p[k] / L) scale, max[row][k] = (max over segments p[k]) scale
 * with np.max's rule (a NaN wins), bins in FFT order.  scale: 1 / (fs sum win^2) for SciPy's 'density', 1 / (sum win)^2 for 'spectrum'.
 * The sum over segments is a fixed tree of L alone (csrc/pss_welch.h states it with the rest of the arithmetic): the same call gives the
 * same bytes, row r of a batch the bytes of a one-row call on row r.  Against SciPy on the capture widened to complex128 every bin is
 * inside the derived bound of tests/welch_bounds.py (PARITY.md "Survey").  A row with a NaN sample in a used segment has no finite bin;
 * other rows are not touched by it.
 * pss_welch_segments: L (0 when n < nperseg); PSS_E_ARG (negative) for an nperseg or step outside the ranges below.
 * pss_welch_default_window: scipy.signal.get_window('hann', nperseg), the periodic Hann 0.5 - 0.5 cos(2 pi i / nperseg) evaluated in SciPy's
 *   order, into h_win.
 * pss_welch: d_iq, d_mean [n_rows][nperseg] and d_max (NULL: no max-hold row) are device pointers, h_win [nperseg] is a HOST table (its
 *   device copy is kept on the context and uploaded when its bytes differ from the last call's).  Two kernels, k_welch (one instance per
 *   nperseg, with and without the max row) and k_welch_fold; the block partials live in context-owned scratch.
 *   PSS_E_ARG (reason in pss_last_error, starting "pss_welch: "; a refused call writes nothing): nperseg not in {256, 512, 1024, 2048,
 *   4096}; step outside [1, nperseg]; n < nperseg; n_rows < 1; row_stride < n; a null window, mean or iq; a detrend outside {0, 1}; a scale
 *   that is not finite and positive; a device pointer not aligned to 8 bytes.
 * pss_h_welch: the same on host buffers, pure C++ (no context, no GPU; the reason of a refusal: pss_last_error(NULL), "pss_h_welch: ").
 *   Its transform is a radix-2 one: it agrees with the device within the same bound, not bit for bit. */
long pss_welch_segments(long n, int nperseg, int step);
int pss_welch_default_window(int nperseg, double *h_win);
int pss_welch(pss_ctx *ctx, const float *d_iq, long n_rows, long n, long row_stride, int nperseg, int step, const double *h_win, int detrend,
              double scale, double *d_mean, double *d_max);
int pss_h_welch(const float *iq, long n_rows, long n, long row_stride, int nperseg, int step, const double *win, int detrend, double scale,
                double *mean, double *max);
/* ---- RDS for broadcast FM: the station's groups (PI, name, RadioText) from rows of IQ — the hooks extract_rds / demodulate_rds_bpsk that the
 * reference's demodulate_wfm calls and never defines (signal_processing.py:165-174).  Four stages, the arithmetic of the three new ones
 * stated once in csrc/pss_rds.h (PARITY.md "RDS"); the device and the host twins agree on every byte, and every output follows from indices
 * in the ROW, never from how the row was cut.
 *   rows of IQ at fs --pss_rds_front--> rows at fs / decim --pss_resample (complex64)--> rows at 19 000 S/s (16 samples a bit)
 *   --pss_rds_bits--> the differentially decoded bits --pss_rds_groups--> the groups whose four blocks pass the check.
 * pss_rds_plan: decim = min(floor(fs / 19 000), 204) — pss_ddc_default_taps(decim) are then the front's default taps — and up / down =
 *   19 000 decim / fs reduced, the resampler's factors.  PSS_E_ARG (reason in pss_last_error(NULL), starting "pss_rds: "): an fs that is
 *   not an integer number of Hz, an fs at or below 120 000, reduced factors outside [1, 4096].
 * pss_rds_front: d_iq complex64, 8-byte aligned: n_rows rows x_stride samples apart, the buffer holding samples [buf_index0, buf_index0 +
 *   n_buf) of every row of n_capture samples.  Per sample i >= 1 the float32 polar discriminator d[i] = arctan2 of the float32 product
 *   x[i] conj(x[i - 1]) (NumPy's routine as pss_decode_mono models it; no gain; d[0] = 0), times pss_ddc's rotor at the word of 57 000 Hz
 *   and index i of the row, then pss_ddc's filter: output m of row r, y[m] = sum over k of taps[k] z[m decim + lead - k], z zero outside
 *   the row, goes to complex64 element r out_stride + (m - m_begin) of d_out for m in [m_begin, m_end).  taps: a HOST table (its device
 *   copy is kept on the context).  A sample's discriminator reads the sample before it: that one must lie in the buffer too.
 *   PSS_E_ARG (reason in pss_last_error, starting "pss_rds_front: "; a refused call writes nothing): fs not above 114 000, n_rows < 1,
 *   x_stride < n_buf, and pss_ddc's refusals for decim, n_taps, lead, the taps, the buffer, the window, out_stride and the alignment.
 *   One kernel, k_rds_front (discriminator and mixer once per sample into LDS, float64 tap loop from there).
 * pss_rds_default_pulse: the matched filter of the standard's biphase symbol at 16 samples a bit, 16 span_bits + 1 taps (span_bits in
 *   [1, 16]; the receiver's default is 4): two impulses of opposite sign half a bit apart shaped by cos(pi f t_d / 4), |f| <= 2 / t_d, in
 *   closed form.  *n_pulse is set, pulse (NULL: only the count) is filled.
 * pss_rds_bits: d_bb complex64 rows of n samples at 19 000 S/s, row_stride samples apart -> d_bits uint8 [n_rows][max_bits] and d_n_bits
 *   int32 [n_rows] (the true count; bits past max_bits are not stored).  Matched filter (pulse: a HOST table of an odd number of taps,
 *   at most 257), feed-forward symbol timing per segment of 64 bits smoothed over 9 segments, one fixed rule where the timing offset
 *   wraps, differential detection without carrier recovery.  Two kernels, k_rds_energy and k_rds_bits; scratch on the context.
 *   PSS_E_ARG ("pss_rds_bits: "): n_rows < 1, n or max_bits outside [0, 2^30], row_stride < n, a pulse that is not odd, in [1, 257] and
 *   finite, a null or misaligned pointer.
 * pss_rds_groups: d_bits [n_rows][max_bits] and d_n_bits as pss_rds_bits left them -> d_groups uint16 [n_rows][max_groups][4] (the four
 *   information words), d_pos int32 [n_rows][max_groups] (the bit index of the group's first bit), d_n_groups int32 [n_rows] (the true
 *   count; the first max_groups are kept), in ascending position.  A group is accepted where all four blocks pass the check as A, B,
 *   C or C' (by the version bit of block 2) and D; there is no error correction.  One kernel, k_rds_groups.  PSS_E_ARG
 *   ("pss_rds_groups: "): n_rows < 1, max_bits outside [0, 2^30], max_groups < 0, a null or misaligned pointer.
 * pss_h_rds_front / _bits / _groups: the same on host buffers, pure host code (no context, no GPU; the reason of a refusal:
 *   pss_last_error(NULL), starting with the twin's own name). */
int pss_rds_plan(double fs, int *decim, int *up, int *down);
int pss_rds_front(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_capture, double fs, int decim,
                  const double *taps, int n_taps, int lead, long m_begin, long m_end, float *d_out, long out_stride);
int pss_h_rds_front(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_capture, double fs, int decim,
                    const double *taps, int n_taps, int lead, long m_begin, long m_end, float *h_out, long out_stride);
int pss_rds_default_pulse(int span_bits, double *pulse, int *n_pulse);
int pss_rds_bits(pss_ctx *ctx, const float *d_bb, long n_rows, long row_stride, long n, const double *pulse, int n_pulse, uint8_t *d_bits,
                 long max_bits, int32_t *d_n_bits);
int pss_h_rds_bits(const float *h_bb, long n_rows, long row_stride, long n, const double *pulse, int n_pulse, uint8_t *h_bits, long max_bits,
                   int32_t *h_n_bits);
int pss_rds_groups(pss_ctx *ctx, const uint8_t *d_bits, const int32_t *d_n_bits, long n_rows, long max_bits, uint16_t *d_groups, int32_t *d_pos,
                   int max_groups, int32_t *d_n_groups);
int pss_h_rds_groups(const uint8_t *h_bits, const int32_t *h_n_bits, long n_rows, long max_bits, uint16_t *h_groups, int32_t *h_pos,
                     int max_groups, int32_t *h_n_groups);
/* ---- ADS-B: the Mode S frames of a 1090 MHz capture — what the reference's command list starts dump1090 for (rtlcoms.json, "Decode Aircraft
 * Transmissions").  The arithmetic is the project's own, stated once in csrc/pss_adsb.h (PARITY.md "ADS-B"); the device and the host twin
 * agree on every byte, and every output follows from indices in the CAPTURE, so no chunking changes one.
 * pss_adsb_plan: spc = fs / 2 000 000, the samples of a 0.5 us chip.  PSS_E_ARG (reason in pss_last_error(NULL), starting "pss_adsb: "): an fs
 *   for which that is no integer in [1, 8].
 * pss_adsb_crc: the 24-bit remainder of the first n_bits bits of msg (whole bytes; n_bits in [0, 112]) under the generator 0x1FFF409.  Pure
 *   host code.  A null msg or an n_bits outside that range: 0xFFFFFFFF.
 * pss_adsb_frames: d_iq complex64, 8-byte aligned, holding samples [buf_index0, buf_index0 + n_buf) of a capture of n_capture samples.  Every
 *   start s in [s_begin, s_end) is a candidate: magnitudes re re + im im, chip energies of spc samples, the 16-chip preamble (pulses at chips
 *   0, 2, 7, 9; the weakest pulse must exceed ratio times the strongest gap), 56 or 112 bits by comparing chip pairs, the remainder, and the
 *   format's rule: DF 17 / 18 with remainder 0, DF 11 with remainder below 128, DF 0 / 4 / 5 / 16 / 20 / 21 with the remainder in d_icao
 *   (n_icao ascending unique uint32 values below 2^24 ON THE DEVICE; the order is the caller's to keep).  Of accepted starts less than 2 spc
 *   apart that slice the same message, the one with the strongest weakest pulse stays (the earlier on a tie).  Records in ascending s:
 *   d_msg uint8 [max_frames][14] (a short frame zero-padded), d_pos int64 [max_frames] (the capture index of the preamble's first sample),
 *   d_meta uint32 [max_frames] (n_bits | DF << 16), d_score float32 [max_frames] (the weakest pulse's energy), d_count int32 [1] (the TRUE
 *   count; nothing is written past max_frames).  The buffer must hold what the window's starts and their possible suppressors read: the
 *   samples from max(0, s_begin - (2 spc - 1)) to min(n_capture, s_end + 2 spc - 2 + 240 spc).
 *   PSS_E_ARG (reason in pss_last_error, starting "pss_adsb_frames: "; a refused call writes nothing): spc outside [1, 8], a ratio that is
 *   negative or not finite, a buffer or a window outside the capture, s_end < s_begin, a window above 2^30 starts, a buffer that does not
 *   cover the window's reach, max_frames < 0, n_icao outside [0, 2^24], a null or misaligned pointer.
 *   Kernels: k_adsb_detect (the one pass over the capture), then k_starts_scan, k_starts_gather, k_adsb_keep, k_starts_scan, k_adsb_emit over the
 *   accepted starts only.  Scratch on the context, 2 bytes per start of the largest window it has been given, grow-only and freed by
 *   pss_destroy (a 2^30-start window keeps 2 GB), shared with pss_ais_frames; the call waits once for the count of accepted starts.
 * pss_h_adsb_frames: the same on host buffers, pure host code (no context, no GPU; the reason: pss_last_error(NULL)); it also refuses an
 *   address list that is not ascending, unique and below 2^24. */
int pss_adsb_plan(double fs, int *spc);
uint32_t pss_adsb_crc(const uint8_t *msg, int n_bits);
int pss_adsb_frames(pss_ctx *ctx, const float *d_iq, long n_buf, long buf_index0, long n_capture, int spc, float ratio, const uint32_t *d_icao,
                    int n_icao, long s_begin, long s_end, uint8_t *d_msg, int64_t *d_pos, uint32_t *d_meta, float *d_score, int32_t *d_count,
                    int max_frames);
int pss_h_adsb_frames(const float *h_iq, long n_buf, long buf_index0, long n_capture, int spc, float ratio, const uint32_t *h_icao, int n_icao,
                      long s_begin, long s_end, uint8_t *h_msg, int64_t *h_pos, uint32_t *h_meta, float *h_score, int32_t *h_count, int max_frames);
/* ---- AIS: the ship reports of a marine VHF capture — what the reference's command list starts `rtl_fm -M fm -s 48k | aisdecoder` for
 * (rtlcoms.json, "Receive AIS").  The arithmetic is the project's own, stated once in csrc/pss_ais.h (PARITY.md "AIS"); the device and the
 * host twins agree on every byte, and every output follows from indices in the ROW, so no chunking changes one.
 * pss_ais_plan: the route from a capture at fs to 48 000 S/s: decim = min(fs / 48 000, 204) for pss_ddc, up / down = 48 000 decim / fs reduced
 *   for pss_resample.  PSS_E_ARG (reason in pss_last_error(NULL), starting "pss_ais: "): an fs that is no integer, below 48 000, or whose
 *   factors leave [1, 4096].
 * pss_ais_default_pulse: the post-filter, a Gaussian of BT 0.4 at 5 samples a bit over span_bits bits (in [1, 12]; the receiver's default is
 *   2), 5 span_bits + 1 taps of sum 1 (an odd span_bits gives an even table, centred between two samples, which pss_ais_front does not
 *   take).  *n_pulse is set, pulse (NULL: only the count) is filled.
 * pss_ais_crc: the CRC-16/X.25 of n bytes (reflected 0x8408, init 0xFFFF, final complement: 0x906E for "123456789"; a frame with its two
 *   check bytes gives 0x0F47, the complement of the register's residue 0xF0B8).  Pure host code.  A null pointer or n < 0: 0xFFFFFFFF.
 * pss_ais_front: d_iq complex64 rows at 48 000 S/s, x_stride samples apart, 8-byte aligned, holding samples [buf_index0, buf_index0 + n_buf)
 *   of rows of n_row samples -> d_y float32, sample i of row r at element r * y_stride + (i - i_begin), i in [i_begin, i_end): the float32
 *   polar discriminator (no gain, d[0] = 0) and the post-filter (pulse: a HOST table of an odd number of taps, at most 65; one float64 fma
 *   chain per output, zero outside the row).  The buffer must hold the samples from max(0, i_begin - (P - 1) / 2 - 1) to
 *   min(n_row, i_end + (P - 1) / 2).  One kernel, k_ais_front.  It reads no rate: rows at any rate go through it with a pulse for that rate
 *   (the POCSAG receiver below feeds it rows at 38 400 S/s and a boxcar).
 *   PSS_E_ARG ("pss_ais_front: "; a refused call writes nothing): n_rows < 1, a buffer or a window outside the row, strides below n_buf or
 *   the window, a window above 2^30 samples, a pulse that is not odd, in [1, 65] and finite, a buffer that does not cover the window's
 *   halo, a null or misaligned pointer.
 * pss_ais_frames: d_y float32 rows at 48 000 S/s (pss_ais_front's, or any FM discriminator's), y_stride samples apart, 4-byte aligned,
 *   holding samples [buf_index0, buf_index0 + n_buf) of rows of n_row samples.  Every start s in [s_begin, s_end) of every row is a candidate:
 *   strobes 5 samples apart, a threshold from the eight strobes before the flag, NRZI, the training sequence and the flag, then the HDLC
 *   walk with bit unstuffing to the closing flag and the CRC-16.  Of accepted starts less than 5 apart in a row that read the same bytes,
 *   the one whose nearest strobe lies farthest from the threshold stays (the earlier on a tie).  Records in ascending (row, s): d_msg uint8
 *   [max_frames][128] (zero-padded; byte j holds bits 8 j .. 8 j + 7, the first received the least significant), d_len int32 (bytes, the
 *   two check bytes included), d_row int32, d_pos int64 (the row index of the flag's first strobe), d_score float32 (that distance),
 *   d_count int32 [1] (the TRUE count; nothing is written past max_frames).  The buffer must hold the samples from
 *   max(0, s_begin - 4 - 45) to min(n_row, s_end + 3 + 6221).
 *   PSS_E_ARG ("pss_ais_frames: "; a refused call writes nothing): n_rows outside [1, 2^20], a buffer or a window outside the row,
 *   y_stride < n_buf, s_end < s_begin, a window above 2^30 starts (2^31 over all rows), a buffer that does not cover the window's reach,
 *   max_frames < 0, a null or misaligned pointer.
 *   Kernels: k_ais_detect (the one pass over every start), then k_starts_scan, k_starts_gather, k_ais_walk, k_ais_keep, k_starts_scan,
 *   k_ais_emit over the survivors of the flag test only.  Scratch on the context (the same buffers as pss_adsb_frames' above), 2 bytes per start of the largest call and 149 bytes per survivor,
 *   grow-only and freed by pss_destroy; the call waits once for the count of survivors.
 * pss_h_ais_front / pss_h_ais_frames: the same on host buffers, pure host code (no context, no GPU; the reason: pss_last_error(NULL),
 *   pss_h_ais_front's starting with its own name, pss_h_ais_frames' with "pss_ais_frames: "). */
int pss_ais_plan(double fs, int *decim, int *up, int *down);
int pss_ais_default_pulse(int span_bits, double *pulse, int *n_pulse);
uint32_t pss_ais_crc(const uint8_t *bytes, long n);
int pss_ais_front(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *pulse,
                  int n_pulse, long i_begin, long i_end, float *d_y, long y_stride);
int pss_h_ais_front(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *pulse, int n_pulse,
                    long i_begin, long i_end, float *h_y, long y_stride);
int pss_ais_frames(pss_ctx *ctx, const float *d_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                   uint8_t *d_msg, int32_t *d_len, int32_t *d_row, int64_t *d_pos, float *d_score, int32_t *d_count, int max_frames);
int pss_h_ais_frames(const float *h_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                     uint8_t *h_msg, int32_t *h_len, int32_t *h_row, int64_t *h_pos, float *h_score, int32_t *h_count, int max_frames);
/* ---- POCSAG: the pager messages of a VHF capture — what the reference's command list starts `rtl_fm ... | multimon-ng -a POCSAG1200` for
 * (rtlcoms.json, "Decode Pager"; "Monitor Pager traffic" is FLEX, below).  The arithmetic is the project's own, stated once in csrc/pss_pocsag.h (PARITY.md
 * "POCSAG"); the device and the host twin agree on every byte, and every output follows from indices in the ROW, so no chunking changes one.
 * The rows run at 38 400 S/s: spb = 75, 32 and 16 samples a bit at 512, 1200 and 2400 bit/s.  The front is pss_ais_front above (it reads no
 * rate) with pss_pocsag_default_pulse's boxcar.
 * pss_pocsag_plan: the route from a capture at fs to 38 400 S/s: decim = min(fs / 38 400, 204) for pss_ddc, up / down = 38 400 decim / fs
 *   reduced for pss_resample.  PSS_E_ARG (reason in pss_last_error(NULL), starting "pss_pocsag: "): an fs that is no integer, below 38 400,
 *   or whose factors leave [1, 4096].
 * pss_pocsag_default_pulse: the post-filter of a rate of spb samples a bit (in [2, 128]): P = the largest odd number <= min(spb, 65) taps
 *   of 1.0 / P.  *n_pulse is set, pulse (NULL: only the count) is filled.
 * pss_pocsag_codeword: the 32-bit codeword of 21 data bits (bits above them ignored): the data in bits 31 .. 11, the BCH(31,21) check bits
 *   of the generator 0x769 in 10 .. 1, even parity in bit 0.  0x7CD215D8 >> 11 gives the sync word, 0x7A89C197 >> 11 the idle word.  Host only.
 * pss_pocsag_check: the receiver's check of one codeword: the bits fixed (0, 1 or 2, at most fix, in [0, 2]) with the corrected codeword in
 *   *fixed (nullable), or -1 with 0 there: uncorrectable.  Errors of weight 1 and 2 in bits 31 .. 1 by their syndrome, bit 0 by the parity.
 *   Host only.
 * pss_pocsag_batches: d_y float32 rows at 38 400 S/s, y_stride samples apart, 4-byte aligned, holding samples [buf_index0, buf_index0 +
 *   n_buf) of rows of n_row samples.  Every start s in [s_begin, s_end) of every row with s + 543 spb < n_row is a candidate: strobes spb
 *   samples apart, a threshold from the mean of the sync word's own 32 strobes, at most sync_errors (in [0, 2]) mismatches against
 *   0x7CD215D8 or its complement (an inverted channel), then the batch's 16 codewords through the check above with the caller's fix; a
 *   batch with more than max_bad (in [0, 16]) uncorrectable codewords is rejected.  Of accepted starts less than spb apart in a row that
 *   read the same 16 codewords, the one whose nearest sync strobe lies farthest from the threshold stays (the earlier on a tie).  Records
 *   in ascending (row, s): d_cw uint32 [max_batches][16] (corrected; 0 where uncorrectable), d_fix uint8 [max_batches][16] (0, 1, 2, or 255),
 *   d_row int32, d_pos int64 (the row index of the sync word's first strobe), d_meta uint32 (sync mismatches | inverted << 8 | n_bad << 16 |
 *   total fixed bits << 24), d_score float32 (that distance), d_count int32 [1] (the TRUE count; nothing is written past max_batches).  The
 *   buffer must hold the samples from max(0, s_begin - (spb - 1)) to min(n_row, s_end + spb - 2 + 543 spb + 1).
 *   PSS_E_ARG ("pss_pocsag_batches: "; a refused call writes nothing): n_rows outside [1, 2^20], spb, sync_errors, fix or max_bad outside
 *   their ranges, a buffer or a window outside the row, y_stride < n_buf, s_end < s_begin, a window above 2^30 starts (2^31 over all rows),
 *   a buffer that does not cover the window's reach, max_batches < 0, a null or misaligned pointer.
 *   Kernels: k_pocsag_detect (the one pass over every start), then k_starts_scan, k_starts_gather, k_pocsag_walk, k_pocsag_keep,
 *   k_starts_scan, k_pocsag_emit over the survivors of the sync test only (about spb of them per batch).  Scratch on the context (the same
 *   buffers as pss_adsb_frames' and pss_ais_frames'), 2 bytes per start of the largest call and 102 bytes per survivor, grow-only and freed
 *   by pss_destroy; the call waits once for the count of survivors.
 * pss_h_pocsag_batches: the same on host buffers, pure host code (no context, no GPU; the reason: pss_last_error(NULL), starting
 *   "pss_pocsag_batches: "). */
int pss_pocsag_plan(double fs, int *decim, int *up, int *down);
int pss_pocsag_default_pulse(int spb, double *pulse, int *n_pulse);
uint32_t pss_pocsag_codeword(uint32_t data21);
int pss_pocsag_check(uint32_t cw, int fix, uint32_t *fixed);
int pss_pocsag_batches(pss_ctx *ctx, const float *d_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                       int spb, int sync_errors, int fix, int max_bad, uint32_t *d_cw, uint8_t *d_fix, int32_t *d_row, int64_t *d_pos, uint32_t *d_meta,
                       float *d_score, int32_t *d_count, int max_batches);
int pss_h_pocsag_batches(const float *h_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, int spb,
                         int sync_errors, int fix, int max_bad, uint32_t *h_cw, uint8_t *h_fix, int32_t *h_row, int64_t *h_pos, uint32_t *h_meta,
                         float *h_score, int32_t *h_count, int max_batches);
/* ---- FLEX: the other pager protocol — what the reference's command list starts `rtl_fm ... | multimon-ng -a FLEX` for (rtlcoms.json,
 * "Monitor Pager traffic (Def. 138M)").  Two- and four-level FSK at 1600 and 3200 baud, a mode word in the frame's own sync, 11 interleaved
 * blocks of up to four multiplexed phases.  The arithmetic is the project's own, stated once in csrc/pss_flex.h (PARITY.md "FLEX"); the
 * air-interface constants there are the published ones written from memory and HAVE NOT BEEN CHECKED AGAINST A TRANSMITTER.  The device and
 * the host twin agree on every byte, and every output follows from indices in the ROW.  The rows are pss_pocsag_plan's at 38 400 S/s: h = 12
 * samples a 3200-baud symbol; the front is pss_ais_front with pss_flex_default_pulse's boxcar, one pass for both baud rates.
 * pss_flex_default_pulse: the post-filter for h samples a 3200-baud symbol (in [1, 64]): P = the largest odd number <= h taps of 1.0 / P.
 * pss_flex_word: the 32-bit word of 21 data bits: the data in bits 0 .. 20, the BCH(31,21) check bits in 21 .. 30, even parity in bit 31: a
 *   POCSAG codeword bit-reversed.  Host only.
 * pss_flex_frames: dev_y float32 rows, y_stride samples apart, 4-byte aligned, holding samples [buf_index0, buf_index0 + n_buf) of rows of
 *   n_row samples.  Every start s in [s_begin, s_end) of every row with s + 5936 h <= n_row is a candidate: 64 sync bits 2 h apart, each the
 *   sum of two samples h apart, sliced at their own mean; at most sync_errors (in [0, 3]) mismatches of the marker 0xA6C6AAAA in either
 *   polarity, of the outer code against its complement, and of the outer code against the nearest of the five mode codes; the frame
 *   information word through the BCH check with the caller's fix (in [0, 2]) and its nibble sum; of accepted starts less than 2 h apart the
 *   one with the fewest mismatches plus FIW fixed bits stays (then the larger mean distance from the threshold, then the earlier); its 11
 *   blocks are sliced at thresholds from the sync's mean and mean distance (four levels: +- 2/3 of it), de-interleaved into the phases A .. D,
 *   88 words each, every word through the check; a frame with more than max_bad (in [0, 352]) uncorrectable words leaves no record.
 *   Records in ascending (row, s): dev_words uint32 [max_frames][4][88] (corrected; 0 where uncorrectable and in unused phases), dev_fix uint8
 *   [max_frames][4][88] (0, 1, 2 or 255), dev_fiw uint32, dev_row int32, dev_pos int64, dev_meta uint32 [max_frames][2] (mismatches | inverted << 8 |
 *   mode << 12 | FIW fixed bits << 16; n_bad | total fixed bits << 16), dev_score float32 (the mean distance), dev_count int32 [1] (the TRUE
 *   count; nothing is written past max_frames).  The buffer must hold the samples from max(0, s_begin - (2 h - 1)) to min(n_row, s_end +
 *   2 h - 2 + 5936 h).
 *   PSS_E_ARG ("pss_flex_frames: "; a refused call writes nothing): n_rows outside [1, 2^20], h, sync_errors, fix or max_bad outside their
 *   ranges, a buffer or a window outside the row, y_stride < n_buf, s_end < s_begin, a window above 2^30 starts (2^31 over all rows), a
 *   buffer that does not cover the window's reach, max_frames < 0, a null or misaligned pointer.
 *   Kernels: k_flex_detect (the one pass over every start), then k_starts_scan, k_starts_gather, k_flex_head, k_flex_keep, k_flex_walk (a
 *   workgroup per kept start), k_starts_scan, k_flex_compact.  Scratch on the context (the start list's buffers), 2 bytes per start of the
 *   largest call and 1796 bytes per survivor, grow-only and freed by pss_destroy; the call waits once for the count of survivors.
 * pss_h_flex_frames: the same on host buffers, pure host code (no context, no GPU; the reason: pss_last_error(NULL), starting
 *   "pss_flex_frames: "). */
int pss_flex_default_pulse(int h, double *pulse, int *n_pulse);
uint32_t pss_flex_word(uint32_t data21);
int pss_flex_frames(pss_ctx *ctx, const float *dev_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                    int h, int sync_errors, int fix, int max_bad, uint32_t *dev_words, uint8_t *dev_fix, uint32_t *dev_fiw, int32_t *dev_row, int64_t *dev_pos,
                    uint32_t *dev_meta, float *dev_score, int32_t *dev_count, int max_frames);
int pss_h_flex_frames(const float *h_y, long n_rows, long y_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, int h,
                      int sync_errors, int fix, int max_bad, uint32_t *h_words, uint8_t *h_fix, uint32_t *h_fiw, int32_t *h_row, int64_t *h_pos,
                      uint32_t *h_meta, float *h_score, int32_t *h_count, int max_frames);
/* ---- NOAA APT: the weather-satellite image of a 137 MHz capture — what the reference's command list starts `rtl_fm -f 137.62M -M fm -s 60k ...
 * | sox ... && wxtoimg` for (rtlcoms.json, "Capture NOAA in .wav"; the band is pyspecconst.py's NOAA_SAT preset).  The arithmetic is the
 * project's own, stated once in csrc/pss_apt.h (PARITY.md "APT"); the device and the host twins agree on every byte, and every output follows
 * from indices in the ROW, so windows of a row concatenate to the whole row's bytes.  The rows run at 62 400 S/s (15 samples a word, 26 a
 * cycle of the 2400 Hz subcarrier), the envelope at 12 480 S/s (3 samples a word, 6240 a line of 2080 words).
 *   rows of IQ at 62 400 S/s --pss_apt_front--> the envelope --pss_apt_syncs--> the line starts found; the caller fits a grid through them
 *   (formats.apt_grid) --pss_apt_lines--> float32 [n_lines][2080] words.
 * pss_apt_plan: the route from a capture at fs to 62 400 S/s: decim = min(fs / 62 400, 204) for pss_ddc, up / down = 62 400 decim / fs
 *   reduced for pss_resample.  PSS_E_ARG (reason in pss_last_error(NULL), starting "pss_apt: "): an fs that is no integer, below 62 400, or
 *   whose factors leave [1, 4096].
 * pss_apt_default_taps: the front's low-pass, scipy.signal.firwin(79, 1 / 15) bit for bit: 2080 Hz at 62 400 S/s.  *n_taps is set (79),
 *   taps (NULL: only the count) is filled.
 * pss_apt_front: d_iq complex64, 8-byte aligned: n_rows rows x_stride samples apart, the buffer holding samples [buf_index0, buf_index0 +
 *   n_buf) of every row of n_row samples.  Per sample i >= 1 the float32 polar discriminator of pss_rds_front (no gain; d[0] = 0), times
 *   pss_ddc's rotor at the word of 2400 Hz and index i of the row, then pss_ddc's filter in float64, y[m] = sum over k of taps[k]
 *   z[m decim + lead - k], z zero outside the row, and the magnitude: env[m] = (float) sqrt(fma(re, re, im im)) goes to float32 element
 *   r env_stride + (m - m_begin) of d_env (4-byte aligned) for m in [m_begin, m_end).  The complex baseband is never stored.  taps: a HOST
 *   table (its device copy is kept on the context).  The receiver passes fs = 62 400 and decim = 5.
 *   PSS_E_ARG (reason in pss_last_error, starting "pss_apt_front: "; a refused call writes nothing): fs not above 4800, n_rows < 1,
 *   x_stride < n_buf, and pss_ddc's refusals for decim, n_taps, lead, the taps, the buffer, the window, env_stride and the alignment.
 *   One kernel, k_apt_front (discriminator and mixer once per sample into LDS, float64 tap loop from there, one float32 store an output).
 * pss_apt_syncs: d_env float32 rows e_stride samples apart, 4-byte aligned, holding samples [buf_index0, buf_index0 + n_buf) of rows of n_row
 *   envelope samples.  Every start s in [s_begin, s_end) of every row with s + 116 < n_row is a candidate: strobes e[k] = env[s + 3 k + 1],
 *   k = 0 .. 38; a threshold from the mean of e[4 .. 31], the pulse train's own 14 high and 14 low words; at most sync_errors (in [0, 4]) of
 *   the 39 bits e[k] > thr differ from sync A (000011001100110011001100110011000000000).  A NaN strobe compares false; a NaN or infinite
 *   threshold leaves 14 mismatches, never accepted.  score = (the sum of the 14 high strobes - the sum of the 14 low ones) / 14.  Of accepted
 *   starts less than 3120 apart in a row, the one with the fewest mismatches stays, then the highest score, then the earliest.  Records in
 *   ascending (row, s): d_row int32, d_pos int64 (the first envelope sample of sync A's first word), d_meta uint32 (the mismatches),
 *   d_score float32, d_count int32 [1] (the TRUE count; nothing is written past max_syncs).  The buffer must hold the samples from
 *   max(0, s_begin - 3119) to min(n_row, s_end + 3118 + 117); starts outside the window still count as neighbours.
 *   PSS_E_ARG ("pss_apt_syncs: "; a refused call writes nothing): n_rows outside [1, 2^20], sync_errors outside [0, 4], a buffer or a window
 *   outside the row, e_stride < n_buf, s_end < s_begin, a window above 2^30 starts (2^31 over all rows), a buffer that does not cover the
 *   window's reach, max_syncs < 0, a null or misaligned pointer.
 *   Kernels: k_apt_detect (the one pass over every start), then k_starts_scan, k_starts_gather, k_apt_score, k_apt_keep, k_starts_scan,
 *   k_apt_emit over the survivors of the sync test only (two or three per line).  Scratch on the context (the same buffers as
 *   pss_adsb_frames', pss_ais_frames' and pss_pocsag_batches'), 2 bytes per start of the largest call and 18 bytes per survivor, grow-only
 *   and freed by pss_destroy; the call waits once for the count of survivors.
 * pss_apt_lines: d_env float32 [n_rows] rows of n_row samples, e_stride apart; line l is cut at d_line_pos[l] (int64, ANY value: the caller
 *   may ask for lines whose sync was not found) of row d_line_row[l] (int32): d_words float32 element l words_stride + j = env[p + 3 j + 1],
 *   j = 0 .. 2079, +0 where that sample lies outside the row and for a row index outside [0, n_rows).  One kernel, k_apt_lines (a workgroup
 *   a line).  PSS_E_ARG ("pss_apt_lines: "; a refused call writes nothing): n_rows outside [1, 2^20], n_row outside [0, 2^60],
 *   e_stride < n_row, n_lines outside [0, 2^24], words_stride < 2080, a null or misaligned pointer.
 * pss_h_apt_front / _syncs / _lines: the same on host buffers, pure host code (no context, no GPU; the reason: pss_last_error(NULL),
 *   pss_h_apt_front's starting with its own name, the others' with "pss_apt_syncs: " and "pss_apt_lines: "). */
int pss_apt_plan(double fs, int *decim, int *up, int *down);
int pss_apt_default_taps(double *taps, int *n_taps);
int pss_apt_front(pss_ctx *ctx, const float *d_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, double fs, int decim,
                  const double *taps, int n_taps, int lead, long m_begin, long m_end, float *d_env, long env_stride);
int pss_h_apt_front(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, double fs, int decim,
                    const double *taps, int n_taps, int lead, long m_begin, long m_end, float *h_env, long env_stride);
int pss_apt_syncs(pss_ctx *ctx, const float *d_env, long n_rows, long e_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                  int sync_errors, int32_t *d_row, int64_t *d_pos, uint32_t *d_meta, float *d_score, int32_t *d_count, int max_syncs);
int pss_h_apt_syncs(const float *h_env, long n_rows, long e_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                    int sync_errors, int32_t *h_row, int64_t *h_pos, uint32_t *h_meta, float *h_score, int32_t *h_count, int max_syncs);
int pss_apt_lines(pss_ctx *ctx, const float *d_env, long n_rows, long e_stride, long n_row, const int32_t *d_line_row, const int64_t *d_line_pos,
                  long n_lines, float *d_words, long words_stride);
int pss_h_apt_lines(const float *h_env, long n_rows, long e_stride, long n_row, const int32_t *h_line_row, const int64_t *h_line_pos, long n_lines,
                    float *h_words, long words_stride);
/* ---- OOK devices: the sensor and remote messages of a 433 MHz capture — what the reference's command list starts `rtl_433 -f {freq}M` for
 * (rtlcoms.json, "Decode smart devices").  The arithmetic is the project's own, stated once in csrc/pss_ook.h (PARITY.md "OOK"); the device
 * and the host twins agree on every byte, and every output follows from indices in the ROW, so no chunking or windowing changes one.  There is
 * no word to look for: the device turns a row into the edges of its keyed envelope, cuts them into messages at long gaps and slices each
 * message into bits under the caller's timing (what rtl_433 -X 'n=..,m=OOK_PPM,s=..,l=..,g=..' takes; formats.ook_spec turns the string into
 * these arguments).  Samples and sample counts only: microseconds live in formats.  Rows are complex64, 8-byte aligned, x_stride samples
 * apart, the buffer holding samples [buf_index0, buf_index0 + n_buf) of every row of n_row samples; samples before index 0 count as 0 + 0j.
 * (dev_*: pointers into device memory; the pss_h_ twins take the same arrays on the host.)
 *   m[n] = fl32(fl32(re re) + fl32(im im)); e[n] = fl32((m[n - P + 1] + ... + m[n] in float64, in that order from +0.0) / P), P in [1, 65].
 * pss_ook_envelope: e[n] for n in [i_begin, i_end) of every row to float32 element r env_stride + (n - i_begin) of dev_env (4-byte aligned).
 *   A stage dump for tests and for the trace; the receiver does not go through it.  The buffer must hold [max(0, i_begin - P + 1), i_end).
 *   One kernel, k_ook_envelope.
 * pss_ook_levels: block b of a row is samples [4096 b, 4096 b + 4096); its mean is the float64 sum of its m in ascending order from +0.0,
 *   divided by 4096, and goes to float64 element r means_stride + (b - b_begin) of dev_means (8-byte aligned) for the whole blocks b in
 *   [b_begin, b_end), which must lie inside the row and the buffer.  The caller turns the means into the thresholds (formats.ook_levels: hi
 *   and lo as multiples of the lower quartile of a row's block means).  One kernel, k_ook_levels: 8 bytes read a sample, 8 written a block.
 * pss_ook_messages: sample n is decisive if e[n] >= hi (high) or e[n] < lo (low), a NaN neither; on(n) holds iff the last decisive sample
 *   d <= n exists, is high, and n - d <= R (R in [0, 4096]; hi >= lo > 0); on(-1) is off and so is everything past the row's end.  A rise at
 *   n: on(n) && !on(n - 1); a fall: the reverse; a pulse still on at the row's last sample falls at n_row (flag OPEN).  A pulse is a rise
 *   with the row's next fall, its gap the distance from that fall to the next rise.  A rise at pos starts a message if no fall lies in
 *   [pos - gap_limit, pos) (gap_limit in [1, 2^20]); the message is that pulse and the following ones up to and including the first whose gap
 *   exceeds gap_limit.  Edges at or past pos + span (span in [1, 2^24]) are not read: a pulse whose fall is not read is dropped with all
 *   later ones (LONG), and so is the 1025th pulse (MANY).  The slicer (mode; tol >= 0; the classes short, long and a non-zero sync more than
 *   2 tol apart) turns widths into bits, MSB first, at most 256 (FULL), every bit flipped where invert is 1:
 *     PSS_OOK_PWM  each pulse's width: within tol of short -> 1, of long -> 0, of sync -> nothing, else one odd symbol.
 *     PSS_OOK_PPM  each pulse's gap, the message's last pulse excluded: short -> 0, long -> 1, sync -> nothing, else one odd symbol.
 *     PSS_OOK_MC   Manchester: pulses and gaps in time order, the last pulse's gap excluded, are 1 half-bit within tol of short and 2 within
 *                  tol of 2 short; the first that is neither ends the list and counts as one odd.  Bit i is the pair of half-bit levels
 *                  (h[2 i + phase], h[2 i + phase + 1]) while inside the list, phase in {0, 1}: (1, 0) -> 1, (0, 1) -> 0, equal -> one odd.
 *   Reported iff n_bits >= min_bits (in [0, 256]) and n_odd <= max_odd (in [0, 2047]), for the messages whose pos lies in [s_begin, s_end) of
 *   every row, in ascending (row, pos): dev_bits uint8 [max_msgs][32], dev_n_bits int32, dev_row int32, dev_pos int64 (the first rise), dev_span int32
 *   (from the first rise to the last fall of a pulse kept), dev_meta uint32 (pulses kept in bits 0 .. 10, min(n_odd, 2047) in bits 11 .. 21,
 *   PSS_OOK_OPEN / _LONG / _MANY / _FULL above them), dev_count int32 [1] (the TRUE count; nothing is written past max_msgs).  The buffer must
 *   hold [max(0, s_begin - before), min(n_row, s_end + after)) with pss_ook_halo's before = gap_limit + R + P and after = span.
 *   PSS_E_ARG (reason in pss_last_error, starting "pss_ook_messages: "; a refused call writes nothing): a buffer or a window outside the
 *   row, s_end < s_begin, a window above 2^30 starts (2^31 edge positions over all rows), n_rows outside [1, 2^20], x_stride < n_buf, P, R,
 *   the thresholds, gap_limit, span, mode, tol, short, long, sync, phase, invert, min_bits or max_odd outside their ranges, classes not more
 *   than 2 tol apart, max_msgs < 0, a buffer that does not cover the window's reach, a null or misaligned pointer.
 *   Kernels: k_ook_detect (the one pass over every sample: m to LDS once per tile of 4096 edge positions, e from there, a workgroup max-scan
 *   of the last decisive sample, the edges compacted; e never reaches memory), then k_starts_scan, k_starts_gather, k_ook_heads,
 *   k_starts_scan, k_ook_list, k_ook_walk, k_starts_scan, k_ook_emit over the edges only.  Scratch on the context (the same buffers as the
 *   other receivers'), grow-only and freed by pss_destroy: 2 bytes per edge position of the largest call and 1 per 4096, 25 bytes per edge
 *   and 53 per possible message (every other edge and one more a row: a row's listed edges may end on a rise); the call waits once for
 *   the count of edges.
 * pss_ook_halo: the reach of a window: *before = gap_limit + R + P samples back from s_begin, *after = span samples on from s_end.
 *   PSS_E_ARG ("pss_ook_halo: "): an argument outside its range, a null pointer.  Host only.
 * pss_h_ook_envelope / _levels / _messages: the same on host buffers, pure host code (no context, no GPU; the reason:
 *   pss_last_error(NULL), starting with the device entry's name). */
#define PSS_OOK_PWM 0
#define PSS_OOK_PPM 1
#define PSS_OOK_MC 2
#define PSS_OOK_MAX_PULSES 1024
#define PSS_OOK_MAX_BITS 256
#define PSS_OOK_OPEN (1u << 22)
#define PSS_OOK_LONG (1u << 23)
#define PSS_OOK_MANY (1u << 24)
#define PSS_OOK_FULL (1u << 25)
int pss_ook_halo(int P, int R, long gap_limit, long span, long *before, long *after);
int pss_ook_envelope(pss_ctx *ctx, const float *dev_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, int P, long i_begin,
                     long i_end, float *dev_env, long env_stride);
int pss_h_ook_envelope(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, int P, long i_begin, long i_end,
                       float *h_env, long env_stride);
int pss_ook_levels(pss_ctx *ctx, const float *dev_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long b_begin, long b_end,
                   double *dev_means, long means_stride);
int pss_h_ook_levels(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long b_begin, long b_end,
                     double *h_means, long means_stride);
int pss_ook_messages(pss_ctx *ctx, const float *dev_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                     int P, float hi, float lo, int R, long gap_limit, long span, int mode, int w_short, int w_long, int w_sync, int tol, int phase,
                     int invert, int min_bits, int max_odd, uint8_t *dev_bits, int32_t *dev_n_bits, int32_t *dev_row, int64_t *dev_pos, int32_t *dev_span,
                     uint32_t *dev_meta, int32_t *dev_count, int max_msgs);
int pss_h_ook_messages(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, int P,
                       float hi, float lo, int R, long gap_limit, long span, int mode, int w_short, int w_long, int w_sync, int tol, int phase,
                       int invert, int min_bits, int max_odd, uint8_t *h_bits, int32_t *h_n_bits, int32_t *h_row, int64_t *h_pos, int32_t *h_span,
                       uint32_t *h_meta, int32_t *h_count, int max_msgs);
/* ---- Packet radio: the AX.25 frames and APRS reports of a 2 m capture — what the reference's command list starts
 * `rtl_fm -f {freq}M -M fm -s 22050 | direwolf` for (rtlcoms.json, "Decode APRS").  The arithmetic is the project's own, stated once in
 * csrc/pss_packet.h (PARITY.md "Packet"); the device and the host twins agree on every byte, and every output follows from indices in the
 * ROW, so no chunking or windowing changes one.  (pss_afsk_bits / pss_ax25_frames below restate the reference's own decode_aprs, which has no
 * NRZI, no check sequence and no bit timing; this receiver shares nothing with them.)
 * pss_packet_plan: the route from a capture at fs to 26 400 S/s (22 samples a bit at 1200 bit/s): decim = min(fs / 26 400, 204) for pss_ddc,
 *   up / down = 26 400 decim / fs reduced for pss_resample (2.4 MS/s and 240 kS/s: 99 / 100).  PSS_E_ARG (reason in pss_last_error(NULL),
 *   starting "pss_packet: "): an fs that is no integer, below 26 400, or whose reduced factors leave [1, 4096].
 * pss_packet_default_tones: the correlator table float64 [4][22]: cos and sin of one cycle a window (mark, 1200 Hz), cos and sin of 11 / 6
 *   cycles a window (space, 2200 Hz), from the host's libm.  The table is always a HOST table handed to the device entry and the twin alike.
 * pss_packet_front: dev_iq complex64 rows at 26 400 S/s, x_stride samples apart, 8-byte aligned, holding samples [buf_index0, buf_index0 +
 *   n_buf) of every row of n_row samples -> dev_z float32, sample i of row r at element r z_stride + (i - i_begin), i in [i_begin, i_end):
 *   d = the float32 polar discriminator (d[0] = 0), four float64 fma chains of the table over d[i - 11 .. i + 10] (zero outside the row),
 *   E_m = c0 c0 + c1 c1, E_s = space_gain (c2 c2 + c3 c3), z = (float)((E_s - E_m) / (E_s + E_m)), +0 where the sum is 0: the tone balance
 *   in [-1, 1], positive on space.  The buffer must hold the samples from max(0, i_begin - 12) to min(n_row, i_end + 10).  One kernel,
 *   k_packet_front.  PSS_E_ARG ("pss_packet_front: "; a refused call writes nothing): n_rows < 1, a buffer or a window outside the row,
 *   strides below n_buf or the window, i_end < i_begin, a window above 2^30 samples, a null table or a table entry that is not finite, a
 *   space_gain that is not finite or not > 0, a buffer that does not cover the window's halo, a null or misaligned pointer.
 * pss_packet_frames: dev_z float32 rows (pss_packet_front's), z_stride samples apart, 4-byte aligned -> the frames whose opening flag's first
 *   strobe s lies in [s_begin, s_end) of every row.  Every s with s - 22 >= 0 and s + 154 < n_row is tested: the nine strobes z[s + 22 k],
 *   k = -1 .. 7, sliced at 0 and NRZI-decoded, must read the flag 01111110 with q = min |z| >= q_min (finite, >= 0).  A survivor is walked
 *   with HDLC destuffing up to the closing flag, its strobes following the sender's bit clock (after each level change the next strobe moves
 *   one sample toward the middle between changes where it is more than two samples off), and accepted iff its length is a whole number of
 *   bytes in [17, 330], the CRC-16/X.25 residue is 0xF0B8, and its 2 to 10 addresses are well formed (A-Z, 0-9, space; the extension bit
 *   first set at the end of an address).  Among accepted starts less than 22 apart in a row with the same bytes the highest q stays, then
 *   the earliest.  Records in ascending (row, s): dev_msg uint8 [max_frames][332] (the frame with its two check bytes, zero-padded), dev_len
 *   int32 (bytes), dev_row int32, dev_pos int64 (s), dev_score float32 (q), dev_count int32 [1] (the TRUE count; nothing is written past
 *   max_frames).  The buffer must hold the samples from max(0, s_begin - 21 - 22) to min(n_row, s_end + 20 + 73 203); starts outside the
 *   window still count as neighbours.
 *   PSS_E_ARG ("pss_packet_frames: "; a refused call writes nothing): n_rows outside [1, 2^20], a buffer or a window outside the row,
 *   z_stride < n_buf, s_end < s_begin, a window above 2^30 starts (2^31 over all rows), a q_min that is negative or not finite, a buffer
 *   that does not cover the window's reach, max_frames < 0, a null or misaligned pointer.
 *   Kernels: k_packet_detect (the one pass over every start), then k_starts_scan, k_starts_gather, k_packet_walk, k_packet_keep,
 *   k_starts_scan, k_packet_emit over the survivors of the flag test only.  Scratch on the context (the same buffers as the other
 *   receivers'), 2 bytes per start of the largest call and 353 bytes per survivor (the start 8, the payload 332, length, score and rank 4
 *   each, the keep flag 1), grow-only and freed by pss_destroy; the call waits once for the count of survivors.
 * pss_h_packet_front / pss_h_packet_frames: the same on host buffers, pure host code (no context, no GPU; the reason: pss_last_error(NULL),
 *   starting with the device entry's name). */
int pss_packet_plan(double fs, int *decim, int *up, int *down);
int pss_packet_default_tones(double *tones);
int pss_packet_front(pss_ctx *ctx, const float *dev_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *tones,
                     double space_gain, long i_begin, long i_end, float *dev_z, long z_stride);
int pss_h_packet_front(const float *h_iq, long n_rows, long x_stride, long n_buf, long buf_index0, long n_row, const double *tones,
                       double space_gain, long i_begin, long i_end, float *h_z, long z_stride);
int pss_packet_frames(pss_ctx *ctx, const float *dev_z, long n_rows, long z_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end,
                      float q_min, uint8_t *dev_msg, int32_t *dev_len, int32_t *dev_row, int64_t *dev_pos, float *dev_score, int32_t *dev_count,
                      int max_frames);
int pss_h_packet_frames(const float *h_z, long n_rows, long z_stride, long n_buf, long buf_index0, long n_row, long s_begin, long s_end, float q_min,
                        uint8_t *h_msg, int32_t *h_len, int32_t *h_row, int64_t *h_pos, float *h_score, int32_t *h_count, int max_frames);
/* decode_afsk (decoders.py:94-112) for n_rows independent float64 audio rows of n samples: the two Bell-202 band-passes,
 * the energy of each band per bit period of int(fs/1200) samples, bit = e2200 > e1200.  d_bits uint8 [n_rows][n_bits],
 * n_bits = pss_afsk_n_bits(n, fs) = len(range(0, n - window, window)).  sos1200 / sos2200: HOST tables of nsec rows
 * (butter(5, [1100,1300] / [2100,2300] Hz, 'band')), or NULL to design them. */
int pss_afsk_n_bits(int n, double fs);
int pss_afsk_bits(pss_ctx *ctx, const double *d_audio, long n_rows, int n, double fs, const double *sos1200,
                  const double *sos2200, int nsec, uint8_t *d_bits);
/* The float32 primitives the path is built from, element by element, as NumPy's AVX512_SKX loops evaluate them (the
 * reference gets them from np.angle -> np.arctan2 :97/:125, np.log10 :328/:270, np.abs :185/:286): PSS_NP_ARCTAN2
 * out = arctan2(a, b) (SVML atan2f16 model), PSS_NP_LOG10 out = log10(a) (SVML log10f16 model; d_b unused),
 * PSS_NP_ABS out = abs(a + i b) (npy_hypotf).  Exposed so the models can be checked bit for bit against NumPy's outputs. */
enum { PSS_NP_ARCTAN2 = 0, PSS_NP_LOG10 = 1, PSS_NP_ABS = 2 };
int pss_np_f32(pss_ctx *ctx, int op, const float *d_a, const float *d_b, long n, float *d_out);
/* samples / np.max(np.abs(samples)) on n_rows float64 rows (decode_aprs's normalisation, decoders.py:126). */
int pss_row_normalise(pss_ctx *ctx, const double *d_x, long n_rows, int n, double *d_y);
/* decode_afsk on one HOST buffer of real float64 audio; normalise != 0 divides by max|x| on the device first, which makes
 * the result the bit stream decode_aprs (decoders.py:115-133) hands to its AX.25 framing.  h_bits uint8 [pss_afsk_n_bits]. */
int pss_h_afsk_bits(pss_ctx *ctx, const double *h_audio, int n, double fs, int normalise, const double *sos1200,
                    const double *sos2200, int nsec, uint8_t *h_bits);
/* bandpass_filter(data, lowcut, highcut, sample_rate) (signal_processing.py:34-42; used by decoders.py:100-101) on one
 * host row: lowcut <= 0 -> butter(5) low-pass at highcut, else band-pass.  sos/nsec: caller's table, or NULL to design it. */
int pss_h_bandpass_filter(pss_ctx *ctx, const double *h_x, int n, double lowcut, double highcut, double fs,
                          const double *sos, int nsec, double *h_y);
/* demodulate_signal(samples, fs, mode) on one host frame (dispatcher semantics: WFM is IQ-corrected first). */
int pss_h_demodulate_signal(pss_ctx *ctx, int mode, const float *h_iq, int n, double fs, double *h_audio_stereo,
                            int16_t *h_pcm);
/* demodulate_signal over n_frames read buffers held in host memory (e.g. an IQ recording, pyspecsdr.py:814-824, cut into
 * the reference's read size): h_pcm int16 [n_frames][n_out][2], chunk_frames frames per round trip. */
int pss_h_demodulate_batch(pss_ctx *ctx, int mode, const float *h_iq, long n_frames, int n, double fs, long chunk_frames,
                           int16_t *h_pcm);
int pss_h_measure_power(pss_ctx *ctx, const float *h_iq, int n, float *h_power);
/* iq_correction(samples) / demodulate_signal(samples, fs, 'RAW') on one host frame; either output may be NULL. */
int pss_h_iq_correction(pss_ctx *ctx, const float *h_iq, int n, float *h_out_iq, float *h_raw);

/* ---- streamed capture (BASELINE.json configs[4]) -------------------------------------------------- */
/* Pinned host memory for the streaming call (plain malloc'ed memory works too, but cannot overlap with compute). */
void *pss_host_alloc(size_t bytes);
void pss_host_free(void *p);
/* Cut a long HOST capture into n_frames frames of n samples and push it through spectrum + NFM demod in chunks of
 * chunk_frames: chunk k+1 is uploaded (hipMemcpyAsync, copy stream) while chunk k computes and chunk k-1's results
 * download — three streams, two device buffer sets.  h_db float32 [n_frames][n] (may be NULL), h_pcm int16
 * [n_frames][n_out][2].  Synchronous: returns when everything has landed in host memory.  Results are identical to
 * the device-resident pss_spectrum_nfm on the same frames. */
int pss_h_stream_spectrum_nfm(pss_ctx *ctx, const float *h_iq, long n_frames, int n, double fs, long chunk_frames,
                              float *h_db, int16_t *h_pcm);

/* The same capture, returning what the application consumes per frame instead of the dB rows: the display accumulator's
 * newest line (mode 0 waterfall: h_line_a = glyph, h_line_b = colour; mode 1 persistence: h_line_a = row index of the newest
 * trace, h_line_b unused) with a history of `window` rows, and the int16 PCM.  int8 [n_frames][disp_w] each.  Post-process
 * and accumulators run on the device chunk by chunk; the history crosses chunk boundaries.  h_halo_lo / h_halo_hi (n_halo
 * floats each, nullable): extremes of the rows preceding this capture (pss_waterfall_rows).  h_db (nullable) also returns
 * the dB rows; h_row_lo / h_row_hi (nullable, n_frames floats) return the per-row extremes (the halo for whatever follows).
 * Results are identical to the device-resident calls on the same frames. */
int pss_h_stream_display_nfm(pss_ctx *ctx, const float *h_iq, long n_frames, int n, double fs, long chunk_frames, int mode,
                             int window, int disp_h, int disp_w, const float *h_halo_lo, const float *h_halo_hi, int n_halo,
                             int8_t *h_line_a, int8_t *h_line_b, int16_t *h_pcm, float *h_db, float *h_row_lo, float *h_row_hi);

/* The same capture (a fresh history: no halo), and additionally the FULL display grid as the reference's screen shows it after the LAST
 * frame of every chunk: draw_waterfall / draw_persistence redraw all `window` lines / traces of the history with the history's current extremes
 * on every frame (pyspecsdr.py:1342-1406, :1512-1564), so older lines cannot be rebuilt from the per-frame lines above — a display refreshed
 * once per chunk needs this grid.  h_grid_a (+ h_grid_b: the waterfall's colour plane) int8 [n_chunks][disp_h][disp_w], n_chunks =
 * ceil(n_frames / chunk_frames); cell values as pss_waterfall_cells / pss_persistence_cells (which produce it from the last `window`
 * post-processed rows, carried from chunk to chunk on the device).  For a resident batch with materialised post-processed rows the grid after
 * frame f is pss_waterfall_cells(d_post + (f - w + 1) * len, w, ...), w = min(window, f + 1). */
int pss_h_stream_display_nfm_grids(pss_ctx *ctx, const float *h_iq, long n_frames, int n, double fs, long chunk_frames, int mode,
                                   int window, int disp_h, int disp_w, int8_t *h_line_a, int8_t *h_line_b, int16_t *h_pcm,
                                   float *h_row_lo, float *h_row_hi, int8_t *h_grid_a, int8_t *h_grid_b);
/* pss_h_stream_display_nfm with compute_fft's own float64 rows from the transform to the cells (n: a power of two in [16, 65536]): the lines —
 * and, with h_grid_a (+ h_grid_b for the waterfall; then no halo), the full screens after every chunk — are the cells the reference draws
 * from this capture.  h_halo_lo / _hi, h_db, h_row_lo / _hi: float64.  The capture is PCIe-bound either way (same time as the float32 call). */
int pss_h_stream_display_nfm_f64(pss_ctx *ctx, const float *h_iq, long n_frames, int n, double fs, long chunk_frames, int mode,
                                 int window, int disp_h, int disp_w, const double *h_halo_lo, const double *h_halo_hi, int n_halo,
                                 int8_t *h_line_a, int8_t *h_line_b, int16_t *h_pcm, double *h_db, double *h_row_lo, double *h_row_hi,
                                 int8_t *h_grid_a, int8_t *h_grid_b);

/* ---- ADC codes: read buffers as the radio delivers them ---------------------------------------------
 * Every entry point above takes complex64 (SoapySDR CF32: the driver's widening of the converter's integer codes).  These take the
 * codes: interleaved I,Q pairs in an 8-bit or int16 container, uploaded as they are (2 or 4 bytes per sample over the link instead
 * of 8) and widened on the device into the complex64 buffer the driver would have produced, bit for bit.  Drivers differ in that
 * widening, so it is not hard-wired:
 *   8-bit containers   iq_word = table256[index], index = the byte (PSS_IQ_U8) or code + 128 (PSS_IQ_S8); whatever the table holds
 *                      comes out unchanged (NaN, -0 included).  pss_h_iq_table fills it for a (scale, offset) grid.
 *   PSS_IQ_S16         iq_word = (float)code / (float)scale: one correctly rounded float32 division (NumPy's
 *                      codes.astype(float32) / float32(scale)); scale 2048 for 12-bit codes, 32768 for 16-bit ones.
 * table256 / h_table256 are HOST pointers, read during the call and not retained: required for the 8-bit containers, NULL for
 * PSS_IQ_S16.  scale: finite and > 0 for PSS_IQ_S16, ignored otherwise.  Violations: PSS_E_ARG (pss_last_error; with NULL for the
 * calls without a context). */
#define PSS_IQ_U8 0   /* uint8 I,Q pairs   (.cu8) */
#define PSS_IQ_S8 1   /* int8 I,Q pairs    (.cs8) */
#define PSS_IQ_S16 2  /* int16 LE I,Q pairs (.cs16; 12-bit codes use scale 2048) */
int pss_iq_code_bytes(int container);   /* bytes per complex sample: 2, 2, 4; < 0: unknown container */
/* table256[i] = (float)(((double)code_i - offset) / scale), rounded once; code_i = i (PSS_IQ_U8) or i - 128 (PSS_IQ_S8). */
int pss_h_iq_table(int container, double scale, double offset, float *table256);
/* The widening restated on the host: codes (any address) -> iq, 2 * n_samples float32 words. */
int pss_h_unpack_iq(int container, const void *codes, long n_samples, double scale, const float *table256, float *iq);
/* The same on the device, queued on the context's stream (no allocation, no host wait).  d_codes: any address with the container's
 * natural alignment (1 byte; 2 for int16); d_iq: 8-byte aligned, 2 * n_samples float32 words.  n_samples == 0: PSS_OK. */
int pss_unpack_iq(pss_ctx *ctx, int container, const void *d_codes, long n_samples, double scale, const float *h_table256, float *d_iq);
/* pss_h_demodulate_batch on a recording of codes (h_codes: n_frames x n samples): the codes go up, are unpacked on the device. */
int pss_h_demodulate_batch_codes(pss_ctx *ctx, int container, double scale, const float *h_table256, int mode, const void *h_codes,
                                 long n_frames, int n, double fs, long chunk_frames, int16_t *h_pcm);
/* pss_h_stream_display_nfm / _f64 on a capture of codes: per chunk the codes are uploaded on the copy stream and unpacked on the compute
 * stream in front of the chunk's kernels.  Every result is that of the complex64 call on the unpacked capture. */
int pss_h_stream_display_nfm_codes(pss_ctx *ctx, int container, double scale, const float *h_table256, const void *h_codes, long n_frames,
                                   int n, double fs, long chunk_frames, int mode, int window, int disp_h, int disp_w, const float *h_halo_lo,
                                   const float *h_halo_hi, int n_halo, int8_t *h_line_a, int8_t *h_line_b, int16_t *h_pcm, float *h_db,
                                   float *h_row_lo, float *h_row_hi);
int pss_h_stream_display_nfm_codes_f64(pss_ctx *ctx, int container, double scale, const float *h_table256, const void *h_codes, long n_frames,
                                       int n, double fs, long chunk_frames, int mode, int window, int disp_h, int disp_w,
                                       const double *h_halo_lo, const double *h_halo_hi, int n_halo, int8_t *h_line_a, int8_t *h_line_b,
                                       int16_t *h_pcm, double *h_db, double *h_row_lo, double *h_row_hi, int8_t *h_grid_a, int8_t *h_grid_b);

/* ---- replaying a capture: the main loop on a host recording, any mode, any view, squelch --------------------------------
 * Dead reads.  Before anything else the reference's loop tests the buffer it has just read,
 *     if len(samples) == 0 or np.all(samples == 0): ...; continue                                   (pyspecsdr.py:2237)
 * and read_samples hands the driver a zero-filled array (:1887), so a read that timed out comes back all zero and is SKIPPED: no AGC, no
 * demodulation, no compute_fft, no push into the waterfall / persistence history, no header, no advance of ui_update_counter.  The rule on
 * bits: a frame is dead iff every one of its 2 n float32 words satisfies (bits & 0x7fffffff) == 0 — NumPy's `== 0` exactly: -0.0 is zero, a
 * NaN and the smallest denormal are not, whatever denormal mode the code runs in.
 *   pss_live_frames     d_iq complex64 [n_frames][n], n >= 1, aligned to one sample (8 bytes; n may be odd) -> d_live uint8 [n_frames]
 *                       (nullable) = !np.all(frame == 0), d_live_idx int32 [n_frames] (nullable): the live frames' indices in ascending
 *                       order, entries behind the *n_live-th stay untouched.  k_live_flags: one wavefront per frame up to 2048 samples, one
 *                       workgroup above; 16-byte loads between the frame's first and last 16-byte boundary; a wavefront votes after a tile
 *                       and leaves the frame at the first set bit, so a live capture costs about one tile (1 KB) per frame and only dead
 *                       frames are read to the end.  No atomics: ballot and popcount, the squelch gate's prefix sum over tiles of 256.
 *                       THIS CALL WAITS like pss_squelch_gate: one asynchronous 16-byte copy of the count into pinned memory and one
 *                       synchronisation of the context's stream.  It cannot be captured into a graph.  n_frames == 0: PSS_OK, *n_live = 0.
 *   pss_h_live_frames   the same on host arrays, pure C, no context and no GPU (iq: any address).
 * PSS_E_ARG: n < 1, n_frames outside [0, 2^31), null n_live, null d_iq with n_frames > 0, d_iq not 8-byte aligned.
 *
 * pss_h_stream_frames plays a HOST capture as the main loop would: per chunk the upload (codes are unpacked by pss_unpack_iq), the dead-read
 * test, the resident step of the chosen view on the live frames, the downloads — on the three streams and two buffer sets of
 * pss_h_stream_display_nfm.  Every per-frame result is COMPACTED to the live frames in order, as pss_demod_gated compacts to the open ones,
 * and equals the resident call on the live frames of the whole capture in one batch.  Request and result are structs (here and only here:
 * the positional form would take about 40 arguments), zero-initialisable, `size` = sizeof the struct the caller compiled against; a size
 * this library does not know is PSS_E_ARG.
 *   request   h_in         the capture, n_frames x n samples: complex64, or ADC codes
 *             container    -1: complex64; PSS_IQ_*: codes with scale / h_table256 as for pss_unpack_iq
 *             n, fs        n a power of two in [16, 65536] (the reference's reads are 256 * 2^k); chunk_frames >= 1
 *             mode         PSS_MODE_*, the dispatcher's semantics (WFM frames IQ-corrected)
 *             view         0 waterfall, 1 persistence, 2 gradient (pss_frame_pipeline_cells' display codes), 3 spectrum bars, 4 surface,
 *                          5 vector
 *             window, disp_h, disp_w   as the view's resident call takes them: views 0 - 2 pss_frame_pipeline_cells' (disp_h: view 1 only);
 *                          view 3 pss_frame_pipeline_bars' disp_h, disp_w; view 4 pss_frame_pipeline_surface's disp_w (max_w - 8); view 5
 *                          pss_frame_pipeline_vector's max_h = disp_h, max_w = disp_w (max_h * ((max_w + 31) / 32) <= 16384)
 *             h_halo_lo / h_halo_hi / n_halo   float64 extremes of the rows preceding the capture; views 0 - 2 only
 *             skip_dead    1: dead reads are skipped as above; 0: every frame is live (a zero frame is drawn as a flat -100 dB row)
 *             squelch      NaN: ungated, every live frame is demodulated (the FIFO path, :2266-2268); otherwise the gate of
 *                          pss_squelch_gate with every / phase / held_in.  The state (held, phase) carries from chunk to chunk; dead
 *                          frames do not advance it
 *   result    host pointers, each nullable unless named as required; [n_live] means caller-sized [n_frames], filled [n_live]
 *             live uint8 [n_frames]; n_live
 *             db32 float32 [n_live][n]; row_lo / row_hi float64 [n_live] (views 0 - 2)
 *             peak / avg float64 [n_live], open uint8 [n_live]: with a squelch only (PSS_E_ARG otherwise: without it no meter runs)
 *             views 0, 2: line_a, line_b int8 [n_live][disp_w], both required; view 1: line_a, required
 *             view 3: height, level int8 [n_live][disp_w], required; range float64 [n_live][2]
 *             view 4: mag int8 [n_live][disp_w], required; range float64 [n_live][2]
 *             view 5: mask uint32 [n_live][disp_h][(disp_w + 31) / 32], required: the samples as read
 *             pcm int16 [n_open][n_out][2] (n_open = n_live without a squelch); n_open; held_out, phase_out: the gate's state behind
 *             the capture (phase_out = (phase + n_live) % every)
 * A chunk with some dead frames is gathered into context scratch (k_gather_frames) in front of its step; a chunk without a live frame launches
 * nothing and leaves history and gate state as they are; buffers behind n_live / n_open stay untouched.  Host waits: with skip_dead the
 * count of live frames, with a squelch the gate's count, one stream synchronisation each per chunk — the upload of chunk k + 1 is queued
 * before them, so the link stays busy; with skip_dead = 0 and squelch NaN there is no wait beyond pss_h_stream_display_nfm's own.
 * Synchronous; on any error everything queued is drained before the call returns.  Not capturable.
 * Out of scope: the per-chunk full-screen grids (pss_h_stream_display_nfm_grids keeps them); AGC, whose interval is wall-clock time; the
 * sharded drivers.
 * PSS_E_ARG: unknown size, view, mode or container (scale / table as pss_unpack_iq); n; chunk_frames < 1; n_frames outside [0, 2^31); a
 * halo with views 3 - 5; display geometry the view's resident call rejects; every < 0 or phase outside [0, every); a missing required
 * output; peak / avg / open without a squelch; null h_in with n_frames > 0. */
typedef struct pss_stream_req {
    uint32_t size;
    int container;
    const void *h_in;
    const float *h_table256;
    double scale;
    long n_frames;
    long chunk_frames;
    double fs;
    int n;
    int mode;
    int view;
    int window;
    int disp_h;
    int disp_w;
    const double *h_halo_lo;
    const double *h_halo_hi;
    int n_halo;
    int skip_dead;
    double squelch;
    double held_in;
    int every;
    int phase;
} pss_stream_req;
typedef struct pss_stream_res {
    uint32_t size;
    int phase_out;
    long n_live;
    long n_open;
    double held_out;
    uint8_t *live;
    float *db32;
    double *row_lo;
    double *row_hi;
    double *peak;
    double *avg;
    uint8_t *open;
    int8_t *line_a;
    int8_t *line_b;
    int8_t *height;
    int8_t *level;
    int8_t *mag;
    double *range;
    uint32_t *mask;
    int16_t *pcm;
} pss_stream_res;
int pss_live_frames(pss_ctx *ctx, const float *d_iq, long n_frames, int n, uint8_t *d_live, int32_t *d_live_idx, long *n_live);
int pss_h_live_frames(const float *iq, long n_frames, int n, uint8_t *live, int32_t *live_idx, long *n_live);
int pss_h_stream_frames(pss_ctx *ctx, const pss_stream_req *req, pss_stream_res *res);

/* ---- Multi-GPU: the path's exchange steps (one process per GPU, RCCL over xGMI) ----------------------------------------------------------
 * The path shards by contiguous blocks of independent frames / scanner slices (the sweep of pyspecsdr.py:2514-2590; every read buffer of
 * the loop :2236-2283 is processed on its own): every rank runs the single-GPU entry points above on its block, with NO collective in
 * the data path.  What crosses ranks is the gather of a rank's results to one rank (or all), and — for the display accumulators — the row
 * extremes of the frames just before a rank's block.  A Python host does both over torch.distributed (pyspecsdr_amd/shard.py); these
 * entry points are the same two steps for a host without it, queued on the context's stream.  librccl.so.1 is opened at the first call
 * ($PSS_RCCL_LIB if set — an explicit choice wins —, else a copy the process already holds, the loader's path, /opt/rocm/lib) — the library does not link against it,
 * and a lone rank (n_ranks = 1, id = NULL) never touches it.  Errors: PSS_E_COMM. */
#define PSS_COMM_ID_BYTES 128
/* contiguous blocks whose sizes differ by at most one: items [*start, *start + *count) belong to `rank` */
int pss_shard_range(long n_items, int rank, int n_ranks, long *start, long *count);
/* rank 0: a rendezvous id (ncclGetUniqueId) to hand to every other rank by whatever the host has — a file, a socket, its launcher */
int pss_comm_id(void *id /* PSS_COMM_ID_BYTES */);
/* every rank, after pss_create on ITS device: join the communicator (ncclCommInitRank; blocks until all n_ranks have called) */
int pss_comm_init(pss_ctx *ctx, const void *id, int rank, int n_ranks);
int pss_comm_free(pss_ctx *ctx);                              /* also done by pss_destroy */
int pss_comm_size(pss_ctx *ctx, int *rank, int *n_ranks);     /* (0, 1) without a communicator */
/* ONE collective for everything a rank produced in a sharded pass: every rank contributes `bytes` bytes (its packed result buffer, sized
 * for the largest block); d_all on the receiving rank(s): n_ranks x bytes, rank r's buffer at r * bytes.  dst < 0: all-gather; dst >= 0:
 * gather to that rank as grouped point-to-point messages (each peer's own xGMI link to the root; d_all is ignored elsewhere). */
int pss_gather_packed(pss_ctx *ctx, const void *d_local, size_t bytes, void *d_all, int dst);
/* The rows preceding this rank's block, up to `halo` of them (waterfall: the (lo, hi) extremes of 30 post-processed rows, persistence: 10
 * — pyspecsdr.py:130-132, :151-154; what pss_waterfall_rows' d_halo_lo / _hi take).  d_rows: this rank's counts[rank] rows of row_bytes
 * each, in frame order; counts: every rank's block size (the same n_ranks values on every rank, e.g. from pss_shard_range); d_halo:
 * room for `halo` rows; *n_halo = rows received = min(halo, rows before this block), in global order. */
int pss_halo_from_left(pss_ctx *ctx, const void *d_rows, const long *counts, size_t row_bytes, long halo, void *d_halo, long *n_halo);

/* Kernel-only time of the most recent batched call on this context, measured with HIP events on the
 * context's stream (ms); negative if timing is disabled.  pss_enable_timing(ctx, 1) turns it on. */
int pss_enable_timing(pss_ctx *ctx, int on);
float pss_last_kernel_ms(pss_ctx *ctx);
/* Per-kernel durations, "name=ms;name=ms;...", one entry per kernel launch since timing was enabled or since the
 * previous pss_kernel_times() call (HIP events around each launch on the context's stream). */
int pss_kernel_times(pss_ctx *ctx, char *buf, int buf_len);
/* Restrict the per-kernel events to launches of ONE kernel (the name pss_kernel_times reports, e.g. "k_nfm_fwd") and
 * drop the per-call events: every event is a barrier packet in the queue (~4 us), which a throughput measurement over
 * many launches should not pay for kernels it is not reporting.  NULL or "" = every kernel (the default). */
int pss_timing_filter(pss_ctx *ctx, const char *kernel);

#ifdef __cplusplus
}
#endif
#endif

"""Engine: one libpss context (one GPU, one stream) with the batched device-pointer entry points.

Device buffers are passed as raw addresses: anything with .data_ptr() (torch tensors), an int, or None.
PyTorch is only plumbing here (device memory / streams / torch.distributed); the library itself is
plain HIP behind a C ABI.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _lib as L


class PssError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libpss error {code}: {msg}")
        self.code = code


def _ptr(x):
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return int(x)


# the batched steps' `display` argument and the reference's history length of each view (pyspecsdr.py:130-131, :151-152, :1648)
_DISPLAYS = {"waterfall": 0, "persistence": 1, "gradient": 2}
_WINDOWS = (30, 10, 30)
# pss_h_stream_frames' `view`: the three display codes, then the views without a history (current_display_mode, pyspecsdr.py:167)
_VIEWS = {"waterfall": 0, "persistence": 1, "gradient": 2, "spectrum": 3, "surface": 4, "vector": 5}


# Read buffers as ADC codes (include/pss.h "ADC codes"): name -> (container, scale, offset), the four grids of tests/adc_cases.GRIDS.
# cu8: rtl_sdr's files (offset binary; 127.4 is SoapyRTLSDR's zero), cs8: hackrf_transfer's, cs12 / cs16: int16 containers (airspy_rx, ...)
IQ_FORMATS = {"cu8": (L.IQ_U8, 128.0, 127.4), "cs8": (L.IQ_S8, 128.0, 0.0), "cs12": (L.IQ_S16, 2048.0, 0.0), "cs16": (L.IQ_S16, 32768.0, 0.0)}
_IQ_DTYPES = {L.IQ_U8: np.uint8, L.IQ_S8: np.int8, L.IQ_S16: np.int16}


def iq_table(fmt, lib=None):
    """pss_h_iq_table: the 256 float32 values an 8-bit format's codes widen to, table[i] = float32((code_i - offset) / scale) with
    code_i = i (cu8) or i - 128 (cs8).  fmt: a name of IQ_FORMATS or (container, scale, offset).  Host code: no GPU needed."""
    container, scale, offset = IQ_FORMATS[fmt] if isinstance(fmt, str) else fmt
    table = np.empty(256, np.float32)
    if (lib or L.load()).pss_h_iq_table(int(container), float(scale), float(offset), _ptr(table)) != 0:
        raise ValueError("iq_table: an 8-bit format with a finite scale > 0 and a finite offset")
    return table


def _iq_args(fmt, table):
    """(container, scale, table or None) of a code format for the C ABI: an 8-bit format's own table unless the caller brings one (the
    driver's: SoapyRTLSDR's float32 formula, pyrtlsdr's c / 127.5 - 1, ...); int16 formats take no table."""
    container, scale, _ = IQ_FORMATS[fmt] if isinstance(fmt, str) else fmt
    if container == L.IQ_S16:
        if table is not None:
            raise ValueError("int16 code formats take a scale, not a table")
        return int(container), float(scale), None
    if table is None:
        table = iq_table(fmt)
    table = np.ascontiguousarray(table, np.float32)
    if table.shape != (256,):
        raise ValueError("table: 256 float32 values")
    return int(container), float(scale), table


def _iq_codes(codes, container):
    """A code array [..., 2] of the container's integer type, C-contiguous (no conversion: another type is an error, not a cast)."""
    dt = _IQ_DTYPES.get(container)
    if dt is None:
        raise ValueError("unknown IQ code container")
    if not isinstance(codes, np.ndarray) or codes.dtype != dt or codes.ndim < 1 or codes.shape[-1] != 2:
        raise ValueError(f"codes: a {np.dtype(dt).name} array [..., 2] (I, Q)")
    return np.ascontiguousarray(codes)


def h_unpack_iq(codes, fmt, table=None, lib=None):
    """pss_h_unpack_iq: codes [..., 2] -> the complex64 array [...] the driver would have delivered.  Host code: no GPU needed."""
    container, scale, table = _iq_args(fmt, table)
    codes = _iq_codes(codes, container)
    out = np.empty(codes.shape[:-1], np.complex64)
    if (lib or L.load()).pss_h_unpack_iq(container, _ptr(codes), out.size, scale, _ptr(table), _ptr(out)) != 0:
        raise ValueError("pss_h_unpack_iq: bad arguments")
    return out


def h_squelch_gate(peak, squelch, every=3, phase=0, held_in=0.0, lib=None):
    """pss_h_squelch_gate: the reference loop's squelch gate (pyspecsdr.py:2261, :2288-2291) over a host array of per-frame peaks ->
    (open uint8 [n_frames], n_open, held_out).  Pure host code: needs the library, not a GPU."""
    lib = lib or L.load()
    peak = np.ascontiguousarray(peak, np.float64)
    opened = np.empty(len(peak), np.uint8)
    n_open, held = C.c_long(), C.c_double()
    r = lib.pss_h_squelch_gate(_ptr(peak), len(peak), float(squelch), int(every), int(phase), float(held_in), _ptr(opened), C.byref(n_open), C.byref(held))
    if r != 0:
        raise PssError(r, "pss_h_squelch_gate: every < 0 or phase outside [0, every)")
    return opened, n_open.value, held.value


def h_scan_gate(peak, bw, threshold_db, min_bw=50e3, lib=None):
    """pss_h_scan_gate: the sweeps' gate (pyspecsdr.py:2549 / :2555, :1054 / :1059) over host arrays of per-slice peaks (float32) and
    bandwidths (float64) -> (hit uint8 [n], hit_idx int32 [n_hit], ascending).  hit = peak > float32(threshold_db) and bw > min_bw: NumPy
    compares the np.float32 peak with the Python-float threshold in float32.  Pure host code: needs the library, not a GPU."""
    lib = lib or L.load()
    peak, bw = np.ascontiguousarray(peak, np.float32), np.ascontiguousarray(bw, np.float64)
    if peak.ndim != 1 or peak.shape != bw.shape:
        raise ValueError("peak and bw: one value per slice each")
    hit, idx, n_hit = np.empty(len(peak), np.uint8), np.empty(len(peak), np.int32), C.c_long()
    r = lib.pss_h_scan_gate(_ptr(peak), _ptr(bw), len(peak), float(threshold_db), float(min_bw), _ptr(hit), _ptr(idx), C.byref(n_hit))
    if r != 0:
        raise PssError(r, "pss_h_scan_gate: bad argument")
    return hit, idx[:n_hit.value].copy()


def h_scan_dedupe(freq, grid_hz=100e3, lib=None):
    """pss_h_scan_dedupe: scan_frequencies' duplicate removal (pyspecsdr.py:1084-1091) -> the kept input indices (int32) in order of
    frequency: a stable sort, key round(f / grid_hz) * grid_hz with Python's round, the first record of every key.  Host code, no GPU."""
    lib = lib or L.load()
    freq = np.ascontiguousarray(freq, np.float64)
    if freq.ndim != 1:
        raise ValueError("freq: one value per record")
    keep, n_keep = np.empty(len(freq), np.int32), C.c_long()
    r = lib.pss_h_scan_dedupe(_ptr(freq), len(freq), float(grid_hz), _ptr(keep), C.byref(n_keep))
    if r != 0:
        raise PssError(r, "pss_h_scan_dedupe: grid_hz <= 0 or a frequency that is not finite")
    return keep[:n_keep.value].copy()


class Engine:
    """order: how calls are ordered against the caller's own GPU work.
         "torch" (default when torch is loaded): the library keeps its own non-blocking stream — which the default stream does NOT
                 synchronise with — and every device-pointer entry point is bracketed with pss_order_after / pss_order_before against
                 torch.cuda.current_stream(): buffers the caller filled on its stream are ready before the kernels read them, and torch work
                 queued after the call sees the results.  No host synchronisation; ~5 us per call.
         "none":  no ordering — for pipelines that order by hand (bench.py, multi.py: events / fences around many calls); the caller must
                 torch.cuda.synchronize() (or record / wait events on stream_handle()) between its own stream's work and the calls.
       stream: run on this hipStream_t / torch stream instead of the library's own (ordering is then the stream's own)."""

    def __init__(self, device=0, stream=None, order=None):
        self.lib = L.load()
        h = C.c_void_p()
        r = self.lib.pss_create(int(device), C.byref(h))
        if r != 0:
            raise PssError(r, self.lib.pss_last_error(None).decode())
        self.h = h
        self.device = device
        if stream is not None:
            self.set_stream(stream)
        if order is None:
            order = "none" if stream is not None else "torch"
        assert order in ("torch", "none")
        self.order = order
        # PSS_OPTIONS="key=value,key=value": pss_set_option switches for A/B measurements without touching the caller
        for kv in filter(None, os.environ.get("PSS_OPTIONS", "").split(",")):
            k, _, v = kv.partition("=")
            self.set_option(k.strip(), int(v))

    def _caller_stream(self):
        """torch's current stream on this engine's device as a hipStream_t (int), or None when there is nothing to order against."""
        if self.order != "torch":
            return None
        torch = sys.modules.get("torch")
        if torch is None or not torch.cuda.is_available() or not torch.cuda.is_initialized():
            return None
        return torch.cuda.current_stream(self.device).cuda_stream

    def _dev(self, fn, *args):
        """A device-pointer entry point, ordered after the caller's stream and the caller's stream after it (order = "torch")."""
        cs = self._caller_stream()
        if cs is not None:
            self._ck(self.lib.pss_order_after(self.h, cs))
        r = fn(self.h, *args)
        rb = self.lib.pss_order_before(self.h, cs) if cs is not None else 0
        self._ck(r)        # the call's own failure first,
        self._ck(rb)       # then a failed event record / stream wait: torch's work would not be ordered after the results

    def order_after(self, stream):
        """Work queued on this engine from now on starts after everything queued on `stream` (a hipStream_t as int, or an object with
        .cuda_stream) so far — e.g. another Engine's stream_handle()."""
        self._ck(self.lib.pss_order_after(self.h, _ptr(getattr(stream, "cuda_stream", stream))))

    def order_before(self, stream):
        """Work queued on `stream` from now on starts after everything this engine has queued so far."""
        self._ck(self.lib.pss_order_before(self.h, _ptr(getattr(stream, "cuda_stream", stream))))

    def close(self):
        if getattr(self, "h", None):
            self.lib.pss_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, r):
        if r != 0:
            msg = self.lib.pss_last_error(self.h).decode()
            if r in (L.PSS_E_PADLEN, L.PSS_E_CUTOFF):
                raise ValueError(msg)  # the exception type the reference's SciPy calls raise
            raise PssError(r, msg)

    # -- plumbing
    def set_stream(self, stream):
        self._ck(self.lib.pss_set_stream(self.h, _ptr(getattr(stream, "cuda_stream", stream))))

    # ---- the exchange steps behind the C ABI (RCCL; include/pss.h "Multi-GPU") — what shard.py does over torch.distributed, for hosts without it
    def comm_id(self):
        """Rank 0: the 128-byte rendezvous id to hand to every other rank."""
        buf = C.create_string_buffer(L.COMM_ID_BYTES)
        r = self.lib.pss_comm_id(buf)
        if r != 0:
            raise PssError(r, "pss_comm_id: librccl.so.1 not available (set PSS_RCCL_LIB)")
        return buf.raw

    def comm_init(self, comm_id, rank, n_ranks):
        """Join the communicator (blocks until all n_ranks have called).  comm_id None with n_ranks 1: a lone rank, no RCCL."""
        if comm_id is not None and len(comm_id) != L.COMM_ID_BYTES:
            raise ValueError("comm_id: the 128 bytes of Engine.comm_id()")
        self._ck(self.lib.pss_comm_init(self.h, comm_id, int(rank), int(n_ranks)))

    def comm_free(self):
        self._ck(self.lib.pss_comm_free(self.h))

    def comm_size(self):
        rank, n = C.c_int(), C.c_int()
        self._ck(self.lib.pss_comm_size(self.h, C.byref(rank), C.byref(n)))
        return rank.value, n.value

    def gather_packed(self, d_local, nbytes, d_all, dst=0):
        """Every rank's `nbytes` bytes at d_local -> d_all (n_ranks x nbytes, rank order) on rank dst, or on all ranks with dst None."""
        self._dev(self.lib.pss_gather_packed, _ptr(d_local), int(nbytes), _ptr(d_all), -1 if dst is None else int(dst))

    def halo_from_left(self, d_rows, counts, row_bytes, halo, d_halo):
        """The rows that precede this rank's block (at most `halo`), from its left neighbours; returns how many arrived."""
        arr = (C.c_long * len(counts))(*[int(c) for c in counts])
        got = C.c_long()
        self._dev(self.lib.pss_halo_from_left, _ptr(d_rows), arr, int(row_bytes), int(halo), _ptr(d_halo), C.byref(got))
        return got.value

    def stream_handle(self):
        """The hipStream_t this engine queues its work on, as an integer (e.g. for torch.cuda.ExternalStream)."""
        return int(self.lib.pss_get_stream(self.h) or 0)

    def set_option(self, key, value):
        self._ck(self.lib.pss_set_option(self.h, key.encode(), int(value)))

    def sync(self):
        self._ck(self.lib.pss_sync(self.h))

    def enable_timing(self, on=True):
        self._ck(self.lib.pss_enable_timing(self.h, int(on)))

    def timing_filter(self, kernel=None):
        """Only launches of `kernel` are bracketed with events (None = every kernel)."""
        self._ck(self.lib.pss_timing_filter(self.h, kernel.encode() if kernel else None))

    def last_kernel_ms(self):
        return float(self.lib.pss_last_kernel_ms(self.h))

    def kernel_times(self):
        """{kernel name: [ms per launch, ...]} for every launch since timing was enabled / last read
        (HIP events on the engine's stream)."""
        buf = C.create_string_buffer(1 << 20)
        self._ck(self.lib.pss_kernel_times(self.h, buf, 1 << 20))
        out = {}
        for item in buf.value.decode().split(";"):
            if item:
                k, v = item.split("=")
                out.setdefault(k, []).append(float(v))
        return out

    # -- filters
    def nfm_filters(self, fs):
        taps, sos, zi = np.empty(65), np.empty((4, 6)), np.empty((4, 2))
        self._ck(self.lib.pss_get_nfm_filters(self.h, float(fs), _ptr(taps), _ptr(sos), _ptr(zi)))
        return taps, sos, zi

    def set_nfm_filters(self, fs, taps, sos, zi):
        taps = np.ascontiguousarray(taps, np.float64)
        sos = np.ascontiguousarray(sos, np.float64)
        zi = np.ascontiguousarray(zi, np.float64)
        assert taps.shape == (65,) and sos.shape == (4, 6) and zi.shape == (4, 2)
        self._ck(self.lib.pss_set_nfm_filters(self.h, float(fs), _ptr(taps), _ptr(sos), _ptr(zi)))

    def ssb_taps(self, fs):
        taps = np.empty(65)
        self._ck(self.lib.pss_get_ssb_taps(self.h, float(fs), _ptr(taps)))
        return taps

    def set_ssb_taps(self, fs, taps):
        taps = np.ascontiguousarray(taps, np.float64)
        assert taps.shape == (65,)
        self._ck(self.lib.pss_set_ssb_taps(self.h, float(fs), _ptr(taps)))

    # -- batched device entry points (asynchronous on the engine's stream)
    def spectrum_db(self, d_iq, n_frames, n_fft, d_db):
        self._dev(self.lib.pss_spectrum_db, _ptr(d_iq), n_frames, n_fft, _ptr(d_db))

    def spectrum_post(self, d_db, n_frames, n_fft, d_post):
        self._dev(self.lib.pss_spectrum_post, _ptr(d_db), n_frames, n_fft, _ptr(d_post))

    def spectrum_post_extremes(self, d_db, n_frames, n_fft, d_post, d_row_lo, d_row_hi):
        """Post-process + the finite min / max of every post-processed row (inputs of waterfall_rows / persistence_rows)."""
        self._dev(self.lib.pss_spectrum_post_extremes, _ptr(d_db), n_frames, n_fft, _ptr(d_post), _ptr(d_row_lo),
                                                     _ptr(d_row_hi))

    def spectrum_db_post(self, d_iq, n_frames, n_fft, d_db, d_post, d_row_lo=None, d_row_hi=None):
        """compute_fft + post-process (+ row extremes) in one call; one fused kernel for 1024-point frames."""
        self._dev(self.lib.pss_spectrum_db_post, _ptr(d_iq), n_frames, n_fft, _ptr(d_db), _ptr(d_post), _ptr(d_row_lo),
                                               _ptr(d_row_hi))

    def row_extremes(self, d_rows, n_rows, length, d_row_lo, d_row_hi, f64=False):
        fn = self.lib.pss_row_extremes_f64 if f64 else self.lib.pss_row_extremes
        self._dev(fn, _ptr(d_rows), n_rows, length, _ptr(d_row_lo), _ptr(d_row_hi))

    def waterfall_rows(self, d_post, n_frames, length, d_row_lo, d_row_hi, disp_w, d_glyph, d_colour, n_halo=0, window=30,
                       f64=False):
        """Batched waterfall accumulator: the newest display line of every frame (history of `window` rows)."""
        fn = self.lib.pss_waterfall_rows_f64 if f64 else self.lib.pss_waterfall_rows
        self._dev(fn, _ptr(d_post), n_frames, length, _ptr(d_row_lo), _ptr(d_row_hi), n_halo, window, disp_w,
                    _ptr(d_glyph), _ptr(d_colour))

    def persistence_rows(self, d_post, n_frames, length, d_row_lo, d_row_hi, disp_h, disp_w, d_y, n_halo=0, window=10,
                         f64=False):
        """Batched persistence accumulator: the newest trace's row index per column for every frame."""
        fn = self.lib.pss_persistence_rows_f64 if f64 else self.lib.pss_persistence_rows
        self._dev(fn, _ptr(d_post), n_frames, length, _ptr(d_row_lo), _ptr(d_row_hi), n_halo, window, disp_h, disp_w,
                    _ptr(d_y))

    def gradient_rows(self, d_post, n_frames, length, d_row_lo, d_row_hi, disp_w, d_glyph, d_colour, n_halo=0, window=30, f64=False):
        """The gradient view's newest line of every frame (draw_gradient_waterfall): glyph = index into ' ._-=+*#@', colour 0..5."""
        fn = self.lib.pss_gradient_rows_f64 if f64 else self.lib.pss_gradient_rows
        self._dev(fn, _ptr(d_post), n_frames, length, _ptr(d_row_lo), _ptr(d_row_hi), n_halo, window, disp_w, _ptr(d_glyph), _ptr(d_colour))

    def spectrum_post_thresholds(self, d_db, n_frames, n_fft, d_row_thr, d_row_lo, d_row_hi):
        """The post-process without writing the rows: clamp threshold and finite extremes per row (inputs of *_rows_db)."""
        self._dev(self.lib.pss_spectrum_post_thresholds, _ptr(d_db), n_frames, n_fft, _ptr(d_row_thr), _ptr(d_row_lo), _ptr(d_row_hi))

    def waterfall_rows_db(self, d_db, n_frames, n_fft, d_row_thr, d_row_lo, d_row_hi, disp_w, d_glyph, d_colour, n_halo=0, window=30):
        """waterfall_rows from the dB rows + clamp thresholds (the post-processed rows are never written)."""
        self._dev(self.lib.pss_waterfall_rows_db, _ptr(d_db), n_frames, n_fft, _ptr(d_row_thr), _ptr(d_row_lo), _ptr(d_row_hi), n_halo,
                                                window, disp_w, _ptr(d_glyph), _ptr(d_colour))

    def persistence_rows_db(self, d_db, n_frames, n_fft, d_row_thr, d_row_lo, d_row_hi, disp_h, disp_w, d_y, n_halo=0, window=10):
        self._dev(self.lib.pss_persistence_rows_db, _ptr(d_db), n_frames, n_fft, _ptr(d_row_thr), _ptr(d_row_lo), _ptr(d_row_hi), n_halo,
                                                  window, disp_h, disp_w, _ptr(d_y))

    def scan(self, d_iq, n_slices, n_fft, fs, d_db, d_peak, d_bw, d_count):
        self._dev(self.lib.pss_scan, _ptr(d_iq), n_slices, n_fft, float(fs), _ptr(d_db), _ptr(d_peak),
                                   _ptr(d_bw), _ptr(d_count))

    def scan_threshold(self, d_iq, n_slices, n, fs, threshold_db, d_db=None, d_peak=None, d_bw=None, d_count=None):
        """The sweep driver's per-read numbers (pyspecsdr.py:1049-1057): max power, bins above an absolute threshold, bandwidth."""
        self._dev(self.lib.pss_scan_threshold, _ptr(d_iq), n_slices, n, float(fs), float(threshold_db), _ptr(d_db), _ptr(d_peak),
                                             _ptr(d_bw), _ptr(d_count))

    def hilbert(self, d_x, n_rows, n, d_analytic):
        """scipy.signal.hilbert along float64 rows -> complex128 rows (n: power of two in 256..1048576)."""
        self._dev(self.lib.pss_hilbert, _ptr(d_x), n_rows, n, _ptr(d_analytic))

    def power_db(self, d_iq, n_frames, n, d_power):
        self._dev(self.lib.pss_power_db, _ptr(d_iq), n_frames, n, _ptr(d_power))

    def iq_correction(self, d_iq, n_frames, n, d_out_iq=None, d_raw=None):
        self._dev(self.lib.pss_iq_correction, _ptr(d_iq), n_frames, n, _ptr(d_out_iq), _ptr(d_raw))

    def agc_steps(self, d_power, n, start_idx, n_gains, d_idx):
        self._dev(self.lib.pss_agc_steps, _ptr(d_power), n, start_idx, n_gains, _ptr(d_idx))

    def demod(self, mode, d_iq, n_frames, n, fs, d_pcm=None, d_audio=None):
        self._dev(self.lib.pss_demod, mode, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_pcm), _ptr(d_audio))

    def demod_signal(self, mode, d_iq, n_frames, n, fs, d_pcm=None, d_audio=None):
        """Dispatcher semantics (demodulate_signal): WFM frames are IQ-corrected first."""
        self._dev(self.lib.pss_demod_signal, mode, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_pcm), _ptr(d_audio))

    def demod_power(self, mode, d_iq, n_frames, n, fs, d_pcm, d_audio, d_power):
        """measure_signal_power + demodulate of the same read buffers (pyspecsdr.py:2251, :2262); AM: one pass over the IQ for both means."""
        self._dev(self.lib.pss_demod_power, mode, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_pcm), _ptr(d_audio), _ptr(d_power))

    def wfm_filters(self, fs):
        lp, pil, lmr = np.empty((3, 6)), np.empty((5, 6)), np.empty((5, 6))
        import ctypes as C
        a = C.c_double()
        self._ck(self.lib.pss_get_wfm_filters(self.h, float(fs), _ptr(lp), _ptr(pil), _ptr(lmr), C.addressof(a)))   # host-only: no stream ordering
        return lp, pil, lmr, a.value

    def set_wfm_filters(self, fs, lp, pilot, lmr, alpha):
        c = lambda x: np.ascontiguousarray(x, np.float64)
        lp, pilot, lmr = c(lp), c(pilot), c(lmr)
        assert lp.shape == (3, 6) and pilot.shape == (5, 6) and lmr.shape == (5, 6)
        self._ck(self.lib.pss_set_wfm_filters(self.h, float(fs), _ptr(lp), _ptr(pilot), _ptr(lmr), float(alpha)))

    def demod_out_len(self, mode, n, fs):
        """Output samples per frame at this engine's target rate (set_target_rate; 22050 unless changed)."""
        return int(self.lib.pss_demod_out_len_ctx(self.h, mode, n, float(fs)))

    def set_target_rate(self, target_rate):
        """demodulate_nfm / demodulate_wfm's target_rate (signal_processing.py:91, :119): decimation factor int(fs / target_rate)."""
        self._ck(self.lib.pss_set_target_rate(self.h, float(target_rate)))

    def spectrum_nfm(self, d_iq, n_frames, n, fs, d_db, d_pcm):
        self._dev(self.lib.pss_spectrum_nfm, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db), _ptr(d_pcm))

    def frame_pipeline_nfm(self, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, disp_w, d_glyph, d_colour, d_pcm,
                           n_halo=0, window=30):
        """One main-loop iteration for a batch of read buffers: NFM -> int16, dB row, post-processed row (+ extremes),
        waterfall line (pyspecsdr.py:2262-2283 + draw_waterfall).  d_post=None: the post-processed rows are not materialised."""
        self._dev(self.lib.pss_frame_pipeline_nfm, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db), _ptr(d_post), _ptr(d_row_lo),
                                                 _ptr(d_row_hi), n_halo, window, disp_w, _ptr(d_glyph), _ptr(d_colour), _ptr(d_pcm))

    def frame_pipeline(self, mode, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, disp_w, d_line_a, d_line_b, d_pcm,
                       n_halo=0, window=None, display="waterfall", disp_h=36):
        """One main-loop iteration per read buffer in any demodulation mode (dispatcher semantics: WFM is IQ-corrected first) and for any
        batched display accumulator: display "waterfall" -> (glyph, colour) lines, "persistence" -> the newest trace's row index (d_line_b
        unused), "gradient" -> (glyph index into ' ._-=+*#@', colour) lines.  window defaults to the reference's history length (30 / 10 / 30)."""
        disp = _DISPLAYS[display]
        window = _WINDOWS[disp] if window is None else int(window)
        self._dev(self.lib.pss_frame_pipeline, int(mode), _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db), _ptr(d_post), _ptr(d_row_lo),
                                             _ptr(d_row_hi), n_halo, window, disp, disp_h, disp_w, _ptr(d_line_a), _ptr(d_line_b), _ptr(d_pcm))

    def frame_pipeline_nfm_f64(self, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, disp_w, d_glyph, d_colour, d_pcm,
                               n_halo=0, window=30):
        """frame_pipeline_nfm with the reference's own row type: float64 dB rows, post-processed rows and extremes; the waterfall lines
        are then the cells the reference draws from this IQ (compute_fft returns float64, signal_processing.py:243-264)."""
        self._dev(self.lib.pss_frame_pipeline_nfm_f64, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db), _ptr(d_post), _ptr(d_row_lo),
                                                     _ptr(d_row_hi), n_halo, window, disp_w, _ptr(d_glyph), _ptr(d_colour), _ptr(d_pcm))

    def frame_pipeline_f64(self, mode, d_iq, n_frames, n, fs, d_db, d_post, d_row_lo, d_row_hi, disp_w, d_line_a, d_line_b, d_pcm,
                           n_halo=0, window=None, display="waterfall", disp_h=36):
        """frame_pipeline with float64 rows: any mode, waterfall line or persistence trace — the reference's cells."""
        disp = _DISPLAYS[display]
        window = _WINDOWS[disp] if window is None else int(window)
        self._dev(self.lib.pss_frame_pipeline_f64, int(mode), _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db), _ptr(d_post), _ptr(d_row_lo),
                  _ptr(d_row_hi), n_halo, window, disp, disp_h, disp_w, _ptr(d_line_a), _ptr(d_line_b), _ptr(d_pcm))

    def frame_pipeline_cells(self, mode, d_iq, n_frames, n, fs, d_db32, d_db64, d_row_lo, d_row_hi, disp_w, d_line_a, d_line_b, d_pcm,
                             n_halo=0, window=None, display="waterfall", disp_h=36):
        """The cell-exact iteration (float64 from the IQ to the cells, frame_pipeline_f64's results) with the dB rows written as float32
        (d_db32: compute_fft's float64 value rounded once) and, if d_db64 is not None, as float64 too.  1024-point frames: the transform and
        the post-process are one kernel and the float64 rows never go through HBM unless d_db64 asks for them."""
        disp = _DISPLAYS[display]
        window = _WINDOWS[disp] if window is None else int(window)
        self._dev(self.lib.pss_frame_pipeline_cells, int(mode), _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db32), _ptr(d_db64), _ptr(d_row_lo),
                  _ptr(d_row_hi), n_halo, window, disp, disp_h, disp_w, _ptr(d_line_a), _ptr(d_line_b), _ptr(d_pcm))

    def spectrum_cells(self, d_iq, n_frames, n, d_db32, d_db64, d_row_lo, d_row_hi, disp_w, d_line_a, d_line_b, n_halo=0, window=None,
                       display="waterfall", disp_h=36):
        """frame_pipeline_cells' display half alone: compute_fft -> post-process -> display line of every frame (no demodulator)."""
        disp = _DISPLAYS[display]
        window = _WINDOWS[disp] if window is None else int(window)
        self._dev(self.lib.pss_spectrum_cells, _ptr(d_iq), n_frames, n, _ptr(d_db32), _ptr(d_db64), _ptr(d_row_lo), _ptr(d_row_hi), n_halo, window,
                  disp, disp_h, disp_w, _ptr(d_line_a), _ptr(d_line_b))

    # -- squelch and the header's Peak / Avg meter (pyspecsdr.py:2261-2263, :388-392, :2288-2291)
    def row_meter(self, d_rows, n_rows, length, d_peak=None, d_avg=None):
        """np.max (NaN-propagating) and np.mean (NumPy's summation tree, every bit) of float64 rows: what draw_header keeps as PEAK_POWER
        and prints as Avg."""
        self._dev(self.lib.pss_row_meter_f64, _ptr(d_rows), n_rows, length, _ptr(d_peak), _ptr(d_avg))

    def squelch_gate(self, d_peak, n_frames, squelch, every=3, phase=0, held_in=0.0, d_open=None, d_open_idx=None):
        """The loop's gate over a batch's peaks -> (n_open, held_out); d_open uint8 [n_frames], d_open_idx int32 [n_frames] (ascending).
        Waits for the count (one stream synchronisation): the one call of the squelch path that does."""
        n_open, held = C.c_long(), C.c_double()
        self._dev(self.lib.pss_squelch_gate, _ptr(d_peak), n_frames, float(squelch), int(every), int(phase), float(held_in), _ptr(d_open),
                  _ptr(d_open_idx), C.byref(n_open), C.byref(held))
        return n_open.value, held.value

    def demod_gated(self, mode, d_iq, n_frames, n, fs, d_open_idx, n_open, d_pcm=None, d_audio=None):
        """demod_signal on the n_open frames d_open_idx names, results compacted in frame order ([n_open][n_out][2]); no host wait."""
        self._dev(self.lib.pss_demod_gated, int(mode), _ptr(d_iq), n_frames, n, float(fs), _ptr(d_open_idx), int(n_open), _ptr(d_pcm), _ptr(d_audio))

    def frame_pipeline_squelch(self, mode, d_iq, n_frames, n, fs, d_db32, d_db64, d_row_lo, d_row_hi, disp_w, d_line_a, d_line_b, d_pcm, squelch,
                               d_peak, d_avg=None, d_open=None, every=3, phase=0, held_in=0.0, n_halo=0, window=None, display="waterfall",
                               disp_h=36):
        """frame_pipeline_cells with the squelch: its display results, every frame's Peak / Avg, the gate, and d_pcm [n_open][n_out][2] of
        the open frames only -> (n_open, held_out).  The next batch continues with held_in = held_out, phase = (phase + n_frames) % every."""
        disp = _DISPLAYS[display]
        window = _WINDOWS[disp] if window is None else int(window)
        n_open, held = C.c_long(), C.c_double()
        self._dev(self.lib.pss_frame_pipeline_squelch, int(mode), _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db32), _ptr(d_db64), _ptr(d_row_lo),
                  _ptr(d_row_hi), n_halo, window, disp, disp_h, disp_w, _ptr(d_line_a), _ptr(d_line_b), _ptr(d_pcm), float(squelch), int(every),
                  int(phase), float(held_in), _ptr(d_peak), _ptr(d_avg), _ptr(d_open), C.byref(n_open), C.byref(held))
        return n_open.value, held.value

    def spectrum_db_f64(self, d_iq, n_frames, n_fft, d_db):
        """compute_fft's float64 rows (n_fft: power of two in 16..65536)."""
        self._dev(self.lib.pss_spectrum_db_f64, _ptr(d_iq), n_frames, n_fft, _ptr(d_db))

    def spectrum_post_f64(self, d_db, n_frames, n_fft, d_post, d_row_lo=None, d_row_hi=None):
        """The caller's smoothing + median clamp on float64 rows (pyspecsdr.py:2278-2283), optionally the rows' finite extremes."""
        self._dev(self.lib.pss_spectrum_post_f64, _ptr(d_db), n_frames, n_fft, _ptr(d_post), _ptr(d_row_lo), _ptr(d_row_hi))

    def waterfall_cells(self, d_rows, n_rows, length, disp_h, disp_w, d_glyph, d_colour, f64=False):
        fn = self.lib.pss_waterfall_cells_f64 if f64 else self.lib.pss_waterfall_cells
        self._dev(fn, _ptr(d_rows), n_rows, length, disp_h, disp_w, _ptr(d_glyph), _ptr(d_colour))

    def spectrogram_cells(self, d_rows, n_rows, length, disp_h, disp_w, d_glyph, d_colour, d_range=None, f64=False):
        fn = self.lib.pss_spectrogram_cells_f64 if f64 else self.lib.pss_spectrogram_cells
        self._dev(fn, _ptr(d_rows), n_rows, length, disp_h, disp_w, _ptr(d_glyph), _ptr(d_colour), _ptr(d_range))

    def spectrum_bars(self, d_rows, n_rows, length, disp_h, disp_w, d_height, d_level, d_range=None, f64=False):
        """draw_spectrogram per row in its compact form: bar height and level per column (int8 [n_rows][disp_w], -1 = not drawn) and the
        scale's dB range [n_rows][2].  formats.bars_cells / bars_cells expand them to spectrogram_cells' grids."""
        fn = self.lib.pss_spectrum_bars_f64 if f64 else self.lib.pss_spectrum_bars
        self._dev(fn, _ptr(d_rows), n_rows, length, disp_h, disp_w, _ptr(d_height), _ptr(d_level), _ptr(d_range))

    def bars_cells(self, d_height, d_level, n_rows, disp_h, disp_w, d_glyph, d_colour):
        """spectrum_bars' bars expanded on the device to the glyph / colour grids [n_rows][disp_h][disp_w] spectrogram_cells writes."""
        self._dev(self.lib.pss_bars_cells, _ptr(d_height), _ptr(d_level), n_rows, disp_h, disp_w, _ptr(d_glyph), _ptr(d_colour))

    def frame_pipeline_bars(self, mode, d_iq, n_frames, n, fs, d_db32, d_db64, d_post, disp_h, disp_w, d_height, d_level, d_range=None, d_pcm=None):
        """One main-loop iteration per read buffer with the reference's default view: frame_pipeline_cells' dB rows, the demodulator's PCM
        (d_pcm=None: the display half alone), the spectrum bars and scale range of every frame.  d_post (optional): the float64
        post-processed rows [n_frames][n - 4], e.g. for row_meter -> squelch_gate -> demod_gated beside this view."""
        self._dev(self.lib.pss_frame_pipeline_bars, int(mode), _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db32), _ptr(d_db64), _ptr(d_post), disp_h,
                  disp_w, _ptr(d_height), _ptr(d_level), _ptr(d_range), _ptr(d_pcm))

    def gradient_cells(self, d_rows, n_rows, length, disp_h, disp_w, d_glyph, d_colour, f64=False):
        fn = self.lib.pss_gradient_cells_f64 if f64 else self.lib.pss_gradient_cells
        self._dev(fn, _ptr(d_rows), n_rows, length, disp_h, disp_w, _ptr(d_glyph), _ptr(d_colour))

    def surface_cells(self, d_row, length, max_h, max_w, d_colour, f64=False):
        fn = self.lib.pss_surface_cells_f64 if f64 else self.lib.pss_surface_cells
        self._dev(fn, _ptr(d_row), length, max_h, max_w, _ptr(d_colour))

    def vector_cells(self, d_iq, n, max_h, max_w, d_grid):
        self._dev(self.lib.pss_vector_cells, _ptr(d_iq), n, max_h, max_w, _ptr(d_grid))

    def surface_mags(self, d_rows, n_rows, length, disp_w, d_mag, d_range=None, f64=False):
        """draw_surface_plot per row in its compact form: int(value * 20) per column (int8 [n_rows][disp_w], disp_w = max_w - 8, -1 = not
        drawn) and the row's finite (min_val, max_val) [n_rows][2].  formats.surface_cells / mags_cells expand them to surface_cells' grids."""
        fn = self.lib.pss_surface_mags_f64 if f64 else self.lib.pss_surface_mags
        self._dev(fn, _ptr(d_rows), n_rows, length, disp_w, _ptr(d_mag), _ptr(d_range))

    def mags_cells(self, d_mag, n_rows, max_h, max_w, d_colour):
        """surface_mags' magnitudes expanded on the device to the colour grids [n_rows][max_h][max_w] surface_cells writes."""
        self._dev(self.lib.pss_mags_cells, _ptr(d_mag), n_rows, max_h, max_w, _ptr(d_colour))

    def vector_masks(self, d_iq, n_frames, n, max_h, max_w, d_mask):
        """draw_vector_display per read buffer in its compact form: one bit per screen cell, uint32 [n_frames][max_h][(max_w + 31) // 32]
        (int32 tensors serve).  formats.vector_cells / masks_cells expand them to vector_cells' grids."""
        self._dev(self.lib.pss_vector_masks, _ptr(d_iq), n_frames, n, max_h, max_w, _ptr(d_mask))

    def masks_cells(self, d_mask, n_frames, max_h, max_w, d_grid):
        """vector_masks' masks expanded on the device to the int8 grids [n_frames][max_h][max_w] vector_cells writes."""
        self._dev(self.lib.pss_masks_cells, _ptr(d_mask), n_frames, max_h, max_w, _ptr(d_grid))

    def frame_pipeline_surface(self, mode, d_iq, n_frames, n, fs, d_db32, d_db64, d_post, disp_w, d_mag, d_range=None, d_pcm=None):
        """One main-loop iteration per read buffer with the SURFACE view: frame_pipeline_bars' rows and PCM (d_pcm=None: the display half
        alone), the surface magnitudes and finite extremes of every frame's post-processed row."""
        self._dev(self.lib.pss_frame_pipeline_surface, int(mode), _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db32), _ptr(d_db64), _ptr(d_post), disp_w,
                  _ptr(d_mag), _ptr(d_range), _ptr(d_pcm))

    def frame_pipeline_vector(self, mode, d_iq, n_frames, n, fs, d_db32, d_db64, d_post, max_h, max_w, d_mask, d_pcm=None):
        """One main-loop iteration per read buffer with the VECTOR view: frame_pipeline_bars' rows and PCM (d_pcm=None: the display half
        alone) and the constellation masks of the read buffers as read."""
        self._dev(self.lib.pss_frame_pipeline_vector, int(mode), _ptr(d_iq), n_frames, n, float(fs), _ptr(d_db32), _ptr(d_db64), _ptr(d_post), max_h,
                  max_w, _ptr(d_mask), _ptr(d_pcm))

    def unpack_iq(self, d_codes, n_samples, d_iq, fmt, table=None):
        """ADC codes on the device -> complex64 (pss_unpack_iq): d_codes any address with the container's alignment, d_iq 8-byte aligned,
        n_samples complex samples.  fmt: a name of IQ_FORMATS or (container, scale, offset); table: an 8-bit format's 256 float32 values
        (default: the format's own, iq_table)."""
        container, scale, table = _iq_args(fmt, table)
        self._dev(self.lib.pss_unpack_iq, container, _ptr(d_codes), int(n_samples), scale, _ptr(table), _ptr(d_iq))

    def morse_edges(self, d_iq, n_frames, n, cap, d_rise, d_fall, d_counts, threshold_db=-20.0):
        self._dev(self.lib.pss_morse_edges, _ptr(d_iq), n_frames, n, float(threshold_db), cap, _ptr(d_rise), _ptr(d_fall),
                                          _ptr(d_counts))

    # -- decoders for batches (include/pss.h): the per-message halves on the device, and decode_morse / decode_aprs in one call per batch
    def morse_text(self, d_rise, d_fall, d_counts, n_frames, cap, fs, d_text, d_text_len, d_timing, d_pulses, text_cap=None):
        """decode_morse from its edge lists on, for every frame of a morse_edges result (pss_morse_text): d_text uint8 [n_frames][text_cap]
        (default 2 * cap: a text has at most 2 bytes per pulse), d_text_len int32, d_timing float64 [n_frames][3], d_pulses int32."""
        text_cap = 2 * int(cap) if text_cap is None else int(text_cap)
        self._dev(self.lib.pss_morse_text, _ptr(d_rise), _ptr(d_fall), _ptr(d_counts), int(n_frames), int(cap), float(fs), text_cap,
                  _ptr(d_text), _ptr(d_text_len), _ptr(d_timing), _ptr(d_pulses))

    def ax25_frames(self, d_bits, n_rows, n_bits, out_cap, d_out, d_out_len):
        """decode_ax25_frame for rows of bits, one 0/1 per byte (pss_ax25_frames): d_out uint8 [n_rows][out_cap], d_out_len int32
        (-1: no packet, else the packet's true length)."""
        self._dev(self.lib.pss_ax25_frames, _ptr(d_bits), int(n_rows), int(n_bits), int(out_cap), _ptr(d_out), _ptr(d_out_len))

    def real_normalise(self, d_iq, n_rows, n, d_audio):
        """real part / max|real part| of complex64 rows in float32, widened to float64 (pss_real_normalise; decoders.py:121-125)."""
        self._dev(self.lib.pss_real_normalise, _ptr(d_iq), int(n_rows), int(n), _ptr(d_audio))

    def decode_morse_batch(self, d_iq, n_frames, n, fs, d_rise, d_fall, d_counts, d_text, d_text_len, d_timing, d_pulses, threshold_db=-20.0,
                           cap=None, text_cap=None):
        """decode_morse for every read buffer of a batch in one call (pss_decode_morse_batch).  cap (default n // 2 + 1, which alternating
        edges cannot exceed) sizes the work buffers d_rise / d_fall int32 [n_frames][cap]; d_counts int32 [n_frames][2]; the rest as
        morse_text."""
        cap = int(n) // 2 + 1 if cap is None else int(cap)
        text_cap = 2 * cap if text_cap is None else int(text_cap)
        self._dev(self.lib.pss_decode_morse_batch, _ptr(d_iq), int(n_frames), int(n), float(fs), float(threshold_db), cap, _ptr(d_rise),
                  _ptr(d_fall), _ptr(d_counts), text_cap, _ptr(d_text), _ptr(d_text_len), _ptr(d_timing), _ptr(d_pulses))

    def decode_aprs_batch(self, d_iq, n_rows, n, fs, d_audio, d_bits, out_cap, d_out, d_out_len, sos1200=None, sos2200=None):
        """decode_aprs for every complex64 read buffer of a batch in one call (pss_decode_aprs_batch).  Work buffers, returned filled:
        d_audio float64 [n_rows][n], d_bits uint8 [n_rows][afsk_n_bits(n, fs)]; d_out / d_out_len as ax25_frames; tables as afsk_bits."""
        c = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
        s1, s2 = c(sos1200), c(sos2200)
        self._dev(self.lib.pss_decode_aprs_batch, _ptr(d_iq), int(n_rows), int(n), float(fs), _ptr(s1), _ptr(s2),
                  5 if s1 is None else s1.shape[0], _ptr(d_audio), _ptr(d_bits), int(out_cap), _ptr(d_out), _ptr(d_out_len))

    def classify(self, d_iq, n_frames, n, fs, d_label=None, d_bw=None, d_mi=None, d_flat=None, d_psd=None):
        """classify_signal for a batch (pss_classify): any of label int32 / bw float64 / mi float32 / flat float32 / psd float32 [.,1024]."""
        self._dev(self.lib.pss_classify, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_label), _ptr(d_bw), _ptr(d_mi),
                                       _ptr(d_flat), _ptr(d_psd))

    # -- scanner sweep report (pyspecsdr.py:2539-2561, :1054-1068): gate the slices, classify only the detections
    def scan_gate(self, d_peak, d_bw, n_slices, threshold_db, min_bw=50e3, d_hit=None, d_hit_idx=None):
        """The sweeps' gate over a scan's peaks (float32) and bandwidths (float64) -> n_hit; d_hit uint8 [n_slices], d_hit_idx int32
        [n_slices] (ascending, n_hit entries written).  Waits for the count (one stream synchronisation), like squelch_gate."""
        n_hit = C.c_long()
        self._dev(self.lib.pss_scan_gate, _ptr(d_peak), _ptr(d_bw), n_slices, float(threshold_db), float(min_bw), _ptr(d_hit), _ptr(d_hit_idx),
                  C.byref(n_hit))
        return n_hit.value

    def classify_gated(self, d_iq, n_frames, n, fs, d_idx, n_idx, d_label=None, d_bw=None, d_mi=None, d_flat=None, d_psd=None):
        """classify on the n_idx frames d_idx names, outputs compacted to n_idx rows in list order; the frames are read in place.  No host wait."""
        self._dev(self.lib.pss_classify_gated, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_idx), int(n_idx), _ptr(d_label), _ptr(d_bw), _ptr(d_mi),
                  _ptr(d_flat), _ptr(d_psd))

    def sweep_report(self, kind, d_iq, n_slices, n, fs, threshold_db, d_peak, d_bw, d_hit_idx, min_bw=50e3, d_db=None, d_count=None, d_hit=None,
                     d_label=None, d_cls_bw=None, d_mi=None, d_flat=None):
        """One sweep: scan ("inline": pss_scan, "driver": pss_scan_threshold) -> gate -> classify_gated -> n_hit.  d_label / d_cls_bw / d_mi /
        d_flat: sized [n_slices], filled [n_hit].  Contains the gate's wait."""
        kind = {"inline": L.SWEEP_INLINE, "driver": L.SWEEP_DRIVER}.get(kind, kind)
        n_hit = C.c_long()
        self._dev(self.lib.pss_sweep_report, int(kind), _ptr(d_iq), n_slices, n, float(fs), float(threshold_db), float(min_bw), _ptr(d_db),
                  _ptr(d_peak), _ptr(d_bw), _ptr(d_count), _ptr(d_hit), _ptr(d_hit_idx), C.byref(n_hit), _ptr(d_label), _ptr(d_cls_bw), _ptr(d_mi),
                  _ptr(d_flat))
        return n_hit.value

    def class_name(self, label):
        return self.lib.pss_class_name(int(label)).decode()

    def persistence_cells(self, d_rows, n_rows, length, disp_h, disp_w, d_colour, f64=False):
        fn = self.lib.pss_persistence_cells_f64 if f64 else self.lib.pss_persistence_cells
        self._dev(fn, _ptr(d_rows), n_rows, length, disp_h, disp_w, _ptr(d_colour))

    # -- stateful display accumulators (device ring of the last rows)
    def ring_create(self, max_rows, length):
        h = C.c_void_p()
        self._ck(self.lib.pss_ring_create(self.h, max_rows, length, C.byref(h)))
        return h

    def _ring(self, fn, ring, *args):
        cs = self._caller_stream()
        if cs is not None:
            self._ck(self.lib.pss_order_after(self.h, cs))
        r = fn(ring, *args)
        if cs is not None:
            self.lib.pss_order_before(self.h, cs)
        self._ck(r)

    def ring_destroy(self, ring):
        self.lib.pss_ring_destroy(ring)

    def ring_push(self, ring, d_row):
        self._ring(self.lib.pss_ring_push, ring, _ptr(d_row))

    def ring_waterfall(self, ring, disp_h, disp_w, d_glyph, d_colour):
        self._ring(self.lib.pss_ring_waterfall, ring, disp_h, disp_w, _ptr(d_glyph), _ptr(d_colour))

    def ring_persistence(self, ring, disp_h, disp_w, d_colour):
        self._ring(self.lib.pss_ring_persistence, ring, disp_h, disp_w, _ptr(d_colour))

    # -- streamed capture from host memory (chunked, double-buffered H2D / compute / D2H)
    def pinned_empty(self, shape, dtype):
        """numpy array backed by pinned host memory (hipHostMalloc); keep a reference to it while in use."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = self.lib.pss_host_alloc(nbytes)
        if not p:
            raise MemoryError("hipHostMalloc failed")
        buf = (C.c_char * nbytes).from_address(p)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def pinned_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            self.lib.pss_host_free(p)

    def stream_display_nfm(self, h_iq, fs, chunk_frames, mode="waterfall", window=None, disp_h=36, disp_w=112, halo=None,
                           want_db=False, out=None):
        """Stream a host capture (complex64 [n_frames, n], pinned for overlap) and get back, per frame, the display
        accumulator's newest line and the int16 PCM (BASELINE configs[4]).  mode "waterfall": lines = (glyph, colour),
        history 30; "persistence": lines = (y,), history 10.  halo: (lo, hi) float32 arrays of the rows preceding the
        capture.  Returns dict(lines=..., pcm=..., row_lo=..., row_hi=..., db=... or None)."""
        assert h_iq.dtype == np.complex64 and h_iq.ndim == 2 and h_iq.flags.c_contiguous
        return self._stream_display(np.float32, h_iq, None, fs, chunk_frames, mode, window, disp_h, disp_w, halo, want_db, False, out)

    def stream_display_nfm_codes(self, h_codes, fs, chunk_frames, fmt, table=None, mode="waterfall", window=None, disp_h=36, disp_w=112,
                                 halo=None, want_db=False, out=None):
        """stream_display_nfm on a capture of ADC codes [n_frames, n, 2] (uint8 / int8 / int16; pinned_empty for overlap): the codes are
        uploaded (2 or 4 bytes per sample instead of 8) and widened on the device.  fmt / table: as unpack_iq.  Same result dict."""
        iq = _iq_args(fmt, table)
        h_codes = _iq_codes(h_codes, iq[0])
        assert h_codes.ndim == 3
        return self._stream_display(np.float32, h_codes, iq, fs, chunk_frames, mode, window, disp_h, disp_w, halo, want_db, False, out)

    def _stream_display(self, dtype, h_in, iq, fs, chunk_frames, mode, window, disp_h, disp_w, halo, want_db, grids, out):
        """The pss_h_stream_display_nfm* call for rows of `dtype` (float32 / float64), a capture of complex64 (iq None) or of ADC codes
        (iq = _iq_args(...)), with the full screens after every chunk or without."""
        f64 = dtype is np.float64
        nf, n = h_in.shape[:2]
        m = 0 if mode == "waterfall" else 1
        window = (30 if m == 0 else 10) if window is None else int(window)
        n_out = self.demod_out_len(L.MODE_NFM, n, fs)
        n_chunks = (nf + int(chunk_frames) - 1) // int(chunk_frames) if nf else 0
        # out: a previous call's result dict to write into again (pass arrays from pinned_empty() to keep the downloads
        # asynchronous: a copy into pageable memory is staged by the runtime and blocks the pipeline)
        if out is not None:
            la, lb = (out["lines"] + (None,))[:2]
            pcm, db, lo, hi = out["pcm"], out.get("db"), out["row_lo"], out["row_hi"]
            assert la.shape == (nf, disp_w) and pcm.shape == (nf, n_out, 2) and (not f64 or lo.dtype == np.float64) and len(lo) == nf and len(hi) == nf
        else:
            la = np.empty((nf, disp_w), np.int8)
            lb = np.empty((nf, disp_w), np.int8) if m == 0 else None
            pcm = np.empty((nf, n_out, 2), np.int16)
            db = np.empty((nf, n), dtype) if want_db else None
            lo, hi = np.empty(nf, dtype), np.empty(nf, dtype)
        ga = np.empty((n_chunks, disp_h, disp_w), np.int8) if grids else None
        gb = np.empty((n_chunks, disp_h, disp_w), np.int8) if grids and m == 0 else None
        hl = hh = None
        n_halo = 0
        if halo is not None and len(halo[0]):
            hl, hh = np.ascontiguousarray(halo[0], dtype), np.ascontiguousarray(halo[1], dtype)
            n_halo = len(hl)
        head = (self.h,) if iq is None else (self.h, iq[0], iq[1], _ptr(iq[2]))
        head += (_ptr(h_in), nf, n, float(fs), int(chunk_frames), m, window, disp_h, disp_w)
        tail = (_ptr(hl), _ptr(hh), n_halo, _ptr(la), _ptr(lb), _ptr(pcm), _ptr(db), _ptr(lo), _ptr(hi))
        codes = "" if iq is None else "_codes"
        if f64:
            self._ck(getattr(self.lib, f"pss_h_stream_display_nfm{codes}_f64")(*head, *tail, _ptr(ga), _ptr(gb)))
        elif grids:     # float32 rows with grids: complex64 captures with a fresh history, no dB rows
            assert iq is None and hl is None and db is None
            self._ck(self.lib.pss_h_stream_display_nfm_grids(*head, _ptr(la), _ptr(lb), _ptr(pcm), _ptr(lo), _ptr(hi), _ptr(ga), _ptr(gb)))
        else:
            self._ck(getattr(self.lib, f"pss_h_stream_display_nfm{codes}")(*head, *tail))
        res = {"lines": (la, lb) if m == 0 else (la,), "pcm": pcm, "row_lo": lo, "row_hi": hi, "db": db}
        if grids:
            res["grids"] = (ga, gb) if m == 0 else (ga,)
        return res

    def stream_display_nfm_f64(self, h_iq, fs, chunk_frames, mode="waterfall", window=None, disp_h=36, disp_w=112, halo=None, want_db=False,
                               grids=False, out=None):
        """stream_display_nfm with compute_fft's own float64 rows from the transform to the cells: the lines (and, grids=True, the full screen
        after every chunk) the REFERENCE draws from this capture.  halo / row_lo / row_hi / db: float64.  PCIe-bound like the float32 call."""
        assert h_iq.dtype == np.complex64 and h_iq.ndim == 2 and h_iq.flags.c_contiguous
        return self._stream_display(np.float64, h_iq, None, fs, chunk_frames, mode, window, disp_h, disp_w, halo, want_db, grids, out)

    def stream_display_nfm_codes_f64(self, h_codes, fs, chunk_frames, fmt, table=None, mode="waterfall", window=None, disp_h=36, disp_w=112,
                                     halo=None, want_db=False, grids=False, out=None):
        """stream_display_nfm_f64 on a capture of ADC codes [n_frames, n, 2] (see stream_display_nfm_codes)."""
        iq = _iq_args(fmt, table)
        h_codes = _iq_codes(h_codes, iq[0])
        assert h_codes.ndim == 3
        return self._stream_display(np.float64, h_codes, iq, fs, chunk_frames, mode, window, disp_h, disp_w, halo, want_db, grids, out)

    def stream_display_nfm_grids(self, h_iq, fs, chunk_frames, mode="waterfall", window=None, disp_h=36, disp_w=112):
        """stream_display_nfm for a capture with a fresh history, plus the FULL display grid after the last frame of every chunk (what the
        reference's screen shows: every line / trace of the history redrawn with the current extremes).  Returns the stream_display_nfm dict
        + "grids": (glyph, colour) int8 [n_chunks][disp_h][disp_w] for the waterfall, (colour,) for persistence."""
        assert h_iq.dtype == np.complex64 and h_iq.ndim == 2 and h_iq.flags.c_contiguous
        res = self._stream_display(np.float32, h_iq, None, fs, chunk_frames, mode, window, disp_h, disp_w, None, False, True, None)
        del res["db"]   # this call has no dB rows to offer
        return res

    def stream_spectrum_nfm(self, h_iq, fs, chunk_frames, h_db=None, h_pcm=None):
        """h_iq: complex64 [n_frames, n] host array (pinned for overlap).  Returns (h_db or None, h_pcm)."""
        assert h_iq.dtype == np.complex64 and h_iq.ndim == 2 and h_iq.flags.c_contiguous
        nf, n = h_iq.shape
        n_out = self.demod_out_len(L.MODE_NFM, n, fs)
        if h_pcm is None:
            h_pcm = np.empty((nf, n_out, 2), np.int16)
        self._ck(self.lib.pss_h_stream_spectrum_nfm(self.h, _ptr(h_iq), nf, n, float(fs), int(chunk_frames),
                                                     _ptr(h_db), _ptr(h_pcm)))
        return h_db, h_pcm

    # -- replaying a capture (include/pss.h "replaying a capture"): dead reads, and the main loop on a host recording
    def live_frames(self, d_iq, n_frames, n, d_live=None, d_live_idx=None):
        """The loop's first test on every read buffer (pyspecsdr.py:2237): d_live uint8 [n_frames] = not np.all(frame == 0), decided on the
        bits; d_live_idx int32 [n_frames]: the live frames in ascending order -> n_live.  Waits for the count like squelch_gate."""
        n_live = C.c_long()
        self._dev(self.lib.pss_live_frames, _ptr(d_iq), n_frames, n, _ptr(d_live), _ptr(d_live_idx), C.byref(n_live))
        return n_live.value

    @staticmethod
    def h_live_frames(frames, lib=None):
        """pss_h_live_frames on a host array complex64 [n_frames][n] -> (live uint8 [n_frames], live_idx int32 [n_live]).  Pure host code:
        needs the library, not a GPU."""
        frames = np.ascontiguousarray(frames, np.complex64)
        if frames.ndim != 2 or frames.shape[1] < 1:
            raise ValueError("frames: complex64 [n_frames][n], n >= 1")
        nf, n = frames.shape
        live, idx, n_live = np.empty(nf, np.uint8), np.empty(nf, np.int32), C.c_long()
        r = (lib or L.load()).pss_h_live_frames(_ptr(frames), nf, n, _ptr(live), _ptr(idx), C.byref(n_live))
        if r != 0:
            raise PssError(r, "pss_h_live_frames: bad argument")
        return live, idx[:n_live.value].copy()

    def stream_frames(self, h_in, fs, chunk_frames, mode=L.MODE_WFM, view="spectrum", fmt=None, table=None, skip_dead=True, squelch=None,
                      meter_every=3, phase=0, peak_power=0.0, window=None, disp_h=36, disp_w=112, halo=None, want_db=False, out=None):
        """pss_h_stream_frames: a host capture played as the main loop would — complex64 [n_frames, n], or with fmt (a name of IQ_FORMATS /
        a (container, scale, offset); table as unpack_iq) ADC codes [n_frames, n, 2]; pinned_empty arrays overlap copy and compute.
        view: "waterfall", "persistence", "gradient" (window: the history, default 30 / 10 / 30; halo = (lo, hi) float64), "spectrum"
        (disp_h, disp_w), "surface" (disp_w = max_w - 8) or "vector" (disp_h = max_h, disp_w = max_w).  skip_dead: all-zero read buffers are
        skipped as the reference's loop skips them.  squelch: a level in dB (None: every live buffer is demodulated), metered every
        meter_every-th live buffer from `phase`, starting from peak_power.
        Returns a dict trimmed to the live / open buffers: live, n_live, n_open, held_out, phase_out, pcm, db (want_db), the view's outputs
        (lines + row_lo / row_hi; height, level, range; mag, range; mask) and, with a squelch, peak, avg, open.  out: a previous call's
        dict with its untrimmed arrays under "buffers" to write into again (keeps pinned outputs)."""
        v = _VIEWS[view] if isinstance(view, str) else int(view)
        iq = None if fmt is None else _iq_args(fmt, table)
        if iq is None:
            assert h_in.dtype == np.complex64 and h_in.ndim == 2 and h_in.flags.c_contiguous
        else:
            h_in = _iq_codes(h_in, iq[0])
            assert h_in.ndim == 3
        nf, n = h_in.shape[:2]
        if window is None:
            window = _WINDOWS[v] if v <= 2 else 0
        n_out = max(self.demod_out_len(int(mode), n, fs), 0)   # a rate the demodulator rejects: the call reports it
        gated = squelch is not None
        words = (int(disp_w) + 31) // 32
        shapes = {"live": ((nf,), np.uint8), "pcm": ((nf, n_out, 2), np.int16)}
        if want_db:
            shapes["db32"] = ((nf, n), np.float32)
        if v <= 2:
            shapes.update(line_a=((nf, disp_w), np.int8), row_lo=((nf,), np.float64), row_hi=((nf,), np.float64))
            if v != 1:
                shapes["line_b"] = ((nf, disp_w), np.int8)
        elif v == 3:
            shapes.update(height=((nf, disp_w), np.int8), level=((nf, disp_w), np.int8), range=((nf, 2), np.float64))
        elif v == 4:
            shapes.update(mag=((nf, disp_w), np.int8), range=((nf, 2), np.float64))
        elif v == 5:
            shapes["mask"] = ((nf, max(int(disp_h), 0), words), np.uint32)
        if gated:
            shapes.update(peak=((nf,), np.float64), avg=((nf,), np.float64), open=((nf,), np.uint8))
        buf = out["buffers"] if out is not None else {k: np.empty(s, dt) for k, (s, dt) in shapes.items()}
        for k, (s, dt) in shapes.items():
            assert buf[k].shape == s and buf[k].dtype == dt and buf[k].flags.c_contiguous, f"out: {k} must be {dt.__name__} {s}"
        hl = hh = None
        if halo is not None and len(halo[0]):
            hl, hh = np.ascontiguousarray(halo[0], np.float64), np.ascontiguousarray(halo[1], np.float64)
        req = L.StreamReq(size=C.sizeof(L.StreamReq), container=-1 if iq is None else iq[0], h_in=_ptr(h_in),
                          h_table256=None if iq is None else _ptr(iq[2]), scale=0.0 if iq is None else iq[1], n_frames=nf,
                          chunk_frames=int(chunk_frames), fs=float(fs), n=n, mode=int(mode), view=v, window=int(window), disp_h=int(disp_h),
                          disp_w=int(disp_w), h_halo_lo=_ptr(hl), h_halo_hi=_ptr(hh), n_halo=0 if hl is None else len(hl), skip_dead=int(bool(skip_dead)),
                          squelch=float(squelch) if gated else float("nan"), held_in=float(peak_power), every=int(meter_every) if gated else 0,
                          phase=int(phase) if gated else 0)
        res = L.StreamRes(size=C.sizeof(L.StreamRes), **{k: _ptr(a) for k, a in buf.items()})
        self._ck(self.lib.pss_h_stream_frames(self.h, C.byref(req), C.byref(res)))
        nl, no = res.n_live, res.n_open
        d = {"buffers": buf, "live": buf["live"], "n_live": nl, "n_open": no, "held_out": res.held_out, "phase_out": res.phase_out,
             "pcm": buf["pcm"][:no], "db": buf["db32"][:nl] if want_db else None}
        for k in ("row_lo", "row_hi", "height", "level", "mag", "range", "mask", "peak", "avg", "open"):
            if k in buf:
                d[k] = buf[k][:nl]
        if v <= 2:
            d["lines"] = (buf["line_a"][:nl],) if v == 1 else (buf["line_a"][:nl], buf["line_b"][:nl])
        return d

    # -- host convenience (single frame, synchronous)
    def h_compute_fft(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64)
        out = np.empty(len(iq), np.float64)
        self._ck(self.lib.pss_h_compute_fft(self.h, _ptr(iq), len(iq), _ptr(out)))
        return out

    def h_compute_fft_c128(self, iq):
        """compute_fft of a complex128 buffer, float64 from the window product on (len(iq): a power of two in 16..65536)."""
        iq = np.ascontiguousarray(iq, np.complex128)
        out = np.empty(len(iq), np.float64)
        self._ck(self.lib.pss_h_compute_fft_c128(self.h, _ptr(iq), len(iq), _ptr(out)))
        return out

    def h_demodulate_am_c128(self, iq):
        """demodulate_am of a complex128 buffer (float64 np.abs / np.mean): (audio float64 (n, 2), pcm int16 (n, 2))."""
        iq = np.ascontiguousarray(iq, np.complex128)
        audio = np.empty((len(iq), 2), np.float64)
        pcm = np.empty((len(iq), 2), np.int16)
        self._ck(self.lib.pss_h_demodulate_am_c128(self.h, _ptr(iq), len(iq), _ptr(audio), _ptr(pcm)))
        return audio, pcm

    def h_demodulate_ssb_c128(self, iq, fs, lower=True):
        """demodulate_ssb of a complex128 buffer (the complex128 convolution on the samples as they are): (audio float64 (n, 2), pcm int16 (n, 2))."""
        iq = np.ascontiguousarray(iq, np.complex128)
        audio = np.empty((len(iq), 2), np.float64)
        pcm = np.empty((len(iq), 2), np.int16)
        self._ck(self.lib.pss_h_demodulate_ssb_c128(self.h, 1 if lower else 0, _ptr(iq), len(iq), float(fs), _ptr(audio), _ptr(pcm)))
        return audio, pcm

    def demod_ssb_c128(self, d_iq, n_frames, n, fs, d_pcm, d_audio, lower=True):
        self._dev(self.lib.pss_demod_ssb_c128, 1 if lower else 0, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_pcm), _ptr(d_audio))

    def h_mean_power_c128(self, iq):
        """np.mean(np.abs(iq) ** 2) of a complex128 buffer in float64 (the array part of measure_signal_power): np.float64."""
        iq = np.ascontiguousarray(iq, np.complex128)
        out = np.empty(1, np.float64)
        self._ck(self.lib.pss_h_mean_power_c128(self.h, _ptr(iq), len(iq), _ptr(out)))
        return out[0]

    def mean_power_c128(self, d_iq, n_frames, n, d_power):
        self._dev(self.lib.pss_mean_power_c128, _ptr(d_iq), n_frames, n, _ptr(d_power))

    def spectrum_db_c128(self, d_iq, n_frames, n_fft, d_db):
        self._dev(self.lib.pss_spectrum_db_c128, _ptr(d_iq), n_frames, n_fft, _ptr(d_db))

    def demod_am_c128(self, d_iq, n_frames, n, d_pcm, d_audio):
        self._dev(self.lib.pss_demod_am_c128, _ptr(d_iq), n_frames, n, _ptr(d_pcm), _ptr(d_audio))

    def h_demodulate(self, mode, iq, fs):
        iq = np.ascontiguousarray(iq, np.complex64)
        n_out = self.demod_out_len(mode, len(iq), fs)
        if n_out < 0:
            raise ValueError("sample rate below the target rate or unknown mode")
        audio = np.empty((n_out, 2), np.float64)
        pcm = np.empty((n_out, 2), np.int16)
        self._ck(self.lib.pss_h_demodulate(self.h, mode, _ptr(iq), len(iq), float(fs), _ptr(audio), _ptr(pcm)))
        return audio, pcm

    def h_demodulate_signal(self, mode, iq, fs):
        iq = np.ascontiguousarray(iq, np.complex64)
        n_out = self.demod_out_len(mode, len(iq), fs)
        if n_out < 0:
            raise ValueError("sample rate below the target rate or unknown mode")
        audio = np.empty((n_out, 2), np.float64)
        pcm = np.empty((n_out, 2), np.int16)
        self._ck(self.lib.pss_h_demodulate_signal(self.h, mode, _ptr(iq), len(iq), float(fs), _ptr(audio), _ptr(pcm)))
        return audio, pcm

    def h_demodulate_batch(self, mode, frames, fs, chunk_frames=4096):
        """frames: complex64 [n_frames][n] in host memory -> int16 PCM [n_frames][n_out][2] (dispatcher semantics)."""
        frames = np.ascontiguousarray(frames, np.complex64)
        nf, n = frames.shape
        n_out = self.demod_out_len(mode, n, fs)
        if n_out < 0:
            raise ValueError("sample rate below the target rate or unknown mode")
        pcm = np.empty((nf, n_out, 2), np.int16)
        self._ck(self.lib.pss_h_demodulate_batch(self.h, mode, _ptr(frames), nf, n, float(fs), int(chunk_frames), _ptr(pcm)))
        return pcm

    def h_demodulate_batch_codes(self, mode, codes, fs, fmt, table=None, chunk_frames=4096):
        """h_demodulate_batch on ADC codes [n_frames][n][2] (uint8 / int8 / int16): uploaded as codes, widened on the device.
        fmt / table: as unpack_iq."""
        container, scale, table = _iq_args(fmt, table)
        codes = _iq_codes(codes, container)
        assert codes.ndim == 3
        nf, n = codes.shape[:2]
        n_out = self.demod_out_len(mode, n, fs)
        if n_out < 0:
            raise ValueError("sample rate below the target rate or unknown mode")
        pcm = np.empty((nf, n_out, 2), np.int16)
        self._ck(self.lib.pss_h_demodulate_batch_codes(self.h, container, scale, _ptr(table), mode, _ptr(codes), nf, n, float(fs), int(chunk_frames),
                                                       _ptr(pcm)))
        return pcm

    def h_iq_correction(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64)
        out = np.empty(len(iq), np.complex64)
        self._ck(self.lib.pss_h_iq_correction(self.h, _ptr(iq), len(iq), _ptr(out), None))
        return out

    def h_morse_edges(self, iq, threshold_db=-20.0):
        """-> (rise_times, fall_times) int32 arrays of decode_morse (decoders.py:159-161) for one buffer."""
        iq = np.ascontiguousarray(iq, np.complex64)
        cap = max(len(iq) // 2 + 1, 1)
        rise, fall = np.empty(cap, np.int32), np.empty(cap, np.int32)
        nr, nf = C.c_int(), C.c_int()
        self._ck(self.lib.pss_h_morse_edges(self.h, _ptr(iq), len(iq), float(threshold_db), cap, _ptr(rise), _ptr(fall),
                                            C.byref(nr), C.byref(nf)))
        return rise[:nr.value].copy(), fall[:nf.value].copy()

    def h_classify_signal(self, iq, fs):
        """-> (label str, signal_bw float, modulation_index np.float32, spectral_flatness np.float32) for one read buffer."""
        iq = np.ascontiguousarray(iq, np.complex64)
        lab, bw, mi, fl = C.c_int(), C.c_double(), C.c_float(), C.c_float()
        self._ck(self.lib.pss_h_classify_signal(self.h, _ptr(iq), len(iq), float(fs), C.byref(lab), C.byref(bw), C.byref(mi), C.byref(fl)))
        return self.class_name(lab.value), bw.value, np.float32(mi.value), np.float32(fl.value)

    def h_raw(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64)
        raw = np.empty(len(iq), np.float32)
        self._ck(self.lib.pss_h_iq_correction(self.h, _ptr(iq), len(iq), None, _ptr(raw)))
        return raw

    def sosfilt(self, d_x, n_rows, n, sos, d_y):
        sos = np.ascontiguousarray(sos, np.float64)
        self._dev(self.lib.pss_sosfilt, _ptr(d_x), n_rows, n, _ptr(sos), sos.shape[0], _ptr(d_y))

    @staticmethod
    def _ba(b, a):
        b, a = np.ascontiguousarray(b, np.float64), np.ascontiguousarray(a, np.float64)
        if b.ndim != 1 or a.shape != b.shape or not 2 <= len(b) <= 9:
            raise ValueError("lfilter: b and a of the same length, 2 .. 9 coefficients each")
        return b, a

    def lfilter(self, d_x, n_rows, n, b, a, d_y):
        """scipy.signal.lfilter(b, a, x) from a zero state on float64 rows [n_rows][n] on the device (pss_lfilter); b, a: host tables."""
        b, a = self._ba(b, a)
        self._dev(self.lib.pss_lfilter, _ptr(d_x), n_rows, n, _ptr(b), _ptr(a), len(b), _ptr(d_y))

    @staticmethod
    def h_lfilter(x, b, a, lib=None):
        """pss_h_lfilter: the same on host rows (1-D or 2-D, along the last axis) -> float64.  Pure host code: needs the library, not a GPU."""
        b, a = Engine._ba(b, a)
        x = np.ascontiguousarray(x, np.float64)
        y = np.empty_like(x)
        n = x.shape[-1] if x.ndim else 0
        if (lib or L.load()).pss_h_lfilter(_ptr(x), x.size // n if n else 0, n, _ptr(b), _ptr(a), len(b), _ptr(y)) != 0:
            raise ValueError("pss_h_lfilter: bad arguments (a[0] must be finite and not 0)")
        return y

    # -- FM mono: decode_mono (signal_processing.py:331-359)
    def decode_mono_len(self, n):
        return self.lib.pss_decode_mono_len(int(n))

    def decode_mono(self, d_iq, n_frames, n, fs, d_pcm=None, d_audio=None, d_dec=None):
        """d_iq complex64 [n_frames][n] -> d_pcm int16 [n_frames][n_out], n_out = decode_mono_len(n); optional d_audio float64 (the value the
        int16 cast sees) and d_dec float32 (the decimated row before the de-emphasis)."""
        self._dev(self.lib.pss_decode_mono, _ptr(d_iq), n_frames, n, float(fs), _ptr(d_pcm), _ptr(d_audio), _ptr(d_dec))

    @staticmethod
    def h_decode_mono(iq, fs, stages=False, lib=None):
        """pss_h_decode_mono: one host buffer -> int16 (n_out,); stages=True: (pcm, audio float64, dec float32).  Pure host code: the
        kernels' statements on one thread, no GPU."""
        lib = lib or L.load()
        iq = np.ascontiguousarray(iq, np.complex64)
        if iq.ndim != 1:
            raise ValueError("samples must be a 1-D complex array")
        n_out = lib.pss_decode_mono_len(len(iq))
        pcm, audio, dec = np.empty(n_out, np.int16), np.empty(n_out, np.float64), np.empty(n_out, np.float32)
        if lib.pss_h_decode_mono(_ptr(iq), len(iq), float(fs), _ptr(pcm), _ptr(audio), _ptr(dec)) != 0:
            raise ValueError("pss_h_decode_mono: the sample rate must be finite and > 0")
        return (pcm, audio, dec) if stages else pcm

    def h_decode_mono_batch(self, frames, fs, chunk_frames=4096):
        """frames: complex64 [n_frames][n] in host memory -> int16 [n_frames][n_out]; chunk_frames frames go through one pss_decode_mono."""
        import torch
        frames = np.ascontiguousarray(frames, np.complex64)
        if frames.ndim != 2 or int(chunk_frames) < 1:
            raise ValueError("frames: [n_frames][n]; chunk_frames >= 1")
        nf, n = frames.shape
        n_out = self.decode_mono_len(n)
        pcm = np.empty((nf, n_out), np.int16)
        if n_out == 0:
            return pcm
        for c0 in range(0, nf, int(chunk_frames)):
            c = min(int(chunk_frames), nf - c0)
            d_iq = torch.from_numpy(frames[c0:c0 + c].view(np.float32)).to(f"cuda:{self.device}")
            d_pcm = torch.empty((c, n_out), dtype=torch.int16, device=f"cuda:{self.device}")
            self.decode_mono(d_iq, c, n, fs, d_pcm)
            pcm[c0:c0 + c] = d_pcm.cpu().numpy()
        return pcm

    # -- digital down-converter: K channels of a capture at fs / decim (pss_ddc; the arithmetic: csrc/pss_ddc.h)
    @staticmethod
    def ddc_word(offset_hz, fs, lib=None):
        """pss_ddc_word -> (word, effective_hz): the 64-bit frequency word of offset_hz at fs and the offset that results.  Host code."""
        w, eff = C.c_uint64(), C.c_double()
        if (lib or L.load()).pss_ddc_word(float(offset_hz), float(fs), C.byref(w), C.byref(eff)) != 0:
            raise ValueError("ddc_word: fs must be finite and > 0 and |offset_hz| <= fs / 2")
        return w.value, eff.value

    @staticmethod
    def _default_taps(lib, entry, why, *args):
        """A pss_*_default_taps entry point asked twice, for the length and then for the table -> float64 taps.  why: the ValueError's
        text where it refuses the integer arguments."""
        f = getattr(lib or L.load(), entry)
        args = [int(a) for a in args]
        n = C.c_int()
        if f(*args, None, C.byref(n)) != 0:
            raise ValueError(why)
        taps = np.empty(n.value, np.float64)
        r = f(*args, _ptr(taps), C.byref(n))
        if r != 0:
            raise PssError(r, entry)
        return taps

    @staticmethod
    def ddc_default_taps(decim, lib=None):
        """pss_ddc_default_taps: scipy.signal.decimate's FIR, firwin(20 decim + 1, 1 / decim); decim = 1: [1.0].  Host code."""
        return Engine._default_taps(lib, "pss_ddc_default_taps", "ddc_default_taps: decim outside [1, 204]; pass taps for a larger decimation", decim)

    @staticmethod
    def h_ddc_rotor(word, index0, n, lib=None):
        """pss_h_ddc_rotor -> (c, s) float64 [n]: the oscillator exp(-2 pi i word (index0 + t) / 2^64).  Host code."""
        lib = lib or L.load()
        c, s = np.empty(int(n), np.float64), np.empty(int(n), np.float64)
        if lib.pss_h_ddc_rotor(int(word) & (2 ** 64 - 1), int(index0), int(n), _ptr(c), _ptr(s)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return c, s

    @staticmethod
    def _ddc_args(lib, n_buf, words, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride):
        """The defaults of ddc / h_ddc -> (words, taps, the integer arguments in the C order behind them)."""
        if not (isinstance(words, np.ndarray) and words.dtype == np.uint64):   # Python integers: NumPy would take a mixed list through float64
            words = np.array([int(w) & (2 ** 64 - 1) for w in np.atleast_1d(np.asarray(words, object))], np.uint64)
        words = np.ascontiguousarray(np.atleast_1d(words), np.uint64)
        taps = Engine.ddc_default_taps(decim, lib) if taps is None else np.ascontiguousarray(np.atleast_1d(taps), np.float64)
        if words.ndim != 1 or taps.ndim != 1:
            raise ValueError("words and taps: 1-D tables")
        n_capture = int(n_buf) if n_capture is None else int(n_capture)
        n_out = lib.pss_ddc_out_len(n_capture, int(decim))
        lead = (len(taps) - 1) // 2 if lead is None else int(lead)
        m_begin = int(m_begin)
        m_end = max(n_out, 0) if m_end is None else int(m_end)
        out_stride = m_end - m_begin if out_stride is None else int(out_stride)
        return words, taps, (int(n_buf), int(buf_index0), n_capture), (len(words), int(decim)), (len(taps), lead, m_begin, m_end), out_stride

    def ddc(self, d_iq, n_buf, words, decim, d_out, taps=None, buf_index0=0, n_capture=None, lead=None, m_begin=0, m_end=None, out_stride=None):
        """d_iq complex64: samples [buf_index0, buf_index0 + n_buf) of a capture of n_capture samples (default: the buffer is the capture)
        -> d_out complex64, output m of channel c at element c * out_stride + (m - m_begin), m in [m_begin, m_end) (default: all
        n_out = ceil(n_capture / decim), rows back to back).  words: the channels' frequency words (ddc_word); taps: host float64 table
        (default: ddc_default_taps(decim)); lead: the tap that sits on the output's own sample (default (len(taps) - 1) // 2: zero phase)."""
        words, taps, a, b, c, out_stride = self._ddc_args(self.lib, n_buf, words, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride)
        self._dev(self.lib.pss_ddc, _ptr(d_iq), *a, _ptr(words), *b, _ptr(taps), *c, _ptr(d_out), out_stride)

    @staticmethod
    def h_ddc(iq, words, decim, taps=None, buf_index0=0, n_capture=None, lead=None, m_begin=0, m_end=None, lib=None):
        """pss_h_ddc: the same on a host buffer -> complex64 [K][m_end - m_begin].  Pure host code: the kernel's statements on one thread."""
        lib = lib or L.load()
        iq = np.ascontiguousarray(iq, np.complex64)
        if iq.ndim != 1:
            raise ValueError("iq: a 1-D complex buffer")
        words, taps, a, b, c, stride = Engine._ddc_args(lib, len(iq), words, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, None)
        out = np.empty((len(words), max(stride, 0)), np.complex64)
        if lib.pss_h_ddc(_ptr(iq), *a, _ptr(words), *b, _ptr(taps), *c, _ptr(out), stride) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return out

    # -- polyphase channeliser: every channel of a uniform grid of n_chan channels at fs / decim (pss_pfb; the arithmetic: csrc/pss_pfb.h)
    @staticmethod
    def pfb_default_taps(n_chan, lib=None):
        """pss_pfb_default_taps: firwin(20 n_chan + 1, 1 / n_chan), n_chan a power of two in [2, 1024].  Host code."""
        return Engine._default_taps(lib, "pss_pfb_default_taps", "pfb_default_taps: n_chan must be a power of two in [2, 1024]", n_chan)

    @staticmethod
    def _pfb_args(lib, n_buf, n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride):
        """The defaults of pfb / h_pfb -> (taps, the integer arguments in the C order either side of them)."""
        taps = Engine.pfb_default_taps(n_chan, lib) if taps is None else np.ascontiguousarray(np.atleast_1d(taps), np.float64)
        if taps.ndim != 1:
            raise ValueError("taps: a 1-D table")
        n_capture = int(n_buf) if n_capture is None else int(n_capture)
        n_out = lib.pss_ddc_out_len(n_capture, int(decim)) if 1 <= int(decim) <= 4096 else 0
        lead = (len(taps) - 1) // 2 if lead is None else int(lead)
        m_begin = int(m_begin)
        m_end = max(n_out, 0) if m_end is None else int(m_end)
        out_stride = m_end - m_begin if out_stride is None else int(out_stride)
        return taps, (int(n_buf), int(buf_index0), n_capture, int(n_chan), int(decim)), (len(taps), lead, m_begin, m_end), out_stride

    def pfb(self, d_iq, n_buf, n_chan, decim, d_out, taps=None, buf_index0=0, n_capture=None, lead=None, m_begin=0, m_end=None, out_stride=None):
        """d_iq complex64: samples [buf_index0, buf_index0 + n_buf) of a capture of n_capture samples (default: the buffer is the capture)
        -> d_out complex64 [n_chan] rows, output m of row c at element c * out_stride + (m - m_begin), m in [m_begin, m_end) (default: all
        n_out = ceil(n_capture / decim), rows back to back).  Row c is the channel at c fs / n_chan (c < n_chan / 2) or (c - n_chan) fs /
        n_chan.  taps: host float64 table (default: pfb_default_taps(n_chan)); lead: the tap that sits on the output's own sample (default
        (len(taps) - 1) // 2: zero phase)."""
        taps, a, b, out_stride = self._pfb_args(self.lib, n_buf, n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride)
        self._dev(self.lib.pss_pfb, _ptr(d_iq), *a, _ptr(taps), *b, _ptr(d_out), out_stride)

    @staticmethod
    def _h_chan(entry, args_of, iq, n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, lib):
        """h_pfb / h_bank: the host twin `entry` with the defaults of args_of (_pfb_args / _bank_args)."""
        lib = lib or L.load()
        iq = np.ascontiguousarray(iq, np.complex64)
        if iq.ndim != 1:
            raise ValueError("iq: a 1-D complex buffer")
        taps, a, b, stride = args_of(lib, len(iq), n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, None)
        out = np.empty((max(int(n_chan), 0), max(stride, 0)), np.complex64)
        if getattr(lib, entry)(_ptr(iq), *a, _ptr(taps), *b, _ptr(out), stride) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return out

    @staticmethod
    def h_pfb(iq, n_chan, decim, taps=None, buf_index0=0, n_capture=None, lead=None, m_begin=0, m_end=None, lib=None):
        """pss_h_pfb: the same on a host buffer -> complex64 [n_chan][m_end - m_begin].  Pure host code: the kernel's statements on one thread."""
        return Engine._h_chan("pss_h_pfb", Engine._pfb_args, iq, n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, lib)

    # -- channeliser for band plans: the same for every n_chan = 2^a 3^b 5^c in [2, 1024] (pss_bank; the arithmetic: csrc/pss_bank.h)
    @staticmethod
    def bank_default_taps(n_chan, lib=None):
        """pss_bank_default_taps: firwin(20 n_chan + 1, 1 / n_chan), n_chan = 2^a 3^b 5^c in [2, 1024].  Host code."""
        return Engine._default_taps(lib, "pss_bank_default_taps", "bank_default_taps: n_chan must be of the form 2^a 3^b 5^c in [2, 1024]", n_chan)

    @staticmethod
    def _bank_args(lib, n_buf, n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride):
        """The defaults of bank / h_bank: _pfb_args' with bank_default_taps."""
        if taps is None:
            taps = Engine.bank_default_taps(n_chan, lib)
        return Engine._pfb_args(lib, n_buf, n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride)

    def bank(self, d_iq, n_buf, n_chan, decim, d_out, taps=None, buf_index0=0, n_capture=None, lead=None, m_begin=0, m_end=None, out_stride=None):
        """pfb for any n_chan = 2^a 3^b 5^c in [2, 1024] (pss_bank): the same arguments and layout.  Row c is the channel at c fs / n_chan
        (c <= (n_chan - 1) / 2) or (c - n_chan) fs / n_chan.  taps default: bank_default_taps(n_chan).  A power-of-two n_chan runs
        pss_pfb's code."""
        taps, a, b, out_stride = self._bank_args(self.lib, n_buf, n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride)
        self._dev(self.lib.pss_bank, _ptr(d_iq), *a, _ptr(taps), *b, _ptr(d_out), out_stride)

    @staticmethod
    def h_bank(iq, n_chan, decim, taps=None, buf_index0=0, n_capture=None, lead=None, m_begin=0, m_end=None, lib=None):
        """pss_h_bank: the same on a host buffer -> complex64 [n_chan][m_end - m_begin].  Pure host code: the kernel's statements on one thread."""
        return Engine._h_chan("pss_h_bank", Engine._bank_args, iq, n_chan, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, lib)

    # -- rational resampler for rows: scipy.signal.resample_poly bit for bit (pss_resample; the arithmetic: csrc/pss_resample.h)
    RS_DTYPES = {np.dtype(np.float32): L.RS_F32, np.dtype(np.float64): L.RS_F64, np.dtype(np.complex64): L.RS_C64}

    @staticmethod
    def resample_out_len(n_in, up, down, lib=None):
        """pss_resample_out_len: ceil(n_in up / down) at the reduced factors.  Host code."""
        n = (lib or L.load()).pss_resample_out_len(int(n_in), int(up), int(down))
        if n < 0:
            raise ValueError("resample_out_len: up and down in [1, 4096], 0 <= n_in <= 2^48")
        return n

    @staticmethod
    def resample_default_taps(up, down, lib=None):
        """pss_resample_default_taps: resample_poly's own design, firwin(20 m + 1, 1 / m, window=('kaiser', 5.0)) with m = max(up, down) after
        the reduction, float64 (before the cast to the row's type and the scaling by up).  Host code."""
        return Engine._default_taps(lib, "pss_resample_default_taps", "resample_default_taps: up and down in [1, 4096]", up, down)

    @staticmethod
    def _resample_args(lib, n_buf, up, down, taps, buf_index0, n_in, j_begin, j_end):
        """The defaults of resample / h_resample -> (taps, n_in, j_begin, j_end)."""
        taps = Engine.resample_default_taps(up, down, lib) if taps is None else np.ascontiguousarray(np.atleast_1d(taps), np.float64)
        if taps.ndim != 1:
            raise ValueError("taps: a 1-D table")
        n_in = int(n_buf) + int(buf_index0) if n_in is None else int(n_in)
        if j_end is None:
            j_end = max(lib.pss_resample_out_len(n_in, int(up), int(down)), 0)
        return taps, n_in, int(j_begin), int(j_end)

    def resample(self, d_x, dtype, n_rows, n_buf, up, down, d_y, taps=None, x_stride=None, buf_index0=0, n_in=None, j_begin=0, j_end=None,
                 y_stride=None):
        """d_x: n_rows rows of `dtype` (float32, float64 or complex64), samples [buf_index0, buf_index0 + n_buf) of rows n_in samples long
        (default: the buffer is the row), x_stride elements apart (default n_buf) -> d_y, output j of row r at element r * y_stride +
        (j - j_begin), j in [j_begin, j_end) (default: all ceil(n_in up / down), rows back to back).  taps: host float64 table (default:
        resample_default_taps(up, down))."""
        taps, n_in, j_begin, j_end = self._resample_args(self.lib, n_buf, up, down, taps, buf_index0, n_in, j_begin, j_end)
        code = self.RS_DTYPES.get(np.dtype(dtype), -1)
        self._dev(self.lib.pss_resample, _ptr(d_x), code, int(n_rows), int(n_buf if x_stride is None else x_stride), int(n_buf), int(buf_index0), n_in,
                  int(up), int(down), _ptr(taps), len(taps), j_begin, j_end, _ptr(d_y), int(j_end - j_begin if y_stride is None else y_stride))

    @staticmethod
    def h_resample(x, up, down, taps=None, buf_index0=0, n_in=None, j_begin=0, j_end=None, lib=None):
        """pss_h_resample: the same on a host array [n_rows][n_buf] or [n_buf] -> the same type, [n_rows][j_end - j_begin] or
        [j_end - j_begin].  Pure host code: the kernel's statements on one thread."""
        lib = lib or L.load()
        x = np.asarray(x)
        if x.ndim not in (1, 2) or x.dtype not in Engine.RS_DTYPES:
            raise ValueError("x: a 1-D or 2-D float32, float64 or complex64 array")
        rows = np.ascontiguousarray(x.reshape(-1, x.shape[-1]))
        taps, n_in, j_begin, j_end = Engine._resample_args(lib, rows.shape[1], up, down, taps, buf_index0, n_in, j_begin, j_end)
        out = np.empty((rows.shape[0], max(j_end - j_begin, 0)), x.dtype)
        if lib.pss_h_resample(_ptr(rows), Engine.RS_DTYPES[x.dtype], rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_in, int(up),
                              int(down), _ptr(taps), len(taps), j_begin, j_end, _ptr(out), out.shape[1]) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return out if x.ndim == 2 else out[0]

    # -- survey of a capture: Welch's averaged periodogram and its max-hold row (pss_welch; the arithmetic: csrc/pss_welch.h)
    _WELCH_WINDOWS = {}   # the default window of each nperseg, made once

    @staticmethod
    def welch_segments(n, nperseg, step, lib=None):
        """pss_welch_segments: (n - nperseg) // step + 1 segments, 0 when n < nperseg.  Host code."""
        L_ = (lib or L.load()).pss_welch_segments(int(n), int(nperseg), int(step))
        if L_ < 0:
            raise ValueError("welch_segments: nperseg in {256, 512, 1024, 2048, 4096}, step in [1, nperseg]")
        return L_

    @staticmethod
    def welch_default_window(nperseg, lib=None):
        """The default window: scipy.signal.get_window('hann', nperseg) where SciPy imports, pss_welch_default_window's table (the same
        periodic Hann, within 2^-53) otherwise.  Host code."""
        lib = lib or L.load()
        if lib.pss_welch_segments(int(nperseg), int(nperseg), 1) < 0:
            raise ValueError("welch_default_window: nperseg in {256, 512, 1024, 2048, 4096}")
        w = Engine._WELCH_WINDOWS.get(int(nperseg))
        if w is None:
            try:
                from scipy.signal import get_window
                w = np.ascontiguousarray(get_window("hann", int(nperseg)), np.float64)
            except ImportError:
                w = Engine.welch_c_window(nperseg, lib)
            Engine._WELCH_WINDOWS[int(nperseg)] = w
        return w.copy()

    @staticmethod
    def welch_c_window(nperseg, lib=None):
        """pss_welch_default_window itself: 0.5 - 0.5 cos(2 pi i / nperseg).  Host code."""
        w = np.empty(max(int(nperseg), 0), np.float64)
        if (lib or L.load()).pss_welch_default_window(int(nperseg), _ptr(w)) != 0:
            raise ValueError("welch_default_window: nperseg in {256, 512, 1024, 2048, 4096}")
        return w

    @staticmethod
    def _welch_args(lib, nperseg, window, scaling, fs):
        """The defaults of welch / h_welch -> (window, scale), the scale computed in NumPy as SciPy does."""
        w = Engine.welch_default_window(nperseg, lib) if window is None else np.ascontiguousarray(window, np.float64)
        if w.shape != (int(nperseg),):
            raise ValueError("window: nperseg float64 values")
        if scaling == "density":
            scale = 1.0 / (float(fs) * (w * w).sum())
        elif scaling == "spectrum":
            scale = 1.0 / w.sum() ** 2
        else:
            raise ValueError("scaling: 'density' or 'spectrum'")
        return w, float(scale)

    def welch(self, d_iq, n_rows, n, nperseg, step, d_mean, d_max=None, window=None, detrend=True, scaling='density', fs=1.0, row_stride=None):
        """d_iq: n_rows rows of n complex64 samples, row_stride samples apart (default n) -> d_mean float64 [n_rows][nperseg]: SciPy's
        welch(x.astype(complex128), fs, window, nperseg, noverlap=nperseg - step, detrend='constant' | False, return_onesided=False,
        scaling=scaling), FFT order; d_max (optional): the max over the segments of the same periodograms
        (spectrogram(..., mode='psd').max(-1)).  window: host float64 [nperseg] (default: periodic Hann)."""
        w, scale = self._welch_args(self.lib, nperseg, window, scaling, fs)
        self._dev(self.lib.pss_welch, _ptr(d_iq), int(n_rows), int(n), int(n if row_stride is None else row_stride), int(nperseg), int(step), _ptr(w),
                  int(detrend), scale, _ptr(d_mean), _ptr(d_max))

    @staticmethod
    def h_welch(x, nperseg, step, window=None, detrend=True, scaling='density', fs=1.0, want_max=True, lib=None):
        """pss_h_welch: the same on a host array [n_rows][n] or [n] (complex64) -> (mean, max) float64 [n_rows][nperseg] or [nperseg]
        (max is None with want_max=False).  Pure host code; its transform is a radix-2 one, so it agrees with the device within the
        bound of tests/welch_bounds.py, not bit for bit."""
        lib = lib or L.load()
        x = np.asarray(x)
        if x.ndim not in (1, 2) or x.dtype != np.complex64:
            raise ValueError("x: a 1-D or 2-D complex64 array")
        rows = np.ascontiguousarray(x.reshape(-1, x.shape[-1]))
        w, scale = Engine._welch_args(lib, nperseg, window, scaling, fs)
        mean = np.empty((rows.shape[0], int(nperseg)), np.float64)
        mx = np.empty_like(mean) if want_max else None
        if lib.pss_h_welch(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(nperseg), int(step), _ptr(w), int(detrend), scale, _ptr(mean),
                           _ptr(mx)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        if x.ndim == 1:
            return mean[0], (mx[0] if want_max else None)
        return mean, mx

    # -- RDS for broadcast FM: rows of IQ -> groups (pss_rds_*; the arithmetic: csrc/pss_rds.h)
    @staticmethod
    def rds_plan(fs, lib=None):
        """pss_rds_plan -> (decim, up, down): the front's decimation min(fs // 19 000, 204) and the resampler's factors to 19 000 S/s.
        Host code."""
        lib = lib or L.load()
        d, u, w = C.c_int(), C.c_int(), C.c_int()
        if lib.pss_rds_plan(float(fs), C.byref(d), C.byref(u), C.byref(w)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return d.value, u.value, w.value

    @staticmethod
    def rds_default_pulse(span_bits=4, lib=None):
        """pss_rds_default_pulse: the biphase symbol's matched filter at 16 samples a bit, 16 span_bits + 1 float64 taps.  Host code."""
        return Engine._default_taps(lib, "pss_rds_default_pulse", "rds_default_pulse: span_bits outside [1, 16]", span_bits)

    @staticmethod
    def _rds_front_args(lib, n_buf, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride):
        """The defaults of rds_front / h_rds_front: ddc's, without the words."""
        _, taps, a, b, c, out_stride = Engine._ddc_args(lib, n_buf, np.zeros(1, np.uint64), decim, taps, buf_index0, n_capture, lead, m_begin, m_end,
                                                        out_stride)
        return taps, a, b[1], c, out_stride

    def rds_front(self, d_iq, n_rows, n_buf, fs, decim, d_out, taps=None, x_stride=None, buf_index0=0, n_capture=None, lead=None, m_begin=0,
                  m_end=None, out_stride=None):
        """d_iq complex64: n_rows rows x_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of n_capture
        samples -> d_out complex64: discriminator, 57 kHz mixer and decimating FIR, output m of row r at element r * out_stride +
        (m - m_begin).  taps, lead and the window: as ddc (default taps: ddc_default_taps(decim))."""
        taps, a, decim, c, out_stride = self._rds_front_args(self.lib, n_buf, decim, taps, buf_index0, n_capture, lead, m_begin, m_end, out_stride)
        self._dev(self.lib.pss_rds_front, _ptr(d_iq), int(n_rows), int(n_buf if x_stride is None else x_stride), *a, float(fs), decim, _ptr(taps), *c,
                  _ptr(d_out), out_stride)

    @staticmethod
    def h_rds_front(iq, fs, decim, taps=None, buf_index0=0, n_capture=None, lead=None, m_begin=0, m_end=None, lib=None):
        """pss_h_rds_front on a host array [n_rows][n_buf] or [n_buf] -> complex64 [n_rows][m_end - m_begin] or [m_end - m_begin].  Pure
        host code: the kernel's statements on one thread."""
        lib = lib or L.load()
        x = np.asarray(iq, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("iq: a 1-D or 2-D complex array")
        rows = Engine._as_rows(x)
        taps, a, decim, c, stride = Engine._rds_front_args(lib, rows.shape[1], decim, taps, buf_index0, n_capture, lead, m_begin, m_end, None)
        out = np.empty((rows.shape[0], max(stride, 0)), np.complex64)
        if lib.pss_h_rds_front(_ptr(rows), rows.shape[0], rows.shape[1], *a, float(fs), decim, _ptr(taps), *c, _ptr(out), stride) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return out if x.ndim == 2 else out[0]

    @staticmethod
    def _as_rows(x):
        """A 1-D array as one row, a 2-D array as it is (an empty one too) -> contiguous [n_rows][n]."""
        return np.ascontiguousarray(x[None, :] if x.ndim == 1 else x)

    @staticmethod
    def _rds_pulse(pulse, lib):
        return Engine.rds_default_pulse(4, lib) if pulse is None else np.ascontiguousarray(np.atleast_1d(pulse), np.float64)

    def rds_bits(self, d_bb, n_rows, n, d_bits, max_bits, d_n_bits, pulse=None, row_stride=None):
        """d_bb complex64: n_rows rows of n samples at 19 000 S/s, row_stride samples apart (default n) -> d_bits uint8 [n_rows][max_bits],
        d_n_bits int32 [n_rows] (the true count).  pulse: host float64 matched filter (default rds_default_pulse())."""
        pulse = self._rds_pulse(pulse, self.lib)
        self._dev(self.lib.pss_rds_bits, _ptr(d_bb), int(n_rows), int(n if row_stride is None else row_stride), int(n), _ptr(pulse), len(pulse),
                  _ptr(d_bits), int(max_bits), _ptr(d_n_bits))

    @staticmethod
    def rds_max_bits(n):
        """Room for every bit of a baseband row of n samples at 19 000 S/s: a strobe every 16 samples and one more per 64-bit segment."""
        return int(n) // 16 + int(n) // 1024 + 2

    @staticmethod
    def h_rds_bits(bb, pulse=None, max_bits=None, lib=None):
        """pss_h_rds_bits on a host array [n_rows][n] or [n] -> a list of uint8 bit rows (or one row).  Pure host code."""
        lib = lib or L.load()
        x = np.asarray(bb, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("bb: a 1-D or 2-D complex array")
        rows = Engine._as_rows(x)
        pulse = Engine._rds_pulse(pulse, lib)
        max_bits = Engine.rds_max_bits(rows.shape[1]) if max_bits is None else int(max_bits)
        bits = np.zeros((rows.shape[0], max(max_bits, 0)), np.uint8)
        n_bits = np.zeros(rows.shape[0], np.int32)
        if lib.pss_h_rds_bits(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], _ptr(pulse), len(pulse), _ptr(bits), max_bits, _ptr(n_bits)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        out = [bits[r, :min(int(n_bits[r]), max_bits)] for r in range(rows.shape[0])]
        return out if x.ndim == 2 else out[0]

    def rds_groups(self, d_bits, d_n_bits, n_rows, max_bits, d_groups, d_pos, max_groups, d_n_groups):
        """d_bits uint8 [n_rows][max_bits], d_n_bits int32 [n_rows] -> d_groups uint16 [n_rows][max_groups][4], d_pos int32
        [n_rows][max_groups], d_n_groups int32 [n_rows] (the true count; the first max_groups are kept)."""
        self._dev(self.lib.pss_rds_groups, _ptr(d_bits), _ptr(d_n_bits), int(n_rows), int(max_bits), _ptr(d_groups), _ptr(d_pos), int(max_groups),
                  _ptr(d_n_groups))

    @staticmethod
    def h_rds_groups(bits, n_bits=None, max_groups=None, lib=None):
        """pss_h_rds_groups on a host bit array [n_rows][max_bits] or [max_bits] (n_bits: the rows' counts, default max_bits) ->
        (groups uint16 [n_rows][max_groups][4], pos int32 [n_rows][max_groups], n_groups int32 [n_rows]), or one row's.  Pure host code."""
        lib = lib or L.load()
        b = np.asarray(bits, np.uint8)
        if b.ndim not in (1, 2):
            raise ValueError("bits: a 1-D or 2-D array")
        rows = Engine._as_rows(b)
        n_rows, max_bits = rows.shape
        nb = np.full(n_rows, max_bits, np.int32) if n_bits is None else np.ascontiguousarray(np.atleast_1d(n_bits), np.int32)
        if nb.shape != (n_rows,):
            raise ValueError("n_bits: one count per row")
        max_groups = max_bits // 104 + 1 if max_groups is None else int(max_groups)
        groups = np.zeros((n_rows, max(max_groups, 0), 4), np.uint16)
        pos = np.zeros((n_rows, max(max_groups, 0)), np.int32)
        n_groups = np.zeros(n_rows, np.int32)
        if lib.pss_h_rds_groups(_ptr(rows), _ptr(nb), n_rows, max_bits, _ptr(groups), _ptr(pos), max_groups, _ptr(n_groups)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return (groups, pos, n_groups) if b.ndim == 2 else (groups[0], pos[0], int(n_groups[0]))

    # -- ADS-B: a 1090 MHz capture -> the Mode S frames that pass their check (pss_adsb_*; the arithmetic: csrc/pss_adsb.h)
    @staticmethod
    def adsb_plan(fs, lib=None):
        """pss_adsb_plan -> spc, the samples of a 0.5 us chip: fs / 2 000 000, an integer in [1, 8].  Host code."""
        lib = lib or L.load()
        spc = C.c_int()
        if lib.pss_adsb_plan(float(fs), C.byref(spc)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return spc.value

    @staticmethod
    def adsb_crc(msg, n_bits=None, lib=None):
        """pss_adsb_crc: the 24-bit remainder of a message (bytes, or a uint8 array) under 0x1FFF409.  n_bits: default every byte.  Host code."""
        lib = lib or L.load()
        m = np.ascontiguousarray(np.frombuffer(bytes(msg), np.uint8) if isinstance(msg, (bytes, bytearray)) else msg, np.uint8)
        n_bits = 8 * len(m) if n_bits is None else int(n_bits)
        if m.ndim != 1 or n_bits < 0 or n_bits > min(8 * len(m), 112):
            raise ValueError("adsb_crc: n_bits outside the message, or above 112")
        return int(lib.pss_adsb_crc(_ptr(m), n_bits))

    def adsb_frames(self, d_iq, n_buf, spc, d_msg, d_pos, d_meta, d_score, d_count, max_frames, ratio=2.0, d_icao=None, n_icao=0, buf_index0=0,
                    n_capture=None, s_begin=0, s_end=None):
        """d_iq complex64: samples [buf_index0, buf_index0 + n_buf) of a capture of n_capture samples (default: the buffer is the capture) ->
        the frames that start in [s_begin, s_end) (default: to the capture's end), ascending: d_msg uint8 [max_frames][14], d_pos int64, d_meta
        uint32 (n_bits | DF << 16), d_score float32, d_count int32 [1] (the true count).  d_icao: n_icao ascending uint32 addresses ON THE
        DEVICE, against which the address-overlaid formats are checked."""
        n_capture = int(buf_index0) + int(n_buf) if n_capture is None else int(n_capture)
        s_end = n_capture if s_end is None else int(s_end)
        self._dev(self.lib.pss_adsb_frames, _ptr(d_iq), int(n_buf), int(buf_index0), n_capture, int(spc), float(ratio), _ptr(d_icao), int(n_icao),
                  int(s_begin), s_end, _ptr(d_msg), _ptr(d_pos), _ptr(d_meta), _ptr(d_score), _ptr(d_count), int(max_frames))

    @staticmethod
    def h_adsb_frames(iq, spc, ratio=2.0, icao=(), buf_index0=0, n_capture=None, s_begin=0, s_end=None, max_frames=None, lib=None):
        """pss_h_adsb_frames on a host complex64 array -> (msg uint8 [k][14], pos int64 [k], meta uint32 [k], score float32 [k], count): the
        first k = min(count, max_frames) records and the true count.  max_frames: default room for every frame the window can hold.  Pure
        host code."""
        lib = lib or L.load()
        x = np.ascontiguousarray(iq, np.complex64)
        if x.ndim != 1:
            raise ValueError("iq: a 1-D complex array")
        n_capture = int(buf_index0) + len(x) if n_capture is None else int(n_capture)
        s_end = n_capture if s_end is None else int(s_end)
        a = np.ascontiguousarray(icao, np.uint32).reshape(-1)
        grow = max_frames is None
        max_frames = 64 if grow else int(max_frames)
        while True:
            room = max(max_frames, 0)
            msg, pos, meta = np.zeros((room, 14), np.uint8), np.zeros(room, np.int64), np.zeros(room, np.uint32)
            score, count = np.zeros(room, np.float32), np.zeros(1, np.int32)
            if lib.pss_h_adsb_frames(_ptr(x), len(x), int(buf_index0), n_capture, int(spc), float(ratio), _ptr(a) if len(a) else None, len(a),
                                     int(s_begin), s_end, _ptr(msg), _ptr(pos), _ptr(meta), _ptr(score), _ptr(count), max_frames) != 0:
                raise ValueError(lib.pss_last_error(None).decode())
            if not grow or int(count[0]) <= room:
                break
            max_frames = int(count[0])   # the first run gave the true count
        k = min(int(count[0]), room)
        return msg[:k], pos[:k], meta[:k], score[:k], int(count[0])

    # -- AIS: rows of IQ at 48 kS/s -> the frames that pass their check (pss_ais_*; the arithmetic: csrc/pss_ais.h)
    @staticmethod
    def ais_plan(fs, lib=None):
        """pss_ais_plan -> (decim, up, down): the down-converter's decimation min(fs // 48 000, 204) and the resampler's factors to
        48 000 S/s.  Host code."""
        lib = lib or L.load()
        d, u, w = C.c_int(), C.c_int(), C.c_int()
        if lib.pss_ais_plan(float(fs), C.byref(d), C.byref(u), C.byref(w)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return d.value, u.value, w.value

    @staticmethod
    def ais_default_pulse(span_bits=2, lib=None):
        """pss_ais_default_pulse: a Gaussian of BT 0.4 at 5 samples a bit, 5 span_bits + 1 float64 taps of sum 1.  Host code."""
        return Engine._default_taps(lib, "pss_ais_default_pulse", "ais_default_pulse: span_bits outside [1, 12]", span_bits)

    @staticmethod
    def ais_crc(data, lib=None):
        """pss_ais_crc: the CRC-16/X.25 of bytes (or a uint8 array): 0x906E for b"123456789".  Host code."""
        lib = lib or L.load()
        m = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8)
        if m.ndim != 1:
            raise ValueError("ais_crc: a 1-D array of bytes")
        return int(lib.pss_ais_crc(_ptr(m) if len(m) else _ptr(np.zeros(1, np.uint8)), len(m)))

    @staticmethod
    def _ais_pulse(pulse, lib):
        return Engine.ais_default_pulse(2, lib) if pulse is None else np.ascontiguousarray(np.atleast_1d(pulse), np.float64)

    def ais_front(self, d_iq, n_rows, n_buf, d_y, pulse=None, x_stride=None, buf_index0=0, n_row=None, i_begin=0, i_end=None, y_stride=None):
        """d_iq complex64 at 48 kS/s: n_rows rows x_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of
        n_row samples (default: the buffer is the row) -> d_y float32: discriminator and post-filter, sample i of row r at element
        r * y_stride + (i - i_begin), i in [i_begin, i_end) (default: to the row's end; y_stride: default the window).  pulse: host float64
        table (default ais_default_pulse())."""
        pulse = self._ais_pulse(pulse, self.lib)
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        i_end = n_row if i_end is None else int(i_end)
        self._dev(self.lib.pss_ais_front, _ptr(d_iq), int(n_rows), int(n_buf if x_stride is None else x_stride), int(n_buf), int(buf_index0), n_row,
                  _ptr(pulse), len(pulse), int(i_begin), i_end, _ptr(d_y), int(i_end - int(i_begin) if y_stride is None else y_stride))

    @staticmethod
    def h_ais_front(iq, pulse=None, buf_index0=0, n_row=None, i_begin=0, i_end=None, lib=None):
        """pss_h_ais_front on a host array [n_rows][n_buf] or [n_buf] -> float32 [n_rows][i_end - i_begin] or [i_end - i_begin].  Pure host
        code: the kernel's statements on one thread."""
        lib = lib or L.load()
        x = np.asarray(iq, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("iq: a 1-D or 2-D complex array")
        rows = Engine._as_rows(x)
        pulse = Engine._ais_pulse(pulse, lib)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        i_end = n_row if i_end is None else int(i_end)
        width = i_end - int(i_begin)
        out = np.empty((rows.shape[0], max(width, 0)), np.float32)
        if lib.pss_h_ais_front(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, _ptr(pulse), len(pulse), int(i_begin),
                               i_end, _ptr(out), width) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return out if x.ndim == 2 else out[0]

    def ais_frames(self, d_y, n_rows, n_buf, d_msg, d_len, d_row, d_pos, d_score, d_count, max_frames, y_stride=None, buf_index0=0, n_row=None,
                   s_begin=0, s_end=None):
        """d_y float32 at 48 kS/s: n_rows rows y_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of n_row
        samples (default: the buffer is the row) -> the frames that start in [s_begin, s_end) (default: to the row's end) of every row, ascending
        in (row, s): d_msg uint8 [max_frames][128], d_len int32 (bytes with the two check bytes), d_row int32, d_pos int64, d_score float32,
        d_count int32 [1] (the true count)."""
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        self._dev(self.lib.pss_ais_frames, _ptr(d_y), int(n_rows), int(n_buf if y_stride is None else y_stride), int(n_buf), int(buf_index0), n_row,
                  int(s_begin), s_end, _ptr(d_msg), _ptr(d_len), _ptr(d_row), _ptr(d_pos), _ptr(d_score), _ptr(d_count), int(max_frames))

    @staticmethod
    def h_ais_frames(y, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, lib=None):
        """pss_h_ais_frames on a host float32 array [n_rows][n_buf] or [n_buf] -> (msg uint8 [k][128], len int32 [k], row int32 [k], pos int64
        [k], score float32 [k], count): the first k = min(count, max_frames) records and the true count.  max_frames: default room for every
        frame.  Pure host code."""
        lib = lib or L.load()
        x = np.asarray(y, np.float32)
        if x.ndim not in (1, 2):
            raise ValueError("y: a 1-D or 2-D float32 array")
        rows = Engine._as_rows(x)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        grow = max_frames is None
        max_frames = 64 if grow else int(max_frames)
        while True:
            room = max(max_frames, 0)
            msg, ln, rw = np.zeros((room, 128), np.uint8), np.zeros(room, np.int32), np.zeros(room, np.int32)
            pos, score, count = np.zeros(room, np.int64), np.zeros(room, np.float32), np.zeros(1, np.int32)
            if lib.pss_h_ais_frames(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, int(s_begin), s_end, _ptr(msg),
                                    _ptr(ln), _ptr(rw), _ptr(pos), _ptr(score), _ptr(count), max_frames) != 0:
                raise ValueError(lib.pss_last_error(None).decode())
            if not grow or int(count[0]) <= room:
                break
            max_frames = int(count[0])   # the first run gave the true count
        k = min(int(count[0]), room)
        return msg[:k], ln[:k], rw[:k], pos[:k], score[:k], int(count[0])

    # -- packet radio: rows of IQ at 26.4 kS/s -> the AX.25 frames that pass their check (pss_packet_*; the arithmetic: csrc/pss_packet.h)
    PACKET_RATE = 26400
    PACKET_REC_BYTES = 332

    @staticmethod
    def packet_plan(fs, lib=None):
        """pss_packet_plan -> (decim, up, down): the down-converter's decimation min(fs // 26 400, 204) and the resampler's factors to
        26 400 S/s.  Host code."""
        lib = lib or L.load()
        d, u, w = C.c_int(), C.c_int(), C.c_int()
        if lib.pss_packet_plan(float(fs), C.byref(d), C.byref(u), C.byref(w)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return d.value, u.value, w.value

    @staticmethod
    def packet_default_tones(lib=None):
        """pss_packet_default_tones: float64 [4][22]: cos and sin of 1200 Hz, cos and sin of 2200 Hz over a bit of 22 samples.  Host code."""
        lib = lib or L.load()
        t = np.empty((4, 22), np.float64)
        r = lib.pss_packet_default_tones(_ptr(t))
        if r != 0:
            raise PssError(r, "pss_packet_default_tones")
        return t

    @staticmethod
    def _packet_tones(tones, lib):
        if tones is None:
            return Engine.packet_default_tones(lib)
        t = np.ascontiguousarray(tones, np.float64)
        if t.shape != (4, 22):
            raise ValueError("tones: a float64 table [4][22]")
        return t

    def packet_front(self, d_iq, n_rows, n_buf, d_z, tones=None, space_gain=1.0, x_stride=None, buf_index0=0, n_row=None, i_begin=0, i_end=None,
                     z_stride=None):
        """d_iq complex64 at 26.4 kS/s: n_rows rows x_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of
        n_row samples (default: the buffer is the row) -> d_z float32: the tone balance (space minus mark over their sum), sample i of row r at
        element r * z_stride + (i - i_begin), i in [i_begin, i_end) (default: to the row's end; z_stride: default the window).  tones: host
        float64 table [4][22] (default packet_default_tones()); space_gain: the weight of the 2200 Hz energy."""
        tones = self._packet_tones(tones, self.lib)
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        i_end = n_row if i_end is None else int(i_end)
        self._dev(self.lib.pss_packet_front, _ptr(d_iq), int(n_rows), int(n_buf if x_stride is None else x_stride), int(n_buf), int(buf_index0), n_row,
                  _ptr(tones), float(space_gain), int(i_begin), i_end, _ptr(d_z), int(i_end - int(i_begin) if z_stride is None else z_stride))

    @staticmethod
    def h_packet_front(iq, tones=None, space_gain=1.0, buf_index0=0, n_row=None, i_begin=0, i_end=None, lib=None):
        """pss_h_packet_front on a host array [n_rows][n_buf] or [n_buf] -> float32 [n_rows][i_end - i_begin] or [i_end - i_begin].  Pure host
        code: the kernel's statements on one thread."""
        lib = lib or L.load()
        x = np.asarray(iq, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("iq: a 1-D or 2-D complex array")
        rows = Engine._as_rows(x)
        tones = Engine._packet_tones(tones, lib)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        i_end = n_row if i_end is None else int(i_end)
        width = i_end - int(i_begin)
        out = np.empty((rows.shape[0], max(width, 0)), np.float32)
        if lib.pss_h_packet_front(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, _ptr(tones), float(space_gain),
                                  int(i_begin), i_end, _ptr(out), width) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return out if x.ndim == 2 else out[0]

    def packet_frames(self, d_z, n_rows, n_buf, d_msg, d_len, d_row, d_pos, d_score, d_count, max_frames, q_min=0.0, z_stride=None, buf_index0=0,
                      n_row=None, s_begin=0, s_end=None):
        """d_z float32 at 26.4 kS/s: n_rows rows z_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of
        n_row samples (default: the buffer is the row) -> the frames whose flag starts in [s_begin, s_end) (default: to the row's end) of every
        row, ascending in (row, s): d_msg uint8 [max_frames][332], d_len int32 (bytes with the two check bytes), d_row int32, d_pos int64,
        d_score float32, d_count int32 [1] (the true count).  q_min: the smallest |z| a flag's strobes may show."""
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        self._dev(self.lib.pss_packet_frames, _ptr(d_z), int(n_rows), int(n_buf if z_stride is None else z_stride), int(n_buf), int(buf_index0), n_row,
                  int(s_begin), s_end, float(q_min), _ptr(d_msg), _ptr(d_len), _ptr(d_row), _ptr(d_pos), _ptr(d_score), _ptr(d_count), int(max_frames))

    @staticmethod
    def h_packet_frames(z, q_min=0.0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, lib=None):
        """pss_h_packet_frames on a host float32 array [n_rows][n_buf] or [n_buf] -> (msg uint8 [k][332], len int32 [k], row int32 [k], pos
        int64 [k], score float32 [k], count): the first k = min(count, max_frames) records and the true count.  max_frames: default room for
        every frame.  Pure host code."""
        lib = lib or L.load()
        x = np.asarray(z, np.float32)
        if x.ndim not in (1, 2):
            raise ValueError("z: a 1-D or 2-D float32 array")
        rows = Engine._as_rows(x)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        grow = max_frames is None
        max_frames = 64 if grow else int(max_frames)
        while True:
            room = max(max_frames, 0)
            msg, ln, rw = np.zeros((room, 332), np.uint8), np.zeros(room, np.int32), np.zeros(room, np.int32)
            pos, score, count = np.zeros(room, np.int64), np.zeros(room, np.float32), np.zeros(1, np.int32)
            if lib.pss_h_packet_frames(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, int(s_begin), s_end, float(q_min),
                                       _ptr(msg), _ptr(ln), _ptr(rw), _ptr(pos), _ptr(score), _ptr(count), max_frames) != 0:
                raise ValueError(lib.pss_last_error(None).decode())
            if not grow or int(count[0]) <= room:
                break
            max_frames = int(count[0])   # the first run gave the true count
        k = min(int(count[0]), room)
        return msg[:k], ln[:k], rw[:k], pos[:k], score[:k], int(count[0])

    # -- POCSAG: float32 discriminator rows at 38.4 kS/s -> the batches whose codewords pass their check (pss_pocsag_*; the arithmetic:
    #    csrc/pss_pocsag.h).  The front is ais_front with pocsag_default_pulse(spb).
    POCSAG_RATE = 38400
    POCSAG_SYNC, POCSAG_IDLE = 0x7CD215D8, 0x7A89C197

    @staticmethod
    def pocsag_plan(fs, lib=None):
        """pss_pocsag_plan -> (decim, up, down): the down-converter's decimation min(fs // 38 400, 204) and the resampler's factors to
        38 400 S/s.  Host code."""
        lib = lib or L.load()
        d, u, w = C.c_int(), C.c_int(), C.c_int()
        if lib.pss_pocsag_plan(float(fs), C.byref(d), C.byref(u), C.byref(w)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return d.value, u.value, w.value

    @staticmethod
    def pocsag_default_pulse(spb, lib=None):
        """pss_pocsag_default_pulse: a boxcar of the largest odd number of taps <= min(spb, 65), each 1 / P (float64).  Host code."""
        return Engine._default_taps(lib, "pss_pocsag_default_pulse", "pocsag_default_pulse: spb outside [2, 128]", spb)

    @staticmethod
    def pocsag_codeword(data21, lib=None):
        """pss_pocsag_codeword: the 32-bit codeword of 21 data bits (BCH(31,21) and even parity).  Host code."""
        lib = lib or L.load()
        return int(lib.pss_pocsag_codeword(int(data21) & 0x1FFFFF))

    @staticmethod
    def pocsag_check(cw, fix=2, lib=None):
        """pss_pocsag_check -> (bits fixed, corrected codeword), or (-1, 0): uncorrectable within `fix` bits.  Host code."""
        lib = lib or L.load()
        out = C.c_uint32()
        n = int(lib.pss_pocsag_check(int(cw) & 0xFFFFFFFF, int(fix), C.byref(out)))
        return n, int(out.value)

    def pocsag_batches(self, d_y, n_rows, n_buf, spb, d_cw, d_fix, d_row, d_pos, d_meta, d_score, d_count, max_batches, sync_errors=2, fix=2, max_bad=0,
                       y_stride=None, buf_index0=0, n_row=None, s_begin=0, s_end=None):
        """d_y float32 at 38.4 kS/s: n_rows rows y_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of n_row
        samples (default: the buffer is the row) -> the batches whose sync word starts in [s_begin, s_end) (default: to the row's end) of every
        row, ascending in (row, s): d_cw uint32 [max_batches][16], d_fix uint8 [max_batches][16], d_row int32, d_pos int64, d_meta uint32 (sync
        mismatches | inverted << 8 | n_bad << 16 | fixed bits << 24), d_score float32, d_count int32 [1] (the true count)."""
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        self._dev(self.lib.pss_pocsag_batches, _ptr(d_y), int(n_rows), int(n_buf if y_stride is None else y_stride), int(n_buf), int(buf_index0), n_row,
                  int(s_begin), s_end, int(spb), int(sync_errors), int(fix), int(max_bad), _ptr(d_cw), _ptr(d_fix), _ptr(d_row), _ptr(d_pos), _ptr(d_meta),
                  _ptr(d_score), _ptr(d_count), int(max_batches))

    @staticmethod
    def h_pocsag_batches(y, spb, sync_errors=2, fix=2, max_bad=0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_batches=None, lib=None):
        """pss_h_pocsag_batches on a host float32 array [n_rows][n_buf] or [n_buf] -> (cw uint32 [k][16], fix uint8 [k][16], row int32 [k], pos
        int64 [k], meta uint32 [k], score float32 [k], count): the first k = min(count, max_batches) records and the true count.  max_batches:
        default room for every batch.  Pure host code."""
        lib = lib or L.load()
        x = np.asarray(y, np.float32)
        if x.ndim not in (1, 2):
            raise ValueError("y: a 1-D or 2-D float32 array")
        rows = Engine._as_rows(x)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        grow = max_batches is None
        max_batches = 64 if grow else int(max_batches)
        while True:
            room = max(max_batches, 0)
            cw, fx, rw = np.zeros((room, 16), np.uint32), np.zeros((room, 16), np.uint8), np.zeros(room, np.int32)
            pos, meta, score, count = np.zeros(room, np.int64), np.zeros(room, np.uint32), np.zeros(room, np.float32), np.zeros(1, np.int32)
            if lib.pss_h_pocsag_batches(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, int(s_begin), s_end, int(spb),
                                        int(sync_errors), int(fix), int(max_bad), _ptr(cw), _ptr(fx), _ptr(rw), _ptr(pos), _ptr(meta), _ptr(score),
                                        _ptr(count), max_batches) != 0:
                raise ValueError(lib.pss_last_error(None).decode())
            if not grow or int(count[0]) <= room:
                break
            max_batches = int(count[0])   # the first run gave the true count
        k = min(int(count[0]), room)
        return cw[:k], fx[:k], rw[:k], pos[:k], meta[:k], score[:k], int(count[0])

    # -- FLEX: float32 discriminator rows at 38.4 kS/s -> the frames whose words pass their check (pss_flex_*; the arithmetic:
    #    csrc/pss_flex.h).  The front is ais_front with flex_default_pulse(h), one pass for both baud rates.
    FLEX_MARKER = 0xA6C6AAAA
    FLEX_MODES = ((0x870C, 1600, 2), (0xB068, 1600, 4), (0x7B18, 3200, 2), (0xDEA0, 3200, 4), (0x4C7C, 3200, 4))   # code, baud, levels

    @staticmethod
    def flex_default_pulse(h, lib=None):
        """pss_flex_default_pulse: a boxcar of the largest odd number of taps <= h (h in [1, 64]), each 1 / P (float64).  Host code."""
        return Engine._default_taps(lib, "pss_flex_default_pulse", "flex_default_pulse: h outside [1, 64]", h)

    @staticmethod
    def flex_word(data21, lib=None):
        """pss_flex_word: the 32-bit word of 21 data bits (data in bits 0 .. 20, BCH(31,21) in 21 .. 30, even parity in 31).  Host code."""
        lib = lib or L.load()
        return int(lib.pss_flex_word(int(data21) & 0x1FFFFF))

    def flex_frames(self, d_y, n_rows, n_buf, h, d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, d_count, max_frames, sync_errors=2, fix=2,
                    max_bad=0, y_stride=None, buf_index0=0, n_row=None, s_begin=0, s_end=None):
        """d_y float32: n_rows rows y_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of n_row samples
        (default: the buffer is the row), h samples a 3200-baud symbol -> the frames whose sync starts in [s_begin, s_end) (default: to the
        row's end) of every row, ascending in (row, s): d_words uint32 [max_frames][4][88], d_fix uint8 [max_frames][4][88], d_fiw uint32,
        d_row int32, d_pos int64, d_meta uint32 [max_frames][2] (mismatches | inverted << 8 | mode << 12 | FIW fixed bits << 16; n_bad |
        fixed bits << 16), d_score float32, d_count int32 [1] (the true count)."""
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        self._dev(self.lib.pss_flex_frames, _ptr(d_y), int(n_rows), int(n_buf if y_stride is None else y_stride), int(n_buf), int(buf_index0), n_row,
                  int(s_begin), s_end, int(h), int(sync_errors), int(fix), int(max_bad), _ptr(d_words), _ptr(d_fix), _ptr(d_fiw), _ptr(d_row), _ptr(d_pos),
                  _ptr(d_meta), _ptr(d_score), _ptr(d_count), int(max_frames))

    @staticmethod
    def h_flex_frames(y, h, sync_errors=2, fix=2, max_bad=0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, lib=None):
        """pss_h_flex_frames on a host float32 array [n_rows][n_buf] or [n_buf] -> (words uint32 [k][4][88], fix uint8 [k][4][88], fiw uint32
        [k], row int32 [k], pos int64 [k], meta uint32 [k][2], score float32 [k], count): the first k = min(count, max_frames) records and
        the true count.  max_frames: default room for every frame.  Pure host code."""
        lib = lib or L.load()
        x = np.asarray(y, np.float32)
        if x.ndim not in (1, 2):
            raise ValueError("y: a 1-D or 2-D float32 array")
        rows = Engine._as_rows(x)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        grow = max_frames is None
        max_frames = 16 if grow else int(max_frames)
        while True:
            room = max(max_frames, 0)
            words, fx, fiw = np.zeros((room, 4, 88), np.uint32), np.zeros((room, 4, 88), np.uint8), np.zeros(room, np.uint32)
            rw, pos, meta = np.zeros(room, np.int32), np.zeros(room, np.int64), np.zeros((room, 2), np.uint32)
            score, count = np.zeros(room, np.float32), np.zeros(1, np.int32)
            if lib.pss_h_flex_frames(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, int(s_begin), s_end, int(h),
                                     int(sync_errors), int(fix), int(max_bad), _ptr(words), _ptr(fx), _ptr(fiw), _ptr(rw), _ptr(pos), _ptr(meta),
                                     _ptr(score), _ptr(count), max_frames) != 0:
                raise ValueError(lib.pss_last_error(None).decode())
            if not grow or int(count[0]) <= room:
                break
            max_frames = int(count[0])   # the first run gave the true count
        k = min(int(count[0]), room)
        return words[:k], fx[:k], fiw[:k], rw[:k], pos[:k], meta[:k], score[:k], int(count[0])

    # -- OOK devices: complex64 rows -> the envelope (a stage dump), the block means the thresholds come from, the sliced messages
    #    (pss_ook_*; the arithmetic: csrc/pss_ook.h).  spec: formats.ook_spec's dict, every length in samples.
    OOK_PWM, OOK_PPM, OOK_MC = 0, 1, 2
    OOK_OPEN, OOK_LONG, OOK_MANY, OOK_FULL = 1 << 22, 1 << 23, 1 << 24, 1 << 25
    OOK_MAX_PULSES, OOK_MAX_BITS, OOK_BLOCK = 1024, 256, 4096

    @staticmethod
    def ook_halo(P, R, gap_limit, span, lib=None):
        """pss_ook_halo -> (before, after): the samples a window of ook_messages reads back from s_begin and on from s_end.  Host code."""
        lib = lib or L.load()
        b, a = C.c_long(), C.c_long()
        if lib.pss_ook_halo(int(P), int(R), int(gap_limit), int(span), C.byref(b), C.byref(a)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return b.value, a.value

    @staticmethod
    def _ook_spec_args(spec):
        return (int(spec['gap_limit']), int(spec['span']), int(spec['mode']), int(spec['short']), int(spec.get('long', 0)), int(spec.get('sync', 0)),
                int(spec['tol']), int(spec.get('phase', 0)), int(spec.get('invert', 0)), int(spec.get('min_bits', 0)), int(spec.get('max_odd', 0)))

    def ook_envelope(self, d_iq, n_rows, n_buf, d_env, P=9, x_stride=None, buf_index0=0, n_row=None, i_begin=0, i_end=None, env_stride=None):
        """d_iq complex64: n_rows rows x_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of n_row samples
        (default: the buffer is the row) -> d_env float32 [n_rows][env_stride]: the envelope of the samples [i_begin, i_end)."""
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        i_end = n_row if i_end is None else int(i_end)
        self._dev(self.lib.pss_ook_envelope, _ptr(d_iq), int(n_rows), int(n_buf if x_stride is None else x_stride), int(n_buf), int(buf_index0), n_row, int(P),
                  int(i_begin), i_end, _ptr(d_env), int(i_end - int(i_begin) if env_stride is None else env_stride))

    def ook_levels(self, d_iq, n_rows, n_buf, d_means, x_stride=None, buf_index0=0, n_row=None, b_begin=0, b_end=None, means_stride=None):
        """-> d_means float64 [n_rows][means_stride]: the mean of m over the whole blocks [b_begin, b_end) of 4096 samples (default: every
        whole block of the row)."""
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        b_end = n_row // self.OOK_BLOCK if b_end is None else int(b_end)
        self._dev(self.lib.pss_ook_levels, _ptr(d_iq), int(n_rows), int(n_buf if x_stride is None else x_stride), int(n_buf), int(buf_index0), n_row,
                  int(b_begin), b_end, _ptr(d_means), int(b_end - int(b_begin) if means_stride is None else means_stride))

    def ook_messages(self, d_iq, n_rows, n_buf, hi, lo, spec, d_bits, d_n_bits, d_row, d_pos, d_span, d_meta, d_count, max_msgs, P=9, R=64, x_stride=None,
                     buf_index0=0, n_row=None, s_begin=0, s_end=None):
        """-> the messages whose first rise lies in [s_begin, s_end) (default: to the row's end) of every row, ascending in (row, pos): d_bits
        uint8 [max_msgs][32], d_n_bits int32, d_row int32, d_pos int64, d_span int32, d_meta uint32 (pulses | n_odd << 11 | flags), d_count
        int32 [1] (the true count)."""
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        self._dev(self.lib.pss_ook_messages, _ptr(d_iq), int(n_rows), int(n_buf if x_stride is None else x_stride), int(n_buf), int(buf_index0), n_row,
                  int(s_begin), s_end, int(P), float(hi), float(lo), int(R), *self._ook_spec_args(spec), _ptr(d_bits), _ptr(d_n_bits), _ptr(d_row),
                  _ptr(d_pos), _ptr(d_span), _ptr(d_meta), _ptr(d_count), int(max_msgs))

    @staticmethod
    def _ook_rows(iq):
        x = np.asarray(iq, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("iq: a 1-D or 2-D complex64 array")
        return Engine._as_rows(x)

    @staticmethod
    def h_ook_envelope(iq, P=9, buf_index0=0, n_row=None, i_begin=0, i_end=None, lib=None):
        """pss_h_ook_envelope on a host complex64 array [n_rows][n_buf] or [n_buf] -> float32 [n_rows][i_end - i_begin].  Pure host code."""
        lib = lib or L.load()
        rows = Engine._ook_rows(iq)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        i_end = n_row if i_end is None else int(i_end)
        env = np.zeros((rows.shape[0], max(i_end - int(i_begin), 0)), np.float32)
        if lib.pss_h_ook_envelope(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, int(P), int(i_begin), i_end, _ptr(env),
                                  env.shape[1]) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return env

    @staticmethod
    def h_ook_levels(iq, buf_index0=0, n_row=None, b_begin=0, b_end=None, lib=None):
        """pss_h_ook_levels on a host complex64 array -> float64 [n_rows][b_end - b_begin].  Pure host code."""
        lib = lib or L.load()
        rows = Engine._ook_rows(iq)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        b_end = n_row // Engine.OOK_BLOCK if b_end is None else int(b_end)
        means = np.zeros((rows.shape[0], max(b_end - int(b_begin), 0)), np.float64)
        if lib.pss_h_ook_levels(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, int(b_begin), b_end, _ptr(means),
                                means.shape[1]) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return means

    @staticmethod
    def h_ook_messages(iq, hi, lo, spec, P=9, R=64, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_msgs=None, lib=None):
        """pss_h_ook_messages on a host complex64 array [n_rows][n_buf] or [n_buf] -> (bits uint8 [k][32], n_bits int32 [k], row int32 [k], pos
        int64 [k], span int32 [k], meta uint32 [k], count): the first k = min(count, max_msgs) records and the true count.  max_msgs: default
        room for every message.  Pure host code."""
        lib = lib or L.load()
        rows = Engine._ook_rows(iq)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        grow = max_msgs is None
        max_msgs = 64 if grow else int(max_msgs)
        while True:
            room = max(max_msgs, 0)
            bits, nb, rw = np.zeros((room, 32), np.uint8), np.zeros(room, np.int32), np.zeros(room, np.int32)
            pos, sp, meta, count = np.zeros(room, np.int64), np.zeros(room, np.int32), np.zeros(room, np.uint32), np.zeros(1, np.int32)
            if lib.pss_h_ook_messages(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, int(s_begin), s_end, int(P), float(hi),
                                      float(lo), int(R), *Engine._ook_spec_args(spec), _ptr(bits), _ptr(nb), _ptr(rw), _ptr(pos), _ptr(sp), _ptr(meta),
                                      _ptr(count), max_msgs) != 0:
                raise ValueError(lib.pss_last_error(None).decode())
            if not grow or int(count[0]) <= room:
                break
            max_msgs = int(count[0])   # the first run gave the true count
        k = min(int(count[0]), room)
        return bits[:k], nb[:k], rw[:k], pos[:k], sp[:k], meta[:k], int(count[0])

    # -- NOAA APT: complex64 rows at 62.4 kS/s -> the envelope, the line starts, the lines' words (pss_apt_*; the arithmetic: csrc/pss_apt.h)
    APT_RATE = 62400
    APT_ENV_RATE = 12480
    APT_DECIM = 5
    APT_LINE_WORDS, APT_LINE_ENV = 2080, 6240

    @staticmethod
    def apt_plan(fs, lib=None):
        """pss_apt_plan -> (decim, up, down): the down-converter's decimation min(fs // 62 400, 204) and the resampler's factors to
        62 400 S/s.  Host code."""
        lib = lib or L.load()
        d, u, w = C.c_int(), C.c_int(), C.c_int()
        if lib.pss_apt_plan(float(fs), C.byref(d), C.byref(u), C.byref(w)) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return d.value, u.value, w.value

    @staticmethod
    def apt_default_taps(lib=None):
        """pss_apt_default_taps: the front's low-pass, scipy.signal.firwin(79, 1 / 15) bit for bit (float64).  Host code."""
        return Engine._default_taps(lib, "pss_apt_default_taps", "apt_default_taps")

    @staticmethod
    def _apt_front_args(lib, n_buf, decim, taps, buf_index0, n_row, lead, m_begin, m_end, env_stride):
        """The defaults of apt_front / h_apt_front: ddc's, without the words, and the receiver's own taps."""
        taps = Engine.apt_default_taps(lib) if taps is None else taps
        return Engine._rds_front_args(lib, n_buf, decim, taps, buf_index0, n_row, lead, m_begin, m_end, env_stride)

    def apt_front(self, d_iq, n_rows, n_buf, d_env, fs=APT_RATE, decim=APT_DECIM, taps=None, x_stride=None, buf_index0=0, n_row=None, lead=None,
                  m_begin=0, m_end=None, env_stride=None):
        """d_iq complex64: n_rows rows x_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of n_row
        samples -> d_env float32: discriminator, 2400 Hz mixer, decimating FIR and magnitude, output m of row r at element r * env_stride +
        (m - m_begin).  taps (default apt_default_taps()), lead and the window: as ddc."""
        taps, a, decim, c, env_stride = self._apt_front_args(self.lib, n_buf, decim, taps, buf_index0, n_row, lead, m_begin, m_end, env_stride)
        self._dev(self.lib.pss_apt_front, _ptr(d_iq), int(n_rows), int(n_buf if x_stride is None else x_stride), *a, float(fs), decim, _ptr(taps), *c,
                  _ptr(d_env), env_stride)

    @staticmethod
    def h_apt_front(iq, fs=APT_RATE, decim=APT_DECIM, taps=None, buf_index0=0, n_row=None, lead=None, m_begin=0, m_end=None, lib=None):
        """pss_h_apt_front on a host array [n_rows][n_buf] or [n_buf] -> float32 [n_rows][m_end - m_begin] or [m_end - m_begin].  Pure host
        code: the kernel's statements on one thread."""
        lib = lib or L.load()
        x = np.asarray(iq, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("iq: a 1-D or 2-D complex array")
        rows = Engine._as_rows(x)
        taps, a, decim, c, stride = Engine._apt_front_args(lib, rows.shape[1], decim, taps, buf_index0, n_row, lead, m_begin, m_end, None)
        out = np.empty((rows.shape[0], max(stride, 0)), np.float32)
        if lib.pss_h_apt_front(_ptr(rows), rows.shape[0], rows.shape[1], *a, float(fs), decim, _ptr(taps), *c, _ptr(out), stride) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return out if x.ndim == 2 else out[0]

    def apt_syncs(self, d_env, n_rows, n_buf, d_row, d_pos, d_meta, d_score, d_count, max_syncs, sync_errors=2, e_stride=None, buf_index0=0,
                  n_row=None, s_begin=0, s_end=None):
        """d_env float32 at 12.48 kS/s: n_rows rows e_stride samples apart (default n_buf), samples [buf_index0, buf_index0 + n_buf) of rows of
        n_row samples (default: the buffer is the row) -> the line starts in [s_begin, s_end) (default: to the row's end) of every row,
        ascending in (row, s): d_row int32, d_pos int64, d_meta uint32 (mismatches), d_score float32, d_count int32 [1] (the true count)."""
        n_row = int(buf_index0) + int(n_buf) if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        self._dev(self.lib.pss_apt_syncs, _ptr(d_env), int(n_rows), int(n_buf if e_stride is None else e_stride), int(n_buf), int(buf_index0), n_row,
                  int(s_begin), s_end, int(sync_errors), _ptr(d_row), _ptr(d_pos), _ptr(d_meta), _ptr(d_score), _ptr(d_count), int(max_syncs))

    @staticmethod
    def h_apt_syncs(env, sync_errors=2, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_syncs=None, lib=None):
        """pss_h_apt_syncs on a host float32 array [n_rows][n_buf] or [n_buf] -> (row int32 [k], pos int64 [k], meta uint32 [k], score
        float32 [k], count): the first k = min(count, max_syncs) records and the true count.  max_syncs: default room for every record.
        Pure host code."""
        lib = lib or L.load()
        x = np.asarray(env, np.float32)
        if x.ndim not in (1, 2):
            raise ValueError("env: a 1-D or 2-D float32 array")
        rows = Engine._as_rows(x)
        n_row = int(buf_index0) + rows.shape[1] if n_row is None else int(n_row)
        s_end = n_row if s_end is None else int(s_end)
        grow = max_syncs is None
        max_syncs = 64 if grow else int(max_syncs)
        while True:
            room = max(max_syncs, 0)
            rw, pos = np.zeros(room, np.int32), np.zeros(room, np.int64)
            meta, score, count = np.zeros(room, np.uint32), np.zeros(room, np.float32), np.zeros(1, np.int32)
            if lib.pss_h_apt_syncs(_ptr(rows), rows.shape[0], rows.shape[1], rows.shape[1], int(buf_index0), n_row, int(s_begin), s_end,
                                   int(sync_errors), _ptr(rw), _ptr(pos), _ptr(meta), _ptr(score), _ptr(count), max_syncs) != 0:
                raise ValueError(lib.pss_last_error(None).decode())
            if not grow or int(count[0]) <= room:
                break
            max_syncs = int(count[0])   # the first run gave the true count
        k = min(int(count[0]), room)
        return rw[:k], pos[:k], meta[:k], score[:k], int(count[0])

    def apt_lines(self, d_env, n_rows, n_row, d_line_row, d_line_pos, n_lines, d_words, e_stride=None, words_stride=None):
        """d_env float32 [n_rows] rows of n_row samples, e_stride apart (default n_row); d_line_row int32 and d_line_pos int64 [n_lines] ->
        d_words float32, word j of line l at element l * words_stride (default 2080) + j: env[pos + 3 j + 1], +0 outside the row."""
        self._dev(self.lib.pss_apt_lines, _ptr(d_env), int(n_rows), int(n_row if e_stride is None else e_stride), int(n_row), _ptr(d_line_row),
                  _ptr(d_line_pos), int(n_lines), _ptr(d_words), int(self.APT_LINE_WORDS if words_stride is None else words_stride))

    @staticmethod
    def h_apt_lines(env, line_row, line_pos, lib=None):
        """pss_h_apt_lines on a host float32 array [n_rows][n_row] or [n_row] -> float32 [n_lines][2080].  Pure host code."""
        lib = lib or L.load()
        x = np.asarray(env, np.float32)
        if x.ndim not in (1, 2):
            raise ValueError("env: a 1-D or 2-D float32 array")
        rows = Engine._as_rows(x)
        lr = np.ascontiguousarray(np.atleast_1d(line_row), np.int32)
        lp = np.ascontiguousarray(np.atleast_1d(line_pos), np.int64)
        if lr.shape != lp.shape or lr.ndim != 1:
            raise ValueError("line_row and line_pos: 1-D lists of one length")
        words = np.zeros((len(lp), Engine.APT_LINE_WORDS), np.float32)
        if lib.pss_h_apt_lines(_ptr(rows), max(rows.shape[0], 1), rows.shape[1], rows.shape[1], _ptr(lr), _ptr(lp), len(lp), _ptr(words),
                               Engine.APT_LINE_WORDS) != 0:
            raise ValueError(lib.pss_last_error(None).decode())
        return words

    def afsk_bits(self, d_audio, n_rows, n, fs, d_bits, sos1200=None, sos2200=None):
        c = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
        s1, s2 = c(sos1200), c(sos2200)
        self._dev(self.lib.pss_afsk_bits, _ptr(d_audio), n_rows, n, float(fs), _ptr(s1), _ptr(s2),
                                        5 if s1 is None else s1.shape[0], _ptr(d_bits))

    def h_afsk_bits(self, x, fs, sos1200=None, sos2200=None, normalise=False):
        """decode_afsk's bit list for one host buffer of real audio (float64) -> uint8 array; normalise=True divides by
        max|x| on the device first (what decode_aprs does before it calls decode_afsk, decoders.py:126)."""
        x = np.ascontiguousarray(x, np.float64)
        nb = self.afsk_n_bits(len(x), fs)
        if nb <= 0:
            return np.zeros(0, np.uint8)
        bits = np.empty(nb, np.uint8)
        s1 = None if sos1200 is None else np.ascontiguousarray(sos1200, np.float64)
        s2 = None if sos2200 is None else np.ascontiguousarray(sos2200, np.float64)
        self._ck(self.lib.pss_h_afsk_bits(self.h, _ptr(x), len(x), float(fs), int(bool(normalise)), _ptr(s1), _ptr(s2),
                                          0 if s1 is None else s1.shape[0], _ptr(bits)))
        return bits

    def np_f32(self, op, d_a, d_b, n, d_out):
        """NumPy's float32 arctan2 (op 0) / log10 (1) / abs of a + ib (2), element by element (pss_np_f32)."""
        self._dev(self.lib.pss_np_f32, int(op), _ptr(d_a), _ptr(d_b), int(n), _ptr(d_out))

    def row_normalise(self, d_x, n_rows, n, d_y):
        self._dev(self.lib.pss_row_normalise, _ptr(d_x), n_rows, n, _ptr(d_y))

    def afsk_n_bits(self, n, fs):
        return self.lib.pss_afsk_n_bits(int(n), float(fs))

    def h_bandpass_filter(self, data, lowcut, highcut, fs, sos=None):
        x = np.ascontiguousarray(data, np.float64)
        y = np.empty_like(x)
        if sos is not None:
            sos = np.ascontiguousarray(sos, np.float64)
        self._ck(self.lib.pss_h_bandpass_filter(self.h, _ptr(x), len(x), float(lowcut), float(highcut), float(fs),
                                                _ptr(sos), 0 if sos is None else sos.shape[0], _ptr(y)))
        return y

    def h_measure_power(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64)
        out = np.empty(1, np.float32)
        self._ck(self.lib.pss_h_measure_power(self.h, _ptr(iq), len(iq), _ptr(out)))
        return out[0]

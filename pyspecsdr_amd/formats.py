"""The data formats either side of the hot path, so that real captures can replace synthetic IQ:

  * IQ recordings     — `record_signal` / `play_recorded_signal` (pyspecsdr.py:814-824): `np.save` of the 1-D complex64 read
                        buffer (SoapySDR CF32, interleaved I/Q float32 — pyspecsdr.py:1870-1891);
  * audio recordings  — `start_audio_recording` / `write_audio_samples` (audio_processing.py:25-43): RIFF/WAVE, 2 channels,
                        16-bit, `np.int16(samples * 32767)`;
  * raw code files    — what `rtl_sdr`, `hackrf_transfer` and `airspy_rx` write (`.cu8`, `.cs8`, `.cs16`): interleaved I/Q ADC codes,
                        no header.  They stay codes up to the device (IQ_FORMATS, load_iq_codes; `codes_format=` below);
  * the audio FIFO    — `/tmp/sdrpipe` (io_manager.py:1-37): the same int16 frames, raw s16le `L R L R ...`.

Nothing here computes: the int16 conversion happens on the GPU (`pss_demod*`), these helpers move bytes.
"""
import os
import wave

import numpy as np

from . import _lib as L
from .engine import IQ_FORMATS, _IQ_DTYPES, _iq_args, _iq_codes, h_scan_dedupe, h_unpack_iq, iq_table  # noqa: F401  (IQ_FORMATS, iq_table: part of this module's interface)
from .signal_processing import DEFAULT_SAMPLE_RATE, _inject_designs, get_engine

_MODES = {'NFM': L.MODE_NFM, 'AM': L.MODE_AM, 'USB': L.MODE_USB, 'LSB': L.MODE_LSB, 'WFM': L.MODE_WFM}


def load_iq_recording(path):
    """play_recorded_signal (pyspecsdr.py:821-824): the saved read buffer as 1-D complex64."""
    s = np.load(path)
    if s.ndim != 1 or not np.iscomplexobj(s):
        raise ValueError("not an IQ recording: expected a 1-D complex array")
    return np.ascontiguousarray(s, np.complex64)


def load_iq_codes(path, fmt):
    """A raw capture file of ADC codes (fmt: a name of IQ_FORMATS; int16 little-endian) as a memory-mapped [n, 2] code array.  A file that
    ends inside a sample (an odd trailing byte or word) is not one of these: ValueError."""
    dt = np.dtype(_IQ_DTYPES[IQ_FORMATS[fmt][0]]).newbyteorder("<")
    size = os.path.getsize(path)
    if size % (2 * dt.itemsize):
        raise ValueError(f"{path}: {size} bytes is not a whole number of {fmt} samples ({2 * dt.itemsize} bytes each)")
    if size == 0:
        return np.empty((0, 2), dt)
    return np.memmap(path, dtype=dt, mode="r").reshape(-1, 2)


def unpack_iq(codes, fmt, table=None):
    """Codes [..., 2] -> the complex64 array [...] the driver would have delivered, on the host (pss_h_unpack_iq).  table: an 8-bit
    format's 256 float32 values when the driver's widening is not the format's own (iq_table)."""
    return h_unpack_iq(codes, fmt, table)


def cut_frames(samples, frame_len):
    """The recording as the read buffers the main loop would have seen (pyspecsdr.py:2236): [n_frames][frame_len];
    an incomplete tail buffer is dropped."""
    nf = len(samples) // frame_len
    return samples[:nf * frame_len].reshape(nf, frame_len)


def write_wav(path, pcm, sample_rate=DEFAULT_SAMPLE_RATE):
    """start_audio_recording + write_audio_samples + stop_audio_recording (audio_processing.py:25-43) for int16 frames
    that are already converted: pcm int16 [..., 2]."""
    pcm = np.ascontiguousarray(pcm, np.int16).reshape(-1, 2)
    with wave.open(path, 'wb') as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(pcm.tobytes())


def pipe_bytes(pcm):
    """What write_to_pipe (io_manager.py:23-27) hands to the FIFO for these frames."""
    return np.ascontiguousarray(pcm, np.int16).tobytes()


def header_strength_text(peak, avg):
    """draw_header's signal strength indicator (pyspecsdr.py:391) for a row's np.max and np.mean."""
    return f"Peak: {peak:.1f} dB Avg: {avg:.1f} dB"


def spectrum_scale_labels(display_min, display_max, disp_h):
    """draw_spectrogram's dB scale (pyspecsdr.py:430-435) for a row's range (spectrum_bars' d_range): the (line, text) pairs of every
    third display line, line 0 at the top (the reference draws line i at screen row i + 2, column 0)."""
    labels = []
    for i in range(int(disp_h)):
        db_value = display_max - (i * (display_max - display_min) / disp_h)
        if i % 3 == 0:
            labels.append((i, f"{db_value:4.0f}dB"))
    return labels


def bars_cells(height, level, disp_h, lib=None):
    """pss_h_bars_cells: spectrum bars (int8 [..., disp_w] height and level, -1 = column not drawn) expanded to draw_spectrogram's
    grids -> (glyph, colour) int8 [..., disp_h, disp_w]; glyph 0 '.', 1 '-', 2 '=', 3 '#', 4 ' ', colour = the curses pair (1 = cleared
    cell).  Pure host code: needs the library, not a GPU."""
    lib = lib or L.load()
    height, level = np.ascontiguousarray(height, np.int8), np.ascontiguousarray(level, np.int8)
    if height.shape != level.shape or height.ndim < 1:
        raise ValueError("height and level must have the same shape [..., disp_w]")
    disp_w = height.shape[-1]
    n_rows = height.size // disp_w if disp_w else 0
    shape = height.shape[:-1] + (int(disp_h), disp_w)
    glyph, colour = np.empty(shape, np.int8), np.empty(shape, np.int8)
    r = lib.pss_h_bars_cells(height.ctypes.data, level.ctypes.data, n_rows, int(disp_h), disp_w, glyph.ctypes.data, colour.ctypes.data)
    if r != 0:
        raise ValueError("pss_h_bars_cells: disp_h outside [1, 127], an empty line or a height above disp_h")
    return glyph, colour


def surface_cells(mag, max_h, max_w, lib=None):
    """pss_h_mags_cells: surface magnitudes (int8 [..., max_w - 8], -1 = column not drawn) expanded to draw_surface_plot's grid -> colour
    int8 [..., max_h, max_w]: 0 = empty, else the curses pair 1..5 of the '#' drawn there.  Pure host code: needs the library, not a GPU."""
    lib = lib or L.load()
    mag = np.ascontiguousarray(mag, np.int8)
    max_h, max_w = int(max_h), int(max_w)
    if mag.ndim < 1 or mag.shape[-1] != max_w - 8:
        raise ValueError("mag must have the shape [..., max_w - 8]")
    n_rows = mag.size // mag.shape[-1] if mag.shape[-1] > 0 else 0
    colour = np.empty(mag.shape[:-1] + (max(max_h, 0), max(max_w, 0)), np.int8)
    if lib.pss_h_mags_cells(mag.ctypes.data, n_rows, max_h, max_w, colour.ctypes.data) != 0:
        raise ValueError("pss_h_mags_cells: max_h < 4, max_w < 10 or a magnitude below -1")
    return colour


def vector_cells(mask, max_h, max_w, lib=None):
    """pss_h_masks_cells: constellation masks (uint32 [..., max_h, (max_w + 31) // 32], bit x & 31 of word x >> 5) expanded to
    draw_vector_display's grid -> int8 [..., max_h, max_w], 1 where a '.' lands.  Pure host code: needs the library, not a GPU."""
    lib = lib or L.load()
    mask = np.ascontiguousarray(mask)
    if mask.dtype != np.uint32:
        mask = mask.view(np.uint32) if mask.dtype == np.int32 else mask.astype(np.uint32)
    max_h, max_w = int(max_h), int(max_w)
    if max_h < 1 or max_w < 1 or mask.ndim < 2 or mask.shape[-2:] != (max_h, (max_w + 31) // 32):
        raise ValueError("mask must have the shape [..., max_h, (max_w + 31) // 32] with max_h, max_w >= 1")
    n_frames = mask.size // (max_h * mask.shape[-1])
    grid = np.empty(mask.shape[:-2] + (max_h, max_w), np.int8)
    if lib.pss_h_masks_cells(mask.ctypes.data, n_frames, max_h, max_w, grid.ctypes.data) != 0:
        raise ValueError("pss_h_masks_cells: bad argument")
    return grid


def surface_scale_labels(min_val, max_val, disp_h):
    """draw_surface_plot's amplitude scale (pyspecsdr.py:1609-1612) for a row's finite extremes (surface_mags' d_range): the (line, text)
    pairs of every third display line (disp_h = max_h - 4; the reference draws line i at screen row i + 2, column 0).  db_range carries
    the zero guard of :1578-1579: a constant row's labels step by 1 / disp_h."""
    db_range = max_val - min_val
    if db_range == 0:
        db_range = 1
    labels = []
    for i in range(int(disp_h)):
        db_value = max_val - (i * db_range / disp_h)
        if i % 3 == 0:
            labels.append((i, f"{db_value:4.0f}dB"))
    return labels


def sweep_frequencies(start, end, step):
    """The centre frequencies a sweep visits (pyspecsdr.py:1033 / :1081, :2523 / :2578): the values current_freq takes in
    `while current_freq <= end: ...; current_freq += step` — repeated float addition, not start + i * step — as float64."""
    if not step > 0:
        raise ValueError("step must be > 0")
    out, current_freq = [], start
    while current_freq <= end:
        out.append(current_freq)
        current_freq += step
    return np.array(out, np.float64)


_CLASS_NAMES = ("UNKNOWN", "FM_BROADCAST", "NARROW_FM", "AM_BROADCAST", "SSB", "DIGITAL")   # pss_class_name


def scan_signals(freqs, peak, bw, hit_idx, labels, dedupe=False):
    """The sweeps' list of records (pyspecsdr.py:2556-2561, :1063-1068) from a sweep report: freqs / peak (float32) / bw (float64) per
    slice, hit_idx the detections, labels their classes in the same order (PSS_CLASS_* numbers or names).  Every record is the
    reference's dict: 'frequency' a Python float, 'power' an np.float32, 'bandwidth' an np.float64, 'type' the class name.
    dedupe: scan_frequencies' duplicate removal on a 100 kHz grid (:1084-1091, h_scan_dedupe)."""
    freqs, peak, bw = np.asarray(freqs, np.float64), np.asarray(peak, np.float32), np.asarray(bw, np.float64)
    hit_idx = np.asarray(hit_idx, np.int64)
    if len(labels) != len(hit_idx):
        raise ValueError("labels: one per detection")
    signals = []
    for i, lab in zip(hit_idx, labels):
        name = lab if isinstance(lab, str) else (_CLASS_NAMES[int(lab)] if 0 <= int(lab) < len(_CLASS_NAMES) else "UNKNOWN")
        signals.append({'frequency': float(freqs[i]), 'power': peak[i], 'bandwidth': bw[i], 'type': str(name)})
    if dedupe:
        signals = [signals[k] for k in h_scan_dedupe([s['frequency'] for s in signals], 100e3)]
    return signals


def scan_result_lines(signals, max_h, max_w, page=0):
    """What display_scan_results (pyspecsdr.py:1203-1262) draws for one page of a record list on a max_h x max_w screen, as
    (y, x, text, colour_pair, bold) tuples in drawing order: header, dash line, max_h - 7 entries per page (cut at max_w - 1, coloured by
    type), the two footer lines.  An empty list: the "No signals found" line and the key prompt (:1212-1213)."""
    if not signals:
        return [(0, 0, "\nNo signals found above threshold.\n", 3, False), (2, 0, "\nPress any key to continue...", 2, False)]
    max_h, max_w = int(max_h), int(max_w)
    results_per_page = max_h - 7
    if results_per_page < 1:
        raise ValueError("max_h must be at least 8")
    total_pages = (len(signals) + results_per_page - 1) // results_per_page
    if not 0 <= page < total_pages:
        raise ValueError(f"page outside [0, {total_pages})")
    header = f"Detected Signals ({len(signals)} found) - Page {page + 1}/{total_pages}"
    lines = [(0, 0, header, 1, True), (1, 0, "-" * len(header), 2, False)]
    start_idx = page * results_per_page
    end_idx = min(start_idx + results_per_page, len(signals))
    for line_no, (i, signal) in enumerate(enumerate(signals[start_idx:end_idx], start_idx + 1), 2):
        power_str = f"{signal['power']:.1f}".rjust(6)
        freq_str = f"{signal['frequency'] / 1e6:.3f}".rjust(8)
        bw_str = f"{signal['bandwidth'] / 1e3:.1f}".rjust(6)
        type_str = signal['type'].ljust(15)
        line = f"{str(i).rjust(3)}. {freq_str} MHz  Power: {power_str} dB  BW: {bw_str} kHz  Type: {type_str}"
        pair = {'FM_BROADCAST': 4, 'DIGITAL': 5, 'UNKNOWN': 2}.get(signal['type'], 1)
        lines.append((line_no, 0, line[:max_w - 1], pair, False))
    lines.append((max_h - 1, 0, "Navigation: [n]ext page, [p]revious page, [number] to select, [q]uit", 2, False))
    lines.append((max_h - 2, 0, "Enter choice: ", 1, True))
    return lines


def _squelch_args(squelch, meter_every, peak_power, frame_len, mode):
    """demodulate_recording's argument checks for the squelch path (host only: made before anything touches the GPU)."""
    if mode not in _MODES:
        raise ValueError(f"unknown demodulation mode {mode!r}")
    squelch, peak_power = float(squelch), float(peak_power)
    if int(meter_every) != meter_every or meter_every < 0:
        raise ValueError("meter_every must be an integer >= 0 (0: the header is never drawn)")
    if frame_len < 16 or frame_len > 65536 or frame_len & (frame_len - 1):
        raise ValueError("squelch needs the cell-exact rows: frame_len must be a power of two in [16, 65536]")
    return squelch, int(meter_every), peak_power


def demodulate_recording(samples, sample_rate, mode='NFM', frame_len=32768, chunk_frames=4096, squelch=None, meter_every=3, peak_power=0.0,
                         codes_format=None, table=None):
    """Every read buffer of a recording through demodulate_signal on the GPU -> int16 [n_frames][n_out][2], i.e. the
    audio the reference would have written had it played the recording buffer by buffer.

    squelch (a level in dB; None: no gate, the result above): the reference's loop buffers audio only while PEAK_POWER >= SQUELCH
    (pyspecsdr.py:2261-2263), PEAK_POWER being the maximum of the post-processed row its header last showed — every meter_every-th
    buffer (:2288-2291), starting from peak_power (:172).  Returns (pcm int16 [n_open][n_out][2] of the open buffers in order,
    open uint8 [n_frames], peak float64 [n_frames], avg float64 [n_frames]): the gate and every buffer's Peak / Avg as
    header_strength_text prints them; rows from the cell-exact pipeline (float64 compute_fft, smoothing, median clamp).

    codes_format (a name of IQ_FORMATS; None: complex64 samples): `samples` is the recording's ADC code array [n, 2] (load_iq_codes); the
    codes are uploaded and widened on the device (table: as unpack_iq), the results are those of the unpacked recording."""
    if squelch is not None:
        squelch, meter_every, peak_power = _squelch_args(squelch, meter_every, peak_power, frame_len, mode)
    if codes_format is not None:
        iq = _iq_args(codes_format, table)
        samples = _iq_codes(samples, iq[0])
        if samples.ndim != 2:
            raise ValueError("codes: [n, 2]")
        nfr = len(samples) // frame_len
        frames = samples[:nfr * frame_len].reshape(nfr, frame_len, 2)
    else:
        frames = cut_frames(np.ascontiguousarray(samples, np.complex64), frame_len)
    fs = float(DEFAULT_SAMPLE_RATE) if mode == 'AM' else float(sample_rate)
    if mode != 'AM':
        _inject_designs({'NFM': 'nfm', 'WFM': 'wfm'}.get(mode, 'ssb'), fs)
    if squelch is None:
        if codes_format is not None:
            return get_engine().h_demodulate_batch_codes(_MODES[mode], frames, fs, codes_format, iq[2], chunk_frames)
        return get_engine().h_demodulate_batch(_MODES[mode], frames, fs, chunk_frames)
    import torch
    e = get_engine()
    nf, n = frames.shape[:2]
    n_out = e.demod_out_len(_MODES[mode], n, fs)
    if n_out < 0:
        raise ValueError("sample rate below the target rate or unknown mode")
    pcm, opened, peak, avg = [], np.empty(nf, np.uint8), np.empty(nf, np.float64), np.empty(nf, np.float64)
    held, phase, disp_w = peak_power, 0, 112
    for c0 in range(0, nf, int(chunk_frames)):
        c = min(int(chunk_frames), nf - c0)
        dev = lambda shape, dt: torch.empty(shape, dtype=dt, device=f"cuda:{e.device}")
        if codes_format is not None:
            d_codes = torch.from_numpy(np.array(frames[c0:c0 + c])).to(f"cuda:{e.device}")
            d_iq = dev((c, 2 * n), torch.float32)
            e.unpack_iq(d_codes, c * n, d_iq, codes_format, iq[2])
        else:
            d_iq = torch.from_numpy(np.ascontiguousarray(frames[c0:c0 + c]).view(np.float32)).to(f"cuda:{e.device}")
        d_db32, d_lo, d_hi = dev((c, n), torch.float32), dev(c, torch.float64), dev(c, torch.float64)
        d_a, d_b, d_pcm = dev((c, disp_w), torch.int8), dev((c, disp_w), torch.int8), dev((c, n_out, 2), torch.int16)
        d_peak, d_avg, d_open = dev(c, torch.float64), dev(c, torch.float64), dev(c, torch.uint8)
        n_open, held = e.frame_pipeline_squelch(_MODES[mode], d_iq, c, n, fs, d_db32, None, d_lo, d_hi, disp_w, d_a, d_b, d_pcm, squelch, d_peak,
                                                d_avg, d_open, every=meter_every, phase=phase, held_in=held)
        phase = (phase + c) % meter_every if meter_every else 0
        pcm.append(d_pcm[:n_open].cpu().numpy())
        opened[c0:c0 + c], peak[c0:c0 + c], avg[c0:c0 + c] = d_open.cpu().numpy(), d_peak.cpu().numpy(), d_avg.cpu().numpy()
    pcm = np.concatenate(pcm) if pcm else np.empty((0, n_out, 2), np.int16)
    return pcm, opened, peak, avg


# display width = screen width - offset, display height = screen height - 4: the layouts of draw_waterfall / draw_persistence (pyspecsdr.py
# :1342, :1512), draw_gradient_waterfall (:1640), draw_spectrogram (:399); the surface plot resamples to max_width - 8 (:1571) and draws on
# the whole screen, as the constellation does (:1719)
_VIEW_OFFSETS = {'waterfall': 8, 'persistence': 8, 'gradient': 10, 'spectrum': 7, 'surface': 8}


def view_geometry(view, screen):
    """(disp_h, disp_w) as Engine.stream_frames takes them for `view` on a screen of (max_height, max_width) cells."""
    max_h, max_w = int(screen[0]), int(screen[1])
    if view == 'vector':
        return max_h, max_w
    if view not in _VIEW_OFFSETS:
        raise ValueError(f"unknown view {view!r}")
    return max_h - 4, max_w - _VIEW_OFFSETS[view]


def replay_recording(samples, sample_rate, mode='WFM', view='spectrum', frame_len=32768, chunk_frames=256, squelch=-60, codes_format=None,
                     table=None, screen=(40, 120), meter_every=3, peak_power=0.0, cells=False):
    """A recording played as the reference's main loop would play it, with the reference's defaults (WFM, the SPECTRUM view, SQUELCH -60,
    pyspecsdr.py:2855, :167, :171): cut into read buffers (cut_frames), all-zero buffers skipped (:2237), every live buffer's view drawn and
    its audio gated by the squelch (None: no gate) -> Engine.stream_frames' dict, everything per buffer compacted to the live ones.
    samples: the 1-D complex64 recording, or with codes_format (a name of IQ_FORMATS) its ADC code array [n, 2] (load_iq_codes; table as
    unpack_iq).  screen: (max_height, max_width) of the terminal; the view's display size follows as the draw functions derive it
    (view_geometry).  cells=True adds "cells": the expanded grids of the views that return a compact form (bars_cells -> (glyph, colour),
    surface_cells, vector_cells)."""
    if mode not in _MODES:
        raise ValueError(f"unknown demodulation mode {mode!r}")
    disp_h, disp_w = view_geometry(view, screen)
    if codes_format is not None:
        iq = _iq_args(codes_format, table)
        samples = _iq_codes(samples, iq[0])
        if samples.ndim != 2:
            raise ValueError("codes: [n, 2]")
        nfr = len(samples) // frame_len
        frames = np.ascontiguousarray(samples[:nfr * frame_len]).reshape(nfr, frame_len, 2)
    else:
        frames = np.ascontiguousarray(cut_frames(np.ascontiguousarray(samples, np.complex64), frame_len))
    fs = float(DEFAULT_SAMPLE_RATE) if mode == 'AM' else float(sample_rate)
    if mode != 'AM':
        _inject_designs({'NFM': 'nfm', 'WFM': 'wfm'}.get(mode, 'ssb'), fs)
    out = get_engine().stream_frames(frames, fs, chunk_frames, mode=_MODES[mode], view=view, fmt=codes_format, table=table, skip_dead=True,
                                     squelch=squelch, meter_every=meter_every, peak_power=peak_power, disp_h=disp_h, disp_w=disp_w)
    if cells:
        if view == 'spectrum':
            out["cells"] = bars_cells(out["height"], out["level"], disp_h)
        elif view == 'surface':
            out["cells"] = surface_cells(out["mag"], screen[0], screen[1])
        elif view == 'vector':
            out["cells"] = vector_cells(out["mask"], screen[0], screen[1])
    return out


def _decode_args(sample_rate, decoder, frame_len, chunk_frames):
    """decode_recording's argument checks (host only: made before anything touches the GPU) -> (sample_rate, frame_len, chunk_frames)."""
    if decoder not in ('morse', 'aprs'):
        raise ValueError(f"unknown decoder {decoder!r}: 'morse' or 'aprs'")
    sample_rate = float(sample_rate)
    if not sample_rate > 0 or (decoder == 'aprs' and sample_rate < 1200):
        raise ValueError("sample_rate must be positive (aprs: at least 1200 Hz, one sample per bit)")
    if frame_len is None:
        frame_len = int(sample_rate * 0.5)      # the read size of both decoder screens (pyspecsdr.py:503-659)
    if int(frame_len) != frame_len or frame_len < 1:
        raise ValueError("frame_len must be an integer >= 1")
    if int(chunk_frames) != chunk_frames or chunk_frames < 1:
        raise ValueError("chunk_frames must be an integer >= 1")
    return sample_rate, int(frame_len), int(chunk_frames)


def decode_recording(samples, sample_rate, decoder, frame_len=None, threshold=-20, chunk_frames=256, codes_format=None, table=None):
    """Every read buffer of a recording through decode_morse (decoder='morse') or decode_aprs ('aprs') on the GPU -> a list with one entry
    per buffer: (text, timing dict) or a packet list, as decoders.decode_morse_batch / decode_aprs_batch return them.  frame_len defaults
    to int(sample_rate * 0.5), the read size of both decoder screens; an incomplete tail buffer is dropped (cut_frames).  chunk_frames
    buffers go through one library call.  codes_format / table: as demodulate_recording — `samples` is the ADC code array [n, 2]."""
    from . import decoders as D
    sample_rate, frame_len, chunk_frames = _decode_args(sample_rate, decoder, frame_len, chunk_frames)
    if codes_format is not None:
        iq = _iq_args(codes_format, table)
        samples = _iq_codes(samples, iq[0])
        if samples.ndim != 2:
            raise ValueError("codes: [n, 2]")
        nfr = len(samples) // frame_len
        frames = samples[:nfr * frame_len].reshape(nfr, frame_len, 2)
    else:
        samples = np.asarray(samples)
        if samples.ndim != 1:
            raise ValueError("samples: a 1-D recording")
        frames = cut_frames(np.ascontiguousarray(samples, np.complex64), frame_len)
    import torch
    e = get_engine()
    nf, n = frames.shape[:2]
    tables = D._bandpass_tables(sample_rate) if decoder == 'aprs' else None
    out = []
    for c0 in range(0, nf, chunk_frames):
        c = min(chunk_frames, nf - c0)
        if codes_format is not None:
            d_codes = torch.from_numpy(np.array(frames[c0:c0 + c])).to(f"cuda:{e.device}")
            d_iq = torch.empty((c, 2 * n), dtype=torch.float32, device=f"cuda:{e.device}")
            e.unpack_iq(d_codes, c * n, d_iq, codes_format, iq[2])
        else:
            d_iq = torch.from_numpy(np.ascontiguousarray(frames[c0:c0 + c]).view(np.float32)).to(f"cuda:{e.device}")
        if decoder == 'morse':
            out += D._morse_batch_dev(e, d_iq, c, n, sample_rate, threshold)
        else:
            out += D._aprs_batch_dev(e, d_iq, c, n, sample_rate, tables)
    return out


def decode_mono_recording(samples, fs, frame_len=32768, codes_format=None, table=None, chunk_frames=4096):
    """Every read buffer of a recording through decode_mono (signal_processing.py:331-359) on the GPU -> int16 [n_frames][n_out], mono
    broadcast-FM audio at fs / 6, n_out = ceil((frame_len - 1) / 6).  An incomplete tail buffer is dropped (cut_frames).  codes_format /
    table: as demodulate_recording — `samples` is the ADC code array [n, 2], widened on the device."""
    if int(frame_len) != frame_len or frame_len < 1 or int(chunk_frames) != chunk_frames or chunk_frames < 1:
        raise ValueError("frame_len and chunk_frames must be integers >= 1")
    frame_len, chunk_frames = int(frame_len), int(chunk_frames)
    e = get_engine()
    if codes_format is None:
        samples = np.asarray(samples)
        if samples.ndim != 1:
            raise ValueError("samples: a 1-D recording")
        return e.h_decode_mono_batch(cut_frames(np.ascontiguousarray(samples, np.complex64), frame_len), fs, chunk_frames)
    iq = _iq_args(codes_format, table)
    samples = _iq_codes(samples, iq[0])
    if samples.ndim != 2:
        raise ValueError("codes: [n, 2]")
    import torch
    nf = len(samples) // frame_len
    frames = samples[:nf * frame_len].reshape(nf, frame_len, 2)
    n_out = e.decode_mono_len(frame_len)
    pcm = np.empty((nf, n_out), np.int16)
    if n_out == 0:
        return pcm
    for c0 in range(0, nf, chunk_frames):
        c = min(chunk_frames, nf - c0)
        d_codes = torch.from_numpy(np.array(frames[c0:c0 + c])).to(f"cuda:{e.device}")
        d_iq = torch.empty((c, 2 * frame_len), dtype=torch.float32, device=f"cuda:{e.device}")
        d_pcm = torch.empty((c, n_out), dtype=torch.int16, device=f"cuda:{e.device}")
        e.unpack_iq(d_codes, c * frame_len, d_iq, codes_format, iq[2])
        e.decode_mono(d_iq, c, frame_len, fs, d_pcm)
        pcm[c0:c0 + c] = d_pcm.cpu().numpy()
    return pcm


def _chunk_device(e, samples, decim, lead, chunk_samples, codes_format, table, m_end, plan, reach_back=0):
    """The streaming _tune_device and _bank_device share -> device tensor float32 [rows][2 * m_end]: the capture goes up in chunks of about
    chunk_samples samples, each with the halo its outputs' taps reach back and ahead for, and every chunk's outputs land in their place
    of the one result.  plan() -> (taps, rows, run) is asked once the capture is in its form; run(d_iq, n_buf, out_ptr, **window) is the
    entry point's call with buf_index0, n_capture, lead, m_begin, m_end and out_stride.  reach_back: samples in front of the taps' halo that
    the entry point reads as well (pss_rds_front's discriminator: 1)."""
    import torch
    if int(chunk_samples) != chunk_samples or chunk_samples < 1:
        raise ValueError("chunk_samples must be an integer >= 1")
    if codes_format is not None:
        iq = _iq_args(codes_format, table)
        samples = _iq_codes(samples, iq[0])
        if samples.ndim != 2:
            raise ValueError("codes: [n, 2]")
    else:
        samples = np.ascontiguousarray(samples, np.complex64)
        if samples.ndim != 1:
            raise ValueError("samples: a 1-D recording")
    taps, rows, run = plan()
    n_taps = len(taps)
    lead = (n_taps - 1) // 2 if lead is None else int(lead)
    n = len(samples)
    n_out = e.lib.pss_ddc_out_len(n, decim)
    if n_out < 0:
        raise ValueError("decim outside [1, 4096]")
    if m_end is None:
        m_end = n_out
    dev = f"cuda:{e.device}"
    d_out = torch.empty((rows, 2 * m_end), dtype=torch.float32, device=dev)
    per_chunk = max(1, int(chunk_samples) // decim)
    for m0 in range(0, max(m_end, 1), per_chunk):
        m1 = min(m_end, m0 + per_chunk)
        lo, hi = max(0, m0 * decim + lead - (n_taps - 1) - reach_back), min(n, (m1 - 1) * decim + lead + 1)
        hi = max(hi, lo)
        if codes_format is not None:
            d_codes = torch.from_numpy(np.array(samples[lo:hi])).to(dev)
            d_iq = torch.empty(2 * (hi - lo) + 2, dtype=torch.float32, device=dev)
            if hi > lo:
                e.unpack_iq(d_codes, hi - lo, d_iq, codes_format, iq[2])
        else:
            d_iq = torch.from_numpy(samples[lo:hi].view(np.float32)).to(dev) if hi > lo else torch.empty(2, dtype=torch.float32, device=dev)
        # m1 == m0 (an empty capture) still goes through the call: it checks the arguments and writes nothing
        run(d_iq, hi - lo, d_out.data_ptr() + 8 * m0, buf_index0=lo, n_capture=n, lead=lead, m_begin=m0, m_end=m1, out_stride=m_end)
    return d_out


def _tune_device(samples, fs, offsets_hz, decim, taps, lead, chunk_samples, codes_format, table, m_end=None):
    """tune_recording's work -> (device tensor float32 [K][2 * m_end], effective offsets), streamed by _chunk_device.  The phase of a
    sample follows from its index in the capture, so no chunking changes a bit."""
    e = get_engine()
    fs, decim = float(fs), int(decim)
    effective = None

    def plan():
        nonlocal effective
        pairs = [e.ddc_word(f, fs) for f in np.atleast_1d(np.asarray(offsets_hz, np.float64))]
        words = np.array([p[0] for p in pairs], np.uint64)
        effective = np.array([p[1] for p in pairs], np.float64)
        t = e.ddc_default_taps(decim) if taps is None else np.ascontiguousarray(taps, np.float64)
        return t, len(words), lambda d_iq, n_buf, out, **window: e.ddc(d_iq, n_buf, words, decim, out, taps=t, **window)

    d_out = _chunk_device(e, samples, decim, lead, chunk_samples, codes_format, table, m_end, plan)
    return d_out, effective


def tune_recording(samples, fs, offsets_hz, decim, taps=None, lead=None, chunk_samples=1 << 22, codes_format=None, table=None):
    """What the reference asks its radio for — another centre frequency (sdr.set_center_freq: the arrow keys, bookmarks, band presets,
    both sweeps) and another sample rate (sdr.sample_rate = 48000 before the Morse decoder reads, pyspecsdr.py:552; the bandwidth keys) —
    done to a capture: the K channels at fs + offsets_hz, low-pass filtered and decimated by `decim` on the GPU (pss_ddc) ->
    (channels complex64 [K][ceil(n / decim)], fs / decim, effective_offsets float64 [K]).  A signal at +offset lands at 0 Hz; the
    offsets that result differ from the asked ones by less than fs / 2^64.  taps: a float64 low-pass table (default:
    scipy.signal.decimate's own FIR, firwin(20 decim + 1, 1 / decim); needs decim <= 204); lead: the tap that sits on an output's own
    sample (default the middle one: zero phase, scipy.signal.decimate(..., ftype='fir')).  The capture is streamed in chunks of
    chunk_samples samples plus the halos the taps need; the result does not depend on chunk_samples.  codes_format / table: as
    demodulate_recording — `samples` is the ADC code array [n, 2], widened per chunk on the device."""
    d_out, effective = _tune_device(samples, fs, offsets_hz, decim, taps, lead, chunk_samples, codes_format, table)
    return d_out.cpu().numpy().view(np.complex64), float(fs) / int(decim), effective


def survey_freqs(fs, nperseg):
    """The frequencies of a survey row in ascending order: fftshift(fftfreq(nperseg, 1 / fs))."""
    return np.fft.fftshift(np.fft.fftfreq(int(nperseg), 1.0 / float(fs)))


def survey_recording(samples, fs, nperseg=4096, overlap=0.5, window=None, detrend=True, scaling='density', chunk_samples=1 << 22, codes_format=None,
                     table=None):
    """What is in this capture, and where — the question the reference answers by retuning its radio and looking (scan_frequencies, the band
    sweep), answered for a capture in one pass on the GPU (pss_welch): Welch's averaged periodogram (scipy.signal.welch in float64, the
    reference's own PSD estimator, signal_processing.py:299) and the max-hold trace of the same periodograms.
    -> dict(freqs_hz, mean, max, mean_db, max_db, n_segments, nperseg, step): float64 rows of nperseg bins in ascending frequency; dB is
    the reference's 10 log10(p + 1e-10) (signal_processing.py:270).  The step is nperseg - int(nperseg * overlap), SciPy's noverlap rule.
    The capture goes up in chunks of chunk_samples samples into one resident device row (codes_format / table: `samples` is the ADC code
    array [n, 2], widened per chunk on the device); the result does not depend on chunk_samples."""
    import torch
    e = get_engine()
    fs, nperseg = float(fs), int(nperseg)
    if int(chunk_samples) != chunk_samples or chunk_samples < 1:
        raise ValueError("chunk_samples must be an integer >= 1")
    if not 0.0 <= overlap < 1.0:
        raise ValueError("overlap in [0, 1)")
    if codes_format is not None:
        iq = _iq_args(codes_format, table)
        samples = _iq_codes(samples, iq[0])
        if samples.ndim != 2:
            raise ValueError("codes: [n, 2]")
    else:
        samples = np.ascontiguousarray(samples, np.complex64)
        if samples.ndim != 1:
            raise ValueError("samples: a 1-D recording")
    n = len(samples)
    step = nperseg - int(nperseg * overlap)
    n_segments = e.welch_segments(n, nperseg, step)
    if n_segments < 1:
        raise ValueError("the capture is shorter than nperseg")
    dev = f"cuda:{e.device}"
    d_iq = torch.empty(2 * n, dtype=torch.float32, device=dev)
    for lo in range(0, n, int(chunk_samples)):
        hi = min(n, lo + int(chunk_samples))
        if codes_format is not None:
            d_codes = torch.from_numpy(np.array(samples[lo:hi])).to(dev)
            e.unpack_iq(d_codes, hi - lo, d_iq.data_ptr() + 8 * lo, codes_format, iq[2])
        else:
            d_iq[2 * lo:2 * hi].copy_(torch.from_numpy(samples[lo:hi].view(np.float32)))
    d_rows = torch.empty((2, nperseg), dtype=torch.float64, device=dev)
    e.welch(d_iq, 1, n, nperseg, step, d_rows[0], d_rows[1], window=window, detrend=detrend, scaling=scaling, fs=fs)
    rows = np.fft.fftshift(d_rows.cpu().numpy(), axes=1)
    with np.errstate(invalid="ignore"):
        db = 10 * np.log10(rows + 1e-10)
    return dict(freqs_hz=survey_freqs(fs, nperseg), mean=rows[0], max=rows[1], mean_db=db[0], max_db=db[1], n_segments=n_segments, nperseg=nperseg,
                step=step)


def survey_signals(db, fs, margin_db=10.0, floor_db=None, min_bins=2):
    """The signals of a survey row: `db` is a dB row in ascending frequency (survey_recording's mean_db or max_db).  A bin is occupied where
    db > floor + margin_db (a NaN compares false); floor: floor_db, or the median of the row's finite values.  Every maximal run [a, b] of
    consecutive occupied bins (no wrap-around) of at least min_bins bins gives
    dict(lo_hz, hi_hz, center_hz, bandwidth_hz, peak_hz, peak_db, bins=(a, b)) with bandwidth_hz = (b - a + 1) fs / N, the reference's
    count * fs / N (pyspecsdr.py:2549-2552), lo_hz and hi_hz the edges of bins a and b, center_hz their middle.  Sorted by frequency.  Host
    code in NumPy: the row is N numbers."""
    db = np.asarray(db, np.float64)
    if db.ndim != 1 or len(db) < 1:
        raise ValueError("db: a 1-D row")
    n, fs = len(db), float(fs)
    if floor_db is None:
        finite = db[np.isfinite(db)]
        if len(finite) == 0:
            return []
        floor_db = float(np.median(finite))
    with np.errstate(invalid="ignore"):
        mask = db > float(floor_db) + float(margin_db)
    edges = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    starts, ends = np.nonzero(edges == 1)[0], np.nonzero(edges == -1)[0] - 1
    freqs = np.fft.fftshift(np.fft.fftfreq(n, 1.0 / fs))
    bin_hz = fs / n
    out = []
    for a, b in zip(starts, ends):
        a, b = int(a), int(b)
        if b - a + 1 < min_bins:
            continue
        lo, hi = float(freqs[a]) - bin_hz / 2, float(freqs[b]) + bin_hz / 2
        k = a + int(np.argmax(db[a:b + 1]))
        out.append(dict(lo_hz=lo, hi_hz=hi, center_hz=(lo + hi) / 2, bandwidth_hz=(b - a + 1) * bin_hz, peak_hz=float(freqs[k]), peak_db=float(db[k]),
                        bins=(a, b)))
    return out


_AUDIO_MID = {'AM': 22050, 'USB': 22050, 'LSB': 22050, 'RAW': 22050, 'NFM': 44100, 'WFM': 110250}


def plan_resample(rate_in, rate_out):
    """The factors that take rate_in to rate_out -> (up, down), reduced by their gcd: 50 000 -> 44 100 is (441, 500).  Both rates must be
    integers (to 1e-9 relative) and neither reduced factor may pass 4096 (pss_resample's limit)."""
    out = []
    for name, rate in (("rate_in", rate_in), ("rate_out", rate_out)):
        rate = float(rate)
        if not (np.isfinite(rate) and rate >= 0.5):
            raise ValueError(f"{name} = {rate!r} must be a positive rate")
        r = int(round(rate))
        if abs(rate - r) > 1e-9 * rate:
            raise ValueError(f"{name} = {rate!r} is not an integer: no ratio of integers takes one rate to the other")
        out.append(r)
    g = int(np.gcd(out[0], out[1]))
    up, down = out[1] // g, out[0] // g
    for name, f in (("up", up), ("down", down)):
        if f > 4096:
            raise ValueError(f"{name} = {f} (rate_out / rate_in = {up} / {down} reduced) is above 4096")
    return up, down


def plan_audio(rate_in, mode):
    """The resampling in front of the demodulator whose PCM then comes out at exactly DEFAULT_SAMPLE_RATE -> (up, down, rate_mid): AM / USB /
    LSB / RAW do not decimate, rate_mid = 22 050; NFM's 15 kHz FIR needs a channel rate above 30 kS/s and decimates by
    int(rate / 22 050): rate_mid = 44 100; WFM (pilot, L - R band up to 53 kHz): 110 250."""
    if mode not in _AUDIO_MID:
        raise ValueError(f"unknown demodulation mode {mode!r}")
    rate_mid = _AUDIO_MID[mode]
    up, down = plan_resample(rate_in, rate_mid)
    return up, down, float(rate_mid)


def resample_halo(n_in, up, down, n_taps, j_begin, j_end):
    """The samples [lo, hi) of a row of n_in samples that outputs [j_begin, j_end) of pss_resample read (csrc/pss_resample.h restated in
    integers; empty: lo == hi)."""
    g = int(np.gcd(int(up), int(down)))
    up, down, n_in = int(up) // g, int(down) // g, int(n_in)
    n_out = -(-n_in * up // down)
    if not 0 <= j_begin <= j_end <= n_out:
        raise ValueError("[j_begin, j_end) outside [0, n_out]")
    if j_begin == j_end:
        return 0, 0
    if up == 1 and down == 1:
        return j_begin, j_end
    half_len = (n_taps - 1) // 2
    pre = down - half_len % down
    pre_remove = (half_len + pre) // down
    post = max(0, (n_out + pre_remove - 1) * down - ((n_in - 1) * up + n_taps + pre - 1))
    hpp = -(-(pre + n_taps + post) // up)
    lo = max(0, (j_begin + pre_remove) * down // up - hpp + 1)
    hi = min(n_in - 1, (j_end - 1 + pre_remove) * down // up) + 1
    return (lo, hi) if lo < hi else (0, 0)


def resample_recording(rows, up, down, taps=None, chunk_samples=1 << 22):
    """scipy.signal.resample_poly(rows, up, down, axis=-1) for host rows [n_rows][n] or [n] (float32, float64 or complex64) on the GPU
    (pss_resample) -> the same type, [n_rows][ceil(n up / down)].  The rows go up in chunks of about chunk_samples input samples, each
    with exactly the halo its outputs read (resample_halo); an output's arithmetic follows from its index in the row, so the result does
    not depend on chunk_samples.  taps: a float64 low-pass table (default: resample_poly's own Kaiser design)."""
    import torch
    e = get_engine()
    x = np.asarray(rows)
    if x.ndim not in (1, 2) or x.dtype not in e.RS_DTYPES:
        raise ValueError("rows: a 1-D or 2-D float32, float64 or complex64 array")
    if int(chunk_samples) != chunk_samples or chunk_samples < 1:
        raise ValueError("chunk_samples must be an integer >= 1")
    r2 = np.ascontiguousarray(x.reshape(-1, x.shape[-1]))
    n_rows, n = r2.shape
    taps = e.resample_default_taps(up, down) if taps is None else np.ascontiguousarray(taps, np.float64)
    n_out = e.resample_out_len(n, up, down)
    cplx = x.dtype == np.complex64
    real = np.float32 if cplx else x.dtype
    width = 2 if cplx else 1
    dev = f"cuda:{e.device}"
    d_y = torch.empty((n_rows, n_out * width), dtype=torch.from_numpy(np.empty(0, real)).dtype, device=dev)
    g = int(np.gcd(int(up), int(down)))
    per_chunk = max(1, int(chunk_samples) * (int(up) // g) // (int(down) // g))
    for j0 in range(0, n_out if n_rows else 0, per_chunk):
        j1 = min(n_out, j0 + per_chunk)
        lo, hi = resample_halo(n, up, down, len(taps), j0, j1)
        d_x = torch.from_numpy(np.ascontiguousarray(r2[:, lo:hi]).view(real)).to(dev) if hi > lo else None
        e.resample(d_x, x.dtype, n_rows, hi - lo, up, down, d_y.data_ptr() + j0 * width * np.dtype(real).itemsize, taps=taps, buf_index0=lo,
                   n_in=n, j_begin=j0, j_end=j1, y_stride=n_out)
    out = d_y.cpu().numpy()
    out = out.view(np.complex64) if cplx else out
    return out if x.ndim == 2 else out[0]


def _exact_rate_rows(d_iq, rate_in, mode, frame_len):
    """exact_rate=True: the complex64 rows d_iq (float32 [K][2 m]) at rate_in resampled on the device to plan_audio's rate_mid and stopped at
    a multiple of frame_len -> (float32 [K][2 n_frames frame_len], n_frames, rate_mid)."""
    import torch
    e = get_engine()
    up, down, rate_mid = plan_audio(rate_in, mode)
    k, m = d_iq.shape[0], d_iq.shape[1] // 2
    n_frames = e.resample_out_len(m, up, down) // frame_len
    d_rs = torch.empty((k, 2 * n_frames * frame_len), dtype=torch.float32, device=d_iq.device)
    if k * n_frames:
        e.resample(d_iq.contiguous(), np.complex64, k, m, up, down, d_rs, j_end=n_frames * frame_len)
    return d_rs, n_frames, rate_mid


def demodulate_channels(samples, fs, offsets_hz, decim, mode='NFM', frame_len=32768, **tune_kw):
    """Listen to K channels of one wideband capture: tune_recording's channels, cut into read buffers of frame_len samples at fs / decim
    and demodulated as demodulate_signal would -> int16 [K][n_frames][n_out][2].  The down-converter stops at a multiple of frame_len
    (an incomplete tail buffer is dropped, as cut_frames does), so its result IS the batch of K * n_frames read buffers on the device:
    nothing comes back to the host between the two steps.  tune_kw: taps, lead, chunk_samples, codes_format, table, exact_rate
    (True: the channels are resampled on the device to plan_audio(fs / decim, mode)'s rate before they are cut into read buffers, so the
    PCM is at exactly DEFAULT_SAMPLE_RATE; the frame count follows the resampled length)."""
    import torch
    if mode not in _MODES:
        raise ValueError(f"unknown demodulation mode {mode!r}")
    if int(frame_len) != frame_len or frame_len < 1:
        raise ValueError("frame_len must be an integer >= 1")
    frame_len, decim = int(frame_len), int(decim)
    e = get_engine()
    n_total = e.lib.pss_ddc_out_len(len(samples), decim)
    if n_total < 0:
        raise ValueError("decim outside [1, 4096]")
    kw = dict(taps=None, lead=None, chunk_samples=1 << 22, codes_format=None, table=None, exact_rate=False)
    for k in tune_kw:
        if k not in kw:
            raise TypeError(f"unexpected argument {k!r}")
    kw.update(tune_kw)
    n_frames = n_total // frame_len
    rate = float(fs) / decim
    if kw['exact_rate']:
        rate = plan_audio(rate, mode)[2]
    if mode == 'AM':
        rate = float(DEFAULT_SAMPLE_RATE)
    else:
        _inject_designs({'NFM': 'nfm', 'WFM': 'wfm'}.get(mode, 'ssb'), rate)
    n_out = e.demod_out_len(_MODES[mode], frame_len, rate)
    if n_out < 0:
        raise ValueError("the channel rate fs / decim is below the target rate")
    d_iq, _ = _tune_device(samples, fs, offsets_hz, decim, kw['taps'], kw['lead'], kw['chunk_samples'], kw['codes_format'], kw['table'],
                           m_end=None if kw['exact_rate'] else n_frames * frame_len)
    if kw['exact_rate']:
        d_iq, n_frames, _ = _exact_rate_rows(d_iq, float(fs) / decim, mode, frame_len)
    k = d_iq.shape[0]
    d_pcm = torch.empty((k * n_frames, n_out, 2), dtype=torch.int16, device=d_iq.device)
    if k * n_frames:
        e.demod_signal(_MODES[mode], d_iq, k * n_frames, frame_len, rate, d_pcm)
    return d_pcm.cpu().numpy().reshape(k, n_frames, n_out, 2)


def bank_offsets(fs, n_chan):
    """The offset in Hz of each row of the channeliser's output -> float64 [n_chan]: c fs / n_chan for c < n_chan / 2 and
    (c - n_chan) fs / n_chan otherwise (row n_chan / 2, the band edge, reads -fs / 2)."""
    n_chan = int(n_chan)
    if n_chan < 2 or n_chan > 1024 or n_chan & (n_chan - 1):
        raise ValueError("n_chan must be a power of two in [2, 1024]")
    c = np.arange(n_chan, dtype=np.float64)
    return np.where(c < n_chan // 2, c, c - n_chan) * (float(fs) / n_chan)


def _bank_device(samples, n_chan, decim, taps, lead, chunk_samples, codes_format, table, m_end=None, entry='pfb'):
    """channelize_recording's work -> (device tensor float32 [n_chan][2 * m_end], decim), streamed by _chunk_device.  The phase of a
    sample follows from its index in the capture, so no chunking changes a bit.  entry: 'pfb' (pss_pfb, n_chan a power of two) or 'bank'
    (pss_bank, n_chan = 2^a 3^b 5^c) — the streaming is the same."""
    e = get_engine()
    n_chan = int(n_chan)
    offsets, default_taps, run = {'pfb': (bank_offsets, e.pfb_default_taps, e.pfb), 'bank': (plan_offsets, e.bank_default_taps, e.bank)}[entry]
    offsets(1.0, n_chan)
    decim = n_chan // 2 if decim is None else int(decim)
    if decim < 1 or decim > n_chan:
        raise ValueError("decim outside [1, n_chan]")

    def plan():
        t = default_taps(n_chan) if taps is None else np.ascontiguousarray(taps, np.float64)
        return t, n_chan, lambda d_iq, n_buf, out, **window: run(d_iq, n_buf, n_chan, decim, out, taps=t, **window)

    return _chunk_device(e, samples, decim, lead, chunk_samples, codes_format, table, m_end, plan), decim


def channelize_recording(samples, fs, n_chan, decim=None, taps=None, lead=None, chunk_samples=1 << 22, codes_format=None, table=None):
    """What the reference's scan_frequencies and band sweep step their tuner through (pyspecsdr.py:1022-1093, :2523-2578) — a uniform grid
    of centre frequencies — done to a capture in one pass: all n_chan channels, fs / n_chan apart, low-pass filtered and decimated by
    `decim` on the GPU (pss_pfb, a polyphase filter bank) -> (channels complex64 [n_chan][ceil(n / decim)], offsets_hz float64 [n_chan]
    (bank_offsets), fs / decim).  A signal at fs + offsets_hz[c] lands at 0 Hz of row c; row c equals tune_recording's channel at that
    offset up to the two statements' rounding.  n_chan: a power of two in [2, 1024]; decim in [1, n_chan] (default n_chan // 2, the 2x
    oversampled bank; n_chan: critically sampled).  taps: a float64 low-pass table of at most 32 n_chan taps (default firwin(20 n_chan +
    1, 1 / n_chan)); lead: the tap that sits on an output's own sample (default the middle one: zero phase).  The capture is streamed in
    chunks of chunk_samples samples plus the halos the taps need; the result does not depend on chunk_samples.  codes_format / table: as
    demodulate_recording — `samples` is the ADC code array [n, 2], widened per chunk on the device."""
    d_out, decim = _bank_device(samples, n_chan, decim, taps, lead, chunk_samples, codes_format, table)
    return d_out.cpu().numpy().view(np.complex64), bank_offsets(fs, n_chan), float(fs) / decim


def _demodulate_rows(samples, fs, n_chan, decim, mode, frame_len, kw, entry, rows=None):
    """demodulate_bank's and monitor_channels' work -> (int16 [K][n_frames][n_out][2], decim, rate of the read buffers): the bank
    (_bank_device through `entry`) stops at a multiple of frame_len, `rows` of its result (None: all n_chan) are gathered on the device and
    demodulated as one batch of K * n_frames read buffers.  kw: taps, lead, chunk_samples, codes_format, table, exact_rate (True: the whole
    rows, resampled to plan_audio's rate by _exact_rate_rows before the cut)."""
    import torch
    if mode not in _MODES:
        raise ValueError(f"unknown demodulation mode {mode!r}")
    if int(frame_len) != frame_len or frame_len < 1:
        raise ValueError("frame_len must be an integer >= 1")
    frame_len, n_chan = int(frame_len), int(n_chan)
    {'pfb': bank_offsets, 'bank': plan_offsets}[entry](1.0, n_chan)
    decim = n_chan // 2 if decim is None else int(decim)
    if decim < 1 or decim > n_chan:
        raise ValueError("decim outside [1, n_chan]")
    opts = dict(taps=None, lead=None, chunk_samples=1 << 22, codes_format=None, table=None, exact_rate=False)
    for k in kw:
        if k not in opts:
            raise TypeError(f"unexpected argument {k!r}")
    opts.update(kw)
    e = get_engine()
    n_frames = e.lib.pss_ddc_out_len(len(samples), decim) // frame_len
    rate_out = float(fs) / decim
    if opts['exact_rate']:
        rate_out = plan_audio(rate_out, mode)[2]
    rate = float(DEFAULT_SAMPLE_RATE) if mode == 'AM' else rate_out
    if mode != 'AM':
        _inject_designs({'NFM': 'nfm', 'WFM': 'wfm'}.get(mode, 'ssb'), rate)
    n_out = e.demod_out_len(_MODES[mode], frame_len, rate)
    if n_out < 0:
        raise ValueError("the channel rate fs / decim is below the target rate")
    d_iq, _ = _bank_device(samples, n_chan, decim, opts['taps'], opts['lead'], opts['chunk_samples'], opts['codes_format'], opts['table'],
                           m_end=None if opts['exact_rate'] else n_frames * frame_len, entry=entry)
    if rows is not None:
        d_iq = d_iq.index_select(0, torch.from_numpy(rows).to(d_iq.device))
    if opts['exact_rate']:
        d_iq, n_frames, _ = _exact_rate_rows(d_iq, float(fs) / decim, mode, frame_len)
    k = d_iq.shape[0]
    d_pcm = torch.empty((k * n_frames, n_out, 2), dtype=torch.int16, device=d_iq.device)
    if k * n_frames:
        e.demod_signal(_MODES[mode], d_iq, k * n_frames, frame_len, rate, d_pcm)
    return d_pcm.cpu().numpy().reshape(k, n_frames, n_out, 2), decim, rate_out


def demodulate_bank(samples, fs, n_chan, decim=None, mode='NFM', frame_len=32768, **kw):
    """Listen to every channel of the grid: channelize_recording's rows, cut into read buffers of frame_len samples at fs / decim and
    demodulated as demodulate_signal would -> int16 [n_chan][n_frames][n_out][2].  The bank stops at a multiple of frame_len (an incomplete
    tail buffer is dropped, as cut_frames does), so its result IS the batch of n_chan * n_frames read buffers on the device: nothing comes
    back to the host between the two steps.  kw: taps, lead, chunk_samples, codes_format, table, exact_rate (as monitor_channels)."""
    return _demodulate_rows(samples, fs, n_chan, decim, mode, frame_len, kw, 'pfb')[0]


def _smooth5(n):
    """n = 2^a 3^b 5^c."""
    for p in (2, 3, 5):
        while n > 1 and n % p == 0:
            n //= p
    return n == 1


def _plan_ok(n_chan):
    return 2 <= n_chan <= 1024 and _smooth5(n_chan)


def plan_offsets(fs, n_chan):
    """bank_offsets for the channeliser of band plans, any n_chan = 2^a 3^b 5^c in [2, 1024] -> float64 [n_chan]: c fs / n_chan for
    c <= (n_chan - 1) / 2 and (c - n_chan) fs / n_chan otherwise (even n_chan: row n_chan / 2, the band edge, reads -fs / 2; odd n_chan
    has no such row)."""
    n_chan = int(n_chan)
    if not _plan_ok(n_chan):
        raise ValueError("n_chan must be of the form 2^a 3^b 5^c in [2, 1024]")
    c = np.arange(n_chan, dtype=np.float64)
    return np.where(c <= (n_chan - 1) // 2, c, c - n_chan) * (float(fs) / n_chan)


def plan_bank(fs, spacing_hz, min_rate=None):
    """The bank of a band plan -> (n_chan, decim): the grid of a capture at fs with channels spacing_hz apart has n_chan = fs / spacing_hz
    channels, which must be an integer (to 1e-9 relative) of the form 2^a 3^b 5^c in [2, 1024]; decim is the largest divisor of n_chan
    that leaves a channel rate fs / decim >= min_rate (default max(2 spacing_hz, 48 000): the NFM demodulator needs a channel rate above
    30 kS/s, which n_chan // 2 misses on a 12.5 kHz grid).  12.5 kHz at 2.4 MS/s -> (192, 48): 50 kS/s."""
    fs, spacing_hz = float(fs), float(spacing_hz)
    if not (fs > 0 and spacing_hz > 0):
        raise ValueError("fs and spacing_hz must be positive")
    ratio = fs / spacing_hz
    n_chan = int(round(ratio))
    if abs(ratio - n_chan) > 1e-9 * ratio:
        raise ValueError(f"fs / spacing_hz = {ratio!r} is not an integer: the grid does not close on this capture")
    if not _plan_ok(n_chan):
        near = [next((m for m in rng if _plan_ok(m)), None) for rng in (range(min(n_chan - 1, 1024), 1, -1), range(max(n_chan + 1, 2), 1025))]
        raise ValueError(f"fs / spacing_hz = {n_chan} channels is not of the form 2^a 3^b 5^c in [2, 1024]; the nearest such counts: "
                         + ", ".join(str(m) for m in near if m is not None))
    min_rate = max(2.0 * spacing_hz, 48000.0) if min_rate is None else float(min_rate)
    fits = [d for d in range(1, n_chan + 1) if n_chan % d == 0 and fs / d >= min_rate]
    if not fits:
        raise ValueError(f"the capture's own rate {fs!r} is below min_rate {min_rate!r}")
    return n_chan, fits[-1]


def channelize_plan(samples, fs, spacing_hz, decim=None, taps=None, lead=None, chunk_samples=1 << 22, codes_format=None, table=None):
    """channelize_recording for a band plan — what the reference's memory-channel mode steps its tuner through, done to a capture in one
    pass: every channel of the grid spacing_hz apart (25 kHz: marine VHF, 2 m repeaters; 12.5 kHz: PMR446; 10 kHz: CB) on the GPU
    (pss_bank) -> (channels complex64 [n_chan][ceil(n / decim)], offsets_hz float64 [n_chan] (plan_offsets), fs / decim).  n_chan and
    the default decim are plan_bank(fs, spacing_hz)'s.  taps, lead, chunk_samples, codes_format, table: as channelize_recording; the
    result does not depend on chunk_samples."""
    n_chan, d = plan_bank(fs, spacing_hz)
    d_out, decim = _bank_device(samples, n_chan, d if decim is None else decim, taps, lead, chunk_samples, codes_format, table, entry='bank')
    return d_out.cpu().numpy().view(np.complex64), plan_offsets(fs, n_chan), float(fs) / decim


def plan_rows(fs, center_hz, channels_hz, spacing_hz):
    """The row of each listed channel frequency in the bank of a capture centred on center_hz -> int array [K]: f belongs to row
    round((f - center_hz) / spacing_hz) mod n_chan.  ValueError lists every f more than 1 Hz off the grid or outside +-fs / 2."""
    n_chan, _ = plan_bank(fs, spacing_hz)
    f = np.atleast_1d(np.asarray(channels_hz, np.float64))
    if f.ndim != 1:
        raise ValueError("channels_hz: a list of frequencies")
    steps = (f - float(center_hz)) / float(spacing_hz)
    rows = np.rint(steps)
    off = (np.abs(steps - rows) * float(spacing_hz) > 1.0) | (np.abs(f - float(center_hz)) > float(fs) / 2) | ~np.isfinite(f)
    if off.any():
        raise ValueError("not on the grid of this capture (more than 1 Hz off a channel centre, or outside +-fs / 2): "
                         + ", ".join(repr(float(v)) for v in f[off]))
    return np.mod(rows.astype(np.int64), n_chan)


def monitor_channels(samples, fs, center_hz, channels_hz, spacing_hz, mode='NFM', frame_len=32768, **kw):
    """The reference's memory-channel mode done to a capture: listen to the listed channel frequencies of one wideband capture centred on
    center_hz -> (pcm int16 [K][n_frames][n_out][2], rows int [K], fs / decim).  The whole grid goes through the bank (channelize_plan's
    work), the K listed rows (plan_rows) are gathered on the device and demodulated as demodulate_signal would; nothing comes back to the
    host in between.  The bank stops at a multiple of frame_len, as demodulate_bank does.  kw: decim, taps, lead, chunk_samples,
    codes_format, table, exact_rate.  exact_rate=True: the gathered rows are resampled on the device (pss_resample) to plan_audio(fs /
    decim, mode)'s rate before they are cut into read buffers, so the PCM is at exactly DEFAULT_SAMPLE_RATE — what write_wav and the
    audio FIFO promise; the frame count follows the resampled length and the rate returned is that rate (44 100.0 for NFM, 22 050.0
    for AM / USB / LSB, 110 250.0 for WFM).  Default False: a 50 kS/s channel row gives NFM audio at 25 000 Hz and AM audio at 50 000 Hz."""
    kw = dict(kw)
    decim = kw.pop('decim', None)
    n_chan, d = plan_bank(fs, spacing_hz)
    rows = plan_rows(fs, center_hz, channels_hz, spacing_hz)
    pcm, decim, rate = _demodulate_rows(samples, fs, n_chan, d if decim is None else decim, mode, frame_len, kw, 'bank', rows=rows)
    return pcm, rows, rate


_RDS_RATE = 19000


def _rds_char(c):
    return chr(c) if 0x20 <= c <= 0x7E or 0xA0 <= c <= 0xFF else '?'


def rds_decode(groups):
    """The groups of ONE row (uint16 [n][4], in the order received) -> dict: 'pi' (the most frequent block 1; None without groups), 'pty',
    'tp' (of the last group), 'group_counts' ({'0A': n, ...}), 'ps' (the eight-character name from groups 0A / 0B, two characters per
    segment address; None until all four segments have been seen), 'radiotext' (from 2A, four characters per address, and 2B, two;
    cleared when the A/B flag toggles; up to 0x0D, or to the first character not yet received; None while character 0 is missing).
    Characters are read as Latin-1 with unprintables as '?' (the standard's own code table is not applied).  Host code, pure Python."""
    groups = np.asarray(groups, np.uint16).reshape(-1, 4)
    out = {'pi': None, 'pty': None, 'tp': None, 'group_counts': {}, 'ps': None, 'radiotext': None}
    if not len(groups):
        return out
    pis, counts = np.unique(groups[:, 0], return_counts=True)
    out['pi'] = int(pis[np.argmax(counts)])
    ps, rt, flag = [None] * 8, [None] * 64, None
    for a, b, c, d in ((int(v) for v in g) for g in groups):
        gtype, version_b = b >> 12, (b >> 11) & 1
        name = f"{gtype}{'B' if version_b else 'A'}"
        out['group_counts'][name] = out['group_counts'].get(name, 0) + 1
        out['tp'], out['pty'] = (b >> 10) & 1, (b >> 5) & 31
        if gtype == 0:
            seg = b & 3
            ps[2 * seg], ps[2 * seg + 1] = d >> 8, d & 255
        elif gtype == 2:
            if flag is not None and flag != (b >> 4) & 1:
                rt = [None] * 64
            flag = (b >> 4) & 1
            addr = b & 15
            chars = [d >> 8, d & 255] if version_b else [c >> 8, c & 255, d >> 8, d & 255]
            rt[len(chars) * addr:len(chars) * (addr + 1)] = chars
    if all(v is not None for v in ps):
        out['ps'] = ''.join(_rds_char(v) for v in ps)
    text = []
    for v in rt:
        if v is None or v == 0x0D:
            break
        text.append(_rds_char(v))
    if rt[0] is not None:
        out['radiotext'] = ''.join(text)
    return out


def _rds_rows(e, d_iq, n_rows, n, fs, taps=None, pulse=None, d_front=None):
    """The stages behind the IQ rows on the device -> (groups uint16 [n_rows][max_groups][4], pos int32 [n_rows][max_groups], n_groups
    int32 [n_rows]) on the host.  d_iq: float32 tensor [n_rows][2 n] at fs, or None with d_front, the front's rows (float32
    [n_rows][2 m] at fs / decim)."""
    import torch
    decim, up, down = e.rds_plan(fs)
    if d_front is None:
        m = e.lib.pss_ddc_out_len(n, decim)
        d_front = torch.empty((n_rows, 2 * m), dtype=torch.float32, device=d_iq.device)
        e.rds_front(d_iq, n_rows, n, fs, decim, d_front, taps=taps)
    m = d_front.shape[1] // 2
    dev = d_front.device
    n19 = e.resample_out_len(m, up, down)
    d_bb = torch.empty((n_rows, 2 * n19), dtype=torch.float32, device=dev)
    e.resample(d_front, np.complex64, n_rows, m, up, down, d_bb)
    max_bits = e.rds_max_bits(n19)
    max_groups = max_bits // 104 + 1
    d_bits = torch.empty((n_rows, max_bits), dtype=torch.uint8, device=dev)
    d_n_bits = torch.empty(n_rows, dtype=torch.int32, device=dev)
    e.rds_bits(d_bb, n_rows, n19, d_bits, max_bits, d_n_bits, pulse=pulse)
    d_groups = torch.zeros((n_rows, max_groups, 4), dtype=torch.int16, device=dev)
    d_pos = torch.zeros((n_rows, max_groups), dtype=torch.int32, device=dev)
    d_n_groups = torch.empty(n_rows, dtype=torch.int32, device=dev)
    e.rds_groups(d_bits, d_n_bits, n_rows, max_bits, d_groups, d_pos, max_groups, d_n_groups)
    return d_groups.cpu().numpy().view(np.uint16), d_pos.cpu().numpy(), d_n_groups.cpu().numpy()


def rds_recording(samples, fs, taps=None, pulse=None, chunk_samples=1 << 22, codes_format=None, table=None):
    """RDS of one station's capture (the station at 0 Hz of a capture at fs, an integer rate above 120 kS/s) -> rds_decode's dict with
    'groups' (uint16 [n][4]) and 'pos' (the bit index of each group) added.  On the GPU: discriminator + 57 kHz mixer + decimating FIR
    (pss_rds_front, streamed in chunks of chunk_samples samples plus their halos; the result does not depend on chunk_samples), the
    resampler to 19 kS/s, symbol timing and differential detection (pss_rds_bits) and the block check (pss_rds_groups) on the whole row.
    taps: the front's float64 low-pass table (default firwin(20 decim + 1, 1 / decim)); pulse: the matched filter (default
    rds_default_pulse()); codes_format / table: as demodulate_recording."""
    e = get_engine()
    fs = float(fs)
    decim = e.rds_plan(fs)[0]

    def plan():
        t = e.ddc_default_taps(decim) if taps is None else np.ascontiguousarray(taps, np.float64)
        return t, 1, lambda d_iq, n_buf, out, **window: e.rds_front(d_iq, 1, n_buf, fs, decim, out, taps=t, **window)

    d_front = _chunk_device(e, samples, decim, None, chunk_samples, codes_format, table, None, plan, reach_back=1)
    groups, pos, n_groups = _rds_rows(e, None, 1, 0, fs, pulse=pulse, d_front=d_front)
    k = min(int(n_groups[0]), groups.shape[1])
    out = rds_decode(groups[0, :k])
    out['groups'], out['pos'] = groups[0, :k].copy(), pos[0, :k].copy()
    return out


def rds_stations(samples, fs, center_hz, spacing_hz=100e3, taps=None, pulse=None, chunk_samples=1 << 22, codes_format=None, table=None):
    """Which station is on each channel of a capture of the FM band centred on center_hz -> a list of (frequency_hz, pi, ps, radiotext,
    n_groups), one entry per row of the bank that produced at least one group, in ascending frequency.  The grid goes through the bank
    (plan_bank(fs, spacing_hz), pss_bank: 100 kHz channels come out at 200 kS/s), then all rows at once through pss_rds_front, the
    resampler, pss_rds_bits and pss_rds_groups; only the groups come back to the host.  A strong station also decodes in the rows next
    to its own: adjacent rows that report the same PI are ALL listed, and merging them is the caller's business.  taps: the BANK's
    table; the default is firwin(20 n_chan + 1, 1.8 / n_chan), a channel 1.8 spacings wide (+-90 kHz on the 100 kHz grid), not
    bank_default_taps' one spacing: the RDS subcarrier sits 57 kHz either side of the FM carrier, outside a +-50 kHz channel.  pulse,
    chunk_samples, codes_format, table: as rds_recording."""
    e = get_engine()
    n_chan, decim = plan_bank(fs, spacing_hz)
    rate = float(fs) / decim
    e.rds_plan(rate)   # refuses a channel rate the receiver does not take before any work is done
    if taps is None:
        taps = np.empty(20 * n_chan + 1, np.float64)
        if e.lib.pss_design_firwin(len(taps), 1.8 / n_chan, taps.ctypes.data) != 0:
            raise ValueError("rds_stations: the bank's filter design failed")
    d_rows, _ = _bank_device(samples, n_chan, decim, taps, None, chunk_samples, codes_format, table, entry='bank')
    groups, _, n_groups = _rds_rows(e, d_rows, n_chan, d_rows.shape[1] // 2, rate, pulse=pulse)
    freqs = float(center_hz) + plan_offsets(fs, n_chan)
    out = []
    for c in np.argsort(freqs):
        k = min(int(n_groups[c]), groups.shape[1])
        if k:
            d = rds_decode(groups[c, :k])
            out.append((float(freqs[c]), d['pi'], d['ps'], d['radiotext'], k))
    return out


# -- ADS-B: what the frames of pss_adsb_frames say (host code), and a capture end to end
_ADSB_CHARS = "#ABCDEFGHIJKLMNOPQRSTUVWXYZ##### ###############0123456789######"
_ADSB_OVERLAID = (0, 4, 5, 16, 20, 21)   # the formats whose parity field carries the address


def adsb_decode(msg, n_bits):
    """One Mode S message (14 bytes as pss_adsb_frames writes them, or the frame's own 7 / 14) -> a dict.  Always 'df' and 'icao' (the AA
    field of DF 11 / 17 / 18; the remainder of the address-overlaid formats).  DF 17 / 18: 'tc', the type code, and with it
      1 - 4    'callsign' (the 6-bit table, trailing spaces stripped)
      9 - 18   'altitude' in feet (None unless the Q bit is set), 'odd' (the CPR format flag), 'cpr_lat', 'cpr_lon' (17 bits each)
      19       subtypes 1 and 2: 'speed' in knots, 'track' in degrees, 'vertical_rate' in ft/min (None where the field says "no data").
    Pure Python: no library call but the remainder."""
    m = bytes(np.asarray(msg, np.uint8).tobytes() if not isinstance(msg, (bytes, bytearray)) else msg)
    n_bits = int(n_bits)
    if n_bits not in (56, 112) or len(m) < n_bits // 8:
        raise ValueError("adsb_decode: n_bits is 56 or 112, and msg holds that many")
    m = m[:n_bits // 8]
    df = m[0] >> 3
    out = {'df': df}
    if df in (11, 17, 18):
        out['icao'] = int.from_bytes(m[1:4], 'big')
    else:
        from .engine import Engine
        out['icao'] = Engine.adsb_crc(m, n_bits) if df in _ADSB_OVERLAID else None
    if df not in (17, 18):
        return out
    me = int.from_bytes(m[4:11], 'big')
    tc = me >> 51
    out['tc'] = tc
    if 1 <= tc <= 4:
        out['callsign'] = "".join(_ADSB_CHARS[(me >> (42 - 6 * k)) & 0x3F] for k in range(8)).rstrip(" ")
    elif 9 <= tc <= 18:
        alt = (me >> 36) & 0xFFF
        out['altitude'] = (((alt & 0xFE0) >> 1) | (alt & 0xF)) * 25 - 1000 if alt & 0x10 else None
        out['odd'] = (me >> 34) & 1
        out['cpr_lat'], out['cpr_lon'] = (me >> 17) & 0x1FFFF, me & 0x1FFFF
    elif tc == 19 and (me >> 48) & 7 in (1, 2):
        scale = 4 if (me >> 48) & 7 == 2 else 1
        ew, ns, vr = (me >> 32) & 0x3FF, (me >> 21) & 0x3FF, (me >> 10) & 0x1FF
        out['speed'] = out['track'] = None
        if ew and ns:
            vx = (ew - 1) * scale * (-1 if (me >> 42) & 1 else 1)
            vy = (ns - 1) * scale * (-1 if (me >> 31) & 1 else 1)
            out['speed'] = float(np.hypot(vx, vy))
            out['track'] = float(np.degrees(np.arctan2(vx, vy)) % 360.0)
        out['vertical_rate'] = (vr - 1) * 64 * (-1 if (me >> 19) & 1 else 1) if vr else None
    return out


def _cpr_nl(lat):
    """The number of longitude zones at a latitude (the standard's NL function)."""
    lat = abs(lat)
    if lat == 0:
        return 59
    if lat == 87:
        return 2
    if lat > 87:
        return 1
    return int(np.floor(2 * np.pi / np.arccos(1 - (1 - np.cos(np.pi / 30)) / np.cos(np.pi / 180 * lat) ** 2)))


def adsb_position(even, odd, newest_odd):
    """The globally unambiguous CPR decode of an even and an odd airborne position, each (cpr_lat, cpr_lon) -> (latitude, longitude) in
    degrees as float64, or None where the two latitudes fall in different longitude zones.  newest_odd: the odd frame is the later one."""
    lat_e, lon_e = even[0] / 131072.0, even[1] / 131072.0
    lat_o, lon_o = odd[0] / 131072.0, odd[1] / 131072.0
    j = int(np.floor(59 * lat_e - 60 * lat_o + 0.5))
    la_e, la_o = 360.0 / 60 * (j % 60 + lat_e), 360.0 / 59 * (j % 59 + lat_o)
    la_e, la_o = (la_e - 360 if la_e >= 270 else la_e), (la_o - 360 if la_o >= 270 else la_o)
    nl = _cpr_nl(la_e)
    if nl != _cpr_nl(la_o):
        return None
    m = int(np.floor(lon_e * (nl - 1) - lon_o * nl + 0.5))
    lat, ni, frac = (la_o, max(nl - 1, 1), lon_o) if newest_odd else (la_e, max(nl, 1), lon_e)
    lon = 360.0 / ni * (m % ni + frac)
    return lat, (lon - 360 if lon >= 180 else lon)


def adsb_tracks(records, fs):
    """records: the frames in order, each a mapping with 'msg', 'n_bits' and 'pos' (adsb_recording's 'frames') -> one dict per aircraft in
    order of first appearance: 'icao', 'callsign', 'altitude' and 'velocity' (the last of each, or None), 'frames', 'first' and 'last' (pos / fs,
    seconds) and 'position': (latitude, longitude) from the newest even and the newest odd position frame where they lie within 10 s of each
    other and their latitudes fall in the same longitude zone, else None."""
    fs = float(fs)
    tracks, cpr = {}, {}
    for rec in records:
        d = adsb_decode(rec['msg'], rec['n_bits'])
        if d['icao'] is None:
            continue
        t = int(rec['pos']) / fs
        tr = tracks.setdefault(d['icao'], {'icao': d['icao'], 'callsign': None, 'altitude': None, 'velocity': None, 'frames': 0, 'first': t,
                                           'last': t, 'position': None})
        tr['frames'] += 1
        tr['last'] = t
        if 'callsign' in d:
            tr['callsign'] = d['callsign']
        if d.get('altitude') is not None:
            tr['altitude'] = d['altitude']
        if 'vertical_rate' in d:
            tr['velocity'] = {k: d[k] for k in ('speed', 'track', 'vertical_rate')}
        if 'cpr_lat' in d:
            cpr.setdefault(d['icao'], {})[d['odd']] = (t, (d['cpr_lat'], d['cpr_lon']))
    for icao, pair in cpr.items():
        if 0 in pair and 1 in pair and abs(pair[0][0] - pair[1][0]) <= 10.0:
            tracks[icao]['position'] = adsb_position(pair[0][1], pair[1][1], newest_odd=pair[1][0] > pair[0][0])
    return list(tracks.values())


def _adsb_pass(e, upload, n, spc, ratio, addresses, chunk):
    """One pass over a capture of n samples -> the records on the host: (msg [k][14], pos, meta, score).  upload(lo, hi) -> a float32 device
    tensor holding samples [lo, hi).  Each chunk of `chunk` starts goes up with the halo its starts and their suppressors read."""
    import torch
    dev = f"cuda:{e.device}"
    a = np.array(sorted({int(x) for x in addresses}), np.uint32)
    d_icao = torch.from_numpy(a.view(np.int32)).to(dev) if len(a) else None
    room = 4096
    d_msg = torch.empty((room, 14), dtype=torch.uint8, device=dev)
    d_pos = torch.empty(room, dtype=torch.int64, device=dev)
    d_meta = torch.empty(room, dtype=torch.int32, device=dev)
    d_score = torch.empty(room, dtype=torch.float32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    parts = []
    for s0 in range(0, n, chunk):
        s1 = min(n, s0 + chunk)
        lo, hi = max(0, s0 - (2 * spc - 1)), min(n, s1 + 2 * spc - 2 + 240 * spc)
        d_iq = upload(lo, hi)
        while True:
            e.adsb_frames(d_iq, hi - lo, spc, d_msg, d_pos, d_meta, d_score, d_count, room, ratio=ratio, d_icao=d_icao, n_icao=len(a), buf_index0=lo,
                          n_capture=n, s_begin=s0, s_end=s1)
            k = int(d_count.cpu()[0])
            if k <= room:
                break
            room = k   # the true count: the chunk again with room for it
            d_msg = torch.empty((room, 14), dtype=torch.uint8, device=dev)
            d_pos = torch.empty(room, dtype=torch.int64, device=dev)
            d_meta = torch.empty(room, dtype=torch.int32, device=dev)
            d_score = torch.empty(room, dtype=torch.float32, device=dev)
        parts.append((d_msg[:k].cpu().numpy(), d_pos[:k].cpu().numpy(), d_meta[:k].cpu().numpy().view(np.uint32), d_score[:k].cpu().numpy()))
    if not parts:
        return np.zeros((0, 14), np.uint8), np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def adsb_recording(samples, fs, ratio=2.0, addresses=(), learn=True, chunk_samples=1 << 22, codes_format=None, table=None):
    """The aircraft of a 1090 MHz capture -> dict(frames=..., tracks=..., fs=...): 'frames' a list of dicts in order of 'pos' (adsb_decode's keys
    and 'msg' (bytes), 'n_bits', 'pos', 'score'), 'tracks' adsb_tracks(frames, fs), 'fs' the rate the positions count in.
    At a multiple of 2 MS/s up to 16 MS/s the capture is streamed through pss_adsb_frames in chunks of chunk_samples starts, each with its
    halo; the result does not depend on chunk_samples.  Another integer rate is first brought to the next multiple of 2 MS/s by pss_resample
    on the resident complex64 row (2.4 MS/s -> 4 MS/s): such a capture has to fit on the device.
    addresses: the aircraft whose address-overlaid replies (DF 0 / 4 / 5 / 16 / 20 / 21) are wanted.  learn: a second pass runs with these
    and every address seen in an accepted DF 11 / 17 / 18 frame of the first, and ITS result is the answer (the capture is read twice).
    codes_format / table: as rds_recording; codes are widened per chunk on the device."""
    import torch
    e = get_engine()
    fs = float(fs)
    if int(chunk_samples) != chunk_samples or chunk_samples < 1:
        raise ValueError("chunk_samples must be an integer >= 1")
    chunk = int(chunk_samples)
    dev = f"cuda:{e.device}"
    if codes_format is not None:
        iq = _iq_args(codes_format, table)
        samples = _iq_codes(samples, iq[0])
        if samples.ndim != 2:
            raise ValueError("codes: [n, 2]")
    else:
        samples = np.ascontiguousarray(samples, np.complex64)
        if samples.ndim != 1:
            raise ValueError("samples: a 1-D recording")

    def from_host(lo, hi):
        if codes_format is None:
            return torch.from_numpy(samples[lo:hi].view(np.float32)).to(dev)
        d_iq = torch.empty(2 * (hi - lo), dtype=torch.float32, device=dev)
        e.unpack_iq(torch.from_numpy(np.array(samples[lo:hi])).to(dev), hi - lo, d_iq, codes_format, iq[2])
        return d_iq

    n = len(samples)
    upload = from_host
    if fs % 2e6 != 0.0:
        rate = 2e6 * np.ceil(fs / 2e6)
        up, down = plan_resample(fs, rate)
        d_in = from_host(0, n) if n else torch.empty(2, dtype=torch.float32, device=dev)
        n_out = e.resample_out_len(n, up, down)
        d_row = torch.empty(2 * max(n_out, 1), dtype=torch.float32, device=dev)
        if n:
            e.resample(d_in, np.complex64, 1, n, up, down, d_row)
        del d_in
        fs, n = float(rate), n_out
        upload = lambda lo, hi: d_row[2 * lo:2 * hi]   # noqa: E731  (resident: a chunk is a view)
    spc = e.adsb_plan(fs)
    known = {int(a) for a in addresses}
    rec = _adsb_pass(e, upload, n, spc, ratio, known, chunk)
    if learn:
        seen = {int.from_bytes(bytes(m[1:4]), 'big') for m, w in zip(rec[0], rec[2]) if (int(w) >> 16) in (11, 17, 18)}
        if not seen <= known:
            rec = _adsb_pass(e, upload, n, spc, ratio, known | seen, chunk)
    frames = []
    for m, p, w, sc in zip(*rec):
        nb = int(w) & 0xFFFF
        d = adsb_decode(m, nb)
        d.update(msg=bytes(m[:nb // 8]), n_bits=nb, pos=int(p), score=float(sc))
        frames.append(d)
    return dict(frames=frames, tracks=adsb_tracks(frames, fs), fs=fs)


# -- AIS: what the frames of pss_ais_frames say (host code), and a capture end to end
_AIS_RATE = 48000


def _ais_bytes(msg):
    return bytes(msg) if isinstance(msg, (bytes, bytearray)) else np.asarray(msg, np.uint8).tobytes()


def ais_decode(msg):
    """One AIS message (the frame's bytes as pss_ais_frames writes them, with or without the two check bytes; message bit p of ITU-R M.1371,
    0 = the most significant bit of the message id, is bit 7 - p % 8 of byte p // 8) -> a dict.  Always 'type', 'repeat', 'mmsi'.  With them
      1 / 2 / 3  'status', 'turn' (degrees a minute; None at "not available"), 'speed' (knots), 'accuracy', 'lon', 'lat' (degrees; None at
                 181 / 91), 'course', 'heading' (degrees), 'second'
      4          'year' ... 'second', 'accuracy', 'lon', 'lat'
      5          'imo', 'callsign', 'name', 'ship_type', 'to_bow', 'to_stern', 'to_port', 'to_starboard', 'eta' (month, day, hour, minute),
                 'draught' (metres), 'destination' (6-bit text: cut at the first '@', trailing spaces stripped)
      18 / 19    class B: 'speed', 'accuracy', 'lon', 'lat', 'course', 'heading', 'second'; 19 adds 'name', 'ship_type' and the dimensions
      21         aid to navigation: 'aid_type', 'name', 'accuracy', 'lon', 'lat', the dimensions, 'second', 'off_position'
      24         'part' 0: 'name'; 1: 'ship_type', 'vendor', 'callsign', the dimensions
    Any other type, or a message too short for its type: only the three common keys.  Pure Python."""
    m = _ais_bytes(msg)
    if len(m) < 5:
        raise ValueError("ais_decode: a message holds at least 38 bits")
    word, n_bits = int.from_bytes(m, 'big'), 8 * len(m)

    def u(p, w):
        if p + w > n_bits:
            raise IndexError
        return (word >> (n_bits - p - w)) & ((1 << w) - 1)

    def s(p, w):
        v = u(p, w)
        return v - (1 << w) if v >> (w - 1) else v

    def text(p, n_chars):
        chars = [u(p + 6 * k, 6) for k in range(n_chars)]
        t = ''.join(chr(c + 64) if c < 32 else chr(c) for c in chars)
        return t.split('@')[0].rstrip(' ')

    def na(v, code, scale=1.0):
        return None if v == code else v / scale

    def lonlat(p):
        lon, lat = s(p, 28), s(p + 28, 27)
        return (None if lon == 181 * 600000 else lon / 600000.0), (None if lat == 91 * 600000 else lat / 600000.0)

    def dims(p):
        return dict(to_bow=u(p, 9), to_stern=u(p + 9, 9), to_port=u(p + 18, 6), to_starboard=u(p + 24, 6))

    out = {'type': u(0, 6), 'repeat': u(6, 2), 'mmsi': u(8, 30)}
    t, d = out['type'], {}
    try:
        if t in (1, 2, 3):
            rot = s(42, 8)
            d = dict(status=u(38, 4), turn=None if rot == -128 else float(np.sign(rot)) * (rot / 4.733) ** 2, speed=na(u(50, 10), 1023, 10.0),
                     accuracy=u(60, 1), course=na(u(116, 12), 3600, 10.0), heading=na(u(128, 9), 511), second=u(137, 6))
            d['lon'], d['lat'] = lonlat(61)
            if d['heading'] is not None:
                d['heading'] = int(d['heading'])
        elif t == 4:
            d = dict(year=u(38, 14), month=u(52, 4), day=u(56, 5), hour=u(61, 5), minute=u(66, 6), second=u(72, 6), accuracy=u(78, 1))
            d['lon'], d['lat'] = lonlat(79)
        elif t == 5:
            d = dict(imo=u(40, 30), callsign=text(70, 7), name=text(112, 20), ship_type=u(232, 8), **dims(240),
                     eta=(u(274, 4), u(278, 5), u(283, 5), u(288, 6)), draught=u(294, 8) / 10.0, destination=text(302, 20))
        elif t in (18, 19):
            d = dict(speed=na(u(46, 10), 1023, 10.0), accuracy=u(56, 1), course=na(u(112, 12), 3600, 10.0), heading=na(u(124, 9), 511), second=u(133, 6))
            d['lon'], d['lat'] = lonlat(57)
            if d['heading'] is not None:
                d['heading'] = int(d['heading'])
            if t == 19:
                d.update(name=text(143, 20), ship_type=u(263, 8), **dims(271))
        elif t == 21:
            d = dict(aid_type=u(38, 5), name=text(43, 20), accuracy=u(163, 1), **dims(219), second=u(253, 6), off_position=u(259, 1))
            d['lon'], d['lat'] = lonlat(164)
        elif t == 24:
            d = dict(part=u(38, 2))
            if d['part'] == 0:
                d['name'] = text(40, 20)
            elif d['part'] == 1:
                d.update(ship_type=u(40, 8), vendor=text(48, 7), callsign=text(90, 7), **dims(132))
    except IndexError:
        d = {}
    out.update(d)
    return out


def ais_nmea(msg, channel='A', seq=0):
    """The !AIVDM sentences of one message (its bytes WITHOUT the two check bytes) -> a list of str: the payload in 6-bit armour, at most 56
    characters (336 bits) a sentence, the fill bits on the last one, the XOR checksum behind '*'.  seq: the sequence digit of a message of
    several sentences (a single sentence leaves the field empty)."""
    m = _ais_bytes(msg)
    n_bits = 8 * len(m)
    fill = (6 - n_bits % 6) % 6
    word = int.from_bytes(m, 'big') << fill
    n_chars = (n_bits + fill) // 6
    chars = []
    for k in range(n_chars):
        v = (word >> (6 * (n_chars - 1 - k))) & 63
        chars.append(chr(v + 48 if v < 40 else v + 56))
    parts = [''.join(chars[i:i + 56]) for i in range(0, max(n_chars, 1), 56)]
    out = []
    for i, part in enumerate(parts):
        body = "AIVDM,%d,%d,%s,%s,%s,%d" % (len(parts), i + 1, "" if len(parts) == 1 else str(int(seq) % 10), channel, part,
                                            fill if i == len(parts) - 1 else 0)
        cs = 0
        for ch in body:
            cs ^= ord(ch)
        out.append("!%s*%02X" % (body, cs))
    return out


def ais_payload(sentences):
    """ais_nmea backwards: the sentences of ONE message in order -> its bytes (the fill bits dropped).  ValueError on a wrong checksum."""
    bits, fill = [], 0
    for sen in sentences:
        body, _, cs = sen[1:].partition('*')
        x = 0
        for ch in body:
            x ^= ord(ch)
        if sen[0] != '!' or int(cs, 16) != x:
            raise ValueError("ais_payload: a wrong checksum")
        f = body.split(',')
        for ch in f[5]:
            v = ord(ch) - 48
            v = v - 8 if v > 40 else v
            bits.extend((v >> (5 - k)) & 1 for k in range(6))
        fill = int(f[6])
    bits = bits[:len(bits) - fill] if fill else bits
    return np.packbits(np.array(bits[:len(bits) // 8 * 8], np.uint8)).tobytes()


def ais_tracks(records, fs=_AIS_RATE):
    """records: the frames in order, each a mapping with 'msg' and 'pos' (ais_recording's 'frames') -> one dict per MMSI in order of first
    appearance: 'mmsi', 'name', 'callsign', 'ship_type', 'position' ((latitude, longitude)), 'speed', 'course' (the last of each, or None),
    'frames', 'first' and 'last' (pos / fs, seconds)."""
    fs = float(fs)
    tracks = {}
    for rec in records:
        d = ais_decode(rec['msg'])
        t = int(rec['pos']) / fs
        tr = tracks.setdefault(d['mmsi'], {'mmsi': d['mmsi'], 'name': None, 'callsign': None, 'ship_type': None, 'position': None, 'speed': None,
                                           'course': None, 'frames': 0, 'first': t, 'last': t})
        tr['frames'] += 1
        tr['first'], tr['last'] = min(tr['first'], t), max(tr['last'], t)
        for key in ('name', 'callsign', 'ship_type', 'speed', 'course'):
            if d.get(key) not in (None, ''):
                tr[key] = d[key]
        if d.get('lat') is not None and d.get('lon') is not None:
            tr['position'] = (d['lat'], d['lon'])
    return list(tracks.values())


def _ais_rows(e, d_y, n_rows, n):
    """pss_ais_frames on resident rows -> the records on the host: (msg [k][128], len, row, pos, score)."""
    import torch
    dev = d_y.device
    room = 4096
    while True:
        d_msg = torch.empty((room, 128), dtype=torch.uint8, device=dev)
        d_len = torch.empty(room, dtype=torch.int32, device=dev)
        d_row = torch.empty(room, dtype=torch.int32, device=dev)
        d_pos = torch.empty(room, dtype=torch.int64, device=dev)
        d_score = torch.empty(room, dtype=torch.float32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        e.ais_frames(d_y, n_rows, n, d_msg, d_len, d_row, d_pos, d_score, d_count, room)
        k = int(d_count.cpu()[0])
        if k <= room:
            break
        room = k   # the true count: again with room for it
    return tuple(t[:k].cpu().numpy() for t in (d_msg, d_len, d_row, d_pos, d_score))


def ais_recording(samples, fs, center_hz=162.0e6, channels_hz=(161.975e6, 162.025e6), taps=None, pulse=None, chunk_samples=1 << 22,
                  codes_format=None, table=None):
    """The ships of a marine VHF capture centred on center_hz -> dict(frames=..., tracks=..., nmea=..., fs=48000): 'frames' a list of dicts in
    order of 'pos' (ais_decode's keys and 'msg' (bytes without the check bytes), 'channel' ('A', 'B', ... by position in channels_hz), 'pos',
    'score'), 'tracks' ais_tracks(frames), 'nmea' the !AIVDM sentences of every frame in that order, 'fs' the rate the positions count in.
    On the GPU from the upload to the records: pss_ddc puts the listed channels at 0 Hz at ais_plan(fs)'s decimation (streamed in chunks of
    chunk_samples samples plus their halos; the result does not depend on chunk_samples), pss_resample brings them to 48 000 S/s where
    the decimated rate is another one, then pss_ais_front and pss_ais_frames on the resident rows.  taps: the down-converter's float64
    low-pass (default firwin(20 decim + 1, 25 000 / fs): half-width 12.5 kHz, one channel of the 25 kHz grid); pulse: the post-filter
    (default ais_default_pulse()); codes_format / table: as demodulate_recording."""
    import torch
    e = get_engine()
    fs = float(fs)
    decim, up, down = e.ais_plan(fs)
    offsets = np.atleast_1d(np.asarray(channels_hz, np.float64)) - float(center_hz)
    if offsets.ndim != 1 or not len(offsets) or len(offsets) > 26:
        raise ValueError("channels_hz: a list of 1 to 26 frequencies")
    if taps is None:
        taps = np.empty(20 * decim + 1, np.float64)
        if e.lib.pss_design_firwin(len(taps), 25000.0 / fs, taps.ctypes.data) != 0:
            raise ValueError("ais_recording: the down-converter's filter design failed")
    d_rows, _ = _tune_device(samples, fs, offsets, decim, taps, None, chunk_samples, codes_format, table)
    k, m = d_rows.shape[0], d_rows.shape[1] // 2
    if (up, down) != (1, 1):
        n = e.resample_out_len(m, up, down)
        d_bb = torch.empty((k, 2 * max(n, 1)), dtype=torch.float32, device=d_rows.device)
        if m:
            e.resample(d_rows, np.complex64, k, m, up, down, d_bb)
        d_rows, m = d_bb[:, :2 * n].contiguous() if n else d_bb[:, :0], n
    frames = []
    if m:
        d_y = torch.empty((k, m), dtype=torch.float32, device=d_rows.device)
        e.ais_front(d_rows, k, m, d_y, pulse=pulse)
        for msg, ln, row, pos, score in zip(*_ais_rows(e, d_y, k, m)):
            body = bytes(msg[:int(ln) - 2])
            d = ais_decode(body)
            d.update(msg=body, channel=chr(ord('A') + int(row)), pos=int(pos), score=float(score))
            frames.append(d)
    frames.sort(key=lambda f: (f['pos'], f['channel']))
    nmea = [sen for f in frames for sen in ais_nmea(f['msg'], f['channel'])]
    return dict(frames=frames, tracks=ais_tracks(frames), nmea=nmea, fs=_AIS_RATE)


_POCSAG_RATE = 38400
_POCSAG_IDLE = 0x7A89C197
_POCSAG_NUMERIC = "0123456789*U -)("
_POCSAG_KEYS = ('cw', 'fix', 'row', 'pos', 'meta', 'score')


def pocsag_records(cw, fix, row, pos, meta, score):
    """The arrays of pss_pocsag_batches / Engine.h_pocsag_batches -> one dict per batch: 'cw' (16 ints), 'fix' (16 ints), 'row', 'pos', 'meta',
    'score', and meta's fields 'sync_errors', 'inverted', 'n_bad', 'fixed'."""
    out = []
    for c, f, r, p, m, q in zip(cw, fix, row, pos, meta, score):
        m = int(m)
        out.append(dict(cw=[int(v) for v in c], fix=[int(v) for v in f], row=int(r), pos=int(p), meta=m, score=float(q), sync_errors=m & 0xFF,
                        inverted=bool((m >> 8) & 1), n_bad=(m >> 16) & 0xFF, fixed=m >> 24))
    return out


def _pocsag_text(bits):
    """A message's data bits in the order received -> (numeric, alpha): every group's first bit is its least significant."""
    numeric = "".join(_POCSAG_NUMERIC[sum(b << i for i, b in enumerate(bits[k:k + 4]))] for k in range(0, len(bits) - 3, 4))
    codes = [sum(b << i for i, b in enumerate(bits[k:k + 7])) for k in range(0, len(bits) - 6, 7)]
    while codes and codes[-1] in (0, 3, 4):   # NUL, ETX, EOT: the fill behind the text
        codes.pop()
    alpha = "".join(chr(c) if 32 <= c < 127 else "?" for c in codes)
    return numeric, alpha


def pocsag_messages(records, spb, stats=None):
    """records: batches of ONE rate (pocsag_records' dicts; any order) -> the messages, in order of (row, pos), each a dict: 'ric' (the 18
    address bits << 3 | the frame the address word stood in), 'function' (0 .. 3), 'numeric' and 'alpha' (both readings of the data bits),
    'bits' (how many data bits), 'pos' (the row index of the address word's first strobe), 'row', 'baud', 'fixed' (bits corrected in its
    codewords), 'damaged' (closed by an uncorrectable codeword).
    1. Among a row's records less than spb apart the one with the smallest (n_bad, fixed bits, -score, pos) stays.
    2. Batch B continues A iff same row, same polarity and 2 |pos_B - pos_A - 544 spb| <= spb.
    3. Along a chain a codeword with bit 31 = 0 that is not the idle word 0x7A89C197 opens a message, codewords with bit 31 = 1 append
       their 20 data bits, an address word, an idle word or the chain's end closes it, an uncorrectable word closes it with damaged=True;
       data words with no open message are counted: stats['orphans'] where a dict is handed in."""
    spb = int(spb)
    key = lambda r: (r['n_bad'], r['fixed'], -r['score'], r['pos'])
    recs = sorted(records, key=lambda r: (r['row'], r['pos']))
    kept = []
    for i, a in enumerate(recs):
        best = True
        for step in (-1, 1):
            j = i + step
            while best and 0 <= j < len(recs) and recs[j]['row'] == a['row'] and abs(recs[j]['pos'] - a['pos']) < spb:
                best = not key(recs[j]) < key(a)
                j += step
        if best:
            kept.append(a)
    follows, has_prev = {}, set()
    for i, a in enumerate(kept):
        for j in range(i + 1, len(kept)):
            b = kept[j]
            if b['row'] != a['row'] or 2 * (b['pos'] - a['pos'] - 544 * spb) > spb:
                break
            if j not in has_prev and b['inverted'] == a['inverted'] and 2 * abs(b['pos'] - a['pos'] - 544 * spb) <= spb:
                follows[i] = j
                has_prev.add(j)
                break
    baud = _POCSAG_RATE // spb if _POCSAG_RATE % spb == 0 else _POCSAG_RATE / spb
    messages, orphans = [], 0
    for head in range(len(kept)):
        if head in has_prev:
            continue
        cur, i = None, head

        def close(damaged=False):
            nonlocal cur
            if cur is not None:
                bits = cur.pop('_bits')
                numeric, alpha = _pocsag_text(bits)
                cur.update(numeric=numeric, alpha=alpha, bits=len(bits), damaged=damaged)
                messages.append(cur)
            cur = None

        while i is not None:
            rec = kept[i]
            for j, (cw, fx) in enumerate(zip(rec['cw'], rec['fix'])):
                if fx == 255:
                    close(damaged=True)
                elif cw == _POCSAG_IDLE:
                    close()
                elif not cw >> 31:
                    close()
                    cur = dict(ric=((cw >> 13) & 0x3FFFF) << 3 | j // 2, function=(cw >> 11) & 3, pos=rec['pos'] + (32 + 32 * j) * spb, row=rec['row'],
                               baud=baud, fixed=fx, _bits=[])
                elif cur is None:
                    orphans += 1
                else:
                    cur['_bits'].extend((cw >> k) & 1 for k in range(30, 10, -1))
                    cur['fixed'] += fx
            i = follows.get(i)
        close()
    if stats is not None:
        stats['orphans'] = stats.get('orphans', 0) + orphans
    messages.sort(key=lambda m: (m['row'], m['pos']))
    return messages


def pocsag_lines(messages):
    """multimon-ng's lines: `POCSAG1200: Address: 1234567  Function: 3  Alpha:   text`; the numeric reading for function 0, the alpha
    reading otherwise, neither for a message without data."""
    out = []
    for m in messages:
        line = f"POCSAG{m['baud']}: Address: {m['ric']:7d}  Function: {m['function']}"
        if m['bits']:
            line += "  Numeric: " + m['numeric'] if m['function'] == 0 else "  Alpha:   " + m['alpha']
        out.append(line)
    return out


def _pocsag_batches(e, d_y, n_rows, n, spb, sync_errors, fix, max_bad):
    """pss_pocsag_batches on resident rows -> the records on the host (pocsag_records)."""
    import torch
    dev = d_y.device
    room = 4096
    while True:
        d_cw = torch.empty((room, 16), dtype=torch.int32, device=dev)
        d_fix = torch.empty((room, 16), dtype=torch.uint8, device=dev)
        d_row = torch.empty(room, dtype=torch.int32, device=dev)
        d_pos = torch.empty(room, dtype=torch.int64, device=dev)
        d_meta = torch.empty(room, dtype=torch.int32, device=dev)
        d_score = torch.empty(room, dtype=torch.float32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        e.pocsag_batches(d_y, n_rows, n, spb, d_cw, d_fix, d_row, d_pos, d_meta, d_score, d_count, room, sync_errors=sync_errors, fix=fix, max_bad=max_bad)
        k = int(d_count.cpu()[0])
        if k <= room:
            break
        room = k   # the true count: again with room for it
    cw, fx, row, pos, meta, score = (t[:k].cpu().numpy() for t in (d_cw, d_fix, d_row, d_pos, d_meta, d_score))
    return pocsag_records(cw.view(np.uint32), fx, row, pos, meta.view(np.uint32), score)


def pocsag_rows(rows, bauds=(512, 1200, 2400), sync_errors=2, fix=2, max_bad=0):
    """rows: complex64 rows at 38 400 S/s — a host array [k][n] or [n], or a resident device tensor float32 [k][2 n] — -> (messages,
    batches): pss_ais_front with pocsag_default_pulse's boxcar and pss_pocsag_batches once per rate on the resident rows, then
    pocsag_messages.  messages in order of (pos, row); batches: pocsag_records' dicts with 'baud'.  Rows from channelize_plan / pss_bank
    come here after pss_resample (50 kS/s -> 96 / 125)."""
    import torch
    e = get_engine()
    if isinstance(rows, torch.Tensor):
        d_rows = rows
    else:
        x = np.asarray(rows, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("rows: a 1-D or 2-D complex array")
        x = np.ascontiguousarray(x[None, :] if x.ndim == 1 else x)
        d_rows = torch.from_numpy(x.view(np.float32)).to(f"cuda:{e.device}")
    if d_rows.dim() != 2 or d_rows.dtype != torch.float32 or d_rows.shape[1] % 2 or not d_rows.is_contiguous():
        raise ValueError("rows: a contiguous device tensor float32 [k][2 n]")
    k, n = d_rows.shape[0], d_rows.shape[1] // 2
    messages, batches = [], []
    if not k or not n:
        return messages, batches
    d_y = torch.empty((k, n), dtype=torch.float32, device=d_rows.device)
    for baud in bauds:
        spb = _POCSAG_RATE // int(baud)
        if spb * int(baud) != _POCSAG_RATE or not 2 <= spb <= 128:
            raise ValueError("bauds: rates that divide 38 400 into 2 to 128 samples a bit")
        e.ais_front(d_rows, k, n, d_y, pulse=e.pocsag_default_pulse(spb))
        recs = _pocsag_batches(e, d_y, k, n, spb, sync_errors, fix, max_bad)
        messages += pocsag_messages(recs, spb)
        for r in recs:
            r['baud'] = int(baud)
        batches += recs
    messages.sort(key=lambda m: (m['pos'], m['row'], m['baud']))
    batches.sort(key=lambda r: (r['pos'], r['row'], r['baud']))
    return messages, batches


def pocsag_recording(samples, fs, center_hz, channels_hz, bauds=(512, 1200, 2400), taps=None, chunk_samples=1 << 22, codes_format=None, table=None,
                     sync_errors=2, fix=2, max_bad=0):
    """The pager messages of a capture centred on center_hz -> dict(messages=..., lines=..., batches=..., fs=38400): 'messages'
    pocsag_messages' dicts in order of 'pos' ('row' is the channel's position in channels_hz), 'lines' pocsag_lines(messages), 'batches' the
    receiver's records, 'fs' the rate the positions count in.  On the GPU from the upload to the records: pss_ddc puts the listed
    channels at 0 Hz at pocsag_plan(fs)'s decimation (streamed in chunks of chunk_samples samples plus their halos; the result does not
    depend on chunk_samples), pss_resample brings them to 38 400 S/s where the decimated rate is another one, then pocsag_rows.  taps: the
    down-converter's float64 low-pass (default firwin(20 decim + 1, 12 500 / fs): half-width 6.25 kHz, one channel of the 12.5 kHz grid);
    codes_format / table: as demodulate_recording."""
    import torch
    e = get_engine()
    fs = float(fs)
    decim, up, down = e.pocsag_plan(fs)
    offsets = np.atleast_1d(np.asarray(channels_hz, np.float64)) - float(center_hz)
    if offsets.ndim != 1 or not len(offsets):
        raise ValueError("channels_hz: a list of frequencies")
    if taps is None:
        taps = np.empty(20 * decim + 1, np.float64)
        if e.lib.pss_design_firwin(len(taps), 12500.0 / fs, taps.ctypes.data) != 0:
            raise ValueError("pocsag_recording: the down-converter's filter design failed")
    d_rows, _ = _tune_device(samples, fs, offsets, decim, taps, None, chunk_samples, codes_format, table)
    k, m = d_rows.shape[0], d_rows.shape[1] // 2
    if (up, down) != (1, 1):
        n = e.resample_out_len(m, up, down)
        d_bb = torch.empty((k, 2 * max(n, 1)), dtype=torch.float32, device=d_rows.device)
        if m:
            e.resample(d_rows, np.complex64, k, m, up, down, d_bb)
        d_rows, m = d_bb[:, :2 * n].contiguous() if n else d_bb[:, :0], n
    messages, batches = pocsag_rows(d_rows.contiguous(), bauds, sync_errors, fix, max_bad) if m else ([], [])
    return dict(messages=messages, lines=pocsag_lines(messages), batches=batches, fs=_POCSAG_RATE)


# ---- FLEX: the pager messages of a capture, two- and four-level FSK (the arithmetic of the device stages: csrc/pss_flex.h).  The constants
#      of the message layer are the published ones as multimon-ng reads them, written from memory: not checked against a transmitter.
_FLEX_MODES = ((1600, 2), (1600, 4), (3200, 2), (3200, 4), (3200, 4))
_FLEX_NUMERIC = "0123456789 U -]["
_FLEX_PHASES = "ABCD"
_FLEX_H = 12          # samples a 3200-baud symbol at 38 400 S/s


def flex_records(words, fix, fiw, row, pos, meta, score):
    """The arrays of pss_flex_frames / Engine.h_flex_frames -> one dict per frame: 'words' and 'fix' (4 lists of 88 ints), 'fiw', 'row', 'pos',
    'meta' (2 ints), 'score', and the fields of meta and fiw: 'sync_errors', 'inverted', 'mode', 'baud', 'levels', 'fiw_fixed', 'n_bad',
    'fixed', 'cycle', 'frame'."""
    out = []
    for w, f, i, r, p, m, q in zip(words, fix, fiw, row, pos, meta, score):
        m0, m1, i = int(m[0]), int(m[1]), int(i)
        mode = (m0 >> 12) & 15
        out.append(dict(words=[[int(v) for v in ph] for ph in w], fix=[[int(v) for v in ph] for ph in f], fiw=i, row=int(r), pos=int(p), meta=[m0, m1],
                        score=float(q), sync_errors=m0 & 0xFF, inverted=bool((m0 >> 8) & 1), mode=mode, baud=_FLEX_MODES[mode][0],
                        levels=_FLEX_MODES[mode][1], fiw_fixed=(m0 >> 16) & 0xFF, n_bad=m1 & 0xFFFF, fixed=m1 >> 16, cycle=(i >> 4) & 15,
                        frame=(i >> 8) & 127))
    return out


def _flex_phases(rec):
    return [p for p in range(4) if p == 0 or (p == 1 and rec['levels'] == 4) or (p == 2 and rec['baud'] == 3200) or
            (p == 3 and rec['baud'] == 3200 and rec['levels'] == 4)]


def flex_messages(records):
    """records: flex_records' dicts -> the messages in order of (row, pos, phase, address word), each a dict: 'capcode' (short addresses: the
    address word's data - 0x8000; None for a long one), 'long', 'address' (the raw data of its one or two words), 'type' ('ALN' for vector
    type 5, 'NUM' for 3, the number otherwise), 'text' (ALN and NUM), 'fragment' and 'cont' (ALN), 'words' (the raw data of its vector
    word(s) for the other types), 'phase' ('A' .. 'D'), 'row', 'pos', 'cycle', 'frame', 'baud', 'levels', 'damaged' (it touches an
    uncorrectable word).  Per phase, d = the low 21 bits of each word:
    word 0 is the block information word: its nibble sum must be 15 (else the phase is skipped); first address word = (d >> 8 & 3) + 1, first
    vector word = d >> 10 & 63.  An address is short when 0x8001 <= d <= 0x1E0000; any other takes two words, and so does its vector.
    Address word i's vector sits at the same offset into the vector field; type = d >> 4 & 7.  Type 5: start = d >> 7 & 127, length = d >> 14
    & 127 words: the first holds fragment (d >> 11 & 3) and continue (d >> 10 & 1), the others three 7-bit characters each from bit 0; the
    first character is a signature when fragment = 3; ETX (3) is dropped.  Type 3: start = d >> 7 & 127, (d >> 14 & 7) + 1 words read as a bit
    stream from bit 0: 10 bits skipped, then 4-bit digits, least significant bit first, through "0123456789 U -]["; trailing spaces dropped."""
    out = []
    for rec in sorted(records, key=lambda r: (r['row'], r['pos'])):
        for p in _flex_phases(rec):
            d = [w & 0x1FFFFF for w in rec['words'][p]]
            bad = [f == 255 for f in rec['fix'][p]]
            biw = d[0]
            s = ((biw & 15) + (biw >> 4 & 15) + (biw >> 8 & 15) + (biw >> 12 & 15) + (biw >> 16 & 15) + (biw >> 20 & 1)) & 15
            if bad[0] or s != 15:
                continue
            first_addr, first_vec = (biw >> 8 & 3) + 1, biw >> 10 & 63
            i = first_addr
            while i < first_vec:
                short = 0x8001 <= d[i] <= 0x1E0000
                n_a = 1 if short else 2
                v = first_vec + (i - first_addr)
                if i + n_a > first_vec or v + n_a > 88:
                    break
                touched = list(range(i, i + n_a)) + list(range(v, v + n_a))
                vec = d[v]
                kind = vec >> 4 & 7
                m = dict(capcode=d[i] - 0x8000 if short else None, long=not short, address=d[i:i + n_a], type=kind, phase=_FLEX_PHASES[p], row=rec['row'],
                         pos=rec['pos'], cycle=rec['cycle'], frame=rec['frame'], baud=rec['baud'], levels=rec['levels'])
                if kind == 5 and not bad[v]:
                    start, length = vec >> 7 & 127, vec >> 14 & 127
                    body = list(range(start, min(start + length, 88)))
                    touched += body
                    codes = []
                    if body:
                        m['fragment'], m['cont'] = d[body[0]] >> 11 & 3, d[body[0]] >> 10 & 1
                        for k in body[1:]:
                            codes += [d[k] & 127, d[k] >> 7 & 127, d[k] >> 14 & 127]
                        if m['fragment'] == 3:
                            codes = codes[1:]
                    m['type'] = 'ALN'
                    m['text'] = "".join(chr(c) if 32 <= c < 127 else "?" for c in codes if c != 3)
                elif kind == 3 and not bad[v]:
                    start, n_w = vec >> 7 & 127, (vec >> 14 & 7) + 1
                    body = list(range(start, min(start + n_w, 88)))
                    touched += body
                    bits = [(d[k] >> b) & 1 for k in body for b in range(21)][10:]
                    m['type'] = 'NUM'
                    m['text'] = "".join(_FLEX_NUMERIC[sum(b << u for u, b in enumerate(bits[k:k + 4]))] for k in range(0, len(bits) - 3, 4)).rstrip(" ")
                else:
                    m['words'] = d[v:v + n_a]
                m['damaged'] = any(bad[k] for k in touched)
                out.append(m)
                i += n_a
    return out


def flex_lines(messages):
    """multimon-ng's lines without the clock a capture does not have: `FLEX: 1600/2/A 03.077 [001234567] ALN text`; the vector type's number
    and the raw words for the other types, `[long aaaaaa bbbbbb]` for a long address."""
    out = []
    for m in messages:
        who = f"[{m['capcode']:09d}]" if not m['long'] else "[long " + " ".join(f"{a:06X}" for a in m['address']) + "]"
        head = f"FLEX: {m['baud']}/{m['levels']}/{m['phase']} {m['cycle']:02d}.{m['frame']:03d} {who} "
        out.append(head + (f"{m['type']} {m['text']}" if 'text' in m else f"T{m['type']} " + " ".join(f"{w:06X}" for w in m['words'])))
    return out


def _flex_frames(e, d_y, n_rows, n, h, sync_errors, fix, max_bad):
    """pss_flex_frames on resident rows -> the records on the host (flex_records)."""
    import torch
    dev = d_y.device
    room = 256
    while True:
        d_words = torch.empty((room, 4, 88), dtype=torch.int32, device=dev)
        d_fix = torch.empty((room, 4, 88), dtype=torch.uint8, device=dev)
        d_fiw = torch.empty(room, dtype=torch.int32, device=dev)
        d_row = torch.empty(room, dtype=torch.int32, device=dev)
        d_pos = torch.empty(room, dtype=torch.int64, device=dev)
        d_meta = torch.empty((room, 2), dtype=torch.int32, device=dev)
        d_score = torch.empty(room, dtype=torch.float32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        e.flex_frames(d_y, n_rows, n, h, d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score, d_count, room, sync_errors=sync_errors, fix=fix,
                      max_bad=max_bad)
        k = int(d_count.cpu()[0])
        if k <= room:
            break
        room = k   # the true count: again with room for it
    words, fx, fiw, row, pos, meta, score = (t[:k].cpu().numpy() for t in (d_words, d_fix, d_fiw, d_row, d_pos, d_meta, d_score))
    return flex_records(words.view(np.uint32), fx, fiw.view(np.uint32), row, pos, meta.view(np.uint32), score)


def h_flex_rows(rows, h=_FLEX_H, sync_errors=2, fix=2, max_bad=0):
    """flex_rows on the host: pss_h_ais_front and pss_h_flex_frames on complex64 rows [k][n] or [n] -> (messages, frames).  No GPU."""
    x = np.asarray(rows, np.complex64)
    if x.ndim not in (1, 2):
        raise ValueError("rows: a 1-D or 2-D complex array")
    x = np.ascontiguousarray(x[None, :] if x.ndim == 1 else x)
    if not x.shape[0] or not x.shape[1]:
        return [], []
    from .engine import Engine
    y = Engine.h_ais_front(x, pulse=Engine.flex_default_pulse(h))
    recs = flex_records(*Engine.h_flex_frames(y, h, sync_errors=sync_errors, fix=fix, max_bad=max_bad)[:7])
    return flex_messages(recs), recs


def flex_rows(rows, h=_FLEX_H, sync_errors=2, fix=2, max_bad=0):
    """rows: complex64 rows at 38 400 S/s (h = 12 samples a 3200-baud symbol) — a host array [k][n] or [n], or a resident device tensor
    float32 [k][2 n] — -> (messages, frames): pss_ais_front with flex_default_pulse's boxcar once (both baud rates read the same rows), then
    pss_flex_frames on the resident rows, then flex_messages.  frames: flex_records' dicts."""
    import torch
    e = get_engine()
    if isinstance(rows, torch.Tensor):
        d_rows = rows
    else:
        x = np.asarray(rows, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("rows: a 1-D or 2-D complex array")
        x = np.ascontiguousarray(x[None, :] if x.ndim == 1 else x)
        d_rows = torch.from_numpy(x.view(np.float32)).to(f"cuda:{e.device}")
    if d_rows.dim() != 2 or d_rows.dtype != torch.float32 or d_rows.shape[1] % 2 or not d_rows.is_contiguous():
        raise ValueError("rows: a contiguous device tensor float32 [k][2 n]")
    k, n = d_rows.shape[0], d_rows.shape[1] // 2
    if not k or not n:
        return [], []
    d_y = torch.empty((k, n), dtype=torch.float32, device=d_rows.device)
    e.ais_front(d_rows, k, n, d_y, pulse=e.flex_default_pulse(h))
    recs = _flex_frames(e, d_y, k, n, h, sync_errors, fix, max_bad)
    return flex_messages(recs), recs


def flex_recording(samples, fs, center_hz, channels_hz, taps=None, chunk_samples=1 << 22, codes_format=None, table=None, sync_errors=2, fix=2,
                   max_bad=0):
    """The FLEX pager messages of a capture centred on center_hz -> dict(messages=..., lines=..., frames=..., fs=38400): 'messages'
    flex_messages' dicts ('row' is the channel's position in channels_hz), 'lines' flex_lines(messages), 'frames' the receiver's records, 'fs'
    the rate the positions count in.  On the GPU from the upload to the records: pss_ddc puts the listed channels at 0 Hz at pocsag_plan(fs)'s
    decimation (streamed in chunks of chunk_samples samples plus their halos; the result does not depend on chunk_samples), pss_resample
    brings them to 38 400 S/s where the decimated rate is another one, then flex_rows.  taps: the down-converter's float64 low-pass (default
    firwin(20 decim + 1, 20 000 / fs): half-width 10 kHz, so the outer levels at +-4800 Hz and the 3200-baud sidebands around them pass);
    codes_format / table: as demodulate_recording."""
    import torch
    e = get_engine()
    fs = float(fs)
    decim, up, down = e.pocsag_plan(fs)
    offsets = np.atleast_1d(np.asarray(channels_hz, np.float64)) - float(center_hz)
    if offsets.ndim != 1 or not len(offsets):
        raise ValueError("channels_hz: a list of frequencies")
    if taps is None:
        taps = np.empty(20 * decim + 1, np.float64)
        if e.lib.pss_design_firwin(len(taps), 20000.0 / fs, taps.ctypes.data) != 0:
            raise ValueError("flex_recording: the down-converter's filter design failed")
    d_rows, _ = _tune_device(samples, fs, offsets, decim, taps, None, chunk_samples, codes_format, table)
    k, m = d_rows.shape[0], d_rows.shape[1] // 2
    if (up, down) != (1, 1):
        n = e.resample_out_len(m, up, down)
        d_bb = torch.empty((k, 2 * max(n, 1)), dtype=torch.float32, device=d_rows.device)
        if m:
            e.resample(d_rows, np.complex64, k, m, up, down, d_bb)
        d_rows, m = d_bb[:, :2 * n].contiguous() if n else d_bb[:, :0], n
    messages, frames = flex_rows(d_rows.contiguous(), _FLEX_H, sync_errors, fix, max_bad) if m else ([], [])
    return dict(messages=messages, lines=flex_lines(messages), frames=frames, fs=_POCSAG_RATE)


# ---- OOK devices: the sensor and remote messages of a 433 MHz capture (the arithmetic of the device stages: csrc/pss_ook.h)
_OOK_MODES = {'OOK_PWM': 0, 'OOK_PPM': 1, 'OOK_MC_ZEROBIT': 2}
_OOK_FLAGS = ((1 << 22, 'OPEN'), (1 << 23, 'LONG'), (1 << 24, 'MANY'), (1 << 25, 'FULL'))
_OOK_BLOCK = 4096
_OOK_US = {'s': 'short', 'l': 'long', 'y': 'sync', 'g': 'gap_limit', 't': 'tol', 'r': 'reset'}
# the project's own statement of two common device families, as the flex strings `rtl_433 -X` takes
OOK_DEVICES = {
    'nexus': "n=nexus,m=OOK_PPM,s=1000,l=2000,g=3000,r=5000,bits>=36",
    'ev1527': "n=ev1527,m=OOK_PWM,s=352,l=1056,g=2400,t=160,r=12000,bits>=24",
}


def ook_spec(text, fs):
    """rtl_433's flex string -> the C arguments in samples at fs, as a dict: 'name', 'mode', 'short', 'long', 'sync', 'gap_limit', 'tol',
    'reset', 'span', 'phase', 'invert', 'min_bits', 'max_odd'.  Keys: n= name; m= OOK_PWM | OOK_PPM | OOK_MC_ZEROBIT; s= short, l= long,
    y= sync, g= gap limit, t= tolerance (default a quarter of s), r= reset (default four gap limits), all in microseconds and converted as
    int(round(us fs / 1e6)); bits>= the fewest bits of a message; invert.  An unknown key is refused by name.  span (the samples a message
    may cover) is 512 of the longer symbol and a gap limit; OOK_MC_ZEROBIT reads the first pulse as the second half of a leading 0, so
    phase = 1."""
    fs = float(fs)
    us = {}
    spec = dict(name='', mode=None, sync=0, phase=0, invert=0, min_bits=0, max_odd=0)
    for item in str(text).split(','):
        item = item.strip()
        if not item:
            continue
        if item == 'invert':
            spec['invert'] = 1
            continue
        if item.startswith('bits>='):
            spec['min_bits'] = int(item[6:])
            continue
        key, eq, value = item.partition('=')
        key = key.strip()
        if not eq or key not in ('n', 'm') + tuple(_OOK_US):
            raise ValueError(f"ook_spec: unknown key {key!r}")
        if key == 'n':
            spec['name'] = value.strip()
        elif key == 'm':
            if value.strip() not in _OOK_MODES:
                raise ValueError(f"ook_spec: unknown modulation {value.strip()!r}")
            spec['mode'] = _OOK_MODES[value.strip()]
        else:
            us[_OOK_US[key]] = float(value)
    if spec['mode'] is None or 'short' not in us:
        raise ValueError("ook_spec: m= and s= are needed")
    if spec['mode'] != 2 and 'long' not in us:
        raise ValueError("ook_spec: l= is needed")
    us.setdefault('long', 2.0 * us['short'] if spec['mode'] == 2 else 0.0)
    us.setdefault('gap_limit', 2.0 * max(us['short'], us['long']))
    us.setdefault('tol', us['short'] / 4.0)
    us.setdefault('reset', 4.0 * us['gap_limit'])
    for key, value in us.items():
        spec[key] = int(round(value * fs / 1e6))
    spec['span'] = min(1 << 24, max(1, 512 * max(spec['long'], 2 * spec['short']) + spec['gap_limit']))
    if spec['mode'] == 2:
        spec['phase'] = 1
    return spec


def ook_levels(block_means, hi_ratio=8.0, lo_ratio=4.0, quantile=0.25):
    """The block means of ONE row (pss_ook_levels) -> (hi, lo) float32: floor = the element at index int(len quantile) of the sorted means
    (len // 4: the lower quartile, which keyed traffic under a quarter of the time does not move), hi = fl32(hi_ratio floor),
    lo = fl32(lo_ratio floor)."""
    m = np.sort(np.asarray(block_means, np.float64).ravel())
    if not len(m):
        raise ValueError("ook_levels: no whole block of 4096 samples")
    floor = m[min(len(m) - 1, int(len(m) * float(quantile)))]
    return np.float32(float(hi_ratio) * floor), np.float32(float(lo_ratio) * floor)


def ook_records(bits, n_bits, row, pos, span, meta):
    """The arrays of pss_ook_messages / Engine.h_ook_messages -> one dict per record: 'bits' (a list of 0 / 1), 'n_bits', 'row', 'pos', 'span',
    'n_pulses', 'n_odd', 'flags' (names of OPEN / LONG / MANY / FULL), 'hex'."""
    out = []
    for b, n, r, p, s, w in zip(bits, n_bits, row, pos, span, meta):
        n, w = int(n), int(w)
        out.append(dict(bits=np.unpackbits(np.asarray(b, np.uint8))[:n].tolist(), n_bits=n, row=int(r), pos=int(p), span=int(s), n_pulses=w & 0x7FF,
                        n_odd=(w >> 11) & 0x7FF, flags=[name for mask, name in _OOK_FLAGS if w & mask], hex=bytes(b[:(n + 7) // 8]).hex()))
    return out


def ook_messages(records, fs, reset_us):
    """records of ONE spec (ook_records' dicts) -> the messages in order of (row, pos): a record with the row and the bits of the message before
    it whose start lies within reset_us of that copy's end is a repeat of it.  Each: 'row', 'pos', 'time' (s), 'bits', 'n_bits', 'hex',
    'count', 'span' (first rise of the first copy to last fall of the last)."""
    reset = int(round(float(reset_us) * float(fs) / 1e6))
    out = []
    for r in sorted(records, key=lambda r: (r['row'], r['pos'])):
        m = out[-1] if out else None
        if m and m['row'] == r['row'] and m['bits'] == r['bits'] and r['pos'] - (m['pos'] + m['span']) <= reset:
            m['count'] += 1
            m['span'] = r['pos'] + r['span'] - m['pos']
        else:
            out.append(dict(row=r['row'], pos=r['pos'], time=r['pos'] / float(fs), bits=list(r['bits']), n_bits=r['n_bits'], hex=r['hex'], count=1,
                            span=r['span']))
    return out


def _ook_field(bits, a, b):
    return int("".join(map(str, bits[a:b])), 2)


def ook_decode(name, bits):
    """The fields of a message of one of OOK_DEVICES' layouts -> dict with 'model': nexus (36 bits: id 8 | battery 1 | 0 | channel 2 |
    temperature 12, two's complement, tenths of a degree C | 1111 | humidity 8) and ev1527 (24 bits: id 20 | buttons 4).  Anything else,
    and a message that does not fit its layout, is reported as hex."""
    bits = [int(b) & 1 for b in bits]
    if name == 'nexus' and len(bits) == 36 and bits[9] == 0 and bits[24:28] == [1, 1, 1, 1]:
        t = _ook_field(bits, 12, 24)
        return dict(model='nexus', id=_ook_field(bits, 0, 8), battery_ok=bits[8], channel=_ook_field(bits, 10, 12) + 1,
                    temperature_c=(t - 4096 if t & 0x800 else t) / 10.0, humidity=_ook_field(bits, 28, 36))
    if name == 'ev1527' and len(bits) == 24:
        return dict(model='ev1527', id=_ook_field(bits, 0, 20), buttons=_ook_field(bits, 20, 24))
    pad = bits + [0] * (-len(bits) % 8)
    return dict(model=name, n_bits=len(bits), hex=bytes(_ook_field(pad, k, k + 8) for k in range(0, len(pad), 8)).hex())


def ook_lines(messages):
    """One text line a message (ook_rows' dicts with 'name' and 'fields')."""
    out = []
    for m in messages:
        f = m['fields']
        if f['model'] == 'nexus' and 'id' in f:
            text = (f"id {f['id']} channel {f['channel']} battery {'ok' if f['battery_ok'] else 'low'} temperature {f['temperature_c']:.1f} C "
                    f"humidity {f['humidity']} %")
        elif f['model'] == 'ev1527' and 'id' in f:
            text = f"id {f['id']:05x} buttons {f['buttons']:04b}"
        else:
            text = f"{f['n_bits']} bits {f['hex']}"
        out.append(f"{m['time']:10.4f} s  row {m['row']}  {m['name']}: {text}  x{m['count']}")
    return out


def _ook_specs(specs, fs):
    items = specs.items() if isinstance(specs, dict) else [(None, s) for s in specs]
    out = []
    for name, s in items:
        s = dict(s) if isinstance(s, dict) else ook_spec(s, fs)
        if name is not None and not s.get('name'):
            s['name'] = name
        out.append(s)
    return out


def _ook_result(specs, per_spec, fs, levels):
    """per_spec[i]: spec i's records of every row -> the recording entries' dict."""
    records, messages = [], []
    for s, recs in zip(specs, per_spec):
        for m in ook_messages(recs, fs, s['reset'] * 1e6 / float(fs)):
            m.update(name=s['name'], fields=ook_decode(s['name'], m['bits']))
            messages.append(m)
        records += [dict(r, name=s['name']) for r in recs]
    messages.sort(key=lambda m: (m['pos'], m['row'], m['name']))
    return dict(messages=messages, lines=ook_lines(messages), records=records, levels=levels, fs=float(fs))


def _ook_host_rows(rows):
    x = np.asarray(rows, np.complex64)
    if x.ndim not in (1, 2):
        raise ValueError("rows: a 1-D or 2-D complex array")
    return np.ascontiguousarray(x[None, :] if x.ndim == 1 else x)


def h_ook_rows(rows, fs, specs=OOK_DEVICES, P=9, R=64, hi_ratio=8.0, lo_ratio=4.0, quantile=0.25):
    """ook_rows on the host twins (pss_h_ook_levels, pss_h_ook_messages): no GPU."""
    from .engine import Engine
    x = _ook_host_rows(rows)
    specs = _ook_specs(specs, fs)
    per_spec, levels = [[] for _ in specs], []
    for k in range(len(x)):
        if x.shape[1] < _OOK_BLOCK:
            levels.append(None)
            continue
        hi, lo = ook_levels(Engine.h_ook_levels(x[k])[0], hi_ratio, lo_ratio, quantile)
        levels.append((float(hi), float(lo)))
        for i, s in enumerate(specs):
            recs = ook_records(*Engine.h_ook_messages(x[k], hi, lo, s, P=P, R=R)[:6])
            per_spec[i] += [dict(r, row=k) for r in recs]
    return _ook_result(specs, per_spec, fs, levels)


def _ook_call(e, ptr, n_buf, hi, lo, spec, P, R, out, **window):
    """pss_ook_messages on one resident row -> (records on the host, out): out holds the device arrays and grows to the true count."""
    import torch
    dev = f"cuda:{e.device}"
    while True:
        if out.get('room', 0) == 0 or out.get('grow'):
            room = out['room'] = max(out.get('grow', 0), 4096)
            out.pop('grow', None)
            out['t'] = (torch.empty((room, 32), dtype=torch.uint8, device=dev), torch.empty(room, dtype=torch.int32, device=dev),
                        torch.empty(room, dtype=torch.int32, device=dev), torch.empty(room, dtype=torch.int64, device=dev),
                        torch.empty(room, dtype=torch.int32, device=dev), torch.empty(room, dtype=torch.int32, device=dev),
                        torch.zeros(1, dtype=torch.int32, device=dev))
        t = out['t']
        e.ook_messages(ptr, 1, n_buf, hi, lo, spec, *t, out['room'], P=P, R=R, **window)
        k = int(t[6].cpu()[0])
        if k <= out['room']:
            break
        out['grow'] = k   # the true count: again with room for it
    bits, nb, row, pos, span, meta = (a[:k].cpu().numpy() for a in t[:6])
    return ook_records(bits, nb, row, pos, span, meta.view(np.uint32))


def ook_rows(rows, fs, specs=OOK_DEVICES, P=9, R=64, hi_ratio=8.0, lo_ratio=4.0, quantile=0.25):
    """rows: complex64 rows at fs — a host array [k][n] or [n], or a resident device tensor float32 [k][2 n] (pss_ddc's, pss_pfb's, pss_bank's
    output) — -> dict(messages, lines, records, levels, fs): per row the block means once (pss_ook_levels) and from them its thresholds
    (ook_levels), then pss_ook_messages once per spec on the resident row.  specs: OOK_DEVICES' kind, a dict or a list of flex strings or of
    ook_spec's dicts.  'records': ook_records' dicts with 'name', per spec in order of (row, pos); 'messages': the repeats joined
    (ook_messages), with 'name' and 'fields' (ook_decode), in order of (pos, row, name); 'lines': ook_lines; 'levels': (hi, lo) per row,
    None for a row shorter than one block, which reports nothing."""
    import torch
    e = get_engine()
    if isinstance(rows, torch.Tensor):
        d_rows = rows
    else:
        d_rows = torch.from_numpy(_ook_host_rows(rows).view(np.float32)).to(f"cuda:{e.device}")
    if d_rows.dim() != 2 or d_rows.dtype != torch.float32 or d_rows.shape[1] % 2 or not d_rows.is_contiguous():
        raise ValueError("rows: a contiguous device tensor float32 [k][2 n]")
    k, n = d_rows.shape[0], d_rows.shape[1] // 2
    specs = _ook_specs(specs, fs)
    per_spec, levels, out = [[] for _ in specs], [], {}
    nb = n // _OOK_BLOCK
    if nb and k:
        d_means = torch.empty((k, nb), dtype=torch.float64, device=d_rows.device)
        e.ook_levels(d_rows, k, n, d_means)
        means = d_means.cpu().numpy()
    for r in range(k):
        if not nb:
            levels.append(None)
            continue
        hi, lo = ook_levels(means[r], hi_ratio, lo_ratio, quantile)
        levels.append((float(hi), float(lo)))
        for i, s in enumerate(specs):
            recs = _ook_call(e, d_rows.data_ptr() + 8 * n * r, n, hi, lo, s, P, R, out)
            per_spec[i] += [dict(rec, row=r) for rec in recs]
    return _ook_result(specs, per_spec, fs, levels)


def ook_recording(samples, fs, specs=OOK_DEVICES, center_hz=None, channels_hz=None, decim=1, taps=None, chunk_samples=1 << 22, codes_format=None,
                  table=None, P=9, R=64, hi_ratio=8.0, lo_ratio=4.0, quantile=0.25):
    """The OOK devices of a capture -> ook_rows' dict; 'fs' is the rate the positions count in.  Without channels_hz the capture is the row: it
    is streamed twice in chunks of chunk_samples samples, once through pss_ook_levels (whole blocks) and once, each chunk with the halo
    pss_ook_halo states for the widest spec, through pss_ook_messages per spec.  With channels_hz (and center_hz) pss_ddc first puts the
    listed channels at 0 Hz at fs / decim (taps: its float64 low-pass, default firwin(20 decim + 1, 1 / decim)), streamed by the shared
    chunk loop, and ook_rows reads the resident rows ('row' is the channel's position in channels_hz).  The result does not depend on
    chunk_samples.  Every chunk goes up with `span` samples of halo behind it (about a second for OOK_DEVICES' timings), so chunks well
    above the widest span are the intended use: a chunk of one tile re-reads its halo 64-fold.  codes_format / table: as
    demodulate_recording; codes are widened per chunk on the device."""
    import torch
    e = get_engine()
    fs = float(fs)
    if channels_hz is not None:
        if center_hz is None:
            raise ValueError("ook_recording: channels_hz needs center_hz")
        offsets = np.atleast_1d(np.asarray(channels_hz, np.float64)) - float(center_hz)
        if offsets.ndim != 1 or not len(offsets):
            raise ValueError("channels_hz: a list of frequencies")
        d_rows, _ = _tune_device(samples, fs, offsets, int(decim), taps, None, chunk_samples, codes_format, table)
        return ook_rows(d_rows.contiguous(), fs / int(decim), specs, P, R, hi_ratio, lo_ratio, quantile)
    if int(chunk_samples) != chunk_samples or chunk_samples < 1:
        raise ValueError("chunk_samples must be an integer >= 1")
    dev = f"cuda:{e.device}"
    if codes_format is not None:
        iq = _iq_args(codes_format, table)
        samples = _iq_codes(samples, iq[0])
        if samples.ndim != 2:
            raise ValueError("codes: [n, 2]")
    else:
        samples = np.ascontiguousarray(samples, np.complex64)
        if samples.ndim != 1:
            raise ValueError("samples: a 1-D recording")

    def upload(lo, hi):
        if codes_format is None:
            return torch.from_numpy(samples[lo:hi].view(np.float32)).to(dev)
        d_iq = torch.empty(2 * (hi - lo), dtype=torch.float32, device=dev)
        e.unpack_iq(torch.from_numpy(np.array(samples[lo:hi])).to(dev), hi - lo, d_iq, codes_format, iq[2])
        return d_iq

    n = len(samples)
    specs = _ook_specs(specs, fs)
    per_spec = [[] for _ in specs]
    nb = n // _OOK_BLOCK
    if not nb:
        return _ook_result(specs, per_spec, fs, [None])
    step = max(1, int(chunk_samples) // _OOK_BLOCK)
    means = np.empty(nb, np.float64)
    for b0 in range(0, nb, step):
        b1 = min(nb, b0 + step)
        d_means = torch.empty((1, b1 - b0), dtype=torch.float64, device=dev)
        e.ook_levels(upload(b0 * _OOK_BLOCK, b1 * _OOK_BLOCK), 1, (b1 - b0) * _OOK_BLOCK, d_means, buf_index0=b0 * _OOK_BLOCK, n_row=n, b_begin=b0, b_end=b1)
        means[b0:b1] = d_means.cpu().numpy()[0]
    hi, lo = ook_levels(means, hi_ratio, lo_ratio, quantile)
    halos = [e.ook_halo(P, R, s['gap_limit'], s['span']) for s in specs]
    before, after = max(h[0] for h in halos), max(h[1] for h in halos)
    out = {}
    chunk = int(chunk_samples)
    for s0 in range(0, n, chunk):
        s1 = min(n, s0 + chunk)
        b_lo, b_hi = max(0, s0 - before), min(n, s1 + after)
        d_iq = upload(b_lo, b_hi)
        for i, s in enumerate(specs):
            per_spec[i] += _ook_call(e, d_iq, b_hi - b_lo, hi, lo, s, P, R, out, buf_index0=b_lo, n_row=n, s_begin=s0, s_end=s1)
    return _ook_result(specs, per_spec, fs, [(float(hi), float(lo))])


# ---- NOAA APT: the image of a 137 MHz capture (the arithmetic of the three device stages: csrc/pss_apt.h)
_APT_RATE = 62400
_APT_ENV_RATE = 12480
_APT_LINE_WORDS, _APT_LINE_ENV = 2080, 6240
_APT_IMAGE_A, _APT_TELEMETRY_A, _APT_HALF = 86, 995, 1040        # the first word of image A and of telemetry A; channel B: + 1040
_APT_IMAGE_WORDS, _APT_TELEMETRY_WORDS = 909, 45
_APT_WEDGES = (31.0, 63.0, 95.0, 127.0, 159.0, 191.0, 224.0, 255.0, 0.0)   # wedges 1 .. 9 of 255
_APT_CHANNEL_IDS = ('1', '2', '3A', '4', '5', '3B')                          # wedge 16 equals wedge 1 .. 6
_APT_TUNE_BLOCK = 1024                                                       # row samples of a block mean of the discriminator


def apt_grid(pos, meta, score, n_env):
    """The lines' positions from one row's sync records (apt_syncs': pos ascending) -> (line_pos int64 [n], found bool [n]).  The longest
    chain of records in which each spacing lies within +-3 of a multiple (>= 1) of 6240 is taken; position is fitted against line number by
    least squares in float64; every line number, negative ones included, whose 6240 samples at floor(fit + 0.5) lie in [0, n_env) is
    returned in ascending order, with found = a record of the chain carries that number.  Ties: of chains of one length the one with the
    fewest mismatches in total wins, then the highest total score, then the one whose last record is the earliest; a record's predecessor
    is chosen by the same order, then the earliest.  No record: no line.  One record: spacing 6240."""
    pos = np.asarray(pos, np.int64).ravel()
    meta = np.asarray(meta, np.int64).ravel()
    score = np.asarray(score, np.float64).ravel()
    n = len(pos)
    if not n:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    if np.any(np.diff(pos) <= 0):
        raise ValueError("apt_grid: pos must ascend")
    # (blen, bmis, bsc)[i] = (length, -mismatches, score) of the best chain that ends at record i; prev[i] its predecessor
    blen, bmis, bsc = np.ones(n, np.int64), -meta.copy(), score.copy()
    prev = np.full(n, -1, np.int64)
    for i in range(1, n):
        d = pos[i] - pos[:i]
        k = (d + _APT_LINE_ENV // 2) // _APT_LINE_ENV
        idx = np.flatnonzero((k >= 1) & (np.abs(d - k * _APT_LINE_ENV) <= 3))
        if len(idx):
            j = idx[np.lexsort((-idx, bsc[idx], bmis[idx], blen[idx]))[-1]]   # the best predecessor, the earliest on a tie
            blen[i], bmis[i], bsc[i], prev[i] = blen[j] + 1, bmis[j] - meta[i], bsc[j] + score[i], j
    end = int(np.lexsort((-np.arange(n), bsc, bmis, blen))[-1])
    chain = []
    while end >= 0:
        chain.append(end)
        end = int(prev[end])
    chain = chain[::-1]
    p = pos[chain].astype(np.float64)
    num = np.zeros(len(chain), np.int64)
    for q in range(1, len(chain)):
        num[q] = num[q - 1] + (int(pos[chain[q]] - pos[chain[q - 1]]) + _APT_LINE_ENV // 2) // _APT_LINE_ENV
    if len(chain) == 1:
        a, b = float(p[0]), float(_APT_LINE_ENV)
    else:
        x = num.astype(np.float64)
        xm, pm = x.mean(), p.mean()
        b = float(((x - xm) * (p - pm)).sum() / ((x - xm) ** 2).sum())
        a = float(pm - b * xm)
    k_lo, k_hi = int(np.floor(-a / b)) - 2, int(np.ceil((n_env - a) / b)) + 2
    ks = np.arange(k_lo, k_hi + 1, dtype=np.int64)
    lp = np.floor(a + b * ks.astype(np.float64) + 0.5).astype(np.int64)
    ok = (lp >= 0) & (lp + _APT_LINE_ENV <= int(n_env))
    return lp[ok], np.isin(ks[ok], num)


def apt_telemetry(words):
    """words float [n][2080] -> (channel A, channel B), each None where n < 128 or dict(levels float64 [16] (the wedges' means of the raw
    words), channel ('1', '2', '3A', '4', '5', '3B': the wedge among 1 .. 6 nearest to wedge 16, the first on a tie), gain, offset (255-scale
    value = gain * word + offset, the least-squares line through the lines of wedges 1 .. 9), phase (the line at which a 128-line frame
    starts, in [0, 128))).  A line's telemetry value is the mean of the inner 37 of the field's 45 words (the front's filter smears the
    outer ones).  The phase is the one at which those values correlate best with the staircase 31, 63, 95, 127, 159, 191, 224, 255, 0 of
    wedges 1 .. 9 (the smallest such phase on a tie)."""
    w = np.asarray(words, np.float64)
    if w.ndim != 2 or w.shape[1] != _APT_LINE_WORDS:
        raise ValueError("words: [n][2080]")
    n = w.shape[0]
    out = []
    stair = np.asarray(_APT_WEDGES)
    for c in range(2):
        if n < 128:
            out.append(None)
            continue
        first = _APT_TELEMETRY_A + c * _APT_HALF
        t = w[:, first + 4:first + _APT_TELEMETRY_WORDS - 4].mean(axis=1)
        lines = np.arange(n)
        best, best_phase = -np.inf, 0
        for phase in range(128):
            wedge = ((lines - phase) % 128) // 8
            m = wedge < 9
            x, y = stair[wedge[m]], t[m]
            xs, ys = x - x.mean(), y - y.mean()
            den = np.sqrt((xs * xs).sum() * (ys * ys).sum())
            r = (xs * ys).sum() / den if den > 0 else -np.inf
            if r > best:
                best, best_phase = r, phase
        wedge = ((lines - best_phase) % 128) // 8
        m = wedge < 9
        x, y = stair[wedge[m]], t[m]
        ys = y - y.mean()
        var = (ys * ys).sum()
        gain = float(((x - x.mean()) * ys).sum() / var) if var > 0 else 0.0
        offset = float(x.mean() - gain * y.mean())
        levels = np.array([t[wedge == k].mean() if np.any(wedge == k) else np.nan for k in range(16)])
        ident = int(np.argmin(np.abs(levels[:6] - levels[15])))
        out.append(dict(levels=levels, channel=_APT_CHANNEL_IDS[ident], gain=gain, offset=offset, phase=best_phase))
    return tuple(out)


def apt_image(words, lo_pct=1, hi_pct=99, telemetry=None):
    """words float [n][2080] -> uint8 [n][2080].  Without telemetry: the lo_pct-th percentile of the finite words goes to 0 and the
    hi_pct-th to 255.  telemetry (apt_telemetry's pair): each half of the line (1040 words) is scaled by its own channel's staircase, value
    = gain * word + offset; a half whose channel is None falls back to the percentiles.  Values are rounded half up and clipped; a word
    that is not finite gives 0."""
    w = np.asarray(words, np.float64)
    if w.ndim != 2 or w.shape[1] != _APT_LINE_WORDS:
        raise ValueError("words: [n][2080]")
    fin = np.isfinite(w)
    if fin.any():
        lo, hi = np.percentile(w[fin], [lo_pct, hi_pct])
    else:
        lo, hi = 0.0, 1.0
    g = 255.0 / (hi - lo) if hi > lo else 0.0
    v = (w - lo) * g
    if telemetry is not None:
        for c in range(2):
            if telemetry[c] is not None:
                half = slice(c * _APT_HALF, (c + 1) * _APT_HALF)
                v[:, half] = w[:, half] * telemetry[c]['gain'] + telemetry[c]['offset']
    v = np.where(fin, v, 0.0)
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def apt_channels(img):
    """[n][2080] -> (image A, image B), the two 909-column images."""
    img = np.asarray(img)
    if img.ndim != 2 or img.shape[1] != _APT_LINE_WORDS:
        raise ValueError("img: [n][2080]")
    a, b = _APT_IMAGE_A, _APT_IMAGE_A + _APT_HALF
    return img[:, a:a + _APT_IMAGE_WORDS], img[:, b:b + _APT_IMAGE_WORDS]


def write_pgm(path, img):
    """uint8 [h][w] -> a binary PGM (P5, maxval 255)."""
    img = np.ascontiguousarray(img)
    if img.ndim != 2 or img.dtype != np.uint8:
        raise ValueError("img: uint8 [h][w]")
    with open(path, 'wb') as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def apt_offset(block_means):
    """The carrier's offset from 0 Hz of one row at 62 400 S/s, in Hz, from the means of its discriminator over blocks of 1024 samples
    (float32 [n_blocks], rad a sample): the median of the inner blocks (the first and the last see the row's ends), in float64, times
    62 400 / 2 pi.  The subcarrier has no mean over a block (39.4 cycles), a click of the discriminator spoils one block and the median
    passes it by.  Fewer than three blocks, or a median that is not finite: 0.0, and the row is left as it is."""
    m = np.asarray(block_means, np.float64).ravel()[1:-1]
    if not len(m):
        return 0.0
    hz = float(np.median(m)) * _APT_RATE / (2.0 * np.pi)
    return hz if np.isfinite(hz) else 0.0


def _apt_tune_taps():
    """(the discriminator alone out of pss_ais_front, the block mean for pss_resample, the bare mixer for pss_ddc)"""
    return np.array([1.0]), np.full(_APT_TUNE_BLOCK + 1, 1.0 / (_APT_TUNE_BLOCK + 1)), np.array([1.0])


def _apt_results(n_rows, n_env, records, lines, offsets=None):
    """The host half of apt_rows: records = (row, pos, meta, score) of all rows; lines(line_row, line_pos) -> words [n][2080]."""
    row, pos, meta, score = records
    grids = []
    for r in range(n_rows):
        m = row == r
        grids.append(apt_grid(pos[m], meta[m], score[m], n_env))
    line_row = np.concatenate([np.full(len(g[0]), r, np.int32) for r, g in enumerate(grids)]) if grids else np.zeros(0, np.int32)
    line_pos = np.concatenate([g[0] for g in grids]) if grids else np.zeros(0, np.int64)
    words = lines(line_row, line_pos)
    out = []
    for r, (lp, found) in enumerate(grids):
        m = row == r
        w = words[line_row == r]
        tel = apt_telemetry(w)
        out.append(dict(words=w, image=apt_image(w, telemetry=tel), found=found, pos=lp,
                        syncs=[dict(pos=int(p), mismatches=int(e), score=float(q)) for p, e, q in zip(pos[m], meta[m], score[m])], telemetry=tel,
                        offset_hz=0.0 if offsets is None else float(offsets[r])))
    return out


def _apt_host_rows(rows):
    x = np.asarray(rows, np.complex64)
    if x.ndim not in (1, 2):
        raise ValueError("rows: a 1-D or 2-D complex array")
    return np.ascontiguousarray(x[None, :] if x.ndim == 1 else x)


def h_apt_rows(rows, sync_errors=2, taps=None, tune=True):
    """apt_rows through the host twins (pss_h_ais_front, pss_h_resample, pss_h_ddc, pss_h_apt_front, pss_h_apt_syncs, pss_h_apt_lines): no
    GPU, the same bytes."""
    from .engine import Engine
    x = _apt_host_rows(rows)
    if not x.shape[0] or not x.shape[1]:
        return [dict(words=np.zeros((0, _APT_LINE_WORDS), np.float32), image=np.zeros((0, _APT_LINE_WORDS), np.uint8), found=np.zeros(0, bool),
                     pos=np.zeros(0, np.int64), syncs=[], telemetry=(None, None), offset_hz=0.0) for _ in range(x.shape[0])]
    offsets = np.zeros(x.shape[0])
    if tune:
        one, box, mix = _apt_tune_taps()
        means = Engine.h_resample(Engine.h_ais_front(x, pulse=one), 1, _APT_TUNE_BLOCK, taps=box)
        offsets = np.array([apt_offset(m) for m in means])
        if offsets.any():
            x = x.copy()
            for r in np.flatnonzero(offsets):
                x[r] = Engine.h_ddc(x[r], [Engine.ddc_word(offsets[r], _APT_RATE)[0]], 1, taps=mix)[0]
    env = Engine.h_apt_front(x, taps=taps)
    rw, pos, meta, score, _ = Engine.h_apt_syncs(env, sync_errors=sync_errors)
    return _apt_results(x.shape[0], env.shape[1], (rw, pos, meta, score), lambda lr, lp: Engine.h_apt_lines(env, lr, lp), offsets)


def apt_rows(rows, sync_errors=2, taps=None, tune=True):
    """rows: complex64 rows at 62 400 S/s — a host array [k][n] or [n], or a resident device tensor float32 [k][2 n] — -> a list per row of
    dict(words float32 [lines][2080], image uint8 [lines][2080], found bool [lines], pos int64 [lines], syncs, telemetry): pss_apt_front
    (taps: default apt_default_taps()), pss_apt_syncs, apt_grid on the host (a few records a row), pss_apt_lines at the grid's positions —
    the lines whose sync was not found included — then apt_telemetry and apt_image.  'syncs': the receiver's records of the row as dicts
    (pos, mismatches, score); positions count envelope samples at 12 480 S/s.
    tune: in front of all that each row's carrier is put at 0 Hz, with kernels the library has: the discriminator alone (pss_ais_front
    with the pulse [1.0]), its means over blocks of 1024 samples (pss_resample, float32, 1 / 1024 with a boxcar), apt_offset on the host
    (a few hundred numbers a row), and the mixer alone (pss_ddc at decimation 1 with the tap [1.0]); 'offset_hz' is what was taken out.  A
    carrier off by f leaves the constant 2 pi f / 62 400 in the discriminator, the front's mixer moves it to 2400 Hz, where the default
    low-pass still passes 0.29 of it, and it beats against the envelope (3 kHz: the image's correlation with what was sent falls from 0.97
    to 0.92).  tune=False: the rows as they are."""
    import torch
    e = get_engine()
    if isinstance(rows, torch.Tensor):
        d_rows = rows
    else:
        d_rows = torch.from_numpy(_apt_host_rows(rows).view(np.float32)).to(f"cuda:{e.device}")
    if d_rows.dim() != 2 or d_rows.dtype != torch.float32 or d_rows.shape[1] % 2 or not d_rows.is_contiguous():
        raise ValueError("rows: a contiguous device tensor float32 [k][2 n]")
    k, n = d_rows.shape[0], d_rows.shape[1] // 2
    if not k or not n:
        return h_apt_rows(np.zeros((k, 0), np.complex64))
    dev = d_rows.device
    offsets = np.zeros(k)
    if tune:
        one, box, mix = _apt_tune_taps()
        d_disc = torch.empty((k, n), dtype=torch.float32, device=dev)
        e.ais_front(d_rows, k, n, d_disc, pulse=one)
        n_blocks = e.resample_out_len(n, 1, _APT_TUNE_BLOCK)
        d_means = torch.empty((k, n_blocks), dtype=torch.float32, device=dev)
        e.resample(d_disc, np.float32, k, n, 1, _APT_TUNE_BLOCK, d_means, taps=box)
        offsets = np.array([apt_offset(m) for m in d_means.cpu().numpy()])
        del d_disc
        if offsets.any():
            d_tuned = d_rows.clone()
            for r in np.flatnonzero(offsets):
                e.ddc(d_rows[r], n, np.array([e.ddc_word(offsets[r], _APT_RATE)[0]], np.uint64), 1, d_tuned[r], taps=mix)
            d_rows = d_tuned
    n_env = -(-n // e.APT_DECIM)
    d_env = torch.empty((k, n_env), dtype=torch.float32, device=dev)
    e.apt_front(d_rows, k, n, d_env, taps=taps)
    room = 4096
    while True:
        d_row = torch.empty(room, dtype=torch.int32, device=dev)
        d_pos = torch.empty(room, dtype=torch.int64, device=dev)
        d_meta = torch.empty(room, dtype=torch.int32, device=dev)
        d_score = torch.empty(room, dtype=torch.float32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        e.apt_syncs(d_env, k, n_env, d_row, d_pos, d_meta, d_score, d_count, room, sync_errors=sync_errors)
        c = int(d_count.cpu()[0])
        if c <= room:
            break
        room = c   # the true count: again with room for it
    records = tuple(t[:c].cpu().numpy() for t in (d_row, d_pos, d_meta, d_score))

    def lines(line_row, line_pos):
        if not len(line_pos):
            return np.zeros((0, _APT_LINE_WORDS), np.float32)
        d_words = torch.empty((len(line_pos), _APT_LINE_WORDS), dtype=torch.float32, device=dev)
        e.apt_lines(d_env, k, n_env, torch.from_numpy(line_row).to(dev), torch.from_numpy(line_pos).to(dev), len(line_pos), d_words)
        return d_words.cpu().numpy()

    return _apt_results(k, n_env, records, lines, offsets)


def apt_recording(samples, fs, center_hz, channels_hz=(137.62e6,), taps=None, front_taps=None, sync_errors=2, chunk_samples=1 << 22,
                  codes_format=None, table=None, tune=True):
    """The weather-satellite images of a capture centred on center_hz -> dict(rows=apt_rows' list, one entry per channel of channels_hz,
    fs=12480: the rate the positions count in).  On the GPU from the upload to the words: pss_ddc puts the listed channels at 0 Hz at
    apt_plan(fs)'s decimation (streamed in chunks of chunk_samples samples plus their halos; the result does not depend on
    chunk_samples), pss_resample brings them to 62 400 S/s where the decimated rate is another one, then apt_rows (front_taps: its taps;
    tune: its carrier step).
    taps: the down-converter's float64 low-pass (default firwin(20 decim + 1, 40 000 / fs): half-width 20 kHz, the reference's NOAA_SAT
    bandwidth); codes_format / table: as demodulate_recording."""
    import torch
    e = get_engine()
    fs = float(fs)
    decim, up, down = e.apt_plan(fs)
    offsets = np.atleast_1d(np.asarray(channels_hz, np.float64)) - float(center_hz)
    if offsets.ndim != 1 or not len(offsets):
        raise ValueError("channels_hz: a list of frequencies")
    if taps is None:
        taps = np.empty(20 * decim + 1, np.float64)
        if e.lib.pss_design_firwin(len(taps), 40000.0 / fs, taps.ctypes.data) != 0:
            raise ValueError("apt_recording: the down-converter's filter design failed")
    d_rows, _ = _tune_device(samples, fs, offsets, decim, taps, None, chunk_samples, codes_format, table)
    k, m = d_rows.shape[0], d_rows.shape[1] // 2
    if (up, down) != (1, 1):
        n = e.resample_out_len(m, up, down)
        d_bb = torch.empty((k, 2 * max(n, 1)), dtype=torch.float32, device=d_rows.device)
        if m:
            e.resample(d_rows, np.complex64, k, m, up, down, d_bb)
        d_rows, m = d_bb[:, :2 * n].contiguous() if n else d_bb[:, :0], n
    return dict(rows=apt_rows(d_rows.contiguous(), sync_errors, front_taps, tune), fs=_APT_ENV_RATE)


# ---- packet radio: the AX.25 frames and APRS reports of a 2 m capture (the arithmetic of the device stages: csrc/pss_packet.h)
_PACKET_RATE = 26400
_PACKET_REC = 332


def _ax25_address(a):
    return dict(call=bytes(b >> 1 for b in a[:6]).decode('latin-1').rstrip(), ssid=(a[6] >> 1) & 0xF, repeated=bool(a[6] & 0x80))


def ax25_decode(frame):
    """An AX.25 frame WITHOUT its two check bytes -> dict(dest=..., source=..., path=[...], control=..., pid=..., info=...): every address
    a dict(call, ssid, repeated: the has-been-repeated bit of a digipeater address, the command / response bit of the first two), pid None
    where the frame type carries none (everything but I and UI frames), info the bytes behind.  ValueError where the address field does
    not end inside the frame on a multiple of 7 bytes."""
    f = bytes(frame)
    end = next((j for j, b in enumerate(f) if b & 1), None)
    if end is None or end % 7 != 6 or end < 13 or len(f) < end + 2:
        raise ValueError("ax25_decode: a malformed address field")
    addrs = [_ax25_address(f[j:j + 7]) for j in range(0, end + 1, 7)]
    control = f[end + 1]
    has_pid = (control & 1) == 0 or (control & 0xEF) == 0x03
    rest = f[end + 2:]
    if has_pid and not rest:
        has_pid = False
    return dict(dest=addrs[0], source=addrs[1], path=addrs[2:], control=control, pid=rest[0] if has_pid else None, info=rest[1:] if has_pid else rest)


def _ax25_name(a):
    return a['call'] + (f"-{a['ssid']}" if a['ssid'] else "")


def aprs_tnc2(frame):
    """The monitor line direwolf prints for a frame (without check bytes): `SRC-7>DST,WIDE1-1*,WIDE2-2:info`, the star behind the last
    digipeater that has repeated the frame, the information field as Latin-1."""
    d = ax25_decode(frame) if not isinstance(frame, dict) else frame
    last = max((i for i, a in enumerate(d['path']) if a['repeated']), default=-1)
    hops = "".join("," + _ax25_name(a) + ("*" if i == last else "") for i, a in enumerate(d['path']))
    return f"{_ax25_name(d['source'])}>{_ax25_name(d['dest'])}{hops}:{bytes(d['info']).decode('latin-1')}"


def _b91(s):
    v = 0
    for c in s:
        v = v * 91 + (ord(c) - 33)
    return v


def _aprs_position(body, out):
    """body: the information field behind the type character and the timestamp."""
    if len(body) >= 19 and body[0].isdigit():
        lat, ns, table, lon, ew, code = body[0:7], body[7], body[8], body[9:17], body[17], body[18]
        try:
            la = int(lat[0:2]) + float(lat[2:7].replace(' ', '0')) / 60.0
            lo = int(lon[0:3]) + float(lon[3:8].replace(' ', '0')) / 60.0
        except ValueError:
            return
        if ns not in 'NS' or ew not in 'EW':
            return
        out.update(lat=-la if ns == 'S' else la, lon=-lo if ew == 'W' else lo, symbol=table + code, compressed=False, comment=body[19:])
        c = body[19:26]
        if len(c) == 7 and c[3] == '/' and c[:3].isdigit() and c[4:].isdigit():
            out.update(course=int(c[:3]), speed=float(int(c[4:])), comment=body[26:])
    elif len(body) >= 13 and all(33 <= ord(ch) <= 124 for ch in body[1:9]):
        table, code, cs, t = body[0], body[9], body[10:12], ord(body[12]) - 33
        out.update(lat=90.0 - _b91(body[1:5]) / 380926.0, lon=-180.0 + _b91(body[5:9]) / 190463.0, symbol=table + code, compressed=True,
                   comment=body[13:])
        c, s = ord(cs[0]) - 33, ord(cs[1]) - 33
        if cs[0] == ' ':
            pass
        elif 0 <= t and (t & 0x18) == 0x10:
            out['altitude_ft'] = 1.002 ** (c * 91 + s)
        elif 0 <= c <= 89:
            out.update(course=c * 4, speed=1.08 ** s - 1.0)
        elif cs[0] == '{':
            out['range_miles'] = 2.0 * 1.08 ** s


def aprs_decode(info):
    """An APRS information field (bytes or str) -> dict: 'type' (its first character), 'raw' (the text behind it, Latin-1) and, by type:
    positions `! = / @` (the last two with 'timestamp', 7 characters), uncompressed or base-91 compressed: 'lat', 'lon' (degrees), 'symbol'
    (table and code), 'compressed', 'comment', and 'course' (degrees) / 'speed' (knots) where given ('altitude_ft' / 'range_miles' where the
    compressed form carries those); status `>`: 'status'; messages `:`: 'addressee', 'text', 'number' (None without one).  Everything else,
    Mic-E (` and ') included, as type and raw text."""
    text = bytes(info).decode('latin-1') if not isinstance(info, str) else info
    out = dict(type=text[:1], raw=text[1:])
    kind, body = text[:1], text[1:]
    if kind in '!=' and kind:
        _aprs_position(body, out)
    elif kind in '/@' and kind and len(body) >= 7:
        out['timestamp'] = body[:7]
        _aprs_position(body[7:], out)
    elif kind == '>':
        out['status'] = body
    elif kind == ':' and len(body) >= 10 and body[9] == ':':
        msg, _, number = body[10:].partition('{')
        out.update(addressee=body[:9].rstrip(), text=msg, number=number if number else None)
    return out


def aprs_tracks(records, fs=_PACKET_RATE):
    """records: the frames in order, each a mapping with 'msg' (the frame without check bytes) and 'pos' (packet_recording's 'frames') ->
    one dict per source call in order of first appearance: 'source', 'position' ((latitude, longitude)), 'symbol', 'course', 'speed',
    'status' (the last of each, or None), 'frames', 'first' and 'last' (pos / fs, seconds)."""
    fs = float(fs)
    tracks = {}
    for rec in records:
        ax = ax25_decode(rec['msg'])
        d = aprs_decode(ax['info'])
        t = int(rec['pos']) / fs
        src = _ax25_name(ax['source'])
        tr = tracks.setdefault(src, dict(source=src, position=None, symbol=None, course=None, speed=None, status=None, frames=0, first=t, last=t))
        tr['frames'] += 1
        tr['first'], tr['last'] = min(tr['first'], t), max(tr['last'], t)
        for key in ('symbol', 'course', 'speed', 'status'):
            if d.get(key) is not None:
                tr[key] = d[key]
        if d.get('lat') is not None:
            tr['position'] = (d['lat'], d['lon'])
    return list(tracks.values())


def _packet_records(msg, ln, row, pos, score):
    """The receiver's arrays -> one dict per frame in order of (pos, row): 'msg' (bytes without the check bytes), 'row', 'pos', 'score',
    ax25_decode's keys, 'tnc2' and 'aprs' (aprs_decode of the information field)."""
    out = []
    for m, n, r, p, q in zip(msg, ln, row, pos, score):
        body = bytes(m[:int(n) - 2])
        d = ax25_decode(body)
        d.update(msg=body, row=int(r), pos=int(p), score=float(q), tnc2=aprs_tnc2(d), aprs=aprs_decode(d['info']))
        out.append(d)
    out.sort(key=lambda f: (f['pos'], f['row']))
    return out


def h_packet_rows(rows, tones=None, space_gain=1.0, q_min=0.0):
    """packet_rows through the host twins (pss_h_packet_front, pss_h_packet_frames): no GPU, the same bytes."""
    from .engine import Engine
    x = np.asarray(rows, np.complex64)
    if x.ndim not in (1, 2):
        raise ValueError("rows: a 1-D or 2-D complex array")
    x = np.ascontiguousarray(x[None, :] if x.ndim == 1 else x)
    if not x.shape[0] or not x.shape[1]:
        return []
    z = Engine.h_packet_front(x, tones=tones, space_gain=space_gain)
    return _packet_records(*Engine.h_packet_frames(z, q_min=q_min)[:5])


def packet_rows(rows, tones=None, space_gain=1.0, q_min=0.0):
    """rows: complex64 rows at 26 400 S/s — a host array [k][n] or [n], or a resident device tensor float32 [k][2 n] — -> the frames, a list
    of dicts in order of (pos, row): pss_packet_front (tones: default packet_default_tones(); space_gain: the weight of the 2200 Hz energy,
    below 1 for a pre-emphasised sender heard without de-emphasis) and pss_packet_frames (q_min) on the resident rows, then ax25_decode,
    aprs_tnc2 and aprs_decode of every record."""
    import torch
    e = get_engine()
    if isinstance(rows, torch.Tensor):
        d_rows = rows
    else:
        x = np.asarray(rows, np.complex64)
        if x.ndim not in (1, 2):
            raise ValueError("rows: a 1-D or 2-D complex array")
        x = np.ascontiguousarray(x[None, :] if x.ndim == 1 else x)
        d_rows = torch.from_numpy(x.view(np.float32)).to(f"cuda:{e.device}")
    if d_rows.dim() != 2 or d_rows.dtype != torch.float32 or d_rows.shape[1] % 2 or not d_rows.is_contiguous():
        raise ValueError("rows: a contiguous device tensor float32 [k][2 n]")
    k, n = d_rows.shape[0], d_rows.shape[1] // 2
    if not k or not n:
        return []
    dev = d_rows.device
    d_z = torch.empty((k, n), dtype=torch.float32, device=dev)
    e.packet_front(d_rows, k, n, d_z, tones=tones, space_gain=space_gain)
    room = 4096
    while True:
        d_msg = torch.empty((room, _PACKET_REC), dtype=torch.uint8, device=dev)
        d_len = torch.empty(room, dtype=torch.int32, device=dev)
        d_row = torch.empty(room, dtype=torch.int32, device=dev)
        d_pos = torch.empty(room, dtype=torch.int64, device=dev)
        d_score = torch.empty(room, dtype=torch.float32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        e.packet_frames(d_z, k, n, d_msg, d_len, d_row, d_pos, d_score, d_count, room, q_min=q_min)
        c = int(d_count.cpu()[0])
        if c <= room:
            break
        room = c   # the true count: again with room for it
    return _packet_records(*(t[:c].cpu().numpy() for t in (d_msg, d_len, d_row, d_pos, d_score)))


def packet_recording(samples, fs, center_hz, channels_hz=(144.8e6,), taps=None, tones=None, chunk_samples=1 << 22, space_gain=1.0, q_min=0.0,
                     codes_format=None, table=None):
    """The packets of a 2 m capture centred on center_hz -> dict(frames=..., tracks=..., lines=..., fs=26400): 'frames' packet_rows' dicts in
    order of 'pos' ('row' is the channel's position in channels_hz), 'tracks' aprs_tracks(frames), 'lines' the monitor line of every frame,
    'fs' the rate the positions count in.  On the GPU from the upload to the records: pss_ddc puts the listed channels at 0 Hz at
    packet_plan(fs)'s decimation (streamed in chunks of chunk_samples samples plus their halos; the result does not depend on
    chunk_samples), pss_resample brings them to 26 400 S/s where the decimated rate is another one, then packet_rows.  taps: the
    down-converter's float64 low-pass (default firwin(20 decim + 1, 16 000 / fs): half-width 8 kHz, 3 kHz deviation and 2.2 kHz audio by
    Carson's rule with room for the carrier's error); codes_format / table: as demodulate_recording."""
    import torch
    e = get_engine()
    fs = float(fs)
    decim, up, down = e.packet_plan(fs)
    offsets = np.atleast_1d(np.asarray(channels_hz, np.float64)) - float(center_hz)
    if offsets.ndim != 1 or not len(offsets):
        raise ValueError("channels_hz: a list of frequencies")
    if taps is None:
        taps = np.empty(20 * decim + 1, np.float64)
        if e.lib.pss_design_firwin(len(taps), 16000.0 / fs, taps.ctypes.data) != 0:
            raise ValueError("packet_recording: the down-converter's filter design failed")
    d_rows, _ = _tune_device(samples, fs, offsets, decim, taps, None, chunk_samples, codes_format, table)
    k, m = d_rows.shape[0], d_rows.shape[1] // 2
    if (up, down) != (1, 1):
        n = e.resample_out_len(m, up, down)
        d_bb = torch.empty((k, 2 * max(n, 1)), dtype=torch.float32, device=d_rows.device)
        if m:
            e.resample(d_rows, np.complex64, k, m, up, down, d_bb)
        d_rows, m = d_bb[:, :2 * n].contiguous() if n else d_bb[:, :0], n
    frames = packet_rows(d_rows.contiguous(), tones, space_gain, q_min) if m else []
    return dict(frames=frames, tracks=aprs_tracks(frames), lines=[f['tnc2'] for f in frames], fs=_PACKET_RATE)


def recording_to_wav(npy_path, wav_path, sample_rate, mode='NFM', frame_len=32768, codes_format=None, table=None):
    """codes_format: npy_path is a raw file of ADC codes (load_iq_codes) instead of the reference's .npy."""
    if codes_format is not None:
        samples = load_iq_codes(npy_path, codes_format)
    else:
        samples = load_iq_recording(npy_path)
    pcm = demodulate_recording(samples, sample_rate, mode, frame_len, codes_format=codes_format, table=table)
    write_wav(wav_path, pcm)
    return pcm

"""The reference's decoders (xqtr/PySpecSDR decoders.py) on libpss.so: same names, arguments and return values.

    decode_morse(samples, sample_rate, threshold=-20) -> (text, {"dot", "dash", "gap"})     decoders.py:136-231
    decode_aprs(samples, sample_rate)                 -> [packet] or []                       :115-133
    decode_afsk(samples, sample_rate)                 -> list of 0 / 1                        :94-112
    decode_ax25_frame(bit_stream)                     -> "SRC>DEST:info" or None             :6-63
    decode_aprs_payload(frame_bytes)                  -> "SRC>DEST:info" or None             :66-91

The sample-rate halves run on the GPU (envelope mask + edge compaction: pss_morse_edges; normalisation, the Bell-202 band-pass pair and
the per-bit energy compare: pss_afsk_bits), the per-message halves in the library's host code (pss_h_morse_decode, pss_h_ax25_frame).
decode_morse's two pulse classes come from a deterministic search where the reference draws random starting points for scipy's kmeans:
identical centroids for keyed signals (include/pss.h), a reproducible answer for noise.  Batched building blocks for callers that want
only the front halves: afsk_bits(), morse_edges().

For batches of read buffers both halves run on the GPU, one library call per batch (pss_decode_morse_batch, pss_decode_aprs_batch):

    decode_morse_batch(frames, sample_rate, threshold=-20) -> [(text, timing dict), ...]
    decode_aprs_batch(frames, sample_rate)                 -> [[packet] or [], ...]      complex64 buffers, normalised in float32

formats.decode_recording cuts a recording into read buffers and runs them through these.

The zero-edit launcher (python -m pyspecsdr_amd.run) leaves the application's own `import decoders` alone by default — its decoders.py
then runs its bookkeeping on top of the GPU band-pass (decoders.py:3 imports bandpass_filter from signal_processing); `--gpu-decoders`
registers this module under the name `decoders` as well.
"""
import ctypes as C

import numpy as np

from . import signal_processing as _sp


def _bandpass_tables(sample_rate):
    if _sp.USE_SCIPY_DESIGNS:
        try:
            import scipy.signal as ss
            nyq = sample_rate / 2
            return tuple(np.ascontiguousarray(ss.butter(_sp.BUTTER_ORDER, [lo / nyq, hi / nyq], btype="band", output="sos"))
                         for lo, hi in ((1100, 1300), (2100, 2300)))
        except ImportError:
            pass
    return (None, None)


def afsk_bits(samples, sample_rate, normalise=False):
    """-> uint8 array, one 0/1 per bit period of int(sample_rate / 1200) samples."""
    x = np.asarray(samples)
    if np.iscomplexobj(x):
        x = np.real(x)
    x = np.ascontiguousarray(x, dtype=np.float64)
    return _sp.get_engine().h_afsk_bits(x, sample_rate, *_bandpass_tables(sample_rate), normalise=normalise)


def morse_edges(samples, threshold=-20):
    """-> (rise_times, fall_times): int32 sample indices where the -20 dB envelope mask switches on / off."""
    return _sp.get_engine().h_morse_edges(_sp._samples(samples), threshold)


def decode_afsk(samples, sample_rate):
    return [int(b) for b in afsk_bits(samples, sample_rate)]


def _lib():
    return _sp.get_engine().lib


def morse_from_edges(rise_times, fall_times, sample_rate):
    """The back half of decode_morse on its own: (text, timing dict) from the rise / fall indices."""
    from . import _lib as L
    lib = L.load()
    rise = np.ascontiguousarray(rise_times, np.int32)
    fall = np.ascontiguousarray(fall_times, np.int32)
    cap = 4 * (len(rise) + 2) + 16
    text = C.create_string_buffer(cap)
    tm = np.zeros(3)
    r = lib.pss_h_morse_decode(rise.ctypes.data, len(rise), fall.ctypes.data, len(fall), float(sample_rate), text, cap, tm.ctypes.data)
    if r < 0:
        raise ValueError("operands could not be broadcast together: rise / fall edges do not alternate")
    n_gaps = _n_gaps(rise, fall)
    if n_gaps < 0:                     # no complete pulse: the reference's early returns
        return "", {"dot": 0, "dash": 0, "gap": 0}
    return text.raw[:r].decode("ascii"), {"dot": np.float64(tm[0]), "dash": np.float64(tm[1]), "gap": np.float64(tm[2]) if n_gaps > 0 else 0}


def _n_gaps(rise, fall):
    """Number of gaps between the complete pulses of an edge list (-1: no complete pulse)."""
    nr, nf = len(rise), len(fall)
    if nr == 0 or nf == 0:
        return -1
    if fall[0] < rise[0]:
        nf -= 1
    if nr > nf:
        nr -= 1
    return nr - 1


def decode_morse(samples, sample_rate, threshold=-20):
    rise, fall = morse_edges(samples, threshold)
    return morse_from_edges(rise, fall, sample_rate)


def _upload_frames(e, frames):
    """Read buffers [n_frames][n] (anything np.asarray takes; complex64 as the application hands them over) -> float32 device view."""
    import torch
    x = np.ascontiguousarray(np.asarray(frames), np.complex64)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("frames: [n_frames][n] read buffers, n >= 1")
    return torch.from_numpy(x.view(np.float32)).to(f"cuda:{e.device}"), x.shape[0], x.shape[1]


def _morse_batch_dev(e, d_iq, n_frames, n, sample_rate, threshold=-20):
    """decode_morse for the complex64 frames on the device (d_iq: float32 [n_frames][2 n]): one library call, one download of the texts'
    used columns -> list of (text, timing dict), each what morse_from_edges returns for that buffer."""
    import torch
    if n_frames == 0:
        return []
    dev = lambda shape, dt: torch.empty(shape, dtype=dt, device=f"cuda:{e.device}")
    cap = n // 2 + 1
    d_rise, d_fall, d_counts = dev((n_frames, cap), torch.int32), dev((n_frames, cap), torch.int32), dev((n_frames, 2), torch.int32)
    d_text, d_len = dev((n_frames, 2 * cap), torch.uint8), dev(n_frames, torch.int32)
    d_tm, d_np = dev((n_frames, 3), torch.float64), dev(n_frames, torch.int32)
    e.decode_morse_batch(d_iq, n_frames, n, sample_rate, d_rise, d_fall, d_counts, d_text, d_len, d_tm, d_np, threshold_db=threshold)
    ln, tm, pulses = d_len.cpu().numpy(), d_tm.cpu().numpy(), d_np.cpu().numpy()
    if (pulses < 0).any():   # cannot happen behind pss_morse_edges with this cap: its edges alternate and number at most n // 2 + 1
        raise ValueError("operands could not be broadcast together: rise / fall edges do not alternate")
    text = d_text[:, :max(int(ln.max()), 1)].cpu().numpy()
    out = []
    for f in range(n_frames):
        if pulses[f] == 0:                 # no complete pulse: the reference's early returns
            out.append(("", {"dot": 0, "dash": 0, "gap": 0}))
        else:
            out.append((text[f, :ln[f]].tobytes().decode("ascii"),
                        {"dot": np.float64(tm[f, 0]), "dash": np.float64(tm[f, 1]), "gap": np.float64(tm[f, 2]) if pulses[f] > 1 else 0}))
    return out


def _aprs_batch_dev(e, d_iq, n_rows, n, sample_rate, tables=None, want_bits=False):
    """decode_aprs for the complex64 frames on the device -> list of packet lists (and the uint8 bit rows [n_rows][n_bits])."""
    import torch
    nb = max(e.afsk_n_bits(n, sample_rate), 0)
    if n_rows == 0:
        return ([], np.zeros((0, nb), np.uint8)) if want_bits else []
    dev = lambda shape, dt: torch.empty(shape, dtype=dt, device=f"cuda:{e.device}")
    s1, s2 = _bandpass_tables(sample_rate) if tables is None else tables
    out_cap = nb // 8 + 64
    d_audio, d_bits = dev((n_rows, n), torch.float64), dev((n_rows, nb), torch.uint8)
    d_out, d_len = dev((n_rows, out_cap), torch.uint8), dev(n_rows, torch.int32)
    e.decode_aprs_batch(d_iq, n_rows, n, sample_rate, d_audio, d_bits, out_cap, d_out, d_len, s1, s2)
    ln = d_len.cpu().numpy()
    pk = d_out[:, :max(int(ln.max()), 1)].cpu().numpy()
    out = [[pk[r, :ln[r]].tobytes().decode("latin-1")] if ln[r] > 0 else [] for r in range(n_rows)]   # `[packet] if packet else []`
    return (out, d_bits.cpu().numpy()) if want_bits else out


def decode_morse_batch(frames, sample_rate, threshold=-20):
    """decode_morse for every read buffer of frames [n_frames][n] -> list of (text, timing dict), one library call for the batch."""
    e = _sp.get_engine()
    d_iq, nf, n = _upload_frames(e, frames)
    return _morse_batch_dev(e, d_iq, nf, n, sample_rate, threshold)


def decode_aprs_batch(frames, sample_rate):
    """decode_aprs for every complex64 read buffer of frames [n_rows][n] -> list of packet lists ([packet] or []).  The real parts are
    normalised in float32, as the reference's division of np.real(complex64) is (decode_aprs above widens first: PARITY.md)."""
    e = _sp.get_engine()
    d_iq, nf, n = _upload_frames(e, frames)
    return _aprs_batch_dev(e, d_iq, nf, n, sample_rate)


def decode_ax25_frame(bit_stream):
    from . import _lib as L
    lib = L.load()
    bits = np.ascontiguousarray(np.asarray(bit_stream, dtype=np.uint8))
    cap = len(bits) // 8 + 64
    out = C.create_string_buffer(cap)
    n = C.c_long(0)
    r = lib.pss_h_ax25_frame(bits.ctypes.data, len(bits), out, cap, C.byref(n))
    if r != 1:
        return None
    return out.raw[:n.value].decode("latin-1")


def decode_aprs_payload(frame_bytes):
    """The address / information fields of a list of frame bytes (the reference's helper; here a thin pure-Python statement of the format:
    it never sees sample data)."""
    fb = [int(b) & 0xFF for b in frame_bytes]
    if len(fb) < 14:
        return None
    dest = "".join(chr((b >> 1) & 0x7F) for b in fb[0:6]).strip()
    source = "".join(chr((b >> 1) & 0x7F) for b in fb[7:13]).strip()
    info = "".join(chr(b) for b in fb[15:]) if len(fb) > 15 else ""
    return f"{source}>{dest}:{info}"


def decode_aprs(samples, sample_rate):
    x = np.asarray(samples)
    if np.iscomplexobj(x):
        x = np.real(x)
    x = np.ascontiguousarray(x, dtype=np.float64)
    eng = _sp.get_engine()
    s1, s2 = _bandpass_tables(sample_rate)
    cap = len(x) // 8 + 64
    out = C.create_string_buffer(cap)
    n = C.c_long(0)
    r = eng.lib.pss_h_decode_aprs(eng.h, x.ctypes.data, len(x), float(sample_rate), None if s1 is None else s1.ctypes.data,
                                  None if s2 is None else s2.ctypes.data, 0 if s1 is None else s1.shape[0], out, cap, C.byref(n))
    if r < 0:
        eng._ck(r)
    return [out.raw[:n.value].decode("latin-1")] if r == 1 else []

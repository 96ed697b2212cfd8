"""ADS-B test captures and an independent statement of the receiver's rules, NumPy only and no library code.

    messages -> chips (a preamble with pulses at chips 0, 2, 7, 9, then one chip pair per bit: pulse first for a 1) at spc samples a chip,
    amplitude and carrier phase stated -> added to seeded unit-variance complex Gaussian noise -> complex64.

numpy_frames restates rules 1-7 of PARITY.md "ADS-B": vectorised float32, the chip sums added one term at a time.
tools/make_goldens_adsb.py stores the messages, positions and expected records of every case in tests/golden/adsb.npz, with a CRC-32 of
each capture; the captures are regenerated here.
"""
import zlib

import numpy as np

GENERATOR = 0x1FFF409
PULSES = (0, 2, 7, 9)

# published vectors (remainder 0) and two messages built from them
IDENT = "8D4840D6202CC371C32CE0576098"       # DF 17, 4840D6, type code 4, KLM1023
POS_EVEN = "8D40621D58C382D690C8AC2863A7"    # type code 11, 38 000 ft, (93000, 51372)
POS_ODD = "8D40621D58C386435CC412692AD6"     # the odd frame: (74158, 50194)
VELOCITY = "8D485020994409940838175B284F"    # type code 19 subtype 1: 159.20 kt, 182.88 deg, -832 ft/min
ALL_CALL = "5D4840D6F8740F"                  # DF 11, remainder 0
ALT_REPLY = "20000B38AB0D0D"                 # DF 4, remainder 4840D6
VECTORS = (IDENT, POS_EVEN, POS_ODD, VELOCITY, ALL_CALL, ALT_REPLY)
ADDRESS = 0x4840D6


def crc24(data):
    """The 24-bit remainder of a byte string under the generator, one bit at a time."""
    r = 0
    for byte in bytes(data):
        for k in range(7, -1, -1):
            r = (r << 1) | ((byte >> k) & 1)
            if r & 0x1000000:
                r ^= GENERATOR
    return r


def with_parity(head_hex):
    """A message whose last three bytes make the remainder zero."""
    head = bytes.fromhex(head_hex)
    return (head + crc24(head + b"\0\0\0").to_bytes(3, "big")).hex().upper()


DF19 = with_parity("9840621D58C382D690C8AC")     # a military extended squitter with correct parity: not a reported format
DF24 = with_parity("C540621D58C382D690C8AC")     # Comm-D, likewise


def msg_bits(msg_hex):
    return np.unpackbits(np.frombuffer(bytes.fromhex(msg_hex), np.uint8))


def chips_of(msg_hex):
    """The frame as chips: 1.0 where a pulse is sent."""
    bits = msg_bits(msg_hex)
    c = np.zeros(16 + 2 * len(bits))
    c[list(PULSES)] = 1.0
    c[16 + 2 * np.arange(len(bits)) + (1 - bits)] = 1.0
    return c


def synth(n, spc, frames, seed=None, sigma=1.0):
    """frames: (msg_hex, pos, amplitude, phase) -> complex64 [n].  seed None: no noise."""
    if seed is None:
        x = np.zeros(n, np.complex128)
    else:
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (sigma / np.sqrt(2.0))
    for msg, pos, amp, phase in frames:
        wave = np.repeat(chips_of(msg), spc) * (amp * np.exp(1j * phase))
        x[pos:pos + len(wave)] += wave
    return x.astype(np.complex64)


RATE_CASE_US = (300.13, 2100.44, 4000.2, 6500.55)     # a 2.4 MS/s capture's frames: on no sample of either rate
RATE_CASE_SEED = 32


def synth_rate(n, fs, frames, seed, fine=20):
    """A capture at a rate that is no multiple of the chip rate: frames (msg_hex, start in microseconds, amplitude, phase); every sample is
    the mean of the chip waveform over its own sample period (`fine` points a sample), added to unit noise -> complex64 [n]."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    t_us = (np.arange(n * fine) + 0.5) / (fs / 1e6 * fine)
    for msg, t0, amp, phase in frames:
        c = chips_of(msg)
        chip = np.floor((t_us - t0) * 2.0).astype(np.int64)
        inside = (chip >= 0) & (chip < len(c))
        w = np.zeros(n * fine)
        w[inside] = c[chip[inside]]
        x += amp * np.exp(1j * phase) * w.reshape(n, fine).mean(1)
    return x.astype(np.complex64)


def numpy_frames(iq, spc, ratio=2.0, icao=(), s_begin=0, s_end=None, buf_index0=0, n_capture=None, max_frames=None, stats=None):
    """Rules 1-7 on a buffer that holds capture samples [buf_index0, buf_index0 + len(iq)) -> (msg uint8 [k][14], pos int64, meta uint32,
    score float32, count).  stats: a dict that receives 'survivors', the evaluated starts whose preamble passed."""
    iq = np.asarray(iq, np.complex64)
    n_capture = buf_index0 + len(iq) if n_capture is None else n_capture
    s_end = n_capture if s_end is None else s_end
    re, im = iq.real.astype(np.float32), iq.imag.astype(np.float32)
    m = re * re + im * im                                     # rule 1: two float32 products and an add
    nb = len(m) - spc + 1
    acc = []
    if nb > 0:
        B = m[:nb].copy()
        for k in range(1, spc):                               # rule 2: ascending, from the first term
            B = B + m[k:k + nb]
        e0, e1 = max(0, s_begin - (2 * spc - 1)), min(n_capture, s_end + 2 * spc - 1)
        s = np.arange(e0, min(e1, n_capture - spc * 128 + 1), dtype=np.int64)     # a short frame fits
        if len(s):
            j = s - buf_index0
            E = np.stack([B[j + spc * c] for c in range(16)])
            with np.errstate(invalid="ignore", over="ignore"):
                hi = np.minimum.reduce(E[list(PULSES)])           # NumPy's minimum and maximum hand a NaN on
                lo = np.maximum.reduce(E[[c for c in range(16) if c not in PULSES]])
                ok = hi > np.float32(ratio) * lo                  # rule 3
            if stats is not None:
                stats['survivors'] = int(np.count_nonzero(ok))
            icao = set(int(a) for a in icao)
            for t in np.flatnonzero(ok):
                s_t, j_t = int(s[t]), int(j[t])
                n_bits = 112 if B[j_t + spc * 16] > B[j_t + spc * 17] else 56
                if s_t + spc * (16 + 2 * n_bits) > n_capture:
                    continue
                at = j_t + spc * (16 + 2 * np.arange(n_bits))
                msg = np.packbits(B[at] > B[at + spc])            # rule 4
                r, df = crc24(msg.tobytes()), int(msg[0]) >> 3
                if (df in (17, 18) and r == 0) or (df == 11 and r & 0xFFFF80 == 0) or (df in (0, 4, 5, 16, 20, 21) and r in icao):   # rule 5
                    acc.append((s_t, n_bits, df, np.float32(hi[t]), np.pad(msg, (0, 14 - len(msg)))))
    out = []
    for a in acc:                                             # rule 6, every pair
        if not s_begin <= a[0] < s_end:
            continue
        if any(b[1] == a[1] and np.array_equal(b[4], a[4]) and 0 < abs(b[0] - a[0]) < 2 * spc and (b[3] > a[3] or (b[3] == a[3] and b[0] < a[0]))
               for b in acc):
            continue
        out.append(a)
    count = len(out)
    if max_frames is not None:
        out = out[:max_frames]
    return (np.array([a[4] for a in out], np.uint8).reshape(-1, 14), np.array([a[0] for a in out], np.int64),
            np.array([a[1] | (a[2] << 16) for a in out], np.uint32), np.array([a[3] for a in out], np.float32), count)


# ---- the fixture's captures: name -> (spc, n, seed, amplitude, addresses, [(message, position, phase)])
def _case(spc, seed, msgs, addresses=(), amp=10.0, gap=37):
    frames, pos = [], 23 * spc + 5
    for k, msg in enumerate(msgs):
        frames.append((msg, pos, 0.7 * k + 0.3))
        pos += spc * (16 + 8 * len(msg)) + gap * spc + k      # offsets that are no multiple of spc
    return (spc, pos + 101, seed, amp, tuple(addresses), frames)


CASES = {
    "spc1": _case(1, 101, [IDENT, ALL_CALL, POS_EVEN, DF19, ALT_REPLY, VELOCITY], [ADDRESS]),
    "spc2": _case(2, 102, [POS_ODD, ALT_REPLY, DF24, IDENT, POS_EVEN], [0x123456, ADDRESS, 0xABCDEF]),
    "spc3": _case(3, 103, [VELOCITY, IDENT, ALL_CALL, DF19, POS_ODD]),
    "spc5": _case(5, 105, [IDENT, POS_EVEN, ALT_REPLY, ALL_CALL, VELOCITY, DF24], [ADDRESS]),
    "spc8": _case(8, 108, [POS_EVEN, IDENT, VELOCITY, ALL_CALL]),
}
REPORTED_DF = (0, 4, 5, 11, 16, 17, 18, 20, 21)


def case_iq(name):
    spc, n, seed, amp, _, frames = CASES[name]
    return synth(n, spc, [(m, p, amp, ph) for m, p, ph in frames], seed)


def case_expected(name):
    """The injected frames that must be reported: (message bytes padded to 14, position), in order."""
    _, _, _, _, addresses, frames = CASES[name]
    out = []
    for m, p, _ in frames:
        b = bytes.fromhex(m)
        df = b[0] >> 3
        if df in (11, 17, 18) or (df in (0, 4, 5, 16, 20, 21) and crc24(b) in addresses):
            out.append((b.ljust(14, b"\0"), p))
    return out


def clean(n, spc, frames):
    """A capture without noise: frames (message, position) at amplitude 1."""
    return synth(n, spc, [(m, p, 1.0, 0.0) for m, p in frames])


def same_score_starts(spc, p, msg=IDENT, tail=9):
    """Hand-made: only the LAST sample of every chip carries the frame, so the starts p .. p + spc - 1 slice the same message with bit-equal
    chip energies (0 + ... + 0 + x, the x further forward in the sum at every later start) -> (capture, p).  tail >= spc - 1: the last of
    them still fits the capture."""
    c = chips_of(msg)
    x = np.zeros(p + spc * len(c) + tail, np.complex64)
    x[p + spc - 1:p + spc - 1 + spc * len(c):spc] = c
    return x, p


def twin_starts(p=41, tail=9):
    """spc 2: only the SECOND sample of every chip carries the frame, so the starts p and p + 1 slice the same message with the same chip
    energies (x + 0 and 0 + x) -> (capture, p)."""
    return same_score_starts(2, p, IDENT, tail)


def overlaid(head_hex, address):
    """with_parity(head) with the address XORed into its last three bytes: a message whose remainder is the address."""
    b = bytearray(bytes.fromhex(with_parity(head_hex)))
    for k in range(3):
        b[len(b) - 3 + k] ^= (address >> (16 - 8 * k)) & 0xFF
    return bytes(b).hex().upper()


def every_format_capture():
    """spc 1, no noise: for each DF 0 .. 31 one frame with remainder zero and one with remainder ADDRESS (DF >= 16 long, the others short; the
    first byte DF << 3 | 5, the bytes behind it a pattern of the DF), odd gaps between them -> (capture, the positions the rules accept
    with the address list [ADDRESS]: remainder zero of DF 11, 17, 18, remainder ADDRESS of DF 0, 4, 5, 16, 20, 21, in that DF order)."""
    frames, accepted, pos = [], [], 7
    for df in range(32):
        head = bytes([df << 3 | 5] + [(37 * df + 11 * j + 3) & 0xFF for j in range(1, 11 if df >= 16 else 4)]).hex()
        for k, msg in enumerate((with_parity(head), overlaid(head, ADDRESS))):
            frames.append((msg, pos))
            if (k == 0 and df in (11, 17, 18)) or (k == 1 and df in (0, 4, 5, 16, 20, 21)):
                accepted.append(pos)
            pos += 16 + 8 * len(msg) + 31 + 2 * ((2 * df + k) % 7)      # the frame (len hex digits: 8 len chips of data), then an odd gap
    return clean(pos + 40, 1, frames), accepted


# ---- captures the CPU and the GPU tests share.  TILE restates DT_S of csrc/pss_adsb.hip (tests/launch_caps.py pins the line).
TILE = 4096


def dense_capture(spc):
    """Unit noise with three strong frames, near survivors 700, 2500 and TILE - 5 of the first detect tile when ratio is 0 (nearly every
    start survives then) -> complex64 [TILE + 240 spc + 600]."""
    n = TILE + 240 * spc + 600
    return synth(n, spc, [(IDENT, 700, 10.0, 0.2), (ALL_CALL, 2500, 10.0, 0.9), (VELOCITY, TILE - 5, 10.0, 1.7)], seed=[88, spc])


TWO_TILE_P = 5000
TWO_TILE_EXTRA = (1, 7, 8, 9, 15, 16)


def two_tile_window_capture():
    """spc 8, no noise: a long frame at TWO_TILE_P and a short one behind it.  A window that begins at TWO_TILE_P - 4066 - c and ends at
    TWO_TILE_P (or one later) evaluates TILE + c starts (15 either side): one whole tile and a last one of c starts."""
    p, spc = TWO_TILE_P, 8
    return clean(p + 240 * spc + 3000, spc, [(POS_EVEN, p), (ALL_CALL, p + 240 * spc + 100)])


def ending_capture(spc, msg):
    """A frame whose last sample is the capture's last, sample TILE + 4 -> (capture, the frame's position)."""
    span = spc * (16 + 8 * len(msg))                # len(msg) hex digits: 8 len chips of data
    p = TILE + 5 - span
    return clean(p + span, spc, [(msg, p)]), p


def windows_capture():
    """spc 2: the twin-start frame, then two noise-free frames back to back -> (capture, the places the window tests cut it at)."""
    x, p = twin_starts()
    q = len(x) + 3
    y = clean(q + 2 * (240 + 128) + 30, 2, [(POS_EVEN, q), (ALL_CALL, q + 480)])
    y[:len(x)] += x
    cuts = [p + 5, p + 1, q + 1, q + 2 * 60, q + 480 + 2 * 50]     # inside a preamble, between the twin starts, one past a start, inside data
    return y, sorted(cuts)


def reach(s_begin, s_end, spc, n_capture):
    """The samples [lo, hi) a window's call reads."""
    return max(0, s_begin - (2 * spc - 1)), min(n_capture, s_end + 2 * spc - 2 + 240 * spc)


def capture_crc32(iq):
    return zlib.crc32(np.ascontiguousarray(iq, np.complex64).tobytes())

"""Shared by tests/test_decode_batch_golden.py (CPU), tests/test_gpu_decode_batch.py and tools/make_goldens_decode.py: the recordings of
tests/golden/decode_batch.npz.

A case is one recording, cut into the read buffers of the decoder screens (0.5 s: int(fs * 0.5) samples), quantised to 16-bit ADC codes /
32768 as a radio delivers them.  The recordings are NOT stored in the fixture: codes() regenerates them from seeded NumPy, and `crc_<case>`
in the fixture pins their bytes.  Plain NumPy; no GPU import.

  morse_<wpm>   48 kS/s, a hard-keyed carrier 0.6 exp(0.05j n) with noise sigma = 0.004 sending MESSAGE at <wpm> words per minute: buffer
                boundaries cut pulses (a fall before the first rise, a last rise without a fall), some buffers hold only dots.
  aprs_<fs>     40 buffers: Bell-202 tones in the real part (bit 1 = 2200 Hz, one bit per int(fs / 1200) samples), noise in both parts
                (sigma = 0.01), one AX.25 frame with random information and a random lead-in per buffer.
"""
import zlib
from collections import namedtuple

import numpy as np

MESSAGE = "CQ CQ DE K1ABC K1ABC PSE K SOS 73"
MORSE_FS = 48000.0
THRESHOLD = -20
# the ITU symbols of MESSAGE's characters (a statement of the code, not of any table in the library)
ITU = {"A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "K": "-.-", "O": "---", "P": ".--.", "Q": "--.-", "S": "...",
       "1": ".----", "3": "...--", "7": "--..."}

Case = namedtuple("Case", "name kind fs n seed wpm n_frames")
CASES = (
    Case("morse_25", "morse", MORSE_FS, 24000, 501, 25, None),
    Case("morse_40", "morse", MORSE_FS, 24000, 502, 40, None),
    Case("morse_60", "morse", MORSE_FS, 24000, 503, 60, None),
    Case("aprs_48000", "aprs", 48000.0, 24000, 511, None, 40),
    Case("aprs_22050", "aprs", 22050.0, 11025, 512, None, 40),
    Case("aprs_9600", "aprs", 9600.0, 4800, 513, None, 40),
)
MORSE = tuple(c for c in CASES if c.kind == "morse")
APRS = tuple(c for c in CASES if c.kind == "aprs")


def case(name):
    return next(c for c in CASES if c.name == name)


def _quantise(z):
    """complex array -> int16 codes [n, 2]"""
    out = np.empty((len(z), 2), np.int16)
    out[:, 0] = np.clip(np.rint(z.real * 32768.0), -32768, 32767).astype(np.int16)
    out[:, 1] = np.clip(np.rint(z.imag * 32768.0), -32768, 32767).astype(np.int16)
    return out


def _morse(c, rng):
    unit = int(round(1.2 / c.wpm * c.fs))
    key = [0] * 2
    for wi, word in enumerate(MESSAGE.split(" ")):
        if wi:
            key += [0] * 4                       # 7 units between words (3 already follow the last letter)
        for ch in word:
            for sym in ITU[ch]:
                key += [1] * (1 if sym == "." else 3) + [0]
            key += [0] * 2
    k = np.repeat(np.array(key, float), unit)
    k = np.concatenate([np.zeros(unit // 3 + 7), k])     # the first element starts off the unit grid
    n = (len(k) // c.n + 1) * c.n                        # whole buffers; the last ends in silence
    k = np.concatenate([k, np.zeros(n - len(k))])
    return 0.6 * k * np.exp(0.05j * np.arange(n)) + 0.004 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def ax25_bits(dest, src, info):
    """flag + the stuffed bits of an AX.25 UI frame + flag; info: a sequence of byte values"""
    by = [(ord(ch) << 1) for ch in dest.ljust(6)] + [0x60] + [(ord(ch) << 1) for ch in src.ljust(6)] + [0x61, 0x03, 0xF0] + [int(b) for b in info]
    st, ones = [], 0
    for b in ((v >> j) & 1 for v in by for j in range(8)):
        st.append(b)
        ones = ones + 1 if b else 0
        if ones == 5:
            st.append(0)
            ones = 0
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    return flag + st + flag


def _aprs(c, rng):
    w = int(c.fs / 1200)
    rows = []
    for f in range(c.n_frames):
        info = rng.integers(32, 127, int(rng.integers(4, 20)))
        bits = [0] * int(rng.integers(0, 40)) + ax25_bits("APRS", "N%dCALL" % (f % 10), info)
        sym = np.repeat(np.array(bits), w)[:c.n]
        tone = np.where(np.concatenate([sym, np.zeros(c.n - len(sym))]) > 0, 2200.0, 1200.0)
        rows.append(0.8 * np.sin(2 * np.pi * np.cumsum(tone) / c.fs) + 0.01 * (rng.standard_normal(c.n) + 1j * rng.standard_normal(c.n)))
    return np.concatenate(rows)


_cache = {}


def codes(c):
    """int16 [n_frames * n, 2]: the case's recording as ADC codes (cached: the tests share one copy and leave it unchanged)."""
    if c.name not in _cache:
        rng = np.random.default_rng(c.seed)
        x = _quantise(_morse(c, rng) if c.kind == "morse" else _aprs(c, rng))
        x.setflags(write=False)
        _cache[c.name] = x
    return _cache[c.name]


def frames(c):
    """complex64 [n_frames][n]: the read buffers, codes / 32768"""
    key = c.name + "/frames"
    if key not in _cache:
        x = (codes(c).astype(np.float32) / np.float32(32768.0)).view(np.complex64).reshape(-1, c.n)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


def real_normalise_np(x):
    """The NumPy statement of pss_real_normalise for complex64 rows [.., n] (decoders.py:121-125; the row-wise division is float32)"""
    r = np.real(x)
    with np.errstate(all="ignore"):
        return (r / np.max(np.abs(r), axis=-1, keepdims=True)).astype(np.float64)

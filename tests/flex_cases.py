"""FLEX outside the library: a NumPy encoder (messages -> block information word, address, vector and message words -> phases -> interleaved
two- and four-level symbols -> discriminator rows or FSK IQ), and a NumPy statement of the receiver's rules (pyspecsdr_amd/csrc/pss_flex.h:
values, candidate, mode, FIW, one record, data, phases, check) that shares no code with the header: the BCH check is
tests/pocsag_cases.py's brute-force dictionary on the bit-reversed word.  The constants are the published air interface as multimon-ng's
demod_flex.c reads it, written from memory and not checked against a transmitter; the encoder and the receiver are written from the same
text.  tests/test_flex_golden.py holds the host twin to the statement record for record; tools/make_flex_golden.py writes
tests/golden/flex.npz from it."""
import zlib

import numpy as np

import pocsag_cases as P

RATE = 38400
MARKER = 0xA6C6AAAA
MODES = ((0x870C, 1600, 2), (0xB068, 1600, 4), (0x7B18, 3200, 2), (0xDEA0, 3200, 4), (0x4C7C, 3200, 4))   # code, baud, levels
FRAME_H = 5936                 # samples of a frame in units of h: 304 of sync and 2816 symbols 2 h apart
DATA_H = 304
N_SYM, N_WORDS = 2816, 88
TILE = 4096                    # k_flex_detect's tile (tests/flex_caps.py pins it through tests/launch_caps.py)
NUMERIC = "0123456789 U -]["
PHASES = "ABCD"
TWO_THIRDS = np.float32(0.6666667)


def brev32(v):
    return int("{:032b}".format(v & 0xFFFFFFFF)[::-1], 2)


def word(data21):
    """The FLEX word of 21 data bits: the POCSAG codeword of the reversed data, reversed."""
    return brev32(P.codeword(brev32(data21 & 0x1FFFFF) >> 11))


def check(w, fix):
    n, cw = P.check(brev32(w), fix)
    return (n, brev32(cw)) if n >= 0 else (-1, 0)


def nibble_sum(d):
    return ((d & 15) + (d >> 4 & 15) + (d >> 8 & 15) + (d >> 12 & 15) + (d >> 16 & 15) + (d >> 20 & 1)) & 15


def with_sum(d):
    """d with its low nibble chosen so that the nibble sum is 15."""
    d &= 0x1FFFF0
    return d | (15 - nibble_sum(d)) & 15


def active(mode):
    _, baud, levels = MODES[mode]
    return [p for p in range(4) if p == 0 or (p == 1 and levels == 4) or (p == 2 and baud == 3200) or (p == 3 and baud == 3200 and levels == 4)]


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------
def fiw_data(cycle, frame):
    return with_sum((cycle & 15) << 4 | (frame & 127) << 8)


def alpha_words(text, fragment=3, cont=0, signature=0x55):
    codes = ([signature] if fragment == 3 else []) + [ord(c) for c in text]
    codes += [3] * (-len(codes) % 3)
    return [fragment << 11 | cont << 10] + [codes[k] | codes[k + 1] << 7 | codes[k + 2] << 14 for k in range(0, len(codes), 3)]


def numeric_words(text):
    bits = [0] * 10 + [(NUMERIC.index(c) >> i) & 1 for c in text for i in range(4)]
    n_words = -(-len(bits) // 21)
    while len(bits) + 4 <= 21 * n_words:
        bits += [0, 0, 1, 1]                      # 0xC, a space
    bits += [0] * (21 * n_words - len(bits))
    return [sum(b << i for i, b in enumerate(bits[k:k + 21])) for k in range(0, len(bits), 21)]


def phase_data(messages, fill=0x0AAAAA):
    """[(capcode, kind, text)] with kind 'ALN', 'NUM', or an int (another vector type, no body), capcode an int (short) or a pair of raw data
    words (long: its vector takes two words as well) -> the 88 data values of a phase."""
    addr, bodies = [], []
    for capcode, kind, text in messages:
        addr.append([capcode + 0x8000] if isinstance(capcode, int) else list(capcode))
        bodies.append(alpha_words(text) if kind == "ALN" else numeric_words(text) if kind == "NUM" else [])
    n_addr = sum(len(a) for a in addr)
    first_vector = 1 + n_addr
    at = first_vector + n_addr
    d = [fill] * N_WORDS
    d[0] = with_sum(0 << 8 | first_vector << 10)
    k = 1
    for a, (capcode, kind, text), body in zip(addr, messages, bodies):
        v = first_vector + (k - 1)
        d[k:k + len(a)] = a
        if kind == "ALN":
            d[v] = with_sum(5 << 4 | at << 7 | len(body) << 14)
        elif kind == "NUM":
            d[v] = with_sum(3 << 4 | at << 7 | (len(body) - 1) << 14)
        else:
            d[v] = with_sum(int(kind) << 4)
        if len(a) == 2:
            d[v + 1] = fill
        d[at:at + len(body)] = body
        at += len(body)
        k += len(a)
    assert at <= N_WORDS and first_vector < 64
    return d


def frame_levels(mode, phases, cycle=3, frame=77, fiw=None, sync_word=None):
    """float64 [5936]: the level (+1, +1/3, -1/3, -1 of the outer deviation) of every slot of h samples.  phases: phase index -> 88 32-bit
    words (missing active phases: idle fill)."""
    code, baud, levels = MODES[mode]
    sync = (code << 48 | MARKER << 16 | (~code & 0xFFFF)) if sync_word is None else sync_word
    bits = [(sync >> (63 - k)) & 1 for k in range(64)] + [k & 1 for k in range(16)]
    w = word(fiw_data(cycle, frame)) if fiw is None else fiw
    bits += [(w >> k) & 1 for k in range(32)] + [k & 1 for k in range(40)]
    lv = np.zeros(FRAME_H)
    lv[:DATA_H] = np.repeat(np.where(np.array(bits) != 0, 1.0, -1.0), 2)
    idle = [word(0x0AAAAA)] * N_WORDS
    i = np.arange(N_SYM)
    at, bit = 8 * (i >> 8) + (i & 7), (i & 255) >> 3
    for p in range(2 if baud == 3200 else 1):
        wa = np.array(phases.get(2 * p, idle), np.uint64)
        wb = np.array(phases.get(2 * p + 1, idle), np.uint64)
        a = ((wa[at] >> bit.astype(np.uint64)) & np.uint64(1)).astype(int)
        b = ((wb[at] >> bit.astype(np.uint64)) & np.uint64(1)).astype(int)
        if levels == 4:
            sym = np.where(a == 1, np.where(b == 1, 1 / 3, 1.0), np.where(b == 1, -1 / 3, -1.0))
        else:
            sym = np.where(a == 1, 1.0, -1.0)
        if baud == 3200:
            lv[DATA_H + 2 * i + p] = sym
        else:
            lv[DATA_H + 2 * i] = sym
            lv[DATA_H + 2 * i + 1] = sym
    return lv


def frame_words(mode, per_phase):
    """{phase: [(capcode, kind, text)]} -> {phase: 88 words} for frame_levels."""
    return {p: [word(d) for d in phase_data(per_phase.get(p, []))] for p in active(mode)}


def direct_y(n, frames, h, hold=1, base=0.0, amp=1.0, inverted=False):
    """float32 [n]: every (levels, at) with its levels on the strobes at + h g, each held `hold` samples, `base` elsewhere."""
    y = np.full(n, base, np.float32)
    for lv, at in frames:
        v = (np.asarray(lv) * (-amp if inverted else amp)).astype(np.float32)
        for u in range(hold):
            idx = at + u + h * np.arange(len(v))
            ok = (idx >= 0) & (idx < n)
            y[idx[ok]] = v[ok]
    return y


def pulse_len(h):
    return h if h & 1 else max(h - 1, 1)


def fsk_iq(n, h, frames, offset_hz=0.0, inverted=False, dev_hz=4800.0):
    """complex128 [n] at 38 400 S/s (h = 12): every (levels, at) as FSK of dev_hz times its level around offset_hz, the carrier off outside
    the frames, no noise."""
    f, on = np.zeros(n), np.zeros(n)
    for lv, at in frames:
        v = np.repeat(np.asarray(lv), h) * (-1.0 if inverted else 1.0)
        lo, hi = max(at, 0), min(at + len(v), n)
        f[lo:hi] = offset_hz + dev_hz * v[lo - at:hi - at]
        on[lo:hi] = 1.0
    return on * np.exp(1j * np.cumsum(2 * np.pi * f / RATE))


def discriminate(x, h):
    """The polar discriminator in float64 and a boxcar of pulse_len(h) samples -> float32."""
    d = np.zeros(len(x))
    d[1:] = np.angle(x[1:] * np.conj(x[:-1]))
    p = pulse_len(h)
    return np.convolve(d, np.full(p, 1.0 / p), mode="same").astype(np.float32)


def fsk_row(n, h, frames, snr_db, offset_hz, seed, inverted=False):
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(10.0 ** (-snr_db / 10.0) / 2)
    x = fsk_iq(n, h, frames, offset_hz, inverted) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return discriminate(x, h)


def row_crc32(y):
    return zlib.crc32(np.ascontiguousarray(y).tobytes())


# ---- what formats.flex_messages reports --------------------------------------------------------------------------------------------------------
def expected(mode, per_phase):
    out = []
    for p in active(mode):
        for capcode, kind, text in per_phase.get(p, []):
            if kind == "ALN":
                out.append((PHASES[p], capcode, "ALN", text))
            elif kind == "NUM":
                out.append((PHASES[p], capcode, "NUM", text))
            else:
                out.append((PHASES[p], capcode if isinstance(capcode, int) else tuple(capcode), int(kind), None))
    return out


def reported(msgs):
    return [(m["phase"], m["capcode"] if not m["long"] else tuple(m["address"]), m["type"], m.get("text")) for m in msgs]


MESSAGES = {
    0: [(1234567, "ALN", "Hello, FLEX pager!"), (42, "NUM", "0123456789"), (99, 2, None)],
    1: [(500001, "ALN", "phase B rides on the inner levels"), (7, "NUM", "555-1234 U[12]")],
    2: [(1900000, "ALN", "phase C: the odd symbols at 3200 baud."), ((0x1F0000, 0x012345), 6, None), (31, "NUM", "42")],
    3: [(8, "NUM", "112 358 13"), (65536, "ALN", "D")],
}


# ---- the rules again --------------------------------------------------------------------------------------------------------------------------
def reach(s_begin, s_end, n, h):
    """The samples [lo, hi) of a row of n that a call for the starts [s_begin, s_end) must be given."""
    e0, e1 = max(0, s_begin - (2 * h - 1)), min(n, s_end + 2 * h - 1)
    return e0, min(n, e1 - 1 + FRAME_H * h)


def _pop(v):
    return bin(int(v)).count("1")


def numpy_frames(y, h, sync_errors=2, fix=2, max_bad=0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, stats=None):
    """Engine.h_flex_frames' result by NumPy: (words, fix, fiw, row, pos, meta, score, count)."""
    y = np.asarray(y, np.float32)
    rows = y[None, :] if y.ndim == 1 else y
    n_row = buf_index0 + rows.shape[1] if n_row is None else n_row
    s_end = n_row if s_end is None else s_end
    e0, e1 = max(0, s_begin - (2 * h - 1)), min(n_row, s_end + 2 * h - 1)
    f32 = np.float32
    out = []
    n_surv = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for r, yr in enumerate(rows):
            if s_begin >= s_end:
                continue
            acc = []
            for c0 in range(e0, e1, 1 << 16):
                s = np.arange(c0, min(e1, c0 + (1 << 16)), dtype=np.int64)
                s = s[s + FRAME_H * h <= n_row]
                if not len(s):
                    continue
                t = s[:, None] + 2 * h * np.arange(64)[None, :] - buf_index0
                v = yr[t] + yr[t + h]
                assert v.dtype == np.float32
                tot = np.zeros(len(s), f32)
                for k in range(64):
                    tot = tot + v[:, k]
                c = tot * f32(0.015625)
                bits = v > c[:, None]
                dsum = np.zeros(len(s), f32)
                for k in range(64):
                    dsum = dsum + np.abs(v[:, k] - c)
                a = dsum * f32(0.015625)
                assert c.dtype == np.float32 and a.dtype == np.float32
                wts = 1 << np.arange(15, -1, -1, dtype=np.int64)
                A = (bits[:, :16] * wts).sum(1)
                M = (bits[:, 16:32] * wts).sum(1) << 16 | (bits[:, 32:48] * wts).sum(1)
                C = (bits[:, 48:] * wts).sum(1)
                for i in range(len(s)):
                    m = _pop(int(M[i]) ^ MARKER)
                    inv = 32 - m <= sync_errors
                    mark = 32 - m if inv else m
                    Ai, Ci = (int(A[i]) ^ 0xFFFF, int(C[i]) ^ 0xFFFF) if inv else (int(A[i]), int(C[i]))
                    outer = _pop((Ai ^ ~Ci) & 0xFFFF)
                    if mark > sync_errors or outer > sync_errors:
                        continue
                    n_surv += 1
                    dists = [_pop(Ai ^ code) for code, _, _ in MODES]
                    dist = min(dists)
                    if dist > sync_errors:
                        continue
                    mode = dists.index(dist)
                    si = int(s[i])
                    tf = si + 2 * h * (80 + np.arange(32)) - buf_index0
                    fb = (yr[tf] + yr[tf + h]) > c[i]
                    w = sum(int(b) << k for k, b in enumerate(fb))
                    if inv:
                        w ^= 0xFFFFFFFF
                    nf, fiw = check(w, fix)
                    if nf < 0 or nibble_sum(fiw & 0x1FFFFF) != 15:
                        continue
                    acc.append(dict(s=si, e=mark + outer + dist + nf, a=a[i], c=c[i], mode=mode, inv=inv, fiw=fiw, mism=mark + outer + dist, nf=nf))
            for k in acc:
                if not s_begin <= k["s"] < s_end:
                    continue
                if any(0 < abs(b["s"] - k["s"]) < 2 * h and (b["e"] < k["e"] or (b["e"] == k["e"] and (b["a"] > k["a"] or (b["a"] == k["a"] and b["s"] < k["s"]))))
                       for b in acc):
                    continue
                _, baud, levels = MODES[k["mode"]]
                fast, four = baud == 3200, levels == 4
                centre = k["c"] * f32(0.5) if fast else k["c"]
                amp = k["a"] * f32(0.5) if fast else k["a"]
                T = TWO_THIRDS * amp
                lo, hi = centre - T, centre + T
                assert lo.dtype == np.float32 and hi.dtype == np.float32
                words = np.zeros((4, N_WORDS), np.uint32)
                fixes = np.zeros((4, N_WORDS), np.uint8)
                i = np.arange(N_SYM)
                at, bit = 8 * (i >> 8) + (i & 7), ((i & 255) >> 3).astype(np.uint32)
                for p in range(2 if fast else 1):
                    t = k["s"] + DATA_H * h + 2 * h * i + p * h - buf_index0
                    val = yr[t] if fast else yr[t] + yr[t + h]
                    ba = (val > centre) != k["inv"]
                    bb = (val > lo) & ~(val > hi)
                    np.bitwise_or.at(words[2 * p], at, ba.astype(np.uint32) << bit)
                    if four:
                        np.bitwise_or.at(words[2 * p + 1], at, bb.astype(np.uint32) << bit)
                n_bad = n_fixed = 0
                for p in active(k["mode"]):
                    for j in range(N_WORDS):
                        nf, cw = check(int(words[p, j]), fix)
                        words[p, j] = cw
                        fixes[p, j] = 255 if nf < 0 else nf
                        n_bad += nf < 0
                        n_fixed += max(nf, 0)
                for p in range(4):
                    if p not in active(k["mode"]):
                        words[p] = 0
                if n_bad > max_bad:
                    continue
                meta = (k["mism"] | int(k["inv"]) << 8 | k["mode"] << 12 | k["nf"] << 16, n_bad | n_fixed << 16)
                out.append((words, fixes, k["fiw"], r, k["s"], meta, k["a"]))
    if stats is not None:
        stats["survivors"] = n_surv
    count = len(out)
    k = count if max_frames is None else min(count, max(max_frames, 0))
    out = out[:k]
    return (np.array([o[0] for o in out], np.uint32).reshape(k, 4, N_WORDS), np.array([o[1] for o in out], np.uint8).reshape(k, 4, N_WORDS),
            np.array([o[2] for o in out], np.uint32), np.array([o[3] for o in out], np.int32), np.array([o[4] for o in out], np.int64),
            np.array([o[5] for o in out], np.uint32).reshape(k, 2), np.array([o[6] for o in out], np.float32), count)


# ---- hand-made rows ----------------------------------------------------------------------------------------------------------------------------
def frame_row(mode, h, at, n, hold=1, inverted=False, amp=1.0, base=0.0, per_phase=None, **kw):
    """direct_y of one frame of MESSAGES (or per_phase) whose first strobe is at `at`."""
    lv = frame_levels(mode, frame_words(mode, MESSAGES if per_phase is None else per_phase), **kw)
    return direct_y(n, [(lv, at)], h, hold=hold, inverted=inverted, amp=amp, base=base)


def stub_levels(mode=0, cycle=0, frame=0):
    """The first 112 bit times of a frame: sync 1, dotting and FIW; 224 slots."""
    return frame_levels(mode, {}, cycle=cycle, frame=frame)[:224]


def stub_train(n_stubs, h=1, mode=0, tail=True):
    """Back-to-back sync + FIW stubs 224 h apart, every level held h samples, on a row long enough that every stub is a candidate: with
    max_bad = 352 each is an accepted frame.  -> (row, the starts that stay)."""
    lv = np.concatenate([stub_levels(mode, frame=k & 127) for k in range(n_stubs)])
    n = 3 + h * len(lv) + (FRAME_H * h if tail else 0)
    return direct_y(n, [(lv, 3)], h, hold=h), [3 + 224 * h * k for k in range(n_stubs)]


# ---- the fixture rows: name -> (mode, h, seed, inverted, snr_db or None for a direct row)
CASES = {
    "m0": (0, 2, 31, False, None),
    "m1": (1, 2, 32, False, None),
    "m2": (2, 2, 33, False, None),
    "m3": (3, 2, 34, False, None),
    "m3inv": (3, 1, 35, True, None),
    "m1noise": (1, 12, 36, False, 25.0),
}
LEAD = 40


def case_row(name):
    mode, h, seed, inverted, snr = CASES[name]
    lv = frame_levels(mode, frame_words(mode, MESSAGES), cycle=seed & 15, frame=seed)
    n = LEAD + FRAME_H * h + 30
    if snr is None:
        rng = np.random.default_rng(seed)
        y = direct_y(n, [(lv, LEAD)], h, hold=h, inverted=inverted)
        return (y + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return fsk_row(n, h, [(lv, LEAD)], snr, 700.0, seed, inverted=inverted)


# ---- end to end: two channels in a 240 kS/s capture (tests/test_gpu_flex.py through formats.flex_recording, tests/test_flex_golden.py
#      through the host twins of the same stages and the NumPy statement)
CHANNELS = ((-50e3, 0, False, {0: [(1234567, "ALN", "Hello from the first channel"), (2000, "NUM", "0123456789")]}),
            (50e3, 3, True, {0: [(77001, "ALN", "four levels, inverted")], 1: [(5, "NUM", "42")], 2: [(654321, "ALN", "phase C")],
                             3: [(9, "NUM", "311 U[7]-2"), (70000, "ALN", "and D")]}))
CAPTURE_FS, CAPTURE_SNR_DB, CAPTURE_H = 240e3, 25.0, 12


def capture(fs=CAPTURE_FS, seed=5, snr_db=CAPTURE_SNR_DB):
    """The channels at their offsets, snr_db in the 38.4 kHz band -> complex64 at fs centred between them."""
    n38 = 400 + FRAME_H * CAPTURE_H + 1200
    n38 += -n38 % 4
    n = n38 * int(fs) // RATE
    assert n * RATE == n38 * int(fs)
    t = np.arange(n) / fs
    x = np.zeros(n, np.complex128)
    for off, mode, inverted, per_phase in CHANNELS:
        lv = frame_levels(mode, frame_words(mode, per_phase), cycle=7, frame=100)
        b = fsk_iq(n38, CAPTURE_H, [(lv, 400)], offset_hz=300.0, inverted=inverted)
        spec = np.fft.fft(b)
        wide = np.zeros(n, np.complex128)
        wide[:n38 // 2], wide[-(n38 // 2):] = spec[:n38 // 2], spec[-(n38 // 2):]
        x += np.fft.ifft(wide) * (n / n38) * np.exp(2j * np.pi * off * t)
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(10.0 ** (-snr_db / 10.0) / 2 * fs / RATE)
    x += sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def capture_lines():
    """What formats.flex_lines reports of the capture, in order of (row, phase, address word)."""
    out = []
    for off, mode, inverted, per_phase in CHANNELS:
        _, baud, levels = MODES[mode]
        for phase, capcode, kind, text in expected(mode, per_phase):
            out.append(f"FLEX: {baud}/{levels}/{phase} 07.100 [{capcode:09d}] {kind} {text}")
    return out

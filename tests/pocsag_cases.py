"""POCSAG outside the library: a NumPy encoder (preamble, batches, frame placement by ric & 7, idle fill, numeric and alpha packing, BCH(31,21)
by polynomial division), a NumPy FSK synthesiser with its own discriminator and boxcar, and a NumPy statement of the receiver's rules
(pyspecsdr_amd/csrc/pss_pocsag.h: candidate, walk, check, accept, one record) that shares no code with the header: the error patterns are
found by brute force over a dictionary built here.  tests/test_pocsag_golden.py holds the host twin to it record for record;
tools/make_pocsag_golden.py writes tests/golden/pocsag.npz from it."""
import zlib

import numpy as np

RATE = 38400
SYNC, IDLE = 0x7CD215D8, 0x7A89C197
GEN = 0x769                    # x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
PREAMBLE = 576
LAST_K = 543                   # 32 sync strobes and 16 codewords of 32
TILE = 4096                    # k_pocsag_detect's tile (tests/pocsag_caps.py pins it through tests/launch_caps.py)
NUMERIC = "0123456789*U -)("
SPB = {512: 75, 1200: 32, 2400: 16}


# ---- the code -----------------------------------------------------------------------------------------------------------------------------
def remainder31(v):
    for i in range(30, 9, -1):
        if (v >> i) & 1:
            v ^= GEN << (i - 10)
    return v & 0x3FF


def codeword(data21):
    cw = (data21 & 0x1FFFFF) << 11
    cw |= remainder31(cw >> 1) << 1
    return cw | (bin(cw).count("1") & 1)


def _patterns():
    table = {}
    for i in range(1, 32):
        table.setdefault(remainder31((1 << i) >> 1), []).append(1 << i)
    for i in range(1, 32):
        for j in range(i + 1, 32):
            e = (1 << i) | (1 << j)
            table.setdefault(remainder31(e >> 1), []).append(e)
    return table


PATTERNS = _patterns()
assert len(PATTERNS) == 31 + 465 and all(len(v) == 1 for v in PATTERNS.values()) and 0 not in PATTERNS


def check(cw, fix):
    """-> (bits fixed, corrected codeword), or (-1, 0)."""
    s, p = remainder31(cw >> 1), bin(cw).count("1") & 1
    if s == 0:
        n, e = p, p
    else:
        if s not in PATTERNS:
            return -1, 0
        e = PATTERNS[s][0]
        w = bin(e).count("1")
        n = w if p == (w & 1) else w + 1
        if n > w:
            e |= 1
    return (n, cw ^ e) if n <= fix else (-1, 0)


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------
def address_word(ric, function):
    return codeword((ric >> 3) << 2 | (function & 3))


def data_words(bits):
    """The message's bit stream, padded with zeros to whole codewords -> the data codewords."""
    bits = list(bits) + [0] * (-len(bits) % 20)
    return [codeword(1 << 20 | int("".join(map(str, bits[k:k + 20])), 2)) for k in range(0, len(bits), 20)]


def numeric_bits(text):
    text = text + " " * (-len(text) % 5)
    return [(NUMERIC.index(c) >> i) & 1 for c in text for i in range(4)]


def alpha_bits(text):
    return [(ord(c) >> i) & 1 for c in text for i in range(7)]


def message_words(ric, function, text):
    """function 0 carries digits, the others text; text None: the address alone."""
    words = [address_word(ric, function)]
    if text is not None:
        words += data_words(numeric_bits(text) if function == 0 else alpha_bits(text))
    return words


def batches_of(messages):
    """[(ric, function, text)] -> the batches, 16 codewords each: every address word in its frame ric & 7, idle words elsewhere."""
    slots = []
    for ric, function, text in messages:
        while (len(slots) % 16) // 2 != ric & 7:
            slots.append(IDLE)
        slots += message_words(ric, function, text)
    slots.append(IDLE)                                  # the last message is closed by an idle word
    slots += [IDLE] * (-len(slots) % 16)
    return [slots[k:k + 16] for k in range(0, len(slots), 16)]


def word_bits(w):
    return [(w >> (31 - k)) & 1 for k in range(32)]


def batch_bits(words):
    return [b for w in [SYNC] + list(words) for b in word_bits(w)]


def transmission_bits(messages, preamble=PREAMBLE):
    bits = [1 - (k & 1) for k in range(preamble)]
    for words in batches_of(messages):
        bits += batch_bits(words)
    return bits


def expected(messages, baud):
    """What formats.pocsag_messages reports of each injected message: (ric, function, text, bits)."""
    out = []
    for ric, function, text in messages:
        if text is None:
            out.append((ric, function, "", 0))
        elif function == 0:
            t = text + " " * (-len(text) % 5)
            out.append((ric, function, t, 4 * len(t)))
        else:
            out.append((ric, function, text, 20 * -(-7 * len(text) // 20)))
    return out


def reported(msgs):
    return [(m["ric"], m["function"], m["numeric"] if m["function"] == 0 else m["alpha"], m["bits"]) for m in msgs]


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------
def direct_y(n, bursts, spb, hold=1, base=0.0, amp=1.0, inverted=False):
    """float32 [n]: every (bits, at) with its levels (a 0 is +amp, the higher frequency; a 1 is -amp) on the strobes at + spb k, each held
    `hold` samples, `base` elsewhere."""
    y = np.full(n, base, np.float32)
    for bits, at in bursts:
        lv = np.where(np.asarray(bits) != 0, -amp, amp).astype(np.float32)
        if inverted:
            lv = -lv
        for h in range(hold):
            idx = at + h + spb * np.arange(len(lv))
            ok = (idx >= 0) & (idx < n)
            y[idx[ok]] = lv[ok]
    return y


def pulse_len(spb):
    m = min(spb, 65)
    return m if m & 1 else m - 1


def fsk_row(n, spb, bursts, snr_db, offset_hz, seed, inverted=False, dev_hz=4500.0):
    """float32 [n] at 38 400 S/s: every (bits, at) as 2-FSK of +-dev_hz around offset_hz (a 0 the higher frequency), the carrier off outside
    the transmissions, on seeded complex Gaussian noise snr_db below an amplitude of 1; then the polar discriminator in float64 and a
    boxcar of pulse_len(spb) samples."""
    f = np.zeros(n)
    on = np.zeros(n)
    for bits, at in bursts:
        lv = np.repeat(np.where(np.asarray(bits) != 0, -1.0, 1.0), spb)
        if inverted:
            lv = -lv
        lo, hi = max(at, 0), min(at + len(lv), n)
        f[lo:hi] = offset_hz + dev_hz * lv[lo - at:hi - at]
        on[lo:hi] = 1.0
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(10.0 ** (-snr_db / 10.0) / 2)
    x = on * np.exp(1j * np.cumsum(2 * np.pi * f / RATE)) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    d = np.zeros(n)
    d[1:] = np.angle(x[1:] * np.conj(x[:-1]))
    P = pulse_len(spb)
    return np.convolve(d, np.full(P, 1.0 / P), mode="same").astype(np.float32)


def fsk_iq(n, spb, bits, at, offset_hz=0.0, inverted=False, dev_hz=4500.0):
    """complex128 [n] at 38 400 S/s: the transmission alone, its carrier off outside it, no noise."""
    lv = np.repeat(np.where(np.asarray(bits) != 0, -1.0, 1.0), spb)
    if inverted:
        lv = -lv
    f, on = np.zeros(n), np.zeros(n)
    f[at:at + len(lv)] = offset_hz + dev_hz * lv[:n - at]
    on[at:at + len(lv)] = 1.0
    return on * np.exp(1j * np.cumsum(2 * np.pi * f / RATE))


# hand-made rows: a sync word and 16 codewords with their levels on the strobes
WORDS = [address_word(1234567, 3) if j == 14 else IDLE if j in (3, 9) else codeword(1 << 20 | (0x13579 * (j + 1)) & 0xFFFFF) for j in range(16)]


def batch_row(spb, at, n, words=None, hold=1, inverted=False, flips=(), amp=1.0, base=0.0):
    """direct_y of one batch whose first strobe is at `at`; flips: the strobes (0 .. 543) whose bit is wrong."""
    bits = batch_bits(WORDS if words is None else words)
    for k in flips:
        bits[k] ^= 1
    return direct_y(n, [(bits, at)], spb, hold=hold, inverted=inverted, amp=amp, base=base)


def row_crc32(y):
    return zlib.crc32(np.ascontiguousarray(y).tobytes())


# ---- the fixture rows: name -> (baud, seed, inverted, [(ric, function, text)]); 15 dB in the 38.4 kHz row, 1.5 kHz off
CASES = {
    "p2400": (2400, 21, True, [(1234567, 3, "POCSAG at 2400 bit/s on an inverted channel: the quick brown fox jumps over the lazy dog 0123456789"),
                               (800001, 0, "0123456789"), (42, 1, None), (2007, 2, "second batch"),
                               (1048570, 3, "a message long enough to run across the sync word of the next batch, and the one after it as well.")]),
    "p1200": (1200, 22, False, [(1234567, 3, "Hello, pager!"), (7, 0, "112*U -)(8"), (65536, 1, "x"), (2097151, 2, None),
                                (555000, 3, "the fourth and fifth batches carry this text, frame placement by the address's low three bits."),
                                (123, 0, "999")]),
    "p512": (512, 23, False, [(1234560, 3, "512 bit/s: seventy-five samples a bit."), (99, 0, "5551234"),
                              (77777, 3, "three more batches of text at the slow rate, to reach six in this row of the fixture..")]),
}
SNR_DB, OFFSET_HZ, LEAD = 15.0, 1500.0, 700


def case_row(name):
    baud, seed, inverted, messages = CASES[name]
    spb = SPB[baud]
    bits = transmission_bits(messages)
    n = LEAD + spb * len(bits) + 900
    return fsk_row(n, spb, [(bits, LEAD)], SNR_DB, OFFSET_HZ, seed, inverted=inverted)


def case_batches(name):
    """(number of batches, the row index of the first sync word's first strobe: the middle of its first bit)."""
    baud, _, _, messages = CASES[name]
    spb = SPB[baud]
    return len(batches_of(messages)), LEAD + spb * PREAMBLE + spb // 2


# ---- the rules again --------------------------------------------------------------------------------------------------------------------------
def reach(s_begin, s_end, n, spb):
    """The samples [lo, hi) of a row of n that a call for the starts [s_begin, s_end) must be given."""
    e0, e1 = max(0, s_begin - (spb - 1)), min(n, s_end + spb - 1)
    return e0, min(n, e1 - 1 + LAST_K * spb + 1)


def _popcount(v):
    v = v.astype(np.uint64)
    c = np.zeros(v.shape, np.int64)
    for k in range(32):
        c += ((v >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
    return c


def numpy_batches(y, spb, sync_errors=2, fix=2, max_bad=0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_batches=None, stats=None):
    """Engine.h_pocsag_batches' result by NumPy: (cw, fix, row, pos, meta, score, count)."""
    y = np.asarray(y, np.float32)
    rows = y[None, :] if y.ndim == 1 else y
    n_row = buf_index0 + rows.shape[1] if n_row is None else n_row
    s_end = n_row if s_end is None else s_end
    e0, e1 = max(0, s_begin - (spb - 1)), min(n_row, s_end + spb - 1)
    out = []
    n_surv = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for r, yr in enumerate(rows):
            s = np.arange(e0, e1, dtype=np.int64)
            s = s[s + LAST_K * spb < n_row]
            if not len(s) or s_begin >= s_end:
                continue
            v = yr[s[:, None] + spb * np.arange(32)[None, :] - buf_index0]
            t = v[:, 0].copy()
            for k in range(1, 32):
                t = t + v[:, k]
            thr = t * np.float32(0.03125)
            assert thr.dtype == np.float32
            data = ~(v > thr[:, None])
            word = np.zeros(len(s), np.int64)
            for k in range(32):
                word |= data[:, k].astype(np.int64) << (31 - k)
            e = _popcount(word ^ SYNC)
            mism = np.minimum(e, 32 - e)
            q = np.abs(v[:, 0] - thr)
            for k in range(32):
                a = np.abs(v[:, k] - thr)
                q = np.where(a < q, a, q)
            acc = []
            for i in np.nonzero(mism <= sync_errors)[0]:
                n_surv += 1
                inv = bool(32 - e[i] < e[i])
                lv = yr[s[i] + spb * np.arange(32, 544) - buf_index0] > thr[i]
                cws, fixes = [], []
                for j in range(16):
                    w = 0
                    for k in range(32):
                        w |= int(not lv[32 * j + k]) << (31 - k)
                    if inv:
                        w ^= 0xFFFFFFFF
                    nf, c = check(w, fix)
                    cws.append(c)
                    fixes.append(255 if nf < 0 else nf)
                n_bad = sum(f == 255 for f in fixes)
                if n_bad <= max_bad:
                    meta = int(mism[i]) | int(inv) << 8 | n_bad << 16 | sum(f for f in fixes if f != 255) << 24
                    acc.append((int(s[i]), q[i], cws, fixes, meta))
            for a in acc:
                if not s_begin <= a[0] < s_end:
                    continue
                if any(b[2] == a[2] and 0 < abs(b[0] - a[0]) < spb and (b[1] > a[1] or (b[1] == a[1] and b[0] < a[0])) for b in acc):
                    continue
                out.append((r,) + a)
    if stats is not None:
        stats["survivors"] = n_surv
    count = len(out)
    k = count if max_batches is None else min(count, max(max_batches, 0))
    out = out[:k]
    return (np.array([o[3] for o in out], np.uint32).reshape(k, 16), np.array([o[4] for o in out], np.uint8).reshape(k, 16),
            np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int64), np.array([o[5] for o in out], np.uint32),
            np.array([o[2] for o in out], np.float32), count)


# ---- the shapes tests/test_gpu_pocsag.py, tests/test_gpu_start_list.py and tests/test_pocsag_shapes.py share (the caps are the callers': tests/pocsag_caps.py) ----
SHORT_SPB = 2
SHORT_N = 60 + LAST_K * SHORT_SPB + 1      # a row of one tile: 61 starts


def sync_train(n_words, hold=2):
    """Back-to-back sync words at 2 samples a bit: each is a sync word followed by 16 codewords (the sync word is one), so with hold = 2
    two starts survive per 64 samples and both are accepted with the same words; the earlier stays."""
    bits = word_bits(SYNC) * n_words
    n = 2 * len(bits) + 7
    return direct_y(n, [(bits, 3)], 2, hold=hold), [3 + 64 * k for k in range(n_words - 16)]


def carrying(n_rows, grid_cap):
    """The rows of a batch of one-tile rows that carry a record: those of every other round of a detect grid of grid_cap workgroups, and
    the last.  A workgroup then meets tiles with, without, with, without survivors, and workgroup 0 a fifth that has them."""
    return [r for r in range(n_rows) if (r // grid_cap) % 2 == 0 or r == n_rows - 1]


def short_start(r):
    return (5 * r) % 60


def short_rows(n_rows, grid_cap, dense=False):
    """float32 [n_rows][1147] at 2 samples a bit, one tile a row.  Plain: a batch at (5 r) % 60 in the carrying rows, zeros elsewhere.
    dense: a batch with every level held both samples in EVERY row: two survivors a row, the earlier stays."""
    y = np.zeros((n_rows, SHORT_N), np.float32)
    for r in (range(n_rows) if dense else carrying(n_rows, grid_cap)):
        y[r] = batch_row(SHORT_SPB, short_start(r), SHORT_N, hold=SHORT_SPB if dense else 1)
    return y


def round_sample(n_rows, grid_cap):
    """The rows a CPU test restates: the first, the last, and the first, a middle and the last row of every round of the detect grid."""
    rows = {0, n_rows - 1}
    for r0 in range(0, n_rows, grid_cap):
        r1 = min(r0 + grid_cap, n_rows)
        rows |= {r0, (r0 + r1) // 2, r1 - 1}
    return sorted(rows)

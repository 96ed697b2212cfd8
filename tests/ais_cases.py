"""AIS test rows and an independent statement of the receiver's rules, NumPy only and no library code.

    message fields -> bits (most significant first) -> bytes -> CRC-16/X.25 -> bits, each byte's least significant first -> a zero stuffed
    in behind every five ones -> 24 training bits + flag + frame + flag -> NRZI (a 0 changes the level) -> either levels at the strobes
    (direct_y: a row the frame search reads without a front) or GMSK (synth: Gaussian BT 0.4 over 5 samples a bit, modulation index 0.5,
    amplitude, carrier offset and seeded complex noise -> complex64 at 48 000 S/s).

numpy_frames restates the candidate, walk, check and one-record rules of PARITY.md "AIS": the flag test vectorised in float32, the walk
on Python lists.  tools/make_goldens_ais.py stores the twin's records of every fixture capture in tests/golden/ais.npz, with a CRC-32
of each capture; the captures are regenerated here.
"""
import zlib

import numpy as np

RATE = 48000
SPB = 5
BACK, HEAD = 45, 35
LAST_K = 1244                  # 8 + 1030 appended + 205 dropped + 2 closing - 1
REACH = SPB * LAST_K + 1       # 6221
TRAINING = 24
FLAG = (0, 1, 1, 1, 1, 1, 1, 0)
TILE = 4096                    # k_ais_detect's tile, FRONT_TILE k_ais_front's (tests/ais_caps.py pins them, the first through tests/launch_caps.py)
FRONT_TILE = 2048

# the published position report: type 1, MMSI 477553000, under way ... longitude -122.345833, latitude 47.582833
VECTOR_PAYLOAD = "177KQJ5000G?tO`K>RA1wUbN0TKH"
VECTOR_SENTENCE = "!AIVDM,1,1,,B,177KQJ5000G?tO`K>RA1wUbN0TKH,0*5C"


def crc16(data):
    """CRC-16/X.25 of a byte string, byte by byte: reflected 0x8408, init 0xFFFF, final complement."""
    r = 0xFFFF
    for byte in bytes(data):
        r ^= byte
        for _ in range(8):
            r = (r >> 1) ^ 0x8408 if r & 1 else r >> 1
    return r ^ 0xFFFF


def pack(fields):
    """[(value, width), ...] most significant first -> bytes (the total width a multiple of 8); a negative value in two's complement."""
    word, n = 0, 0
    for v, w in fields:
        word = (word << w) | (int(v) & ((1 << w) - 1))
        n += w
    assert n % 8 == 0
    return word.to_bytes(n // 8, "big")


def sixbit(text, n_chars):
    """Text in the 6-bit table, padded with '@' -> [(value, 6)] * n_chars."""
    t = text.upper().ljust(n_chars, "@")[:n_chars]
    return [((ord(c) - 64) if ord(c) >= 64 else ord(c), 6) for c in t]


def armour_to_bytes(payload):
    bits = []
    for ch in payload:
        v = ord(ch) - 48
        v = v - 8 if v > 40 else v
        bits += [(v >> (5 - k)) & 1 for k in range(6)]
    return np.packbits(np.array(bits[:len(bits) // 8 * 8], np.uint8)).tobytes()


VECTOR = armour_to_bytes(VECTOR_PAYLOAD)


def type1(mmsi, lon, lat, status=0, turn=0, speed=0, course=0, heading=511, second=60, kind=1):
    """A class A position report from its fields: lon / lat in degrees, speed in knots, course in degrees."""
    return pack([(kind, 6), (0, 2), (mmsi, 30), (status, 4), (turn, 8), (round(speed * 10), 10), (0, 1), (round(lon * 600000), 28),
                 (round(lat * 600000), 27), (round(course * 10), 12), (heading, 9), (second, 6), (0, 2), (0, 3), (0, 1), (0, 19)])


def type5(mmsi, imo, callsign, name, ship_type, dims, eta, draught, destination):
    return pack([(5, 6), (0, 2), (mmsi, 30), (0, 2), (imo, 30)] + sixbit(callsign, 7) + sixbit(name, 20) + [(ship_type, 8), (dims[0], 9), (dims[1], 9),
                (dims[2], 6), (dims[3], 6), (1, 4), (eta[0], 4), (eta[1], 5), (eta[2], 5), (eta[3], 6), (round(draught * 10), 8)]
                + sixbit(destination, 20) + [(0, 1), (0, 1)])


def type18(mmsi, lon, lat, speed=0, course=0, heading=511, second=60):
    return pack([(18, 6), (0, 2), (mmsi, 30), (0, 8), (round(speed * 10), 10), (0, 1), (round(lon * 600000), 28), (round(lat * 600000), 27),
                 (round(course * 10), 12), (heading, 9), (second, 6), (0, 2), (1, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 20)])


def type24a(mmsi, name):
    return pack([(24, 6), (0, 2), (mmsi, 30), (0, 2)] + sixbit(name, 20))


def with_crc(body):
    """The frame's bytes: the message and its check bytes, low byte first."""
    return bytes(body) + crc16(body).to_bytes(2, "little")


def wire_bits(frame_bytes):
    """The bytes of a frame in the order sent: each byte's least significant bit first."""
    return np.unpackbits(np.frombuffer(bytes(frame_bytes), np.uint8), bitorder="little").tolist()


def stuff(bits):
    out, run = [], 0
    for b in bits:
        out.append(b)
        run = run + 1 if b else 0
        if run == 5:
            out.append(0)
            run = 0
    return out


def burst_bits(frame_bytes, stuffed=None):
    """Training, flag, the stuffed frame (stuffed: the bits between the flags, given outright), flag -> a list of data bits."""
    mid = stuff(wire_bits(frame_bytes)) if stuffed is None else list(stuffed)
    return [k & 1 for k in range(TRAINING)] + list(FLAG) + mid + list(FLAG)


def nrzi(bits, level=1.0):
    out = []
    for b in bits:
        level = level if b else -level
        out.append(level)
    return np.array(out)


def flag_start(at):
    """The start s of a burst whose first training bit's strobe lies at sample `at`."""
    return at + SPB * TRAINING


def direct_y(n, bursts, hold=1, base=0.0):
    """A float32 row of n samples: `base` everywhere, and for every (bits, at[, amp[, dc]]) the NRZI levels amp * (+-1) + dc on the `hold`
    samples from each bit's strobe on, the first bit's strobe at `at`.  Samples past the row are cut."""
    y = np.full(n, base, np.float32)
    for bits, at, *rest in bursts:
        amp = rest[0] if rest else 1.0
        dc = rest[1] if len(rest) > 1 else 0.0
        lv = nrzi(bits) * amp + dc
        for h in range(hold):
            idx = at + h + SPB * np.arange(len(lv))
            ok = (idx >= 0) & (idx < n)
            y[idx[ok]] = lv[ok]
    return y


def gaussian(bt=0.4, span_bits=4):
    t = np.arange(-SPB * span_bits // 2, SPB * span_bits // 2 + 1) / SPB
    h = np.exp(-(2 * np.pi ** 2 / np.log(2)) * bt ** 2 * t ** 2)
    return h / h.sum()


def synth(n, bursts, snr_db=None, seed=0):
    """complex64 [n] at 48 000 S/s: every (frame_bytes, at, amp, offset_hz) as a GMSK burst whose first training bit starts at sample
    `at`, on seeded complex Gaussian noise snr_db below an amplitude of 1 (None: no noise)."""
    x = np.zeros(n, np.complex128)
    h = gaussian()
    for frame, at, amp, off in bursts:
        lv = np.repeat(nrzi(burst_bits(frame)), SPB)
        f = np.convolve(np.concatenate([np.zeros(SPB), lv, np.zeros(SPB)]), h, mode="same")
        ph = np.cumsum(f) * (np.pi / 2 / SPB)
        k = np.arange(len(ph))
        sig = amp * np.exp(1j * (ph + 2 * np.pi * off * (k + at) / RATE))
        a = at - SPB
        lo, hi = max(a, 0), min(a + len(sig), n)
        x[lo:hi] += sig[lo - a:hi - a]
    if snr_db is not None:
        rng = np.random.default_rng(seed)
        sigma = np.sqrt(10.0 ** (-snr_db / 10.0) / 2)
        x += sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def capture_crc32(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


# ---- the fixture captures: name -> (n, seed, snr_db, [(message, at, amp, offset_hz)])
SHIPS = [
    type1(477553000, -122.345833, 47.582833, status=5, course=51.0, heading=181, second=15),
    type1(366998410, -122.4001, 47.6502, speed=12.3, course=180.5, heading=181, second=30, kind=3),
    type18(338123456, 4.2501, 51.9502, speed=6.1, course=271.0, second=7),
    type5(244660000, 9074729, "PBQR", "NOORDZEE", 70, (100, 20, 8, 7), (5, 17, 6, 30), 6.4, "ROTTERDAM"),
    type24a(338123456, "SEA BREEZE"),
]
CASES = {
    "quiet": (48000, 11, 20.0, [(SHIPS[0], 2000, 1.0, 0.0), (SHIPS[1], 9000, 1.0, 0.0), (SHIPS[3], 20000, 1.0, 0.0), (SHIPS[2], 40000, 1.0, 0.0)]),
    "plus500": (48000, 12, 15.0, [(SHIPS[0], 1500, 1.0, 500.0), (SHIPS[4], 8000, 0.7, 500.0), (SHIPS[3], 15000, 1.0, 500.0), (SHIPS[1], 30000, 1.3, 500.0)]),
    "minus500": (40000, 13, 15.0, [(SHIPS[2], 100, 1.0, -500.0), (SHIPS[1], 12000, 1.0, -500.0), (SHIPS[0], 38000, 1.0, -500.0)]),
}


def case_iq(name):
    n, seed, snr, bursts = CASES[name]
    return synth(n, [(with_crc(m), at, amp, off) for m, at, amp, off in bursts], snr_db=snr, seed=seed)


def many_bursts(count, snr_db, offset_hz, seed, gap=2000):
    """count distinct type 1 reports, one every `gap` samples -> (complex64 row, the frames' bytes)."""
    msgs = [with_crc(type1(200000000 + 1000 * seed + i, -5.0 + 0.01 * i, 50.0 + 0.01 * i, speed=i, course=3.0 * i, second=i % 60)) for i in range(count)]
    x = synth(gap * count + 500, [(m, 300 + gap * i, 1.0, offset_hz) for i, m in enumerate(msgs)], snr_db=snr_db, seed=seed)
    return x, msgs


# ---- the rules again -------------------------------------------------------------------------------------------------------------------------
def reach(s_begin, s_end, n):
    """The samples [lo, hi) a window's starts and their possible suppressors read."""
    e0, e1 = max(0, s_begin - 4), min(n, s_end + 4)
    return max(0, e0 - BACK), min(n, e1 - 1 + REACH)


def _walk(levels_after, level7):
    """levels_after: the levels at k = 8, 9, ... to the row's end -> the payload's bit list, or None."""
    bits, prev = [], level7
    for lv in levels_after:
        bits.append(1 if lv == prev else 0)
        prev = lv
    out, run, i = [], 0, 0
    while True:
        if i >= len(bits):
            return None
        b = bits[i]
        i += 1
        if run == 5:
            if b == 0:
                run = 0
                continue
            if i >= len(bits) or bits[i] == 1:
                return None
            break
        if len(out) == 1030:
            return None
        out.append(b)
        run = run + 1 if b else 0
    return out[:-6] if len(out) >= 6 else None


def numpy_frames(y, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, stats=None):
    """y float32 [n_rows][n_buf] or [n_buf] -> (msg uint8 [k][128], len int32, row int32, pos int64, score float32, count)."""
    rows = np.asarray(y, np.float32)
    rows = rows[None, :] if rows.ndim == 1 else rows
    n = buf_index0 + rows.shape[1] if n_row is None else n_row
    s_end = n if s_end is None else s_end
    recs, survivors = [], 0
    for r, yr in enumerate(rows):
        if s_begin >= s_end:
            break
        e0, e1 = max(0, s_begin - 4), min(n, s_end + 4)
        s = np.arange(max(e0, BACK), min(e1, n - HEAD), dtype=np.int64)
        acc = []
        if len(s):
            v = np.stack([yr[s + SPB * k - buf_index0] for k in range(-9, 8)])          # [17][starts]
            thr = v[1].copy()
            for k in range(2, 9):
                thr = thr + v[k]
            thr = thr * np.float32(0.125)
            with np.errstate(invalid="ignore"):
                lv = v > thr
                b = lv[1:] == lv[:-1]                                                       # b[-8 .. 7]
                dist = np.abs(v[1:] - thr)
            q = dist[0].copy()
            for k in range(1, 16):
                q = np.where(dist[k] < q, dist[k], q)
            train = b[:8].astype(int)
            alt = np.all(train == np.array([0, 1] * 4)[:, None], axis=0) | np.all(train == np.array([1, 0] * 4)[:, None], axis=0)
            ok = alt & np.all(b[8:].astype(int) == np.array(FLAG)[:, None], axis=0)
            for j in np.nonzero(ok)[0]:
                survivors += 1
                s0 = int(s[j])
                with np.errstate(invalid="ignore"):
                    after = yr[s0 + 8 * SPB - buf_index0:n - buf_index0:SPB][:LAST_K] > thr[j]
                pay = _walk(after.tolist(), bool(lv[16, j]))
                if pay is None or len(pay) % 8 or not 56 <= len(pay) <= 1024:
                    continue
                by = np.packbits(np.array(pay, np.uint8), bitorder="little").tobytes()
                if crc16(by[:-2]) != int.from_bytes(by[-2:], "little"):
                    continue
                acc.append((s0, by, np.float32(q[j])))
        for s_a, by_a, q_a in acc:
            if not s_begin <= s_a < s_end:
                continue
            if any(by_b == by_a and 0 < abs(s_b - s_a) < 5 and (q_b > q_a or (q_b == q_a and s_b < s_a)) for s_b, by_b, q_b in acc):
                continue
            recs.append((r, s_a, by_a, q_a))
    if stats is not None:
        stats["survivors"] = survivors
    count = len(recs)
    recs = recs if max_frames is None else recs[:max(max_frames, 0)]
    msg = np.zeros((len(recs), 128), np.uint8)
    for i, rec in enumerate(recs):
        msg[i, :len(rec[2])] = np.frombuffer(rec[2], np.uint8)
    return (msg, np.array([len(r[2]) for r in recs], np.int32), np.array([r[0] for r in recs], np.int32), np.array([r[1] for r in recs], np.int64),
            np.array([r[3] for r in recs], np.float32), count)


# ---- crafted rows (direct_y) the CPU and the GPU tests share ---------------------------------------------------------------------------------
def long_frame():
    """A frame of 1024 payload bits: 126 message bytes and the check bytes."""
    body = bytes((37 * i + 11) & 0xFF for i in range(126))
    return with_crc(body)


def dense_row(n_patterns, period=80):
    """Training + flag every `period` samples and nothing behind the flags (the rest is the level the flag ends on, so every walk runs
    into seven ones): n_patterns survivors of the flag test, no frame.  -> (row, the starts)."""
    assert period >= 80 and period % SPB == 0
    pat = [k & 1 for k in range(8)] + list(FLAG)                  # 16 bits: 80 samples
    n = BACK + period * n_patterns + HEAD + 50
    y = np.zeros(n, np.float32)
    y[5] = 1.0                                                     # the level in front of the first pattern
    starts = []
    for i in range(n_patterns):
        at = 10 + period * i                                       # the strobe of the pattern's first bit; the level before it: the last one
        lv = nrzi(pat)
        y[at + SPB * np.arange(16)] = lv
        starts.append(at + 8 * SPB)
    return y, starts


# ---- the shapes tests/test_gpu_ais.py and tests/test_gpu_start_list.py share (the caps are the callers': tests/ais_caps.py) ----------------------
SHORT_FRAME = with_crc(SHIPS[0][:4] + bytes([0]))             # 56 bits: the shortest frame
SHORT_N = 50 + SPB * (len(burst_bits(SHORT_FRAME)) - 1) + 1    # a row of one tile: a burst that starts at 49 ends with it


def carrying(n_rows, grid_cap):
    """The rows of a batch of one-tile rows that carry a record: those of every other round of a detect grid of grid_cap workgroups, and
    the last.  A workgroup then meets tiles with, without, with, without survivors, and workgroup 0 a fifth that has them."""
    return [r for r in range(n_rows) if (r // grid_cap) % 2 == 0 or r == n_rows - 1]


def short_start(r):
    return flag_start((3 * r) % 50)


def short_rows(n_rows, grid_cap, dense=False):
    """float32 [n_rows][SHORT_N], one tile a row.  Plain: the shortest burst, its first strobe at (3 r) % 50, in the carrying rows, zeros
    elsewhere.  dense: that burst with every level held all five samples in EVERY row: five survivors a row, the earliest stays."""
    y = np.zeros((n_rows, SHORT_N), np.float32)
    bits = burst_bits(SHORT_FRAME)
    for r in (range(n_rows) if dense else carrying(n_rows, grid_cap)):
        y[r] = direct_y(SHORT_N, [(bits, (3 * r) % 50)], hold=SPB if dense else 1)
    return y

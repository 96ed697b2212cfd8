"""Packet-radio test rows and an independent statement of the receiver's rules, NumPy only and no library code.

    addresses, control, PID, information -> bytes -> CRC-16/X.25 -> bits, each byte's least significant first -> a zero stuffed in behind
    every five ones -> n flags + frame + n flags (frames in a row may share ONE flag) -> NRZI (a 0 changes the level) -> either levels held
    over each bit's 22 samples (direct_z: a row the frame search reads without a front) or audio (synth: continuous-phase 1200 / 2200 Hz at a
    stated clock factor, optionally pre-emphasised, frequency-modulated at 3 kHz deviation, seeded complex noise at a stated SNR in the
    26.4 kHz band -> complex64 at 26 400 S/s, or at any other rate for the captures of packet_recording).

numpy_front and numpy_frames restate PARITY.md "Packet" from the rules: the front vectorised, with the fused multiply-add of the four chains
rebuilt from error-free transformations (NumPy has none), the flag test vectorised in float32, the walk on Python lists in two stages (the
strobes with their clock tracking, then the HDLC reading of the bits).  tools/make_packet_golden.py stores the statement's records of every
fixture row in tests/golden/packet.npz with a CRC-32 of each row; the rows are regenerated here.
"""
import zlib

import numpy as np

RATE = 26400
SPB = 22
BACK, HEAD = 22, 154
NEAR = 22
LAST_K = 3183                  # 8 + 2646 appended + 528 dropped + 2 closing - 1
REACH = HEAD + 23 * (LAST_K - 7) + 1      # 73 203
MAX_BYTES, REC_BYTES = 330, 332
FLAG = (0, 1, 1, 1, 1, 1, 1, 0)
TILE = 4096                    # k_packet_detect's tile, FRONT_TILE k_packet_front's (tests/packet_caps.py pins them)
FRONT_TILE = 2048
MARK_HZ, SPACE_HZ, DEVIATION_HZ = 1200.0, 2200.0, 3000.0


# ---- frames ------------------------------------------------------------------------------------------------------------------------------------
def crc16(data):
    """CRC-16/X.25 of a byte string, byte by byte: reflected 0x8408, init 0xFFFF, final complement."""
    r = 0xFFFF
    for byte in bytes(data):
        r ^= byte
        for _ in range(8):
            r = (r >> 1) ^ 0x8408 if r & 1 else r >> 1
    return r ^ 0xFFFF


def with_crc(body):
    """The frame's bytes: the body and its check bytes, low byte first."""
    return bytes(body) + crc16(body).to_bytes(2, "little")


def address(call, ssid=0, last=False, repeated=False):
    """Seven address bytes: six characters shifted left by one, then 0 r r SSID e with the reserved bits set."""
    return bytes(ord(c) << 1 for c in call.ljust(6)[:6]) + bytes([0x60 | (0x80 if repeated else 0) | ((ssid & 15) << 1) | (1 if last else 0)])


def ui_frame(dest, source, path, info, control=0x03, pid=0xF0):
    """dest, source: (call, ssid); path: [(call, ssid, repeated), ...] -> the frame's body (no check bytes)."""
    out = address(dest[0], dest[1], repeated=True) + address(source[0], source[1], last=not path)
    for i, (call, ssid, rep) in enumerate(path):
        out += address(call, ssid, last=i == len(path) - 1, repeated=rep)
    return out + bytes([control, pid]) + bytes(info)


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


def burst_bits(frames, lead=20, tail=2, stuffed=None):
    """lead flags, the stuffed frames with ONE flag between two of them, tail flags -> a list of data bits.  frames: one frame's bytes or a
    list of them (stuffed: the bits between the flags, given outright, for one frame)."""
    if isinstance(frames, (bytes, bytearray)):
        frames = [frames]
    out = list(FLAG) * lead
    for i, f in enumerate(frames):
        if i:
            out += list(FLAG)
        out += stuff(wire_bits(f)) if stuffed is None else list(stuffed)
    return out + list(FLAG) * tail


def nrzi(bits, level=0):
    """Data bits -> levels 0 / 1: a 0 changes the level."""
    out = []
    for b in bits:
        level = level if b else 1 - level
        out.append(level)
    return out


def flag_start(at, lead=20, which=None):
    """The start s (the first strobe of a flag, at its bit's centre) of a burst whose first bit's centre lies at sample `at`: flag `which`
    of the leading ones (default the last: the one a frame follows)."""
    which = lead - 1 if which is None else which
    return at + SPB * 8 * which


def direct_z(n, bursts, base=0.0):
    """A float32 row of n samples: `base` everywhere, and for every (bits, at[, amp[, peak]]) the NRZI levels +-amp over the 22 samples of
    each bit, bit k's centre at at + 22 k (its cell: [centre - 11, centre + 11)); peak: the value at the centres themselves (default amp).
    Samples past the row are cut.  The level in front of the first bit is -amp's opposite: the first bit of a flag changes it."""
    z = np.full(n, base, np.float32)
    for bits, at, *rest in bursts:
        amp = rest[0] if rest else 1.0
        peak = rest[1] if len(rest) > 1 else amp
        lv = np.array(nrzi([1] + list(bits)), np.float64) * 2 - 1      # one bit of the level before the burst in front
        for k, v in enumerate(lv):
            c = at + SPB * (k - 1)
            lo, hi = max(c - 11, 0), min(c + 11, n)
            if lo < hi:
                z[lo:hi] = v * amp
            if 0 <= c < n:
                z[c] = v * peak
    return z


def synth(n, bursts, snr_db=None, seed=0, rate=RATE, preemph=False):
    """complex64 [n] at `rate` S/s: every (bits, at, clock[, offset_hz]) as audio FSK under FM, the first bit starting at sample `at`, the
    sender's bit clock 1200 `clock` bit/s, on seeded complex Gaussian noise snr_db below the carrier in the whole band (None: no noise).
    The carrier is on for the whole row (an unmodulated carrier between bursts: the discriminator rests at 0), at offset_hz in the burst
    with the largest `at` before each sample (0 in front of the first).  preemph: the audio through y[i] = x[i] - 0.9 x[i - 1] (about
    +4.8 dB at 2200 Hz over 1200 Hz at 26.4 kS/s), scaled back to a peak of 1."""
    audio = np.zeros(n, np.float64)
    carrier = np.zeros(n, np.float64)
    for bits, at, clock, *rest in bursts:
        lv = np.array(nrzi(bits), np.int64)
        spb = rate / (1200.0 * clock)
        count = int(np.floor(len(lv) * spb))
        idx = np.minimum((np.arange(count) / spb).astype(np.int64), len(lv) - 1)
        f = np.where(lv[idx] == 1, SPACE_HZ, MARK_HZ)
        ph = 2 * np.pi * np.cumsum(f) / rate
        a = np.sin(ph)
        if preemph:
            a = a - 0.9 * np.concatenate([[0.0], a[:-1]])
            a = a / np.max(np.abs(a))
        lo, hi = max(at, 0), min(at + count, n)
        audio[lo:hi] = a[lo - at:hi - at]
        if rest:
            carrier[lo:] = rest[0]
    phase = 2 * np.pi * np.cumsum(DEVIATION_HZ * audio + carrier) / rate
    x = np.exp(1j * phase)
    if snr_db is not None:
        rng = np.random.default_rng(seed)
        sigma = np.sqrt(10.0 ** (-snr_db / 10.0) / 2)
        x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def row_crc32(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


# ---- the rules again: the front ------------------------------------------------------------------------------------------------------------------
def tones():
    u = np.arange(22, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * u / 22), np.sin(2 * np.pi * u / 22), np.cos(2 * np.pi * u / 12), np.sin(2 * np.pi * u / 12)])


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma64(t, d, c):
    """round(t d + c) once, in float64, for d that hold float32 values (24 significant bits): the product's two parts by Veltkamp's split
    of t (both partial products are exact), the sum of three by Boldo and Melquiond's rule (the small parts added with rounding to odd,
    then one rounding to nearest).  Element-wise on arrays; a NaN stays a NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = 134217729.0 * t
        th = f - (f - t)
        tl = t - th
        uh = t * d
        ul = (th * d - uh) + tl * d
        sh, sl = _two_sum(c, uh)
        v, w = _two_sum(sl, ul)
        even = (v.view(np.uint64) & np.uint64(1)) == 0
        fix = (w != 0) & even & np.isfinite(v)
        toward = np.where(w > 0, np.inf, -np.inf)
        # v = 0 with w != 0 cannot happen: two_sum's error is below half an ulp of a non-zero v
        v = np.where(fix, np.nextafter(v, toward), v)
        return sh + v


def numpy_disc(x):
    """d[0] = 0, d[i] = float32 angle of the complex64 product x[i] conj(x[i - 1]): NumPy's own complex64 arithmetic and float32 arctan2."""
    x = np.asarray(x, np.complex64)
    d = np.zeros(len(x), np.float32)
    if len(x) > 1:
        with np.errstate(invalid="ignore"):
            d[1:] = np.angle(x[1:] * np.conj(x[:-1]))
    return d


def numpy_front(x, table=None, space_gain=1.0, d=None):
    """x complex64 [n] -> z float32 [n] by the rules of the front (d: the discriminator row, where the caller has one)."""
    t = tones() if table is None else np.asarray(table, np.float64)
    d = numpy_disc(x) if d is None else np.asarray(d, np.float32)
    n = len(d)
    pad = np.concatenate([np.zeros(11), d.astype(np.float64), np.zeros(10)])
    c = np.zeros((4, n), np.float64)
    for u in range(22):
        c = fma64(t[:, u:u + 1] * np.ones((1, n)), pad[None, u:u + n] * np.ones((4, 1)), c)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        em = c[0] * c[0] + c[1] * c[1]
        es = np.float64(space_gain) * (c[2] * c[2] + c[3] * c[3])
        den = es + em
        z = np.where(den == 0, 0.0, (es - em) / np.where(den == 0, 1.0, den))
    return z.astype(np.float32)


def front_span(i_begin, i_end, n):
    return max(0, i_begin - 12), min(n, i_end + 10)


# ---- the rules again: the frame search -------------------------------------------------------------------------------------------------------------
def reach(s_begin, s_end, n):
    """The samples [lo, hi) a window's starts and their possible suppressors read."""
    e0, e1 = max(0, s_begin - 21), min(n, s_end + 21)
    return max(0, e0 - BACK), min(n, e1 - 1 + REACH)


def _strobes(pos, p7, n):
    """pos: the row's z > 0 as a list; p7: the row index of the flag's last strobe -> yields (data bit, level, row index) of the strobes k = 8,
    9, ... while they lie inside the row, each placed by the tracking rule."""
    p_prev, a = p7, 0
    while True:
        p = p_prev + SPB + a
        if p >= n:
            return
        lv = pos[p]
        a = 0
        if lv != pos[p_prev]:
            c = next(j for j in range(p_prev + 1, p + 1) if pos[j] == lv)
            e = 2 * c - (p_prev + p) - 1
            a = 1 if e > 4 else -1 if e < -4 else 0
        yield (0 if lv != pos[p_prev] else 1), lv, p
        p_prev = p


def _hdlc(strobes, pos, n):
    """The bits of _strobes -> the payload's bit list, or None."""
    out, run = [], 0
    for b, lv, p in strobes:
        if run == 5:
            if b == 0:
                run = 0
                continue
            if p + SPB >= n or pos[p + SPB] == lv:      # the look-ahead outside the row, or a seventh one
                return None
            return out[:-6] if len(out) >= 6 else None
        if len(out) == 2646:
            return None
        out.append(b)
        run = run + 1 if b else 0
    return None


def address_ok(frame):
    """direwolf's sanity check on a frame with its check bytes."""
    end = next((j for j, b in enumerate(frame) if b & 1), None)
    if end is None or end % 7 != 6:
        return False
    m = (end + 1) // 7
    if not 2 <= m <= 10 or len(frame) < 7 * m + 3:
        return False
    ok = set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ")
    return all((frame[7 * a + j] >> 1) in ok for a in range(m) for j in range(6))


def numpy_frames(z, q_min=0.0, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_frames=None, stats=None):
    """z float32 [n_rows][n_buf] or [n_buf] -> (msg uint8 [k][332], len int32, row int32, pos int64, score float32, count)."""
    rows = np.asarray(z, np.float32)
    rows = rows[None, :] if rows.ndim == 1 else rows
    n = buf_index0 + rows.shape[1] if n_row is None else n_row
    s_end = n if s_end is None else s_end
    recs, survivors, strobes_read = [], 0, []
    for r, zr in enumerate(rows):
        if s_begin >= s_end:
            break
        e0, e1 = max(0, s_begin - 21), min(n, s_end + 21)
        s = np.arange(max(e0, BACK), min(e1, n - HEAD), dtype=np.int64)
        acc = []
        if len(s):
            v = np.stack([zr[s + SPB * k - buf_index0] for k in range(-1, 8)])            # [9][starts]
            with np.errstate(invalid="ignore"):
                lv = v > 0
                b = lv[1:] == lv[:-1]                                                       # b[0 .. 7]
                dist = np.abs(v)
                q = dist[0].copy()
                for k in range(1, 9):
                    q = np.where(dist[k] < q, dist[k], q)
                ok = np.all(b.astype(int) == np.array(FLAG)[:, None], axis=0) & (q >= np.float32(q_min))
            hits = np.nonzero(ok)[0]
            if len(hits):
                lo = int(s[hits[0]]) - buf_index0
                with np.errstate(invalid="ignore"):
                    pos = [False] * (lo + buf_index0) + (zr[lo:] > 0).tolist()             # indexed by row index; only [s, n) is read
            for j in hits:
                survivors += 1
                s0 = int(s[j])
                count = [0]

                def counted(gen):
                    for item in gen:
                        count[0] += 1
                        yield item
                pay = _hdlc(counted(_strobes(pos, s0 + HEAD, n)), pos, n)
                strobes_read.append(count[0])
                if pay is None or len(pay) % 8 or not 136 <= len(pay) <= 2640:
                    continue
                by = np.packbits(np.array(pay, np.uint8), bitorder="little").tobytes()
                if crc16(by[:-2]) != int.from_bytes(by[-2:], "little") or not address_ok(by):
                    continue
                acc.append((s0, by, np.float32(q[j])))
        for s_a, by_a, q_a in acc:
            if not s_begin <= s_a < s_end:
                continue
            if any(by_b == by_a and 0 < abs(s_b - s_a) < NEAR and (q_b > q_a or (q_b == q_a and s_b < s_a)) for s_b, by_b, q_b in acc):
                continue
            recs.append((r, s_a, by_a, q_a))
    if stats is not None:
        stats["survivors"] = survivors
        stats["strobes"] = strobes_read
    count = len(recs)
    recs = recs if max_frames is None else recs[:max(max_frames, 0)]
    msg = np.zeros((len(recs), REC_BYTES), np.uint8)
    for i, rec in enumerate(recs):
        msg[i, :len(rec[2])] = np.frombuffer(rec[2], np.uint8)
    return (msg, np.array([len(r[2]) for r in recs], np.int32), np.array([r[0] for r in recs], np.int32), np.array([r[1] for r in recs], np.int64),
            np.array([r[3] for r in recs], np.float32), count)


# ---- the frames the fixtures send ------------------------------------------------------------------------------------------------------------------
POSITION = b"!4903.50N/07201.75W-Test 001234"
COMPRESSED = b"=/5L!!<*e7>7P[via base 91"
FRAMES = {
    "position": ui_frame(("APRS", 0), ("N0CALL", 7), [("WIDE1", 1, True), ("WIDE2", 2, False)], POSITION),
    "compressed": ui_frame(("APDW16", 0), ("W1AW", 9), [("WIDE2", 1, False)], COMPRESSED),
    "status": ui_frame(("APRS", 0), ("DL1ABC", 0), [], b">Net Control Center"),
    "message": ui_frame(("APRS", 0), ("N0CALL", 7), [("RELAY", 0, True), ("WIDE2", 1, False)], b":W1AW-9   :Testing 1 2 3{042"),
    "short": address("CQ", 0) + address("N0CALL", 1, last=True) + bytes([0x03]),           # 15 bytes: with its check bytes the shortest frame
    "long": ui_frame(("APRS", 0), ("N0CALL", 15), [("DIGI%d" % i, i, i < 3) for i in range(1, 9)], bytes([0xFF]) * 256),
    "ten": ui_frame(("APRS", 0), ("N0CALL", 2), [("HOP%d" % i, i, False) for i in range(1, 9)], b">ten addresses"),
    "lower": ui_frame(("APRS", 0), ("n0call", 7), [], b">lower-case source"),
    "one": address("N0CALL", 1, last=True) + bytes([0x03, 0xF0]) + b">one address only",
}
assert len(with_crc(FRAMES["short"])) == 17 and len(with_crc(FRAMES["long"])) == 330


def _flipped(frame):
    f = bytearray(with_crc(frame))
    f[20] ^= 0x04
    return bytes(f)


# name -> dict(n, seed, snr, clock, bursts=[(frames with check bytes, at, lead flags)], expect=[frames], preemph, gain, nan_at)
def _case(n, seed, snr, clock, bursts, expect=None, preemph=False, gain=1.0, nan_at=None):
    sent = [f for fs, _, _ in bursts for f in fs]
    return dict(n=n, seed=seed, snr=snr, clock=clock, bursts=bursts, expect=sent if expect is None else expect, preemph=preemph, gain=gain, nan_at=nan_at)


_P, _C, _S, _M = (with_crc(FRAMES[k]) for k in ("position", "compressed", "status", "message"))
CASES = {
    "clock_1000": _case(40000, 31, 15.0, 1.0, [([_P], 600, 20), ([_M], 21000, 20)]),
    "clock_1004": _case(40000, 32, 15.0, 1.004, [([_P], 600, 20), ([_M], 21000, 20)]),
    "clock_0996": _case(40000, 33, 15.0, 0.996, [([_P], 600, 20), ([_M], 21000, 20)]),
    "preemph_gain_100": _case(40000, 34, 15.0, 1.0, [([_C], 600, 20), ([_S], 21000, 20)], preemph=True, gain=1.0),
    "preemph_gain_035": _case(40000, 34, 15.0, 1.0, [([_C], 600, 20), ([_S], 21000, 20)], preemph=True, gain=0.35),
    "two_flags": _case(30000, 35, 15.0, 1.0, [([_P], 600, 2), ([_S], 16000, 2)]),
    "shared_flag": _case(36000, 36, 15.0, 1.0, [([_P, _C, _S], 600, 20)]),
    "short_and_long": _case(84000, 37, 15.0, 1.0, [([with_crc(FRAMES["short"])], 600, 20), ([with_crc(FRAMES["long"])], 9000, 20)]),
    "ten_addresses": _case(30000, 38, 15.0, 1.002, [([with_crc(FRAMES["ten"])], 600, 20)]),
    "refused": _case(48000, 39, 15.0, 1.0, [([with_crc(FRAMES["lower"])], 600, 20), ([with_crc(FRAMES["one"])], 12000, 20), ([_flipped(FRAMES["position"])], 22000, 20),
                                           ([_S], 36000, 20)], expect=[_S]),
    "nan_inside": _case(40000, 40, 15.0, 1.0, [([_P], 600, 20), ([_M], 21000, 20)], expect=[_P], nan_at=(26000, 26200)),
    "all_zero": _case(6000, 0, None, 1.0, [], expect=[]),
}


def case_iq(name):
    c = CASES[name]
    if name == "all_zero":
        return np.zeros(c["n"], np.complex64)
    x = synth(c["n"], [(burst_bits(fs, lead=lead), at, c["clock"]) for fs, at, lead in c["bursts"]], snr_db=c["snr"], seed=c["seed"], preemph=c["preemph"])
    if c["nan_at"] is not None:
        x[c["nan_at"][0]:c["nan_at"][1]] = np.nan      # nine bits: longer than any level is held, so a space among them reads as mark
    return x


def many_frames(count, snr_db, clock, seed, gap=14000):
    """count distinct position reports, one every `gap` samples -> (complex64 row, the frames' bytes)."""
    frames = [with_crc(ui_frame(("APRS", 0), ("N%dCALL" % (i % 10), i % 16), [("WIDE2", 1, False)],
                                b"!49%02d.%02dN/072%02d.%02dW>seed %d frame %d" % (i % 60, seed % 100, (7 * i) % 60, i % 100, seed, i))) for i in range(count)]
    x = synth(gap * count + 1000, [(burst_bits(f, lead=12), 500 + gap * i, clock) for i, f in enumerate(frames)], snr_db=snr_db, seed=seed)
    return x, frames


# ---- crafted rows (direct_z) the CPU and the GPU tests share ---------------------------------------------------------------------------------------
SHORT_FRAME = with_crc(FRAMES["short"])
SHORT_BITS = burst_bits(SHORT_FRAME, lead=1, tail=1)
# a row of one burst whose first bit's centre lies at `at`: the level before it, the bits, and the row ends with the closing flag's look-ahead
# (the walk stops at the first closing flag: the strobe behind its six ones is the look-ahead, the flag's last bit)


def edge_row(at=BACK):
    """(z, s, n): the shortest frame between one flag and one, |z| = 0.25 over every cell and 1 at the bit centres, so that with q_min = 0.5
    only the start at the centres passes the flag test; the row ends ON the closing look-ahead's sample (the closing flag's last bit)."""
    n = at + SPB * (len(SHORT_BITS) - 1) + 1
    return direct_z(n, [(SHORT_BITS, at, 0.25, 1.0)]), at, n


def dense_row(n_flags, period=8 * SPB):
    """Flag after flag and nothing behind (the level rests, so the last walk runs into seven ones and every other one closes a frame of no
    bits): 22 n_flags survivors of the flag test at q_min = 0, no frame.  -> (row, the centred starts)."""
    assert period == 8 * SPB
    bits = list(FLAG) * n_flags
    n = BACK + 11 + SPB * len(bits) + HEAD + 60
    return direct_z(n, [(bits, BACK + 11)]), [BACK + 11 + period * i for i in range(n_flags)]


def carrying(n_rows, grid_cap):
    """The rows of a batch of one-tile rows that carry a record: those of every other round of a detect grid of grid_cap workgroups, and
    the last."""
    return [r for r in range(n_rows) if (r // grid_cap) % 2 == 0 or r == n_rows - 1]


SHORT_N = 60 + SPB * (len(SHORT_BITS) - 1) + 12     # a row of one tile: a burst whose first centre lies at 33 .. 59 fits with its last cell


def short_at(r):
    return BACK + 11 + (3 * r) % 27                  # the earliest start of the flag's cell, 11 in front of the centre, still has its 22 samples in front


def short_rows(n_rows, grid_cap):
    """float32 [n_rows][SHORT_N], one tile a row: the shortest burst, its first centre at 33 + (3 r) % 27, in the carrying rows, zeros
    elsewhere."""
    z = np.zeros((n_rows, SHORT_N), np.float32)
    for r in carrying(n_rows, grid_cap):
        z[r] = direct_z(SHORT_N, [(SHORT_BITS, short_at(r))])
    return z

"""OOK outside the library: seeded generators (keyed bursts in noise, hand-made envelopes, edge lists) and a NumPy statement of the receiver's
rules (pyspecsdr_amd/csrc/pss_ook.h: magnitude, envelope, levels, state, edges, messages, slicers, records) that shares no code with the
header: it works on whole rows with array operations (np.maximum.accumulate for the state, np.repeat for the Manchester half-bits) where the
header walks samples and edges.  tests/test_ook_golden.py holds the host twin to it byte for byte; tools/make_ook_golden.py writes
tests/golden/ook.npz from it."""
import zlib

import numpy as np

BLOCK = 4096
TILE = 4096                    # k_ook_detect's tile (tests/ook_caps.py pins it)
MAX_PULSES, MAX_BITS = 1024, 256
PWM, PPM, MC = 0, 1, 2
OPEN, LONG, MANY, FULL = 1 << 22, 1 << 23, 1 << 24, 1 << 25
NO_GAP = 1 << 62
FS = 250000.0

# the two fixtures' timings in samples at 250 kS/s (PARITY.md "OOK", fixtures)
PPM_SPEC = dict(mode=PPM, short=250, long=500, sync=0, tol=60, gap_limit=750, span=1 << 16, phase=0, invert=0, min_bits=16, max_odd=0)
PWM_SPEC = dict(mode=PWM, short=88, long=264, sync=0, tol=40, gap_limit=600, span=1 << 16, phase=0, invert=0, min_bits=16, max_odd=0)
DETECT = dict(P=9, R=64)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


# ---- the rules ----------------------------------------------------------------------------------------------------------------------------
def magnitude(x):
    x = np.asarray(x, np.complex64)
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    return re * re + im * im          # float32 products and one float32 sum


def envelope(m, P):
    """m: float32 [n] from index 0 of the row -> e float32 [n]."""
    m = np.asarray(m, np.float32)
    mp = np.concatenate([np.zeros(P - 1, np.float64), m.astype(np.float64)])
    acc = np.zeros(len(m), np.float64)
    for k in range(P - 1, -1, -1):    # m[n - k], the oldest first
        acc = acc + mp[P - 1 - k:P - 1 - k + len(m)]
    return (acc / np.float64(P)).astype(np.float32)


def block_means(m):
    nb = len(m) // BLOCK
    if not nb:
        return np.zeros(0, np.float64)
    b = np.asarray(m[:nb * BLOCK], np.float32).astype(np.float64).reshape(nb, BLOCK)
    return np.add.accumulate(b, axis=1)[:, -1] / np.float64(BLOCK)


def levels(means, hi_ratio=8.0, lo_ratio=4.0):
    floor = np.sort(np.asarray(means, np.float64))[len(means) // 4]
    return np.float32(hi_ratio * floor), np.float32(lo_ratio * floor)


def state(e, hi, lo, R):
    n = len(e)
    idx = np.arange(n)
    with np.errstate(invalid="ignore"):
        high, low = e >= np.float32(hi), e < np.float32(lo)
    last = np.maximum.accumulate(np.where(high | low, idx, -1)) if n else idx
    return (last >= 0) & high[np.maximum(last, 0)] & (idx - last <= R)


def edges(on):
    """-> (rises, falls): equally long; a pulse on at the last sample falls at len(on)."""
    d = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)


def slice_message(r, f, gap_limit, span, n_row, spec):
    """r, f: the rises and falls of the pulses from the message's first on, to the row's end -> dict(bits, n_bits, span, meta)."""
    pos = int(r[0])
    lim = pos + span
    gaps = np.append(r[1:] - f[:-1], NO_GAP)
    chain = int(np.flatnonzero(gaps > gap_limit)[0]) + 1            # the pulses up to and including the first long gap
    readable = int(np.count_nonzero(r[:chain] < lim))
    n_fit = int(np.count_nonzero(f[:readable] < lim))
    flags = 0
    if n_fit < readable and n_fit < MAX_PULSES:
        flags |= LONG
    if readable > MAX_PULSES and n_fit >= MAX_PULSES:
        flags |= MANY
    n = min(n_fit, MAX_PULSES)
    r, f = r[:n].astype(np.int64), f[:n].astype(np.int64)
    if n and f[-1] == n_row:
        flags |= OPEN
    short, long_, sync, tol = spec['short'], spec.get('long', 0), spec.get('sync', 0), spec['tol']
    n_odd = 0
    if spec['mode'] == MC:
        sym = np.empty(max(2 * n - 1, 0), np.int64)
        sym[0::2] = f - r
        sym[1::2] = r[1:] - f[:-1]
        k = np.where(np.abs(sym - short) <= tol, 1, np.where(np.abs(sym - 2 * short) <= tol, 2, 0))
        bad = np.flatnonzero(k == 0)
        if len(bad):
            k = k[:bad[0]]
            n_odd += 1
        h = np.repeat(1 - (np.arange(len(k)) & 1), k)[spec.get('phase', 0):]
        h = h[:len(h) // 2 * 2].reshape(-1, 2)
        differ = h[:, 0] != h[:, 1]
        n_odd += int(np.count_nonzero(~differ))
        bits = h[differ, 0]
    else:
        w = (f - r) if spec['mode'] == PWM else (r[1:] - f[:-1])
        is_s, is_l = np.abs(w - short) <= tol, np.abs(w - long_) <= tol
        is_y = (np.abs(w - sync) <= tol) if sync else np.zeros(len(w), bool)
        n_odd = int(np.count_nonzero(~(is_s | is_l | is_y)))
        one = is_s if spec['mode'] == PWM else is_l
        bits = one[is_s | is_l].astype(np.int64)
    if len(bits) > MAX_BITS:
        flags |= FULL
        bits = bits[:MAX_BITS]
    bits = bits ^ spec.get('invert', 0)
    packed = np.zeros(32, np.uint8)
    pk = np.packbits(bits.astype(np.uint8))
    packed[:len(pk)] = pk
    return dict(bits=packed, n_bits=len(bits), pos=pos, span=int(f[-1] - pos) if n else 0, meta=n | min(n_odd, 2047) << 11 | flags, n_odd=n_odd)


def row_messages(x, hi, lo, spec, P=9, R=64, s_begin=0, s_end=None):
    """The whole row's records with pos in [s_begin, s_end): windows are a filter on what the whole row gives."""
    n_row = len(x)
    s_end = n_row if s_end is None else s_end
    on = state(envelope(magnitude(x), P), hi, lo, R)
    r, f = edges(on)
    out = []
    for i in range(len(r)):
        if not s_begin <= r[i] < s_end:
            continue
        if i and r[i] - f[i - 1] <= spec['gap_limit']:
            continue
        rec = slice_message(r[i:], f[i:], spec['gap_limit'], spec['span'], n_row, spec)
        if rec['n_bits'] >= spec.get('min_bits', 0) and rec['n_odd'] <= spec.get('max_odd', 0):
            out.append(rec)
    return out


def messages(rows, hi, lo, spec, P=9, R=64, s_begin=0, s_end=None):
    """rows [k][n] -> the arrays of pss_ook_messages: (bits, n_bits, row, pos, span, meta)."""
    rows = np.atleast_2d(rows)
    recs = [(k, rec) for k in range(len(rows)) for rec in row_messages(rows[k], hi, lo, spec, P, R, s_begin, s_end)]
    return (np.array([rec['bits'] for _, rec in recs], np.uint8).reshape(-1, 32), np.array([rec['n_bits'] for _, rec in recs], np.int32),
            np.array([k for k, _ in recs], np.int32), np.array([rec['pos'] for _, rec in recs], np.int64),
            np.array([rec['span'] for _, rec in recs], np.int32), np.array([rec['meta'] for _, rec in recs], np.uint32))


# ---- generators -----------------------------------------------------------------------------------------------------------------------------
def keying_ppm(bits, pulse=125, zero=250, one=500):
    """-> [(on, off), ...]: a pulse and its gap per bit, then the closing pulse (its gap is the caller's)."""
    return [(pulse, one if b else zero) for b in bits] + [(pulse, 0)]


def keying_pwm(bits, short=88, long_=264, period=352):
    """a short pulse is a 1, a long one a 0; every pulse and its gap fill one period"""
    return [((short, period - short) if b else (long_, period - long_)) for b in bits]


def keying_mc(bits, half=100):
    """Manchester: 1 is (on, off), 0 is (off, on) -> the runs as (on, off) pairs; a leading off run is dropped with its half-bit"""
    h = [v for b in bits for v in ((1, 0) if b else (0, 1))]
    while h and not h[0]:
        h = h[1:]
    runs, k = [], 0
    while k < len(h):
        j = k
        while j < len(h) and h[j] == h[k]:
            j += 1
        runs.append((h[k], (j - k) * half))
        k = j
    out = []
    for a in range(0, len(runs), 2):
        out.append((runs[a][1], runs[a + 1][1] if a + 1 < len(runs) else 0))
    return out


def key_row(n, placements):
    """placements: [(start, [(on, off), ...]), ...] -> uint8 [n], 1 where the carrier is keyed"""
    key = np.zeros(n, np.uint8)
    for start, pulses in placements:
        t = start
        for on, off in pulses:
            key[t:t + on] = 1
            t += on + off
    return key


def clean_row(key, amp=4.0, floor=0.01):
    """A noiseless row whose m is amp^2 where keyed and floor^2 elsewhere: hand-made envelopes, exact in float32 for powers of two"""
    return (np.where(key, np.float32(amp), np.float32(floor)) + 0j).astype(np.complex64)


def burst_fixture(kind, snr_db, seed, n=8_000_000, n_tx=30, repeats=3):
    """Unit-power complex noise and a keyed carrier with a frequency offset, snr_db above it: n_tx transmissions of `repeats` copies each ->
    (row complex64 [n], sent: the list of each copy's bits, spec)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(2 * n, dtype=np.float32).view(np.complex64) * np.float32(np.sqrt(0.5))
    n_bits = 36 if kind == 'ppm' else 24
    slot = n // max(n_tx, 1)
    placements, sent = [], []
    for k in range(n_tx):
        bits = rng.integers(0, 2, n_bits).tolist()
        if kind == 'ppm':                      # the nexus layout's fixed bits
            bits[9], bits[24:28] = 0, [1, 1, 1, 1]
        t = k * slot + int(rng.integers(20000, slot // 2))
        for _ in range(repeats):
            pulses = keying_ppm(bits) if kind == 'ppm' else keying_pwm(bits)
            placements.append((t, pulses))
            sent.append(bits)
            t += sum(a + b for a, b in pulses) + (1000 if kind == 'ppm' else 2728 - pulses[-1][1])
    key = key_row(n, placements)
    idx = np.flatnonzero(key)
    amp = np.float32(10.0 ** (snr_db / 20.0))
    phase = (2 * np.pi * 0.0137) * idx + 0.3
    x[idx] += (amp * np.exp(1j * phase)).astype(np.complex64)
    return x, sent, dict(PPM_SPEC if kind == 'ppm' else PWM_SPEC)


def channel_capture(seed=77, n=4_000_000, fs=1e6, n_tx=3):
    """Two keyed carriers in one capture at 1 MS/s, 200 kHz below and 150 kHz above its centre, PPM (nexus layout) on the first and PWM on
    the second, 15 dB above unit-power noise; their timings are the fixtures' at the 250 kS/s the channels have after decimation by 4 ->
    (capture complex64 [n], fs, center_hz, channels_hz, sent: per channel the list of each transmission's bits)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(2 * n, dtype=np.float32).view(np.complex64) * np.float32(np.sqrt(0.5))
    center, channels = 433.92e6, [433.72e6, 434.07e6]
    amp = np.float32(10.0 ** (15.0 / 20.0))
    sent = []
    slot = n // n_tx
    for c, kind in enumerate(('ppm', 'pwm')):
        placements, mine = [], []
        for k in range(n_tx):
            bits = rng.integers(0, 2, 36 if kind == 'ppm' else 24).tolist()
            if kind == 'ppm':
                bits[9], bits[24:28] = 0, [1, 1, 1, 1]
            pulses = [(4 * a, 4 * b) for a, b in (keying_ppm(bits) if kind == 'ppm' else keying_pwm(bits))]
            t = k * slot + int(rng.integers(40000, slot // 2))
            for _ in range(3):
                placements.append((t, pulses))
                t += sum(a + b for a, b in pulses) + 4 * (1000 if kind == 'ppm' else 2728 - pulses[-1][1] // 4)
            mine.append(bits)
        idx = np.flatnonzero(key_row(n, placements))
        x[idx] += (amp * np.exp(2j * np.pi * ((channels[c] - center) / fs) * idx)).astype(np.complex64)
        sent.append(mine)
    return x, fs, center, channels, sent


FIXTURES = [(kind, snr, 100 * snr + k) for snr in (12, 15, 20) for k, kind in enumerate(('ppm', 'pwm'))]


# small_rows' four slicers: every message reported, whatever its bits
SMALL_SPECS = [dict(PPM_SPEC, min_bits=0, max_odd=2047), dict(PWM_SPEC, min_bits=0, max_odd=2047),
               dict(mode=MC, short=100, tol=30, gap_limit=400, span=1 << 16, phase=0, invert=0, min_bits=0, max_odd=2047),
               dict(mode=MC, short=100, tol=30, gap_limit=400, span=1 << 16, phase=1, invert=1, min_bits=0, max_odd=2047)]


def bits_of(packed, n_bits):
    return np.unpackbits(np.asarray(packed, np.uint8))[:n_bits].tolist()


def small_rows(seed=7):
    """A handful of short rows that reach every rule cheaply: three slicers, an OPEN pulse, a pulse on at sample 0, NaN and inf samples, a sync
    pulse, odd symbols, a long message -> (rows complex64 [k][n], hi, lo)."""
    rng = np.random.default_rng(seed)
    n = 3 * TILE + 321
    rows = []
    # row 0: PPM and PWM copies straddling tile boundaries
    p = [(TILE - 700, keying_ppm([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0], 125, 250, 500)),
         (2 * TILE - 1500, keying_pwm([1, 1, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1], 88, 264, 352))]
    rows.append(clean_row(key_row(n, p)))
    # row 1: Manchester, a pulse on at sample 0, and one on at the last sample
    p = [(0, [(300, 0)]), (1000, keying_mc([1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1], 100)), (n - 150, [(150, 0)])]
    rows.append(clean_row(key_row(n, p)))
    # row 2: noise with strong bursts, a NaN and an inf
    x = (rng.standard_normal(2 * n, dtype=np.float32).view(np.complex64) * np.float32(0.01)).copy()
    key = key_row(n, [(500, keying_ppm([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 0, 0], 125, 250, 500)), (TILE + 4000, keying_pwm([1, 0] * 9, 88, 264, 352))])
    x[key == 1] += np.complex64(4.0)
    x[9000] = np.complex64(complex(np.nan, 0.0))
    x[9500] = np.complex64(complex(np.inf, 0.0))
    x[700] = np.complex64(complex(0.0, np.nan))
    rows.append(x)
    return np.stack(rows), np.float32(2.0), np.float32(1.0)


# ---- the shapes of the GPU test (tests/test_ook_shapes.py runs them through the host twin first) ---------------------------------------------
HI, LO = np.float32(4.0), np.float32(1.0)           # with level_row's m: 16 is high, 2 is neither, 0.25 is low
ANY = dict(min_bits=0, max_odd=2047)
PWM_S = dict(mode=PWM, short=4, long=8, sync=12, tol=1, gap_limit=10, span=1 << 16, phase=0, invert=0, **ANY)
PPM_S = dict(mode=PPM, short=4, long=8, sync=12, tol=1, gap_limit=14, span=1 << 16, phase=0, invert=0, **ANY)
MC_S = dict(mode=MC, short=5, tol=1, gap_limit=14, span=1 << 16, phase=0, invert=0, **ANY)


def level_row(n, seed, mean_run=12):
    """Runs of three exact levels, m = 16 (high), 2 (neither) and 0.25 (low), with geometric lengths: the hysteresis and the reach at work"""
    rng = np.random.default_rng(seed)
    amp = np.array([4.0, np.sqrt(2.0), 0.5], np.float32)
    runs = rng.geometric(1.0 / mean_run, n // 2 + 2)
    lev = rng.integers(0, 3, len(runs))
    return (np.repeat(amp[lev], runs)[:n] + 0j).astype(np.complex64)


def pulses_row(n, start, pulses, amp=4.0):
    return clean_row(key_row(n, [(start, pulses)]), amp, 0.5)


def case(name, rows, spec, P=1, R=0, hi=HI, lo=LO, **kw):
    return dict(name=name, rows=np.atleast_2d(rows), spec=dict(spec), P=P, R=R, hi=np.float32(hi), lo=np.float32(lo), **kw)


def shape_cases():
    """-> the list of cases: dict(name, rows [k][n] complex64, spec, P, R, hi, lo[, max_msgs])"""
    out = []
    # row lengths around P and the tile, every P and R at its ends
    for n in (1, 8, 9, 4095, 4096, 4097, 8193):
        out.append(case(f"len{n}", level_row(n, n), PWM_S, P=9, R=64))
    for P in (1, 2, 65):
        for R in (0, 1, 63, 64, 4096):
            out.append(case(f"P{P}_R{R}", np.stack([level_row(2 * TILE + 77, 100 * P + R + k, 40 if R > 64 else 12) for k in range(2)]), PPM_S, P=P, R=R))
    # the last decisive-high sample exactly R and R + 1 back, inside a tile and across the boundary: m = 16 up to a, then 2 (neither)
    for R in (64, 4096):
        T = TILE if R < TILE else 2 * TILE
        for a in (1000, T - R - 2, T - R - 1, T - R, T - 1, T):
            x = np.full(4 * TILE, np.sqrt(2.0), np.float32)
            x[:10] = 0.5
            x[max(a - 20, 10):a + 1] = 4.0
            x[a + R + 1 + (a % 3):a + R + 40] = 4.0      # on again R + 1, R + 2 or R + 3 behind a: no fall, a one-sample gap, a two-sample gap
            out.append(case(f"reach_R{R}_a{a}", (x + 0j).astype(np.complex64), dict(PWM_S, gap_limit=1), P=1, R=R))
    # a pulse, a gap of exactly gap_limit and gap_limit + 1, and a whole message across a tile boundary
    for g in (10, 11):
        for start in (TILE - 30, TILE - 8 - g, TILE - 4, 2 * TILE - 8 - g // 2):
            out.append(case(f"gap{g}_at{start}", pulses_row(3 * TILE, start, [(4, 4), (8, g), (4, 4), (8, 4), (4, 0)]), PWM_S))
    # a pulse on at sample 0 and one on at the row's last sample; adjacent rows that must not run into each other
    a = pulses_row(2 * TILE, 0, [(8, 4), (4, 4), (4, 2 * TILE - 28), (4, 0)])
    b = pulses_row(2 * TILE, 0, [(4, 4), (8, 4), (4, 0)])
    out.append(case("open_and_zero", np.stack([a, b, a]), PWM_S))
    # e exactly equal to hi (high) and to lo (not low)
    out.append(case("e_eq_hi_lo", level_row(TILE + 99, 5), PWM_S, P=1, R=3, hi=2.0, lo=2.0))
    out.append(case("e_eq_hi", level_row(TILE + 99, 6), PWM_S, P=1, R=3, hi=16.0, lo=0.25))
    x = level_row(2 * TILE, 8).copy()
    x[[5, 4000, 4100, 6000]] = [complex(np.nan, 1), complex(np.inf, 0), complex(0, -np.inf), complex(np.nan, np.nan)]
    out.append(case("nan_inf", x, PWM_S, P=9, R=64))
    # every other sample an edge: a tile's list fills to 4096 entries, and the chain passes 1024 pulses
    n = 2 * TILE + 10
    out.append(case("alternate", clean_row(np.arange(n) & 1, 4.0, 0.5), dict(PWM_S, short=1, long=3, sync=0, tol=0, gap_limit=1)))
    # more edges than one pass of the lane kernels (2048 * 256) and one step of the scan; more messages than one pass of the walk (2048 * 4)
    n = 2048 * 256 + 3 * TILE
    out.append(case("many_edges", clean_row(np.arange(n) & 1, 4.0, 0.5), dict(PWM_S, short=1, long=3, sync=0, tol=0, gap_limit=1)))
    n = 3 * (2048 * 4 + 50)
    out.append(case("many_messages", clean_row(np.arange(n) % 3 == 0, 4.0, 0.5), dict(PWM_S, short=1, long=3, sync=0, tol=0, gap_limit=1)))
    # 1023, 1024, 1025 pulses; 255, 256, 257 bits; exactly span and span + 1 samples
    for k in (1023, 1024, 1025):
        out.append(case(f"pulses{k}", pulses_row(4 * TILE, 100, [(4, 8)] * k), PWM_S))
    for k in (255, 256, 257):
        out.append(case(f"bits{k}", pulses_row(TILE, 100, [(4, 8), (8, 4)] * (k // 2) + [(4, 8)] * (k % 2)), PWM_S))
        out.append(case(f"ppm_bits{k}", pulses_row(2 * TILE, TILE - 100, [(4, 4), (4, 8)] * (k // 2) + [(4, 4)] * (k % 2) + [(4, 0)]), PPM_S))
    msg = [(4, 8), (8, 4), (4, 8), (4, 0)]
    length = sum(a + b for a, b in msg)
    for span in (length - 1, length, length + 1, length - 4, length - 5):
        out.append(case(f"span{span}", pulses_row(TILE + 50, TILE - 10, msg), dict(PWM_S, span=span)))
    # min_bits and max_odd at their boundaries; a true count above max_msgs
    rows, hi, lo = small_rows()
    for mb, mo in ((11, 15), (12, 15), (11, 14), (0, 0), (5, 2)):      # row 0's first message has 11 bits and 15 odd symbols
        out.append(case(f"min{mb}_odd{mo}", rows, dict(PPM_SPEC, min_bits=mb, max_odd=mo), P=9, R=64, hi=hi, lo=lo))
    out.append(case("over_max", rows, dict(PWM_SPEC, **ANY), P=9, R=64, hi=hi, lo=lo, max_msgs=2))
    out.append(case("max0", rows, dict(PWM_SPEC, **ANY), P=9, R=64, hi=hi, lo=lo, max_msgs=0))
    # three slicers x invert x phase; tol = 0
    for spec in (dict(PPM_SPEC), dict(PWM_SPEC), dict(MC_S, short=100, tol=30, gap_limit=400)):
        for invert in (0, 1):
            for phase in ((0, 1) if spec['mode'] == MC else (0,)):
                out.append(case(f"mode{spec['mode']}_i{invert}_p{phase}", rows, dict(spec, invert=invert, phase=phase, **ANY), P=9, R=64, hi=hi, lo=lo))
    out.append(case("tol0", pulses_row(TILE, 50, [(4, 8), (8, 4), (5, 7), (4, 9), (12, 4), (4, 0)]), dict(PWM_S, tol=0)))
    out.append(case("tol0_ppm", pulses_row(TILE, 50, [(4, 8), (8, 4), (5, 7), (4, 9), (12, 4), (4, 0)]), dict(PPM_S, tol=0)))
    mc = keying_mc([1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 0, 1, 0, 1] * 9, 5)
    for phase in (0, 1):
        out.append(case(f"mc_long_p{phase}", pulses_row(2 * TILE, TILE - 300, mc), dict(MC_S, phase=phase)))
        out.append(case(f"mc_odd_p{phase}", pulses_row(2 * TILE, TILE - 300, mc[:20] + [(5, 17)] + mc[20:60] + [(13, 5)] + mc[60:]), dict(MC_S, phase=phase, gap_limit=20)))
    # rows whose listed edges end on a rise that starts a message: span = 1 lists no edge at n_row, so every row ends rise, fall, rise and
    # there are more messages than every other edge
    tail = np.stack([clean_row(key_row(600, [(10 + k, [(8, 0)]), (590 - k, [(10 + k, 0)])]), 4.0, 0.5) for k in range(4)])
    out.append(case("heads_span1", tail, dict(PWM_S, span=1)))
    out.append(case("heads_span1_open_only", tail[:2, 580:], dict(PWM_S, span=1)))
    out.append(case("heads_span9", tail, dict(PWM_S, span=9)))
    # 4097 one-tile rows
    out.append(case("rows4097", np.stack([level_row(48, k, 5) for k in range(64)] * 64 + [level_row(48, 999, 5)]), PWM_S, P=2, R=3))
    # one tile past the detect grid cap: a message in the last tile
    out.append(case("grid_cap", pulses_row(1025 * TILE, 1024 * TILE + 17, [(4, 8), (8, 4), (4, 8), (4, 0)]), PWM_S))
    return out


def window_cases():
    """-> (name, buffer complex64 [k][n_buf], buf_index0, n_row, s_begin, s_end, spec, P, R, whole rows [k][3 TILE], base): windows given
    exactly their reach, the rows lying at `base` of a longer row (one base past 2^40: the samples are the same, so are the records but for
    pos); and one whose every row holds a pulse that rises inside the window and is longer than span, so that each row's listed edges end
    on a rise that starts a message."""
    P, R = 9, 64
    out = []

    def add(name, x, spec, base):
        before, after = spec['gap_limit'] + R + P, spec['span']
        s_begin, s_end = base + before + 100, base + before + 100 + TILE + 7
        n_row = base + x.shape[1]
        lo_i, hi_i = s_begin - before, min(n_row, s_end + after)
        out.append((name, x[:, lo_i - base:hi_i - base], lo_i, n_row, s_begin, s_end, spec, P, R, x, base))

    x = np.stack([level_row(3 * TILE, 70 + k, 6) for k in range(2)])
    for base in (0, (1 << 40) + 12345):
        add(f"win_{base >> 40}", x, dict(PPM_S), base)
    spec = dict(PWM_S, span=40)
    s_end = spec['gap_limit'] + R + P + 100 + TILE + 7
    msg = [(6, 14), (6, 0)]           # the mean of 9 widens a pulse by 7 samples: two pulses 7 apart, 33 in all
    x = np.stack([clean_row(key_row(3 * TILE, [(300 + 7 * k, msg), (s_end - 6 - k, [(spec['span'] + 60, 0)])]), 4.0, 0.5) for k in range(4)])
    add("win_long_pulse", x, spec, 0)
    return out

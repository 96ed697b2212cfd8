"""The APT fixtures and the NumPy statement of the receiver's rules — no part of the library is used to MAKE either.

The reference holds no APT code (its command list hands the audio to wxtoimg), so the truth is made here: a seeded synthesiser builds
the words of a pass (sync A, space A, image A, telemetry A, sync B, space B, image B, telemetry B: 2080 words a line at 4160 words/s),
amplitude-modulates them on a 2400 Hz subcarrier, frequency-modulates that on a carrier at 62 400 S/s with +-17 kHz deviation, a tuning
offset, a sample-clock error in ppm and white noise at a carrier-to-noise ratio in the row's bandwidth; and numpy_front / numpy_syncs /
numpy_lines restate pyspecsdr_amd/csrc/pss_apt.h's three stages in array form.  tests/golden/apt.npz holds CRC-32s of the rows and the
statement's records (tools/make_apt_golden.py)."""
import zlib

import numpy as np

RATE = 62400
ENV_RATE = 12480
DECIM = 5
SPW = 15                     # row samples a word
ENV_SPW = 3
LINE_WORDS = 2080
LINE_ENV = 6240
LINE_ROW = LINE_WORDS * SPW  # 31 200 row samples a line
SUBCARRIER = 2400.0
DEVIATION = 17000.0
NEAR = 3120
REACH = 117
TILE = 4096
SYNC_A = np.array([int(c) for c in "000011001100110011001100110011000000000"], np.uint8)
SYNC_B = np.array([int(c) for c in "0000" + "11100" * 7], np.uint8)
WEDGES = np.array([31, 63, 95, 127, 159, 191, 224, 255, 0], np.float64) / 255.0
IMAGE_A, TELEMETRY_A, HALF = 86, 995, 1040
HIGH_K = np.array([k for k in range(4, 32) if (k - 4) & 2 == 0])
LOW_K = np.array([k for k in range(4, 32) if (k - 4) & 2])
assert len(SYNC_A) == len(SYNC_B) == 39 and SYNC_A[HIGH_K].all() and not SYNC_A[LOW_K].any()

# name: (seed, lines, start offset in row samples, tuning offset Hz, clock error ppm, C/N dB in 62.4 kHz, image)
CASES = {
    "smooth_30db": (11, 3, 4321, 0.0, 0.0, 30.0, "smooth"),
    "noise_10db_3khz_40ppm": (12, 3, 2777, 3000.0, 40.0, 10.0, "noise"),
    "smooth_10db_minus_4khz_minus_60ppm": (13, 3, 97, -4000.0, -60.0, 10.0, "smooth"),
}
TAIL = 1500                   # row samples behind the last line
DEPTH_LOW = 0.07              # the subcarrier's amplitude at black, of white's: a modulation index of 87 % gives (1 - 0.87) / (1 + 0.87)


def pass_words(n_lines, image, seed, ids=(1, 3), first_line=0):
    """float64 [n_lines][2080] in [0, 1]: the words of a pass.  image: 'smooth' (gradients and slow waves), 'noise' (white, uniform);
    ids: the wedges (1 .. 6) that channel A's and channel B's wedge 16 repeat; telemetry wedges 10 .. 15 hold fixed mid greys."""
    rng = np.random.default_rng(seed)
    w = np.zeros((n_lines, LINE_WORDS))
    lines = np.arange(first_line, first_line + n_lines)
    for c in range(2):
        o = c * HALF
        w[:, o:o + 39] = SYNC_A if c == 0 else SYNC_B
        w[:, o + 39:o + 86] = 0.0 if c == 0 else 1.0
        w[(lines % 120) < 2, o + 39:o + 86] = 1.0 if c == 0 else 0.0          # the minute markers
        if image == "smooth":
            u, v = np.meshgrid(np.arange(909) / 909.0, lines / 64.0)
            w[:, o + 86:o + 995] = 0.5 + 0.4 * np.sin(2 * np.pi * (1.5 * u + 0.7 * v + 0.25 * c)) * np.cos(2 * np.pi * (0.8 * u - 0.3 * v))
        elif image == "noise":
            w[:, o + 86:o + 995] = rng.random((n_lines, 909))
        else:
            raise ValueError(image)
        frame = ((lines % 128) // 8)
        levels = np.concatenate([WEDGES, [0.31, 0.42, 0.55, 0.48, 0.36, 0.61], [WEDGES[ids[c] - 1]]])
        w[:, o + 995:o + 1040] = levels[frame][:, None]
    return w


def modulate(words, start, offset_hz, ppm, cnr_db, seed, tail=TAIL):
    """complex64 row at 62 400 S/s: `start` samples of unmodulated subcarrier at mid level, the lines, `tail` more."""
    rng = np.random.default_rng(seed + 1000)
    flat = np.asarray(words, np.float64).reshape(-1)
    n = start + int(np.ceil(len(flat) * SPW / (1.0 + ppm * 1e-6))) + tail
    t = (np.arange(n) - start) * (1.0 + ppm * 1e-6) / RATE        # the satellite's time at each of the receiver's samples
    k = np.floor(t * 4160.0).astype(np.int64)
    a = np.where((k >= 0) & (k < len(flat)), flat[np.clip(k, 0, len(flat) - 1)], 0.5)
    s = (DEPTH_LOW + (1.0 - DEPTH_LOW) * a) * np.sin(2 * np.pi * SUBCARRIER * t)
    phase = 2 * np.pi * np.cumsum(DEVIATION * s + offset_hz) / RATE
    sigma = np.sqrt(0.5 * 10.0 ** (-cnr_db / 10.0))
    x = np.exp(1j * phase) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


_ROWS = {}


def case_words(name):
    seed, n_lines, _, _, _, _, image = CASES[name]
    return pass_words(n_lines, image, seed)


def case_row(name):
    """The case's row (made once; callers must not write to it)."""
    if name not in _ROWS:
        seed, n_lines, start, off, ppm, cnr, image = CASES[name]
        x = modulate(case_words(name), start, off, ppm, cnr, seed)
        x.setflags(write=False)
        _ROWS[name] = x
    return _ROWS[name]


def case_starts(name):
    """Where the lines' sync A starts in the envelope (float: the clock error moves them by fractions of a sample)."""
    _, n_lines, start, _, ppm, _, _ = CASES[name]
    return (start + np.arange(n_lines) * LINE_ROW / (1.0 + ppm * 1e-6)) / DECIM


def row_crc32(x):
    return zlib.crc32(np.ascontiguousarray(x).view(np.uint8).tobytes())


# ---- the NumPy statement of the three stages ------------------------------------------------------------------------------------------------
def numpy_front(d, taps, fs=float(RATE), decim=DECIM, lead=None):
    """The front behind the discriminator, in float64: d (the float32 discriminator, d[0] = 0) times exp(-2 pi i 2400 i / fs), the FIR
    y[m] = sum_k taps[k] z[m decim + lead - k] with z zero outside the row, and its magnitude -> float64 [ceil(n / decim)]."""
    d = np.asarray(d, np.float64)
    taps = np.asarray(taps, np.float64)
    n, T = len(d), len(taps)
    lead = (T - 1) // 2 if lead is None else lead
    i = np.arange(n, dtype=np.float64)
    z = d * np.exp(-2j * np.pi * ((SUBCARRIER / fs * i) % 1.0))
    full = np.convolve(z, taps)                      # full[j] = sum_k taps[k] z[j - k]
    m = np.arange(-(-n // decim))
    j = m * decim + lead
    return np.abs(np.where(j < len(full), full[np.minimum(j, len(full) - 1)], 0.0))


def candidates(env, sync_errors):
    """Every start of one float32 row with its test -> (s, mism, score) of the accepted ones.  float32 sums one at a time."""
    env = np.asarray(env, np.float32)
    n = len(env)
    ns = n - (REACH - 1)
    if ns <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    s = np.arange(ns)
    with np.errstate(all="ignore"):
        e = np.stack([env[3 * k + 1:3 * k + 1 + ns] for k in range(39)])          # e[k][s]
        t = e[4].copy()
        for k in range(5, 32):
            t = (t + e[k]).astype(np.float32)
        thr = (t / np.float32(28.0)).astype(np.float32)
        bits = e > thr[None, :]
        mism = (bits != SYNC_A[:, None].astype(bool)).sum(axis=0)
        hi = e[HIGH_K[0]].copy()
        for k in HIGH_K[1:]:
            hi = (hi + e[k]).astype(np.float32)
        lo = e[LOW_K[0]].copy()
        for k in LOW_K[1:]:
            lo = (lo + e[k]).astype(np.float32)
        score = ((hi - lo).astype(np.float32) / np.float32(14.0)).astype(np.float32)
    ok = mism <= sync_errors
    return s[ok], mism[ok], score[ok]


def numpy_syncs(env, sync_errors=2, s_begin=0, s_end=None, max_syncs=None):
    """pss_h_apt_syncs' answer on whole rows [n_rows][n] or [n] -> (row, pos, meta, score, count)."""
    env = np.asarray(env, np.float32)
    rows = env[None, :] if env.ndim == 1 else env
    n = rows.shape[1]
    s_end = n if s_end is None else s_end
    out = []
    for r in range(rows.shape[0]):
        s, mism, q = candidates(rows[r], sync_errors)
        for a in range(len(s)):
            if not s_begin <= s[a] < s_end:
                continue
            kept = True
            for b in range(len(s)):
                d = abs(int(s[b]) - int(s[a]))
                if d == 0 or d >= NEAR:
                    continue
                if mism[b] < mism[a] or (mism[b] == mism[a] and (q[b] > q[a] or (q[b] == q[a] and s[b] < s[a]))):
                    kept = False
                    break
            if kept:
                out.append((r, int(s[a]), int(mism[a]), q[a]))
    count = len(out)
    if max_syncs is not None:
        out = out[:max_syncs]
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out], np.uint32),
            np.array([o[3] for o in out], np.float32), count)


def numpy_lines(env, line_row, line_pos):
    """word[l][j] = env[row][p + 3 j + 1], +0 outside the row (and for a row that does not exist)."""
    env = np.asarray(env, np.float32)
    rows = env[None, :] if env.ndim == 1 else env
    n = rows.shape[1]
    out = np.zeros((len(line_pos), LINE_WORDS), np.float32)
    j = 3 * np.arange(LINE_WORDS) + 1
    for l, (r, p) in enumerate(zip(np.asarray(line_row).tolist(), np.asarray(line_pos).tolist())):
        r, p = int(r), int(p)
        if not 0 <= r < rows.shape[0] or p <= -LINE_ENV or p >= n:
            continue
        i = p + j
        ok = (i >= 0) & (i < n)
        out[l, ok] = rows[r, i[ok]]
    return out


def sync_env(n, starts, high=1.0, low=0.2, pattern=SYNC_A, base=None, full=False):
    """A float32 envelope row of n samples at `low` (or a copy of base) with the 39-word pattern planted at each start: a high word is
    high at its middle sample alone (the starts one sample either side then read 39 low words), or, with full, at all three samples."""
    e = np.full(n, low, np.float32) if base is None else np.array(base, np.float32)
    w = np.full(39 * ENV_SPW, low, np.float32)
    for k in np.flatnonzero(pattern):
        w[3 * k:3 * k + 3 if full else 3 * k + 2] = high if full else low
        w[3 * k + 1] = high
    for s in starts:
        e[s:s + len(w)] = w[:max(0, n - s)]
    return e


# ---- the shapes tests/test_gpu_apt.py, tests/test_gpu_start_list.py and tests/test_apt_shapes.py share (the caps are the callers': tests/apt_caps.py) ----
SHORT_N = 300                 # a row of one tile: 184 starts


def carrying(n_rows, grid_cap):
    """The rows of a batch of one-tile rows that carry a record: those of every other round of a detect grid of grid_cap workgroups, and
    the last.  A workgroup then meets tiles with, without, with, without survivors, and workgroup 0 a fifth that has them."""
    return [r for r in range(n_rows) if (r // grid_cap) % 2 == 0 or r == n_rows - 1]


def short_start(r, dense=False):
    """Where row r's record lies.  dense: the sync's three samples a word are all high, so the starts one sample either side score the same
    and the earliest stays."""
    s = (7 * r) % 183
    return max(s - 1, 0) if dense else s


def short_rows(n_rows, grid_cap, dense=False):
    """float32 [n_rows][300] for the detect grid's tile reuse, the counts' carry and the gather's second pass: one tile a row.  Plain: a
    sync at (7 r) % 183 in the carrying rows, 0.2 elsewhere (sync_errors 0: one survivor a sync).  dense: a full sync in EVERY row
    (sync_errors 4: nine survivors a sync where the row holds them all), so every tile has survivors and every row one record."""
    env = np.full((n_rows, SHORT_N), 0.2, np.float32)
    for r in (range(n_rows) if dense else carrying(n_rows, grid_cap)):
        env[r] = sync_env(SHORT_N, [(7 * r) % 183], full=dense)
    return env


def round_sample(n_rows, grid_cap):
    """The rows a CPU test restates: the first, the last, and the first, a middle and the last row of every round of the detect grid."""
    rows = {0, n_rows - 1}
    for r0 in range(0, n_rows, grid_cap):
        r1 = min(r0 + grid_cap, n_rows)
        rows |= {r0, (r0 + r1) // 2, r1 - 1}
    return sorted(rows)


def dense_train(n_tiles, strong):
    """float32 [n_tiles * TILE - 1000]: full syncs back to back (nine survivors a sync at sync_errors 4, equal scores: each is dropped by
    the one before it), a quiet stretch behind tile 5, and a sync of three times the height at every start in `strong`."""
    n = n_tiles * TILE - 1000
    unit = sync_env(REACH, [0], full=True)
    env = np.tile(unit, n // REACH + 1)[:n].copy()
    env[5 * TILE:5 * TILE + 3 * NEAR] = 0.2
    for s in strong:
        env[s:s + REACH] = sync_env(REACH, [0], high=3.0)
    return env


GRID_DECIMS = (1, 2, 3, 5, 8, 13, 64, 100, 1000, 4096)
GRID_TAPS = (1, 2, 63, 64, 65, 128, 129, 1000, 4097)


def grid_case(decim, n_taps, tile):
    """k_apt_front's grid point (decim, n_taps), `tile` = its outputs a tile: (the first decim (2 tile + 3) samples of the noisy case's
    row: two whole tiles and one of three outputs; seeded taps)."""
    x = case_row("noise_10db_3khz_40ppm")[:decim * (2 * tile + 3)]
    assert len(x) == decim * (2 * tile + 3)
    taps = np.random.default_rng([decim, n_taps]).standard_normal(n_taps) / np.sqrt(n_taps)
    return x, taps


def halo(m0, m1, decim, n_taps, n):
    """The samples [lo, hi) of a row of n that the outputs [m0, m1) need at the default lead: the taps' span and the discriminator's one
    sample before it."""
    lead = (n_taps - 1) // 2
    return max(0, m0 * decim + lead - (n_taps - 1) - 1), min(n, (m1 - 1) * decim + lead + 1)

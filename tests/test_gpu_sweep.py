"""The scanner sweep report on the GPU: pss_scan_gate, pss_classify_gated, pss_sweep_report.  Every comparison is equality of bits, bytes or
strings: the gate against its host twin pss_h_scan_gate, the gated classifier against pss_classify of the whole batch, the one-call sweep
against the separate calls and against tests/golden/sweep.npz (the reference's own sweeps, records and drawn lines).

New capped grids, each walked one item past its cap here: k_scan_flags / k_scan_index (4096 workgroups of 256 slices), k_cls_modidx_gated /
k_cls_welch_gated (16 384 workgroups of one listed frame).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_util as G
import sweep_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats
from pyspecsdr_amd.engine import h_scan_gate

FS = S.FS
GATE_TILE = 256
GATE_CAP_SLICES = 4096 * GATE_TILE      # pss_squelch.hip: k_scan_flags / k_scan_index
CLS_CAP_FRAMES = 16384                  # pss_demod.hip: the classifier's grids
SENT32 = 0x7F7F7F7F


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep.npz"))


def sentinel(shape, dtype):
    """A device buffer of 0x7f bytes: a value the kernels never produce, so an element never written fails."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0x7F)
    return t


def is_sentinel(t):
    return bool((t.contiguous().view(torch.uint8) == 0x7F).all())


def dev(a):
    return G.dev(np.array(a))      # a copy: the shared inputs are read-only


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- gate -----------------------------------------------------------------------------------------------------------------------------
def random_pairs(n, seed, threshold, min_bw):
    """(peak float32, bw float64) around the two limits, seeded with the values a comparison can get wrong."""
    rng = np.random.default_rng(seed)
    cast = np.float32(threshold)
    peak = (float(cast) + 8.0 * rng.standard_normal(n)).astype(np.float32)
    bw = min_bw + 40e3 * rng.standard_normal(n)
    k = max(n // 50, 1)
    pos = rng.integers(0, n, (11, k))
    peak[pos[0]], peak[pos[1]], peak[pos[2]] = np.nan, np.inf, -np.inf
    peak[pos[3]] = cast
    peak[pos[4]], peak[pos[5]] = np.nextafter(cast, np.float32(np.inf)), np.nextafter(cast, np.float32(-np.inf))
    bw[pos[6]], bw[pos[7]], bw[pos[8]] = np.nan, np.inf, -np.inf
    bw[pos[9]] = min_bw
    bw[pos[10]] = np.nextafter(min_bw, np.inf)
    return peak, bw


def gate_on_device(peak, bw, threshold, min_bw, want_hit=True, want_idx=True):
    e = G.engine()
    n = len(peak)
    d_hit = sentinel((max(n, 1),), torch.uint8) if want_hit else None
    d_idx = sentinel((max(n, 1),), torch.int32) if want_idx else None
    n_hit = e.scan_gate(dev(peak) if n else None, dev(bw) if n else None, n, threshold, min_bw, d_hit, d_idx)
    return (G.host(d_hit)[:n] if want_hit else None), (G.host(d_idx)[:n] if want_idx else None), n_hit


def check_gate(peak, bw, threshold, min_bw):
    want_hit, want_idx = h_scan_gate(peak, bw, threshold, min_bw)
    hit, idx, n_hit = gate_on_device(peak, bw, threshold, min_bw)
    assert n_hit == len(want_idx)
    assert np.array_equal(hit, want_hit)
    assert np.array_equal(idx[:n_hit], want_idx), "hit list: ascending and complete"
    assert np.all(idx[n_hit:] == SENT32), "nothing written past the count"
    return n_hit


@pytest.mark.parametrize("threshold,min_bw", [(-30.05, 50e3), (0.0, 50e3), (20.5, 12.5e3)])
def test_gate_equals_the_host_gate_on_a_million_pairs(threshold, min_bw):
    n = 1_000_000
    peak, bw = random_pairs(n, 7, threshold, min_bw)
    n_hit = check_gate(peak, bw, threshold, min_bw)
    assert n // 8 < n_hit < n // 2
    cast = np.float32(threshold)
    on = np.flatnonzero((peak == cast) & (bw > min_bw))
    up = np.flatnonzero((peak == np.nextafter(cast, np.float32(np.inf))) & (bw > min_bw))
    assert len(on) and len(up)
    hit = h_scan_gate(peak, bw, threshold, min_bw)[0]
    assert not hit[on].any() and hit[up].all(), "the comparison runs in float32 against the cast threshold"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, GATE_TILE - 1, GATE_TILE, GATE_TILE + 1, 1000, GATE_CAP_SLICES + 1])
def test_gate_slice_counts_around_wavefront_tile_and_grid_cap(n):
    peak, bw = random_pairs(max(n, 400), 100 + n % 97, -10.0, 50e3)
    n_hit = check_gate(peak[:n], bw[:n], -10.0, 50e3)
    assert n < 63 or 0 < n_hit < n
    assert check_gate(peak[:n], bw[:n], np.inf, 50e3) == 0
    if n:
        ones_p, ones_b = np.full(n, 1.0, np.float32), np.full(n, 60e3)
        assert check_gate(ones_p, ones_b, 0.0, 50e3) == n           # every slice a hit: the list is 0 .. n - 1


def test_gate_with_null_outputs():
    peak, bw = random_pairs(70_000, 3, 0.0, 50e3)
    want_hit, want_idx = h_scan_gate(peak, bw, 0.0, 50e3)
    hit, idx, n_hit = gate_on_device(peak, bw, 0.0, 50e3, want_idx=False)
    assert idx is None and n_hit == len(want_idx) and np.array_equal(hit, want_hit)
    hit, idx, n_hit = gate_on_device(peak, bw, 0.0, 50e3, want_hit=False)
    assert hit is None and n_hit == len(want_idx) and np.array_equal(idx[:n_hit], want_idx) and np.all(idx[n_hit:] == SENT32)
    hit, idx, n_hit = gate_on_device(peak, bw, 0.0, 50e3, want_hit=False, want_idx=False)
    assert n_hit == len(want_idx)


# ---- gated classifier -------------------------------------------------------------------------------------------------------------------
_batches = {}


def batch(n, count=70):
    """`count` slices of n samples interleaving the fixture's slices (every case at least n long; a repeat is rolled, not copied)."""
    if (n, count) not in _batches:
        pools = [S.slices(c) for c in S.CASES if c.n >= n]
        rows = []
        for i in range(count):
            pool = pools[i % len(pools)]
            rows.append(np.roll(pool[(i // len(pools)) % len(pool)][:n], 37 * (i // (len(pools) * len(pool)))))
        x = np.stack(rows).astype(np.complex64)
        x.setflags(write=False)
        _batches[(n, count)] = x
    return _batches[(n, count)]


_classified = {}


def classify_all(n):
    """pss_classify of batch(n): (device IQ, label, bw, mi, flat, psd) — computed once, shared, left unchanged."""
    if n not in _classified:
        e, x = G.engine(), batch(n)
        nf = len(x)
        d_iq = dev(x)
        out = [G.empty((nf,), torch.int32), G.empty((nf,), torch.float64), G.empty((nf,), torch.float32), G.empty((nf,), torch.float32),
               G.empty((nf, 1024), torch.float32)]
        for t in out:
            t.view(torch.uint8).fill_(0x7F)       # psd rows of a short read hold n bins: the rest must match as left
        e.classify(d_iq, nf, n, FS, *out)
        e.sync()
        _classified[n] = (d_iq,) + tuple(G.host(t) for t in out)
    return _classified[n]


def gated(d_iq, nf, n, idx, pad=3, which=(True,) * 5):
    e = G.engine()
    n_idx = len(idx)
    rows = n_idx + pad
    dtypes = (torch.int32, torch.float64, torch.float32, torch.float32, torch.float32)
    out = [sentinel((rows, 1024) if k == 4 else (rows,), dt) if w else None for k, (dt, w) in enumerate(zip(dtypes, which))]
    d_idx = dev(np.asarray(idx, np.int32)) if n_idx else None
    e.classify_gated(d_iq, nf, n, FS, d_idx, n_idx, *out)
    e.sync()
    return out


def lists(nf):
    return {"empty": [], "first": [0], "last": [nf - 1], "every other": list(range(0, nf, 2)), "all but one": [i for i in range(nf) if i != 31],
            "all": list(range(nf)), "descending with repeats": [nf - 1, 5, 5, 0, 17]}


@pytest.mark.parametrize("n", [600, 1024, 1500, 4096, 24000])
def test_classify_gated_equals_classify_of_the_batch(n):
    d_iq, *want = classify_all(n)
    nf = len(want[0])
    assert nf == 70
    for name, idx in lists(nf).items():
        out = gated(d_iq, nf, n, idx)
        for k, (t, w) in enumerate(zip(out, want)):
            got = G.host(t)
            assert same_bytes(got[:len(idx)], w[np.asarray(idx, np.int64)]), (n, name, k)
            assert is_sentinel(t[len(idx):]), (n, name, k, "rows past n_idx stay untouched")
    if n >= 1024:
        labels = set(want[0].tolist())
        assert len(labels) >= 2, "the batch exercises more than one branch of the decision tree"


def test_classify_gated_clamps_indices_and_takes_null_outputs():
    n = 1500
    d_iq, *want = classify_all(n)
    nf = len(want[0])
    idx = [-5, 3, nf, nf + 1000, 2 ** 31 - 1, -2 ** 31]
    clamped = [0, 3, nf - 1, nf - 1, nf - 1, 0]
    out = gated(d_iq, nf, n, idx)
    for t, w in zip(out, want):
        assert same_bytes(G.host(t)[:len(idx)], w[clamped])
    for k in range(5):                                               # each output alone
        which = tuple(j == k for j in range(5))
        out = gated(d_iq, nf, n, [4, 9, 60], which=which)
        assert same_bytes(G.host(out[k])[:3], want[k][[4, 9, 60]]) and is_sentinel(out[k][3:])
    gated(d_iq, nf, n, [4, 9], which=(False,) * 5)                   # nothing asked for: still a valid call


def test_classify_gated_one_slice_past_the_grid_cap():
    e = G.engine()
    n, nf = 1024, CLS_CAP_FRAMES + 2
    base = batch(1024)
    rng = np.random.default_rng(8)
    pick = rng.integers(0, len(base), nf)
    d_iq = dev(base)[torch.from_numpy(pick).cuda()].contiguous()
    d_iq += torch.from_numpy((1e-4 * rng.standard_normal((nf, 1))).astype(np.float32)).cuda()     # no two slices alike
    want = [G.empty((nf,), torch.int32), G.empty((nf,), torch.float64), G.empty((nf,), torch.float32), G.empty((nf,), torch.float32),
            G.empty((nf, 1024), torch.float32)]
    e.classify(d_iq, nf, n, FS, *want)
    idx = np.delete(np.arange(nf), 4097)                             # all but one: 16 385 listed slices
    assert len(idx) == CLS_CAP_FRAMES + 1
    out = gated(d_iq, nf, n, idx, pad=1)
    sel = torch.from_numpy(idx).cuda()
    for k, (t, w) in enumerate(zip(out, want)):
        assert torch.equal(t[:len(idx)].view(torch.uint8), w[sel].contiguous().view(torch.uint8)), k
        assert is_sentinel(t[len(idx):])
    assert len(set(G.host(want[2]).tolist())) > nf // 2


# ---- one call per sweep -------------------------------------------------------------------------------------------------------------------
KINDS = {"inline": L.SWEEP_INLINE, "driver": L.SWEEP_DRIVER}


def separate_calls(kind, d_iq, ns, n, threshold, min_bw):
    """What a caller does without pss_sweep_report: the scan, the gate, the gated classifier."""
    e = G.engine()
    d_db, d_peak, d_bw, d_count = G.empty((ns, n), torch.float32), G.empty((ns,), torch.float32), G.empty((ns,), torch.float64), G.empty((ns,), torch.int32)
    if kind == "inline":
        e.scan(d_iq, ns, n, FS, d_db, d_peak, d_bw, d_count)
    else:
        e.scan_threshold(d_iq, ns, n, FS, threshold, d_db, d_peak, d_bw, d_count)
    d_hit, d_idx = G.empty((ns,), torch.uint8), sentinel((ns,), torch.int32)
    n_hit = e.scan_gate(d_peak, d_bw, ns, threshold, min_bw, d_hit, d_idx)
    cls = [sentinel((ns,), torch.int32), sentinel((ns,), torch.float64), sentinel((ns,), torch.float32), sentinel((ns,), torch.float32)]
    e.classify_gated(d_iq, ns, n, FS, d_idx, n_hit, *cls)
    e.sync()
    return dict(db=G.host(d_db), peak=G.host(d_peak), bw=G.host(d_bw), count=G.host(d_count), hit=G.host(d_hit), idx=G.host(d_idx), n_hit=n_hit,
                cls=[G.host(t) for t in cls])


def report(kind, d_iq, ns, n, threshold, min_bw, nullable=True):
    e = G.engine()
    d_peak, d_bw, d_idx = sentinel((ns,), torch.float32), sentinel((ns,), torch.float64), sentinel((ns,), torch.int32)
    opt = dict(d_db=sentinel((ns, n), torch.float32), d_count=sentinel((ns,), torch.int32), d_hit=sentinel((ns,), torch.uint8),
               d_label=sentinel((ns,), torch.int32), d_cls_bw=sentinel((ns,), torch.float64), d_mi=sentinel((ns,), torch.float32),
               d_flat=sentinel((ns,), torch.float32)) if nullable else {}
    n_hit = e.sweep_report(kind, d_iq, ns, n, FS, threshold, d_peak, d_bw, d_idx, min_bw, **opt)
    e.sync()
    r = dict(peak=G.host(d_peak), bw=G.host(d_bw), idx=G.host(d_idx), n_hit=n_hit)
    if nullable:
        r.update(db=G.host(opt["d_db"]), count=G.host(opt["d_count"]), hit=G.host(opt["d_hit"]),
                 cls=[G.host(opt[k]) for k in ("d_label", "d_cls_bw", "d_mi", "d_flat")])
    return r


def same_report(r, s):
    assert r["n_hit"] == s["n_hit"]
    for k in ("peak", "bw", "idx") + (("db", "count", "hit") if "db" in r else ()):
        assert same_bytes(r[k], s[k]), k
    if "cls" in r:
        for a, b in zip(r["cls"], s["cls"]):
            assert same_bytes(a, b)                                  # the filled rows and the sentinels behind them


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_sweep_report_equals_the_golden_sweep_and_the_separate_calls(name, gold):
    c = S.case(name)
    x = S.slices(c)
    assert S.crc(x) == int(gold[f"crc_{name}"])
    ns, d_iq = len(x), dev(x)
    for kind in ("inline", "driver"):
        s = separate_calls(kind, d_iq, ns, c.n, c.threshold, S.MIN_BW)
        r = report(kind, d_iq, ns, c.n, c.threshold, S.MIN_BW)
        same_report(r, s)
        assert np.all(r["idx"][r["n_hit"]:] == SENT32) and all(np.all(a[r["n_hit"]:].view(np.uint8) == 0x7F) for a in r["cls"])
        bare = report(kind, d_iq, ns, c.n, c.threshold, S.MIN_BW, nullable=False)      # every nullable output null
        same_report(bare, s)
        if kind != c.kind:
            continue
        n_hit = r["n_hit"]
        assert same_bytes(r["peak"], gold[f"peak_{name}"]) and same_bytes(r["bw"], gold[f"bw_{name}"])
        assert np.array_equal(r["count"], gold[f"count_{name}"])
        assert np.array_equal(r["hit"], gold[f"hit_{name}"]) and np.array_equal(r["idx"][:n_hit], gold[f"hit_idx_{name}"])
        labels = [G.engine().class_name(v) for v in r["cls"][0][:n_hit]]
        assert labels == [str(t) for t in gold[f"labels_{name}"]]
        freqs = formats.sweep_frequencies(c.start, S.sweep_end(c), c.step)
        assert same_bytes(freqs, gold[f"freqs_{name}"])
        signals = formats.scan_signals(freqs, r["peak"], r["bw"], r["idx"][:n_hit], r["cls"][0][:n_hit])
        check_records(signals, gold, f"rec_{name}")
        if c.kind == "driver":
            signals = formats.scan_signals(freqs, r["peak"], r["bw"], r["idx"][:n_hit], r["cls"][0][:n_hit], dedupe=True)
            check_records(signals, gold, f"ded_{name}")
        for hw in S.SCREENS:
            for page in range((len(signals) + hw[0] - 8) // (hw[0] - 7)):
                key = S.lines_key(c, hw, page)
                want = [(int(y), int(xx), str(t), int(p), bool(b)) for y, xx, t, p, b in
                        zip(gold[key + "_y"], gold[key + "_x"], gold[key + "_text"], gold[key + "_pair"], gold[key + "_bold"])]
                assert formats.scan_result_lines(signals, hw[0], hw[1], page) == want, (name, hw, page)


def check_records(signals, gold, prefix):
    assert len(signals) == len(gold[prefix + "_freq"])
    for s, f, p, b, t in zip(signals, gold[prefix + "_freq"], gold[prefix + "_power"], gold[prefix + "_bw"], gold[prefix + "_type"]):
        assert type(s['frequency']) is float and type(s['power']) is np.float32 and type(s['bandwidth']) is np.float64
        assert s['frequency'] == float(f) and s['power'].tobytes() == p.tobytes() and s['bandwidth'].tobytes() == b.tobytes() and s['type'] == str(t)


def test_sweep_report_with_no_hit_and_with_every_slice_a_hit(gold):
    c = S.case("inline_2048")
    x = S.slices(c)
    d_iq = dev(x)
    for kind in ("inline", "driver"):
        r = report(kind, d_iq, len(x), c.n, 200.0, S.MIN_BW)
        assert r["n_hit"] == 0 and not r["hit"].any() and np.all(r["idx"] == SENT32)
        assert all(np.all(a.view(np.uint8) == 0x7F) for a in r["cls"]), "no detection: the classifier's outputs stay untouched"
        same_report(r, separate_calls(kind, d_iq, len(x), c.n, 200.0, S.MIN_BW))
    hits = x[gold["hit_idx_inline_2048"]]
    d_hits = dev(hits)
    for kind, threshold in (("inline", c.threshold), ("driver", -40.0)):
        r = report(kind, d_hits, len(hits), c.n, threshold, S.MIN_BW)
        assert r["n_hit"] == len(hits) and r["hit"].all() and np.array_equal(r["idx"], np.arange(len(hits)))
        same_report(r, separate_calls(kind, d_hits, len(hits), c.n, threshold, S.MIN_BW))
    labels = [G.engine().class_name(v) for v in r["cls"][0]]
    assert labels == [str(t) for t in gold["labels_inline_2048"]]
    e = G.engine()
    d_idx = sentinel((4,), torch.int32)
    assert e.sweep_report("inline", None, 0, c.n, FS, 0.0, None, None, d_idx) == 0 and is_sentinel(d_idx)      # an empty sweep


def test_sweep_report_on_a_seeded_batch_of_300_slices():
    n, ns = 2048, 300
    rng = np.random.default_rng(2024)
    base = batch(2048, 48)
    x = base[rng.integers(0, len(base), ns)] * rng.uniform(0.05, 1.0, (ns, 1)).astype(np.float32)
    x = (x + 0.002 * (rng.standard_normal((ns, n)) + 1j * rng.standard_normal((ns, n)))).astype(np.complex64)
    d_iq = dev(x)
    for kind, threshold in (("inline", -5.0), ("driver", 0.0), ("driver", 12.25)):
        s = separate_calls(kind, d_iq, ns, n, threshold, S.MIN_BW)
        assert 0 < s["n_hit"] < ns
        same_report(report(kind, d_iq, ns, n, threshold, S.MIN_BW), s)
        want_hit, want_idx = h_scan_gate(s["peak"], s["bw"], threshold, S.MIN_BW)
        assert np.array_equal(s["hit"], want_hit) and np.array_equal(s["idx"][:s["n_hit"]], want_idx)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
def raises_arg(fn, *args, **kw):
    with pytest.raises(Exception) as ei:
        fn(*args, **kw)
    assert getattr(ei.value, "code", None) == L.PSS_E_ARG, ei.value


def test_argument_errors_on_every_new_entry_point():
    e = G.engine()
    n, ns = 2048, 8
    d_iq = dev(batch(2048)[:ns])
    d_peak, d_bw, d_idx = G.empty((ns,), torch.float32), G.empty((ns,), torch.float64), G.empty((ns,), torch.int32)
    d_peak.zero_(); d_bw.zero_(); d_idx.zero_()
    raises_arg(e.scan_gate, None, d_bw, ns, 0.0)
    raises_arg(e.scan_gate, d_peak, None, ns, 0.0)
    raises_arg(e.scan_gate, d_peak, d_bw, -1, 0.0)
    raises_arg(e.scan_gate, d_peak, d_bw, 1 << 31, 0.0)
    assert e.scan_gate(None, None, 0, 0.0) == 0
    raises_arg(e.classify_gated, d_iq, ns, n, FS, d_idx, -1)
    raises_arg(e.classify_gated, d_iq, ns, n, FS, d_idx, ns + 1)
    raises_arg(e.classify_gated, d_iq, ns, n, FS, None, 3)
    raises_arg(e.classify_gated, None, ns, n, FS, d_idx, 3)
    raises_arg(e.classify_gated, d_iq, ns, 0, FS, d_idx, 3)
    raises_arg(e.classify_gated, d_iq, ns, n, 0.0, d_idx, 3)
    raises_arg(e.classify_gated, d_iq, -1, n, FS, d_idx, 0)
    e.classify_gated(d_iq, ns, n, FS, None, 0)                      # an empty list needs no list
    raises_arg(e.sweep_report, 2, d_iq, ns, n, FS, 0.0, d_peak, d_bw, d_idx)
    raises_arg(e.sweep_report, -1, d_iq, ns, n, FS, 0.0, d_peak, d_bw, d_idx)
    raises_arg(e.sweep_report, "inline", None, ns, n, FS, 0.0, d_peak, d_bw, d_idx)
    raises_arg(e.sweep_report, "inline", d_iq, ns, n, FS, 0.0, None, d_bw, d_idx)
    raises_arg(e.sweep_report, "driver", d_iq, ns, n, FS, 0.0, d_peak, None, d_idx)
    raises_arg(e.sweep_report, "driver", d_iq, ns, n, FS, 0.0, d_peak, d_bw, None)
    raises_arg(e.sweep_report, "inline", d_iq, -1, n, FS, 0.0, d_peak, d_bw, d_idx)
    raises_arg(e.sweep_report, "inline", d_iq, 1 << 31, n, FS, 0.0, d_peak, d_bw, d_idx)
    raises_arg(e.sweep_report, "inline", d_iq, ns, n, 0.0, 0.0, d_peak, d_bw, d_idx)
    raises_arg(e.sweep_report, "driver", d_iq, ns, 1, FS, 0.0, d_peak, d_bw, d_idx)
    e.sync()

"""The OOK kernels (k_ook_envelope, k_ook_levels, k_ook_detect, pss_starts.h's k_starts_scan and k_starts_gather, k_ook_heads, k_ook_list,
k_ook_walk, k_ook_emit) against the host twins on every byte of every output, and formats.ook_recording end to end.  Buffers lie between NaNs,
rows are strided with NaNs in the gaps, and a sentinel sits behind max_msgs.  The shapes are tests/ook_cases.py's shape_cases and
window_cases, the smallest at which each path can go wrong (tests/test_ook_shapes.py runs the same arrays through the host twin against the
NumPy statement first); the caps and tile sizes they are sized by are pinned to the source lines by tests/test_ook_caps.py."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ook_cases as K
from bytes_util import same_bytes
from gpu_util import dev
from ook_caps import TILE
from pyspecsdr_amd import formats as F
from pyspecsdr_amd.engine import Engine, PssError

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
WHAT = ("bits", "n_bits", "row", "pos", "span", "meta")
CASES = K.shape_cases()
assert K.TILE == TILE


@pytest.fixture(scope="module")
def e():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    eng = Engine(0)
    yield eng
    eng.close()


def strided(rows, gap):
    """complex64 [R][n] -> a flat device tensor of float32 pairs holding the rows `n + gap` samples apart between NaNs, two samples of NaN in
    front; -> (tensor, byte offset of row 0, stride in samples)."""
    rows = np.ascontiguousarray(rows, np.complex64)
    r, n = rows.shape
    stride = n + gap
    wide = np.full(2 + r * stride + 2, complex(np.nan, np.nan), np.complex64)
    for k in range(r):
        wide[2 + k * stride:2 + k * stride + n] = rows[k]
    return dev(wide), 16, stride


def on_device(e, rows, hi, lo, spec, P, R, buf_index0=0, n_row=None, s_begin=0, s_end=None, max_msgs=None, gap=3):
    """h_ook_messages' result from the device."""
    rows = np.atleast_2d(rows)
    r, n = rows.shape
    d_x, off, stride = strided(rows, gap)
    mm = 16384 if max_msgs is None else max_msgs
    room = mm + 3
    d_bits = torch.full((room, 32), SENTINEL, dtype=torch.uint8, device="cuda")
    d_nb, d_row, d_span, d_meta = (torch.full((room,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
    d_pos = torch.full((room,), -7, dtype=torch.int64, device="cuda")
    d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    e.ook_messages(d_x.data_ptr() + off, r, n, hi, lo, spec, d_bits, d_nb, d_row, d_pos, d_span, d_meta, d_count, mm, P=P, R=R, x_stride=stride,
                   buf_index0=buf_index0, n_row=n_row, s_begin=s_begin, s_end=s_end)
    e.sync()
    bits, nb, rw, pos, sp, meta, count = (t.cpu().numpy() for t in (d_bits, d_nb, d_row, d_pos, d_span, d_meta, d_count))
    assert count[1] == -7
    k = min(int(count[0]), mm)
    assert np.all(bits[k:] == SENTINEL) and np.all(nb[k:] == -7) and np.all(rw[k:] == -7) and np.all(pos[k:] == -7) and np.all(sp[k:] == -7)
    assert np.all(meta[k:] == -7)
    return bits[:k], nb[:k], rw[:k], pos[:k], sp[:k], meta[:k].view(np.uint32), int(count[0])


def check(e, rows, hi, lo, spec, P, R, max_msgs=None, **kw):
    """Device == twin on every byte -> the twin's result."""
    want = Engine.h_ook_messages(rows, hi, lo, spec, P=P, R=R, max_msgs=16384 if max_msgs is None else max_msgs, **kw)
    got = on_device(e, rows, hi, lo, spec, P, R, max_msgs=max_msgs, **kw)
    assert got[6] == want[6]
    for g, w, what in zip(got[:6], want[:6], WHAT):
        assert same_bytes(g, w), (what, g, w)
    return want


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c['name'] for c in CASES])
def test_shapes(e, k):
    c = CASES[k]
    check(e, c['rows'], c['hi'], c['lo'], c['spec'], c['P'], c['R'], max_msgs=c.get('max_msgs'))


@pytest.mark.parametrize("w", K.window_cases(), ids=lambda w: w[0])
def test_windows_with_exactly_their_reach(e, w):
    _, buf, buf_index0, n_row, s_begin, s_end, spec, P, R, _, _ = w
    r = check(e, buf, K.HI, K.LO, spec, P, R, buf_index0=buf_index0, n_row=n_row, s_begin=s_begin, s_end=s_end)
    assert r[6] > 0 and np.all((r[3] >= s_begin) & (r[3] < s_end))
    with pytest.raises(PssError, match="pss_ook_messages: the buffer does not cover the window's reach"):
        on_device(e, buf[:, 1:], K.HI, K.LO, spec, P, R, buf_index0=buf_index0 + 1, n_row=n_row, s_begin=s_begin, s_end=s_end)


@pytest.mark.parametrize("P", [1, 2, 9, 65])
def test_envelope_and_levels(e, P):
    rows, _, _ = K.small_rows()
    rows = np.concatenate([rows, K.level_row(rows.shape[1], 3)[None, :]])
    r, n = rows.shape
    d_x, off, stride = strided(rows, 5)
    d_env = torch.full((r, n + 2), -7.0, dtype=torch.float32, device="cuda")
    e.ook_envelope(d_x.data_ptr() + off, r, n, d_env, P=P, x_stride=stride, env_stride=n + 2)
    nb = n // K.BLOCK
    d_means = torch.full((r, nb + 1), -7.0, dtype=torch.float64, device="cuda")
    e.ook_levels(d_x.data_ptr() + off, r, n, d_means, x_stride=stride, means_stride=nb + 1)
    e.sync()
    env, means = d_env.cpu().numpy(), d_means.cpu().numpy()
    assert np.all(env[:, n:] == -7.0) and np.all(means[:, nb:] == -7.0)
    assert same_bytes(env[:, :n], Engine.h_ook_envelope(rows, P=P))
    assert same_bytes(means[:, :nb], Engine.h_ook_levels(rows))
    # a window of both, the buffer holding exactly its reach
    i0, i1 = 5000, 9001
    lo_i = i0 - (P - 1)
    d_w = torch.full((r, i1 - i0), -7.0, dtype=torch.float32, device="cuda")
    e.ook_envelope(d_x.data_ptr() + off + 8 * lo_i, r, i1 - lo_i, d_w, P=P, x_stride=stride, buf_index0=lo_i, n_row=n, i_begin=i0, i_end=i1)
    d_m = torch.full((r, 1), -7.0, dtype=torch.float64, device="cuda")
    e.ook_levels(d_x.data_ptr() + off + 8 * K.BLOCK, r, K.BLOCK, d_m, x_stride=stride, buf_index0=K.BLOCK, n_row=n, b_begin=1, b_end=2)
    e.sync()
    assert same_bytes(d_w.cpu().numpy(), env[:, i0:i1]) and same_bytes(d_m.cpu().numpy(), means[:, 1:2])


@pytest.fixture(scope="module", params=[f for f in K.FIXTURES if f[1] == 15], ids=lambda f: f[0])
def fixture15(request):
    return K.burst_fixture(*request.param) + (request.param[0],)


def test_fixture_on_the_device(e, fixture15):
    x, sent, spec, _ = fixture15
    d_x = dev(x)
    nb = len(x) // K.BLOCK
    d_means = torch.empty((1, nb), dtype=torch.float64, device="cuda")
    e.ook_levels(d_x, 1, len(x), d_means)
    e.sync()
    means = d_means.cpu().numpy()
    assert same_bytes(means, Engine.h_ook_levels(x))
    hi, lo = F.ook_levels(means[0])
    r = check(e, x, hi, lo, spec, 9, 64)
    assert [K.bits_of(b, n) for b, n in zip(r[0], r[1])] == sent


def test_recording_end_to_end(e, fixture15):
    x, sent, _, kind = fixture15
    name = {'ppm': 'nexus', 'pwm': 'ev1527'}[kind]
    want = F.h_ook_rows(x, K.FS)
    assert [(m['name'], m['bits'], m['count']) for m in want['messages']] == [(name, sent[k], 3) for k in range(0, len(sent), 3)]
    assert all(m['fields']['model'] == name and 'id' in m['fields'] for m in want['messages'])
    for chunk in (K.TILE, 1_000_003, len(x)):
        got = F.ook_recording(x, K.FS, chunk_samples=chunk)
        assert got['records'] == want['records'] and got['messages'] == want['messages'] and got['lines'] == want['lines'], chunk
        assert got['levels'] == want['levels']
    # cu8 codes: the same bytes as the complex64 path on the widened capture
    codes = np.clip(np.round(x.view(np.float32) * 6.0 + 127.5), 0, 255).astype(np.uint8).reshape(-1, 2)
    wide = F.unpack_iq(codes, "cu8")
    a = F.ook_recording(codes, K.FS, codes_format="cu8", chunk_samples=1_000_003)
    b = F.h_ook_rows(wide, K.FS)
    assert a['records'] == b['records'] and a['messages'] == b['messages'] and [m['bits'] for m in a['messages']] == [sent[k] for k in range(0, len(sent), 3)]


def test_rows_and_channels_on_the_device(e):
    """formats.ook_rows on resident rows, and formats.ook_recording's channel branch (pss_ddc, then ook_rows): two channels of one capture,
    each with its own thresholds, against h_ook_rows on the same rows; streamed tuning at two chunk sizes."""
    x, fs, center, channels, sent = K.channel_capture()
    rows, rate, _ = F.tune_recording(x, fs, np.array(channels) - center, 4)
    assert rate == K.FS and rows.shape == (2, len(x) // 4)
    want = F.h_ook_rows(rows, rate)
    assert [(m['row'], m['name'], m['bits'], m['count']) for m in want['messages'] if m['row'] == 0] == [(0, 'nexus', b, 3) for b in sent[0]]
    assert [(m['row'], m['name'], m['bits'], m['count']) for m in want['messages'] if m['row'] == 1] == [(1, 'ev1527', b, 3) for b in sent[1]]
    assert len(want['levels']) == 2 and want['levels'][0] != want['levels'][1]
    got = F.ook_rows(rows, rate)
    assert got == want
    d_rows = dev(rows)
    assert F.ook_rows(d_rows, rate) == want
    for chunk in (1 << 22, 300_001):
        rec = F.ook_recording(x, fs, center_hz=center, channels_hz=channels, decim=4, chunk_samples=chunk)
        assert rec == want, chunk

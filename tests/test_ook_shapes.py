"""The inputs of tests/test_gpu_ook.py's shape and window cases on the CPU: the host twin against the NumPy statement of tests/ook_cases.py on
every array, so that "device = twin" there and "twin = statement" here meet on the same bytes, and the shapes are known good before a GPU
sees them.  No GPU."""
import numpy as np
import pytest

import ook_cases as K
from bytes_util import same_bytes
from pyspecsdr_amd.engine import Engine as E

WHAT = ("bits", "n_bits", "row", "pos", "span", "meta")
CASES = K.shape_cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c['name'] for c in CASES])
def test_twin_is_the_statement(k):
    c = CASES[k]
    want = K.messages(c['rows'], c['hi'], c['lo'], c['spec'], c['P'], c['R'])
    twin = E.h_ook_messages(c['rows'], c['hi'], c['lo'], c['spec'], P=c['P'], R=c['R'], max_msgs=c.get('max_msgs'))
    room = len(twin[0])
    assert twin[6] == len(want[0]) and room == (twin[6] if c.get('max_msgs') is None else min(twin[6], c['max_msgs']))
    for t, w, what in zip(twin[:6], want, WHAT):
        assert same_bytes(t, w[:room]), (what, t, w)


def test_the_cases_reach_what_they_are_there_for():
    got = {c['name']: E.h_ook_messages(c['rows'], c['hi'], c['lo'], c['spec'], P=c['P'], R=c['R'], max_msgs=c.get('max_msgs')) for c in CASES}
    flags = {name: int(np.bitwise_or.reduce(r[5] & np.uint32(0xFFC00000))) if len(r[5]) else 0 for name, r in got.items()}
    assert flags['pulses1023'] == K.FULL and flags['pulses1024'] == K.FULL and flags['pulses1025'] == K.FULL | K.MANY
    assert [int(got[f'pulses{k}'][5][0]) & 0x7FF for k in (1023, 1024, 1025)] == [1023, 1024, 1024]
    assert [(int(got[f'bits{k}'][1][0]), flags[f'bits{k}']) for k in (255, 256, 257)] == [(255, 0), (256, 0), (256, K.FULL)]
    assert [(int(got[f'ppm_bits{k}'][1][0]), flags[f'ppm_bits{k}']) for k in (255, 256, 257)] == [(255, 0), (256, 0), (256, K.FULL)]
    assert flags['span41'] == 0 and flags['span40'] == K.LONG and int(got['span40'][1][0]) == 3 and int(got['span41'][1][0]) == 4
    assert flags['span36'] == 0 and flags['span35'] == 0          # the last rise is not read: nothing is cut short
    r = got['open_and_zero']
    assert r[2].tolist() == [0, 0, 1, 2, 2] and r[3].tolist() == [0, 2 * K.TILE - 4, 0, 0, 2 * K.TILE - 4]
    assert [int(m) & K.OPEN for m in r[5]] == [0, K.OPEN, 0, 0, K.OPEN] and r[4].tolist()[1] == 4
    assert flags['alternate'] == K.MANY | K.FULL and got['many_edges'][6] == 1 and got['many_messages'][6] > 8192
    assert got['over_max'][6] == 5 and len(got['over_max'][0]) == 2 and got['max0'][6] == 5 and len(got['max0'][0]) == 0
    assert [got[f'gap{g}_at4066'][6] for g in (10, 11)] == [1, 2]
    assert [got[n][6] for n in ('min11_odd15', 'min12_odd15', 'min11_odd14')] == [got['min11_odd15'][6]] + [got['min11_odd15'][6] - 1] * 2
    # more messages than every other edge: 4 rows of rise, fall, rise give 8 messages from 12 listed edges; 2 rows of one rise give 2 from 2
    assert (got['heads_span1'][6], got['heads_span1_open_only'][6], got['heads_span9'][6]) == (8, 2, 8)
    assert got['heads_span1'][2].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and flags['heads_span1'] == K.LONG
    assert [int(m) & 0x7FF for m in got['heads_span9'][5]] == [1, 0] * 4
    assert got['grid_cap'][3].tolist() == [1024 * K.TILE + 17] and got['rows4097'][2].max() == 4096
    for p in (0, 1):
        assert int(got[f'mc_odd_p{p}'][5][0] >> 11) & 0x7FF >= 1 and got[f'mc_long_p{p}'][1][0] > 60
    # the reach: a pulse whose last decisive-high sample lies exactly R back is still on, one sample later it has fallen
    for R in (64, 4096):
        T = K.TILE if R < K.TILE else 2 * K.TILE
        for a in (1000, T - R - 2, T - R - 1, T - R, T - 1, T):
            r = got[f'reach_R{R}_a{a}']
            # on again R + 1 behind a: one pulse; R + 2: a one-sample gap inside the message; R + 3: the first message falls at a + R + 1
            assert (r[6], int(r[5][0]) & 0x7FF) == [(1, 1), (1, 2), (2, 1)][a % 3], (R, a, r)
            assert a % 3 != 2 or int(r[3][0] + r[4][0]) == a + R + 1


@pytest.mark.parametrize("w", K.window_cases(), ids=lambda w: w[0])
def test_windows_with_exactly_their_reach(w):
    """The window given exactly pss_ook_halo's reach gives what the whole rows give between its ends, wherever the rows lie in a longer
    row; one sample less is refused."""
    name, buf, buf_index0, n_row, s_begin, s_end, spec, P, R, x, base = w
    got = E.h_ook_messages(buf, K.HI, K.LO, spec, P=P, R=R, buf_index0=buf_index0, n_row=n_row, s_begin=s_begin, s_end=s_end)
    want = K.messages(x, K.HI, K.LO, spec, P, R, s_begin - base, s_end - base)
    assert got[6] == len(want[0]) > 0 and same_bytes(got[3] - base, want[3])
    for i in (0, 1, 2, 4, 5):
        assert same_bytes(got[i], want[i]), WHAT[i]
    if name == "win_long_pulse":      # every row: its message, then the rise of a pulse whose fall is not listed (LONG, no pulse kept)
        assert got[2].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and [int(m) & 0x7FF for m in got[5]] == [2, 0] * 4
        assert [int(m) & K.LONG for m in got[5]] == [0, K.LONG] * 4
    before, after = E.ook_halo(P, R, spec['gap_limit'], spec['span'])
    assert buf_index0 == s_begin - before and buf_index0 + buf.shape[1] == min(n_row, s_end + after)
    with pytest.raises(ValueError, match="the buffer does not cover the window's reach"):
        E.h_ook_messages(buf[:, 1:], K.HI, K.LO, spec, P=P, R=R, buf_index0=buf_index0 + 1, n_row=n_row, s_begin=s_begin, s_end=s_end)

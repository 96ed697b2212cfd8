"""Squelch and the header's Peak / Avg meter against tests/golden/squelch.npz (CPU only): the host gate pss_h_squelch_gate against
the traces the reference's own loop condition and draw_header produced, the NumPy and oracle models of the meter against the values
draw_header left, the strength text, and the argument checks.  Every comparison is equality of bits or bytes."""
import numpy as np
import pytest

import squelch_cases as S
from pyspecsdr_amd import _lib as L
from pyspecsdr_amd import formats
from pyspecsdr_amd.engine import PssError, h_squelch_gate


@pytest.fixture(scope="module")
def gold():
    return S.golden()


def _traces(gold):
    peak = gold["peak"]
    n_hand = int(gold["n_hand"])
    for meta, opened, held in zip(gold["trace_meta"], gold["trace_open"], gold["trace_held"]):
        yield peak[:34], float(meta[0]), int(meta[1]), opened, held
    for meta, opened, held in zip(gold["hand_trace_meta"], gold["hand_trace_open"], gold["hand_trace_held"]):
        yield peak[35:35 + n_hand], float(meta[0]), int(meta[1]), opened, held


def test_fixture_has_what_the_issue_lists(gold):
    assert len(gold["peak"]) == 34 + 1 + int(gold["n_hand"]) == len(gold["avg"]) == len(gold["text"])
    assert {(float(s), int(e)) for s, e in gold["trace_meta"]} >= {(s, e) for s in (-60, 20, 35, 36, 37, 40, 50) for e in (1, 3, 7)}
    assert {int(e) for _, e in gold["trace_meta"]} >= {0} and {int(e) for _, e in gold["hand_trace_meta"]} >= {0, 1, 3}
    hand = gold["peak"][35:]
    assert np.isnan(hand).any() and np.isposinf(hand).any() and np.isneginf(hand).any()
    kinds = set()
    for _, s, e, opened, _ in _traces(gold):       # runs of both kinds in some trace; everything open at -60
        kinds |= set(opened.tolist())
        if s == -60 and e == 3 and len(opened) == 34:
            assert opened.all()
        if s > 0 and len(opened) == 34:
            assert not opened[:e if e else 34].any()       # PEAK_POWER starts at 0: closed up to and including the first metered frame
    assert kinds == {0, 1}


def test_host_gate_equals_every_golden_trace(gold):
    for peak, squelch, every, want_open, want_held in _traces(gold):
        opened, n_open, held_out = h_squelch_gate(peak, squelch, every, 0, 0.0)
        assert np.array_equal(opened, want_open), (squelch, every)
        assert n_open == int(want_open.sum())
        assert S.exact_bits(held_out, want_held[-1]), (squelch, every)
        m_open, m_held = S.gate_model(peak, squelch, every)                  # the test's own model reads the fixture the same way
        assert np.array_equal(m_open, want_open) and S.exact_bits(m_held, want_held)


def test_host_gate_cut_in_two_calls_with_the_carry(gold):
    for peak, squelch, every, want_open, want_held in _traces(gold):
        for cut in range(len(peak) + 1):
            o1, n1, h1 = h_squelch_gate(peak[:cut], squelch, every, 0, 0.0)
            phase = cut % every if every else 0
            o2, n2, h2 = h_squelch_gate(peak[cut:], squelch, every, phase, h1)
            assert np.array_equal(np.concatenate([o1, o2]), want_open), (squelch, every, cut)
            assert n1 + n2 == int(want_open.sum()) and S.exact_bits(h2, want_held[-1])
            if cut:
                assert S.exact_bits(h1, want_held[cut - 1])


def test_host_gate_no_frames_and_special_levels():
    opened, n_open, held = h_squelch_gate(np.empty(0), -60.0, 3, 2, 12.5)
    assert len(opened) == 0 and n_open == 0 and held == 12.5
    opened, n_open, held = h_squelch_gate(np.empty(0), -60.0, 0, 0, np.nan)
    assert n_open == 0 and np.isnan(held)
    peak = np.array([np.nan, 1.0, np.inf, -np.inf, 2.0])
    assert h_squelch_gate(peak, -60.0, 1)[0].tolist() == [1, 0, 1, 1, 0]      # held: 0, NaN (closed), 1, +inf (open), -inf (closed)
    assert h_squelch_gate(peak, -np.inf, 1)[0].tolist() == [1, 0, 1, 1, 1]    # -inf >= -inf; a NaN never opens
    assert h_squelch_gate(peak, -60.0, 0, 0, np.nan)[0].tolist() == [0] * 5   # never metered: the carried-in NaN stays
    assert h_squelch_gate(peak, 5.0, 0, 0, np.inf)[1] == 5                     # +inf carried in opens every frame


def test_host_gate_argument_errors():
    lib = L.load()
    peak = np.zeros(4)
    for every, phase in ((-1, 0), (3, 3), (3, -1), (0, 1), (1, 1)):
        with pytest.raises(PssError):
            h_squelch_gate(peak, 0.0, every, phase)
    import ctypes as C
    assert lib.pss_h_squelch_gate(None, 4, 0.0, 3, 0, 0.0, None, None, None) == L.PSS_E_ARG      # null peaks
    assert lib.pss_h_squelch_gate(None, -1, 0.0, 3, 0, 0.0, None, None, None) == L.PSS_E_ARG
    n = C.c_long(-1)
    assert lib.pss_h_squelch_gate(peak.ctypes.data, 4, 0.0, 3, 0, 0.0, None, C.byref(n), None) == 0 and n.value == 4   # outputs are optional
    assert {"pss_row_meter_f64", "pss_squelch_gate", "pss_h_squelch_gate", "pss_demod_gated", "pss_frame_pipeline_squelch"} <= set(L.exported_symbols())


def test_meter_models_equal_what_draw_header_left(gold):
    rows = S.golden_rows()
    peak, avg = S.meter_model(rows)
    assert S.same_bits(peak, gold["peak"])
    assert S.exact_bits(avg, gold["avg"])
    assert S.exact_bits(np.array([S.oracle_mean(r) for r in rows]), gold["avg"])      # the summation tree the device restates
    assert len(rows[34]) == 32764 and {len(r) for r in rows[35:]} >= {1, 4, 12, 124, 128, 132, 8193}


def test_header_strength_text(gold):
    for p, a, t in zip(gold["peak"], gold["avg"], gold["text"]):
        assert formats.header_strength_text(p, a) == str(t)
    assert str(gold["text"][0]).startswith("Peak: ") and " dB Avg: " in str(gold["text"][0])


def test_demodulate_recording_squelch_argument_checks():
    x = np.zeros(4096, np.complex64)
    with pytest.raises(ValueError):
        formats.demodulate_recording(x, 2.4e6, "NFM", frame_len=1000, squelch=-60)       # not a power of two: no cell-exact rows
    with pytest.raises(ValueError):
        formats.demodulate_recording(x, 2.4e6, "NFM", frame_len=8, squelch=-60)
    with pytest.raises(ValueError):
        formats.demodulate_recording(x, 2.4e6, "NFM", frame_len=1024, squelch=-60, meter_every=-1)
    with pytest.raises(ValueError):
        formats.demodulate_recording(x, 2.4e6, "NFM", frame_len=1024, squelch=-60, meter_every=2.5)
    with pytest.raises(ValueError):
        formats.demodulate_recording(x, 2.4e6, "FM", frame_len=1024, squelch=-60)
    with pytest.raises((ValueError, TypeError)):
        formats.demodulate_recording(x, 2.4e6, "NFM", frame_len=1024, squelch="open")

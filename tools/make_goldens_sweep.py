#!/usr/bin/env python3
"""Golden values for the scanner sweep report (tests/golden/sweep.npz) — made like tools/make_goldens.py: the build container imports the
reference's hot path (signal_processing.py) and, stubbed, its caller (pyspecsdr.py), runs them on the sweeps of tests/sweep_cases.py and
stores DATA only.  The slices themselves are not stored: sweep_cases regenerates them, and `crc_<case>` pins their bytes.

Driver cases run the reference's own scan_frequencies (pyspecsdr.py:1022-1093) on a fake sdr whose read_samples hands out the prepared
slices, with time.sleep a no-op and a fake screen; classify_signal has `welch` bound as make_goldens.py binds it.  The records before the
duplicate removal are the calls of classify_signal, in order.  The inline sweep's loop body sits inside main(): its per-slice numbers are the
five statements of :2542-2552, the gate as :2549 / :2555 write it, the label the reference's classify_signal.  Every list then goes through
the reference's display_scan_results (:1203-1262) on the screens of sweep_cases.SCREENS, page after page.

Per case <c>:   crc  freqs  peak (float32)  bw  count  hit  hit_idx  labels (of the hits)
                rec_freq rec_power rec_bw rec_type   the records as the sweep appended them
                keep (driver: indices into rec_* that survive the duplicate removal)  ded_freq ded_power ded_bw ded_type (the list returned)
                lines_<c>_<h>x<w>_p<page>_{y,x,text,pair,bold}   every addstr of one page (the driver's pages show the returned list)
lines_empty_*: display_scan_results on an empty list.  `margins`: the smallest distances the assertions below found.

    python tools/make_goldens_sweep.py
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import numpy as np
import scipy.signal as ss

import make_goldens as mg            # puts the reference tree on sys.path; caller_module(), stamp()
import make_goldens_adc as mga       # save_deterministic
import sweep_cases as S

sp = mg.sp
WELCH_BIN = S.FS / 1024


class Screen:
    """A fake curses screen: records addstr; getch returns -1 (no key); getstr plays a script of answers, then 'q'."""
    def __init__(s, h, w, answers=()): s.h, s.w, s.calls, s.pages, s.answers = h, w, [], [], list(answers)
    def getmaxyx(s): return s.h, s.w
    def addstr(s, *a): s.calls.append(a)
    def refresh(s): pass
    def nodelay(s, flag): pass
    def getch(s): return -1
    def clear(s):
        if s.calls:
            s.pages.append(s.calls)
        s.calls = []
    def getstr(s):
        return s.answers.pop(0) if s.answers else b"q"


class Sdr:
    def __init__(s, x): s.sample_rate, s.x, s.k, s.freqs, s.center_freq = S.FS, x, 0, [], None
    def read_samples(s, count):
        s.freqs.append(s.center_freq)
        s.k += 1
        return s.x[s.k - 1].copy()


def scan_numbers(x, kind, threshold):
    """The per-slice statements: pyspecsdr.py:2542-2552 (inline) / :1049-1057 (driver)."""
    spectrum = np.fft.fftshift(np.fft.fft(x))
    power_db = 10 * np.log10(np.abs(spectrum) ** 2 + 1e-10)
    peak_power = np.max(power_db)
    mask = power_db > (peak_power - 20) if kind == "inline" else power_db > threshold
    bandwidth = np.sum(mask) * (S.FS / len(power_db))
    assert power_db.dtype == np.float32 and type(peak_power) is np.float32 and type(bandwidth) is np.float64
    return peak_power, bandwidth, int(np.sum(mask))


def features(x):
    freqs, psd = sp.welch(x, fs=S.FS, nperseg=1024)
    power_db = 10 * np.log10(psd + 1e-10)                       # estimate_bandwidth's own mask, signal_processing.py:270-272
    cut_db = float(np.min(np.abs(power_db.astype(np.float64) - (float(np.max(power_db)) - 20.0))))
    return (float(sp.estimate_bandwidth(psd, freqs)), float(sp.estimate_modulation_index(x)),
            float(np.exp(np.mean(np.log(psd + 1e-10))) / np.mean(psd)), cut_db)


def draw(P, d, key, signals, hw, n_pages):
    import curses
    scr = Screen(hw[0], hw[1], [b"n"] * (n_pages - 1))
    P.display_scan_results(scr, signals, 0.0)
    scr.clear()
    assert len(scr.pages) == n_pages, (key, len(scr.pages))
    for page, calls in enumerate(scr.pages):
        k = f"{key}_p{page}"
        d[k + "_y"] = np.array([c[0] for c in calls], np.int32)
        d[k + "_x"] = np.array([c[1] for c in calls], np.int32)
        d[k + "_text"] = np.array([c[2] for c in calls])
        attrs = [c[3] if len(c) > 3 else 0 for c in calls]
        d[k + "_pair"] = np.array([(a & ~curses.A_BOLD) >> 8 for a in attrs], np.int32)
        d[k + "_bold"] = np.array([bool(a & curses.A_BOLD) for a in attrs])


def records(d, prefix, signals):
    assert all(type(s['frequency']) is float and type(s['power']) is np.float32 and type(s['bandwidth']) is np.float64 for s in signals)
    d[prefix + "_freq"] = np.array([s['frequency'] for s in signals], np.float64)
    d[prefix + "_power"] = np.array([s['power'] for s in signals], np.float32)
    d[prefix + "_bw"] = np.array([s['bandwidth'] for s in signals], np.float64)
    d[prefix + "_type"] = np.array([s['type'] for s in signals], dtype="U15")


def main():
    import curses
    import time
    P = mg.caller_module()
    sp.welch = ss.welch
    time.sleep = lambda s: None
    curses.echo = curses.noecho = lambda: None
    curses.curs_set = lambda v: None
    classified = []
    real_classify = sp.classify_signal

    def logging_classify(samples, fs, bandwidth):
        label = real_classify(samples, fs, bandwidth)
        classified.append(label)
        return label
    P.classify_signal = logging_classify
    assert P.MIN_SIGNAL_BANDWIDTH == S.MIN_BW

    d, margins = {}, {"peak_db": np.inf, "bw_bins": np.inf, "cls_bw_welch_bins": np.inf, "cls_bw_dc_span_welch_bins": np.inf,
                    "cls_mask_cut_db": np.inf, "mi_rel": np.inf, "flat": np.inf}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for c in S.CASES:
            x = S.slices(c)
            ns = len(x)
            d[f"crc_{c.name}"] = np.array(S.crc(x), np.uint32)
            nums = [scan_numbers(s, c.kind, c.threshold) for s in x]
            peak, bw = np.array([a[0] for a in nums], np.float32), np.array([a[1] for a in nums], np.float64)
            if c.kind == "driver":
                sdr, scr = Sdr(x), Screen(40, 120)
                del classified[:]
                unique = P.scan_frequencies(scr, sdr, c.start, S.sweep_end(c), c.threshold, c.step)
                assert sdr.k == ns and not any(str(a[2]).startswith("Error") for a in scr.calls if len(a) > 2), "the sweep raised"
                freqs = np.array(sdr.freqs, np.float64)
                found = [a[2] for a in scr.calls if len(a) > 2 and str(a[2]).startswith("Signal detected")]
                hit = np.zeros(ns, np.uint8)
                # the records as appended: one per classify_signal call; which slice it was follows from the status line's frequency
                shown = [f"Signal detected at {f / 1e6:.3f} MHz" for f in freqs]
                k = 0
                for i in range(ns):
                    if k < len(found) and found[k].startswith(shown[i]) and bool(peak[i] > c.threshold) and bool(bw[i] > S.MIN_BW):
                        hit[i] = 1
                        k += 1
                assert k == len(found) == len(classified)
                labels = list(classified)
                signals = [{'frequency': float(freqs[i]), 'power': peak[i], 'bandwidth': bw[i], 'type': labels[j]}
                           for j, i in enumerate(np.flatnonzero(hit))]
                # the returned list is those records, some dropped: find which (the reference's own dicts decide, not a restatement)
                keep, j = [], 0
                for u in unique:
                    while not (signals[j]['frequency'] == u['frequency'] and signals[j]['power'] == u['power'] and
                               signals[j]['bandwidth'] == u['bandwidth'] and signals[j]['type'] == u['type']):
                        j += 1
                    keep.append(j)
                    j += 1
                d[f"keep_{c.name}"] = np.array(keep, np.int32)
                records(d, f"ded_{c.name}", unique)
                shown_list = unique
            else:
                freqs, current_freq = [], c.start
                while current_freq <= S.sweep_end(c):
                    freqs.append(current_freq)
                    current_freq += c.step
                freqs = np.array(freqs, np.float64)
                assert len(freqs) == ns
                signals, hit = [], np.zeros(ns, np.uint8)
                for i in range(ns):
                    peak_power, bandwidth = nums[i][0], nums[i][1]
                    if peak_power > c.threshold:                       # :2549
                        if bandwidth > P.MIN_SIGNAL_BANDWIDTH:         # :2555
                            hit[i] = 1
                            signals.append({'frequency': float(freqs[i]), 'power': peak_power, 'bandwidth': bandwidth,
                                            'type': real_classify(x[i], S.FS, bandwidth)})
                labels = [s['type'] for s in signals]
                shown_list = signals
            d[f"freqs_{c.name}"], d[f"peak_{c.name}"], d[f"bw_{c.name}"] = freqs, peak, bw
            d[f"count_{c.name}"] = np.array([a[2] for a in nums], np.int32)
            d[f"hit_{c.name}"], d[f"hit_idx_{c.name}"] = hit, np.flatnonzero(hit).astype(np.int32)
            d[f"labels_{c.name}"] = np.array(labels, dtype="U15")
            records(d, f"rec_{c.name}", signals)
            for hw in S.SCREENS:
                per_page = hw[0] - 7
                draw(P, d, f"lines_{c.name}_{hw[0]}x{hw[1]}", shown_list, hw, (len(shown_list) + per_page - 1) // per_page)

            # ---- the conditions under which hit and label can be compared with == on a device whose PSD differs by float32 FFT noise
            below = [i for i in range(ns) if not peak[i] > c.threshold]
            narrow = [i for i in range(ns) if peak[i] > c.threshold and not bw[i] > S.MIN_BW]
            assert below and narrow and hit.any() and not hit.all(), (c.name, below, narrow, hit)
            margins["peak_db"] = min(margins["peak_db"], float(np.min(np.abs(peak.astype(np.float64) - c.threshold))))
            margins["bw_bins"] = min(margins["bw_bins"], float(np.min(np.abs(bw - S.MIN_BW)) / (S.FS / c.n)))
            for i in np.flatnonzero(hit):
                cbw, mi, flat, cut_db = features(x[i])
                edge = min(abs(cbw - e) for e in (2e3, 3e3, 8e3, 10e3, 16e3, 150e3)) / WELCH_BIN
                # A carrier that spans 0 Hz has its first masked bin at 0 Hz and its last at -fs/1024 (FFT order), so estimate_bandwidth returns
                # -fs/1024 for it whatever its width: 1.85 Welch bins below the 2 kHz edge, by arithmetic and not by the seed.  Those hits
                # are held by the direct condition instead — no PSD bin within 1e-3 dB of the mask's cut, so the mask cannot differ.
                if cbw == -WELCH_BIN:
                    margins["cls_bw_dc_span_welch_bins"] = min(margins["cls_bw_dc_span_welch_bins"], edge)
                else:
                    margins["cls_bw_welch_bins"] = min(margins["cls_bw_welch_bins"], edge)
                margins["cls_mask_cut_db"] = min(margins["cls_mask_cut_db"], cut_db)
                if cut_db < 1e-3:
                    print("   ", c.name, "slice", i, S.ORDER[i], f"a PSD bin lies {cut_db:.2g} dB from the mask's cut: pick another seed")
                margins["mi_rel"] = min(margins["mi_rel"], min(abs(mi - e) / e for e in (0.2, 0.3, 0.8)))
                margins["flat"] = min(margins["flat"], min(abs(flat - e) for e in (0.2, 0.3, 0.7)))
            print(c.name, "hits", np.flatnonzero(hit).tolist(), "below", below, "narrow", narrow, "labels", labels,
                  "" if c.kind == "inline" else f"keep {keep}")
        assert margins["peak_db"] >= 1e-3 and margins["bw_bins"] >= 2 and margins["cls_bw_welch_bins"] >= 2, margins
        assert margins["mi_rel"] >= 0.01 and margins["flat"] >= 1e-3 and margins["cls_mask_cut_db"] >= 1e-3, margins
        k = d["keep_driver_2048"]
        assert d["hit_driver_2048"][[0, 1, 3]].tolist() == [1, 1, 1] and 0 in k and 1 not in k, "88.00 / 88.05 MHz: the second is dropped"
        scr = Screen(40, 120)
        P.display_scan_results(scr, [], 0.0)
        scr.clear()
        calls = scr.pages[0]
        d["lines_empty_y"], d["lines_empty_x"] = np.array([a[0] for a in calls], np.int32), np.array([a[1] for a in calls], np.int32)
        d["lines_empty_text"], d["lines_empty_pair"] = np.array([a[2] for a in calls]), np.array([a[3] >> 8 for a in calls], np.int32)
    del sp.welch
    d["cases"] = np.array([c.name for c in S.CASES])
    d["margins"] = np.array(json.dumps(margins, sort_keys=True))
    d["stamp"] = np.array(mg.stamp())
    mga.save_deterministic("sweep", d)
    print("margins", margins)


if __name__ == "__main__":
    main()

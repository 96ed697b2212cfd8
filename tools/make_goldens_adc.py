#!/usr/bin/env python3
"""Golden values for ADC-quantised read buffers (tests/golden/adc.npz) — made like tools/make_goldens.py: the build container imports the
reference's hot path (signal_processing.py) and, stubbed, its caller (pyspecsdr.py), feeds them the fixture cases of tests/adc_cases.py
and stores DATA only.  The buffers themselves are not stored: adc_cases regenerates them, and `crc_<case>` pins their bytes.

Per case <c> (an item whose call raised is absent and `err_<item>_<c>` holds the exception's type name instead):
    db        compute_fft (signal_processing.py:243-264), float64        post      the caller's three statements on it (pyspecsdr.py:2278-2283)
    nfm wfm am usb   demodulate_signal's float64 audio (wfm: both channels; the others: channel 0, the channels asserted equal)
    <mode>_pcm       np.int16(audio * 32767) of the same call, both channels     (LSB is asserted equal to USB and not stored again)
    raw       demodulate_signal(..., 'RAW'), float32                     corr      iq_correction (:46-80), complex64
    power     measure_signal_power (:325-328), float32
    scan_db scan_peak scan_bw   the inline scanner's statements (pyspecsdr.py:2542-2552), float32 row, its maximum, the bandwidth
    cls_label cls_bw cls_mi cls_flat   classify_signal with `welch` bound as make_goldens.py binds it, and its three features
The one full read buffer (32 768 samples) stores db, corr, nfm, wfm, power and the classification only: a committed file stays under 1 MiB.
History (`hist_cases`: the 1024-sample cases in fixture order, all-zero buffer first; rows = their `post`): after each push,
    wf_glyph wf_colour   draw_waterfall's grid as caller.npz stores it; `wf_err[i]` = 1 where the reference raised (a flat history)
    ps_colour            draw_persistence's grid over the last 10 rows; `ps_err[i]` likewise

    python tools/make_goldens_adc.py
"""
import io
import os
import sys
import warnings
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import numpy as np
import scipy.signal as ss

import make_goldens as mg            # puts the reference tree on sys.path; stubs (caller_module, Scr), stamp()
import adc_cases as A

sp = mg.sp
FS = A.FS
BIG = 32768


def save_deterministic(name, arrs):
    """np.savez_compressed with fixed member timestamps and order: the same arrays give the same bytes on every run."""
    path = os.path.join(mg.OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def attempt(d, item, name, fn):
    try:
        out = fn()
    except Exception as e:  # noqa: BLE001 — the fact that the reference raised is the datum
        d[f"err_{item}_{name}"] = np.array(type(e).__name__)
        return None
    return out


def one_case(d, c):
    x, name, big = c.iq, c.name, c.n >= BIG
    d[f"crc_{name}"] = np.array(A.crc(x), np.uint32)
    db = attempt(d, "db", name, lambda: sp.compute_fft(x))
    if db is not None:
        d[f"db_{name}"] = db
        if not big:
            def post():
                # caller-side post-process, exactly the three statements at pyspecsdr.py:2278-2283
                fd = np.convolve(db, np.ones(5) / 5, mode="valid")
                thr = np.median(fd) - 10
                fd[fd < thr] = thr
                return fd
            p = attempt(d, "post", name, post)
            if p is not None:
                d[f"post_{name}"] = p
    for mode in ("NFM", "WFM") if big else ("NFM", "WFM", "AM", "USB"):
        a = attempt(d, mode.lower(), name, lambda: sp.demodulate_signal(x, FS, mode))
        if a is None:
            continue
        assert a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 2
        if mode == "WFM":
            d[f"wfm_{name}"] = a
        else:
            assert A.same_bits(a[:, 0].copy(), a[:, 1].copy())
            d[f"{mode.lower()}_{name}"] = a[:, 0].copy()
        d[f"{mode.lower()}_pcm_{name}"] = np.int16(a * 32767)
        if mode == "USB":
            assert A.same_bits(a, sp.demodulate_signal(x, FS, "LSB"))
    if not big:
        r = attempt(d, "raw", name, lambda: sp.demodulate_signal(x, FS, "RAW"))
        if r is not None:
            assert r.dtype == np.float32
            d[f"raw_{name}"] = r
    cc = attempt(d, "corr", name, lambda: sp.iq_correction(x))
    if cc is not None:
        assert cc.dtype == np.complex64
        d[f"corr_{name}"] = cc
    p = attempt(d, "power", name, lambda: sp.measure_signal_power(x))
    if p is not None:
        assert p.dtype == np.float32
        d[f"power_{name}"] = np.array(p)
    if not big:
        def scan():
            # the inline scanner's five statements, pyspecsdr.py:2542-2552
            spectrum = np.fft.fftshift(np.fft.fft(x))
            power_db = 10 * np.log10(np.abs(spectrum) ** 2 + 1e-10)
            peak = np.max(power_db)
            mask = power_db > (peak - 20)
            bw = np.sum(mask) * (FS / len(power_db))
            return power_db, peak, bw
        s = attempt(d, "scan", name, scan)
        if s is not None:
            assert s[0].dtype == np.float32
            d[f"scan_db_{name}"], d[f"scan_peak_{name}"], d[f"scan_bw_{name}"] = s[0], np.array(s[1]), np.array(s[2])

    def classify():
        freqs, psd = sp.welch(x, fs=FS, nperseg=1024)
        return (sp.classify_signal(x, FS, 0.0), float(sp.estimate_bandwidth(psd, freqs)), sp.estimate_modulation_index(x),
                np.exp(np.mean(np.log(psd + 1e-10))) / np.mean(psd))
    k = attempt(d, "cls", name, classify)
    if k is not None:
        assert k[2].dtype == np.float32 and k[3].dtype == np.float32
        d[f"cls_label_{name}"], d[f"cls_bw_{name}"], d[f"cls_mi_{name}"], d[f"cls_flat_{name}"] = (np.array(k[0]), np.array(k[1]),
                                                                                                   np.array(k[2]), np.array(k[3]))


def history(d, P, names):
    H, W = 40, 120
    rows = [d[f"post_{n}"] for n in names]
    d["hist_cases"], d["hist_hw"] = np.array(names), np.array([H, W])
    glyphs = {".": 0, "-": 1, "=": 2, "#": 3}
    P.WATERFALL_HISTORY.clear()
    gs, cs, errs = [], [], []
    for r in rows:
        scr = mg.Scr(H, W)
        g = -np.ones((H - 4, W - 8), np.int8); c = -np.ones((H - 4, W - 8), np.int8)
        try:
            P.draw_waterfall(scr, r, None, 100e6, 2.4e6, 0, 0, None)
            errs.append(0)
        except Exception:  # noqa: BLE001
            errs.append(1)
        else:
            for call in scr.calls:
                y, x, s, attr = call
                if s in glyphs and x >= 9 and y >= 3 and len(s) == 1 and (attr >> 8) >= 10:
                    g[y - 3, x - 9] = glyphs[s]; c[y - 3, x - 9] = (attr >> 8) - 10
        gs.append(g); cs.append(c)
    d["wf_glyph"], d["wf_colour"], d["wf_err"] = np.stack(gs), np.stack(cs), np.array(errs, np.uint8)
    P.WATERFALL_HISTORY.clear()
    P.PERSISTENCE_HISTORY.clear()
    ps, errs = [], []
    for r in rows:
        scr = mg.Scr(H, W)
        g = np.zeros((H - 4, W - 8), np.int8)
        try:
            P.draw_persistence(scr, r, None, 100e6, 2.4e6, 0, 0, None)
            errs.append(0)
        except Exception:  # noqa: BLE001
            errs.append(1)
        else:
            for call in scr.calls:
                y, x, s, attr = call
                if s == "*":
                    g[y - 2, x - 8] = attr >> 8
        ps.append(g)
    d["ps_colour"], d["ps_err"] = np.stack(ps), np.array(errs, np.uint8)
    P.PERSISTENCE_HISTORY.clear()


def main():
    sp.welch = ss.welch
    d = {}
    cases = A.golden_cases()
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for c in cases:
            one_case(d, c)
        names = [c.name for c in cases if c.n == 1024]
        names.sort(key=lambda n: n != "dead_zero_1024")          # the all-zero buffer first: the history starts flat
        history(d, mg.caller_module(), names)
    del sp.welch
    d["cases"] = np.array([c.name for c in cases])
    d["stamp"] = np.array(mg.stamp())
    save_deterministic("adc", d)
    print(len(cases), "cases;", sorted(k for k in d if k.startswith("err_")), "; wf_err", d["wf_err"], "ps_err", d["ps_err"])


if __name__ == "__main__":
    main()

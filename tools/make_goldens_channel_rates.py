#!/usr/bin/env python3
"""Golden vectors at the channel rates (tests/golden/channel_rates.npz) — made like tools/make_goldens_lengths.py: the build container
imports the reference's own module from /root/reference, feeds it the seeded read buffers of tests/length_cases.py and stores DATA only
(outputs, SciPy's filter tables, a digest of every input).

One frame, length_cases.fm_frames(1, n, seed=1), per length of channel_rate_cases.GOLDEN_LENGTHS:
    NFM_RATES    demodulate_signal(NFM) (one column: mono_to_stereo's columns are equal, asserted here) and SciPy's firwin / cheby1 /
                 sosfilt_zi tables as the reference designs them inside every call — cheby1(8, 0.05, 0.8) at 37 500 S/s, where q = 1
    WFM_RATES    demodulate_signal(WFM) (iq_correction first; both columns), the three butter(5) tables, alpha and the decimator's tables
    SSB_RATES    demodulate_signal(USB) (LSB runs the same statements, asserted here) and the firwin taps
The read buffers are not stored: crc_<n> pins the bytes that length_cases gives for them.  The refusals are recorded as well: the
rates of NFM_REFUSED / WFM_REFUSED must raise ValueError in the reference (asserted here; the suite holds the library to the same).

    python tools/make_goldens_channel_rates.py
"""
import hashlib
import os
import sys
import warnings

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import numpy as np
import scipy.signal as ss

import channel_rate_cases as CR
import length_cases as LC
import make_goldens as mg            # the generators' helpers (stamp, save); importing it writes nothing
import signal_processing as sp      # the reference hot path


def digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).digest(), np.uint8).copy()


def mono(aud):
    assert np.array_equal(aud[:, 0], aud[:, 1], equal_nan=True)      # mono_to_stereo: the columns are equal, one is stored
    return aud[:, 0].copy()


def raises_value_error(mode, fs):
    try:
        sp.demodulate_signal(LC.fm_frames(1, 256, seed=1)[0], fs, mode)
    except ValueError:
        return True
    return False


def main():
    nfm, wfm, ssb = ([fs for fs, _, _ in rows] for rows in (CR.NFM_RATES, CR.WFM_RATES, CR.SSB_RATES))
    d = {"lengths": np.array(CR.GOLDEN_LENGTHS), "nfm_rates": np.array(nfm), "wfm_rates": np.array(wfm), "ssb_rates": np.array(ssb),
         "nfm_refused": np.array(CR.NFM_REFUSED), "wfm_refused": np.array(CR.WFM_REFUSED)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n in CR.GOLDEN_LENGTHS:
            fm = LC.fm_frames(1, n, seed=1)[0]
            d[f"crc_{n}"] = digest(fm)
            for fs in nfm:
                out = mono(sp.demodulate_signal(fm, fs, "NFM"))
                assert len(out) == -(-(n - 1) // CR.factor(fs))
                d[f"nfm_{n}_{int(fs)}"] = out
            for fs in wfm:
                out = sp.demodulate_signal(fm, fs, "WFM")                       # (n_out, 2): iq_correction first
                assert out.shape == (-(-(n - 1) // CR.factor(fs)), 2)
                d[f"wfm_{n}_{int(fs)}"] = out
            for fs in ssb:
                usb, lsb = sp.demodulate_signal(fm, fs, "USB"), sp.demodulate_signal(fm, fs, "LSB")
                assert np.array_equal(usb, lsb, equal_nan=True)
                d[f"ssb_{n}_{int(fs)}"] = mono(usb)
        for fs in CR.NFM_REFUSED:
            assert raises_value_error("NFM", fs), fs
        for fs in CR.WFM_REFUSED:
            assert raises_value_error("WFM", fs), fs
    # SciPy's tables, as the reference designs them inside every call
    for fs in sorted(set(nfm + wfm)):
        k, q, nyq = f"{int(fs)}", CR.factor(fs), fs / 2
        d["taps_" + k] = ss.firwin(numtaps=65, cutoff=15000 / nyq)
        d["dec_sos_" + k] = ss.cheby1(8, 0.05, 0.8 / q, output="sos")
        d["dec_zi_" + k] = ss.sosfilt_zi(d["dec_sos_" + k])
    for fs in wfm:
        k, nyq = f"{int(fs)}", fs / 2
        d["lp_sos_" + k] = ss.butter(5, 15000 / nyq, btype="low", output="sos")
        d["pilot_sos_" + k] = ss.butter(5, [18800 / nyq, 19200 / nyq], btype="band", output="sos")
        d["lmr_sos_" + k] = ss.butter(5, [23000 / nyq, 53000 / nyq], btype="band", output="sos")
        d["alpha_" + k] = np.array(np.exp(-1 / (75e-6 * fs)))
    for fs in ssb:
        d[f"ssb_taps_{int(fs)}"] = ss.firwin(65, 3000 / fs, window="hamming")
    mg.save("channel_rates", **d)


if __name__ == "__main__":
    main()

"""Write tests/golden/welch.npz: the truth the capture survey's host twin and kernels are held to.  NumPy and SciPy only; DATA only.
Captures and windows are not stored: tests/welch_cases.py regenerates them from their seeds, `crc_<case>` and `wcrc_<case>` pin their bytes.

    python tools/make_goldens_welch.py

  mean_<case>   scipy.signal.welch(x.astype(complex128), fs, window=w, nperseg=N, noverlap=N - S, nfft=N, detrend='constant' | False,
                return_onesided=False, scaling=..., average='mean') for every row of the case, float64 [K][N], FFT order
  max_<case>    scipy.signal.spectrogram(... the same ..., mode='psd').max(-1)
  L_<case>      the number of segments SciPy formed
"""
import os
import sys

import numpy as np
import scipy
import scipy.signal as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import welch_cases as WC  # noqa: E402


def main():
    out = {"stamp": np.array(f"numpy {np.__version__} scipy {scipy.__version__} cases {WC.VERSION}")}
    for name, N, S, L, left, detrend, scaling, _, kinds, gap in WC.CASES:
        buf, n = WC.case_rows(name)
        w = WC.case_window(name)
        kw = dict(fs=WC.FS, window=w, nperseg=N, noverlap=N - S, nfft=N, detrend="constant" if detrend else False, return_onesided=False,
                  scaling=scaling)
        mean, mx = [], []
        for r in range(len(kinds)):
            x = buf[r, :n].astype(np.complex128)
            mean.append(ss.welch(x, average="mean", **kw)[1])
            sxx = ss.spectrogram(x, mode="psd", **kw)[2]
            assert sxx.shape == (N, L), (name, sxx.shape)
            assert np.array_equal(sxx.mean(-1), mean[-1]), name      # welch is the spectrogram's mean, exactly
            mx.append(sxx.max(-1))
        out["crc_" + name], out["wcrc_" + name] = np.uint32(WC.crc(buf)), np.uint32(WC.crc(w))
        out["mean_" + name], out["max_" + name], out["L_" + name] = np.array(mean), np.array(mx), np.int64(L)
        print(name, n, L, float(np.max(mean)))
    path = os.path.join(ROOT, "tests", "golden", "welch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()

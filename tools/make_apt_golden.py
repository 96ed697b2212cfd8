"""tests/golden/apt.npz: the APT fixture rows of tests/apt_cases.py.

    python tools/make_apt_golden.py

NumPy and SciPy only: it needs neither the built library nor a GPU.  Per case (three lines at 62 400 S/s, about 100 000 samples) a CRC-32
of the complex64 row (the rows are not stored: 800 KB each; tests regenerate them from the seeds, apt_cases.case_row, and hold them to the
CRC-32) and the records the NumPy statement of the rules reports at sync_errors = 2 (apt_cases.numpy_syncs) on the statement's own
envelope: the float64 discriminator np.angle(x[i] conj(x[i - 1])), apt_cases.numpy_front with scipy.signal.firwin(79, 1 / 15), rounded to
float32.  The library's float32 discriminator differs from that one in the last bit, so the tests hold the twin's positions and mismatches
to these records exactly and its scores to 1e-4.  Before anything is written the records are held to the condition: every sent line
within +-2 envelope samples of where it was put, no other record.
"""
import os
import sys

import numpy as np
from scipy.signal import firwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import apt_cases as A  # noqa: E402


def main():
    out = {"names": np.array(sorted(A.CASES))}
    taps = firwin(79, 1.0 / 15.0)
    for name in sorted(A.CASES):
        x = A.case_row(name)
        z = x.astype(np.complex128)
        d = np.concatenate([[0.0], np.angle(z[1:] * np.conj(z[:-1]))])
        env = A.numpy_front(d, taps).astype(np.float32)
        row, pos, meta, score, count = A.numpy_syncs(env, 2)
        want = A.case_starts(name)
        assert count == len(want) and np.all(np.abs(pos - want) <= 2), (name, pos, want)
        out[name + "/crc32"] = np.array([A.row_crc32(x)], np.int64)
        out[name + "/pos"], out[name + "/meta"], out[name + "/score"] = pos, meta, score
        print(f"{name}: {len(x)} samples, {count} lines at {pos.tolist()} (sent {np.round(want, 1).tolist()}), mismatches {meta.tolist()}")
    path = os.path.join(ROOT, "tests", "golden", "apt.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""tests/golden/adsb.npz: the ADS-B cases of tests/adsb_cases.py, made with NumPy alone — no library code.

    python tools/make_goldens_adsb.py

Per case: the synthesiser's parameters, the injected messages with their positions and phases, the address list, the records that the NumPy
statement of the rules (adsb_cases.numpy_frames) reports, and a CRC-32 of the capture.  The captures are not stored: tests regenerate them
from the seeds (adsb_cases.case_iq) and hold them to the CRC-32.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adsb_cases as A  # noqa: E402


def main():
    out = {"names": np.array(sorted(A.CASES)), "vectors": np.array(A.VECTORS + (A.DF19, A.DF24))}
    for name in sorted(A.CASES):
        spc, n, seed, amp, addresses, frames = A.CASES[name]
        iq = A.case_iq(name)
        msg, pos, meta, score, count = A.numpy_frames(iq, spc, 2.0, addresses)
        out[name + "/params"] = np.array([spc, n, seed, amp], np.float64)
        out[name + "/addresses"] = np.array(addresses, np.uint32)
        out[name + "/tx_msg"] = np.array([m for m, _, _ in frames])
        out[name + "/tx_pos"] = np.array([p for _, p, _ in frames], np.int64)
        out[name + "/tx_phase"] = np.array([ph for _, _, ph in frames], np.float64)
        out[name + "/msg"], out[name + "/pos"], out[name + "/meta"], out[name + "/score"] = msg, pos, meta, score
        out[name + "/crc32"] = np.array([A.capture_crc32(iq)], np.uint32)
        assert count == len(pos)
    path = os.path.join(ROOT, "tests", "golden", "adsb.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

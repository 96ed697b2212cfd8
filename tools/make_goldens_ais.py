"""tests/golden/ais.npz: the AIS fixture captures of tests/ais_cases.py.

    python tools/make_goldens_ais.py

Per case a CRC-32 of the capture (the captures are not stored: tests regenerate them from the seeds, ais_cases.case_iq, and hold them to
the CRC-32) and the records the host twins report (pss_h_ais_front with the default pulse, then pss_h_ais_frames), after they have been
held to the NumPy statement of the rules (ais_cases.numpy_frames) and to the injected frames.  Needs the built library, no GPU.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ais_cases as A  # noqa: E402
from pyspecsdr_amd.engine import Engine as E  # noqa: E402


def main():
    out = {"names": np.array(sorted(A.CASES))}
    for name in sorted(A.CASES):
        x = A.case_iq(name)
        y = E.h_ais_front(x)
        twin, ref = E.h_ais_frames(y), A.numpy_frames(y)
        for t, r in zip(twin[:5], ref[:5]):
            assert t.dtype == r.dtype and t.tobytes() == r.tobytes(), name
        sent = [A.with_crc(m) for m, _, _, _ in A.CASES[name][3]]
        assert [bytes(m[:n]) for m, n in zip(twin[0], twin[1])] == sent, name
        out[name + "/crc32"] = np.array([A.capture_crc32(x)], np.int64)
        for what, v in zip(("msg", "len", "row", "pos", "score"), twin[:5]):
            out[name + "/" + what] = v
        print(f"{name}: {twin[5]} frames at {twin[3].tolist()}")
    path = os.path.join(ROOT, "tests", "golden", "ais.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Write tests/golden/ook.npz: the records the NumPy statement of the OOK rules (tests/ook_cases.py) gives for the seeded fixtures, and the
CRC-32 of every generated row.  NumPy only: the reference holds no OOK code, and nothing from it is used.

    python tools/make_ook_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ook_cases as K  # noqa: E402

WHAT = ("bits", "n_bits", "row", "pos", "span", "meta")


def main():
    out = {"names": []}
    for kind, snr, seed in K.FIXTURES:
        name = f"{kind}{snr}"
        x, sent, spec = K.burst_fixture(kind, snr, seed)
        means = K.block_means(K.magnitude(x))
        hi, lo = K.levels(means)
        rec = K.messages(x, hi, lo, spec, **K.DETECT)
        out["names"].append(name)
        out[name + "_crc"] = np.uint32(K.crc(x))
        out[name + "_levels"] = np.array([hi, lo], np.float32)
        out[name + "_means_crc"] = np.uint32(K.crc(means))
        out[name + "_sent"] = np.array(sent, np.uint8)
        for w, a in zip(WHAT, rec):
            out[f"{name}_{w}"] = a
        print(name, hex(K.crc(x)), hi, lo, len(rec[0]))
    rows, hi, lo = K.small_rows()
    out["small_crc"] = np.uint32(K.crc(rows))
    for k, spec in enumerate(K.SMALL_SPECS):
        for w, a in zip(WHAT, K.messages(rows, hi, lo, spec, **K.DETECT)):
            out[f"small{k}_{w}"] = a
    out["cases_crc"] = np.array([K.crc(c['rows']) for c in K.shape_cases()], np.uint32)
    out["names"] = np.array(out["names"])
    path = os.path.join(ROOT, "tests", "golden", "ook.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

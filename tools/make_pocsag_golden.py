"""tests/golden/pocsag.npz: the POCSAG fixture rows of tests/pocsag_cases.py.

    python tools/make_pocsag_golden.py

NumPy only: it needs neither the built library nor a GPU.  Per case (one row each at 2400, 1200 and 512 bit/s: 16, 32 and 75 samples a bit,
15 dB in the 38.4 kHz row, 1.5 kHz off, the 2400 bit/s row inverted) a CRC-32 of the float32 discriminator row (the rows are not stored:
five to seven batches at 75 samples a bit alone are a megabyte; tests regenerate them from the seeds, pocsag_cases.case_row, and hold them
to the CRC-32) and the records the NumPy statement of the rules reports at the defaults (pocsag_cases.numpy_batches), after they have been
held to the condition: every injected batch reported with n_bad = 0, each within half a bit of where it was put, nothing else accepted.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pocsag_cases as P  # noqa: E402

WHAT = ("cw", "pos", "meta", "score")   # fix and row are all zeros here, which is asserted, not stored


def main():
    out = {"names": np.array(sorted(P.CASES))}
    for name in sorted(P.CASES):
        baud, _, inverted, messages = P.CASES[name]
        spb = P.SPB[baud]
        y = P.case_row(name)
        ref = P.numpy_batches(y, spb)
        n_batches, first = P.case_batches(name)
        assert ref[6] == n_batches, (name, ref[6], n_batches)
        for k, (pos, meta) in enumerate(zip(ref[3].tolist(), ref[4].tolist())):
            assert 2 * abs(pos - (first + 544 * spb * k)) <= spb and (meta >> 16) & 0xFF == 0 and bool((meta >> 8) & 1) == inverted, (name, k, pos, hex(meta))
        assert ref[0].reshape(-1).tolist() == [w for b in P.batches_of(messages) for w in b], name
        out[name + "/crc32"] = np.array([P.row_crc32(y)], np.int64)
        assert not ref[1].any() and not ref[2].any(), name
        for what, v in zip(WHAT, (ref[0], ref[3], ref[4], ref[5])):
            out[name + "/" + what] = v
        print(f"{name}: {len(y)} samples, {ref[6]} batches at {ref[3].tolist()}, fixed bits {[m >> 24 for m in ref[4].tolist()]}")
    path = os.path.join(ROOT, "tests", "golden", "pocsag.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

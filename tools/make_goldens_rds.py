"""tests/golden/rds.npz: the RDS cases of tests/rds_cases.py, made with NumPy alone — no library code.

    python tools/make_goldens_rds.py

Per case: the parameters and seeds of the synthesiser, the transmitted groups and the data bits of the row (filler bits included).  Once:
the matched filter sampled from the NUMERICAL inversion of the shaping spectrum (rds_cases.golden_pulse), the truth the library's
closed form is held to.  The IQ is not stored: tests regenerate it from the seeds (rds_cases.case_iq).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rds_cases as R  # noqa: E402


def main():
    out = {"names": np.array(sorted(R.CASES)), "pulse": R.golden_pulse(4), "pulse_span8": R.golden_pulse(8)}
    for name in sorted(R.CASES):
        fs, ppm, sub, tune, side, n_groups, seed = R.CASES[name]
        groups = R.case_groups(name)
        out[name + "/params"] = np.array([fs, ppm, sub, tune, side, n_groups, seed], np.float64)
        out[name + "/groups"] = groups
        out[name + "/bits"] = R.data_bits(groups, seed)
    path = os.path.join(ROOT, "tests", "golden", "rds.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

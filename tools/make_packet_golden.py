"""tests/golden/packet.npz: for every fixture row of tests/packet_cases.py its seed, SNR and clock factor, the CRC-32 of the regenerated row
(the rows themselves are not stored), the frames sent, and the records of the NumPy statement of the rules (packet_cases.numpy_front on the
discriminator row, then packet_cases.numpy_frames) — no GPU.

    python tools/make_packet_golden.py

The discriminator is pss_ais.h's (the project's model of NumPy's float32 arctan2, held to NumPy by the AIS and FM-mono suites); it is taken
from pss_h_ais_front with the one-tap pulse [1.0], which returns d itself.  Everything behind it is NumPy alone.  The script refuses to write
a fixture whose records are not exactly the frames it expects: change the fixture then, not the rule."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import packet_cases as P                                     # noqa: E402
from pyspecsdr_amd.engine import Engine as E                 # noqa: E402


def records(name):
    c = P.CASES[name]
    x = P.case_iq(name)
    d = E.h_ais_front(x, pulse=np.array([1.0]))
    z = P.numpy_front(x, space_gain=c["gain"], d=d)
    return x, P.numpy_frames(z)


def main():
    out = {"names": np.array(sorted(P.CASES))}
    for name in sorted(P.CASES):
        c = P.CASES[name]
        x, rec = records(name)
        got = [bytes(m[:n]) for m, n in zip(rec[0], rec[1])]
        if got != c["expect"]:
            raise SystemExit(f"{name}: the statement reads {len(got)} frames, {sum(g in c['expect'] for g in got)} of the {len(c['expect'])} expected")
        out[name + "/crc32"] = np.array([P.row_crc32(x)], np.uint32)
        out[name + "/seed"] = np.array([c["seed"]], np.int64)
        out[name + "/snr_clock_gain"] = np.array([np.nan if c["snr"] is None else c["snr"], c["clock"], c["gain"]], np.float64)
        sent = [f for fs, _, _ in c["bursts"] for f in fs]
        out[name + "/sent"] = np.frombuffer(b"".join(sent), np.uint8)
        out[name + "/sent_len"] = np.array([len(f) for f in sent], np.int32)
        for key, arr in zip(("msg", "len", "row", "pos", "score"), rec[:5]):
            out[name + "/" + key] = arr
        print(f"{name}: {len(x)} samples, {rec[5]} records at {rec[3].tolist()}")
    path = os.path.join(ROOT, "tests", "golden", "packet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

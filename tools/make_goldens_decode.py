#!/usr/bin/env python3
"""Golden values for the batched decoders (tests/golden/decode_batch.npz) — made like tools/make_goldens.py: the build container imports
the reference's decoders.py, runs it on the recordings of tests/decode_cases.py buffer by buffer and stores DATA only.  The recordings
themselves are not stored: decode_cases regenerates them, and `crc_<case>` pins their bytes.

Per Morse case <c>:  crc  text (one string per buffer)  timing (uint64 [n_frames][3]: the bits of float(dot), float(dash), float(gap))
                     rise / fall are not stored (the edge kernel is pinned by decoders.npz)
Per APRS case <c>:   crc  packets (JSON: one list per buffer, as decode_aprs returns it)  bits (uint8 [n_frames][n_bits]: decode_afsk of
                     the normalised real part, the stream decode_aprs hands to its framing code)

decode_morse draws kmeans' starting points from NumPy's global generator: every buffer is decoded under SEEDS and must give the same text
and the same timing bits under each — no buffer is excluded.  At least a third of every APRS case's buffers must carry a packet.  Both
conditions are asserted here and recorded in `conditions`.

    python tools/make_goldens_decode.py
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import numpy as np

import make_goldens as mg            # puts the reference tree on sys.path; stamp()
import make_goldens_adc as mga       # save_deterministic
import decode_cases as S

SEEDS = (1234, 1, 99, 20240229)


def main():
    import decoders
    d, cond = {}, {"seeds": list(SEEDS)}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for c in S.MORSE:
            x = S.frames(c)
            d[f"crc_{c.name}"] = np.array(S.crc(S.codes(c)), np.uint32)
            texts, timing = [], np.zeros((len(x), 3), np.float64)
            for f, buf in enumerate(x):
                got = []
                for seed in SEEDS:
                    np.random.seed(seed)
                    text, tm = decoders.decode_morse(buf.copy(), c.fs, S.THRESHOLD)
                    got.append((text, np.array([float(tm["dot"]), float(tm["dash"]), float(tm["gap"])]).tobytes()))
                assert all(g == got[0] for g in got), (c.name, f, "the reference's answer depends on its random draw")
                texts.append(got[0][0])
                timing[f] = np.frombuffer(got[0][1], np.float64)
            d[f"text_{c.name}"] = np.array(texts, dtype="U64")
            d[f"timing_{c.name}"] = timing.view(np.uint64)
            cond[c.name] = {"buffers": len(x), "empty": int(sum(t == "" for t in texts))}
            print(c.name, len(x), "buffers:", " | ".join(texts))
        for c in S.APRS:
            x = S.frames(c)
            d[f"crc_{c.name}"] = np.array(S.crc(S.codes(c)), np.uint32)
            packets, rows = [], []
            for buf in x:
                packets.append(decoders.decode_aprs(buf.copy(), c.fs))
                r = np.real(buf)
                rows.append(np.array(decoders.decode_afsk(r / np.max(np.abs(r)), c.fs), np.uint8))     # decoders.py:122-128
            n_pk = sum(1 for p in packets if p)
            assert 3 * n_pk >= len(x), (c.name, n_pk, "fewer than a third of the buffers carry a packet")
            d[f"packets_{c.name}"] = np.array(json.dumps(packets))        # JSON text: NumPy's str dtype drops trailing NULs
            d[f"bits_{c.name}"] = np.stack(rows)
            cond[c.name] = {"buffers": len(x), "with_packet": n_pk}
            print(c.name, len(x), "buffers,", n_pk, "with a packet")
    d["cases"] = np.array([c.name for c in S.CASES])
    d["conditions"] = np.array(json.dumps(cond, sort_keys=True))
    d["stamp"] = np.array(mg.stamp())
    mga.save_deterministic("decode_batch", d)


if __name__ == "__main__":
    main()

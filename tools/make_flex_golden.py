"""tests/golden/flex.npz: the FLEX fixture rows of tests/flex_cases.py.

    python tools/make_flex_golden.py

NumPy only: it needs neither the built library nor a GPU.  Per case (one frame of flex_cases.MESSAGES in each of the modes 0 .. 3 at 2 samples
a 3200-baud symbol on 5 % noise, mode 3 inverted at 1, and mode 1 as FSK at 12 samples a symbol, 25 dB in the 38.4 kHz row, 700 Hz off) the
seed's CRC-32 of the float32 discriminator row (the rows are not stored; tests regenerate them, flex_cases.case_row, and hold them to the
CRC-32) and the record the NumPy statement of the rules reports at the defaults (flex_cases.numpy_frames): pos, fiw, meta, score, and a
CRC-32 each of its 352 words and fix bytes, after it has been held to the condition: the one injected frame reported with n_bad = 0 within
one symbol of where it was put, its words those that were sent.
"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flex_cases as F  # noqa: E402


def main():
    names = sorted(F.CASES)
    crc, pos, fiw, meta, score = [], [], [], [], []
    for name in sorted(F.CASES):
        mode, h, seed, inverted, snr = F.CASES[name]
        y = F.case_row(name)
        ref = F.numpy_frames(y, h)
        assert ref[7] == 1 and abs(int(ref[4][0]) - F.LEAD) <= h, (name, ref[7], ref[4])
        m0, m1 = (int(v) for v in ref[5][0])
        assert m1 & 0xFFFF == 0 and bool((m0 >> 8) & 1) == inverted and (m0 >> 12) & 15 == mode, (name, hex(m0), hex(m1))
        sent = F.frame_words(mode, F.MESSAGES)
        assert all(ref[0][0, p].tolist() == sent[p] for p in F.active(mode)), name
        crc.append([F.row_crc32(y), zlib.crc32(ref[0].tobytes()), zlib.crc32(ref[1].tobytes())])
        pos.append(ref[4][0]), fiw.append(ref[2][0]), meta.append(ref[5][0]), score.append(ref[6][0])
        print(f"{name}: {len(y)} samples, frame at {ref[4].tolist()}, meta {[hex(v) for v in ref[5][0]]}, score {ref[6].tolist()}")
    path = os.path.join(ROOT, "tests", "golden", "flex.npz")
    # one array a field, a row a case in the order of `names`: crc32 = (the row, the 352 words, the 352 fix bytes)
    np.savez_compressed(path, names=np.array(names), crc32=np.array(crc, np.int64), pos=np.array(pos, np.int64), fiw=np.array(fiw, np.uint32),
                        meta=np.array(meta, np.uint32), score=np.array(score, np.float32))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

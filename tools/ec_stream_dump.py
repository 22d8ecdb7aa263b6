#!/usr/bin/env python3
"""Write the golden mixed token streams (tests/golden/ref_ec_mode.npz, every
tile of every case) for tools/ec_stream_check.cpp: tokens, the initial CDFs,
and what the plain-Python restatement (tests/ec_rate_ref.py's counter,
tests/ec_mode_ref.py's gather) gives for the rate, the final CDFs and the two
gathers of every partition CDF.  No device and no library call is involved.

  python tools/ec_stream_dump.py streams.bin
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from tests import ec_mode_ref as M  # noqa: E402
from tests import ec_rate_ref as RR  # noqa: E402

F = M.F


def streams(g):
    for row in g["cases"]:
        cid, j0, nj, o0, no = (int(v) for v in row[:5])
        jobs = g["jobs"][j0:j0 + nj]
        per_tile, t = {}, 0
        for o in g["ops"][o0:o0 + no].astype(np.int64):
            if o[0] >= 0:
                t = int(jobs[o[0], F["tile"]])
            per_tile.setdefault(t, []).append(o)
        for t in sorted(per_tile):
            tok, w, cdf = [], RR.Counter(), [int(v) for v in g["init_cdf"][cid]]
            before = w.tell_frac()
            for src, kind, a, ln, s, gather in per_tile[t]:
                if kind == 2:
                    tok.append(0x80000000 | int(a))
                    w.bit(int(a))
                    continue
                word = int(a) | int(ln) << 13 | int(s) << 18
                if kind == 1:
                    word |= int(gather) << 23 | (M.BSIZE_LG[int(jobs[src, F["bsize"]])] - 3) << 25
                    w.symbol(int(s), M.gather_cdf(cdf[a:a + ln], int(gather)))
                else:
                    sl = cdf[a:a + ln]
                    w.symbol_with_update(int(s), sl)
                    cdf[a:a + ln] = sl
                tok.append(word)
            yield (np.array(tok, np.uint32), g["init_cdf"][cid].astype(np.uint16),
                   w.tell_frac() - before, np.array(cdf, np.uint16))


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_ec_mode.npz"))
    out = list(streams(g))
    with open(sys.argv[1], "wb") as f:
        f.write(struct.pack("<I", len(out)))
        for tok, init, rate, fin in out:
            f.write(struct.pack("<II", len(tok), len(init)))
            f.write(tok.tobytes())
            f.write(init.tobytes())
            f.write(struct.pack("<q", rate))
            f.write(fin.tobytes())
            P = M.OFF["PARTITION"]
            for gather in (1, 2):
                f.write(np.array([M.gather_cdf(fin[P + 11 * i:P + 11 * i + 11], gather)[0]
                                  for i in range(20)], np.uint16).tobytes())
    print(f"{len(out)} streams, {sum(len(o[0]) for o in out)} tokens -> {sys.argv[1]}")


if __name__ == "__main__":
    main()

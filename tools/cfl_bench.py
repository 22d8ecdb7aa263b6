#!/usr/bin/env python3
"""Time rv_cfl_alpha_search_batch on one batch: every BLOCK_32X32 of a
3840 x 2160 4:2:0 8-bit frame (120 x 67 = 8040 jobs), HIP events around
back-to-back launches after a warm-up, enough repeats to fill half a second.

Prints one JSON line: microseconds per call, jobs per second, and the
achieved bytes per second over the algorithmic bytes of a job (the luma
block, the two source chroma blocks, the chroma neighbours and the answers).
The kernel is bound by integer VALU work, not by memory: per job and plane it
evaluates 33 predictions of 256 pixels (about 10 VALU operations per pixel
and alpha pair) against 1.6 KB of traffic, so the bytes-per-second figure
sits far below the HBM rate by construction.

  python tools/cfl_bench.py [--width 3840 --height 2160 --bsize 9 --bd 8]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rav1e_amd as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bsize", type=int, default=int(R.BlockSize.BLOCK_32X32))
    ap.add_argument("--bd", type=int, default=8)
    ap.add_argument("--xdec", type=int, default=1)
    ap.add_argument("--ydec", type=int, default=1)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    R.require_device(0)
    L = R.lib()
    rng = np.random.default_rng(7)
    dtype = np.uint16 if a.bd > 8 else np.uint8
    b = R.BlockSize(a.bsize)
    bw, bh = b.width(), b.height()
    w, h = R.subsampled_size(b, a.xdec, a.ydec)

    def planes():
        out = []
        for p in range(3):
            xd, yd = (a.xdec, a.ydec) if p else (0, 0)
            img = rng.integers(0, 1 << a.bd, (a.height >> yd, a.width >> xd)).astype(dtype)
            out.append(R.DevicePlane.from_array(img, xpad=16, ypad=16, xdec=xd, ydec=yd,
                                                bit_depth=a.bd))
        return out
    rec, src = planes(), planes()
    px, py = max(bw, 8), max(bh, 8)
    ox = 4 if a.xdec and bw == 4 else 0
    oy = 4 if a.ydec and bh == 4 else 0
    pos = [(x + ox, y + oy) for y in range(0, a.height - py + 1, py)
           for x in range(0, a.width - px + 1, px)]
    jobs = np.zeros(len(pos), R.CFL_JOB)
    for k, (x, y) in enumerate(pos):
        jobs[k] = (x, y, (1 if x >= px else 0) | (2 if y >= py else 0), 0)
    n = len(jobs)
    # the same call through the checked wrapper first: positions are in bounds
    first = R.cfl_alpha_search_batch(rec, src, jobs[:64], b, a.bd)
    rp = (R.RvPlane * 3)(*(p.desc for p in rec))
    sp = (R.RvPlane * 3)(*(p.desc for p in src))
    dj = R.DeviceBuffer.from_array(jobs)
    da, dc = R.DeviceBuffer(4 * n), R.DeviceBuffer(16 * n)

    def launch(reps):
        for _ in range(reps):
            rc = L.rv_cfl_alpha_search_batch(rp, sp, dj.ptr, n, a.bsize, a.bd, da.ptr, dc.ptr, None)
            if rc != R.RV_OK:
                raise R.Rav1eHipError(L.rv_last_error().decode())

    e0, e1 = L.rv_event_create(), L.rv_event_create()

    def timed(reps):
        L.rv_event_record(e0, None)
        launch(reps)
        L.rv_event_record(e1, None)
        L.rv_event_sync(e1)
        return L.rv_event_elapsed_ms(e0, e1) * 1e-3

    launch(20)  # warm-up
    L.rv_stream_sync(None)
    reps = 50
    t = timed(reps)
    while t < a.min_seconds:
        reps = int(reps * max(2.0, 1.2 * a.min_seconds / max(t, 1e-6)))
        t = timed(reps)
    alpha = da.download(np.int16, 2 * n).reshape(n, 2)
    assert (alpha[:64] == first).all()
    px_bytes = 2 if a.bd > 8 else 1
    job_bytes = ((w << a.xdec) * (h << a.ydec) + 2 * w * h + 2 * (w + h)) * px_bytes + 2 * (2 + 8)
    per_call = t / reps
    print(json.dumps({
        "kernel": "rv_cfl_alpha_search_batch", "bsize": b.name, "width": a.width,
        "height": a.height, "xdec": a.xdec, "ydec": a.ydec, "bit_depth": a.bd, "jobs": n,
        "repeats": reps, "seconds": round(t, 4), "us_per_call": round(per_call * 1e6, 2),
        "jobs_per_s": round(n / per_call), "bytes_per_job": job_bytes,
        "GB_per_s": round(n * job_bytes / per_call / 1e9, 1), "bound": "VALU (integer)",
        "alpha_histogram_u": np.bincount(alpha[:, 0] + 16, minlength=33).tolist()}))
    L.rv_event_destroy(e0)
    L.rv_event_destroy(e1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the fused intra-mode screening (rv_intra_screen.hip) against the same
result composed from separate operators, on one 1920 x 1080 luma frame as one
tile, every block of the size a job, at 8 and 10 bit:

  fused     one rv_intra_screen_batch launch (edges, 13 predictions, 13
            SATDs, the sorts and the mode list; modes and SATDs written)
  composed  rv_intra_edges_batch, then per mode of RAV1E_INTRA_MODES one
            rv_predict_intra_batch into a scratch plane and one rv_satd_batch
            of it against the source: 27 launches.  The selection then runs
            on the host (intra_screen_select); its time is stated apart, and
            the device time leaves out the copy of the SATDs to the host.

HIP events around back-to-back calls after a warm-up; five rounds of
>= --min-seconds each, the two variants alternating; median, minimum and
maximum of the rounds.  Both paths' results are compared before timing.  No
threshold: the numbers are stated as measured.

  python tools/intra_screen_bench.py [--out profiles/intra_screen_bench_1080p.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)
import rav1e_amd as R  # noqa: E402
from mvstack_bench import ROUNDS, timed_rounds, us  # noqa: E402

SIZES = ("BLOCK_8X8", "BLOCK_16X16", "BLOCK_32X32", "BLOCK_64X64")


def scene(width, height, bd, seed=23):
    rng = np.random.default_rng(seed + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    base = rng.integers(0, 1 << bd, (height + 8, width + 8))
    smooth = (np.cumsum(np.cumsum(base, 0), 1) // 53) % (1 << bd)
    src = smooth[4:4 + height, 4:4 + width].astype(dt)
    rec = np.clip(smooth[3:3 + height, 2:2 + width] + rng.integers(-4, 5, (height, width)), 0,
                  (1 << bd) - 1).astype(dt)
    return rec, src


def block_jobs(width, height, bsize, rng):
    b = R.BlockSize[bsize]
    w, h = b.width(), b.height()
    ys, xs = np.mgrid[0:height // h, 0:width // w]
    j = np.zeros(xs.size, R.INTRA_BLK_JOB)
    j["bo_x"], j["bo_y"] = xs.ravel() * (w // 4), ys.ravel() * (h // 4)
    j["po_x"], j["po_y"] = 4 * j["bo_x"], 4 * j["bo_y"]
    # key-frame rows by random neighbour modes
    j["cdf_off"] = [R.intra_mode_cdf_offset(R.FRAME_TYPE_KEY, b, int(a), int(l))
                    for a, l in rng.integers(0, 13, (len(j), 2))]
    return b, w, h, j


def run_size(L, a, bd, bsize, rec, src, scratch, dcdf, cdf):
    rng = np.random.default_rng(5)
    b, w, h, jobs = block_jobs(a.width, a.height, bsize, rng)
    n = len(jobs)
    tx = R._BSIZE_TX[int(b)]
    tiles = np.array([(0, 0, a.width, a.height)], R.INTRA_TILE)
    dt, dj = R.DeviceBuffer.from_array(tiles), R.DeviceBuffer.from_array(jobs)
    px = 2 if bd > 8 else 1
    dm, ds = R.DeviceBuffer(8 * n), R.DeviceBuffer(52 * n)
    de = R.DeviceBuffer(R.EDGE_PX * px * n)
    dsat = [R.DeviceBuffer(4 * n) for _ in range(13)]
    var = np.where((jobs["po_x"] == 0) & (jobs["po_y"] == 0), 0,
                   np.where(jobs["po_y"] == 0, 1, np.where(jobs["po_x"] == 0, 2, 3)))
    dij = []
    for m in R.RAV1E_INTRA_MODES:
        ij = np.zeros(n, R.INTRA_JOB)
        ij["x"], ij["y"], ij["mode"], ij["variant"] = jobs["po_x"], jobs["po_y"], m, var
        dij.append(R.DeviceBuffer.from_array(ij))
    dd = np.zeros(n, R.DIST_JOB)
    dd["org_x"] = dd["ref_x"] = jobs["po_x"]
    dd["org_y"] = dd["ref_y"] = jobs["po_y"]
    ddj = R.DeviceBuffer.from_array(dd)

    def checked(rc):
        if rc != R.RV_OK:
            raise R.Rav1eHipError(L.rv_last_error().decode())

    def fused():
        checked(L.rv_intra_screen_batch(C.byref(rec.desc), C.byref(src.desc), dt.ptr, 1, dj.ptr, n,
                                        int(b), bd, dcdf.ptr, len(cdf), 7, dm.ptr, ds.ptr, None,
                                        None))

    def composed():
        checked(L.rv_intra_edges_batch(C.byref(rec.desc), dt.ptr, 1, dj.ptr, n, int(b), int(tx), bd,
                                       -1, de.ptr, None))
        for k in range(13):
            checked(L.rv_predict_intra_batch(C.byref(scratch.desc), dij[k].ptr, de.ptr, n, int(tx),
                                             bd, None))
            checked(L.rv_satd_batch(C.byref(src.desc), C.byref(scratch.desc), ddj.ptr, n, w, h,
                                    dsat[k].ptr, None))

    fused()
    composed()
    L.rv_stream_sync(None)
    fs = ds.download(np.uint32, 13 * n).reshape(n, 13)
    cs = np.stack([d.download(np.uint32, n) for d in dsat], 1)
    fm = dm.download(np.uint8, 8 * n).reshape(n, 8)
    t0 = time.perf_counter()
    sel = [R.intra_screen_select(cs[k], cdf[jobs["cdf_off"][k]:jobs["cdf_off"][k] + 14], 7)
           for k in range(n)]
    host_sel = time.perf_counter() - t0
    same = bool((fs == cs).all()) and all(
        [int(v) for v in fm[k, 1:1 + fm[k, 0]]] == sel[k] for k in range(n))
    t, reps = timed_rounds(L, {"fused": fused, "composed": composed}, a.min_seconds)
    L.rv_stream_sync(None)
    mf, mc = float(np.median(t["fused"])), float(np.median(t["composed"]))
    return {"bsize": bsize, "bit_depth": bd, "jobs": n, "results_equal": same,
            "fused_us": us(t["fused"]), "composed_us": us(t["composed"]),
            "repeats": reps, "rounds": ROUNDS,
            "fused_jobs_per_second": round(n / mf), "composed_jobs_per_second": round(n / mc),
            "composed_over_fused": round(mc / mf, 2),
            "host_selection_us": round(host_sel * 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_screen_bench_1080p.json"))
    a = ap.parse_args()
    R.require_device(0)
    L = R.lib()
    cdf = R.ec_default_cdf_all(0)
    cdf = np.ascontiguousarray(cdf, np.uint16).reshape(-1)
    dcdf = R.DeviceBuffer.from_array(cdf)
    rows = []
    for bd in (8, 10):
        rec_a, src_a = scene(a.width, a.height, bd)
        rec = R.DevicePlane.from_array(rec_a, xpad=16, ypad=16, bit_depth=bd)
        src = R.DevicePlane.from_array(src_a, xpad=16, ypad=16, bit_depth=bd)
        scratch = R.DevicePlane(a.width, a.height, xpad=16, ypad=16, hbd=bd > 8, bit_depth=bd)
        for bsize in SIZES:
            rows.append(run_size(L, a, bd, bsize, rec, src, scratch, dcdf, cdf))
            print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/intra_screen_bench.py", "frame": [a.width, a.height],
           "num_modes_rdo": 7, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

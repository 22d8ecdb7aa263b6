#!/usr/bin/env python3
"""Time the fused motion compensation launch (rv_inter.hip) against the same
prediction composed from the separate operators, on one 1920 x 1080 4:2:0
frame as one tile, every block of the size a job, single and compound jobs
half and half, at 8 and 10 bit:

  fused     one rv_motion_compensate_batch launch: get_params and the clamp on
            the device, three planes, the prep tiles in LDS
  composed  per plane rv_put_8tap_batch over the single jobs, rv_prep_8tap_batch
            twice and rv_mc_avg_batch over the compound ones: 12 launches, the
            i16 tiles through HBM.  Its jobs (get_params, the clamp) are made on
            the host before the clock starts.

All jobs take reference set 0 (and 1 for the second reference): the composed
operators take one source plane a launch.  The fused launch is also timed at
every lanes-per-job packing the size allows (rv_motion_compensate_batch_lanes).
HIP events around back-to-back calls after a warm-up; five rounds of
>= --min-seconds each, the variants alternating; median, minimum and maximum
of the rounds.  Both paths' pixels are compared before timing.  No threshold:
the numbers are stated as measured.

  python tools/inter_front_bench.py [--out profiles/inter_front_bench_1080p.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)
import rav1e_amd as R  # noqa: E402
from mvstack_bench import ROUNDS, timed_rounds, us  # noqa: E402

SIZES = ("BLOCK_8X8", "BLOCK_16X16", "BLOCK_32X32", "BLOCK_64X64")
PAD = 88  # SB_SIZE + FRAME_MARGIN (src/frame/mod.rs:60)
LANES = (16, 32, 64, 128, 256)


def planes(width, height, bd, seed, fill=None):
    rng = np.random.default_rng(seed + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    out = []
    for p in range(3):
        w, h = (width, height) if p == 0 else (width // 2, height // 2)
        a = rng.integers(0, 1 << bd, (h, w)) if fill is None else np.full((h, w), fill)
        out.append(R.DevicePlane.from_array(a.astype(dt), xpad=PAD >> (1 if p else 0),
                                            ypad=PAD >> (1 if p else 0), xdec=1 if p else 0,
                                            ydec=1 if p else 0, bit_depth=bd))
    return out


def table(sets):
    arr = (R.RvPlane * (3 * len(sets)))()
    for s, ps in enumerate(sets):
        for p in range(3):
            arr[3 * s + p] = ps[p].desc
    return arr


def host_jobs(jobs, which, d, w, h, dec):
    """rv_mc_job records of reference `which` for one plane: get_params and
    PlaneSlice::clamp (src/predict.rs:267-284) on the host."""
    sh = 3 + dec
    mv = jobs["mv"][:, which].astype(np.int64)
    off = mv >> sh
    frac = (mv - (off << sh)) << (4 - sh)
    fx, fy = (4 * jobs["bo_x"]) >> dec, (4 * jobs["bo_y"]) >> dec
    out = np.zeros(len(jobs), R.MC_JOB)
    out["src_x"] = np.clip(fx + off[:, 1] - 3, -d.xorigin, d.width) + 3
    out["src_y"] = np.clip(fy + off[:, 0] - 3, -d.yorigin, d.height) + 3
    out["dst_x"], out["dst_y"] = fx, fy
    out["col_frac"], out["row_frac"] = frac[:, 1], frac[:, 0]
    return out


def run_case(L, a, bd, bsize, refs, dst_f, dst_c):
    b = R.BlockSize[bsize]
    w, h = b.width(), b.height()
    ys, xs = np.mgrid[0:a.height // h, 0:a.width // w]
    n = xs.size
    rng = np.random.default_rng(3 + int(b))
    jobs = np.zeros(n, R.INTER_MC_JOB)
    jobs["bo_x"], jobs["bo_y"] = xs.ravel() * (w // 4), ys.ravel() * (h // 4)
    jobs["mv"] = rng.integers(-64, 65, (n, 2, 2))
    comp = (np.arange(n) % 2) == 1
    jobs["ref_slot"][:, 1] = np.where(comp, 1, -1)
    tiles = np.array([(0, 0, a.width, a.height)], R.INTRA_TILE)
    dt, dj, dst = R.DeviceBuffer.from_array(tiles), R.DeviceBuffer.from_array(jobs), R.DeviceBuffer(4)
    prm = R.RvInterMcParams(int(b), 0, 0, bd)
    tr, tf = table(refs), table([dst_f])

    def checked(rc):
        if rc != R.RV_OK:
            raise R.Rav1eHipError(L.rv_last_error().decode())

    def fused(lanes=0):
        checked(L.rv_motion_compensate_batch_lanes(tr, len(refs), tf, 1, dt.ptr, 1, dj.ptr, n,
                                                   C.byref(prm), dst.ptr, lanes, None))

    per = []
    ns, nc = int((~comp).sum()), int(comp.sum())
    for p in range(3):
        dec = 1 if p else 0
        pw, ph = w >> dec, h >> dec
        d = refs[0][p].desc
        per.append(dict(w=pw, h=ph, n_s=ns, n_c=nc,
                        put=R.DeviceBuffer.from_array(host_jobs(jobs[~comp], 0, d, pw, ph, dec)),
                        p0=R.DeviceBuffer.from_array(host_jobs(jobs[comp], 0, d, pw, ph, dec)),
                        p1=R.DeviceBuffer.from_array(host_jobs(jobs[comp], 1, d, pw, ph, dec)),
                        t0=R.DeviceBuffer(2 * pw * ph * nc), t1=R.DeviceBuffer(2 * pw * ph * nc)))

    def composed():
        for p in range(3):
            c = per[p]
            dd, s0, s1 = C.byref(dst_c[p].desc), C.byref(refs[0][p].desc), C.byref(refs[1][p].desc)
            checked(L.rv_put_8tap_batch(dd, s0, c["put"].ptr, c["n_s"], c["w"], c["h"], 0, 0, bd, None))
            checked(L.rv_prep_8tap_batch(c["t0"].ptr, s0, c["p0"].ptr, c["n_c"], c["w"], c["h"], 0, 0,
                                         bd, None))
            checked(L.rv_prep_8tap_batch(c["t1"].ptr, s1, c["p1"].ptr, c["n_c"], c["w"], c["h"], 0, 0,
                                         bd, None))
            checked(L.rv_mc_avg_batch(dd, c["t0"].ptr, c["t1"].ptr, c["p0"].ptr, c["n_c"], c["w"],
                                      c["h"], bd, None))

    fused()
    composed()
    L.rv_stream_sync(None)
    same = int(dst.download(np.uint32)[0]) == 0
    for p in range(3):
        same &= bool((dst_f[p].download_visible() == dst_c[p].download_visible()).all())
    variants = {"fused": fused, "composed": composed}
    lds_ok = []
    for lanes in LANES:  # the packings a workgroup's LDS allows at this size
        per_job = (h + 7) * (w + 7) + (h + 7) * w + w * h
        if 2 * per_job * (256 // lanes) <= 64 * 1024:
            lds_ok.append(lanes)
            variants["lanes_%d" % lanes] = (lambda l=lanes: fused(l))
    t, reps = timed_rounds(L, variants, a.min_seconds)
    L.rv_stream_sync(None)
    mf, mc = float(np.median(t["fused"])), float(np.median(t["composed"]))
    spread = max(max(t["fused"]) - min(t["fused"]), max(t["composed"]) - min(t["composed"]))
    return {"bsize": bsize, "bit_depth": bd, "jobs": n, "compound_jobs": nc, "results_equal": same,
            "fused_us": us(t["fused"]), "composed_us": us(t["composed"]), "composed_launches": 12,
            "lanes_us": {str(l): us(t["lanes_%d" % l]) for l in lds_ok},
            "repeats": reps["fused"], "rounds": ROUNDS,
            "fused_jobs_per_second": round(n / mf), "composed_jobs_per_second": round(n / mc),
            "composed_over_fused": round(mc / mf, 2),
            "gain_exceeds_spread": bool(mc - mf > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inter_front_bench_1080p.json"))
    a = ap.parse_args()
    R.require_device(0)
    L = R.lib()
    rows = []
    for bd in (8, 10):
        refs = [planes(a.width, a.height, bd, 40 + s) for s in range(3)]
        fill = (1 << bd) - 3
        dst_f, dst_c = planes(a.width, a.height, bd, 0, fill), planes(a.width, a.height, bd, 0, fill)
        for bsize in SIZES:
            rows.append(run_case(L, a, bd, bsize, refs, dst_f, dst_c))
            print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/inter_front_bench.py", "frame": [a.width, a.height], "layout": "4:2:0",
           "filter_mode": "REGULAR", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

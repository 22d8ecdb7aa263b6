#!/usr/bin/env python3
"""Time the fused motion estimation launch (rv_motion_est.hip) against the
same searches composed from rv_diamond_search_batch, on the luma plane of one
1920 x 1080 4:2:0 8-bit frame as one tile, every whole block of the size an
item against 2 single reference sets, SATD sub-pel (use_satd_subpel):

  fused     one rv_motion_estimation_batch launch: pmv pair, MV range,
            get_subset_predictors, full-pel and sub-pel diamond on the device
  composed  per reference rv_diamond_search_batch full-pel, then sub-pel: 4
            launches on job records that are already in device memory.  The
            sub-pel records hold the full-pel winners of an earlier run (the
            parent has no device path from one search to the next).
  host      what the composition needs before its first launch, timed apart on
            one CPU thread and reported beside it: the copy of the stacks to
            the host and the building of the job records (get_mv_range, the pmv
            pair, get_subset_predictors); the copy of the full-pel winners and
            the re-upload between the two searches are not in it.

HIP events around back-to-back launches after a warm-up; --rounds (>= 20)
rounds, the two variants alternating inside every round; median, minimum and
maximum of the rounds.  The MVs and costs of both paths are compared before
timing.  No threshold: the numbers are stated as measured.

  python tools/motion_est_bench.py [--out profiles/motion_est_bench_1080p.json]
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
from tests import motion_est_ref as M  # noqa: E402

SIZES = ("BLOCK_8X8", "BLOCK_16X16", "BLOCK_32X32", "BLOCK_64X64")
PAD = 88  # SB_SIZE + FRAME_MARGIN (src/frame/mod.rs:60)
SETS = [(1, 0), (5, 1)]  # (RefType, DPB slot)
LAMBDA = 175


def scene(width, height, seed=5):
    """A smooth frame and two references: the frame moved by a few pixels, plus noise."""
    rng = np.random.default_rng(seed)
    a = rng.random((height + 64, width + 64))
    for ax in (0, 1):
        c = np.cumsum(a, axis=ax)
        a = np.take(c, np.arange(6, c.shape[ax]), axis=ax) - np.take(c, np.arange(0, c.shape[ax] - 6),
                                                                      axis=ax)
    a = (a - a.min()) / (a.max() - a.min()) * 255
    cut = lambda dy, dx: a[24 + dy:24 + dy + height, 24 + dx:24 + dx + width]  # noqa: E731
    org = np.rint(cut(0, 0)).astype(np.uint8)
    refs = [np.clip(np.rint(cut(dy, dx) + rng.integers(-2, 3, (height, width))), 0, 255).astype(np.uint8)
            for dy, dx in ((2, -3), (-1, 4))]
    return org, refs


def fields(rng, w_in_b, h_in_b):
    f = rng.integers(-48, 49, (7, h_in_b, w_in_b, 2)).astype(np.int16)
    f[rng.random((7, h_in_b, w_in_b)) < 0.5] = 0
    return f


def host_jobs(stacks, cmv, blocks, bsize, w_in_b, h_in_b, tile_mvs, prev_mvs, tile):
    """The composition's full-pel DS_JOB records, [reference][block]."""
    w, h = M.BLK_W[bsize], M.BLK_H[bsize]
    n = len(blocks)
    jobs = np.zeros((len(SETS), n), R.DS_JOB)
    for i, (ref, _) in enumerate(SETS):
        tf, pf = tile_mvs[ref - 1], prev_mvs[ref - 1]
        for b in range(n):
            bx, by = int(blocks[b]["bo_x"]), int(blocks[b]["bo_y"])
            j = jobs[i, b]
            j["po_x"], j["po_y"] = 4 * bx, 4 * by
            j["mvx_min"], j["mvx_max"], j["mvy_min"], j["mvy_max"] = M.mv_range(w_in_b, h_in_b, bx, by, w, h)
            st = stacks[b, i]
            p0, p1 = M.pmv_pair(int(st["n"]), st["stack"]["this_mv"])
            j["pmv0_row"], j["pmv0_col"], j["pmv1_row"], j["pmv1_col"] = p0[0], p0[1], p1[0], p1[1]
            j["lambda_"] = LAMBDA
            pr, _ = M.predictor_sources(tf, pf, tile, bx, by, tuple(int(v) for v in cmv[b, i]), w_in_b,
                                        h_in_b)
            j["n_pred"] = len(pr)
            j["pred"][:len(pr)] = [m for _, m in pr]
    return jobs


def run_case(L, a, name, org, refs, dorg, drefs):
    bsize = int(getattr(R.BlockSize, name))
    w, h = M.BLK_W[bsize], M.BLK_H[bsize]
    w_in_b, h_in_b = a.width // 4, a.height // 4
    rng = np.random.default_rng(bsize)
    tile = (0, 0, a.width, a.height)
    blocks = np.array([(0, x, y) for y in range(0, h_in_b - h // 4 + 1, h // 4)
                       for x in range(0, w_in_b - w // 4 + 1, w // 4)], R.INTER_BLK)
    n, ns = len(blocks), len(SETS)
    tile_mvs, prev_mvs = fields(rng, w_in_b, h_in_b), fields(rng, w_in_b, h_in_b)
    stacks = np.zeros((n, ns), R.MVREF_RESULT)
    stacks["n"] = rng.integers(0, 5, (n, ns))
    stacks["stack"]["this_mv"] = rng.integers(-40, 41, (n, ns, 9, 2))
    cmv = rng.integers(-40, 41, (n, ns, 2)).astype(np.int16)
    sets = R.RvInterRefSets()
    sets.n_single, sets.compound, sets.fwd, sets.bwd = ns, 0, 0, 1
    for i, (ref, slot) in enumerate(SETS):
        sets.ref[i], sets.slot[i] = ref, slot

    def checked(rc):
        if rc != R.RV_OK:
            raise R.Rav1eHipError(L.rv_last_error().decode())

    table = (R.RvPlane * 6)()
    table[0], table[3] = drefs[0].desc, drefs[1].desc
    tiles = np.array([tile], np.int32).view(R.INTRA_TILE).reshape(-1)
    dt, db, dstk, dcm = (R.DeviceBuffer.from_array(x) for x in (tiles, blocks, stacks, cmv))
    dtm, dpm = R.DeviceBuffer.from_array(tile_mvs), R.DeviceBuffer.from_array(prev_mvs)
    dme, dres, dst = R.DeviceBuffer(n * ns * 4), R.DeviceBuffer(n * ns * 16), R.DeviceBuffer(4)
    prm = R.RvMeParams(bsize, 8, 1, 0, w_in_b, h_in_b, LAMBDA, 0)

    def fused():
        checked(L.rv_motion_estimation_batch(C.byref(dorg.desc), table, 2, dt.ptr, 1, db.ptr, n, sets,
                                             dstk.ptr, dcm.ptr, dtm.ptr, dpm.ptr, C.byref(prm), dme.ptr,
                                             dres.ptr, dst.ptr, None))

    # the composition's host side, timed apart
    t0 = time.perf_counter()
    host_stacks = dstk.download(R.MVREF_RESULT, n * ns).reshape(n, ns)
    t1 = time.perf_counter()
    jobs = host_jobs(host_stacks, cmv, blocks, bsize, w_in_b, h_in_b, tile_mvs, prev_mvs, tile)
    t2 = time.perf_counter()
    dfull = [R.DeviceBuffer.from_array(jobs[i]) for i in range(ns)]
    ofull = [R.DeviceBuffer(16 * n) for _ in range(ns)]
    osub = [R.DeviceBuffer(16 * n) for _ in range(ns)]

    def full_pel():
        for i, (_, slot) in enumerate(SETS):
            checked(L.rv_diamond_search_batch(C.byref(dorg.desc), C.byref(drefs[slot].desc), dfull[i].ptr,
                                              n, w, h, 0, 0, 0, 8, ofull[i].ptr, None))

    full_pel()
    L.rv_stream_sync(None)
    dsub = []
    for i in range(ns):  # the sub-pel records: the full-pel winner as the only predictor
        win = ofull[i].download(R.FS_RESULT, n)
        sj = jobs[i].copy()
        sj["n_pred"] = 1
        sj["pred"][:, 0, 0], sj["pred"][:, 0, 1] = win["mv_row"], win["mv_col"]
        dsub.append(R.DeviceBuffer.from_array(sj))

    def composed():
        full_pel()
        for i, (_, slot) in enumerate(SETS):
            checked(L.rv_diamond_search_batch(C.byref(dorg.desc), C.byref(drefs[slot].desc), dsub[i].ptr,
                                              n, w, h, 1, 1, 0, 8, osub[i].ptr, None))

    fused()
    composed()
    L.rv_stream_sync(None)
    got = dres.download(R.FS_RESULT, n * ns).reshape(n, ns)
    same = int(dst.download(np.uint32)[0]) == 0
    for i in range(ns):
        want = osub[i].download(R.FS_RESULT, n)
        same &= bool((got[:, i]["mv_row"] == want["mv_row"]).all() and
                     (got[:, i]["mv_col"] == want["mv_col"]).all() and
                     (got[:, i]["cost"] == want["cost"]).all())
    e0, e1 = L.rv_event_create(), L.rv_event_create()

    def window(fn, reps):
        L.rv_event_record(e0, None)
        for _ in range(reps):
            fn()
        L.rv_event_record(e1, None)
        L.rv_event_sync(e1)
        return L.rv_event_elapsed_ms(e0, e1) * 1e-3 / reps

    variants = {"fused": fused, "composed": composed}
    reps = {}
    for k, fn in variants.items():  # warm-up, and windows of about --window-seconds
        window(fn, 3)
        reps[k] = max(1, int(a.window_seconds / max(window(fn, 3), 1e-6)))
    t = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            t[k].append(window(fn, reps[k]))
    L.rv_event_destroy(e0)
    L.rv_event_destroy(e1)
    us = lambda v: {"median": round(float(np.median(v)) * 1e6, 2), "min": round(min(v) * 1e6, 2),  # noqa: E731
                    "max": round(max(v) * 1e6, 2)}
    mf, mc = float(np.median(t["fused"])), float(np.median(t["composed"]))
    spread = max(max(t["fused"]) - min(t["fused"]), max(t["composed"]) - min(t["composed"]))
    return {"bsize": name, "blocks": n, "items": n * ns, "results_equal": same,
            "nonzero_mvs": int(((got["mv_row"] != 0) | (got["mv_col"] != 0)).sum()),
            "fused_us": us(t["fused"]), "composed_us": us(t["composed"]), "composed_launches": 2 * ns,
            "rounds": a.rounds, "repeats": reps,
            "host_stack_copy_ms": round((t1 - t0) * 1e3, 2), "host_job_build_ms": round((t2 - t1) * 1e3, 1),
            "composed_over_fused": round(mc / mf, 2), "difference_exceeds_spread": bool(abs(mc - mf) > spread),
            "lanes_per_item": "not measured (4 * min(chunks, 16), rv_motion_est.hip)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--window-seconds", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_est_bench_1080p.json"))
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds is at least 20")
    R.require_device(0)
    L = R.lib()
    org, refs = scene(a.width, a.height)
    dorg = R.DevicePlane.from_array(org, xpad=PAD, ypad=PAD, bit_depth=8)
    drefs = [R.DevicePlane.from_array(r, xpad=PAD, ypad=PAD, bit_depth=8) for r in refs]
    rows = []
    for name in SIZES:
        rows.append(run_case(L, a, name, org, refs, dorg, drefs))
        print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/motion_est_bench.py", "frame": [a.width, a.height], "layout": "4:2:0 (luma)",
           "bit_depth": 8, "reference_sets": 2, "use_satd": True, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

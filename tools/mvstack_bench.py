#!/usr/bin/env python3
"""Time the MV-stack operator (rv_mvstack.hip) on one 3840 x 2160 frame cut
into 8 tile columns, every 8x8 block an inter leaf: 129,600 blocks, three
reference pairs per block = 388,800 queries.

  paint    rv_mvref_grid_paint of the frame's blocks into the 8 tiles' grids
  batch    rv_find_mvrefs_batch of every block x ((1, 8), (2, 8), (1, 2))
  fill     rv_ec_mode_fill_stacks of the same blocks (one query per block,
           the block's own references), with and without the full stacks

HIP events around back-to-back calls after a warm-up; five rounds of
>= --min-seconds each; median, minimum and maximum of the rounds.  The timed
launches run in one child process under one `timeout`.  Beside them: the
oracle's find_mvrefs (oracle/orc_mvref.c) on one host thread over a sample of
the same queries, through ctypes -- the loop's time, and the time of the same
loop over calls that return at once (ref_frames[0] = INTRA_FRAME), so the
call's cost can be read off.  A sample of the device results is compared with
the oracle's.  No threshold: the numbers are stated as measured.

  python tools/mvstack_bench.py [--out profiles/mvstack_bench_2160p.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)
import rav1e_amd as R  # noqa: E402

ROUNDS = 5
PAIRS = ((1, 8), (2, 8), (1, 2))
SIGN_BIAS = 0b0000010


def frame_scene(width, height, tile_cols, seed=17):
    """(tiles, frame (cols, rows), jobs in coding order, queries)"""
    rng = np.random.default_rng(seed)
    fcols, frows = width // 4, height // 4
    sbw = (fcols + 15) // 16
    per = (sbw + tile_cols - 1) // tile_cols
    tiles = []
    for t in range(tile_cols):
        x0 = t * per * 16
        tiles.append((min(per * 16, fcols - x0), frows, x0, 0))
    jobs = []
    pool = rng.integers(-64, 65, (6, 2))
    for t, (cols, rows, _, _) in enumerate(tiles):
        # coding order: superblocks in raster order, 8x8 blocks in z-order inside
        ys, xs = np.mgrid[0:rows // 2, 0:cols // 2]
        sb = (ys // 8) * ((cols + 15) // 16) + xs // 8
        z = np.zeros_like(xs)
        for b in range(3):
            z |= ((xs >> b) & 1) << (2 * b) | ((ys >> b) & 1) << (2 * b + 1)
        order = np.lexsort((z.ravel(), sb.ravel()))
        n = len(order)
        j = np.zeros(n, R.EC_MODE_JOB)
        j["tile"], j["bx"], j["by"], j["bsize"] = t, 2 * xs.ravel()[order], 2 * ys.ravel()[order], 3
        comp = rng.random(n) < 0.3
        j["ref0"] = np.where(comp, 1, rng.integers(1, 3, n))
        j["ref1"] = np.where(comp, 2, 8)
        mode = np.where(comp, rng.integers(20, 28, n), rng.integers(14, 20, n))
        j["luma_mode"] = j["chroma_mode"] = mode
        mv = np.where((rng.random(n) < 0.7)[:, None], pool[rng.integers(0, 6, n)],
                      rng.integers(-300, 301, (n, 2)))
        mv1 = np.where((rng.random(n) < 0.7)[:, None], pool[rng.integers(0, 6, n)],
                       rng.integers(-300, 301, (n, 2))) * comp[:, None]
        j["mv0_row"], j["mv0_col"], j["mv1_row"], j["mv1_col"] = mv[:, 0], mv[:, 1], mv1[:, 0], mv1[:, 1]
        jobs.append(j)
    jobs = np.concatenate(jobs)
    q = np.zeros((len(jobs), 3), R.MVREF_QUERY)
    for f in ("tile", "bx", "by"):
        q[f] = jobs[f][:, None]
    q["bw4"] = q["bh4"] = 2
    q["ref"] = np.array(PAIRS, np.int32)[None]
    return np.array(tiles, np.int32), (fcols, frows), jobs, q.reshape(-1)


def timed_rounds(L, variants, min_seconds):
    """variants: name -> launch().  name -> [seconds per call] * ROUNDS, the
    variants alternating inside every round (tools/ec_cand_bench.py's scheme)."""
    e0, e1 = L.rv_event_create(), L.rv_event_create()

    def window(fn, reps):
        L.rv_event_record(e0, None)
        for _ in range(reps):
            fn()
        L.rv_event_record(e1, None)
        L.rv_event_sync(e1)
        return L.rv_event_elapsed_ms(e0, e1) * 1e-3

    reps = {}
    for name, fn in variants.items():
        window(fn, 5)
        r, t = 5, window(fn, 5)
        while t < min_seconds:
            r = int(r * max(2.0, 1.2 * min_seconds / max(t, 1e-6)))
            t = window(fn, r)
        reps[name] = r
    out = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            out[name].append(window(fn, reps[name]) / reps[name])
    L.rv_event_destroy(e0)
    L.rv_event_destroy(e1)
    return out, reps


def us(v):
    return {"median": round(float(np.median(v)) * 1e6, 2), "min": round(min(v) * 1e6, 2),
            "max": round(max(v) * 1e6, 2)}


def device_part(a):
    """The child process: the timed launches, a results sample for the parent"""
    R.require_device(0)
    L = R.lib()
    tiles, frame, jobs, q = frame_scene(a.width, a.height, a.tile_cols)
    grid = R.BlockGrid(tiles, frame[0], frame[1], SIGN_BIAS)
    geom = grid.geom()
    n, nq = len(jobs), len(q)
    dj, dq = R.DeviceBuffer.from_array(jobs), R.DeviceBuffer.from_array(q)
    dfill = R.DeviceBuffer.from_array(jobs)
    scr = R.DeviceBuffer(L.rv_mvref_paint_scratch_bytes(geom))
    dres = R.DeviceBuffer(nq * R.MVREF_RESULT.itemsize)
    dstk = R.DeviceBuffer(n * R.MVREF_RESULT.itemsize)
    dst = R.DeviceBuffer(4)

    def checked(rc):
        if rc != R.RV_OK:
            raise R.Rav1eHipError(L.rv_last_error().decode())
    v = {
        "paint": lambda: checked(L.rv_mvref_grid_paint(dj.ptr, n, geom, grid.dtiles.ptr, grid.buf.ptr,
                                                       scr.ptr, dst.ptr, None)),
        "batch": lambda: checked(L.rv_find_mvrefs_batch(dq.ptr, nq, geom, grid.dtiles.ptr,
                                                        grid.buf.ptr, dres.ptr, dst.ptr, None)),
        "fill": lambda: checked(L.rv_ec_mode_fill_stacks(dfill.ptr, n, geom, grid.dtiles.ptr,
                                                         grid.buf.ptr, None, dst.ptr, None)),
        "fill_with_stacks": lambda: checked(L.rv_ec_mode_fill_stacks(
            dfill.ptr, n, geom, grid.dtiles.ptr, grid.buf.ptr, dstk.ptr, dst.ptr, None)),
    }
    v["paint"]()  # the grid the queries read
    t, reps = timed_rounds(L, v, a.min_seconds)
    L.rv_stream_sync(None)
    assert int(dst.download(np.uint32)[0]) == 0
    res = dres.download(R.MVREF_RESULT, nq)
    sample = np.random.default_rng(3).choice(nq, a.check, replace=False)
    np.save(a.child + ".npy", res[sample])
    return {"blocks": n, "queries": nq, "tiles": len(tiles), "grid": [geom.grid_w, geom.grid_h],
            "launches": {k: {"us_per_call": us(t[k]), "repeats": reps[k], "rounds": ROUNDS} for k in v},
            "ns_per_query": {"batch": round(float(np.median(t["batch"])) * 1e9 / nq, 3),
                             "fill": round(float(np.median(t["fill"])) * 1e9 / n, 3)}}


def host_part(a, dev_sample):
    """The oracle on one thread over a sample of the queries"""
    from tests import oracle_lib as O
    tiles, frame, jobs, q = frame_scene(a.width, a.height, a.tile_cols)
    grids = R.default_block_grid(len(tiles), (frame[1] + 15) // 16 * 16,
                                 (int(tiles[:, 0].max()) + 15) // 16 * 16)
    for t in range(len(tiles)):
        jt = jobs[jobs["tile"] == t]
        g = grids[t]
        for dy in (0, 1):
            for dx in (0, 1):
                c = g[jt["by"] + dy, jt["bx"] + dx]
                c["ref"] = np.stack([jt["ref0"], jt["ref1"]], 1)
                c["n4_w"] = c["n4_h"] = 2
                c["newmv"] = np.isin(jt["luma_mode"], (19, 22, 23, 24, 25, 27))
                c["mv"] = np.stack([jt["mv0_row"], jt["mv0_col"], jt["mv1_row"],
                                    jt["mv1_col"]], 1).reshape(-1, 2, 2)
                g[jt["by"] + dy, jt["bx"] + dx] = c
    sample = np.random.default_rng(3).choice(len(q), a.check, replace=False)
    sb = [(SIGN_BIAS >> i) & 1 for i in range(7)]
    bad = 0
    for i, s in enumerate(sample):
        k = q[s]
        tl = tiles[k["tile"]]
        ctx, st = O.find_mvrefs(grids[k["tile"]], int(tl[0]), int(tl[1]), int(tl[2]), int(tl[3]),
                                frame[0], frame[1], int(k["bx"]), int(k["by"]), 2, 2,
                                tuple(int(v) for v in k["ref"]), sb)
        d = dev_sample[i]
        bad += not (int(d["mode_context"]) == ctx and int(d["n"]) == len(st) and
                    d["stack"][:len(st)].tobytes() == st.tobytes())
    # the timed loop: prebuilt arguments, the C function through ctypes
    L = O.lib()
    sel = np.random.default_rng(4).choice(len(q), a.host_queries, replace=False)
    sbv = np.array(sb, np.uint8)
    st = np.zeros(9, O.CAND)
    nout = C.c_int(0)
    gptr = [grids[t].ctypes.data for t in range(len(tiles))]
    pitch = grids.shape[2]

    def loop(first_ref):
        args = []
        for s in sel:
            k = q[s]
            tl = tiles[k["tile"]]
            rf = np.array([first_ref if first_ref is not None else k["ref"][0], k["ref"][1]], np.int32)
            args.append((gptr[k["tile"]], pitch, int(tl[0]), int(tl[1]), int(tl[2]), int(tl[3]),
                         frame[0], frame[1], int(k["bx"]), int(k["by"]), 2, 2, rf.ctypes.data, rf))
        f, sp, stp, npt = L.orc_find_mvrefs, sbv.ctypes.data, st.ctypes.data, C.addressof(nout)
        best = []
        for _ in range(3):
            t0 = time.perf_counter()
            for x in args:
                f(*x[:13], sp, stp, npt)
            best.append(time.perf_counter() - t0)
        return float(np.median(best))
    O.find_mvrefs(grids[0], 16, 16, 0, 0, 16, 16, 0, 0, 2, 2, (1, 8), sb)  # binds the argtypes
    full, empty = loop(None), loop(0)
    return {"checked_against_oracle": int(a.check), "mismatches": int(bad),
            "host_oracle": {"queries": int(a.host_queries),
                            "ns_per_query_loop": round(full * 1e9 / a.host_queries, 1),
                            "ns_per_query_call_only": round(empty * 1e9 / a.host_queries, 1),
                            "whole_frame_seconds_at_loop_rate":
                                round(full / a.host_queries * len(q), 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--tile-cols", type=int, default=8)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--check", type=int, default=2000)
    ap.add_argument("--host-queries", type=int, default=40000)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for the timed launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvstack_bench_2160p.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        json.dump(device_part(a), open(a.child, "w"))
        return
    tmp = a.out + ".device"
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__),
           "--child", tmp] + [x for k in ("width", "height", "tile_cols", "min_seconds", "check")
                              for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
    subprocess.check_call(cmd)  # the only process that opens the GPU
    dev = json.load(open(tmp))
    sample = np.load(tmp + ".npy")
    os.remove(tmp)
    os.remove(tmp + ".npy")
    host = host_part(a, sample)
    out = dict({"tool": "tools/mvstack_bench.py", "frame": [a.width, a.height],
                "tile_cols": a.tile_cols, "block": "8x8", "pairs": PAIRS}, **dev, **host)
    out["host_over_device_batch"] = round(
        host["host_oracle"]["ns_per_query_loop"] / max(dev["ns_per_query"]["batch"], 1e-9), 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

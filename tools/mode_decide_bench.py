#!/usr/bin/env python3
"""Time the fused mode decision launch (rv_mode_decide.hip) against the same
decision composed from the operators the library had before it, on one
1920 x 1080 4:2:0 frame as one tile, every block of the size, 8 candidates a
block in 4 plane sets, the pixel path under Tune::Psychovisual, at 8 and 10
bit:

  fused     one rv_mode_decide_batch launch: the biases, cdef_dist_wxh of luma
            and sse_wxh of U and V per candidate, the three scalings, the cost
            and the walk on the device
  composed  per plane set rv_cdef_moments_batch on luma and rv_sse_batch on U
            and V over the set's candidates (12 launches), then the f64 tail
            (cdef_dist_wxh_8x8's boost, bias and dist_scale with their
            truncations, compute_rd_cost) and the first-of-equals argmin as
            torch operations on the device.  Its jobs and the sub-blocks'
            biases are made on the host before the clock starts, and it has no
            early-outs to honour: every candidate is its own intra group.

All launches and the torch operations go to one stream.  The fused launch is
also timed at every lanes-per-block packing the size allows
(rv_mode_decide_batch_lanes).  HIP events around back-to-back calls after a
warm-up; five rounds of >= --min-seconds each, the variants alternating;
median, minimum and maximum of the rounds.  Both paths' distortions, costs and
winners are compared before timing.  No threshold: the numbers are stated as
measured.

  python tools/mode_decide_bench.py [--out profiles/mode_decide_bench_1080p.json]
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
from inter_front_bench import PAD, table  # noqa: E402
from mvstack_bench import ROUNDS, us  # noqa: E402

SIZES = ("BLOCK_8X8", "BLOCK_16X16", "BLOCK_32X32", "BLOCK_64X64")
LANES = (8, 16, 32, 64, 128, 256)
N_SETS, N_CANDS = 4, 8
SCALE = (0.9375, 1.28125, 1.6171875)
LAMBDA = 37.5


def planes(width, height, bd, seed, near=None):
    """Three 4:2:0 planes; with `near`, those pixels plus a small error."""
    rng = np.random.default_rng(seed + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    out, host = [], []
    for p in range(3):
        w, h = (width, height) if p == 0 else (width // 2, height // 2)
        if near is None:
            a = rng.integers(0, 1 << bd, (h, w))
        else:
            a = np.clip(near[p].astype(np.int64) + rng.integers(-9, 10, (h, w)) * (1 << (bd - 8)), 0,
                        (1 << bd) - 1)
        host.append(a.astype(dt))
        out.append(R.DevicePlane.from_array(host[-1], xpad=PAD >> (1 if p else 0),
                                            ypad=PAD >> (1 if p else 0), xdec=1 if p else 0,
                                            ydec=1 if p else 0, bit_depth=bd))
    return out, host


def timed_rounds(L, variants, min_seconds, stream):
    """tools/mvstack_bench.py's scheme on a given stream."""
    e0, e1 = L.rv_event_create(), L.rv_event_create()

    def window(fn, reps):
        L.rv_event_record(e0, stream)
        for _ in range(reps):
            fn()
        L.rv_event_record(e1, stream)
        L.rv_event_sync(e1)
        return L.rv_event_elapsed_ms(e0, e1) * 1e-3

    reps = {}
    for name, fn in variants.items():
        window(fn, 3)
        r, t = 3, window(fn, 3)
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


def composed_tail(torch, mom, sse_u, sse_v, bias_l, bias_c, rate, bd, scale, lam):
    """The decision from the raw partials.  mom: int64 (sets, 2, n, nsub, 5);
    sse_u / sse_v: int64 (sets, 2, n, nsub_c); bias_l (n, nsub), bias_c (n,
    nsub_c) f64; rate (n, 8) f64.  Returns (dist (n, 8) i64, cost (n, 8) f64,
    winner (n,) i64); candidate c = 4 * j + s is [s, j]."""
    cs = bd - 8
    ss, sd, s2, d2, sdp = mom.unbind(-1)
    svar = (s2 - ((ss * ss + 32) >> 6)).double()
    dvar = (d2 - ((sd * sd + 32) >> 6)).double()
    sse = (d2 + s2 - 2 * sdp).double()
    boost = (4033.0 / 16384.0) * (svar + dvar + float(16384 << (2 * cs))) / \
        torch.sqrt(float(16265089 << (4 * cs)) + svar * dvar)
    v = (sse * boost + 0.5).long()
    dl = ((v.double() * bias_l).long().sum(-1).double() * scale[0]).long()
    du = ((sse_u.double() * bias_c).long().sum(-1).double() * scale[1]).long()
    dv = ((sse_v.double() * bias_c).long().sum(-1).double() * scale[2]).long()
    n = mom.shape[2]
    dist = (dl + du + dv).permute(2, 1, 0).reshape(n, -1)
    cost = dist.double() + lam * (rate / 8.0)
    low = cost.min(1, keepdim=True).values
    idx = torch.arange(cost.shape[1], device=cost.device).expand_as(cost)
    winner = torch.where(cost == low, idx, cost.shape[1]).min(1).values
    return dist, cost, winner


def run_case(L, torch, a, bd, bsize, src, sets, imp, stream, sp):
    from tests import mode_decide_ref as M
    b = R.BlockSize[bsize]
    w, h = b.width(), b.height()
    ys, xs = np.mgrid[0:a.height // h, 0:a.width // w]
    n = xs.size
    rng = np.random.default_rng(3 + int(b))
    w_in_b, h_in_b = a.width // 4, a.height // 4
    blocks = np.zeros(n, R.MODE_BLOCK)
    blocks["bo_x"], blocks["bo_y"] = xs.ravel() * (w // 4), ys.ravel() * (h // 4)
    blocks["cand_first"], blocks["cand_count"] = np.arange(n) * N_CANDS, N_CANDS
    ts = [t for t in R.TxSize if (t.width(), t.height()) == (w, h)][0]
    cands = np.zeros((n, N_CANDS), R.MODE_CAND)
    cands["group"], cands["set"] = np.arange(N_CANDS), np.arange(N_CANDS) % N_SETS
    cands["flags"], cands["tx_size"] = R.MODE_CAND_INTRA, int(ts)
    cands["rate"] = rng.integers(0, 4000, (n, N_CANDS))
    tiles = np.array([(0, 0, a.width, a.height)], R.INTRA_TILE)
    lay = R.tx_blocks_layout(b, ts)
    eob = np.ones(lay.blocks_per_job, np.uint32)
    dt, db, dc = (R.DeviceBuffer.from_array(x) for x in (tiles, blocks, cands))
    dd, de = R.DeviceBuffer(8 * lay.blocks_per_job), R.DeviceBuffer.from_array(eob)
    di = R.DeviceBuffer.from_array(imp)
    do = R.DeviceBuffer(R.MODE_DECISION.itemsize * n)
    dcd, dcc, dcs = R.DeviceBuffer(8 * n * N_CANDS), R.DeviceBuffer(8 * n * N_CANDS), \
        R.DeviceBuffer(4 * n * N_CANDS)
    dst = R.DeviceBuffer(8)
    prm = R.RvModeDecideParams(int(b), bd, int(R.Tune.Psychovisual), 0, 1, w_in_b, h_in_b, imp.shape[1],
                               LAMBDA)
    for p in range(3):
        prm.dist_scale[p] = SCALE[p]
    tsrc, tset = table([src]), table(sets)

    def checked(rc):
        if rc != R.RV_OK:
            raise R.Rav1eHipError(L.rv_last_error().decode())

    def fused(lanes=0):
        checked(L.rv_mode_decide_batch_lanes(tsrc, tset, N_SETS, None, dt.ptr, 1, db.ptr, n, dc.ptr,
                                             n * N_CANDS, None, dd.ptr, de.ptr, lay.blocks_per_job, di.ptr,
                                             C.byref(prm), do.ptr, dcd.ptr, dcc.ptr, dcs.ptr, dst.ptr, lanes,
                                             sp))

    # ---- the composed path's inputs, made on the host
    per = N_CANDS // N_SETS  # candidates of a block on one set
    jl = np.zeros((per, n), R.DIST_JOB)
    jl["org_x"] = jl["ref_x"] = 4 * blocks["bo_x"]
    jl["org_y"] = jl["ref_y"] = 4 * blocks["bo_y"]
    jc = jl.copy()
    for f in ("org_x", "org_y", "ref_x", "ref_y"):
        jc[f] //= 2
    djl, djc = R.DeviceBuffer.from_array(jl), R.DeviceBuffer.from_array(jc)
    nsub = (w // 8) * (h // 8)
    cw, chh = w // 2, h // 2
    sbw = min(cw, 8) >> 1
    nsub_c = (cw // sbw) * (chh // sbw)
    dev = torch.device("cuda")
    mom = torch.empty((N_SETS, per, n, nsub, 5), dtype=torch.int64, device=dev)
    su = torch.empty((N_SETS, per, n, nsub_c), dtype=torch.int64, device=dev)
    sv = torch.empty((N_SETS, per, n, nsub_c), dtype=torch.int64, device=dev)
    fr = M.Frame(w_in_b, h_in_b, imp)
    bl, bc = np.zeros((n, nsub)), np.zeros((n, nsub_c))
    mwc = min(cw, 8) // 4
    for i in range(n):
        x0, y0 = int(blocks["bo_x"][i]), int(blocks["bo_y"][i])
        for k in range(nsub):
            bl[i, k] = M.distortion_bias(fr, x0 + 2 * (k % (w // 8)), y0 + 2 * (k // (w // 8)), 2, 2)
        for k in range(nsub_c):
            px, py = 2 * x0 + (k % (cw // sbw)) * sbw, 2 * y0 + (k // (cw // sbw)) * sbw
            bc[i, k] = M.distortion_bias(fr, px >> 1, py >> 1, mwc, mwc)
    tbl, tbc = torch.from_numpy(bl).to(dev), torch.from_numpy(bc).to(dev)
    trate = torch.from_numpy(cands["rate"].astype(np.float64)).to(dev)
    torch.cuda.synchronize()  # the uploads above went to torch's own stream
    keep = {}

    def composed():
        for s in range(N_SETS):
            checked(L.rv_cdef_moments_batch(C.byref(src[0].desc), C.byref(sets[s][0].desc), djl.ptr, per * n,
                                            w, h, mom[s].data_ptr(), sp))
            checked(L.rv_sse_batch(C.byref(src[1].desc), C.byref(sets[s][1].desc), djc.ptr, per * n, cw, chh,
                                   su[s].data_ptr(), sp))
            checked(L.rv_sse_batch(C.byref(src[2].desc), C.byref(sets[s][2].desc), djc.ptr, per * n, cw, chh,
                                   sv[s].data_ptr(), sp))
        with torch.cuda.stream(stream):
            keep["out"] = composed_tail(torch, mom, su, sv, tbl, tbc, trate, bd, SCALE, LAMBDA)

    fused()
    composed()
    L.rv_stream_sync(sp)
    dist, cost, win = (t.cpu().numpy() for t in keep["out"])
    got_d = dcd.download(np.uint64, n * N_CANDS).reshape(n, N_CANDS)
    got_c = dcc.download(np.float64, n * N_CANDS).reshape(n, N_CANDS)
    got_w = do.download(R.MODE_DECISION, n)["cand"] - blocks["cand_first"]
    same = bool((got_d == dist.astype(np.uint64)).all() and (got_c == cost).all() and (got_w == win).all())
    same &= not dst.download(np.uint32, 2).any()
    variants = {"fused": fused, "composed": composed}
    ok = []
    for lanes in LANES:
        if L.rv_mode_decide_check(tsrc, tset, N_SETS, None, C.byref(prm), 1, lanes) == R.RV_OK:
            ok.append(lanes)
            variants["lanes_%d" % lanes] = (lambda l=lanes: fused(l))
    t, reps = timed_rounds(L, variants, a.min_seconds, sp)
    L.rv_stream_sync(sp)
    mf, mc = float(np.median(t["fused"])), float(np.median(t["composed"]))
    spread = max(max(t["fused"]) - min(t["fused"]), max(t["composed"]) - min(t["composed"]))
    return {"bsize": bsize, "bit_depth": bd, "blocks": n, "candidates": n * N_CANDS, "results_equal": same,
            "fused_us": us(t["fused"]), "composed_us": us(t["composed"]), "composed_launches": 12,
            "lanes_us": {str(l): us(t["lanes_%d" % l]) for l in ok},
            "repeats": reps["fused"], "rounds": ROUNDS,
            "fused_candidates_per_second": round(n * N_CANDS / mf),
            "composed_candidates_per_second": round(n * N_CANDS / mc),
            "composed_over_fused": round(mc / mf, 2),
            "gain_exceeds_spread": bool(mc - mf > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mode_decide_bench_1080p.json"))
    a = ap.parse_args()
    import torch
    R.require_device(0)
    L = R.lib()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    rng = np.random.default_rng(1)
    imp = (rng.random(((a.height // 4 + 1) // 2, (a.width // 4 + 1) // 2)) * 6).astype(np.float32)
    rows = []
    for bd in (8, 10):
        src, host = planes(a.width, a.height, bd, 40)
        sets = [planes(a.width, a.height, bd, 50 + s, host)[0] for s in range(N_SETS)]
        for bsize in SIZES:
            rows.append(run_case(L, torch, a, bd, bsize, src, sets, imp, stream, sp))
            print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/mode_decide_bench.py", "frame": [a.width, a.height], "layout": "4:2:0",
           "tune": "Psychovisual", "candidates_per_block": N_CANDS, "plane_sets": N_SETS, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

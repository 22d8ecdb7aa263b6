#!/usr/bin/env python3
"""Time the fused transform-block launch (rv_tx_blocks.hip) against the same
result composed from the separate operators, on one 1920 x 1080 4:2:0 frame as
one tile, every block of the size a job, at 8 and 10 bit:

  fused     one rv_tx_blocks_batch launch (levels, eobs, distortions and the
            partition's pixels written)
  composed  per plane, one round per transform block: rv_intra_edges_batch ->
            rv_predict_intra_batch (intra only) -> rv_diff_fwd_txfm_batch ->
            rv_quantize_batch -> rv_inv_txfm_add_batch -> rv_tx_dist_batch.
            With luma tx_size = bsize.tx_size() that is one round a plane: 18
            launches intra, 12 inter.

Intra is DC_PRED / DC_PRED with need_recon_pixel, inter takes a prediction
plane set.  One qindex (the composed quantizer takes one a launch).  HIP
events around back-to-back calls after a warm-up; five rounds of
>= --min-seconds each, the two variants alternating; median, minimum and
maximum of the rounds.  Both paths' results are compared before timing.  No
threshold: the numbers are stated as measured.

  python tools/tx_blocks_bench.py [--out profiles/tx_blocks_bench_1080p.json]
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
QINDEX = 100


def scene(width, height, bd, seed=31):
    """rec, src, pred: three 4:2:0 planes each."""
    rng = np.random.default_rng(seed + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    out = []
    for k in range(3):
        planes = []
        for p in range(3):
            w, h = (width, height) if p == 0 else (width // 2, height // 2)
            base = rng.integers(0, 1 << bd, (h + 8, w + 8))
            smooth = (np.cumsum(np.cumsum(base, 0), 1) // 53) % (1 << bd)
            a = np.clip(smooth[4:4 + h, 4:4 + w] + rng.integers(-6, 7, (h, w)), 0, (1 << bd) - 1)
            planes.append(a.astype(dt))
        out.append(planes)
    return out


def device(planes, bd):
    return [R.DevicePlane.from_array(a, xpad=16, ypad=16, xdec=1 if p else 0, ydec=1 if p else 0,
                                     bit_depth=bd) for p, a in enumerate(planes)]


def plane_set(ps):
    return (R.RvPlane * 3)(*[p.desc for p in ps])


def run_case(L, a, bd, bsize, inter, dev):
    rec, src, pred, work, dst = dev
    b = R.BlockSize[bsize]
    w, h = b.width(), b.height()
    tx = R._BSIZE_TX[int(b)]
    lay = R.tx_blocks_layout(b, tx, 1, 1)
    ys, xs = np.mgrid[0:a.height // h, 0:a.width // w]
    n = xs.size
    jobs = np.zeros(n, R.TX_BLOCKS_JOB)
    jobs["bo_x"], jobs["bo_y"], jobs["qindex"] = xs.ravel() * (w // 4), ys.ravel() * (h // 4), QINDEX
    tiles = np.array([(0, 0, a.width, a.height)], R.INTRA_TILE)
    dt, dj = R.DeviceBuffer.from_array(tiles), R.DeviceBuffer.from_array(jobs)
    dl = R.DeviceBuffer(4 * lay.levels_per_job * n)
    de, dd = R.DeviceBuffer(4 * lay.blocks_per_job * n), R.DeviceBuffer(8 * lay.blocks_per_job * n)
    mode = int(R.PredictionMode.NEWMV if inter else R.PredictionMode.DC_PRED)
    prm = R.RvTxBlocksParams(int(b), int(tx), 0, mode, 0, 0, 0, 1, 1, bd)
    srec, ssrc, spred, sdst = plane_set(rec), plane_set(src), plane_set(pred), plane_set(dst)

    def checked(rc):
        if rc != R.RV_OK:
            raise R.Rav1eHipError(L.rv_last_error().decode())

    def fused():
        checked(L.rv_tx_blocks_batch(srec, ssrc, spred, sdst, dt.ptr, 1, dj.ptr, n, C.byref(prm),
                                     dl.ptr, de.ptr, dd.ptr, None))

    # the composed path's per-plane records and buffers
    px = 2 if bd > 8 else 1
    per = []
    for p in range(3):
        ts = lay.tx_size[p]
        tw, th = R.TxSize(ts).width(), R.TxSize(ts).height()
        xd = 1 if p else 0
        bj = np.zeros(n, R.INTRA_BLK_JOB)
        bj["bo_x"], bj["bo_y"] = jobs["bo_x"], jobs["bo_y"]
        bj["po_x"], bj["po_y"] = (jobs["bo_x"] >> xd) << 2, (jobs["bo_y"] >> xd) << 2
        ij = np.zeros(n, R.INTRA_JOB)
        ij["x"], ij["y"] = bj["po_x"], bj["po_y"]
        ij["variant"] = np.where((ij["x"] == 0) & (ij["y"] == 0), 0,
                                 np.where(ij["y"] == 0, 1, np.where(ij["x"] == 0, 2, 3)))
        tj = np.zeros(n, R.TX_JOB)
        tj["src_x"] = tj["pred_x"] = bj["po_x"]
        tj["src_y"] = tj["pred_y"] = bj["po_y"]
        ca = lay.coded_area[p]
        per.append(dict(ts=ts, area=tw * th, ca=ca, dbj=R.DeviceBuffer.from_array(bj),
                        dij=R.DeviceBuffer.from_array(ij), dtj=R.DeviceBuffer.from_array(tj),
                        edges=R.DeviceBuffer(R.EDGE_PX * px * n), co=R.DeviceBuffer(4 * tw * th * n),
                        q=R.DeviceBuffer(4 * ca * n), r=R.DeviceBuffer(4 * ca * n),
                        eob=R.DeviceBuffer(4 * n), dist=R.DeviceBuffer(8 * n)))

    def composed():
        for p in range(3):
            c = per[p]
            target = work[p]
            if not inter:
                checked(L.rv_intra_edges_batch(C.byref(rec[p].desc), dt.ptr, 1, c["dbj"].ptr, n,
                                               int(b), c["ts"], bd, 0, c["edges"].ptr, None))
                checked(L.rv_predict_intra_batch(C.byref(target.desc), c["dij"].ptr, c["edges"].ptr,
                                                 n, c["ts"], bd, None))
            checked(L.rv_diff_fwd_txfm_batch(C.byref(src[p].desc), C.byref(target.desc),
                                             c["dtj"].ptr, n, c["ts"], 0, bd, c["co"].ptr, None))
            checked(L.rv_quantize_batch(c["co"].ptr, c["area"], n, c["ts"], 0, QINDEX, bd,
                                        0 if inter else 1, 0, 0, c["q"].ptr, c["r"].ptr,
                                        c["eob"].ptr, None))
            checked(L.rv_inv_txfm_add_batch(c["r"].ptr, C.byref(target.desc), c["dtj"].ptr, n,
                                            c["ts"], 0, bd, None))
            checked(L.rv_tx_dist_batch(c["co"].ptr, c["area"], c["r"].ptr, n, c["ts"], c["dist"].ptr,
                                       None))

    def reset_work():  # the inter path adds the residual into a copy of the prediction
        for p in range(3):
            src_p = pred[p] if inter else rec[p]
            checked(L.rv_memcpy_d2d(work[p].buf.ptr, src_p.buf.ptr, src_p.buf.nbytes, None))

    reset_work()
    fused()
    composed()
    L.rv_stream_sync(None)
    lv = dl.download(np.int32, lay.levels_per_job * n).reshape(n, -1)
    di = dd.download(np.uint64, lay.blocks_per_job * n).reshape(n, -1)
    same = True
    for p in range(3):
        c = per[p]
        same &= bool((lv[:, lay.level_off[p]:lay.level_off[p] + c["ca"]] ==
                      c["q"].download(np.int32, c["ca"] * n).reshape(n, -1)).all())
        same &= bool((di[:, lay.first_block[p]] == c["dist"].download(np.uint64, n)).all())
        # the pixels: inside the jobs' area
        hh, ww = (a.height // h * h) >> (1 if p else 0), (a.width // w * w) >> (1 if p else 0)
        same &= bool((dst[p].download_visible()[:hh, :ww] == work[p].download_visible()[:hh, :ww]).all())
    t, reps = timed_rounds(L, {"fused": fused, "composed": composed}, a.min_seconds)
    L.rv_stream_sync(None)
    mf, mc = float(np.median(t["fused"])), float(np.median(t["composed"]))
    return {"bsize": bsize, "bit_depth": bd, "kind": "inter" if inter else "intra DC/DC", "jobs": n,
            "results_equal": same, "fused_us": us(t["fused"]), "composed_us": us(t["composed"]),
            "composed_launches": 12 if inter else 18, "repeats": reps, "rounds": ROUNDS,
            "fused_jobs_per_second": round(n / mf), "composed_jobs_per_second": round(n / mc),
            "composed_over_fused": round(mc / mf, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx_blocks_bench_1080p.json"))
    a = ap.parse_args()
    R.require_device(0)
    L = R.lib()
    rows = []
    for bd in (8, 10):
        rec_a, src_a, pred_a = scene(a.width, a.height, bd)
        dev = [device(x, bd) for x in (rec_a, src_a, pred_a, rec_a, rec_a)]
        for bsize in SIZES:
            for inter in (False, True):
                rows.append(run_case(L, a, bd, bsize, inter, dev))
                print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/tx_blocks_bench.py", "frame": [a.width, a.height], "layout": "4:2:0",
           "qindex": QINDEX, "need_recon_pixel": 1, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

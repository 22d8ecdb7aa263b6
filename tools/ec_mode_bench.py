#!/usr/bin/env python3
"""Time rv_ec_mode_tokenize on the mode-info jobs of one 3840 x 2160 frame at
the two extremes of the partition tree:

  leaves64  every superblock one 64x64 leaf (what speed 10 codes): 2040 blocks
            and their partition nodes (the tile is taken as 34 whole
            superblock rows so that the last row's leaves are legal);
  leaves8   every superblock split down to 8x8: 129,600 blocks and the
            partition nodes above them, the frame's bottom edge (540 rows of
            4x4) cutting the last superblock row.

Blocks are an INTER frame's with compound prediction allowed: a quarter intra
(CfL among the chroma modes), half single-reference, a quarter compound, MV
differences Laplacian with a few pixels' scale.  HIP events around
back-to-back calls after a warm-up, enough repeats to fill half a second.
Prints one JSON line per case: microseconds per call, tokens per second, and
beside it rv_ec_code_stream over the same tokens on one core (median of 5).

  python tools/ec_mode_bench.py [--width 3840 --height 2160]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rav1e_amd as R  # noqa: E402


def sb_template(min_lg):
    """(kind, dx, dy, lg, partition) of one superblock in coding order"""
    out = []

    def tree(x, y, lg):
        n4 = 1 << (lg - 2)
        split = lg > min_lg
        out.append((1, x, y, lg, 3 if split else 0))
        if split:
            for dy in (0, n4 // 2):
                for dx in (0, n4 // 2):
                    tree(x + dx, y + dy, lg - 1)
        else:
            out.append((0, x, y, lg, 0))
    tree(0, 0, 6)
    return np.array(out, np.int64)


def frame_jobs(rng, cols, rows, min_lg):
    t = sb_template(min_lg)
    sbw, sbh = (cols + 15) // 16, (rows + 15) // 16
    sy, sx = np.divmod(np.arange(sbw * sbh), sbw)
    kind = np.tile(t[:, 0], sbw * sbh)
    bx = (sx[:, None] * 16 + t[None, :, 1]).reshape(-1)
    by = (sy[:, None] * 16 + t[None, :, 2]).reshape(-1)
    lg = np.tile(t[:, 3], sbw * sbh)
    part = np.tile(t[:, 4], sbw * sbh)
    keep = (bx < cols) & (by < rows)
    kind, bx, by, lg, part = kind[keep], bx[keep], by[keep], lg[keep], part[keep]
    n = len(kind)
    j = np.zeros(n, R.EC_MODE_JOB)
    j["kind"], j["bx"], j["by"], j["bsize"], j["partition"] = kind, bx, by, 3 * (lg - 2), part
    blk = kind == 0
    cls = rng.random(n)
    intra, comp = blk & (cls < 0.25), blk & (cls >= 0.75)
    single = blk & ~intra & ~comp
    P = R.PredictionMode
    luma = np.where(intra, rng.integers(0, 13, n),
                    np.where(comp, rng.integers(P.NEAREST_NEARESTMV, P.NEW_NEWMV + 1, n),
                             rng.integers(P.NEARESTMV, P.NEWMV + 1, n)))
    chroma = np.where(intra, np.where(lg < 6, rng.integers(0, 14, n), rng.integers(0, 13, n)), luma)
    j["luma_mode"], j["chroma_mode"] = np.where(blk, luma, 0), np.where(blk, chroma, 0)
    j["skip"] = blk & (rng.random(n) < 0.3)
    j["ref0"] = np.where(comp, rng.integers(1, 5, n), np.where(single, rng.integers(1, 8, n), 0))
    j["ref1"] = np.where(comp, rng.integers(5, 8, n), np.where(blk, 8, 0))
    inter = single | comp
    j["num_mv_found"] = np.where(inter, 4, 0)
    j["mode_context"] = np.where(inter, rng.integers(0, 6, n) | rng.integers(0, 2, n) << 3 |
                                 rng.integers(0, 6, n) << 4, 0)
    for k in range(4):
        j["weight%d" % k] = np.where(inter, rng.integers(0, 1280, n), 0)
    for f in ("mv0_row", "mv0_col", "mv1_row", "mv1_col"):
        rm = np.where(inter, rng.integers(-256, 256, n) * 2, 0)
        j["ref_" + f] = rm
        j[f] = rm + np.where(inter, np.round(rng.laplace(0, 24, n)).astype(np.int64) * 2, 0)
    j["cfl_joint_sign"] = np.where(chroma == 13, rng.integers(0, 8, n), 0)
    j["cfl_scale_u"] = j["cfl_scale_v"] = np.where(chroma == 13, rng.integers(1, 17, n), 0)
    return j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--qctx", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    R.require_device(0)
    L = R.lib()
    cols, rows = (a.width + 7) // 8 * 2, (a.height + 7) // 8 * 2
    cdf0 = R.ec_default_cdf_all(a.qctx)
    for name, min_lg, trows in (("leaves64", 6, (rows + 15) // 16 * 16), ("leaves8", 3, rows)):
        rng = np.random.default_rng(11)
        jobs = frame_jobs(rng, cols, trows, min_lg)
        prm = R.EcModeParams(R.FRAME_INTER, 1, 0, 0, 0, 0, ((cols, trows),))
        tok, off, bad = R.ec_tokenize_modes(jobs, prm, check=False)  # the checked wrapper first
        assert bad == 0, bad
        n = len(jobs)
        mw, mh = cols // 2, (trows + 1) // 2
        dj, ddim = R.DeviceBuffer.from_array(jobs), R.DeviceBuffer.from_array(prm.tile_dims)
        dmap, scr = R.DeviceBuffer(4 * mw * mh), R.DeviceBuffer(L.rv_ec_mode_scratch_bytes(n))
        doff, dtok, dst = R.DeviceBuffer(4 * (n + 1)), R.DeviceBuffer(4 * (len(tok) + 16)), \
            R.DeviceBuffer(12)

        def launch(reps):
            for _ in range(reps):
                rc = L.rv_ec_mode_tokenize(dj.ptr, n, prm.c_struct(), 1, ddim.ptr, mw, mh, dmap.ptr,
                                           scr.ptr, doff.ptr, dtok.ptr, len(tok) + 16, dst.ptr, None)
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
        reps = 20
        t = timed(reps)
        while t < a.min_seconds:
            reps = int(reps * max(2.0, 1.2 * a.min_seconds / max(t, 1e-6)))
            t = timed(reps)
        assert (dtok.download(np.uint32)[:len(tok)] == tok).all()
        per_call = t / reps
        out = np.zeros(tok.size // 2 + 4096, np.uint8)
        host = []
        for _ in range(5):
            c2 = cdf0.copy()
            t0 = time.perf_counter()
            nb = L.rv_ec_code_stream(tok.ctypes.data, tok.size, c2.ctypes.data, out.ctypes.data,
                                     out.size)
            host.append(time.perf_counter() - t0)
            assert nb > 0
        host_s = float(np.median(host))
        per_job = np.diff(off.astype(np.int64))[jobs["kind"] == 0]
        print(json.dumps({
            "kernel": "rv_ec_mode_tokenize", "case": name, "width": a.width, "height": a.height,
            "jobs": n, "blocks": int((jobs["kind"] == 0).sum()), "tokens": int(tok.size),
            "repeats": reps, "seconds": round(t, 4), "us_per_call": round(per_call * 1e6, 2),
            "tokens_per_s": round(tok.size / per_call),
            "tokens_per_block": {"median": int(np.median(per_job)), "max": int(per_job.max())},
            "host_coder_us": round(host_s * 1e6, 1),
            "host_coder_tokens_per_s": round(tok.size / host_s),
            "device_over_host": round(host_s / per_call, 2), "bytes": int(nb)}), flush=True)
        L.rv_event_destroy(e0)
        L.rv_event_destroy(e1)


if __name__ == "__main__":
    main()

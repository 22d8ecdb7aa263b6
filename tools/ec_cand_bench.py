#!/usr/bin/env python3
"""Time the pricing of whole RDO candidates on the candidates of one round of
a 3840 x 2160 4:2:0 frame: 60 x 34 = 2040 groups, one per superblock.

  stream   rv_ec_rate_stream_batch (combined table, 5954 u16 per LDS slice)
           on coefficient-only streams against rv_ec_rate_batch (4317 u16) on
           the same tokens, tools/ec_rate_bench.py's three scales, with 1, 2
           and 4 groups per workgroup: the cost of the larger slice alone.
  copy     the same kernels on groups of one token: what the snapshot copy and
           the launch cost, with no token walk behind them.
  cand     rv_ec_cand_rates end to end (candidate tokenizer + counter, one
           stream, no host synchronisation) on mixed candidates -- a 64x64
           block's partition node, mode info and three transform blocks per
           superblock, a third of them skip -- beside rv_ec_count_stream on
           one host core over the same streams, each from a fresh copy of the
           snapshot (median of 5).

HIP events around back-to-back calls after a warm-up.  The variants of one
case are timed in turn, five rounds of >= --min-seconds each, and the median,
minimum and maximum of the rounds are reported, so that a difference can be
read against the spread.  One JSON line per measurement.

  python tools/ec_cand_bench.py [--scales 0.3 6 400] [--min-seconds 0.2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import rav1e_amd as R  # noqa: E402
from ec_mode_bench import frame_jobs  # noqa: E402
from ec_rate_bench import round_jobs  # noqa: E402
from tests.test_ec_util import rand_coeffs  # noqa: E402

ROUNDS = 5


def timed_rounds(L, variants, min_seconds):
    """variants: name -> launch().  Returns name -> [seconds per call] * ROUNDS,
    the variants alternating inside every round."""
    e0, e1 = L.rv_event_create(), L.rv_event_create()

    def window(fn, reps):
        L.rv_event_record(e0, None)
        for _ in range(reps):
            fn()
        L.rv_event_record(e1, None)
        L.rv_event_sync(e1)
        return L.rv_event_elapsed_ms(e0, e1) * 1e-3

    reps = {}
    for name, fn in variants.items():  # warm-up, and the repeats that fill a window
        window(fn, 10)
        r, t = 10, window(fn, 10)
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


def checked(L, rc):
    if rc != R.RV_OK:
        raise R.Rav1eHipError(L.rv_last_error().decode())


def counter_variants(L, tok, off, gf, cdf_all, total):
    """The four launches over one token array, their rate buffers"""
    ng = len(gf) - 1
    dtok, doff = R.DeviceBuffer.from_array(tok), R.DeviceBuffer.from_array(off)
    dgf = R.DeviceBuffer.from_array(gf)
    dold = R.DeviceBuffer.from_array(np.ascontiguousarray(cdf_all[:total]))
    dall = R.DeviceBuffer.from_array(cdf_all)
    dst = R.DeviceBuffer(4)
    rate = {k: R.DeviceBuffer(4 * ng) for k in ("batch", "stream_w1", "stream_w2", "stream_w4")}
    keep = (dtok, doff, dgf, dold, dall, dst)
    v = {"batch": lambda: checked(L, L.rv_ec_rate_batch(
        dtok.ptr, doff.ptr, dgf.ptr, ng, dold.ptr, 1, None, None, rate["batch"].ptr, dst.ptr, None))}
    for w in (1, 2, 4):
        v["stream_w%d" % w] = lambda w=w: checked(L, L.rv_ec_rate_stream_batch_waves(
            dtok.ptr, doff.ptr, dgf.ptr, ng, dall.ptr, 1, None, None, rate["stream_w%d" % w].ptr,
            dst.ptr, w, None))
    return v, rate, keep


def report_counters(L, a, case, extra, tok, off, gf, cdf_all, total):
    ng = len(gf) - 1
    v, rate, keep = counter_variants(L, tok, off, gf, cdf_all, total)
    t, reps = timed_rounds(L, v, a.min_seconds)
    L.rv_stream_sync(None)
    base = rate["batch"].download(np.uint32, ng)
    for name in v:
        assert (rate[name].download(np.uint32, ng) == base).all(), name
    for name in v:
        print(json.dumps(dict(
            {"kernel": "rv_ec_rate_batch" if name == "batch" else "rv_ec_rate_stream_batch",
             "case": case, "variant": name, "groups": ng, "tokens": int(off[gf[-1]] - off[gf[0]]),
             "repeats": reps[name], "rounds": ROUNDS, "us_per_call": us(t[name]),
             "over_batch": round(float(np.median(t[name]) / np.median(t["batch"])), 3)}, **extra)),
            flush=True)
    return base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--scales", type=float, nargs="+", default=[0.3, 6.0, 400.0])
    ap.add_argument("--cand-scale", type=float, default=6.0)
    ap.add_argument("--qctx", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    a = ap.parse_args()
    R.require_device(0)
    L = R.lib()
    sbw, sbh = (a.width + 63) // 64, (a.height + 63) // 64
    cdf_all = R.ec_default_cdf_all(a.qctx)
    total = L.rv_ec_cdf_total()

    # ---- stream: coefficient-only streams through both counters
    for scale in a.scales:
        jobs, co, gf = round_jobs(np.random.default_rng(7), sbw, sbh, scale)
        _, tok, off = R.coefficient_rates(jobs, co, gf, cdf_all[:total], 1, 1)
        per_group = np.diff(off[gf].astype(np.int64))
        rates = report_counters(L, a, "coefficients", {
            "scale": scale, "tokens_per_group": {"median": int(np.median(per_group)),
                                                 "max": int(per_group.max())}},
            tok, off, gf, cdf_all, total)
        for g in range(0, len(gf) - 1, max(1, (len(gf) - 1) // 16)):
            want = R.ec_count_stream(tok[off[gf[g]]:off[gf[g + 1]]], cdf_all.copy())[0]
            assert int(rates[g]) == want & 0xFFFFFFFF, g

    # ---- copy: one token per group, so the snapshot copy is what is left
    ng = sbw * sbh
    one = np.full(ng, 3 << 13, np.uint32)  # txb_skip context 0, symbol 0
    ar = np.arange(ng + 1, dtype=np.int32)
    report_counters(L, a, "one token per group", {}, one, ar.astype(np.uint32), ar, cdf_all, total)

    # ---- cand: whole candidates end to end
    rng = np.random.default_rng(11)
    cols, rows = sbw * 16, sbh * 16  # whole superblock rows: every 64x64 leaf is legal
    mode = frame_jobs(rng, cols, rows, 6)
    prm = R.EcModeParams(R.FRAME_INTER, 1, 0, 0, 0, 0, ((cols, rows),))
    crow, co, nco, cands = [(3, 0, 0, 0, 0, 0, 0, 0, 0, 0)], [], 0, []
    blocks = np.nonzero(mode["kind"] == 0)[0]
    for i in blocks:
        j = mode[i]
        bx, by = int(j["bx"]), int(j["by"])
        if bx == 0:
            crow.append((2, 0, 0, 0, 0, 0, 0, 0, 0, 0))
        if j["skip"]:
            crow.append((1, 0, bx, by, 0, 0, 0, 6, 6, 0))
            cands.append((mode[i - 1], j, []))
            continue
        tx = []
        for p in range(3):
            c = rand_coeffs(rng, 32, a.cand_scale if p == 0 else a.cand_scale / 2)
            tx.append((0, p, bx, by, 3 if p else 4, 0, int(j["luma_mode"] >= 14), 5 if p else 6,
                       5 if p else 6, nco))
            co.append(c)
            nco += len(c)
        crow += tx
        cands.append((mode[i - 1], j, tx))
    co = np.concatenate(co).astype(np.int32)
    # the frame's own blocks are the committed state: a candidate reads only
    # what lies above and left of it
    state = R.EcCodingState(mode, np.array(crow, np.int64), co, prm, 1, 1)
    want, tok, off, rejected, bad = R.ec_candidate_rates(state, cands, cdf_all, check=False)
    assert (rejected, bad) == (0, 0), (rejected, bad)
    cd, mj, trows, tiles = R.pack_candidates(cands, check=False)
    n, ntx = len(cd), len(trows)
    ej = np.zeros(ntx, R.EC_JOB)
    for k, f in enumerate(["kind", "plane", "bx", "by", "tx_size", "tx_type", "is_inter", "bw_lg",
                           "bh_lg"]):
        ej[f] = trows[:, k]
    ej["tile"] = tiles
    ej["coeffs"] = state.co.ptr + 4 * trows[:, 9].astype(np.uint64)
    cap = int(off[-1]) + 1024
    dc, dm, dt = (R.DeviceBuffer.from_array(x) for x in (cd, mj, ej))
    scr = R.DeviceBuffer(L.rv_ec_cand_scratch_bytes(n, ntx) + 16)
    doff, dtok, dst = R.DeviceBuffer(4 * (n + 1)), R.DeviceBuffer(4 * cap), R.DeviceBuffer(16)
    dcdf, drate = R.DeviceBuffer.from_array(cdf_all), R.DeviceBuffer(4 * n)
    head = (dc.ptr, n, dm.ptr, len(mj), dt.ptr, ntx, prm.c_struct(), 1, state.ddim.ptr, 1, 1,
            state.mw4, state.mh4, state.coef_map.ptr, state.mw8, state.mh8, state.mode_map.ptr,
            scr.ptr, doff.ptr, dtok.ptr, cap)
    v = {"cand_rates": lambda: checked(L, L.rv_ec_cand_rates(*head, dcdf.ptr, 1, None, None,
                                                             drate.ptr, dst.ptr, None)),
         "cand_tokenize": lambda: checked(L, L.rv_ec_cand_tokenize(*head, dst.ptr, None))}
    t, reps = timed_rounds(L, v, a.min_seconds)
    v["cand_rates"]()
    L.rv_stream_sync(None)
    assert (drate.download(np.uint32, n) == want).all()
    # the yardstick: the host counter over every candidate's stream, one core
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        for g in range(n):
            c2 = cdf_all.copy()
            r = L.rv_ec_count_stream(tok[off[g]:].ctypes.data, int(off[g + 1] - off[g]),
                                     c2.ctypes.data, None)
            assert r & 0xFFFFFFFF == int(want[g])
        host.append(time.perf_counter() - t0)
    per = np.diff(off.astype(np.int64))
    for name in v:
        print(json.dumps({
            "kernel": "rv_ec_" + name, "case": "mixed candidates", "scale": a.cand_scale,
            "candidates": n, "transform_blocks": ntx,
            "skip_candidates": int((cd["tx_count"] == 0).sum()), "tokens": int(off[-1]),
            "mode_tokens": int(((tok >> 31 == 0) & ((tok & 0x1FFF) >= total)).sum()),
            "tokens_per_candidate": {"median": int(np.median(per)), "max": int(per.max())},
            "repeats": reps[name], "rounds": ROUNDS, "us_per_call": us(t[name]),
            "host_count_stream_us": round(float(np.median(host)) * 1e6, 1),
            "device_over_host": round(float(np.median(host) / np.median(t[name])), 2)}), flush=True)


if __name__ == "__main__":
    main()

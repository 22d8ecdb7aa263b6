#!/usr/bin/env python3
"""Time rv_ec_rate_batch on the candidates of one round of a 3840 x 2160 4:2:0
frame: 60 x 34 = 2040 superblocks, one group each of a 64x64 luma block
(coded 32x32) and its two 32x32 chroma blocks, coefficients from the entropy
tests' rand_coeffs at scales 0.3 (near-empty), 6 and 400 (Golomb range).

HIP events around back-to-back launches after a warm-up, enough repeats to
fill half a second.  Prints one JSON line per scale: microseconds per call,
tokens per second, the tokens-per-group distribution, and the yardstick --
the host range coder rv_ec_code_tokens over the same tokens on one core, in
tokens per second (median of 5 runs).  The kernel is bound by the dependent
chain of a token (LDS read -> lane reads -> the scalar range update -> LDS
write, ordered against the next token's read), not by bandwidth: a group is
one wavefront's serial walk, the groups of a round run side by side.

  python tools/ec_rate_bench.py [--width 3840 --height 2160 --scales 0.3 6 400]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rav1e_amd as R  # noqa: E402
from tests.test_ec_util import rand_coeffs  # noqa: E402


def round_jobs(rng, sbw, sbh, scale):
    jobs, co, nco = [(3, 0, 0, 0, 0, 0, 0, 0, 0, 0)], [], 0
    first = []
    for sby in range(sbh):
        jobs.append((2, 0, 0, 0, 0, 0, 0, 0, 0, 0))
        for sbx in range(sbw):
            first.append(len(jobs))
            for p in range(3):
                c = rand_coeffs(rng, 32, scale if p == 0 else scale / 2)
                jobs.append((0, p, sbx * 16, sby * 16, 3 if p else 4, 0, 1, 5 if p else 6,
                             5 if p else 6, nco))
                co.append(c)
                nco += len(c)
    first.append(len(jobs))
    return np.array(jobs, np.int64), np.concatenate(co).astype(np.int32), np.array(first, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--scales", type=float, nargs="+", default=[0.3, 6.0, 400.0])
    ap.add_argument("--qctx", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    R.require_device(0)
    L = R.lib()
    sbw, sbh = (a.width + 63) // 64, (a.height + 63) // 64
    cdf = R.ec_default_cdf(a.qctx)
    for scale in a.scales:
        rng = np.random.default_rng(7)
        jobs, co, gf = round_jobs(rng, sbw, sbh, scale)
        ng = len(gf) - 1
        # the checked wrapper first: the tokens, and the rates to compare with
        rates, tok, off = R.coefficient_rates(jobs, co, gf, cdf, 1, 1)
        per_group = np.diff(off[gf].astype(np.int64))
        for g in range(0, ng, max(1, ng // 16)):
            want = R.ec_count_tokens(tok[off[gf[g]]:off[gf[g + 1]]], cdf.copy())[0]
            assert int(rates[g]) == want, (g, int(rates[g]), want)
        dtok, doff = R.DeviceBuffer.from_array(tok), R.DeviceBuffer.from_array(off)
        dgf, dcdf = R.DeviceBuffer.from_array(gf), R.DeviceBuffer.from_array(cdf)
        drate, dst = R.DeviceBuffer(4 * ng), R.DeviceBuffer(4)

        def launch(reps):
            for _ in range(reps):
                rc = L.rv_ec_rate_batch(dtok.ptr, doff.ptr, dgf.ptr, ng, dcdf.ptr, 1, None, None,
                                        drate.ptr, dst.ptr, None)
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
        assert (drate.download(np.uint32, ng) == rates).all()
        per_call = t / reps
        # the yardstick: the host range coder over the same tokens, one core
        out = np.zeros(tok.size // 2 + 4096, np.uint8)
        host = []
        for _ in range(5):
            c2 = cdf.copy()
            t0 = time.perf_counter()
            nb = L.rv_ec_code_tokens(tok.ctypes.data, tok.size, c2.ctypes.data, out.ctypes.data,
                                     out.size)
            host.append(time.perf_counter() - t0)
            assert nb > 0
        host_s = float(np.median(host))
        dev_tps, host_tps = tok.size / per_call, tok.size / host_s
        print(json.dumps({
            "kernel": "rv_ec_rate_batch", "width": a.width, "height": a.height, "scale": scale,
            "groups": ng, "tokens": int(tok.size), "repeats": reps, "seconds": round(t, 4),
            "us_per_call": round(per_call * 1e6, 2), "tokens_per_s": round(dev_tps),
            "tokens_per_group": {"min": int(per_group.min()),
                                 "median": int(np.median(per_group)),
                                 "p90": int(np.percentile(per_group, 90)),
                                 "max": int(per_group.max())},
            "raw_bit_share": round(float(np.mean(tok >> 31)), 3),
            "host_coder_us": round(host_s * 1e6, 1), "host_coder_tokens_per_s": round(host_tps),
            "device_over_host": round(dev_tps / host_tps, 2),
            "bound": "dependent chain per token"}), flush=True)
        L.rv_event_destroy(e0)
        L.rv_event_destroy(e1)


if __name__ == "__main__":
    main()

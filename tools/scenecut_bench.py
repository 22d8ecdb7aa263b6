#!/usr/bin/env python3
"""Time rv_frame_delta_batch: the steady-state call of the scene-change
detector (6 frames, the newest against the 5 before it: 5 pairs) and the
general one (6 frames, the 9 pairs of exclude_scene_flashes), on

  2160p 8-bit, luma only            (fast mode: speed 10)
  2160p 10-bit 4:2:0, three planes  (YUV mode: below speed 10)

HIP events around back-to-back calls after a warm-up, enough repeats to fill
half a second.  The calls rotate over several windows of frames whose total
size is past the 256 MiB Infinity Cache, so the pixels come from HBM, as they
do in a stream.  Beside each rate stands that of a plain device-to-device
copy (hipMemcpyAsync) of the same frame allocations, rotated the same way
and measured in the same run: the copy, not a nominal peak, is the yardstick.
A copy reads and writes every byte, the kernel only reads, so the copy moves
twice the traffic per counted byte.

Prints one JSON line per measurement: microseconds per call, algorithmic
bytes (the visible planes of every frame of the window, read once) and GB/s.

  python tools/scenecut_bench.py [--width 3840 --height 2160 --min-seconds 0.5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rav1e_amd as R  # noqa: E402

STEADY = [(i, 5) for i in range(5)]
GENERAL = [(0, j) for j in range(1, 6)] + [(i, 5) for i in range(1, 5)]
CACHE_BYTES = 256 << 20


def make_window(rng, w, h, bd, n_planes):
    dtype = np.uint16 if bd > 8 else np.uint8
    frames = []
    for _ in range(6):
        planes = []
        for k in range(n_planes):
            s = (h, w) if k == 0 else ((h + 1) >> 1, (w + 1) >> 1)
            # a few random rows tiled: cheap to make, no two frames alike
            rows = rng.integers(0, 1 << bd, (8, s[1])).astype(dtype)
            img = np.tile(rows, ((s[0] + 7) // 8, 1))[:s[0]]
            planes.append(R.DevicePlane.from_array(img, xpad=16, ypad=16, xdec=1 if k else 0,
                                                   ydec=1 if k else 0, bit_depth=bd))
        frames.append(tuple(planes))
    return frames


def timed(L, fn, min_seconds):
    e0, e1 = L.rv_event_create(), L.rv_event_create()

    def run(reps):
        L.rv_event_record(e0, None)
        for i in range(reps):
            fn(i)
        L.rv_event_record(e1, None)
        L.rv_event_sync(e1)
        return L.rv_event_elapsed_ms(e0, e1) * 1e-3

    run(20)  # warm-up
    reps = 50
    t = run(reps)
    while t < min_seconds:
        reps = int(reps * max(2.0, 1.2 * min_seconds / max(t, 1e-6)))
        t = run(reps)
    L.rv_event_destroy(e0)
    L.rv_event_destroy(e1)
    return t / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    R.require_device(0)
    L = R.lib()
    rng = np.random.default_rng(7)
    for name, bd, n_planes in (("luma 8-bit (fast mode)", 8, 1), ("4:2:0 10-bit (YUV mode)", 10, 3)):
        px = 2 if bd > 8 else 1
        windows = [make_window(rng, a.width, a.height, bd, n_planes)]
        visible = 6 * sum(p.desc.width * p.desc.height * px for p in windows[0][0])
        alloc = sum(p.buf.nbytes for f in windows[0] for p in f)
        while len(windows) * alloc < 2 * CACHE_BYTES:
            windows.append(make_window(rng, a.width, a.height, bd, n_planes))
        descs = [(R.RvPlane * (6 * n_planes))(*(p.desc for f in win for p in f)) for win in windows]
        out = R.DeviceBuffer(8 * 16 * 3)
        results = {}
        for label, pairs in (("steady", STEADY), ("general", GENERAL)):
            # through the checked wrapper once: the sums the timed calls must give
            first = R.frame_deltas(windows[0], pairs)
            pa = np.ascontiguousarray(pairs, dtype=np.int32)

            def call(i, pa=pa):
                rc = L.rv_frame_delta_batch(descs[i % len(windows)], 6, n_planes, pa.ctypes.data,
                                            len(pa), out.ptr, None)
                if rc != R.RV_OK:
                    raise R.Rav1eHipError(L.rv_last_error().decode())
            per_call, reps = timed(L, call, a.min_seconds)
            call(0)
            R._sync()
            assert (out.download(np.uint64, len(pa) * n_planes).reshape(len(pa), n_planes) ==
                    first).all()
            results[label] = (per_call, reps, len(pa))
        # the copy of the same allocations (padding included: alloc bytes)
        dst = [R.DeviceBuffer(p.buf.nbytes) for p in windows[0][0]]

        def copy(i):
            for f in windows[i % len(windows)]:
                for p, d in zip(f, dst):
                    L.rv_memcpy_d2d(d.ptr, p.buf.ptr, p.buf.nbytes, None)
        copy_call, copy_reps = timed(L, copy, a.min_seconds)
        copy_gbs = alloc / copy_call / 1e9
        for label, (per_call, reps, n_pairs) in results.items():
            gbs = visible / per_call / 1e9
            print(json.dumps({
                "kernel": "rv_frame_delta_batch", "case": name, "call": label, "width": a.width,
                "height": a.height, "bit_depth": bd, "planes": n_planes, "frames": 6,
                "pairs": n_pairs, "windows_rotated": len(windows), "repeats": reps,
                "us_per_call": round(per_call * 1e6, 2), "bytes_per_call": visible,
                "GB_per_s": round(gbs, 1), "copy_bytes_per_call": alloc,
                "copy_us_per_call": round(copy_call * 1e6, 2),
                "copy_GB_per_s": round(copy_gbs, 1), "ratio_to_copy": round(gbs / copy_gbs, 3)}),
                flush=True)
        del windows, descs, dst


if __name__ == "__main__":
    main()

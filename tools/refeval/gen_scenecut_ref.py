"""Golden vectors for scene-change detection, produced by RUNNING the
reference's own Rust function text (rsinterp.py) -- needs the reference
checkout that gen_golden_ref.py reads:

    python tools/refeval/gen_scenecut_ref.py

Functions evaluated: PixelIter::new / width / height / next (src/frame/mod.rs:
126-172) and SceneChangeDetector::new / analyze_next_frame / is_key_frame /
exclude_scene_flashes / has_scenecut (src/scenechange/mod.rs).  Host side:
the frames (three rshost Planes and an iter() that steps the interpreted
PixelIter), BTreeSet, and the three settings the functions read.  The sums
and delta_avg are local to has_scenecut: they are recorded as the interpreter
binds `delta_yuv` / `delta_avg` and returns from `sum`.  Only the resulting
numbers are written (tests/golden/ref_scenecut.npz); tests/test_scenecut.py
checks tests/scenecut_ref.py against them.

pair_*: one has_scenecut per case in YUV mode and one in fast mode.
seq_*: analyze_next_frame over a sequence, called as compute_lookahead_data
calls it (frame N with the frames N .. N + 6 that the queue then holds, fewer
at the end); keyframes and excluded_frames after every call as bit masks.
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "ref_scenecut.npz")
SIZES = ((16, 10), (17, 9), (9, 7), (4, 4))
SAMPLINGS = ((1, 1), (1, 0), (0, 0))
DISTANCE = 5  # keyframe_lookahead_distance() with the reorder pyramid


def u64(v):
    return RI.TInt(int(v), "u64")


class BTreeSet:
    def __init__(self, items=()):
        self.s = set(int(v) for v in items)

    @staticmethod
    def new():
        return BTreeSet()

    def insert(self, v):
        self.s.add(int(RI.deref(v)))

    def contains(self, v):
        return int(RI.deref(v)) in self.s

    def iter(self):
        return RI.It(iter([u64(v) for v in sorted(self.s)]))

    def mask(self):
        return sum(1 << v for v in self.s)


class Frame:
    """Frame<T>: the planes, and iter() = PixelIter::new(&self.planes) of the
    reference's text, stepped by its own next()."""

    def __init__(self, I, arrays, xdec, ydec, bd):
        self.I = I
        ty = "u8" if bd == 8 else "u16"
        self.planes = []
        for k, a in enumerate(arrays):
            pl = H.Plane.from_full(np.asarray(a, np.int64), 0, 0, a.shape[1], a.shape[0],
                                   xdec if k else 0, ydec if k else 0)
            pl.data = [RI.TInt(int(v), ty) for v in pl.data]
            self.planes.append(pl)

    def iter(self):
        I = self.I
        it = I.make_method("PixelIter", "new", None, I.globals)(self.planes)
        nxt = I.make_method("PixelIter", "next", it, I.globals)

        def items():
            while True:
                o = RI.deref(nxt())
                if o is None:
                    return
                yield o
        return RI.It(items())


class _NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Log:
    """What has_scenecut computes on the way: hooks on the interpreter."""

    def __init__(self, I):
        self.rows = []
        bind0 = I.bind

        def bind(pat, v, env):
            if pat[0] == "bind" and pat[1] in ("delta_yuv", "delta_avg"):
                self.rows.append((pat[1], v))
            return bind0(pat, v, env)
        I.bind = bind
        iter0 = RI._iter_method

        def iter_method(g, name, args, gty):
            r = iter0(g, name, args, gty)
            if name == "sum":
                self.rows.append(("sum", r))
            return r
        RI._iter_method = iter_method

    def take(self):
        r, self.rows = self.rows, []
        return r


def interp():
    I = G.make_interp()
    I.release = True
    fr = RI.Source(G.REF + "frame/mod.rs")
    sc = RI.Source(G.REF + "scenechange/mod.rs")
    I.sources += [fr, sc]
    for name, src in (("PixelIter", fr), ("SceneChangeDetector", sc)):
        fns = []
        for m in re.finditer(r"\bimpl\b[^{;]*\b%s\b[^{;]*\{" % name, src.src):
            fns += RI.parse_impl_fns(RI.find_item(src.src, "impl", name, m.start()))
        I.define_impl(name, fns)
        I.globals.vars[name] = RI.StructType(name)
    assert set(I.impls["PixelIter"]) == {"new", "width", "height", "next"}
    assert set(I.impls["SceneChangeDetector"]) == {
        "new", "analyze_next_frame", "is_key_frame", "exclude_scene_flashes", "has_scenecut"}
    I.globals.vars["BTreeSet"] = BTreeSet
    return I


def detector(I, bd, fast):
    return I.make_method("SceneChangeDetector", "new", None, I.globals)(
        RI.TInt(bd, "u8"), bool(fast))


def chroma_shape(w, h, xdec, ydec):
    return (h + ydec) >> ydec, (w + xdec) >> xdec


def gen_pairs(I, log, rng, out):
    meta, data, off, sums, fast_sum, avg, cut = [], [], [0], [], [], [], []
    k = 0
    for (w, h) in SIZES:
        for (xdec, ydec) in SAMPLINGS:
            for bd in (8, 10, 12):
                maxv = (1 << bd) - 1
                thr = 12 * bd // 8
                # differences around the threshold: both answers occur
                spread = (thr * (k % 5 + 2)) // 2
                shapes = [(h, w)] + [chroma_shape(w, h, xdec, ydec)] * 2
                a = [rng.integers(0, maxv + 1, s) for s in shapes]
                b = [np.clip(p + rng.integers(-spread, spread + 1, p.shape) *
                             (1 if i == 0 or k % 3 else 0), 0, maxv) for i, p in enumerate(a)]
                if k % 7 == 3:  # only the pixel PixelIter never yields differs
                    b = [p.copy() for p in a]
                    b[0][-1, -1] = maxv - a[0][-1, -1]
                f1, f2 = Frame(I, a, xdec, ydec, bd), Frame(I, b, xdec, ydec, bd)
                row_avg, row_cut = [], []
                for fast in (False, True):
                    det = detector(I, bd, fast)
                    log.take()
                    r = I.make_method("SceneChangeDetector", "has_scenecut", det, I.globals)(f1, f2)
                    rows = log.take()
                    row_avg.append([int(v) for n, v in rows if n == "delta_avg"][0])
                    row_cut.append(bool(r))
                    if fast:
                        fast_sum.append([int(v) for n, v in rows if n == "sum"][0])
                    else:  # the first delta_yuv is the fold's, the second the u16 averages
                        sums.append([int(v) for v in [v for n, v in rows if n == "delta_yuv"][0]])
                meta.append((w, h, xdec, ydec, bd))
                for p in a + b:
                    data.append(p.ravel())
                    off.append(off[-1] + p.size)
                avg.append(row_avg)
                cut.append(row_cut)
                k += 1
        print("has_scenecut %dx%d: %d cases" % (w, h, k), flush=True)
    out["pair_meta"] = np.array(meta, np.int32)
    out["pair_px"] = np.concatenate(data).astype(np.uint16)
    out["pair_off"] = np.array(off, np.int64)
    out["pair_sums"] = np.array(sums, np.uint64)
    out["pair_fast_sum"] = np.array(fast_sum, np.uint64)
    out["pair_avg"] = np.array(avg, np.int64)
    out["pair_cut"] = np.array(cut, np.bool_)
    assert out["pair_cut"].any(axis=0).all() and not out["pair_cut"].all(axis=0).any()


# (w, h, (xdec, ydec), bit depth, fast_mode, min interval, max interval,
#  forced key frame or -1, scene of every frame: a letter, lower case = the
#  same scene with other noise)
SEQUENCES = (
    (16, 10, (1, 1), 8, True, 0, 240, -1, "AAABBBBBBAcAAAA"),    # a cut, a one-frame flash
    (17, 9, (1, 1), 10, False, 0, 240, -1, "AABBCCDDEEEEEEE"),   # the staircase of :149-153
    (9, 7, (1, 0), 12, False, 2, 6, -1, "AAAAAAAAABAAAA"),       # max interval, min interval
    (4, 4, (0, 0), 8, False, 0, 240, 3, "AAAABBAAAAAA"),         # a forced key, a two-frame flash
    (9, 7, (1, 0), 10, True, 0, 240, -1, "AB"),                  # two frames: distance 1
    (4, 4, (0, 0), 12, True, 0, 4, -1, "AAAAAABBBBBBB"),
    (16, 10, (1, 0), 8, False, 0, 240, -1, "ABBBBBBBAAAAAAA"),
    (17, 9, (0, 0), 10, True, 3, 240, -1, "AABAAAAAABBBB"),
)


def gen_sequences(I, log, rng, out):
    meta, data, off, calls = [], [], [0], []
    for si, (w, h, (xdec, ydec), bd, fast, min_kf, max_kf, forced, scenes) in enumerate(SEQUENCES):
        maxv = (1 << bd) - 1
        shapes = [(h, w)] + [chroma_shape(w, h, xdec, ydec)] * 2
        base = {}
        frames = []
        for ch in scenes:
            if ch.upper() not in base:  # scenes far apart: level steps of a quarter range
                lvl = (len(base) * 5 % 4) * (maxv // 4) + maxv // 16
                base[ch.upper()] = [np.clip(lvl + rng.integers(0, maxv // 8, s), 0, maxv)
                                    for s in shapes]
            px = [np.clip(p + rng.integers(-2, 3, p.shape), 0, maxv) for p in base[ch.upper()]]
            frames.append(Frame(I, px, xdec, ydec, bd))
            for p in px:
                data.append(p.ravel())
                off.append(off[-1] + p.size)
        det = detector(I, bd, fast)
        analyze = I.make_method("SceneChangeDetector", "analyze_next_frame", det, I.globals)
        config = _NS(min_key_frame_interval=u64(min_kf), max_key_frame_interval=u64(max_kf),
                     speed_settings=_NS(no_scene_detection=False))
        inter_cfg = _NS(keyframe_lookahead_distance=lambda: u64(DISTANCE))
        keyframes = BTreeSet()
        keyframes_forced = BTreeSet([forced] if forced >= 0 else [])
        n = len(frames)
        for N in range(n):
            # compute_lookahead_data: frame N is analysed when the queue ends at
            # N + distance + 1, or holds everything
            frame_set = frames[N:min(n, N + DISTANCE + 2)]
            log.take()
            analyze(frames[N - 1] if N else None, frame_set, u64(N), config, inter_cfg, keyframes,
                    keyframes_forced)
            compared = sum(1 for name, _ in log.take() if name == "delta_avg")
            calls.append((si, N, len(frame_set), compared, keyframes.mask(),
                          det.excluded_frames.mask()))
        meta.append((w, h, xdec, ydec, bd, int(fast), min_kf, max_kf, forced, n))
        print("sequence %d (%s): keyframes %s excluded %s" % (
            si, scenes, sorted(keyframes.s), sorted(det.excluded_frames.s)), flush=True)
    out["seq_meta"] = np.array(meta, np.int32)
    out["seq_px"] = np.concatenate(data).astype(np.uint16)
    out["seq_off"] = np.array(off, np.int64)
    out["seq_calls"] = np.array(calls, np.int64)


def main():
    I = interp()
    log = Log(I)
    rng = np.random.default_rng(20261020)
    out = {}
    gen_pairs(I, log, rng, out)
    gen_sequences(I, log, rng, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

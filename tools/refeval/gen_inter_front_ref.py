"""Golden vectors for the inter front of rdo_mode_decision: get_params and
PlaneSlice::clamp, predict_inter's pixels through motion_compensate's plane
loop, the reference sets and the inter mode set -- needs the reference
checkout that gen_golden_ref.py reads:

    python tools/refeval/gen_inter_front_ref.py

Evaluated from the reference's own text (rsinterp.py):
  PredictionMode::predict_inter with its nested get_params (src/predict.rs:
  255-338), PlaneSlice::clamp (src/frame/plane.rs:521-533),
  TileRect::decimated / to_frame_plane_offset (src/tiling/tile.rs:27-47),
  put_8tap_ref / prep_8tap_ref / mc_avg_ref and get_filter (src/mc.rs:182-408).
  For the get_params section put_8tap / prep_8tap are recorders: they keep the
  fracs and the slice they were handed.

Restated below in Python, because the interpreter is not taken through
rdo_mode_decision's ContextWriter / FrameInvariants / TileStateMut:
  motion_compensate's plane loop (src/encoder.rs:1259-1266, 1416-1428): the
  plane's block size, po and the decimated tile rect handed to predict_inter;
  the reference sets (src/rdo.rs:815-835, 914-927) and the inter mode set
  (src/rdo.rs:858-986), written as a transliteration over Python lists with
  the ArrayVec capacities and the indexing panics as exceptions.

Only the resulting numbers are written (tests/golden/ref_inter_front.npz);
tests/test_inter_front.py checks tests/inter_front_ref.py against them.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "ref_inter_front.npz")
LUMA_PAD = 88  # SB_SIZE + FRAME_MARGIN (src/frame/mod.rs:23, 60)


def usz(v):
    return RI.TInt(v, "usize")


def isz(v):
    return RI.TInt(v, "isize")


class Fi(G.Fi):
    """The FrameInvariants fields predict_inter reads."""

    def __init__(self, bd, slots, mode):
        super().__init__(bd)
        self.default_filter = usz(mode)
        self.slots = slots  # per DPB slot: the three planes
        self.ref_frames = [RI.TInt(0, "u8")] * 7
        self.plane(0)

    def plane(self, p):
        self.rec_buffer = RI.Struct("ReferenceFramesSet", {"frames": [
            RI.Struct("ReferenceFrame", {"frame": RI.Struct("Frame", {"planes": [s[0], s[1], s[2]]})})
            if s is not None else None for s in self.slots]})


def setup():
    I = G.make_interp()
    tile = RI.Source(G.REF + "tiling/tile.rs")
    I.define_impl("TileRect", tile.impl("TileRect"))
    I.globals.vars["TileRect"] = RI.StructType("TileRect")
    I.globals.vars["RefType"] = G._RefType
    I.globals.vars["NONE_FRAME"] = G._RefType.NONE_FRAME
    # AlignedArray<[i16; 128 * 128]> (src/util/align.rs): the prep tiles
    I.globals.vars["AlignedArray"] = type("AlignedArray", (), {"uninitialized": staticmethod(
        lambda: RI.Struct("AlignedArray", {"array": [RI.TInt(0, "i16")] * (128 * 128)}))})
    pred = RI.Source(G.REF + "predict.rs")
    G.PredModeV.fn = I.make_fn(pred.fn("predict_inter"), I.globals)
    # PlaneSlice::clamp from the reference's text, on rshost's slice
    pl = RI.Source(G.REF + "frame/plane.rs")
    I.globals.vars["PlaneSlice"] = RI.StructType("PlaneSlice")
    clamp = I.make_fn(pl.fn("clamp", "impl<'a, T: Pixel> PlaneSlice<'a, T>"), I.globals)

    def clamp_host(self):
        r = clamp(RI.Struct("PlaneSlice", {"plane": self.plane, "x": isz(self.x), "y": isz(self.y)}))
        return H.PlaneSlice(self.plane, int(r.x), int(r.y))
    H.PlaneSlice.clamp = clamp_host
    return I


def tile_rect(I, t, xdec, ydec):
    """luma_tile_rect.decimated(xdec, ydec) (src/encoder.rs:1266)"""
    r = RI.Struct("TileRect", {"x": usz(t[0]), "y": usz(t[1]), "width": usz(t[2]),
                               "height": usz(t[3])})
    return I.make_method("TileRect", "decimated", r, None)(usz(xdec), usz(ydec))


def predict(fi, bd, trect, p, po, w, h, refs, mvs, dst=None):
    """luma_mode.predict_inter(fi, tile_rect, p, po, dst, w, h, ref_frames, mvs)"""
    G.PredModeV.pixel = G.prim(bd)
    if dst is None:
        dst = H.Plane.from_full(np.zeros((h, w), np.int64), 0, 0, w, h)
    G.PredModeV(19).predict_inter(
        fi, trect, usz(p), RI.Struct("PlaneOffset", {"x": isz(po[0]), "y": isz(po[1])}),
        G.region_at(dst, 0, 0), usz(w), usz(h), [G.RefV(refs[0]), G.RefV(refs[1])],
        [H.motion_vector(*mvs[0]), H.motion_vector(*mvs[1])])
    return np.array(dst.data, np.int64).reshape(h, w)


def padded(vis, xdec, ydec):
    px, py = LUMA_PAD >> xdec, LUMA_PAD >> ydec
    return np.pad(vis, ((py, py), (px, px)), mode="edge"), px, py


def host_plane(vis, xdec, ydec):
    full, px, py = padded(vis, xdec, ydec)
    return H.Plane.from_full(full, px, py, vis.shape[1], vis.shape[0], xdec, ydec)


# ---------------------------------------------------------------- get_params
def gen_params(I, out):
    rec = []

    def recorder(dst, src, w, h, cf, rf, *a, **kw):
        rec.append((int(rf), int(cf), int(src.x), int(src.y)))
    I.globals.vars["put_8tap"] = recorder
    I.globals.vars["prep_8tap"] = recorder
    I.globals.vars["mc_avg"] = lambda *a, **kw: None
    comps = sorted(set(list(range(-17, 18)) + [-32768, -32767, 32767, -3000, 3000, -801, 799,
                                                 -1234, 1237, 20000, -20001, 100, -100, 1023]))
    W_, H_ = 48, 40
    rows = []
    for xdec, ydec in ((0, 0), (1, 1), (1, 0)):
        w, h = W_ >> xdec, H_ >> ydec
        pls = [host_plane(np.zeros((h, w), np.int64), xdec, ydec)] * 3
        fi = Fi(8, [pls] + [None] * 7, 0)
        t = (16, 8, 32, 32)
        trect = tile_rect(I, t, xdec, ydec)
        # positions in the tile's plane region: its corners and the middle
        tw, th = 32 >> xdec, 32 >> ydec
        poss = [(0, 0), (tw - 4, 0), (0, th - 4), (tw - 4, th - 4), (tw // 2, th // 2)]
        n = len(comps)
        for k, r in enumerate(comps):
            for c in (comps[(7 * k + 3) % n], comps[(11 * k + 5) % n]):
                for po in (poss[k % 5], poss[(k + 2) % 5]):
                    del rec[:]
                    predict(fi, 8, trect, 1 if xdec else 0, po, 4, 4, (1, 8), ((r, c), (0, 0)))
                    assert len(rec) == 1
                    rows.append((xdec, ydec, w, h, pls[0].cfg.xorigin, pls[0].cfg.yorigin,
                                 t[0], t[1], po[0], po[1], r, c) + rec[0])
        # every corner and side of the clamp, by large MVs from each position
        for po in poss:
            for r in (-32768, 0, 32767):
                for c in (-32768, 0, 32767):
                    del rec[:]
                    predict(fi, 8, trect, 0, po, 4, 4, (1, 8), ((r, c), (0, 0)))
                    rows.append((xdec, ydec, w, h, pls[0].cfg.xorigin, pls[0].cfg.yorigin,
                                 t[0], t[1], po[0], po[1], r, c) + rec[0])
    out["gp_cases"] = np.array(rows, np.int32)
    print("get_params: %d cases" % len(rows))


# ---------------------------------------------------------------- pixels
PIX_CASES = [  # (bsize, w, h, xdec, ydec)
    (3, 8, 8, 1, 1), (5, 16, 8, 1, 1), (4, 8, 16, 1, 1), (6, 16, 16, 0, 0)]


def gen_pixels(I, rng, out):
    put_ref, prep_ref, avg_ref = G.F(I, "put_8tap_ref"), G.F(I, "prep_8tap_ref"), G.F(I, "mc_avg_ref")
    W_, H_ = 48, 40
    tile = (16, 8, 32, 32)
    cases, pix = [], []
    for bd in (8, 10):
        g = {"T": G.prim(bd)}
        I.globals.vars["put_8tap"] = lambda *a, _g=g: put_ref(*a, generics=_g)
        I.globals.vars["prep_8tap"] = lambda *a, _g=g: prep_ref(*a, generics=_g)
        I.globals.vars["mc_avg"] = lambda *a, _g=g: avg_ref(*a, generics=_g)
        for fmt, (xdec, ydec) in enumerate(((1, 1), (0, 0))):
            vis = [[G.rand_plane(rng, H_ >> (ydec if p else 0), W_ >> (xdec if p else 0), bd)
                    for p in range(3)] for _ in range(2)]
            out["px_bd%d_f%d" % (bd, fmt)] = np.concatenate(
                [v.reshape(-1) for s in vis for v in s]).astype(np.uint16)
            slots = [[host_plane(v, xdec if p else 0, ydec if p else 0) for p, v in enumerate(s)]
                     for s in vis]
            for (b, bw, bh, xd, yd) in PIX_CASES:
                if (xd, yd) != (xdec, ydec):
                    continue
                for comp in (0, 1):
                    for clampd in (0, 1):
                        mode = int(rng.integers(0, 4))
                        fi = Fi(bd, slots + [None] * 6, mode)
                        fi.ref_frames = [RI.TInt(0, "u8")] * 4 + [RI.TInt(1, "u8")] * 3
                        bo = (int(rng.integers(0, 32 // bw + 1 - 1)) * (bw // 4),
                              int(rng.integers(0, 32 // bh + 1 - 1)) * (bh // 4))
                        mvs = [[int(v) for v in rng.integers(-90, 90, 2)] for _ in range(2)]
                        if clampd:  # far outside: the clamp engages on both axes
                            mvs[0] = [int(rng.choice([-1, 1])) * int(rng.integers(1500, 3000)) + 3,
                                      int(rng.choice([-1, 1])) * int(rng.integers(1500, 3000)) + 5]
                            mvs[1][1] = 8 * 400 + 2
                        refs = (1, 5) if comp else (1, 8)
                        # motion_compensate's plane loop (src/encoder.rs:1259-1266, 1416-1428)
                        for p in range(3):
                            pxd, pyd = (xd, yd) if p else (0, 0)
                            pw, ph = (bw >> pxd, bh >> pyd)
                            po = ((bo[0] >> pxd) << 2, (bo[1] >> pyd) << 2)  # plane_offset
                            trect = tile_rect(I, tile, pxd, pyd)
                            blk = predict(fi, bd, trect, p, po, pw, ph, refs, mvs)
                            pix.append(blk.reshape(-1))
                        cases.append((bd, fmt, b, comp, mode, bo[0], bo[1], mvs[0][0], mvs[0][1],
                                      mvs[1][0], mvs[1][1]))
                        print("  pixels bd%d %dx%d fmt%d comp%d clamp%d" % (bd, bw, bh, fmt, comp, clampd))
    out["px_cases"] = np.array(cases, np.int32)
    out["px_pred"] = np.concatenate(pix).astype(np.uint16)
    out["px_geom"] = np.array([W_, H_, LUMA_PAD] + list(tile), np.int32)


# ---------------------------------------------------------------- sets and modes
class Panic(Exception):
    pass


class ArrayVec(list):
    def __init__(self, cap):
        super().__init__()
        self.cap = cap

    def push(self, v):
        if len(self) >= self.cap:
            raise Panic("ArrayVec: capacity")
        self.append(v)


def rs_index(v, i):
    if not 0 <= i < len(v):
        raise Panic("index out of bounds")
    return v[i]


def rs_ref_sets(allowed, fi_ref_frames):
    """src/rdo.rs:815-835"""
    ref_frames_set, ref_slot_set = ArrayVec(7), ArrayVec(7)
    fwdref = bwdref = None
    for i in allowed:
        if i == 3:  # LAST3_FRAME
            continue
        if fi_ref_frames[i - 1] not in ref_slot_set:
            if fwdref is None and i < 5:
                fwdref = len(ref_frames_set)
            if bwdref is None and i >= 5:
                bwdref = len(ref_frames_set)
            ref_frames_set.push([i, 8])
            ref_slot_set.push(fi_ref_frames[i - 1])
    assert ref_frames_set
    return ref_frames_set, ref_slot_set, fwdref, bwdref


def rs_mode_set(ref_frames_set, fwdref, bwdref, stacks_in, me, near, ref_mode_not_single, w_mi, h_mi):
    """src/rdo.rs:837-986; stacks_in[i] = (mode_context, [(this_mv, comp_mv)...])
    stands for cw.find_mvrefs of set i, me[i] for motion_estimation."""
    ZERO = (0, 0)
    ref_frames_set = list(ref_frames_set)
    inter_mode_set, mv_stacks, mode_contexts, mvs_from_me = ArrayVec(20), ArrayVec(20), ArrayVec(7), []
    for i, ref_frames in enumerate(list(ref_frames_set)):
        mode_contexts.push(stacks_in[i][0])
        mv_stack = list(stacks_in[i][1])
        b_me = tuple(me[i])
        mvs_from_me.append([b_me, ZERO])
        inter_mode_set.push((14, i))  # RAV1E_INTER_MODES_MINIMAL
        if mv_stack:
            inter_mode_set.push((15, i))
        if len(mv_stack) >= 2:
            inter_mode_set.push((18, i))
        if near:
            if len(mv_stack) >= 3:
                inter_mode_set.push((16, i))
            if len(mv_stack) >= 4:
                inter_mode_set.push((17, i))
        same = lambda x: x[0][0] == mvs_from_me[i][0][0] and x[0][1] == mvs_from_me[i][0][1]  # noqa: E731
        if not any(same(x) for x in mv_stack[:4 if near else 2]) and \
                (mvs_from_me[i][0][0] != 0 or mvs_from_me[i][0][1] != 0):
            inter_mode_set.push((19, i))
        mv_stacks.push(mv_stack)
    sz = min(w_mi, h_mi)
    if ref_mode_not_single and sz >= 2:
        if fwdref is not None and bwdref is not None:
            ref_frames = [ref_frames_set[fwdref][0], ref_frames_set[bwdref][0]]
            ref_frames_set.append(ref_frames)
            mvs_from_me.append([mvs_from_me[fwdref][0], mvs_from_me[bwdref][0]])
            k = len(ref_frames_set) - 1
            mode_contexts.push(stacks_in[k][0])
            for x in (26, 20, 27, 22, 23, 21):  # RAV1E_INTER_COMPOUND_MODES
                inter_mode_set.push((x, k))
            mv_stacks.push(list(stacks_in[k][1]))
    res = []
    for luma_mode, i in inter_mode_set:
        if luma_mode in (19, 27):
            mvs = mvs_from_me[i]
        elif luma_mode in (14, 20):
            mvs = [mv_stacks[i][0][0], mv_stacks[i][0][1]] if mv_stacks[i] else [ZERO, ZERO]
        elif luma_mode in (15, 21):
            mvs = [mv_stacks[i][1][0], mv_stacks[i][1][1]] if len(mv_stacks[i]) > 1 else [ZERO, ZERO]
        elif luma_mode in (16, 17):
            e = rs_index(mv_stacks[i], luma_mode - 15 + 1)
            mvs = [e[0], e[1]]
        elif luma_mode == 22:
            mvs = [rs_index(mv_stacks[i], 0)[0], mvs_from_me[i][1]]
        elif luma_mode == 23:
            mvs = [mvs_from_me[i][0], rs_index(mv_stacks[i], 0)[1]]
        else:
            mvs = [ZERO, ZERO]
        res.append((luma_mode, i, ref_frames_set[i][0], ref_frames_set[i][1], mvs[0][0], mvs[0][1],
                    mvs[1][0], mvs[1][1], mode_contexts[i]))
    return res


def rand_stack(rng, n, me=None, dup_at=None):
    st = [((int(rng.integers(-200, 200)), int(rng.integers(-200, 200))),
           (int(rng.integers(-200, 200)), int(rng.integers(-200, 200)))) for _ in range(n)]
    if dup_at is not None and dup_at < n:
        st[dup_at] = (tuple(me), st[dup_at][1])
    return st


def gen_modes(rng, out):
    ALL = [1, 2, 3, 4, 5, 6, 7]
    set_cases = [  # (allowed, fi.ref_frames, reference_mode != SINGLE, bsize)
        (ALL, [0, 1, 2, 3, 4, 5, 6], 1, 6), (ALL, [0, 1, 2, 3, 4, 5, 6], 0, 6),
        (ALL, [0, 0, 0, 0, 1, 1, 1], 1, 6), (ALL, [0, 1, 2, 0, 0, 0, 0], 1, 9),
        ([1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 6], 1, 6), ([1], [3, 1, 2, 3, 4, 5, 6], 1, 12),
        (ALL, [2, 2, 5, 2, 7, 7, 2], 1, 3), (ALL, [0, 1, 2, 3, 4, 5, 6], 1, 0),
        (ALL, [0, 1, 2, 3, 4, 5, 6], 1, 1), (ALL, [0, 1, 2, 3, 4, 5, 6], 1, 2),
        (ALL, [0, 0, 0, 0, 0, 0, 0], 1, 6), (ALL, [4, 4, 1, 4, 4, 6, 6], 1, 10),
        (ALL, [0, 0, 7, 0, 3, 3, 3], 1, 16), (ALL, [0, 0, 7, 0, 3, 3, 3], 1, 13)]
    rs_rows = []
    for allowed, rf, rm, b in set_cases:
        fs, ss, fwd, bwd = rs_ref_sets(allowed, rf)
        bs = H.BlockSizeV(b)
        comp = int(bool(rm) and min(bs.w, bs.h) // 4 >= 2 and fwd is not None and bwd is not None)
        row = [len(allowed)] + allowed + [0] * (7 - len(allowed)) + rf + [rm, b, len(fs)]
        row += [f[0] for f in fs] + [0] * (7 - len(fs)) + list(ss) + [0] * (7 - len(ss))
        row += [-1 if fwd is None else fwd, -1 if bwd is None else bwd, comp]
        rs_rows.append(row)
    out["rs_cases"] = np.array(rs_rows, np.int32)

    cfg, stk, mes, cnt, cands = [], [], [], [], []

    def add(allowed, rf, rm, b, near, stacks, me):
        fs, ss, fwd, bwd = rs_ref_sets(allowed, rf)
        bs = H.BlockSizeV(b)
        try:
            res = rs_mode_set(fs, fwd, bwd, stacks, me, near, rm, bs.w // 4, bs.h // 4)
            n = len(res)
        except Panic:
            res, n = [], -1
        comp = int(bool(rm) and min(bs.w, bs.h) // 4 >= 2 and fwd is not None and bwd is not None)
        cfg.append([len(fs), comp, -1 if fwd is None else fwd, -1 if bwd is None else bwd, near] +
                   [f[0] for f in fs] + [0] * (7 - len(fs)) + list(ss) + [0] * (7 - len(ss)))
        s = np.zeros((8, 2 + 36), np.int32)
        for i, (ctx, st) in enumerate(stacks):
            s[i, 0], s[i, 1] = ctx, len(st)
            for k, (a, c) in enumerate(st):
                s[i, 2 + 4 * k:6 + 4 * k] = (a[0], a[1], c[0], c[1])
        stk.append(s)
        m = np.zeros((7, 2), np.int32)
        m[:len(me)] = me
        mes.append(m)
        cnt.append(n)
        c = np.zeros((20, 9), np.int32)
        if n > 0:
            c[:n] = res
        cands.append(c)

    ONE = ([1], [0] * 7)                       # one single set
    THREE = (ALL, [0, 1, 0, 0, 2, 2, 2])       # LAST, LAST2, BWDREF: fwd 0, bwd 2, compound
    TWO = (ALL, [0, 0, 0, 0, 2, 2, 2])         # LAST, BWDREF: compound, at most 18 + ...
    for near in (0, 1):
        for n in (0, 1, 2, 3, 4, 9):
            me = (int(rng.integers(-60, 60)) | 1, int(rng.integers(-60, 60)))
            add(*ONE, 1, 6, near, [(int(rng.integers(0, 512)), rand_stack(rng, n))], [me])
            add(*ONE, 1, 6, near, [(int(rng.integers(0, 512)), rand_stack(rng, n))], [(0, 0)])
            for d in range(4):  # the NEWMV duplicate test at positions 0..3
                add(*ONE, 1, 6, near, [(7, rand_stack(rng, n, me, d))], [me])
            # row equal, col different: not a duplicate
            st = rand_stack(rng, n)
            if n:
                st[0] = ((me[0], me[1] + 1), st[0][1])
            add(*ONE, 1, 6, near, [(9, st)], [me])
        for rm, b in ((1, 6), (0, 6), (1, 3), (1, 1), (1, 2), (1, 0)):  # compound on / off, sz < 2 off
            for trial in range(6):
                for sets in (TWO, THREE):
                    fs = rs_ref_sets(*sets)[0]
                    lens = [int(rng.choice([0, 1, 2, 3, 4, 9])) for _ in range(len(fs) + 1)]
                    if trial == 0:
                        lens[-1] = 0  # the empty compound stack
                    if trial == 1:
                        lens = [9] * len(lens)  # the longest lists
                    me = [(int(rng.integers(-40, 40)), int(rng.integers(-40, 40))) for _ in fs]
                    stacks = [(int(rng.integers(0, 512)), rand_stack(rng, k)) for k in lens]
                    add(*sets, rm, b, near, stacks, me)
    out["ms_cfg"] = np.array(cfg, np.int32)
    out["ms_stacks"] = np.array(stk, np.int16)
    out["ms_me"] = np.array(mes, np.int16)
    out["ms_count"] = np.array(cnt, np.int32)
    out["ms_cands"] = np.array(cands, np.int16)
    print("mode set: %d cases, %d rejected" % (len(cnt), sum(1 for c in cnt if c < 0)))


def main():
    t0 = time.time()
    rng = np.random.default_rng(20250)
    out = {}
    I = setup()
    gen_params(I, out)
    gen_pixels(I, rng, out)
    gen_modes(rng, out)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes) in %.0f s" % (OUT, os.path.getsize(OUT), time.time() - t0))


if __name__ == "__main__":
    main()

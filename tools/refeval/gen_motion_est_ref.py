"""Golden vectors for motion estimation in rdo_mode_decision
(tests/golden/ref_motion_est.npz) -- needs the reference checkout that
gen_golden_ref.py reads:

    python tools/refeval/gen_motion_est_ref.py

Evaluated from the reference's own text (rsinterp.py):
  get_mv_range (src/me.rs:64-80);
  save_block_motion (src/encoder.rs:1432-1444), over a TileStateMut that holds
  mvs, mi_width and mi_height, with rectangles that cross the tile's edge;
  the pmv_idx expression of src/rdo.rs:1532-1536, wrapped in a function header;
  get_subset_predictors (src/me.rs:82-174) with MotionVector's Add / Div /
  quantize_to_fullpel / is_zero (src/mc.rs:33-58);
  diamond_me_search with get_best_predictor, get_mv_rd_cost,
  compute_mv_rd_cost, get_mv_rate (src/me.rs:655-856, 1006-1021) over
  predict_inter (src/predict.rs:255-338) and get_sad_ref / get_satd_ref /
  put_8tap_ref, as gen_golden_ref.py's `ds` section sets them up.

Restated below in Python, because the interpreter is not taken through
FrameInvariants / TileStateMut and the trait dispatch of MotionEstimation:
  DiamondSearch::motion_estimation's body (src/me.rs:198-273): get_mv_range of
  the frame block offset, the call of full_pixel_me, the call of sub_pixel_me;
  the SATD recost between them (:232-253) is left out: get_best_predictor
  resets the cost it would produce (:663-664);
  full_pixel_me (src/me.rs:392-432): get_subset_predictors with iter::once(cmv)
  over ts.mvs[ref.to_index()] and the frame of fi.ref_frames[0], then
  diamond_me_search with use_satd = false, subpixel = false;
  sub_pixel_me (src/me.rs:434-463): predictors = vec![*best_mv], then
  diamond_me_search with subpixel = true;
  the pmv pair of src/rdo.rs:859-865 (the cases carry the pair itself).

Only numbers are written:
  range:    w_in_b, h_in_b, bo x, y, blk_w, blk_h, then the four bounds
  pmv_idx:  bsize, tile bo x, y, pmv_idx
  sbm_*:    per case a tile (x, y, width, height; rows, cols of its field), its
            jobs (bo x, y, bsize, ref index, mv row, col) and the seven fields
            after them
  me_*:     one small frame (org, ref, geometry), per case bsize, the tile,
            bo, has_prev, use_satd, allow_hp, lambda, stack length, pmv pair,
            cmv; the tile field and the previous frame's field (frame-wide,
            of the case's reference); the full-pel winner, the MV and cost
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_epzs_ref as E  # noqa: E402
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "ref_motion_est.npz")
usz, mv = E.usz, E.mv


def isz(v):
    return RI.TInt(int(v), "isize")


class MvRows:
    """TileMotionVectorsMut / FrameMotionVectors over rows of MotionVector:
    [y][x] reads and writes, cols(), rows(), x(), y()."""

    def __init__(self, a, x=0, y=0):
        self.r = [[mv(r, c) for r, c in row] for row in a]
        self._x, self._y = x, y
        self.cols_, self.rows_ = usz(a.shape[1]), usz(a.shape[0])

    def index_row(self, i):
        return self.r[int(i)]

    def cols(self):
        return self.cols_

    def rows(self):
        return self.rows_

    def x(self):
        return usz(self._x)

    def y(self):
        return usz(self._y)

    def as_const(self):
        return self

    def array(self):
        return np.array([[(int(m.row), int(m.col)) for m in row] for row in self.r], np.int64)


class FrameRows(MvRows):
    """FrameMotionVectors: cols / rows are fields."""

    def __init__(self, a):
        super().__init__(a)
        self.cols, self.rows = self.cols_, self.rows_


def tbo(x, y):
    return RI.Struct("TileBlockOffset", {"0": RI.Struct("BlockOffset", {"x": usz(x), "y": usz(y)})})


def pbo(x, y):
    return RI.Struct("PlaneBlockOffset", {"0": RI.Struct("BlockOffset", {"x": usz(x), "y": usz(y)})})


def gen_range(I, rng, out):
    f = G.F(I, "get_mv_range", "me.rs")
    rows = []
    for _ in range(60):
        bw, bh = [(8, 8), (16, 8), (8, 16), (16, 16), (32, 16), (32, 32), (64, 32), (64, 64)][
            int(rng.integers(0, 8))]
        w_in_b, h_in_b = int(rng.integers(bw // 4, 80)), int(rng.integers(bh // 4, 60))
        x = int(rng.integers(0, w_in_b - bw // 4 + 1))
        y = int(rng.integers(0, h_in_b - bh // 4 + 1))
        if len(rows) % 4 == 0:
            x, y = w_in_b - bw // 4, 0  # the last column, the first row
        r = f(usz(w_in_b), usz(h_in_b), pbo(x, y), usz(bw), usz(bh))
        rows.append([w_in_b, h_in_b, x, y, bw, bh] + [int(v) for v in r])
    out["range"] = np.array(rows, np.int32)


def gen_pmv_idx(I, out):
    src = G.src_of(I, "rdo.rs").src
    a = src.index("let pmv_idx = if bsize > BlockSize::BLOCK_32X32")
    b = src.index("};", a) + 2
    text = "fn pmv_idx_of(bsize: BlockSize, tile_bo: TileBlockOffset) -> usize {\n%s\npmv_idx\n}" % src[a:b]
    f = I.make_fn(RI.parse_fn_text(text), I.globals)
    rows = []
    for b_ in range(16):
        for x in (0, 8, 31, 32, 33, 63, 64, 65, 96):
            for y in (0, 31, 32, 63, 64, 65):
                rows.append((b_, x, y, int(f(H.BlockSizeV(b_), tbo(x, y)))))
    out["pmv_idx"] = np.array(rows, np.int32)


def gen_sbm(I, rng, out):
    enc = RI.Source(G.REF + "encoder.rs")
    f = I.make_fn(enc.fn("save_block_motion"), I.globals)
    cases, jobs_all, outs, offs = [], [], [], [0]
    for case in range(12):
        cols, rows = int(rng.integers(2, 24)), int(rng.integers(2, 20))
        fields = [MvRows(np.zeros((rows, cols, 2), np.int64)) for _ in range(7)]
        ts = RI.Struct("TileStateMut", {"mvs": fields, "mi_width": usz(cols), "mi_height": usz(rows)})
        nj = int(rng.integers(3, 9))
        for k in range(nj):
            bs = int(rng.choice([0, 1, 3, 4, 5, 6, 8, 9, 12, 15, 18]))
            x, y = int(rng.integers(0, cols)), int(rng.integers(0, rows))
            if k == 0:  # crosses the tile's right / bottom edge
                bs, x, y = 9, max(0, cols - 3), max(0, rows - 2)
            ridx = int(rng.integers(0, 7)) if k % 3 else 0
            m = (int(rng.integers(-500, 500)), int(rng.integers(-500, 500)))
            f(ts, H.BlockSizeV(bs), tbo(x, y), usz(ridx), mv(*m), generics={"T": G.prim(8)})
            jobs_all.append((x, y, bs, ridx, m[0], m[1]))
        cases.append((0, 0, 4 * cols, 4 * rows, rows, cols, nj))
        o = np.stack([fl.array() for fl in fields]).reshape(-1)
        outs.append(o)
        offs.append(offs[-1] + len(o))
    out["sbm_case"] = np.array(cases, np.int32)
    out["sbm_jobs"] = np.array(jobs_all, np.int32)
    out["sbm_out"] = np.concatenate(outs).astype(np.int16)
    out["sbm_off"] = np.array(offs, np.int64)


def gen_me(I, rng, out):
    """motion_estimation's chain on one small 8-bit frame."""
    # the `ds` section's environment (gen_golden_ref.gen_ds)
    tile = RI.Source(G.REF + "tiling/tile.rs")
    I.define_impl("TileRect", tile.impl("TileRect"))
    env = I.globals.vars
    env["TileRect"] = RI.StructType("TileRect")
    env["RefType"] = G._RefType
    env["NONE_FRAME"] = G._RefType.NONE_FRAME
    env["PredictionMode"] = type("PM", (), {"NEWMV": G.PredModeV(16)})
    env["Plane"] = type("PlaneNS", (), {"new": staticmethod(
        lambda w, h, xd, yd, xp, yp: H.Plane.from_full(np.zeros((int(h), int(w)), np.int64),
                                                       0, 0, int(w), int(h)))})
    pred = RI.Source(G.REF + "predict.rs")
    G.PredModeV.fn = I.make_fn(pred.fn("predict_inter"), I.globals)
    ds = G.F(I, "diamond_me_search", "me.rs")
    rngf = G.F(I, "get_mv_range", "me.rs")
    gsp = env["get_subset_predictors"]
    sad_ref, satd_ref = G.F(I, "get_sad_ref"), G.F(I, "get_satd_ref")
    put_ref, prep_ref, avg_ref = G.F(I, "put_8tap_ref"), G.F(I, "prep_8tap_ref"), G.F(I, "mc_avg_ref")
    bd = 8
    g = {"T": G.prim(bd)}
    G.PredModeV.pixel = G.prim(bd)
    env["get_sad"] = lambda *a, _g=g: sad_ref(*a, generics=_g)
    env["get_satd"] = lambda *a, _g=g: satd_ref(*a, generics=_g)
    env["put_8tap"] = lambda *a, _g=g: put_ref(*a, generics=_g)
    env["prep_8tap"] = lambda *a, _g=g: prep_ref(*a, generics=_g)
    env["mc_avg"] = lambda *a, _g=g: avg_ref(*a, generics=_g)

    pad, H_, W_ = 88, 48, 64
    w_in_b, h_in_b = W_ // 4, H_ // 4
    # a smooth scene; the reference is the scene moved by (1.5, -1.25) pixels,
    # so the block's MV is about (-12, 10)
    S = 8
    hr = rng.random((H_ * S + 256, W_ * S + 256))
    for _ in range(2):
        for ax in (0, 1):
            c = np.cumsum(hr, axis=ax)
            k = 4 * S
            hr = np.take(c, np.arange(k, c.shape[ax]), axis=ax) - np.take(
                c, np.arange(0, c.shape[ax] - k), axis=ax)
    hr = (hr - hr.min()) / (hr.max() - hr.min()) * 255
    cut = lambda dy, dx: np.clip(np.rint(hr[64 + dy:64 + dy + H_ * S:S, 64 + dx:64 + dx + W_ * S:S]),  # noqa: E731
                                 0, 255).astype(np.int64)
    true = (12, -10)
    org, ref = cut(0, 0), np.clip(cut(*true) + rng.integers(-2, 3, (H_, W_)), 0, 255)
    fo, fr = np.pad(org, pad, mode="edge"), np.pad(ref, pad, mode="edge")
    po, pr = H.Plane.from_full(fo, pad, pad, W_, H_), H.Plane.from_full(fr, pad, pad, W_, H_)

    def field():
        a = np.zeros((h_in_b, w_in_b, 2), np.int64)
        for y in range(h_in_b):
            for x in range(w_in_b):
                u = rng.random()
                if u < 0.45:
                    continue
                a[y, x] = (-8 + 8 * int(rng.integers(-1, 2)), 8 + 8 * int(rng.integers(-1, 2))) \
                    if u < 0.8 else rng.integers(-120, 121, 2)
        return a

    # (bsize, tile, bo, has_prev, use_satd, allow_hp)
    specs = [(3, (0, 0, 64, 48), (4, 4), 1, 1, 0), (3, (32, 0, 32, 48), (0, 6), 1, 0, 1),
             (3, (0, 0, 64, 48), (14, 0), 0, 1, 1), (5, (0, 0, 64, 48), (8, 6), 1, 1, 0),
             (5, (32, 0, 32, 48), (4, 10), 1, 0, 0), (4, (0, 0, 64, 48), (2, 4), 1, 1, 1),
             (4, (0, 0, 32, 48), (6, 8), 0, 0, 0), (9, (0, 0, 64, 48), (8, 0), 1, 0, 0),
             (9, (0, 0, 64, 48), (0, 4), 1, 1, 0)]
    cases, tfs, pfs, fulls, mvs_, costs = [], [], [], [], [], []
    for n, (bs, tl, (bx, by), has_prev, satd, hp) in enumerate(specs):
        t0 = time.time()
        bsize = H.BlockSizeV(bs)
        tx4, ty4 = tl[0] // 4, tl[1] // 4
        tfield, pfield = field(), field()
        lam = int(rng.integers(50, 600))
        sn = n % 3
        pm = [(int(rng.integers(-30, 30)), int(rng.integers(-30, 30))) if k < sn else (0, 0)
              for k in range(2)]
        cm = (int(rng.integers(-40, 40)), int(rng.integers(-40, 40))) if n % 4 else (11, -13)
        fi = G.DsFi(bd, pr, hp)
        # --- motion_estimation (src/me.rs:198-273), restated -------------------
        fbo = (tx4 + bx, ty4 + by)  # ts.to_frame_block_offset(tile_bo)
        lo = rngf(usz(w_in_b), usz(h_in_b), pbo(*fbo), bsize.width(), bsize.height())
        # full_pixel_me (:392-432)
        tile_mvs = MvRows(tfield[ty4:ty4 + tl[3] // 4, tx4:tx4 + tl[2] // 4], tx4, ty4)
        fref = RI.Struct("ReferenceFrame", {"frame_mvs": [FrameRows(pfield)] * 7}) if has_prev else None
        preds = gsp(tbo(bx, by), [mv(*cm)], tile_mvs, fref, usz(0))
        best, cost = [H.motion_vector(0, 0)], [RI.TInt(2 ** 64 - 1, "u64")]
        bref = RI.Ref(lambda: best[0], lambda v: best.__setitem__(0, v))
        cref = RI.Ref(lambda: cost[0], lambda v: cost.__setitem__(0, v))
        plane_po = RI.Struct("PlaneOffset", {"x": isz(4 * fbo[0]), "y": isz(4 * fbo[1])})
        pmv = [H.motion_vector(*pm[0]), H.motion_vector(*pm[1])]
        ds(fi, plane_po, po, pr, list(preds), usz(bd), pmv, RI.TInt(lam, "u32"), lo[0], lo[1], lo[2],
           lo[3], bsize, False, bref, cref, False, G._RefType.LAST_FRAME, generics=g)
        full = (int(best[0].row), int(best[0].col))
        # sub_pixel_me (:434-463)
        # vec![*best_mv] is a copy: get_best_predictor resets *best_mv before it reads the list
        ds(fi, plane_po, po, pr, [H.motion_vector(*full)], usz(bd), pmv, RI.TInt(lam, "u32"), lo[0], lo[1], lo[2],
           lo[3], bsize, bool(satd), bref, cref, True, G._RefType.LAST_FRAME, generics=g)
        cases.append([bs, tl[0], tl[1], tl[2], tl[3], bx, by, has_prev, satd, hp, lam, sn,
                      pm[0][0], pm[0][1], pm[1][0], pm[1][1], cm[0], cm[1]])
        tfs.append(tfield)
        pfs.append(pfield)
        fulls.append(full)
        mvs_.append((int(best[0].row), int(best[0].col)))
        costs.append(int(cost[0]))
        print("  me case %d %s: %d predictors, full %s -> %s cost %d (%.0f s)" % (
            n, specs[n], len(preds), full, mvs_[-1], costs[-1], time.time() - t0), flush=True)
    out["me_org"] = fo.astype(np.uint8)
    out["me_ref"] = fr.astype(np.uint8)
    out["me_geom"] = np.array([pad, pad, W_, H_], np.int32)
    out["me_cases"] = np.array(cases, np.int32)
    out["me_tile_field"] = np.array(tfs, np.int16)
    out["me_prev_field"] = np.array(pfs, np.int16)
    out["me_full"] = np.array(fulls, np.int16)
    out["me_mv"] = np.array(mvs_, np.int16)
    out["me_cost"] = np.array(costs, np.uint64)


def main():
    rng = np.random.default_rng(0x3E57)
    I = E.make()  # MotionVector's impls and get_subset_predictors
    I.globals.vars["TileBlockOffset"] = RI.StructType("TileBlockOffset")
    out = {}
    t0 = time.time()
    gen_range(I, rng, out)
    gen_pmv_idx(I, out)
    gen_sbm(I, rng, out)
    gen_me(I, rng, out)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes) in %.0f s" % (OUT, os.path.getsize(OUT), time.time() - t0))


if __name__ == "__main__":
    main()

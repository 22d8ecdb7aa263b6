"""Reference for rv_motion_estimation_batch / rv_save_block_motion_batch:
DiamondSearch::motion_estimation (src/me.rs:193-278, 391-463) composed from
the oracle pieces that are already pinned to the reference's text --
orc_subset_predictors (tests/golden/ref_epzs.npz) and orc_diamond_search
(ref_me.npz / ref_ds.npz) -- with plain restatements of the glue between them:
get_mv_range (me.rs:64-80), the pmv pair (src/rdo.rs:859-865),
save_block_motion (src/encoder.rs:1432-1444) and pmv_idx (rdo.rs:1532-1536).
tests/golden/ref_motion_est.npz (tools/refeval/gen_motion_est_ref.py) pins the
glue and the chain to the reference's own text."""
import ctypes as C

import numpy as np

from tests import oracle_lib as O

# BlockSize -> pixels (src/partition.rs:116-139 order)
BLK_W = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64]
BLK_H = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16]
# the predictor sources in get_subset_predictors' push order
SOURCES = ("zero", "coarse", "left", "top", "top_right", "mean", "c_left", "c_top", "c_right",
           "c_bottom", "c_colocated")


def mv_range(w_in_b, h_in_b, fx4, fy4, blk_w, blk_h):
    """get_mv_range (src/me.rs:64-80): (mvx_min, mvx_max, mvy_min, mvy_max)."""
    border_w, border_h = 128 + blk_w * 8, 128 + blk_h * 8
    assert w_in_b - fx4 - blk_w // 4 >= 0 and h_in_b - fy4 - blk_h // 4 >= 0  # usize
    return (-fx4 * 32 - border_w, (w_in_b - fx4 - blk_w // 4) * 32 + border_w,
            -fy4 * 32 - border_h, (h_in_b - fy4 - blk_h // 4) * 32 + border_h)


def pmv_pair(n, this_mvs):
    """src/rdo.rs:859-865: entries 0 and 1 of the stack's this_mv, else zero."""
    p0 = tuple(int(v) for v in this_mvs[0]) if n > 0 else (0, 0)
    p1 = tuple(int(v) for v in this_mvs[1]) if n > 1 else (0, 0)
    return p0, p1


def pmv_index(bsize, bo_x, bo_y):
    """src/rdo.rs:1532-1536 (`bsize > BLOCK_32X32` in enum order)."""
    return 0 if bsize > 9 else ((bo_x & 32) >> 5) + ((bo_y & 32) >> 4) + 1


def save_block_motion(field, tiles, jobs):
    """src/encoder.rs:1432-1444 for a coding-order list, in place.  field:
    (7, h_in_b, w_in_b, 2); tiles: (x, y, width, height) pixels; jobs: (tile,
    bo_x, bo_y, bsize, ref_index, (row, col)); ref_index < 0 is skipped."""
    for tile, bx, by, bsize, ridx, mv in jobs:
        if ridx < 0:
            continue
        tx, ty, tw, th = (int(v) for v in tiles[tile])
        x_end = min(bx + BLK_W[bsize] // 4, tw >> 2)  # ts.mi_width
        y_end = min(by + BLK_H[bsize] // 4, th >> 2)
        field[ridx, (ty >> 2) + by:(ty >> 2) + y_end, (tx >> 2) + bx:(tx >> 2) + x_end] = mv
    return field


def _qfull(v):
    q = lambda a: int(a / 8) * 8 if a >= 0 else -int(-a / 8) * 8  # noqa: E731  (truncating)
    return (q(int(v[0])), q(int(v[1])))


def _i16(v):
    return ((int(v) + 0x8000) & 0xFFFF) - 0x8000


def predictor_sources(tile_field, prev_field, tile, bx, by, cmv, w_in_b, h_in_b):
    """The (source, mv) list get_subset_predictors (src/me.rs:82-174) pushes, in
    order, and the has_left / has_top / has_top_right flags: which input each
    list position came from.  The values are checked against
    orc_subset_predictors by subset_predictors()."""
    tx4, ty4, cols = tile[0] >> 2, tile[1] >> 2, tile[2] >> 2
    out = [("zero", (0, 0)), ("coarse", _qfull(cmv))]
    med = []
    hl, ht = bx > 0, by > 0
    htr = ht and bx < cols - 1
    cell = lambda f, x, y: tuple(int(v) for v in f[y, x])  # noqa: E731
    for name, has, dx, dy in (("left", hl, -1, 0), ("top", ht, 0, -1), ("top_right", htr, 1, -1)):
        if has:
            v = cell(tile_field, tx4 + bx + dx, ty4 + by + dy)
            med.append(v)
            if v != (0, 0):
                out.append((name, v))
    if med:
        sr = sc = 0
        for v in med:
            sr, sc = _i16(sr + v[0]), _i16(sc + v[1])
        n = len(med)
        tdiv = lambda a: int(a / n) if a >= 0 else -int(-a / n)  # noqa: E731
        q = _qfull((tdiv(sr), tdiv(sc)))
        if q != (0, 0):
            out.append(("mean", q))
    if prev_field is not None:
        fx, fy = tx4 + bx, ty4 + by
        for name, has, dx, dy in (("c_left", fx > 0, -1, 0), ("c_top", fy > 0, 0, -1),
                                  ("c_right", fx < w_in_b - 1, 1, 0),
                                  ("c_bottom", fy < h_in_b - 1, 0, 1), ("c_colocated", True, 0, 0)):
            if has:
                v = cell(prev_field, fx + dx, fy + dy)
                if v != (0, 0):
                    out.append((name, v))
    return out, (hl, ht, htr)


def subset_predictors(tile_field, prev_field, tile, bx, by, cmv, w_in_b, h_in_b):
    """orc_subset_predictors on the frame-wide fields read through the tile's
    rectangle: tile_field / prev_field (h_in_b, w_in_b, 2) int16 of one
    reference (prev_field None: no subset C).  Returns [(row, col)]."""
    f = O.lib().orc_subset_predictors
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                  C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    tx4, ty4, cols = tile[0] >> 2, tile[1] >> 2, tile[2] >> 2
    tf = np.ascontiguousarray(tile_field, np.int16)
    tptr = tf.ctypes.data + 4 * (ty4 * w_in_b + tx4)  # the tile's cell (0, 0), pitch w_in_b
    pf = np.ascontiguousarray(prev_field, np.int16) if prev_field is not None else None
    cm = np.array([cmv], np.int16)
    out = np.zeros((17, 2), np.int16)
    n = f(bx, by, cm.ctypes.data, 1, tptr, w_in_b, cols, pf.ctypes.data if pf is not None else None,
          w_in_b, w_in_b, h_in_b, tx4 + bx, ty4 + by, out.ctypes.data)
    preds = [tuple(int(v) for v in out[k]) for k in range(n)]
    tagged, _ = predictor_sources(tile_field, prev_field, tile, bx, by, cmv, w_in_b, h_in_b)
    assert [m for _, m in tagged] == preds, (tagged, preds)
    return preds


def _rate(mv, pmv, hp):
    """get_mv_rate (src/me.rs:1006-1021)."""
    r = 0
    for a, b in zip(mv, pmv):
        d = _i16(a - b)
        d = d if hp else d >> 1
        r += 0 if d == 0 else 2 * abs(d).bit_length()
    return r


def fullpel_cost(org_full, ref_full, xo, yo, px, py, w, h, mv, rng_, pmv, lam, hp):
    """get_mv_rd_cost (src/me.rs:787-856) of a full-pel candidate with SAD."""
    if mv[1] < rng_[0] or mv[1] > rng_[1] or mv[0] < rng_[2] or mv[0] > rng_[3]:
        return 2 ** 64 - 1
    tq = lambda a: int(a / 8) if a >= 0 else -int(-a / 8)  # noqa: E731
    o = org_full[yo + py:yo + py + h, xo + px:xo + px + w].astype(np.int64)
    ry, rx = yo + py + tq(mv[0]), xo + px + tq(mv[1])
    r = ref_full[ry:ry + h, rx:rx + w].astype(np.int64)
    sad = int(np.abs(o - r).sum())
    rate = min(_rate(mv, pmv[0], hp), _rate(mv, pmv[1], hp) + 1)
    return 256 * sad + rate * lam


def motion_estimation(org_full, ref_full, geom, w_in_b, h_in_b, tile, bx, by, bsize, stack_n,
                      stack_mvs, cmv, tile_field, prev_field, lam, use_satd, allow_hp, bd,
                      info=None):
    """DiamondSearch::motion_estimation (src/me.rs:193-278) of one block against
    one reference.  org_full / ref_full: padded arrays of one geometry, geom =
    (xorigin, yorigin, width, height); tile (x, y, width, height) pixels;
    (bx, by) the tile block offset.  The recost of me.rs:232-253 is dead for
    DiamondSearch (get_best_predictor resets the cost, :663-664) and is not
    formed.  Returns ((row, col), cost); info (a dict) receives the full-pel
    winner, the chosen start's source and the has_* flags."""
    xo, yo, width, height = geom
    w, h = BLK_W[bsize], BLK_H[bsize]
    fx4, fy4 = (tile[0] >> 2) + bx, (tile[1] >> 2) + by
    rng_ = mv_range(w_in_b, h_in_b, fx4, fy4, w, h)
    pmv = pmv_pair(stack_n, stack_mvs)
    preds = subset_predictors(tile_field, prev_field, tile, bx, by, cmv, w_in_b, h_in_b)
    job = {"po_x": 4 * fx4, "po_y": 4 * fy4, "mvx_min": rng_[0], "mvx_max": rng_[1],
           "mvy_min": rng_[2], "mvy_max": rng_[3], "pmv0_row": pmv[0][0], "pmv0_col": pmv[0][1],
           "pmv1_row": pmv[1][0], "pmv1_col": pmv[1][1], "lambda_": lam, "n_pred": len(preds),
           "pred": preds}
    full, _ = O.diamond_search(org_full, ref_full, xo, yo, width, height, job, w, h, False, False,
                               allow_hp, bd)
    job["n_pred"], job["pred"] = 1, [full]
    best, cost = O.diamond_search(org_full, ref_full, xo, yo, width, height, job, w, h, True,
                                  use_satd, allow_hp, bd)
    if info is not None:
        tagged, flags = predictor_sources(tile_field, prev_field, tile, bx, by, cmv, w_in_b, h_in_b)
        costs = [fullpel_cost(org_full, ref_full, xo, yo, 4 * fx4, 4 * fy4, w, h, m, rng_, pmv, lam,
                              allow_hp) for _, m in tagged]
        info["full"], info["flags"] = full, flags
        info["start"] = tagged[costs.index(min(costs))][0]  # strict <: the first minimum
    return best, cost

"""Chroma from luma, restated in plain numpy from the reference's text
(geobacter-rs/rav1e) for the tests of rav1e_amd's CfL operators:

  luma_ac                src/encoder.rs:1714-1755
  get_scaled_luma_q0     src/predict.rs:485-493
  predict_intra(CFL)     src/predict.rs:202-241 (alpha == 0 -> DC_PRED),
                         pred_cfl / _128 / _left / _top / _inner :836-892
  get_intra_edges(CFL)   src/partition.rs:542-595 (what a DC reads)
  rdo_cfl_alpha          src/rdo.rs:1261-1336

The DC part goes through the C oracle (tests.oracle_lib.predict_intra with
DC_PRED), so nothing here shares code with the HIP kernels.  Planes are the
whole padded allocation as a 2-D array plus the (yorigin, xorigin) of pixel
(0, 0); positions are in visible coordinates.
"""
import numpy as np

from tests import oracle_lib as O

EDGE_PX = 4 * 64 + 1
# BlockSize order (src/partition.rs:116-140) up to BLOCK_32X32, the sizes
# cfl_allowed() admits (:174-177)
BLOCK_WH = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32)]
SUBSAMPLINGS = [(0, 0), (1, 0), (1, 1)]


def subsampled_size(bsize, xdec, ydec):
    """BlockSize::subsampled_size (src/partition.rs:245-286) for the sizes of
    BLOCK_WH: (w, h) of the chroma-plane block, None for BLOCK_INVALID."""
    w, h = BLOCK_WH[bsize]
    if (xdec, ydec) == (0, 0):
        return w, h
    if (xdec, ydec) == (1, 0):
        # 4:2:2 lists 4X4, 8X4, 8X8, 16X8, 16X16, 32X16, 32X32 of these
        if (w, h) in ((4, 8), (8, 16), (16, 32)):
            return None
        return max(4, w // 2), h
    assert (xdec, ydec) == (1, 1)
    return max(4, w // 2), max(4, h // 2)


def allowed_cells():
    """Every (bsize, xdec, ydec) the operators accept."""
    return [(b, xd, yd) for xd, yd in SUBSAMPLINGS for b in range(len(BLOCK_WH))
            if subsampled_size(b, xd, yd) is not None]


def has_chroma(x, y, bsize, xdec, ydec):
    """has_chroma (src/context.rs:551-560); (x, y) luma pixels = 4 * bo."""
    w, h = BLOCK_WH[bsize]
    bx, by = x >> 2, y >> 2
    return (((bx & 1) == 1 or ((w >> 2) & 1) == 0 or xdec == 0) and
            ((by & 1) == 1 or ((h >> 2) & 1) == 0 or ydec == 0))


def luma_origin(x, y, bsize, xdec, ydec):
    """The luma pixel luma_ac starts from: is_sub8x8 / sub8x8_offset
    (src/partition.rs:303-312) move the block offset by -1."""
    w, h = BLOCK_WH[bsize]
    return (x - 4 if xdec != 0 and w == 4 else x), (y - 4 if ydec != 0 and h == 4 else y)


def chroma_pos(x, y, xdec, ydec):
    """plane_offset / Area::BlockStartingAt: (bo >> dec) << 2 per axis."""
    return ((x >> 2) >> xdec) << 2, ((y >> 2) >> ydec) << 2


def luma_ac(luma_full, yo, xo, x, y, bsize, xdec, ydec):
    """src/encoder.rs:1714-1755: (h, w) int16."""
    w, h = subsampled_size(bsize, xdec, ydec)
    lx, ly = luma_origin(x, y, bsize, xdec, ydec)
    blk = luma_full[yo + ly: yo + ly + (h << ydec), xo + lx: xo + lx + (w << xdec)].astype(np.int64)
    assert blk.shape == (h << ydec, w << xdec)
    sample = blk[::1 << ydec, ::1 << xdec].copy()
    if xdec != 0:
        sample += blk[::1 << ydec, 1::2]
    if ydec != 0:
        sample += blk[1::2, ::2] + blk[1::2, 1::2]
    sample <<= 3 - xdec - ydec
    assert sample.max() <= 32767  # the reference's i16 does not wrap
    shift = (w.bit_length() - 1) + (h.bit_length() - 1)
    average = (int(sample.sum()) + (1 << (shift - 1))) >> shift
    return (sample - average).astype(np.int16)


def scaled_luma_q0(alpha, ac):
    """get_scaled_luma_q0 (src/predict.rs:485-493), elementwise."""
    q6 = np.asarray(alpha, np.int64) * np.asarray(ac, np.int64)
    a0 = (np.abs(q6) + 32) >> 6
    return np.where(q6 < 0, -a0, a0)


def predict_cfl(variant, w, h, edge, ac, alpha, bd):
    """predict_intra(UV_CFL_PRED): the DC_PRED fill of the variant, then
    pred_cfl_inner with avg = output[0][0] (src/predict.rs:836-860)."""
    dc = O.predict_intra(0, variant, w, h, edge, bd)
    if alpha == 0:
        return dc
    avg = int(dc[0, 0])
    v = avg + scaled_luma_q0(alpha, np.asarray(ac).reshape(h, w))
    return np.clip(v, 0, (1 << bd) - 1).astype(dc.dtype)


def cfl_edges(rec_full, yo, xo, cx, cy, w, h, variant):
    """get_intra_edges(.., Some(UV_CFL_PRED)) (src/partition.rs:542-595) for
    the block at plane pixel (cx, cy): the left column where the variant has
    a left (x != 0), the above row where it has a top (y != 0); the rest of
    edge_buf is never read by a DC and stays 0."""
    e = np.zeros(EDGE_PX, rec_full.dtype)
    if variant & 1:
        for i in range(h):
            e[128 - h + i] = rec_full[yo + cy + h - 1 - i, xo + cx - 1]
    if variant & 2:
        e[129:129 + w] = rec_full[yo + cy - 1, xo + cx: xo + cx + w]
    return e


def alpha_costs(src_blk, dc_blk, ac, bd):
    """sse_wxh with bias 1 (src/rdo.rs:286-335: the plain sum of squared
    differences) of the source against the prediction for the alphas
    -16 .. 16: costs[alpha + 16]."""
    alphas = np.arange(-16, 17).reshape(33, 1, 1)
    avg = int(dc_blk[0, 0])
    pred = np.clip(avg + scaled_luma_q0(alphas, ac[None]), 0, (1 << bd) - 1)
    pred[16] = dc_blk  # alpha == 0 -> DC_PRED
    d = src_blk.astype(np.int64)[None] - pred
    return [int(v) for v in (d * d).sum(axis=(1, 2))]


def alpha_scan(costs):
    """The scan of rdo_cfl_alpha (src/rdo.rs:1311-1327) over costs[alpha +
    16]: (alpha, cost, the step `a` it stopped after)."""
    best = (costs[16], 0)
    count = 2
    a = 0
    for a in range(1, 17):
        c0, c1 = costs[16 + a], costs[16 - a]
        if c0 < best[0]:
            best = (c0, a)
            count += 2
        if c1 < best[0]:
            best = (c1, -a)
            count += 2
        if count < a:
            break
    return best[1], best[0], a


def rdo_cfl_alpha(rec, src, x, y, variant, bsize, bd):
    """rdo_cfl_alpha for the partition at luma pixel (x, y).  rec / src: three
    (full array, yorigin, xorigin, xdec, ydec) each.  Returns per chroma
    plane (alpha, cost, stop step, costs)."""
    xdec, ydec = rec[1][3], rec[1][4]
    w, h = subsampled_size(bsize, xdec, ydec)
    ac = luma_ac(rec[0][0], rec[0][1], rec[0][2], x, y, bsize, xdec, ydec)
    cx, cy = chroma_pos(x, y, xdec, ydec)
    out = []
    for p in (1, 2):
        rf, ryo, rxo = rec[p][:3]
        sf, syo, sxo = src[p][:3]
        edge = cfl_edges(rf, ryo, rxo, cx, cy, w, h, variant)
        dc = O.predict_intra(0, variant, w, h, edge, bd)
        s = sf[syo + cy: syo + cy + h, sxo + cx: sxo + cx + w]
        costs = alpha_costs(s, dc, ac, bd)
        out.append(alpha_scan(costs) + (costs,))
    return out

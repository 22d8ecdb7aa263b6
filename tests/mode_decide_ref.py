"""Plain Python / numpy restatement of the end of rdo_mode_decision (src/
rdo.rs), the checker of rav1e_amd.mode_decide_batch / block_segments_batch:

  compute_mean_importance (:477-493), compute_distortion_bias (:495-508),
  the three Mul impls (:525-543), cdef_dist_wxh_8x8 / cdef_dist_wxh
  (:219-283), sse_wxh (:286-335), compute_distortion (:338-411),
  compute_tx_distortion (:414-475) with encode_tx_block's per-block product
  (src/encoder.rs:1234-1236), compute_rd_cost (:563-568), the heuristic
  segment index (:655-679), get_qidx (src/encoder.rs:1061-1072),
  segmentation_optimize's deltas (src/segmentation.rs:29-48), and the control
  flow of luma_chroma_mode_rdo / rdo_mode_decision over a candidate list.

tests/test_mode_decide.py pins every function here to the vectors the
reference's own text produced (tests/golden/ref_mode_decide.npz).

Planes are (full, xorigin, yorigin): the whole padded allocation as a 2-D
array and the position of pixel (0, 0) in it.  f32 steps go through
numpy.float32, f64 steps through Python floats (IEEE double), integers through
Python ints."""
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
RD_MAX = float(np.finfo(np.float64).max)
SKIP, INTRA, NEED_RECON = 1, 2, 4
NONE, EVALUATED, GATED_ZERO_DIST, GATED_SKIP, REJECTED = range(5)
BLK_W = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64]
BLK_H = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64]
TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
U64 = (1 << 64) - 1


def segmentation_data(base_q_idx):
    return [0, 21, max(-21, 1 - base_q_idx)]


def as_u64(v):
    """Rust's `f64 as u64`: truncating, saturating, NaN -> 0."""
    if not v > 0.0:
        return 0
    return U64 if v >= 18446744073709551616.0 else int(v)


def mul(value, f):
    """RawDistortion * f64 and Distortion * f64: (self.0 as f64 * rhs) as u64."""
    return as_u64(float(value) * f)


class Frame:
    """What the functions read of FrameInvariants."""

    def __init__(self, w_in_b, h_in_b, importance=None, lambda_=1.0, dist_scale=(1.0, 1.0, 1.0),
                 bit_depth=8, psy=False, use_tx=False, coeff_rate=True):
        self.w_in_b, self.h_in_b = w_in_b, h_in_b
        self.imp = None if importance is None else np.asarray(importance, F32)
        self.lambda_, self.dist_scale = float(lambda_), [float(v) for v in dist_scale]
        self.bit_depth, self.psy, self.use_tx, self.coeff_rate = bit_depth, psy, use_tx, coeff_rate


def mean_importance(fr, mi_x, mi_y, mw, mh):
    x2, y2 = min(mi_x + mw, fr.w_in_b), min(mi_y + mh, fr.h_in_b)
    tot = F32(0)
    if fr.imp is not None:
        for y in range(mi_y, y2):
            for x in range(mi_x, x2):
                tot = F32(tot + fr.imp[y // 2, x // 2])
    return F32(tot / F32(mw * mh))


def distortion_bias(fr, mi_x, mi_y, mw, mh):
    return float(F32(mean_importance(fr, mi_x, mi_y, mw, mh) / F32(3))) + 0.65


def block_segment(fr, mi_x, mi_y, bsize, base_q_idx, data=None):
    """(sidx, qindex, mean importance) of a block at frame 4x4 offset (mi_x, mi_y)."""
    data = segmentation_data(base_q_idx) if data is None else data
    m = mean_importance(fr, mi_x, mi_y, BLK_W[bsize] // 4, BLK_H[bsize] // 4)
    sidx = 2 if m >= 4 else 0 if m >= 2 else 1
    if base_q_idx + data[sidx] < 2:
        sidx = 0
    return sidx, min(255, max(0, base_q_idx + data[sidx])), m


def region(plane, x, y, w, h):
    full, xo, yo = plane
    return full[yo + y:yo + y + h, xo + x:xo + x + w].astype(np.int64)


def cdef_dist_8x8(s, d, bit_depth):
    cs = bit_depth - 8
    ss, sd = int(s.sum()), int(d.sum())
    s2, d2, sdp = int((s * s).sum()), int((d * d).sum()), int((s * d).sum())
    svar = float(s2 - ((ss * ss + 32) >> 6))
    dvar = float(d2 - ((sd * sd + 32) >> 6))
    sse = float(d2 + s2 - 2 * sdp)
    boost = (4033.0 / 16384.0) * (svar + dvar + float(16384 << (2 * cs))) / \
        math.sqrt(float(16265089 << (4 * cs)) + svar * dvar)
    return as_u64(sse * boost + 0.5)


def plane_distortion(fr, src, rec, x, y, w, h, xdec, ydec, cdef, area=None):
    """cdef_dist_wxh or sse_wxh of the w x h region at plane pixel (x, y) of a
    plane decimated by (xdec, ydec): the Distortion, and the (bias, value) of
    every importance sub-block.  The bias is compute_distortion_bias of
    imp_bsize at the sub-block's frame_block_offset (rect >> (2 - dec))."""
    iw, ih = min(8, w), min(8, h)
    bw, bh = iw >> xdec, ih >> ydec
    if cdef:
        assert xdec == 0 and ydec == 0 and w % 8 == 0 and h % 8 == 0
    total, parts = 0, []
    for by in range(h // bh):
        for bx in range(w // bw):
            px, py = x + bx * bw, y + by * bh
            s, d = region(src, px, py, bw, bh), region(rec, px, py, bw, bh)
            v = cdef_dist_8x8(s, d, fr.bit_depth) if cdef else int(((s - d) ** 2).sum())
            mw, mh = (iw // 4, ih // 4) if area is None else area
            bias = distortion_bias(fr, px >> (2 - xdec), py >> (2 - ydec), mw, mh)
            parts.append((bias, v))
            total = (total + mul(v, bias)) & U64
    return total, parts


def block_origin(tile, bo_x, bo_y, xdec, ydec):
    return (tile[0] >> xdec) + ((bo_x >> xdec) << 2), (tile[1] >> ydec) + ((bo_y >> ydec) << 2)


def pixel_distortion(fr, src, rec, tile, bo_x, bo_y, bsize, xdec, ydec, luma_sse=False,
                     scale_sum=False, chroma_area=None):
    """compute_distortion (or compute_tx_distortion's skip arm with luma_sse).
    scale_sum / chroma_area: the mutations the tests try, off by default."""
    bw, bh = BLK_W[bsize], BLK_H[bsize]
    x, y = block_origin(tile, bo_x, bo_y, 0, 0)
    d, _ = plane_distortion(fr, src[0], rec[0], x, y, bw, bh, 0, 0, fr.psy and not luma_sse)
    planes = [d]
    w_uv, h_uv = (bw >> xdec) & ~3, (bh >> ydec) & ~3
    for p in (1, 2):
        x, y = block_origin(tile, bo_x, bo_y, xdec, ydec)
        d, _ = plane_distortion(fr, src[p], rec[p], x, y, w_uv, h_uv, xdec, ydec, False, chroma_area)
        planes.append(d)
    if scale_sum:
        return mul(sum(planes) & U64, fr.dist_scale[0])
    return sum(mul(d, fr.dist_scale[p]) for p, d in enumerate(planes)) & U64


def tx_layout(bsize, tx_size, xdec, ydec):
    """Per plane (tx_w, tx_h, cols, rows) of write_tx_blocks / write_tx_tree
    (src/encoder.rs:1764-1765, 1821-1832); tests/tx_blocks_ref.py is pinned to
    the reference's call sequences, and the tests compare this with it."""
    bw, bh = BLK_W[bsize], BLK_H[bsize]
    out = [(TX_W[tx_size], TX_H[tx_size], bw // TX_W[tx_size], bh // TX_H[tx_size])]
    pw, ph = bw >> xdec, bh >> ydec
    uw, uh = min(pw, 32), min(ph, 32)
    out += [(uw, uh, pw // uw, ph // uh)] * 2
    return out


def tx_distortion(fr, tile, bo_x, bo_y, bsize, tx_size, xdec, ydec, dists, bias_by_tx_size=False):
    """The non-skip arm of compute_tx_distortion: the sum over the candidate's
    transform blocks of RawDistortion(d) * bias * dist_scale[p], the bias of
    the partition's bsize at tx_bo.  dists: the job's row of tx_blocks_batch."""
    out, o = 0, 0
    for p, (tw, th, cols, rows) in enumerate(tx_layout(bsize, tx_size, xdec, ydec)):
        xd, yd = (xdec, ydec) if p else (0, 0)
        for i in range(cols * rows):
            bx, by = i % cols, i // cols
            mi_x = (tile[0] >> 2) + bo_x + ((bx * (tw // 4)) << xd)
            mi_y = (tile[1] >> 2) + bo_y + ((by * (th // 4)) << yd)
            mw, mh = (max(1, (tw << xd) // 4), max(1, (th << yd) // 4)) if bias_by_tx_size else \
                (BLK_W[bsize] // 4, BLK_H[bsize] // 4)
            bias = distortion_bias(fr, mi_x, mi_y, mw, mh)
            out = (out + mul(mul(int(dists[o]), bias), fr.dist_scale[p])) & U64
            o += 1
    return out


def n_tx_blocks(bsize, tx_size, xdec, ydec):
    return sum(c * r for _, _, c, r in tx_layout(bsize, tx_size, xdec, ydec))


def rd_cost(fr, rate, distortion):
    return float(distortion) + fr.lambda_ * (float(rate) / 8.0)


def has_coeff(fr, flags, eobs):
    if flags & SKIP:
        return False
    if (flags & NEED_RECON) or fr.coeff_rate:
        return any(int(e) != 0 for e in eobs)
    return True


Best = namedtuple("Best", "cand rd_cost distortion rate skip has_coeff")


def walk(cands, seed=None, replace_on_equal=False, zero_from_any_skip=False):
    """rdo_mode_decision + luma_chroma_mode_rdo's control flow over a list of
    (group, flags, rate, distortion, cost, has_coeff, rejected) in the
    reference's order.  Returns (Best, states).  seed: (rd_cost, skip) to
    continue from.  The two keyword mutations are off by default."""
    best_rd, best_skip = (RD_MAX, False) if seed is None else (float(seed[0]), bool(seed[1]))
    best = None
    states = []
    group, first, zero, gate = 0, True, False, False
    for k, (grp, flags, rate, dist, cost, hc, rejected) in enumerate(cands):
        if rejected:
            states.append(REJECTED)
            continue
        intra, skip = bool(flags & INTRA), bool(flags & SKIP)
        if first or grp != group:
            first, group, zero = False, grp, False
            gate = intra and best_skip
        if gate if intra else (not skip and zero):
            states.append(GATED_SKIP if intra else GATED_ZERO_DIST)
            continue
        states.append(EVALUATED)
        if not intra and skip and zero_from_any_skip:
            zero = zero or dist == 0
        if cost < best_rd or (replace_on_equal and cost == best_rd):
            best_rd, best_skip = cost, skip
            best = Best(k, cost, dist, rate, skip, hc)
            if not intra and skip and not zero_from_any_skip:
                zero = dist == 0
    return best, states


def decide_block(fr, src, sets, tile, block, cands, bsize, xdec, ydec, tx_dist=None, tx_eob=None,
                 seed=None, n_sets=None, **mut):
    """One block of mode_decide_batch.  block: (bo_x, bo_y); cands: MODE_CAND
    records (or dicts with the same keys) in order; sets: the candidate plane
    sets.  Returns (Best or None, dists, costs, states)."""
    n_sets = len(sets) if n_sets is None else n_sets
    n_tx = 0 if tx_dist is None else len(tx_dist)
    rows = []
    for c in cands:
        flags, ts, st = int(c["flags"]), int(c["tx_size"]), int(c["set"])
        ok = 0 <= st < n_sets and 0 <= ts < 19 and TX_W[ts] <= BLK_W[bsize] and TX_H[ts] <= BLK_H[bsize]
        nb = n_tx_blocks(bsize, ts, xdec, ydec) if ok else 0
        do, eo = int(c["dist_off"]), int(c["eob_off"])
        if ok and not flags & SKIP:
            ok = do >= 0 and eo >= 0 and do + nb <= n_tx and eo + nb <= n_tx
        if not ok:
            rows.append((int(c["group"]), flags, int(c["rate"]), 0, RD_MAX, False, True))
            continue
        skip = bool(flags & SKIP)
        if not fr.use_tx or flags & NEED_RECON or skip:
            d = pixel_distortion(fr, src, sets[st], tile, block[0], block[1], bsize, xdec, ydec,
                                 luma_sse=fr.use_tx and not flags & NEED_RECON,
                                 **{k: v for k, v in mut.items() if k in ("scale_sum", "chroma_area")})
        else:
            d = tx_distortion(fr, tile, block[0], block[1], bsize, ts, xdec, ydec, tx_dist[do:do + nb],
                              bias_by_tx_size=mut.get("bias_by_tx_size", False))
        hc = has_coeff(fr, flags, [] if skip else tx_eob[eo:eo + nb])
        rows.append((int(c["group"]), flags, int(c["rate"]), d, rd_cost(fr, int(c["rate"]), d), hc, False))
    best, states = walk(rows, seed, **{k: v for k, v in mut.items()
                                       if k in ("replace_on_equal", "zero_from_any_skip")})
    return best, [r[3] for r in rows], [r[4] for r in rows], states


def synth_planes(seed, bit_depth, xdec, ydec, width, height, pad, noise_of=None):
    """The pixel inputs of the golden vectors, by formula (so the vectors hold
    results only): three padded planes (full, pad, pad) of a width x height
    frame; with noise_of, those planes plus a bounded pseudo-random error."""
    out = []
    for p in range(3):
        xd, yd = (xdec, ydec) if p else (0, 0)
        h, w = (height >> yd) + 2 * pad, (width >> xd) + 2 * pad
        y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
        v = (x * np.uint64(73) + y * np.uint64(151) + np.uint64(31 * p + 7 * seed + 1)) * \
            np.uint64(2654435761)
        v = (v ^ (v >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
        v = v ^ (v >> np.uint64(13))
        if noise_of is None:
            a = (v >> np.uint64(3)) & np.uint64((1 << bit_depth) - 1)
        else:
            e = (v % np.uint64(25)).astype(np.int64) - 12
            e[(y // np.uint64(8) + x // np.uint64(8) + np.uint64(seed + p)) % np.uint64(5) == 0] = 0  # exact 8x8 areas
            a = np.clip(noise_of[p][0].astype(np.int64) + e * (1 << (bit_depth - 8)), 0,
                        (1 << bit_depth) - 1)
        out.append((a.astype(np.uint16), pad, pad))
    return out

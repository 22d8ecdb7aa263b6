"""numpy restatement of the general get_intra_edges (src/partition.rs:
500-693) with has_top_right / has_bottom_left (src/recon_intra.rs:174-243,
376-458) and of the intra-mode screening (src/rdo.rs:1029-1127), over the
oracle's predict_intra and get_satd.  The checker of the GPU tests;
tests/test_intra_screen.py holds it to the vectors the reference's own text
produced (tests/golden/ref_intra_screen.npz).

The coded-before test of the availability's general case is derived here
from the coding order itself: the blocks of a 64x64 superblock are numbered
in the order a uniform partition into that size codes them, and a neighbour
is available when its number is lower."""
import functools

import numpy as np

from tests import oracle_lib as O

RAV1E_INTRA_MODES = [0, 2, 1, 9, 11, 10, 12, 3, 4, 5, 6, 7, 8]  # src/predict.rs:32-46
BLK_W = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64]
BLK_H = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64]
TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
SIZES = list(range(13))
FORMATS = ((0, 0), (1, 0), (1, 1))


def tx_size_of(w, h):
    return [i for i in range(19) if (TX_W[i], TX_H[i]) == (w, h)][0]


def supersample(bw, bh, xdec, ydec):
    """supersample_chroma_bsize (src/partition.rs:459-498) in pixels, for the
    sizes up to 64x64 without the 4:1 ones."""
    if (bw, bh) == (4, 4):
        return bw << xdec, bh << ydec
    if (bw, bh) == (4, 8):
        return bw << xdec, bh
    if (bw, bh) == (8, 4):
        return bw, bh << ydec
    return bw, bh


@functools.lru_cache(None)
def coding_order(bw4, bh4):
    """order[r][c] of the 4x4 cells of a superblock split uniformly into
    bw4 x bh4 blocks: quadrants top-left, top-right, bottom-left,
    bottom-right down to the square, then its two halves."""
    order = np.zeros((16, 16), np.int32)
    count = [0]

    def code(r, c, s):
        if s > max(bw4, bh4):
            h = s // 2
            for dr, dc in ((0, 0), (0, h), (h, 0), (h, h)):
                code(r + dr, c + dc, h)
            return
        if bw4 == bh4:
            parts = [(r, c)]
        elif bw4 > bh4:
            parts = [(r, c), (r + bh4, c)]
        else:
            parts = [(r, c), (r, c + bw4)]
        for pr, pc in parts:
            order[pr:pr + bh4, pc:pc + bw4] = count[0]
            count[0] += 1
    code(0, 0, 16)
    return order


def has_top_right(bw, bh, mi_col, mi_row, top, right, tx_w, row_off, col_off, ss_x):
    """bw x bh: the partition in pixels after supersample; row_off / col_off
    in 4x4 units of the plane."""
    if not top or not right:
        return False
    bw4, bh4 = bw // 4, bh // 4
    plane_bw = max(bw4 >> ss_x, 1)
    if row_off > 0:
        return col_off + tx_w // 4 < plane_bw
    if col_off + tx_w // 4 < plane_bw:
        return True
    r, c = mi_row & 15, mi_col & 15
    r, c = r - r % bh4, c - c % bw4
    if r == 0:
        return True
    if c + bw4 >= 16:
        return False
    o = coding_order(bw4, bh4)
    return bool(o[r - 1, c + bw4] < o[r, c])


def has_bottom_left(bw, bh, mi_col, mi_row, bottom, left, tx_h, row_off, col_off, ss_y):
    if not bottom or not left or col_off > 0:
        return False
    bw4, bh4 = bw // 4, bh // 4
    plane_bh = max(bh4 >> ss_y, 1)
    if row_off + tx_h // 4 < plane_bh:
        return True
    r, c = mi_row & 15, mi_col & 15
    r, c = r - r % bh4, c - c % bw4
    if c == 0:
        return (r >> ss_y) + row_off + tx_h // 4 < (16 >> ss_y)
    if r + bh4 >= 16:
        return False
    o = coding_order(bw4, bh4)
    return bool(o[r + bh4, c - 1] < o[r, c])


def edge_needs(mode, x, y):
    """needs_left, _topleft, _top, _topright, _bottomleft under opt_mode
    (src/partition.rs:525-557); mode None or < 0: all."""
    if mode is None or mode < 0:
        return (True,) * 5
    if mode == 12:
        mode = 0 if (x, y) == (0, 0) else 2 if y == 0 else 1 if x == 0 else 12
    dc = mode in (0, 13)
    return (mode != 1 and (not dc or x != 0) and mode not in (3, 8),
            mode in (12, 5, 4, 6),
            mode != 2 and (not dc or y != 0),
            mode in (3, 8),
            mode == 7)


def get_intra_edges(reg, bo_x, bo_y, bx, by, bsize, po_x, po_y, tx_size, xdec, ydec, bd,
                    mode=None):
    """reg: the tile's region of the plane (2-D array, pixel (0, 0) the
    region's origin).  Returns the 257 entries, zero where nothing is
    written."""
    th_, tw_ = reg.shape
    w, h = TX_W[tx_size], TX_H[tx_size]
    x, y = po_x, po_y
    base = 128 << (bd - 8)
    e = np.zeros(257, np.int64)
    left, above = e[:128], e[129:]
    n_left, n_tl, n_top, n_tr, n_bl = edge_needs(mode, x, y)
    if n_left:
        if x != 0:
            left[128 - h:] = reg[y:y + h, x - 1][::-1]
        else:
            left[128 - h:] = reg[y - 1, 0] if y != 0 else base + 1
    if n_tl:
        e[128] = base if (x, y) == (0, 0) else reg[0, x - 1] if y == 0 else \
            reg[y - 1, 0] if x == 0 else reg[y - 1, x - 1]
    if n_top:
        if y != 0:
            above[:w] = reg[y - 1, x:x + w]
        else:
            above[:w] = reg[0, x - 1] if x != 0 else base - 1
    bx4, by4 = bx * (w // 4), by * (h // 4)
    have_top = by4 != 0 or bo_y > (1 if ydec else 0)
    have_left = bx4 != 0 or bo_x > (1 if xdec else 0)
    right, bottom = x + w < tw_, y + h < th_
    sw, sh = supersample(BLK_W[bsize], BLK_H[bsize], xdec, ydec)
    if n_tr:
        n = min(w, tw_ - x - w) if y != 0 and has_top_right(
            sw, sh, bo_x, bo_y, have_top, right, w, by4, bx4, xdec) else 0
        if n > 0:
            above[w:w + n] = reg[y - 1, x + w:x + w + n]
        if n < h:
            above[w + n:w + h] = above[w + n - 1]
    if n_bl:
        n = min(h, th_ - y - h) if x != 0 and has_bottom_left(
            sw, sh, bo_x, bo_y, bottom, have_left, h, by4, bx4, ydec) else 0
        if n > 0:
            left[128 - h - n:128 - h] = reg[y + h:y + h + n, x - 1][::-1]
        if n < w:
            left[128 - h - w:128 - h - n] = left[128 - h - n]
    return e


def variant_of(x, y):
    return 0 if (x, y) == (0, 0) else 1 if y == 0 else 2 if x == 0 else 3


def satds_of(edge, src_blk, w, h, x, y, bd):
    """get_satd of the 13 RAV1E_INTRA_MODES' predictions against the source
    block, in that order."""
    dt = np.uint16 if bd > 8 else np.uint8
    src_blk = np.ascontiguousarray(src_blk, dtype=dt)
    out = []
    for m in RAV1E_INTRA_MODES:
        pred = O.predict_intra(m, variant_of(x, y), w, h, edge.astype(dt), bd)
        out.append(O.get_satd(src_blk, 0, 0, pred, 0, 0, w, h))
    return out


def select(satds, row, num):
    """src/rdo.rs:1086-1127: the stable sort by SATD, the stable descending
    sort by probability (sort_by_key(!d)), the merge and the truncation."""
    order = sorted(range(13), key=lambda k: int(satds[k]))
    z, probs_all = 32768, []
    for a in list(row)[:13]:
        probs_all.append((z - int(a)) & 0xffff)
        z = int(a)
    porder = sorted(range(13), key=lambda k: 0xffff ^ probs_all[RAV1E_INTRA_MODES[k]])
    modes = [RAV1E_INTRA_MODES[k] for k in porder[:num // 2]]
    for k in order[:num]:
        if RAV1E_INTRA_MODES[k] not in modes:
            modes.append(RAV1E_INTRA_MODES[k])
    return modes[:num]


def screen(rec_reg, src_reg, bo_x, bo_y, bsize, bd, row, num):
    """One block: (edges, the 13 SATDs, the mode list).  rec_reg / src_reg:
    the tile's regions of the reconstruction and the source (luma)."""
    w, h = BLK_W[bsize], BLK_H[bsize]
    x, y = 4 * bo_x, 4 * bo_y
    e = get_intra_edges(rec_reg, bo_x, bo_y, 0, 0, bsize, x, y, tx_size_of(w, h), 0, 0, bd)
    s = satds_of(e, src_reg[y:y + h, x:x + w], w, h, x, y, bd)
    return e, s, select(s, row, num)

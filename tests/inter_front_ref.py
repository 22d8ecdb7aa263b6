"""The inter front of rdo_mode_decision restated in Python: the checker of
tests/test_inter_front.py.

  ref_sets           src/rdo.rs:815-835 and the compound condition of :914-927
  mode_set           src/rdo.rs:858-986 (the pushes and the MV table)
  get_params         src/predict.rs:267-284 with PlaneSlice::clamp
                     (src/frame/plane.rs:521-533)
  predict_inter      src/predict.rs:255-338, the pixels from the C oracle's
                     put_8tap / prep_8tap / mc_avg (tests/oracle_lib.py)
  motion_compensate  src/encoder.rs:1239-1430, the arm of :1416-1428

tests/golden/ref_inter_front.npz (tools/refeval/gen_inter_front_ref.py) pins
every function here to what the reference's own text gives.
"""
import numpy as np

from tests import oracle_lib as O

# BlockSize (src/partition.rs:85-108 order) in pixels
BLK_W = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64]
BLK_H = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16]
SIZES = list(range(3, 13))  # BLOCK_8X8 .. BLOCK_64X64: squares, 2:1 and 1:2
LAYOUTS = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}

LAST3_FRAME, NONE_FRAME = 3, 8
NEARESTMV, NEAR0MV, NEAR1MV, NEAR2MV, GLOBALMV, NEWMV = 14, 15, 16, 17, 18, 19
NEAREST_NEARESTMV, NEAR_NEARMV, NEAREST_NEWMV, NEW_NEARESTMV = 20, 21, 22, 23
GLOBAL_GLOBALMV, NEW_NEWMV = 26, 27
# RAV1E_INTER_COMPOUND_MODES (src/predict.rs:51-58)
COMPOUND_MODES = [GLOBAL_GLOBALMV, NEAREST_NEARESTMV, NEW_NEWMV, NEAREST_NEWMV, NEW_NEARESTMV,
                  NEAR_NEARMV]
MAX_CANDS = 20


def has_subsampled_size(b, xdec, ydec):
    """BlockSize::subsampled_size (src/partition.rs:245-286) is not
    BLOCK_INVALID: at 4:2:2 the 1:2 sizes have none."""
    return not (xdec == 1 and ydec == 0 and BLK_H[b] == 2 * BLK_W[b])


def ref_sets(allowed, ref_frames, compound_allowed, bsize):
    """(refs, slots, fwd, bwd, compound): the single sets' RefTypes and DPB
    slots, the first forward / backward set (-1: none), whether the compound
    set follows."""
    refs, slots, fwd, bwd = [], [], -1, -1
    for r in allowed:
        if r == LAST3_FRAME:
            continue
        s = int(ref_frames[r - 1])
        if s in slots:
            continue
        if fwd < 0 and r < 5:
            fwd = len(refs)
        if bwd < 0 and r >= 5:
            bwd = len(refs)
        refs.append(int(r))
        slots.append(s)
    sz = min(BLK_W[bsize], BLK_H[bsize]) // 4
    compound = bool(compound_allowed) and sz >= 2 and fwd >= 0 and bwd >= 0
    return refs, slots, fwd, bwd, compound


def mode_set(stacks, me, refs, fwd, bwd, compound, near):
    """stacks: per set (mode_context, [(this_mv, comp_mv), ...]) with MVs as
    (row, col), the compound set's last; me: per single set (row, col).
    Returns the candidates in push order as (luma_mode, set, (ref0, ref1),
    (mv0, mv1), mode_context), or None where the reference panics."""
    zero = (0, 0)
    modes = []
    for i in range(len(refs)):
        n = len(stacks[i][1])
        modes.append((NEARESTMV, i))
        if n >= 1:
            modes.append((NEAR0MV, i))
        if n >= 2:
            modes.append((GLOBALMV, i))
        if near and n >= 3:
            modes.append((NEAR1MV, i))
        if near and n >= 4:
            modes.append((NEAR2MV, i))
        m = tuple(me[i])
        if m != zero and all(tuple(e[0]) != m for e in stacks[i][1][:4 if near else 2]):
            modes.append((NEWMV, i))
    from_me = [(tuple(m), zero) for m in me]
    set_refs = [(r, NONE_FRAME) for r in refs]
    if compound:
        ns = len(refs)
        set_refs.append((refs[fwd], refs[bwd]))
        from_me.append((tuple(me[fwd]), tuple(me[bwd])))
        modes += [(m, ns) for m in COMPOUND_MODES]
        if not stacks[ns][1]:
            return None  # mv_stacks[i][0] of NEAREST_NEWMV
    if len(modes) > MAX_CANDS:
        return None  # the ArrayVec's capacity
    out = []
    for mode, i in modes:
        ctx, st = stacks[i]
        st = [(tuple(a), tuple(b)) for a, b in st]
        if mode in (NEWMV, NEW_NEWMV):
            mvs = from_me[i]
        elif mode in (NEARESTMV, NEAREST_NEARESTMV):
            mvs = st[0] if st else (zero, zero)
        elif mode in (NEAR0MV, NEAR_NEARMV):
            mvs = st[1] if len(st) > 1 else (zero, zero)
        elif mode in (NEAR1MV, NEAR2MV):
            mvs = st[mode - NEAR0MV + 1]
        elif mode == NEAREST_NEWMV:
            mvs = (st[0][0], from_me[i][1])
        elif mode == NEW_NEARESTMV:
            mvs = (from_me[i][0], st[0][1])
        else:
            mvs = (zero, zero)
        out.append((mode, i, set_refs[i], mvs, int(ctx)))
    return out


def get_params(mv, po, xdec, ydec, width, height, xorigin, yorigin):
    """(row_frac, col_frac, x, y): the fracs and the source block's position
    in the plane after the clamp.  mv: (row, col); po: (x, y)."""
    sr, sc = 3 + ydec, 3 + xdec
    ro, co = int(mv[0]) >> sr, int(mv[1]) >> sc
    rf = (int(mv[0]) - (ro << sr)) << (4 - sr)
    cf = (int(mv[1]) - (co << sc)) << (4 - sc)
    x = max(min(po[0] + co - 3, width), -xorigin) + 3
    y = max(min(po[1] + ro - 3, height), -yorigin) + 3
    return rf, cf, x, y


class RefPlane:
    """A padded reference plane: the whole allocation and its geometry."""

    def __init__(self, full, xorigin, yorigin, width, height, xdec=0, ydec=0):
        self.full = np.ascontiguousarray(full)
        self.xorigin, self.yorigin, self.width, self.height = xorigin, yorigin, width, height
        self.xdec, self.ydec = xdec, ydec

    @classmethod
    def from_device(cls, plane):
        d = plane.desc
        return cls(plane.download_full(), d.xorigin, d.yorigin, d.width, d.height, d.xdec, d.ydec)


def predict_inter(planes, frame_po, w, h, mvs, mode, bd):
    """predict_inter of one plane: planes = the one or two references' RefPlane
    of this plane, mvs their MVs; returns the w x h block."""
    outs = []
    for pl, mv in zip(planes, mvs):
        rf, cf, x, y = get_params(mv, frame_po, pl.xdec, pl.ydec, pl.width, pl.height, pl.xorigin,
                                  pl.yorigin)
        f = O.put_8tap if len(planes) == 1 else O.prep_8tap
        outs.append(f(pl.full, pl.yorigin + y, pl.xorigin + x, w, h, cf, rf, mode, mode, bd))
    if len(outs) == 1:
        return outs[0]
    return O.mc_avg(outs[0], outs[1], bd, 1 if bd > 8 else 0)


def motion_compensate(ref_sets_, tile, bo, bsize, ref_slot, mvs, mode, bd, luma_only=False):
    """ref_sets_: per DPB slot three RefPlanes; tile: (x, y, width, height) in
    luma pixels; bo: tile_bo (x, y) in 4x4 units; ref_slot: (slot0, slot1),
    slot1 < 0 for a single reference.  Returns {plane: (x, y, pixels)}: the
    block's position in the frame's plane and its prediction."""
    out = {}
    nref = 2 if ref_slot[1] >= 0 else 1
    for p in range(1 if luma_only else 3):
        pl0 = ref_sets_[ref_slot[0]][p]
        xd, yd = pl0.xdec, pl0.ydec
        w, h = (BLK_W[bsize], BLK_H[bsize]) if p == 0 else (BLK_W[bsize] >> xd, BLK_H[bsize] >> yd)
        # tile_bo.plane_offset, tile_rect.decimated().to_frame_plane_offset
        fx = (tile[0] >> xd) + ((4 * bo[0]) >> xd)
        fy = (tile[1] >> yd) + ((4 * bo[1]) >> yd)
        planes = [ref_sets_[ref_slot[k]][p] for k in range(nref)]
        out[p] = (fx, fy, predict_inter(planes, (fx, fy), w, h, mvs[:nref], mode, bd))
    return out

"""A plain-Python serial restatement of the block mode-info symbols the
device tokenizer (rv_ec_mode.hip) forms: encode_block_pre_cdef and the symbol
part of encode_block_post_cdef (src/encoder.rs:1446-1662) and write_partition
(src/context.rs:2059-2109), with the ContextWriter / BlockContext methods
they call.  It walks the jobs in coding order and keeps what the reference
keeps: a per-tile block map (TileBlocks) and the above / left partition
context arrays.  No ctypes.  tests/test_ec_mode.py pins it to the
reference-evaluated vectors (tests/golden/ref_ec_mode.npz) and compares the
device tokens with it.

Per job it returns a list of ops (offset, length, symbol, gather): a
symbol_with_update on the CDF slice [offset, offset + length) of the combined
table (gather 0), or the frame-edge partition symbol (gather 1:
partition_gather_vert_alike, 2: _horz_alike) against the partition CDF at
[offset, offset + length).
"""
import numpy as np

# ---- the combined table's mode families (rv_ec_mode_tables.h) --------------
EC_TOTAL = 4317
_FAMILIES = [("PARTITION", 20 * 11), ("KF_Y", 25 * 14), ("Y_MODE", 4 * 14), ("UV_MODE", 26 * 15),
             ("CFL_SIGN", 9), ("CFL_ALPHA", 6 * 17), ("NEWMV", 7 * 3), ("ZEROMV", 2 * 3),
             ("REFMV", 6 * 3), ("SKIP", 3 * 3), ("INTRA_INTER", 4 * 3), ("ANGLE_DELTA", 8 * 8),
             ("COMP_MODE", 5 * 3), ("COMP_REF_TYPE", 5 * 3), ("COMP_REF", 9 * 3),
             ("COMP_BWD_REF", 6 * 3), ("SINGLE_REF", 18 * 3), ("DRL", 3 * 3),
             ("COMPOUND_MODE", 8 * 9), ("MV_JOINTS", 5), ("MV_COMP", 2 * 69), ("SEG", 3 * 9)]
OFF = {}
_o = EC_TOTAL
for _n, _c in _FAMILIES:
    OFF[_n] = _o
    _o += _c
EC_TOTAL_ALL = _o
# NMVComponent's fields inside one component
MVC_CLASSES, MVC_CLASS0_FP, MVC_FP, MVC_SIGN, MVC_CLASS0_HP, MVC_HP, MVC_CLASS0, MVC_BITS = (
    0, 12, 22, 27, 30, 33, 36, 39)

# ---- the job row (EC_MODE_JOB's fields, in order) ---------------------------
FIELDS = ["kind", "tile", "bx", "by", "bsize", "partition", "skip", "seg_idx", "luma_mode",
          "chroma_mode", "ref0", "ref1", "mv0_row", "mv0_col", "mv1_row", "mv1_col",
          "ref_mv0_row", "ref_mv0_col", "ref_mv1_row", "ref_mv1_col", "mode_context",
          "num_mv_found", "weight0", "weight1", "weight2", "weight3", "cfl_joint_sign",
          "cfl_scale_u", "cfl_scale_v"]
F = {n: i for i, n in enumerate(FIELDS)}
NF = 32  # int32 words per job

BLOCK_8X8, BLOCK_16X16, BLOCK_32X32, BLOCK_64X64 = 3, 6, 9, 12
BSIZE_LG = {BLOCK_8X8: 3, BLOCK_16X16: 4, BLOCK_32X32: 5, BLOCK_64X64: 6}
PARTITION_NONE, PARTITION_SPLIT = 0, 3
DC_PRED, V_PRED, D63_PRED, UV_CFL_PRED = 0, 1, 8, 13
NEARESTMV, NEAR0MV, NEAR1MV, NEAR2MV, GLOBALMV, NEWMV = 14, 15, 16, 17, 18, 19
(NEAREST_NEARESTMV, NEAR_NEARMV, NEAREST_NEWMV, NEW_NEARESTMV, NEAR_NEWMV, NEW_NEARMV,
 GLOBAL_GLOBALMV, NEW_NEWMV) = range(20, 28)
INTRA_FRAME, LAST_FRAME, LAST2_FRAME, LAST3_FRAME, GOLDEN_FRAME = 0, 1, 2, 3, 4
BWDREF_FRAME, ALTREF2_FRAME, ALTREF_FRAME, NONE_FRAME = 5, 6, 7, 8
REF_CAT_LEVEL = 640
KEY, INTER = 0, 1
INTRA_MODE_CONTEXT = [0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0]
SIZE_GROUP = {BLOCK_8X8: 1, BLOCK_16X16: 2, BLOCK_32X32: 3, BLOCK_64X64: 3}


class Params:
    """The frame parameters rv_ec_mode_tokenize takes by value, and every
    tile's cols / rows in luma 4x4 units."""

    def __init__(self, frame_type=INTER, reference_mode=0, force_integer_mv=0,
                 allow_high_precision_mv=0, seg_enabled=0, last_active_segid=0,
                 tile_dims=((32, 32),)):
        self.frame_type, self.reference_mode = frame_type, reference_mode
        self.force_integer_mv, self.allow_high_precision_mv = force_integer_mv, allow_high_precision_mv
        self.seg_enabled, self.last_active_segid = seg_enabled, last_active_segid
        self.tile_dims = [tuple(int(v) for v in d) for d in tile_dims]


def has_near(m):
    return NEAR0MV <= m <= NEAR2MV or m in (NEAR_NEARMV, NEAR_NEWMV, NEW_NEARMV)


def near_ref_mv_idx(m):
    return m - NEAR0MV + 1 if NEAR0MV <= m <= NEAR2MV else 1


def job_ok(j, prm):
    """The tokenizer's restrictions (rv_ec_mode.hip's header comment)."""
    g = lambda n: int(j[F[n]])
    if g("kind") not in (0, 1) or not 0 <= g("tile") < len(prm.tile_dims):
        return False
    if g("bsize") not in BSIZE_LG:
        return False
    cols, rows = prm.tile_dims[g("tile")]
    n4 = 1 << (BSIZE_LG[g("bsize")] - 2)
    bx, by = g("bx"), g("by")
    if cols < 2 or rows < 2 or (cols | rows) & 1:
        return False
    if bx < 0 or by < 0 or bx >= cols or by >= rows or (bx | by) & (n4 - 1):
        return False
    if g("kind") == 1:
        if g("partition") not in (PARTITION_NONE, PARTITION_SPLIT):
            return False
        hbs = n4 >> 1
        if (bx + hbs < cols) != (by + hbs < rows):  # an edge form
            return g("partition") == PARTITION_SPLIT and g("bsize") > BLOCK_8X8
        return True
    if g("skip") not in (0, 1) or not 0 <= g("seg_idx") <= 7:
        return False
    if prm.seg_enabled and not (0 <= prm.last_active_segid <= 7 and g("seg_idx") <= prm.last_active_segid):
        return False
    lm, cm, r0, r1 = g("luma_mode"), g("chroma_mode"), g("ref0"), g("ref1")
    if not (0 <= lm <= 27) or lm == UV_CFL_PRED:
        return False
    if lm < NEARESTMV:
        if not 0 <= cm <= UV_CFL_PRED or r0 != INTRA_FRAME or r1 not in (INTRA_FRAME, NONE_FRAME):
            return False
        if cm == UV_CFL_PRED:
            js = g("cfl_joint_sign")
            if g("bsize") > BLOCK_32X32 or not 0 <= js <= 7:
                return False
            sg = ((js + 1) // 3, (js + 1) % 3)
            for uv in range(2):
                if sg[uv] and not 1 <= g(("cfl_scale_u", "cfl_scale_v")[uv]) <= 16:
                    return False
        return True
    if prm.frame_type != INTER or cm != lm:
        return False
    ctx = g("mode_context")
    if ctx < 0 or (ctx & 7) > 6 or ((ctx >> 4) & 15) > 5:
        return False
    nf = g("num_mv_found")
    if not 0 <= nf <= 9:
        return False
    if lm >= NEAREST_NEARESTMV:
        if not prm.reference_mode or not LAST_FRAME <= r0 <= GOLDEN_FRAME or \
                not BWDREF_FRAME <= r1 <= ALTREF_FRAME:
            return False
    elif not LAST_FRAME <= r0 <= ALTREF_FRAME or r1 not in (INTRA_FRAME, NONE_FRAME):
        return False
    if lm == NEW_NEWMV and nf < 2:
        return False
    if has_near(lm) and lm != NEAR0MV and nf <= near_ref_mv_idx(lm):
        return False
    for k, on in ((0, lm in (NEWMV, NEW_NEWMV, NEW_NEARESTMV)), (1, lm in (NEW_NEWMV, NEAREST_NEWMV))):
        if on:
            for c in ("row", "col"):
                if abs(g("mv%d_%s" % (k, c)) - g("ref_mv%d_%s" % (k, c))) > (1 << 14):
                    return False
    return True


class _Tile:
    def __init__(self, cols, rows):
        self.cols, self.rows = cols, rows
        w, h = (cols + 1) // 2 + 8, (rows + 1) // 2 + 8  # a leaf may hang over the edge
        self.skip = np.zeros((h, w), np.int64)
        self.mode = np.zeros((h, w), np.int64)  # DC_PRED: Block::default
        self.ref = np.zeros((h, w, 2), np.int64)  # [INTRA_FRAME; 2]
        self.seg = np.zeros((h, w), np.int64)
        self.above_pc = np.zeros(w, np.int64)
        self.left_pc = np.zeros(8, np.int64)
        self.sb_row = -1


def segment_pred(t, bx, by):
    """get_segment_pred (src/context.rs:3465-3505): (pred, cdf_index)"""
    x, y = bx >> 1, by >> 1
    ul = t.seg[y - 1, x - 1] if bx > 0 and by > 0 else -1
    u = t.seg[y - 1, x] if by > 0 else -1
    l = t.seg[y, x - 1] if bx > 0 else -1
    if ul < 0 or u < 0 or l < 0:
        ci = 0
    elif ul == u and ul == l:
        ci = 2
    elif ul == u or ul == l or u == l:
        ci = 1
    else:
        ci = 0
    if u == -1:
        r = 0 if l == -1 else l
    elif l == -1:
        r = u
    else:
        r = u if ul == u else l
    return int(r), ci


def neg_interleave(x, r, mx):
    """src/context.rs:3507-3534"""
    if r == 0:
        return x
    if r >= mx - 1:
        return -x + mx - 1
    diff = x - r
    if 2 * r < mx:
        if abs(diff) <= r:
            return (diff << 1) - 1 if diff > 0 else (-diff) << 1
        return x
    if abs(diff) < mx - r:
        return (diff << 1) - 1 if diff > 0 else (-diff) << 1
    return (mx - x) - 1


def ref_count_ctx(a, b):
    return 0 if a < b else 1 if a == b else 2


def mv_component_ops(ops, comp, base, precision):
    """encode_mv_component (src/context.rs:4319-4370); precision -1 NONE, 0 LOW, 1 HIGH"""
    sign = 1 if comp < 0 else 0
    mag = -comp if sign else comp
    z = mag - 1
    c = 10 if z >= 2 * 4096 else max(0, (z >> 3).bit_length() - 1)
    offset = z - ((2 << (c + 2)) if c else 0)
    d, fr, hp = offset >> 3, (offset >> 1) & 3, offset & 1
    ops.append((base + MVC_SIGN, 3, sign, 0))
    ops.append((base + MVC_CLASSES, 12, c, 0))
    if c == 0:
        ops.append((base + MVC_CLASS0, 3, d, 0))
    else:
        for i in range(c):
            ops.append((base + MVC_BITS + 3 * i, 3, (d >> i) & 1, 0))
    if precision > -1:
        ops.append((base + (MVC_CLASS0_FP + 5 * d if c == 0 else MVC_FP), 5, fr, 0))
    if precision > 0:
        ops.append((base + (MVC_CLASS0_HP if c == 0 else MVC_HP), 3, hp, 0))


def tokenize(jobs, prm):
    """(ops per job, rejected job count, seg_idx per job as the reference
    leaves it: a skip block's becomes its prediction when segmentation is on)."""
    jobs = np.asarray(jobs, np.int64).reshape(-1, NF)
    tiles = {}
    out, bad = [], 0
    seg_out = jobs[:, F["seg_idx"]].copy()
    precision = -1 if prm.force_integer_mv else (1 if prm.allow_high_precision_mv else 0)
    for ji, j in enumerate(jobs):
        ops = []
        out.append(ops)
        if not job_ok(j, prm):
            bad += 1
            continue
        g = lambda n: int(j[F[n]])
        ti = g("tile")
        if ti not in tiles:
            tiles[ti] = _Tile(*prm.tile_dims[ti])
        t = tiles[ti]
        bx, by, bsize = g("bx"), g("by"), g("bsize")
        lg = BSIZE_LG[bsize]
        n4 = 1 << (lg - 2)
        x8, y8, n8 = bx >> 1, by >> 1, n4 >> 1
        if by >> 4 != t.sb_row:  # reset_left_contexts at a superblock row's start
            t.sb_row = by >> 4
            t.left_pc[:] = 0
        if g("kind") == 1:
            # write_partition (src/context.rs:2059-2109)
            hbs = n4 >> 1
            has_cols, has_rows = bx + hbs < t.cols, by + hbs < t.rows
            bsl = lg - 3
            above = (int(t.above_pc[x8]) >> bsl) & 1
            left = (int(t.left_pc[(by & 15) >> 1]) >> bsl) & 1
            ctx = left * 2 + above + bsl * 4
            off, ln = OFF["PARTITION"] + ctx * 11, (5 if bsize == BLOCK_8X8 else 11)
            p = g("partition")
            if has_rows and has_cols:
                ops.append((off, ln, p, 0))
            elif not has_rows and has_cols:
                ops.append((off, ln, int(p == PARTITION_SPLIT), 1))
            elif has_rows and not has_cols:
                ops.append((off, ln, int(p == PARTITION_SPLIT), 2))
            continue
        skip, lm, cm = g("skip"), g("luma_mode"), g("chroma_mode")
        is_inter = lm >= NEARESTMV
        has_above, has_left = by > 0, bx > 0
        # encode_block_pre_cdef: write_skip, write_segmentation (preskip false)
        sctx = int(has_above and t.skip[y8 - 1, x8]) + int(has_left and t.skip[y8, x8 - 1])
        t.skip[y8:y8 + n8, x8:x8 + n8] = skip
        ops.append((OFF["SKIP"] + 3 * sctx, 3, skip, 0))
        seg = g("seg_idx")
        if prm.seg_enabled:
            pred, ci = segment_pred(t, bx, by)
            if skip:
                seg = pred
            else:
                ops.append((OFF["SEG"] + 9 * ci, 9,
                            neg_interleave(seg, pred, prm.last_active_segid + 1), 0))
        seg_out[ji] = seg
        t.seg[y8:y8 + n8, x8:x8 + n8] = seg
        # encode_block_post_cdef
        if prm.frame_type == INTER:
            # intra_inter_context (src/context.rs:1744-1774)
            ai = has_above and t.mode[y8 - 1, x8] < NEARESTMV
            li = has_left and t.mode[y8, x8 - 1] < NEARESTMV
            if has_above and has_left:
                ictx = 3 if ai and li else int(ai or li)
            elif has_above or has_left:
                ictx = 2 if (ai or li) else 0
            else:
                ictx = 0
            ops.append((OFF["INTRA_INTER"] + 3 * ictx, 3, int(is_inter), 0))
            if is_inter:
                rf = (g("ref0"), g("ref1"))
                # fill_neighbours_ref_counts (:2967-2990)
                cnt = [0] * 7
                for have, yy, xx in ((has_above, y8 - 1, x8), (has_left, y8, x8 - 1)):
                    if have and t.mode[yy, xx] >= NEARESTMV:
                        cnt[int(t.ref[yy, xx, 0]) - 1] += 1
                        if t.ref[yy, xx, 1] not in (INTRA_FRAME, NONE_FRAME):
                            cnt[int(t.ref[yy, xx, 1]) - 1] += 1
                a0, a1 = (int(t.ref[y8 - 1, x8, 0]), int(t.ref[y8 - 1, x8, 1])) if has_above else (0, 8)
                l0, l1 = (int(t.ref[y8, x8 - 1, 0]), int(t.ref[y8, x8 - 1, 1])) if has_left else (0, 8)
                ll2_l3g = ref_count_ctx(cnt[0] + cnt[1], cnt[2] + cnt[3])
                l_l2 = ref_count_ctx(cnt[0], cnt[1])
                l3_g = ref_count_ctx(cnt[2], cnt[3])
                bf2_a = ref_count_ctx(cnt[4] + cnt[5], cnt[6])
                b_a2 = ref_count_ctx(cnt[4], cnt[5])
                comp = rf[1] not in (INTRA_FRAME, NONE_FRAME)
                if prm.reference_mode:  # sz >= 2 holds for every block in scope
                    ls, as_ = l1 == NONE_FRAME, a1 == NONE_FRAME
                    lin, ain = l0 == INTRA_FRAME, a0 == INTRA_FRAME
                    lb, ab = l0 >= 5, a0 >= 5
                    if has_left and has_above:
                        if as_ and ls:
                            c = int(ab ^ lb)
                        elif as_:
                            c = 2 + int(ab or ain)
                        elif ls:
                            c = 2 + int(lb or lin)
                        else:
                            c = 4
                    elif has_above:
                        c = int(ab) if as_ else 3
                    elif has_left:
                        c = int(lb) if ls else 3
                    else:
                        c = 1
                    ops.append((OFF["COMP_MODE"] + 3 * c, 3, int(comp), 0))
                if comp:
                    samedir = lambda r0, r1: (r0 >= 5 and r0 != 8) == (r1 >= 5 and r1 != 8)
                    ls, as_ = l1 == NONE_FRAME, a1 == NONE_FRAME
                    lin, ain = l0 == INTRA_FRAME, a0 == INTRA_FRAME
                    aci = has_above and not ain and not as_
                    lci = has_left and not lin and not ls
                    auc = aci and samedir(a0, a1)
                    luc = lci and samedir(l0, l1)
                    if has_above and not ain and has_left and not lin:
                        sd = int(samedir(a0, l0))
                        if not aci and not lci:
                            c = 1 + 2 * sd
                        elif not aci:
                            c = 1 if not luc else 3 + sd
                        elif not lci:
                            c = 1 if not auc else 3 + sd
                        elif not auc and not luc:
                            c = 0
                        elif not auc or not luc:
                            c = 2
                        else:
                            c = 3 + int((a0 == BWDREF_FRAME) == (l0 == BWDREF_FRAME))
                    elif has_above and has_left:
                        c = 1 + 2 * int(auc) if aci else 1 + 2 * int(luc) if lci else 2
                    elif aci:
                        c = 4 * int(auc)
                    elif lci:
                        c = 4 * int(luc)
                    else:
                        c = 2
                    ops.append((OFF["COMP_REF_TYPE"] + 3 * c, 3, 1, 0))
                    cr = rf[0] in (GOLDEN_FRAME, LAST3_FRAME)
                    ops.append((OFF["COMP_REF"] + (ll2_l3g * 3 + 0) * 3, 3, int(cr), 0))
                    if not cr:
                        ops.append((OFF["COMP_REF"] + (l_l2 * 3 + 1) * 3, 3, int(rf[0] == LAST2_FRAME), 0))
                    else:
                        ops.append((OFF["COMP_REF"] + (l3_g * 3 + 2) * 3, 3, int(rf[0] == GOLDEN_FRAME), 0))
                    cb = rf[1] == ALTREF_FRAME
                    ops.append((OFF["COMP_BWD_REF"] + (bf2_a * 2 + 0) * 3, 3, int(cb), 0))
                    if not cb:
                        ops.append((OFF["COMP_BWD_REF"] + (b_a2 * 2 + 1) * 3, 3,
                                    int(rf[1] == ALTREF2_FRAME), 0))
                else:
                    b0c = ref_count_ctx(cnt[0] + cnt[1] + cnt[2] + cnt[3], cnt[4] + cnt[5] + cnt[6])
                    sr = lambda c, k, s: ops.append((OFF["SINGLE_REF"] + (c * 6 + k) * 3, 3, int(s), 0))
                    b0 = rf[0] >= 5
                    sr(b0c, 0, b0)
                    if b0:
                        b1 = rf[0] == ALTREF_FRAME
                        sr(bf2_a, 1, b1)
                        if not b1:
                            sr(b_a2, 5, rf[0] == ALTREF2_FRAME)
                    else:
                        b2 = rf[0] in (LAST3_FRAME, GOLDEN_FRAME)
                        sr(ll2_l3g, 2, b2)
                        if not b2:
                            sr(l_l2, 3, rf[0] != LAST_FRAME)
                        else:
                            sr(l3_g, 4, rf[0] != LAST3_FRAME)
                ctx = g("mode_context")
                newmv_ctx, refmv_ctx = ctx & 7, (ctx >> 4) & 15
                if lm >= NEAREST_NEARESTMV:  # write_compound_mode
                    if refmv_ctx < 2:
                        c = min(newmv_ctx, 1)
                    elif refmv_ctx < 4:
                        c = min(newmv_ctx + 1, 4)
                    else:
                        c = min(max(newmv_ctx, 1) + 3, 7)
                    ops.append((OFF["COMPOUND_MODE"] + 9 * c, 9, lm - NEAREST_NEARESTMV, 0))
                else:  # write_inter_mode
                    ops.append((OFF["NEWMV"] + 3 * newmv_ctx, 3, int(lm != NEWMV), 0))
                    if lm != NEWMV:
                        ops.append((OFF["ZEROMV"] + 3 * ((ctx >> 3) & 1), 3, int(lm != GLOBALMV), 0))
                        if lm != GLOBALMV:
                            ops.append((OFF["REFMV"] + 3 * refmv_ctx, 3, int(lm != NEARESTMV), 0))
                nf = g("num_mv_found")
                wt = [g("weight%d" % k) for k in range(4)]
                drl_ctx = lambda i: int(wt[i] < REF_CAT_LEVEL) + int(wt[i + 1] < REF_CAT_LEVEL)
                if lm in (NEWMV, NEW_NEWMV):
                    for idx in range(2):
                        if nf > idx + 1:
                            ops.append((OFF["DRL"] + 3 * drl_ctx(idx), 3, 0, 0))  # ref_mv_idx 0
                            break
                for k, on in ((0, lm in (NEWMV, NEW_NEWMV, NEW_NEARESTMV)),
                              (1, lm in (NEW_NEWMV, NEAREST_NEWMV))):
                    if not on:
                        continue
                    dr = g("mv%d_row" % k) - g("ref_mv%d_row" % k)
                    dc = g("mv%d_col" % k) - g("ref_mv%d_col" % k)
                    jt = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
                    ops.append((OFF["MV_JOINTS"], 5, jt, 0))
                    if jt in (2, 3):
                        mv_component_ops(ops, dr, OFF["MV_COMP"], precision)
                    if jt in (1, 3):
                        mv_component_ops(ops, dc, OFF["MV_COMP"] + 69, precision)
                if has_near(lm):
                    rmi = near_ref_mv_idx(lm)
                    for idx in range(1, 3):
                        if nf > idx + 1:
                            drl = rmi > idx
                            ops.append((OFF["DRL"] + 3 * drl_ctx(idx), 3, int(drl), 0))
                            if not drl:
                                break
            else:
                ops.append((OFF["Y_MODE"] + 14 * SIZE_GROUP[bsize], 14, lm, 0))
        else:
            am = int(t.mode[y8 - 1, x8]) if has_above else DC_PRED
            lmode = int(t.mode[y8, x8 - 1]) if has_left else DC_PRED
            ops.append((OFF["KF_Y"] + (INTRA_MODE_CONTEXT[am] * 5 + INTRA_MODE_CONTEXT[lmode]) * 14,
                        14, lm, 0))
        if not is_inter:
            if V_PRED <= lm <= D63_PRED:
                ops.append((OFF["ANGLE_DELTA"] + 8 * (lm - V_PRED), 8, 3, 0))
            cfl_ok = bsize <= BLOCK_32X32
            ops.append((OFF["UV_MODE"] + (int(cfl_ok) * 13 + lm) * 15, 15 if cfl_ok else 14, cm, 0))
            if cm == UV_CFL_PRED:
                js = g("cfl_joint_sign")
                sg = ((js + 1) // 3, (js + 1) % 3)
                sc = (g("cfl_scale_u"), g("cfl_scale_v"))
                ops.append((OFF["CFL_SIGN"], 9, js, 0))
                for uv in range(2):
                    if sg[uv]:
                        ops.append((OFF["CFL_ALPHA"] + 17 * ((sg[uv] - 1) * 3 + sg[1 - uv]), 17,
                                    sc[uv] - 1, 0))
            if V_PRED <= cm <= D63_PRED:
                ops.append((OFF["ANGLE_DELTA"] + 8 * (cm - V_PRED), 8, 3, 0))
        t.mode[y8:y8 + n8, x8:x8 + n8] = lm
        t.ref[y8:y8 + n8, x8:x8 + n8] = (g("ref0"), g("ref1"))
        # update_partition_context of a PARTITION_NONE leaf (src/encoder.rs:2711-2717)
        pc = (31 << (lg - 2)) & 31  # partition_context_lookup of a square size
        t.above_pc[x8:x8 + n8] = pc
        y0 = (by & 15) >> 1
        t.left_pc[y0:y0 + n8] = pc
    return out, bad, seg_out


def op_token(op):
    off, ln, s, gather = op  # an edge op's block-size class: tokens() adds it
    return off | ln << 13 | s << 18 | gather << 23


def tokens(jobs, prm):
    """The u32 tokens of every job and the offsets, as the device lays them out."""
    jobs = np.asarray(jobs, np.int64).reshape(-1, NF)
    ops, bad, _ = tokenize(jobs, prm)
    tok, offs = [], [0]
    for j, o in zip(jobs, ops):
        for op in o:
            t = op_token(op)
            if op[3]:
                t |= (BSIZE_LG[int(j[F["bsize"]])] - 3) << 25
            tok.append(t)
        offs.append(len(tok))
    return np.array(tok, np.uint32), np.array(offs, np.uint32), bad


def gather_cdf(cdf, gather):
    """partition_gather_vert_alike (1) / _horz_alike (2) (src/context.rs:1995-2057):
    the 2-entry CDF of the edge symbol from the 10-type partition CDF."""
    prob = lambda e: (int(cdf[e - 1]) if e > 0 else 32768) - int(cdf[e])
    types = (2, 3, 4, 6, 7, 9) if gather == 1 else (1, 3, 4, 5, 6, 8)
    o = 32768
    for e in types:
        o = (o - prob(e)) & 0xFFFF
    return [(32768 - o) & 0xFFFF, 0]

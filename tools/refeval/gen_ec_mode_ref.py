"""Reference-evaluated vectors for the block mode-info symbols
(tests/golden/ref_ec_mode.npz).

    python tools/refeval/gen_ec_mode_ref.py        (in the build container)

Runs the reference's own text through tools/refeval/rsinterp.py:

  src/context.rs  ContextWriter::write_partition with partition_gather_*_alike
                  and cdf_element_prob (:1991-2109), write_intra_mode_kf,
                  write_intra_mode, write_intra_uv_mode, write_cfl_alphas,
                  write_angle_delta (:2223-2295), fill_neighbours_ref_counts,
                  ref_count_ctx, get_ref_frame_ctx_b0, get_pred_ctx_*,
                  get_comp_mode_ctx, get_comp_ref_type_ctx, write_ref_frames
                  (:2967-3334), write_compound_mode, write_inter_mode,
                  write_drl_mode, write_mv (:3336-3417), write_skip,
                  get_segment_pred, neg_interleave, write_segmentation
                  (:3458-3557), write_is_inter (:3743-3753);
                  BlockContext::partition_plane_context,
                  update_partition_context, skip_context, intra_inter_context,
                  reset_left_contexts (:1681-1774); Block::is_inter /
                  has_second_ref (:1416-1423); CFLParams::joint_sign / context /
                  index (:1893-1905); av1_get_mv_joint, mv_joint_*,
                  mv_class_base, log_in_base_2, get_mv_class,
                  encode_mv_component (:4268-4370); and for the interleaved
                  case everything gen_ec_ref.py loads for write_coeffs_lv_map.
  src/ec.rs       WriterBase<WriterEncoder> (as gen_ec_ref.py)

What this script restates is call order only:
  * of a leaf, encode_partition_topdown's set_segmentation_idx
    (src/encoder.rs:2523), then encode_block_pre_cdef (:1446-1480: set_skip,
    write_skip, write_segmentation with preskip false) and the symbol part of
    encode_block_post_cdef (:1482-1662: set_block_size / set_mode /
    set_ref_frames, write_is_inter, fill_neighbours_ref_counts,
    write_ref_frames, write_compound_mode | write_inter_mode, the first DRL
    loop, write_mv x2, the second DRL loop | write_intra_mode |
    write_intra_mode_kf, then write_angle_delta, write_intra_uv_mode,
    write_cfl_alphas, write_angle_delta), update_partition_context
    (:2711-2717);
  * of a partition node, encode_partition_topdown's early return (:2399-2401)
    and its write_partition call (:2490-2493) before the children;
  * of a tile, encode_tile's reset_left_contexts per superblock row.
The TileBlocks accessors (src/tiling/tile_blocks.rs: above_of, left_of,
above_left_of, set_*) are a data model over a grid of Block values.

Every symbol goes through the reference's methods into a recording writer
that forwards to WriterBase<WriterEncoder>.  Recorded per call: the flat
offset of the CDF (family + context, the combined layout of
rv_ec_mode_tables.h), the slice length, the symbol; for the frame-edge
partition symbol the partition CDF it was gathered from and which gather
(read off the entries the gather touched).  Per tile: the bytes of done() and
the final CDFs.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_ec_mode_tables as M  # noqa: E402
import gen_ec_ref as E  # noqa: E402
import gen_ec_tables as T  # noqa: E402
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402
from gen_mvref_ref import PM, REF_NAMES, usz  # noqa: E402

REF = G.REF
OUT = os.path.join(E.ROOT, "tests", "golden", "ref_ec_mode.npz")
NF = 32
FIELDS = ["kind", "tile", "bx", "by", "bsize", "partition", "skip", "seg_idx", "luma_mode",
          "chroma_mode", "ref0", "ref1", "mv0_row", "mv0_col", "mv1_row", "mv1_col",
          "ref_mv0_row", "ref_mv0_col", "ref_mv1_row", "ref_mv1_col", "mode_context",
          "num_mv_found", "weight0", "weight1", "weight2", "weight3", "cfl_joint_sign",
          "cfl_scale_u", "cfl_scale_v"]
F = {n: i for i, n in enumerate(FIELDS)}
MODE_FIELDS = [("partition_cdf", "PARTITION"), ("kf_y_cdf", "KF_Y"), ("y_mode_cdf", "Y_MODE"),
               ("uv_mode_cdf", "UV_MODE"), ("cfl_sign_cdf", "CFL_SIGN"),
               ("cfl_alpha_cdf", "CFL_ALPHA"), ("newmv_cdf", "NEWMV"), ("zeromv_cdf", "ZEROMV"),
               ("refmv_cdf", "REFMV"), ("skip_cdfs", "SKIP"), ("intra_inter_cdfs", "INTRA_INTER"),
               ("angle_delta_cdf", "ANGLE_DELTA"), ("comp_mode_cdf", "COMP_MODE"),
               ("comp_ref_type_cdf", "COMP_REF_TYPE"), ("comp_ref_cdf", "COMP_REF"),
               ("comp_bwd_ref_cdf", "COMP_BWD_REF"), ("single_ref_cdfs", "SINGLE_REF"),
               ("drl_cdfs", "DRL"), ("compound_mode_cdf", "COMPOUND_MODE"),
               ("nmv_context", None), ("spatial_segmentation_cdfs", "SEG")]
BLOCK_OF_LG = {3: 3, 4: 6, 5: 9, 6: 12}


class RefT(int):
    def __new__(cls, v):
        return int.__new__(cls, v)

    def to_index(self):
        assert 1 <= int(self) <= 7
        return usz(int(self) - 1)

    def is_bwd_ref(self):
        return int(self) >= 5

    def is_fwd_ref(self):
        return int(self) < 5


class Tracked(list):
    """A partition CDF that notes its reads: the edge symbol's 2-entry CDF is
    a local of write_partition, so the CDF it came from and which gather made
    it are read off the entries the gather touched."""
    log = []

    def __getitem__(self, i):
        if not isinstance(i, slice):
            Tracked.log.append((self, int(i)))
        return list.__getitem__(self, i)


def tile_bo(x, y):
    bo = RI.Struct("BlockOffset", {"x": usz(x), "y": usz(y)})
    return RI.Struct("TileBlockOffset", {
        "0": bo, "y_in_sb": lambda: usz(y & 15),
        "with_offset": lambda dx, dy: tile_bo(x + int(RI.deref(dx)), y + int(RI.deref(dy)))})


def new_block():
    """Block::default (src/context.rs:1425-1443), the fields the scope reads"""
    return RI.Struct("Block", {
        "mode": PM["DC_PRED"], "skip": False, "ref_frames": [RefT(0), RefT(0)],
        "neighbors_ref_counts": [usz(0)] * 7, "n4_w": usz(16), "n4_h": usz(16),
        "segmentation_idx": RI.TInt(0, "u8")})


class Blocks:
    """TileBlocksMut over a grid of Block values (src/tiling/tile_blocks.rs)."""

    def __init__(self, cols, rows):
        self._cols, self._rows = cols, rows
        self.grid = [[new_block() for _ in range(cols + 16)] for _ in range(rows + 16)]

    def index_any(self, bo):
        b = bo._f["0"]
        return self.grid[int(b._f["y"])][int(b._f["x"])]

    def above_of(self, bo):
        b = bo._f["0"]
        return self.grid[int(b._f["y"]) - 1][int(b._f["x"])]

    def left_of(self, bo):
        b = bo._f["0"]
        return self.grid[int(b._f["y"])][int(b._f["x"]) - 1]

    def above_left_of(self, bo):
        b = bo._f["0"]
        return self.grid[int(b._f["y"]) - 1][int(b._f["x"]) - 1]

    def cols(self):
        return usz(self._cols)

    def rows(self):
        return usz(self._rows)

    def for_each(self, bo, bsize, f):  # clipped to the tile like TileBlocksMut::for_each
        b = bo._f["0"]
        x, y = int(b._f["x"]), int(b._f["y"])
        for j in range(y, min(y + (bsize.h >> 2), self._rows)):
            for i in range(x, min(x + (bsize.w >> 2), self._cols)):
                f(self.grid[j][i])

    def set_segmentation_idx(self, bo, bsize, idx):
        self.for_each(bo, bsize, lambda b: setattr(b, "segmentation_idx", RI.TInt(int(idx), "u8")))

    def set_skip(self, bo, bsize, skip):
        self.for_each(bo, bsize, lambda b: setattr(b, "skip", bool(skip)))

    def set_mode(self, bo, bsize, mode):
        self.for_each(bo, bsize, lambda b: setattr(b, "mode", int(mode)))

    def set_block_size(self, bo, bsize):
        def f(b):
            b.n4_w, b.n4_h = usz(bsize.w >> 2), usz(bsize.h >> 2)
        self.for_each(bo, bsize, f)

    def set_ref_frames(self, bo, bsize, r):
        self.for_each(bo, bsize, lambda b: setattr(b, "ref_frames", [RefT(r[0]), RefT(r[1])]))


def make():
    I = E.make()
    ctx = G.src_of(I, "context.rs")
    I.define_impl("BlockContext", [ctx.fn(n, "impl<'a> BlockContext<'a>") for n in (
        "partition_plane_context", "update_partition_context", "skip_context",
        "intra_inter_context")])
    I.define_impl("ContextWriter", [ctx.fn(n, "impl<'a> ContextWriter<'a>") for n in (
        "cdf_element_prob", "partition_gather_horz_alike", "partition_gather_vert_alike",
        "write_partition", "write_intra_mode_kf", "write_intra_mode", "write_intra_uv_mode",
        "write_cfl_alphas", "write_angle_delta", "fill_neighbours_ref_counts", "ref_count_ctx",
        "get_ref_frame_ctx_b0", "get_pred_ctx_brfarf2_or_arf", "get_pred_ctx_ll2_or_l3gld",
        "get_pred_ctx_last_or_last2", "get_pred_ctx_last3_or_gold", "get_pred_ctx_brf_or_arf2",
        "get_comp_mode_ctx", "get_comp_ref_type_ctx", "write_ref_frames", "write_compound_mode",
        "write_inter_mode", "write_drl_mode", "write_mv", "write_skip", "get_segment_pred",
        "neg_interleave", "write_segmentation", "write_is_inter")])
    I.define_impl("Block", [ctx.fn(n, "impl Block") for n in ("is_inter", "has_second_ref")])
    I.define_impl("CFLParams", [ctx.fn(n, "impl CFLParams") for n in (
        "joint_sign", "context", "index")])
    env = I.globals.vars

    def is_sqr(b):
        return b.w == b.h

    def cfl_allowed(b):  # src/partition.rs:174-177
        return int(b) <= 9
    H.BlockSizeV.is_sqr = is_sqr
    H.BlockSizeV.cfl_allowed = cfl_allowed
    env["BlockSize"] = type("BlockSizeNS", (), {"BLOCK_" + n: H.BlockSizeV(i)
                                                for i, n in enumerate(H.BLOCK_NAMES)})
    env["PredictionMode"] = type("PredictionModeNS", (), dict(PM))
    env["PartitionType"] = type("PartitionTypeNS", (), {n: i for i, n in enumerate((
        "PARTITION_NONE", "PARTITION_HORZ", "PARTITION_VERT", "PARTITION_SPLIT",
        "PARTITION_HORZ_A", "PARTITION_HORZ_B", "PARTITION_VERT_A", "PARTITION_VERT_B",
        "PARTITION_HORZ_4", "PARTITION_VERT_4", "PARTITION_INVALID"))})
    env["ReferenceMode"] = type("ReferenceModeNS", (), {"SINGLE": 0, "COMPOUND": 1, "SELECT": 2})
    env["MvSubpelPrecision"] = type("MvSubpelNS", (), {
        "MV_SUBPEL_NONE": -1, "MV_SUBPEL_LOW_PRECISION": 0, "MV_SUBPEL_HIGH_PRECISION": 1})
    env["MvJointType"] = type("MvJointNS", (), {
        "MV_JOINT_ZERO": 0, "MV_JOINT_HNZVZ": 1, "MV_JOINT_HZVNZ": 2, "MV_JOINT_HNZVNZ": 3})
    for i, n in enumerate(REF_NAMES):
        env[n] = RefT(i)
    for i, n in enumerate(("CFL_SIGN_ZERO", "CFL_SIGN_NEG", "CFL_SIGN_POS")):
        env[n] = i
    env["Block"] = RI.StructType("Block")
    env["CFLParams"] = RI.StructType("CFLParams")
    env["NMVComponent"] = RI.StructType("NMVComponent")
    return I


def mode_fields():
    """CDFContext's mode-info fields as CDFContext::new copies them"""
    em = T.strip_comments(open(os.path.join(REF, "entropymode.rs")).read())
    ctx = T.strip_comments(open(os.path.join(REF, "context.rs")).read())
    stat = {n: st for n, st, _, _ in M.FAMILIES}

    def typed(v, leaf=list):
        if isinstance(v, list) and v and isinstance(v[0], list):
            return [typed(x, leaf) for x in v]
        return leaf(E.u16(x) for x in v)
    f = {}
    for field, fam in MODE_FIELDS:
        if fam is not None:
            f[field] = typed(M.const_or_static(em, stat[fam]),
                             Tracked if fam == "PARTITION" else list)
    body = T.static_text(ctx, "default_nmv_context")
    comps = []
    for c in body.split("NMVComponent")[1:]:
        comps.append(RI.Struct("NMVComponent", {
            n: typed(M.field_value(c, n)) for n, _, _ in M.MV_FIELDS}))
    f["nmv_context"] = RI.Struct("NMVContext", {
        "joints_cdf": typed(M.field_value(body, "joints_cdf")), "comps": comps})
    return f


def walk(v, fn):
    if isinstance(v, list) and v and isinstance(v[0], list):
        for x in v:
            walk(x, fn)
    else:
        fn(v)


def cdf_lists(fc):
    """every CDF (innermost list) of the combined layout, in flat order"""
    out = []
    for n in E.FLAT_ORDER:
        walk(fc[n], out.append)
    for field, fam in MODE_FIELDS:
        if fam is not None:
            walk(fc[field], out.append)
        else:
            nm = fc[field]
            out.append(nm.joints_cdf)
            for c in nm.comps:
                for n, _, _ in M.MV_FIELDS:
                    walk(getattr(c, n), out.append)
    return out


class Rec:
    """The Writer the reference's methods see: records, then forwards to
    WriterBase<WriterEncoder>."""

    def __init__(self, I, lists):
        self.I, self.w = I, E.new_writer()
        self.idmap, o = {}, 0
        for l in lists:
            self.idmap[id(l)] = o
            o += len(l)
        self.total = o
        self.ops = []
        self.src = 0

    def _where(self, cdf):
        cdf = RI.deref(cdf)
        if isinstance(cdf, RI.Slice):
            return self.idmap[id(cdf.base)] + cdf.start, len(cdf)
        return self.idmap[id(cdf)], len(cdf)

    def symbol_with_update(self, s, cdf):
        off, ln = self._where(cdf)
        self.ops.append((self.src, 0, off, ln, int(s), 0))
        E.call(self.I, self.w, "symbol_with_update", s, cdf)

    def symbol(self, s, cdf):  # the frame-edge partition symbol only
        touched = Tracked.log  # cleared before write_partition: the gather's 12 reads
        src = touched[-1][0]
        assert len(touched) == 12 and all(t[0] is src for t in touched)
        idx = {t[1] for t in touched}
        # vert_alike reads PARTITION_VERT_4 (entry 9), horz_alike PARTITION_HORZ (entry 0)
        assert (9 in idx) != (0 in idx)
        gather = 1 if 9 in idx else 2
        self.ops.append((self.src, 1, self.idmap[id(src)], len(src), int(s), gather))
        E.call(self.I, self.w, "symbol", s, cdf)

    def bit(self, b):
        self.ops.append((self.src, 2, int(b), 0, 0, 0))
        E.call(self.I, self.w, "bit", b)

    def literal(self, bits, s):
        for k in reversed(range(int(bits))):
            self.ops.append((self.src, 2, (int(s) >> k) & 1, 0, 0, 0))
        E.call(self.I, self.w, "literal", bits, s)

    def write_golomb(self, level):
        x = int(level) + 1
        n = x.bit_length()
        for _ in range(n - 1):
            self.ops.append((self.src, 2, 0, 0, 0, 0))
        for k in reversed(range(n)):
            self.ops.append((self.src, 2, (x >> k) & 1, 0, 0, 0))
        E.call(self.I, self.w, "write_golomb", level)


class Cycle:
    def __init__(self, items, rng):
        self.items = list(items)
        rng.shuffle(self.items)
        self.i = 0

    def next(self):
        v = self.items[self.i % len(self.items)]
        self.i += 1
        return v


def mv_diff(rng, cls, precision):
    """a component difference of MV class cls"""
    lo = 1 if cls == 0 else (2 << (cls + 2)) + 1
    hi = (2 << (cls + 3)) if cls else 16
    if cls == 10:
        hi = 1 << 14
    m = int(rng.integers(lo, hi + 1))
    if precision < 0:
        m = min(max((m + 7) // 8 * 8, (lo + 7) // 8 * 8), hi // 8 * 8)
    elif precision == 0:
        m = min(max((m + 1) // 2 * 2, (lo + 1) // 2 * 2), hi // 2 * 2)
    return -m if rng.random() < 0.5 else m


class Gen:
    def __init__(self, rng):
        self.rng = rng
        self.I = make()
        self.inter = Cycle(range(14, 20), rng)
        self.comp = Cycle(range(20, 28), rng)
        self.single_ref = Cycle(range(1, 8), rng)
        self.comp_ref = Cycle([(a, b) for a in range(1, 5) for b in range(5, 8)], rng)
        self.intra = Cycle(range(13), rng)
        self.chroma = Cycle(list(range(14)) + [13] * 8, rng)
        self.cfl_js = Cycle(range(8), rng)
        self.mvcls = Cycle(range(11), rng)
        self.joint = Cycle([1, 2, 3, 3, 0], rng)
        self.nf = Cycle([0, 1, 2, 3, 4, 5, 2, 3, 4], rng)
        self.jobs, self.ops, self.cases, self.tile_dims = [], [], [], []
        self.tile_bytes, self.bytes, self.finals, self.inits = [], [], [], []
        self.seg_stored = []
        self.lv_jobs, self.lv_coeffs = [], []

    def rand_block(self, prm, lg):
        """a leaf's decision: a job row without position"""
        rng = self.rng
        j = [0] * NF
        j[F["bsize"]] = BLOCK_OF_LG[lg]
        j[F["skip"]] = int(rng.random() < 0.3)
        j[F["seg_idx"]] = int(rng.integers(0, prm["last_active"] + 1)) if prm["seg"] else 0
        precision = -1 if prm["force_int"] else (1 if prm["allow_hp"] else 0)
        r = rng.random()
        # intra_tx_cdf is outside the combined table: with coefficients, intra leaves
        # stay at the sizes whose transform has one type (32x32 and up)
        if prm["frame_type"] == 0 or (r < 0.25 and lg >= prm.get("intra_min_lg", 3)):
            lm = self.intra.next()
            cm = self.chroma.next()
            if cm == 13 and lg == 6:
                cm = self.intra.next()
            j[F["luma_mode"]], j[F["chroma_mode"]] = lm, cm
            j[F["ref0"]], j[F["ref1"]] = 0, 8
            if cm == 13:
                js = self.cfl_js.next()
                j[F["cfl_joint_sign"]] = js
                sg = ((js + 1) // 3, (js + 1) % 3)
                j[F["cfl_scale_u"]] = int(rng.integers(1, 17)) if sg[0] else 0
                j[F["cfl_scale_v"]] = int(rng.integers(1, 17)) if sg[1] else 0
            return j
        compound = prm["reference_mode"] != 0 and r < 0.6
        lm = self.comp.next() if compound else self.inter.next()
        rf = self.comp_ref.next() if compound else (self.single_ref.next(), 8)
        nf = self.nf.next()
        if lm == PM["NEW_NEWMV"]:
            nf = max(nf, 2)
        if lm in (PM["NEAR1MV"], PM["NEAR2MV"]):
            nf = max(nf, lm - PM["NEAR0MV"] + 2)
        if lm in (PM["NEAR_NEARMV"], PM["NEAR_NEWMV"], PM["NEW_NEARMV"]):
            nf = max(nf, 2)
        j[F["luma_mode"]] = j[F["chroma_mode"]] = lm
        j[F["ref0"]], j[F["ref1"]] = rf
        j[F["num_mv_found"]] = nf
        for k in range(4):
            j[F["weight0"] + k] = int(rng.integers(0, 1280)) if k < nf else 0
        # mode_context as find_mvrefs forms it (src/context.rs:2805-2830): newmv 0..5,
        # GLOBALMV bit 3, refmv 0..5 from bit 4
        j[F["mode_context"]] = int(rng.integers(0, 6)) | int(rng.integers(0, 2)) << 3 | \
            int(rng.integers(0, 6)) << 4
        rm = [(int(rng.integers(-64, 64)) * 8, int(rng.integers(-64, 64)) * 8) if nf else (0, 0)
              for _ in range(2)]
        mvs = [rm[0], rm[1] if compound else (0, 0)]
        for k, on in ((0, lm in (PM["NEWMV"], PM["NEW_NEWMV"], PM["NEW_NEARESTMV"])),
                      (1, lm in (PM["NEW_NEWMV"], PM["NEAREST_NEWMV"]))):
            if on:
                jt = self.joint.next()
                dr = mv_diff(rng, self.mvcls.next(), precision) if jt in (2, 3) else 0
                dc = mv_diff(rng, self.mvcls.next(), precision) if jt in (1, 3) else 0
                mvs[k] = (rm[k][0] + dr, rm[k][1] + dc)
        for k in range(2):
            j[F["mv0_row"] + 2 * k], j[F["mv0_col"] + 2 * k] = mvs[k]
            j[F["ref_mv0_row"] + 2 * k], j[F["ref_mv0_col"] + 2 * k] = rm[k]
        return j

    def tree(self, x, y, lg, cols, rows, minlg, out):
        """the coding-order node / leaf list of encode_partition_topdown"""
        if x >= cols or y >= rows:  # src/encoder.rs:2399-2401
            return
        n4 = 1 << (lg - 2)
        must = x + n4 > cols or y + n4 > rows
        split = lg > minlg and (must or self.rng.random() < 0.5)
        if must and not split:
            split = True
        out.append(("node", x, y, lg, 3 if split else 0))
        if split:
            h = n4 // 2
            for dy in (0, h):
                for dx in (0, h):
                    self.tree(x + dx, y + dy, lg - 1, cols, rows, minlg, out)
        else:
            out.append(("leaf", x, y, lg, 0))

    def code_block(self, cw, w, fi, prm, j, bo, bs):
        """the call order of encode_block_pre_cdef / encode_block_post_cdef"""
        I, bl = self.I, cw.bc.blocks
        c = lambda name, *a: E.call(I, cw, name, *a)
        lm, cm = j[F["luma_mode"]], j[F["chroma_mode"]]
        skip = bool(j[F["skip"]])
        bl.set_segmentation_idx(bo, bs, j[F["seg_idx"]])  # src/encoder.rs:2523
        bl.set_skip(bo, bs, skip)  # :1450
        c("write_skip", w, bo, skip)  # :1463
        if prm["seg"]:  # :1464-1475 (update_map, preskip false)
            c("write_segmentation", w, bo, bs, skip, RI.TInt(prm["last_active"], "u8"))
        bl.set_block_size(bo, bs)  # :1504-1507
        bl.set_mode(bo, bs, lm)
        bl.set_ref_frames(bo, bs, (j[F["ref0"]], j[F["ref1"]]))
        is_inter = lm >= PM["NEARESTMV"]
        if prm["frame_type"] == 1:  # :1519
            c("write_is_inter", w, bo, is_inter)
            if is_inter:
                c("fill_neighbours_ref_counts", bo)
                c("write_ref_frames", w, fi, bo)
                ctx = usz(j[F["mode_context"]])
                if lm >= PM["NEAREST_NEARESTMV"]:
                    c("write_compound_mode", w, lm, ctx)
                else:
                    c("write_inter_mode", w, lm, ctx)
                nf = j[F["num_mv_found"]]
                wt = [j[F["weight0"] + k] for k in range(4)]
                if lm in (PM["NEWMV"], PM["NEW_NEWMV"]):  # :1534-1551, ref_mv_idx = 0
                    assert lm != PM["NEW_NEWMV"] or nf >= 2
                    for idx in range(2):
                        if nf > idx + 1:
                            drl = 0 > idx
                            c("write_drl_mode", w, drl, usz(int(wt[idx] < 640) + int(wt[idx + 1] < 640)))
                            if not drl:
                                break
                prec = -1 if prm["force_int"] else (1 if prm["allow_hp"] else 0)  # :1559-1565
                mvs = [H.motion_vector(j[F["mv0_row"] + 2 * k], j[F["mv0_col"] + 2 * k]) for k in range(2)]
                rms = [H.motion_vector(j[F["ref_mv0_row"] + 2 * k], j[F["ref_mv0_col"] + 2 * k])
                       for k in range(2)]
                if lm in (PM["NEWMV"], PM["NEW_NEWMV"], PM["NEW_NEARESTMV"]):  # :1567-1572
                    c("write_mv", w, mvs[0], rms[0], prec)
                if lm in (PM["NEW_NEWMV"], PM["NEAREST_NEWMV"]):  # :1573-1577
                    c("write_mv", w, mvs[1], rms[1], prec)
                has_near = PM["NEAR0MV"] <= lm <= PM["NEAR2MV"] or lm in (
                    PM["NEAR_NEARMV"], PM["NEAR_NEWMV"], PM["NEW_NEARMV"])
                if has_near:  # :1579-1602
                    rmi = lm - PM["NEAR0MV"] + 1 if PM["NEAR0MV"] <= lm <= PM["NEAR2MV"] else 1
                    if lm != PM["NEAR0MV"]:
                        assert nf > rmi
                    for idx in range(1, 3):
                        if nf > idx + 1:
                            drl = rmi > idx
                            c("write_drl_mode", w, drl, usz(int(wt[idx] < 640) + int(wt[idx + 1] < 640)))
                            if not drl:
                                break
            else:
                c("write_intra_mode", w, bs, lm)  # :1620
        else:
            c("write_intra_mode_kf", w, bo, lm)  # :1623
        if not is_inter:  # :1626-1639 (bsize >= 8x8, has_chroma holds)
            if 1 <= lm <= 8:
                c("write_angle_delta", w, RI.TInt(0, "i8"), lm)
            c("write_intra_uv_mode", w, cm, lm, bs)
            if cm == 13:
                js = j[F["cfl_joint_sign"]]
                cfl = RI.Struct("CFLParams", {
                    "sign": [(js + 1) // 3, (js + 1) % 3],
                    "scale": [RI.TInt(j[F["cfl_scale_u"]], "u8"), RI.TInt(j[F["cfl_scale_v"]], "u8")]})
                c("write_cfl_alphas", w, cfl)
            if 1 <= cm <= 8:
                c("write_angle_delta", w, RI.TInt(0, "i8"), cm)

    def case(self, name, prm, tiles, minlg=3, coeffs=False):
        t0 = time.time()
        I, rng = self.I, self.rng
        q = int(rng.integers(0, 4))
        job0, op0, lv0, tile0 = len(self.jobs), len(self.ops), len(self.lv_jobs), len(self.tile_dims)
        fi = RI.Struct("FrameInvariants", {"reference_mode": 2 if prm["reference_mode"] else 0})
        for ti, (cols, rows) in enumerate(tiles):
            self.tile_dims.append((cols, rows))
            fc = E.cdf_fields(q)
            fc.update(mode_fields())
            lists = cdf_lists(fc)
            if ti == 0:
                self.inits.append([int(v) for l in lists for v in l])
            w = Rec(I, lists)
            assert w.total == M.coeff_total() + len(M.mode_tables()[1]), w.total
            bc = RI.Struct("BlockContext", {
                "above_coeff_context": [[RI.TInt(0, "u8")] * 1024 for _ in range(3)],
                "left_coeff_context": [[RI.TInt(0, "u8")] * 16 for _ in range(3)],
                "above_partition_context": [RI.TInt(0, "u8")] * 512,
                "left_partition_context": [RI.TInt(0, "u8")] * 8,
                "left_tx_context": [RI.TInt(0, "u8")] * 16,
                "blocks": Blocks(cols, rows)})
            cw = RI.Struct("ContextWriter", {"bc": bc, "fc": RI.Struct("CDFContext", fc)})
            for sby in range((rows + 15) // 16):
                E.call(I, bc, "reset_left_contexts")
                for sbx in range((cols + 15) // 16):
                    order = []
                    self.tree(sbx * 16, sby * 16, 6, cols, rows, minlg, order)
                    for what, x, y, lg, p in order:
                        bo, bs = tile_bo(x, y), H.BlockSizeV(BLOCK_OF_LG[lg])
                        w.src = len(self.jobs) - job0
                        if what == "node":
                            j = [0] * NF
                            j[F["kind"]], j[F["tile"]], j[F["bx"]], j[F["by"]] = 1, ti, x, y
                            j[F["bsize"]], j[F["partition"]] = BLOCK_OF_LG[lg], p
                            self.jobs.append(j)
                            self.seg_stored.append(0)
                            Tracked.log.clear()
                            E.call(I, cw, "write_partition", w, bo, p, bs)  # src/encoder.rs:2490-2493
                            continue
                        j = self.rand_block(prm, lg)
                        j[F["tile"]], j[F["bx"]], j[F["by"]] = ti, x, y
                        self.jobs.append(j)
                        self.code_block(cw, w, fi, prm, j, bo, bs)
                        self.seg_stored.append(int(bc.blocks.index_any(bo).segmentation_idx))
                        if coeffs:
                            self.code_coeffs(cw, w, j, x, y, lg, lv0, job0)
                        # src/encoder.rs:2711-2717 (PARTITION_NONE: subsize = bsize)
                        E.call(I, bc, "update_partition_context", bo, bs, bs)
            b = E.call(I, w.w, "done")
            self.tile_bytes.append(len(b))
            self.bytes += [int(x) for x in b]
            self.finals.append([int(v) for l in lists for v in l])
            self.ops += w.ops
        self.cases.append((len(self.cases), job0, len(self.jobs) - job0, op0, len(self.ops) - op0,
                           prm["frame_type"], prm["reference_mode"], prm["force_int"],
                           prm["allow_hp"], prm["seg"], prm["last_active"], tile0, len(tiles), q,
                           lv0, len(self.lv_jobs) - lv0, int(coeffs)))
        print("%s: %d jobs, %d ops, %.0f s" % (name, len(self.jobs) - job0, len(self.ops) - op0,
                                               time.time() - t0), flush=True)

    def code_coeffs(self, cw, w, j, x4, y4, lg, lv0, job0):
        """4:2:0 transform blocks of a leaf as gen_ec_ref.py codes them: a skip
        leaf resets its contexts (src/encoder.rs:1501-1503), a coded one writes
        luma, U, V through write_coeffs_lv_map"""
        I, rng = self.I, self.rng
        bo = tile_bo(x4, y4)
        rel = len(self.jobs) - 1 - job0  # the leaf's mode job
        if j[F["skip"]]:
            E.call(I, cw.bc, "reset_skip_context", bo, H.BlockSizeV(BLOCK_OF_LG[lg]), usz(1), usz(1))
            self.lv_jobs.append((1, 0, x4, y4, 0, 0, 0, lg, lg, 0, rel))
            return
        inter = j[F["luma_mode"]] >= 14
        mode = RI.TInt(j[F["luma_mode"]], "usize")
        for p in range(3):
            xd = 1 if p else 0
            plg = lg - xd
            tx = min(plg - 2, 4)
            cwid = min(4 << tx, 32)
            co = E.rand_coeffs(rng, cwid, 6.0 if p == 0 else 3.0)
            cin = [RI.TInt(int(v), "i32") for v in co]
            w.src = -(len(self.lv_jobs) - lv0) - 1
            E.call(I, cw, "write_coeffs_lv_map", w, usz(p), bo, RI.Slice(cin), mode, E.TxSq(tx),
                   usz(0), H.BlockSizeV(BLOCK_OF_LG[plg]) if plg >= 3 else H.BlockSizeV(0),
                   usz(xd), usz(xd), True)
            self.lv_jobs.append((0, p, x4, y4, tx, 0, int(inter), plg, plg, len(self.lv_coeffs), rel))
            self.lv_coeffs += [int(v) for v in co]


def coverage(g):
    """Assert what the vectors must reach; print what they do not."""
    jobs = np.array(g.jobs, np.int64)
    ops = np.array(g.ops, np.int64)
    offs, vals = M.mode_tables()
    blk = jobs[jobs[:, F["kind"]] == 0]
    lm = blk[:, F["luma_mode"]]
    sym = ops[ops[:, 1] == 0]
    fam_of = sorted((o, n) for n, o in offs.items())
    hit = {}
    for o in sym[:, 2]:
        if o >= offs["PARTITION"]:
            n = [nm for oo, nm in fam_of if oo <= o][-1]
            hit.setdefault(n, set()).add(int(o))
    for n in offs:
        assert n in hit, "family %s never coded" % n
    assert set(range(14, 28)) <= set(lm.tolist()), "inter / compound modes"
    single = blk[(lm >= 14) & (lm < 20)]
    assert set(range(1, 8)) <= set(single[:, F["ref0"]].tolist()), "single refs"
    comp = blk[lm >= 20]
    assert set(range(1, 5)) <= set(comp[:, F["ref0"]].tolist()), "compound forward refs"
    assert set(range(5, 8)) <= set(comp[:, F["ref1"]].tolist()), "compound backward refs"
    cls = sym[(sym[:, 3] == 12) & (sym[:, 2] >= offs["PARTITION"])]
    assert set(range(11)) <= set(cls[:, 4].tolist()), "mv classes"
    jt = sym[sym[:, 2] == offs["MV_JOINTS"]]
    assert set(range(4)) <= set(jt[:, 4].tolist()), "mv joints"
    cases = np.array(g.cases)
    assert {(0, 0), (0, 1), (1, 0)} <= {(int(c[7]), int(c[8])) for c in cases if c[5] == 1}, "precisions"
    nf = blk[lm >= 14][:, F["num_mv_found"]]
    assert {2, 3, 4} <= set(nf.tolist()), "drl stack sizes"
    drl = sym[(sym[:, 2] >= offs["DRL"]) & (sym[:, 2] < offs["DRL"] + 9)]
    assert {offs["DRL"], offs["DRL"] + 3, offs["DRL"] + 6} <= set(drl[:, 2].tolist()), "drl contexts"
    for ft in (0, 1):
        sel = np.zeros(len(jobs), bool)
        for c in cases:
            if c[5] == ft:
                sel[c[1]:c[1] + c[2]] = True
        m = jobs[sel & (jobs[:, F["kind"]] == 0)][:, F["luma_mode"]]
        assert set(range(13)) <= set(m.tolist()), "intra modes, frame type %d" % ft
    cfl = blk[(lm < 14) & (blk[:, F["chroma_mode"]] == 13)]
    assert set(range(8)) <= set(cfl[:, F["cfl_joint_sign"]].tolist()), "cfl sign pairs"
    segc = [c for c in cases if c[9]]
    assert segc, "segmentation"
    sj = np.concatenate([jobs[c[1]:c[1] + c[2]] for c in segc])
    sj = sj[sj[:, F["kind"]] == 0]
    assert {0, 1, 2} <= set(sj[:, F["seg_idx"]].tolist()) and sj[:, F["skip"]].any(), "segments"
    edge = ops[ops[:, 1] == 1]
    assert {1, 2} <= set(edge[:, 5].tolist()), "edge partition forms"
    silent = [i for c in cases for i in range(c[2]) if jobs[c[1] + i, F["kind"]] == 1 and
              not ((ops[c[3]:c[3] + c[4], 0] == i).any())]
    assert silent, "no-symbol corner"
    assert any(c[12] > 1 for c in cases), "second tile"
    assert any(c[16] for c in cases), "interleaved case"
    # information: (family, context) pairs of the mode families never coded
    missing = []
    for n, st, shape, e in M.FAMILIES:
        cnt = M.count(shape, 1)
        if n == "MV_COMP":
            continue
        for k in range(cnt):
            if offs[n] + k * e not in hit.get(n, ()):
                missing.append((n, k))
    print("unreached (family, context): %d" % len(missing))
    by = {}
    for n, k in missing:
        by.setdefault(n, []).append(k)
    for n, ks in by.items():
        print("  %s: %s" % (n, ks))


def main():
    t0 = time.time()
    rng = np.random.default_rng(0xEC0DE)
    g = Gen(rng)
    base = {"frame_type": 1, "reference_mode": 1, "force_int": 0, "allow_hp": 0, "seg": 0,
            "last_active": 0}
    g.case("inter select low seg, 2 tiles", dict(base, seg=1, last_active=2), [(32, 32), (32, 32)])
    g.case("inter single high, edge", dict(base, reference_mode=0, allow_hp=1), [(34, 26)])
    g.case("inter select integer, col edge", dict(base, force_int=1), [(24, 32)])
    g.case("key, edge", dict(base, frame_type=0), [(34, 26)])
    g.case("key seg", dict(base, frame_type=0, seg=1, last_active=2), [(16, 32)])
    g.case("inter select low, interleaved", dict(base, intra_min_lg=5), [(32, 16)], minlg=4, coeffs=True)
    coverage(g)
    np.savez_compressed(
        OUT, jobs=np.array(g.jobs, np.int32), ops=np.array(g.ops, np.int32),
        cases=np.array(g.cases, np.int32), tile_dims=np.array(g.tile_dims, np.int32),
        tile_bytes=np.array(g.tile_bytes, np.int32), bytes=np.array(g.bytes, np.uint8),
        final_cdf=np.array(g.finals, np.uint16), init_cdf=np.array(g.inits, np.uint16),
        seg_stored=np.array(g.seg_stored, np.int32),
        lv_jobs=np.array(g.lv_jobs, np.int32).reshape(-1, 11),
        lv_coeffs=np.array(g.lv_coeffs, np.int32))
    print("wrote %s (%d bytes) in %.0f s" % (OUT, os.path.getsize(OUT), time.time() - t0))


if __name__ == "__main__":
    main()

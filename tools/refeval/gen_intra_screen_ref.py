"""Golden vectors for the general get_intra_edges and the intra-mode
screening, produced by RUNNING the reference's own Rust function text
(rsinterp.py) -- needs the reference checkout that gen_golden_ref.py reads:

    python tools/refeval/gen_intra_screen_ref.py

Functions evaluated: has_top_right / has_bottom_left (src/recon_intra.rs:
174-243, 376-458) with their tables, supersample_chroma_bsize and
get_intra_edges (src/partition.rs:459-693), PredictionMode::predict_intra
(src/predict.rs:202-241) over the native Intra trait, get_satd_ref
(src/dist.rs:197-328).  The screening's two sorts and merge (src/rdo.rs:
1086-1127) are restated below in Python over those evaluated SATDs: the
interpreter is not taken through rdo_mode_decision's ContextWriter and
FrameInvariants.  Only the resulting numbers are written
(tests/golden/ref_intra_screen.npz); tests/test_intra_screen.py checks
tests/intra_screen_ref.py against them.
"""
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402
from gen_cfl_ref import PAD, plane, tile_bo, tx_size_of, usz  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "ref_intra_screen.npz")
SIZES = list(range(13))  # BLOCK_4X4 .. BLOCK_64X64: the squares and the 2:1 / 1:2 sizes
FORMATS = ((0, 0), (1, 0), (1, 1))  # 4:4:4, 4:2:2, 4:2:0
RAV1E_INTRA_MODES = [0, 2, 1, 9, 11, 10, 12, 3, 4, 5, 6, 7, 8]  # src/predict.rs:32-46


def interp():
    I = G.make_interp()
    I.release = True
    G.intra_env(I)
    rin = RI.Source(G.REF + "recon_intra.rs")
    # the file keeps C declarations in block comments, one with an open brace
    rin.src = re.sub(r"/\*.*?\*/", " ", rin.src, flags=re.S)
    I.sources.append(rin)
    I.globals.vars["MAX_MIB_SIZE_LOG2"] = usz(5)  # src/context.rs: MAX_SB_SIZE_LOG2 - MI_SIZE_LOG2
    # TxSize::width_mi / height_mi (src/transform/mod.rs) on the host value
    G.TxSizeV.width_mi = lambda self: usz(self.w >> 2)
    G.TxSizeV.height_mi = lambda self: usz(self.h >> 2)
    for n in ("has_top_right", "has_bottom_left"):
        G.F(I, n, "recon_intra.rs")
    G.F(I, "supersample_chroma_bsize", "partition.rs")
    return I


def plane_block(b, xdec, ydec):
    """The partition's block in a plane: supersample_chroma_bsize, decimated."""
    bs = H.BlockSizeV(b)
    return max(4, bs.w >> xdec), max(4, bs.h >> ydec)


def avail_tx_sizes(b, xdec, ydec):
    """The transform sizes the availability is enumerated for: the plane
    block itself and its half per axis (2 x 2 offsets where both halve)."""
    w, h = plane_block(b, xdec, ydec)
    out = [(w, h)]
    half = (max(4, w // 2), max(4, h // 2))
    if half != (w, h):
        out.append(half)  # always a TxSize: the blocks are at most 4:1 in a plane
    return out


def avail_cases():
    """Every (bsize, mi_col, mi_row, xdec, ydec, tx w, tx h, row_off, col_off)
    the availability is recorded for; the test enumerates the same set."""
    for b in SIZES:
        bs = H.BlockSizeV(b)
        for xdec, ydec in FORMATS:
            pw, ph = plane_block(b, xdec, ydec)
            for tw, th in avail_tx_sizes(b, xdec, ydec):
                for mi_row in range(0, 16, bs.h // 4):
                    for mi_col in range(0, 16, bs.w // 4):
                        for by in range(ph // th):
                            for bx in range(pw // tw):
                                yield b, mi_col, mi_row, xdec, ydec, tw, th, by * (th // 4), \
                                    bx * (tw // 4)


def gen_avail(I, out):
    htr, hbl = I.globals.vars["has_top_right"], I.globals.vars["has_bottom_left"]
    ss = I.globals.vars["supersample_chroma_bsize"]
    rows = []
    t0 = time.time()
    for b, mi_col, mi_row, xdec, ydec, tw, th, row_off, col_off in avail_cases():
        sb = ss(H.BlockSizeV(b), usz(xdec), usz(ydec))
        bo = tile_bo(mi_col, mi_row)
        ts = tx_size_of(tw, th)
        tr = bl = 0
        for k in range(4):
            a0, a1 = bool(k & 1), bool(k & 2)
            tr |= int(bool(htr(sb, bo, a0, a1, ts, usz(row_off), usz(col_off), usz(xdec),
                               usz(ydec)))) << k
            bl |= int(bool(hbl(sb, bo, a0, a1, ts, usz(row_off), usz(col_off), usz(xdec),
                               usz(ydec)))) << k
        rows.append((b, mi_col, mi_row, xdec, ydec, tw, th, row_off, col_off, tr, bl))
        if len(rows) % 2000 == 0:
            print("availability: %d positions, %.0f s" % (len(rows), time.time() - t0), flush=True)
    # bit k of tr: has_top_right(top = k & 1, right = k & 2); of bl:
    # has_bottom_left(bottom = k & 1, left = k & 2)
    out["avail"] = np.array(rows, np.uint8)
    print("availability: %d positions" % len(rows), flush=True)


def rand_plane(rng, w, h, bd):
    maxv = (1 << bd) - 1
    img = rng.integers(0, maxv + 1, (h, w))
    img[h // 3:h // 2, w // 4:w // 2] = maxv  # saturated regions
    img[h // 2:h // 2 + 6, 0:w // 5] = 0
    return img


def tile_region(pl, rect):
    x, y, w, h = rect
    return pl.region(RI.Struct("Area::Rect", {"x": x, "y": y, "width": w, "height": h}))


def po_struct(x, y):
    return RI.Struct("PlaneOffset", {"x": RI.TInt(x, "isize"), "y": RI.TInt(y, "isize")})


def edges_of(I, region, b, bo_x, bo_y, bx, by, po_x, po_y, tw, th, bd, mode):
    e = I.globals.vars["get_intra_edges"](
        region, tile_bo(bo_x, bo_y), usz(bx), usz(by), H.BlockSizeV(b), po_struct(po_x, po_y),
        tx_size_of(tw, th), usz(bd), None if mode < 0 else G.PModeV(mode))
    return np.array([int(v) for v in e.array[:257]], np.int64)


# one mode of each needs_* class (src/partition.rs:545-556): left + top (H /
# V drop one), top-left (D135), top-right (D45), bottom-left (D207), the
# PAETH demotion, and the DC / CfL rule
EDGE_MODES = (-1, 3, 7, 4, 12, 0, 13, 1, 2, 8)


def gen_edges(I, rng, out):
    """get_intra_edges over the blocks of a 88 x 88 luma tile (neither a
    multiple of 64 nor of 32) at luma (8, 8) of a 104 x 104 frame, per format
    and bit depth: every transform block of a spread of partitions."""
    LW, LH, TX0, TY0, TW, TH = 104, 104, 8, 8, 88, 88
    out["edge_tile"] = np.array([TX0, TY0, TW, TH], np.int32)
    meta, res = [], []
    t0 = time.time()
    k = 0
    for pi, (bd, (xdec, ydec)) in enumerate(((8, (0, 0)), (8, (1, 1)), (10, (1, 0)), (12, (1, 1)),
                                             (10, (0, 0)), (12, (1, 0)))):
        G.PModeV.pixel = G.prim(bd)
        pw_, ph_ = LW >> xdec, LH >> ydec
        img = rand_plane(rng, pw_, ph_, bd)
        full = np.pad(img, PAD, mode="edge")
        out["edge_plane%d" % pi] = full.astype(np.uint16)
        out["edge_plane%d_cfg" % pi] = np.array([bd, xdec, ydec, pw_, ph_], np.int32)
        pl = plane(full, bd, xdec, ydec)
        rw, rh = TW >> xdec, TH >> ydec
        region = tile_region(pl, (TX0 >> xdec, TY0 >> ydec, rw, rh))
        for b in SIZES:
            bs = H.BlockSizeV(b)
            pw, ph = plane_block(b, xdec, ydec)
            txs = [(pw, ph)]
            if b == 12 and (xdec, ydec) == (0, 0):
                txs = [(32, 32)]  # a 64x64 partition's four 32x32 chroma blocks at 4:4:4
            elif b in (9, 6, 5, 4) and pw >= 8 and ph >= 8:
                txs.append((pw // 2, ph // 2))
            # partition positions: the tile's corners and edges, and an
            # interior spread that walks the superblock's coding order
            step_x, step_y = bs.w // 4, bs.h // 4
            cols = list(range(0, TW // 4 - step_x + 1, step_x))
            rows_ = list(range(0, TH // 4 - step_y + 1, step_y))
            pos = [(c, r) for r in rows_ for c in cols]
            if len(pos) > 14:
                keep = {0, len(cols) - 1, len(pos) - len(cols), len(pos) - 1}
                keep |= set(int(v) for v in rng.choice(len(pos), 10, replace=False))
                pos = [pos[i] for i in sorted(keep)]
            for (bo_x, bo_y) in pos:
                # sub-8x8 chroma: the block with chroma is the odd one
                ox = bo_x | (1 if xdec and bs.w == 4 else 0)
                oy = bo_y | (1 if ydec and bs.h == 4 else 0)
                for (tw, th) in txs:
                    for by in range(ph // th):
                        for bx in range(pw // tw):
                            po_x = ((ox >> xdec) << 2) + bx * tw
                            po_y = ((oy >> ydec) << 2) + by * th
                            if po_x + tw > rw or po_y + th > rh:
                                continue
                            modes = (-1, EDGE_MODES[1 + k % (len(EDGE_MODES) - 1)])
                            for mode in modes:
                                e = edges_of(I, region, b, ox, oy, bx, by, po_x, po_y, tw, th, bd,
                                             mode)
                                meta.append((pi, b, ox, oy, bx, by, po_x, po_y, tw, th, mode))
                                res.append(e)
                            k += 1
        print("edges: plane %d (bd %d, dec %d%d): %d cases, %.0f s" % (
            pi, bd, xdec, ydec, len(meta), time.time() - t0), flush=True)
    out["edge_meta"] = np.array(meta, np.int32)
    out["edge_out"] = np.array(res, np.uint16)


def select(satds, row, num):
    """src/rdo.rs:1086-1127 restated: stable sort by SATD, stable descending
    sort by probability, the merge, the truncation."""
    order = sorted(range(13), key=lambda k: satds[k])
    z, probs_all = 32768, []
    for a in row[:13]:
        probs_all.append((z - int(a)) & 0xffff)
        z = int(a)
    porder = sorted(range(13), key=lambda k: 0xffff ^ probs_all[RAV1E_INTRA_MODES[k]])
    modes = [RAV1E_INTRA_MODES[k] for k in porder[:num // 2]]
    for k in order[:num]:
        if RAV1E_INTRA_MODES[k] not in modes:
            modes.append(RAV1E_INTRA_MODES[k])
    return modes[:num]


def perturb(rng, row):
    """A valid adapted row: 13 strictly decreasing values in (0, 32768), the
    terminating 0 and the adaptation counter."""
    cuts = np.sort(rng.choice(np.arange(1, 32768), 13, replace=False))[::-1]
    r = np.array(row).copy()
    r[:13] = cuts
    return r


def gen_screen(I, rng, out, cdf_all, kf_off, ym_off):
    """The 13 SATDs of every case by the reference's get_intra_edges /
    predict_intra / get_satd_ref, and the mode list."""
    satd_ref = G.F(I, "get_satd_ref")
    LW, LH = 96, 80
    TILE = (8, 8, 88, 72)
    out["scr_tile"] = np.array(TILE, np.int32)
    size_group = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3]
    meta, satds, modes, rows = [], [], [], []
    t0 = time.time()
    for pi, bd in enumerate((8, 10, 12)):
        G.PModeV.pixel = G.prim(bd)
        I.globals.vars["T"] = G.prim(bd)
        rec = rand_plane(rng, LW, LH, bd)
        # a source near the reconstruction shifted, so the modes differ in cost
        src = np.clip(np.roll(rec, (1, 2), (0, 1)) + rng.integers(-6, 7, rec.shape), 0,
                      (1 << bd) - 1)
        fr, fs = np.pad(rec, PAD, mode="edge"), np.pad(src, PAD, mode="edge")
        out["scr_rec%d" % pi], out["scr_src%d" % pi] = fr.astype(np.uint16), fs.astype(np.uint16)
        for b in SIZES:
            if (b >= 9 and bd == 12) or (b >= 10 and bd == 10):
                continue  # the large blocks once or twice: the interpreter is slow
            bs = H.BlockSizeV(b)
            ts = tx_size_of(bs.w, bs.h)
            npos = 1 if b >= 9 else 2 if b >= 6 else 3
            cand = [(0, 0), (bs.w // 4, 0), (0, bs.h // 4), (bs.w // 4, bs.h // 4)]
            cand = [(x, y) for x, y in cand if 4 * x + bs.w <= TILE[2] and 4 * y + bs.h <= TILE[3]]
            for n in range(npos):
                bo_x, bo_y = cand[(n + b + pi) % len(cand)]
                prec, psrc = plane(fr.copy(), bd), plane(fs, bd)
                rreg, sreg = tile_region(prec, TILE), tile_region(psrc, TILE)
                po_x, po_y = 4 * bo_x, 4 * bo_y
                eb = I.globals.vars["get_intra_edges"](
                    rreg, tile_bo(bo_x, bo_y), usz(0), usz(0), bs, po_struct(po_x, po_y), ts,
                    usz(bd), None)
                trect = RI.Struct("TileRect", {"x": usz(TILE[0]), "y": usz(TILE[1]),
                                               "width": usz(TILE[2]), "height": usz(TILE[3])})
                area = RI.Struct("Area::BlockStartingAt", {"bo": tile_bo(bo_x, bo_y)._f["0"]})
                s13 = []
                for m in RAV1E_INTRA_MODES:
                    dst = rreg.subregion(area)
                    G.PModeV(m).predict_intra(trect, dst, ts, usz(bd), RI.Slice(
                        [RI.TInt(0, "i16")] * 2), RI.TInt(0, "i16"), eb, 0)
                    s13.append(int(satd_ref(sreg.subregion(area), dst, bs, usz(bd), 0,
                                            generics={"T": G.prim(bd)})))
                # frame type, CDF row (default or perturbed), mode count
                c = len(meta) // 2  # the case's number
                kf = (c % 2) == 0
                off = kf_off + 14 * ((c * 7) % 25) if kf else ym_off + 14 * size_group[b]
                row = np.array(cdf_all[off:off + 14])
                pert = (c % 3) == 1
                if pert:
                    row = perturb(rng, row)
                for num in (3, 7):
                    meta.append((pi, b, bo_x, bo_y, int(kf), off, int(pert), num))
                    satds.append(s13)
                    rows.append(row)
                    modes.append(select(s13, row, num) + [255] * 7)
                print("screen: bd %d %s at (%d, %d): %s, %.0f s" % (
                    bd, H.BLOCK_NAMES[b], bo_x, bo_y, s13, time.time() - t0), flush=True)
    out["scr_meta"] = np.array(meta, np.int32)
    out["scr_satd"] = np.array(satds, np.uint32)
    out["scr_row"] = np.array(rows, np.uint16)
    out["scr_modes"] = np.array([m[:7] for m in modes], np.uint8)


def main():
    I = interp()
    rng = np.random.default_rng(20261020)
    out = {}
    # the default rows of the combined table, from the committed generator's
    # output (rv_ec_mode_tables.h: numbers evaluated from the reference)
    hdr = open(os.path.join(G.ROOT, "rav1e_amd", "csrc", "rv_ec_mode_tables.h")).read()
    kf_off = int(re.search(r"#define RV_ECM_KF_Y (\d+)", hdr).group(1))
    ym_off = int(re.search(r"#define RV_ECM_Y_MODE (\d+)", hdr).group(1))
    base = int(re.search(r"#define RV_ECM_PARTITION (\d+)", hdr).group(1))
    body = hdr[hdr.index("RV_ECM_DEFAULT_CDF["):]
    vals = [int(v) for v in re.findall(r"\d+", body[body.index("{"):body.index("}")])]
    cdf_all = [0] * base + vals
    which = sys.argv[1:] or ["avail", "edges", "screen"]
    if os.path.exists(OUT):
        out.update(np.load(OUT))
    if "avail" in which:
        gen_avail(I, out)
    if "edges" in which:
        gen_edges(I, rng, out)
    if "screen" in which:
        gen_screen(I, np.random.default_rng(20261021), out, cdf_all, kf_off, ym_off)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

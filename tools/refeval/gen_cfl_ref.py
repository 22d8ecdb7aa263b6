"""Golden vectors for chroma from luma, produced by RUNNING the reference's
own Rust function text (rsinterp.py) -- needs the reference checkout that
gen_golden_ref.py reads:

    python tools/refeval/gen_cfl_ref.py

Functions evaluated: PredictionMode::predict_intra with UV_CFL_PRED
(src/predict.rs:202-241) over native::predict_intra_inner (:538-597), the
Intra trait's pred_cfl / _128 / _left / _top / _inner (:836-892) and
get_scaled_luma_q0 (:485-493); luma_ac (src/encoder.rs:1714-1755) with
BlockSize::subsampled_size / is_sub8x8 / sub8x8_offset (src/partition.rs:
245-312); rdo_cfl_alpha (src/rdo.rs:1261-1336) over those, get_intra_edges
(src/partition.rs:500-693) and sse_wxh (src/rdo.rs:286-335).  Only the
resulting numbers are written (tests/golden/ref_cfl.npz); tests/test_cfl.py
checks tests/cfl_ref.py against them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "ref_cfl.npz")
PAD = 8
ALLOWED = 10  # BLOCK_4X4 .. BLOCK_32X32: cfl_allowed (src/partition.rs:174-177)


def usz(v):
    return RI.TInt(int(v), "usize")


def px_type(bd):
    return "u8" if bd == 8 else "u16"


def plane(full, bd, xdec=0, ydec=0):
    """A plane of (h + 2 PAD) x (w + 2 PAD) with the visible area at PAD."""
    h, w = full.shape[0] - 2 * PAD, full.shape[1] - 2 * PAD
    pl = H.Plane.from_full(full, PAD, PAD, w, h, xdec, ydec)
    pl.data = [RI.TInt(int(v), px_type(bd)) for v in pl.data]
    return pl


def block_offset(x, y):
    """BlockOffset (src/context.rs:1276-1329) with with_offset and
    plane_offset."""
    return RI.Struct("BlockOffset", {
        "x": usz(x), "y": usz(y),
        "with_offset": lambda dx, dy: block_offset(x + int(RI.deref(dx)), y + int(RI.deref(dy))),
        "plane_offset": lambda cfg: RI.Struct("PlaneOffset", {
            "x": RI.TInt(x >> int(RI.deref(cfg).xdec) << 2, "isize"),
            "y": RI.TInt(y >> int(RI.deref(cfg).ydec) << 2, "isize")})})


def tile_bo(x, y):
    """TileBlockOffset (src/context.rs:1331-1360)."""
    bo = block_offset(x, y)
    return RI.Struct("TileBlockOffset", {
        "0": bo,
        "with_offset": lambda dx, dy: tile_bo(x + int(RI.deref(dx)), y + int(RI.deref(dy))),
        "plane_offset": lambda cfg: bo._f["plane_offset"](cfg)})


def interp():
    I = G.make_interp()
    I.release = True
    G.intra_env(I)
    enc = RI.Source(G.REF + "encoder.rs")
    I.sources.append(enc)
    part = G.src_of(I, "partition.rs")
    I.globals.vars["BLOCK_INVALID"] = _Invalid()
    # BlockSize's own methods, from the reference's text, on the host value
    for m in ("subsampled_size", "is_sub8x8", "sub8x8_offset", "cfl_allowed"):
        f = I.make_fn(part.fn(m, "impl BlockSize"), I.globals)
        setattr(H.BlockSizeV, m, (lambda self, *a, _f=f: _f(self, *a)))
    return I


class _Invalid:
    """BlockSize::BLOCK_INVALID: equal to nothing else."""

    def __repr__(self):
        return "BLOCK_INVALID"


def tx_size_of(w, h):
    for i in range(19):
        if (1 << G.TX_W_LOG2[i], 1 << G.TX_H_LOG2[i]) == (w, h):
            return G.TxSizeV(i)
    raise KeyError((w, h))


def gen_predict(I, rng, out):
    """predict_intra(UV_CFL_PRED) into a block at (x, y) of a tile at the
    plane's origin: x, y in {0, 32} give the four variants."""
    meta, edges, acs, outs, off = [], [], [], [], [0]
    sizes = [i for i in range(19) if max(G.TX_W_LOG2[i], G.TX_H_LOG2[i]) <= 5]
    assert len(sizes) == 14
    cfl = G.PModeV(13)
    k = 0
    for bd in (8, 10, 12):
        G.PModeV.pixel = G.prim(bd)
        maxv = (1 << bd) - 1
        amax = min(32767, maxv << 3)
        for tx in sizes:
            ts = G.TxSizeV(tx)
            w, h = ts.w, ts.h
            for rep in range(1 if bd == 12 and w * h > 256 else 2):
                variant = (k + rep) % 4
                alpha = [-16, -1, 0, 1, 7, 16, -9, 3][k % 8]
                kind = k % 3
                e = rng.integers(0, maxv + 1, 257) if kind == 0 else \
                    np.full(257, maxv if kind == 1 else 0)
                ac = rng.integers(-amax, amax + 1, w * h)
                ac[0] = amax if k & 1 else -amax
                x, y = (32 if variant & 1 else 0), (32 if variant & 2 else 0)
                full = np.zeros((64 + 2 * PAD, 64 + 2 * PAD), np.int64)
                dst = plane(full, bd)
                region = G.region_at(dst, x, y)
                rect = RI.Struct("TileRect", {"x": usz(0), "y": usz(0), "width": usz(64),
                                              "height": usz(64)})
                eb = G.AlignedArray([RI.TInt(int(v), px_type(bd)) for v in e])
                acl = [RI.TInt(int(v), "i16") for v in ac] + \
                    [RI.TInt(0, "i16")] * (32 * 32 - w * h)
                cfl.predict_intra(rect, region, ts, usz(bd), RI.Slice(acl), RI.TInt(alpha, "i16"),
                                  eb, 0)
                o = np.array([int(v) for v in dst.data], np.int64).reshape(full.shape)
                blk = o[PAD + y:PAD + y + h, PAD + x:PAD + x + w].copy()
                o[PAD + y:PAD + y + h, PAD + x:PAD + x + w] = 0
                assert not o.any()  # nothing written outside the block
                meta.append((tx, variant, alpha, bd))
                edges.append(e)
                acs.append(ac)
                outs.append(blk.ravel())
                off.append(off[-1] + w * h)
                k += 1
        print("predict_cfl bd%d: %d cases" % (bd, k), flush=True)
    out["pred_meta"] = np.array(meta, np.int32)
    out["pred_edge"] = np.array(edges, np.uint16)
    out["pred_ac"] = np.concatenate(acs).astype(np.int16)
    out["pred_out"] = np.concatenate(outs).astype(np.uint16)
    out["pred_off"] = np.array(off, np.int64)


class _NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def plane_cfg(xdec, ydec):
    return RI.Struct("PlaneConfig", {"xdec": usz(xdec), "ydec": usz(ydec)})


def allowed_cells(I):
    """(bsize, xdec, ydec) with cfl_allowed and a valid subsampled_size, by
    the reference's own methods."""
    cells = []
    for xdec, ydec in ((0, 0), (1, 0), (1, 1)):
        for b in range(22):
            bs = H.BlockSizeV(b)
            if not bs.cfl_allowed():
                continue
            if isinstance(bs.subsampled_size(usz(xdec), usz(ydec)), _Invalid):
                continue
            cells.append((b, xdec, ydec))
    return cells


def job_pos(bs, xdec, ydec, gx, gy):
    """A luma position with chroma (has_chroma, src/context.rs:551-560: an
    odd block offset where the block is 4 wide / high and subsampled)."""
    x = gx + (4 if xdec and bs.w == 4 else 0)
    y = gy + (4 if ydec and bs.h == 4 else 0)
    return x, y


def gen_luma_ac(I, rng, out):
    luma_ac = G.F(I, "luma_ac", "encoder.rs")
    LW, LH = 64, 48
    meta, outs, off = [], [], [0]
    cells = allowed_cells(I)
    assert len(cells) == 27 and all(b < ALLOWED for b, _, _ in cells)
    out["ac_origin"] = np.array([PAD, PAD], np.int32)
    for bd in (8, 10, 12):
        maxv = (1 << bd) - 1
        img = rng.integers(0, maxv + 1, (LH, LW))
        img[16:48, 32:64] = maxv  # saturated: the i16 samples reach 32760 at 12 bit
        img[20:24, 36:40] = maxv - 1
        full = np.pad(img, PAD, mode="edge")
        out["ac_luma_bd%d" % bd] = full.astype(np.uint16)
        rec0 = plane(full, bd)
        for n, (b, xdec, ydec) in enumerate(cells):
            if (n + bd // 2) % 3 == 0 and b not in (0, 9):
                continue  # two thirds of the cells per depth, the extremes always
            bs = H.BlockSizeV(b)
            gx, gy = ((0, 0), (32, 16), (16, 8))[(n + bd) % 3]
            x, y = job_pos(bs, xdec, ydec, gx, gy)
            ts = _NS(input=_NS(planes=[None, _NS(cfg=plane_cfg(xdec, ydec))]),
                     rec=_NS(planes=[rec0.as_region()]))
            ac = [RI.TInt(0, "i16")] * 1024
            luma_ac(ac, ts, tile_bo(x >> 2, y >> 2), bs, generics={"T": G.prim(bd)})
            w, h = max(4, bs.w >> xdec), max(4, bs.h >> ydec)
            meta.append((b, xdec, ydec, bd, x, y))
            outs.append(np.array([int(v) for v in ac[:w * h]], np.int64))
            off.append(off[-1] + w * h)
        print("luma_ac bd%d: %d cases" % (bd, len(meta)), flush=True)
    out["ac_meta"] = np.array(meta, np.int32)
    out["ac_out"] = np.concatenate(outs).astype(np.int16)
    out["ac_off"] = np.array(off, np.int64)


def cfg_struct(pl):
    """The plane's PlaneConfig as a struct value (rdo_cfl_alpha destructures
    it: `let &PlaneConfig { xdec, ydec, .. } = ...plane_cfg`)."""
    c = pl.cfg
    return RI.Struct("PlaneConfig", {k: usz(getattr(c, k)) for k in (
        "stride", "alloc_height", "width", "height", "xdec", "ydec", "xpad", "ypad", "xorigin",
        "yorigin")})


class _CFLParams:
    """Records what CFLParams::from_alpha (src/context.rs:1909-1914) gets."""

    @staticmethod
    def from_alpha(u, v):
        return (int(RI.deref(u)), int(RI.deref(v)))


def gen_rdo_cfl(I, rng, out):
    """rdo_cfl_alpha on a tile at the frame's origin: blocks at x == 0 / y ==
    0 exercise the NONE / LEFT / TOP variants.  The source chroma follows
    clip(dc-ish + scaled(a*, ac) + noise) so the answers spread over the
    alphas and the early break both fires and does not."""
    import re
    rdo = G.src_of(I, "rdo.rs")
    for n in ("RawDistortion", "Distortion", "ScaledDistortion"):
        fns = []
        for m in re.finditer(r"\bimpl\b[^{;]*\b%s\s*\{" % n, rdo.src):
            fns += RI.parse_impl_fns(RI.find_item(rdo.src, "impl", n, m.start()))
        I.define_impl(n, fns)
    G.F(I, "sse_wxh", "rdo.rs")
    G.F(I, "luma_ac", "encoder.rs")
    search = G.F(I, "rdo_cfl_alpha", "rdo.rs")
    I.globals.vars["CFLParams"] = _CFLParams
    H.BlockSizeV.largest_chroma_tx_size = lambda self, xdec, ydec: tx_size_of(
        min(32, max(4, self.w >> int(xdec))), min(32, max(4, self.h >> int(ydec))))
    G.TxSizeV.block_size = lambda self: H.BlockSize.from_width_and_height(self.w, self.h)
    LW, LH = 64, 64
    out["rdo_origin"] = np.array([PAD, PAD], np.int32)
    meta, alphas = [], []
    cells = allowed_cells(I)
    for cfg, (xdec, ydec, bd) in enumerate(((1, 1, 8), (1, 0, 10), (0, 0, 12), (1, 1, 10),
                                            (0, 0, 8), (1, 0, 12))):
        G.PModeV.pixel = G.prim(bd)
        I.globals.vars["T"] = G.prim(bd)
        maxv = (1 << bd) - 1
        mine = [c for c in cells if (c[1], c[2]) == (xdec, ydec)]
        # smooth-ish luma so that ac is moderate and alpha matters at every step
        base = rng.integers(0, maxv + 1, (LH + 8, LW + 8))
        luma = (np.cumsum(np.cumsum(base, 0), 1) // 61) % (maxv + 1)
        luma = luma[4:4 + LH, 4:4 + LW]
        cw, ch = LW >> xdec, LH >> ydec
        rec_c = [rng.integers(maxv // 4, 3 * maxv // 4, (ch, cw)) for _ in range(2)]
        src_c = [np.zeros((ch, cw), np.int64) for _ in range(2)]
        picks = [mine[(3 * cfg + 2 * i) % len(mine)] for i in range(3)]
        jobs = []
        for i, (b, _, _) in enumerate(picks):
            bs = H.BlockSizeV(b)
            gx, gy = ((0, 0), (32, 0), (0, 32))[i]
            jobs.append((b,) + job_pos(bs, xdec, ydec, gx, gy))
        jobs.append((picks[0][0],) + job_pos(H.BlockSizeV(picks[0][0]), xdec, ydec, 32, 32))
        for n, (b, x, y) in enumerate(jobs):
            bs = H.BlockSizeV(b)
            w, h = max(4, bs.w >> xdec), max(4, bs.h >> ydec)
            cx, cy = (x >> 2 >> xdec) << 2, (y >> 2 >> ydec) << 2
            lx = x - (4 if xdec and bs.w == 4 else 0)
            ly = y - (4 if ydec and bs.h == 4 else 0)
            blk = luma[ly:ly + (h << ydec), lx:lx + (w << xdec)]
            smp = blk.reshape(h, 1 << ydec, w, 1 << xdec).sum(axis=(1, 3)) << (3 - xdec - ydec)
            ac = smp - int(round(smp.mean()))
            for p in range(2):
                a = int(rng.integers(-20, 21)) if n != 3 else int(rng.integers(-4, 5))
                q6 = a * ac
                sc = np.sign(q6) * ((np.abs(q6) + 32) >> 6)
                dc = int(rec_c[p][max(cy - 1, 0), cx:cx + w].mean()) if cy else maxv // 2
                src_c[p][cy:cy + h, cx:cx + w] = np.clip(dc + sc + rng.integers(-3, 4, (h, w)), 0,
                                                         maxv)
        fulls_rec = [np.pad(luma, PAD, mode="edge")] + [np.pad(c, PAD, mode="edge") for c in rec_c]
        fulls_src = [np.pad(luma, PAD, mode="edge")] + [np.pad(c, PAD, mode="edge") for c in src_c]
        for p in range(3):
            out["rdo_rec%d_p%d" % (cfg, p)] = fulls_rec[p].astype(np.uint16)
            out["rdo_src%d_p%d" % (cfg, p)] = fulls_src[p].astype(np.uint16)
        for (b, x, y) in jobs:
            def planes(fulls):
                pls = []
                for p, f in enumerate(fulls):
                    pl = plane(f.copy(), bd, xdec if p else 0, ydec if p else 0)
                    pl.cfg = cfg_struct(pl)
                    pls.append(pl)
                return pls
            rec, src = planes(fulls_rec), planes(fulls_src)
            trect = RI.Struct("TileRect", {"x": usz(0), "y": usz(0), "width": usz(LW),
                                           "height": usz(LH)})
            trect._f["decimated"] = lambda xd, yd: RI.Struct("TileRect", {
                "x": usz(0), "y": usz(0), "width": usz(LW >> int(xd)), "height": usz(LH >> int(yd))})
            ts = _NS(input=_NS(planes=src), input_tile=_NS(planes=[p.as_region() for p in src]),
                     rec=_NS(planes=[p.as_region() for p in rec]), tile_rect=lambda: trect)
            r = search(ts, tile_bo(x >> 2, y >> 2), H.BlockSizeV(b), usz(bd), 0,
                       generics={"T": G.prim(bd)})
            r = (0, 0) if r is None else r
            meta.append((cfg, b, xdec, ydec, bd, x, y))
            alphas.append(r)
            print("rdo_cfl_alpha cfg %d %s at (%d, %d): %s" % (cfg, H.BLOCK_NAMES[b], x, y, r),
                  flush=True)
    out["rdo_meta"] = np.array(meta, np.int32)
    out["rdo_alpha"] = np.array(alphas, np.int16)


def main():
    I = interp()
    rng = np.random.default_rng(20261019)
    out = {}
    gen_predict(I, rng, out)
    gen_luma_ac(I, rng, out)
    gen_rdo_cfl(I, rng, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

"""Golden vectors for the mode decision's arithmetic, produced by RUNNING the
reference's own Rust function text (rsinterp.py) -- needs the reference
checkout that gen_golden_ref.py reads:

    python tools/refeval/gen_mode_decide_ref.py

Functions evaluated from src/rdo.rs: compute_mean_importance (:477-493),
compute_distortion_bias (:495-508), compute_distortion (:338-411) and
compute_tx_distortion (:414-475) whole -- with cdef_dist_wxh / sse_wxh and the
bias closures they pass -- on stand-ins for `fi` and `ts` that hold the fields
they read, compute_rd_cost (:563-568) and the three Mul impls (:525-543).
PlaneRegion::frame_block_offset (src/tiling/plane_region.rs:264-302, inside a
macro the interpreter does not expand) is a host method here.

Restated, not run: encode_tx_block's last two lines (src/encoder.rs:1234-1236),
composed per transform block from the interpreted compute_distortion_bias and
Mul impls with tx_bo as write_tx_blocks / write_tx_tree form it (:1785-1788,
1864-1869); and the control flow of luma_chroma_mode_rdo / rdo_mode_decision
(:648-780, 949-1153), a transliteration with the reference's nested
closures over random candidate lists (`rdo_walk` below).

The pixels are tests/mode_decide_ref.py's synth_planes, a formula, so that
only results are stored.  Only numbers are written (tests/golden/ref_mode_decide.npz); tests/
test_mode_decide.py checks tests/mode_decide_ref.py against them.
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402
from gen_cfl_ref import plane_cfg, usz  # noqa: E402

sys.path.insert(0, G.ROOT)
from tests.mode_decide_ref import synth_planes  # noqa: E402  (the vectors' pixel inputs, by formula)

OUT = os.path.join(G.ROOT, "tests", "golden", "ref_mode_decide.npz")
W_IN_B, H_IN_B = 17, 9
W_IMP, H_IMP = 9, 5
FW, FH, PAD = 68, 36, 64


class _NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class TuneV(int):
    pass


Tune = type("Tune", (), {"Psnr": TuneV(0), "Psychovisual": TuneV(1)})


def block_offset(kind, x, y):
    return RI.Struct(kind, {"0": RI.Struct("BlockOffset", {"x": usz(x), "y": usz(y)})})


def _frame_block_offset(self):
    """PlaneRegion::frame_block_offset (src/tiling/plane_region.rs:264-302)."""
    c = self.plane_cfg
    r = self.rect()
    return block_offset("PlaneBlockOffset", int(r.x) >> (2 - int(c.xdec)), int(r.y) >> (2 - int(c.ydec)))


H.PlaneRegion.frame_block_offset = _frame_block_offset


def interp():
    I = G.make_interp()
    I.release = True
    rdo = G.src_of(I, "rdo.rs")
    for n in ("RawDistortion", "Distortion", "ScaledDistortion"):
        fns = []
        for m in re.finditer(r"\bimpl\b[^{;]*\b%s\s*\{" % n, rdo.src):
            fns += RI.parse_impl_fns(RI.find_item(rdo.src, "impl", n, m.start()))
        I.define_impl(n, fns)
    I.globals.vars["Tune"] = Tune
    I.globals.vars["OD_BITRES"] = RI.TInt(3, "u8")  # src/ec.rs
    I.globals.vars["PlaneConfig"] = RI.StructType("PlaneConfig")
    for n in ("cdef_dist_wxh_8x8", "cdef_dist_wxh", "sse_wxh", "compute_mean_importance",
              "compute_distortion_bias", "compute_distortion", "compute_tx_distortion",
              "compute_rd_cost"):
        G.F(I, n, "rdo.rs")
    return I


def make_fi(imp, bd, tune, scale, lam):
    return _NS(config=_NS(tune=TuneV(tune)), sequence=_NS(bit_depth=usz(bd)),
               dist_scale=[float(v) for v in scale], w_in_b=usz(W_IN_B), h_in_b=usz(H_IN_B),
               w_in_imp_b=usz(W_IMP), block_importances=[np.float32(v) for v in imp.reshape(-1)],
               **{"lambda": float(lam)})


def host_planes(planes, xdec, ydec):
    return [H.Plane.from_full(a, xo, yo, FW >> (xdec if p else 0), FH >> (ydec if p else 0),
                              xdec if p else 0, ydec if p else 0)
            for p, (a, xo, yo) in enumerate(planes)]


def tile_regions(planes, tile):
    out = []
    for pl in planes:
        xd, yd = int(pl.cfg.xdec), int(pl.cfg.ydec)
        rect = RI.Struct("Rect", {"x": RI.wrap(tile[0] >> xd, "isize"), "y": RI.wrap(tile[1] >> yd, "isize"),
                                  "width": RI.wrap(tile[2] >> xd, "usize"),
                                  "height": RI.wrap(tile[3] >> yd, "usize")})
        out.append(H.PlaneRegion(pl, rect))
    return out


def make_ts(src, rec, tile, xdec, ydec):
    cfgs = [_NS(cfg=plane_cfg(0, 0)), _NS(cfg=plane_cfg(xdec, ydec)), _NS(cfg=plane_cfg(xdec, ydec))]
    return _NS(input_tile=_NS(planes=tile_regions(src, tile)), rec=_NS(planes=tile_regions(rec, tile)),
               input=_NS(planes=cfgs))


def u64(v):
    return int(RI.deref(v)._f["0"])


def rdo_walk(inter_groups, intra_groups):
    """rdo_mode_decision's calls of luma_chroma_mode_rdo (src/rdo.rs:949-1006,
    1008, 1127-1152) and that function's own flow (:648-780), transliterated:
    a group is (skip candidates, coded candidates), a candidate (index, rd,
    distortion).  Returns (the winner's index or -1, the indices evaluated)."""
    best = {"rd_cost": float(np.finfo(np.float64).max), "skip": False, "cand": -1}
    evaluated = []

    def luma_chroma_mode_rdo(luma_mode_is_intra, skips, coded):
        def chroma_rdo(skip):
            zero_distortion = False
            for k, rd, distortion in (skips if skip else coded):
                evaluated.append(k)
                is_zero_dist = distortion == 0
                if rd < best["rd_cost"]:
                    best["rd_cost"], best["skip"], best["cand"] = rd, skip, k
                    zero_distortion = is_zero_dist
            return zero_distortion
        # Don't skip when using intra modes
        zero_distortion = chroma_rdo(True) if not luma_mode_is_intra else False
        if not zero_distortion:  # early skip
            chroma_rdo(False)

    for skips, coded in inter_groups:
        luma_chroma_mode_rdo(False, skips, coded)
    if not best["skip"]:
        for skips, coded in intra_groups:
            luma_chroma_mode_rdo(True, [], coded)
    return best["cand"], evaluated


def gen_walks(rng, out):
    """Random candidate lists in the reference's order: the inter groups, then
    the intra groups; costs from a small pool so that equal costs occur."""
    rows, off, winners = [], [0], []
    for _ in range(300):
        k0 = len(rows)
        groups = ([], [])
        g = 0
        for intra in (0, 1):
            for _ in range(int(rng.integers(0, 4))):
                skips, coded = [], []
                for flags in ([] if intra else [1] * int(rng.integers(0, 3))) + [0] * int(rng.integers(0 + intra, 3)):
                    dist = int(rng.choice([0, 0, 7, 120, 120, 3000]))
                    rate = int(rng.choice([0, 8, 8, 40, 900]))
                    rd = float(dist) + 2.5 * (rate / 8.0)
                    (skips if flags else coded).append((len(rows) - k0, rd, dist))
                    rows.append((g, flags | 2 * intra, rate, dist, rd, 0))
                groups[intra].append((skips, coded))
                g += 1
        win, ev = rdo_walk(*groups)
        for k in ev:
            rows[k0 + k] = rows[k0 + k][:5] + (1,)
        winners.append(win)
        off.append(len(rows))
    out["walk_rows"] = np.array([r[:4] + r[5:] for r in rows], np.int64)  # group, flags, rate, dist, evaluated
    out["walk_cost"] = np.array([r[4] for r in rows], np.float64)
    out["walk_off"] = np.array(off, np.int64)
    out["walk_winner"] = np.array(winners, np.int64)
    print("walks: %d lists, %d candidates, %d gated" % (len(winners), len(rows), sum(1 - r[5] for r in rows)))


def main():
    I = interp()
    V = I.globals.vars
    rng = np.random.default_rng(20240607)
    out = {}
    imp = (rng.random((H_IMP, W_IMP)) * 7).astype(np.float32)
    imp[0, 0], imp[0, 1], imp[1, 0], imp[1, 1] = 0.0, 2.0, 4.0, np.float32(1.9999999)
    imp[2, 2:4] = np.float32(3.9999998)
    imp[4, 8] = 250.0
    out["importance"] = imp
    out["frame"] = np.array([W_IN_B, H_IN_B, W_IMP, FW, FH, PAD], np.int32)

    # ---- compute_mean_importance / compute_distortion_bias
    fi = make_fi(imp, 8, 0, (1, 1, 1), 1)
    cases, means, biases = [], [], []
    for b in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12):
        bs = H.BlockSizeV(b)
        pos = [(0, 0), (2, 0), (16, 8), (15, 7), (16, 0), (0, 8), (18, 10), (4, 4), (6, 2)]
        for x, y in pos:
            fbo = block_offset("PlaneBlockOffset", x, y)
            m = V["compute_mean_importance"](fi, fbo, bs, generics={"T": G.prim(8)})
            bias = V["compute_distortion_bias"](fi, fbo, bs, generics={"T": G.prim(8)})
            assert isinstance(m, np.float32), type(m)
            cases.append((b, x, y))
            means.append(m)
            biases.append(float(bias))
    out["bias_cases"] = np.array(cases, np.int32)
    out["bias_mean"] = np.array(means, np.float32)
    out["bias_value"] = np.array(biases, np.float64)
    print("bias: %d cases" % len(cases), flush=True)

    # ---- the Mul impls and compute_rd_cost
    vals = [0, 1, 2, 1000, 123456789, (1 << 53) + 1, (1 << 63) + 12345, (1 << 64) - 1] + \
        [int(v) for v in rng.integers(0, 1 << 40, 24)]
    facs = [0.0, 0.65, 1.0, 0.9999999999999999, 1.3166667222976685, 84.0, 1e-9, 2.5e7] + \
        [float(v) for v in rng.random(24) * 3]
    mc, mr, md = [], [], []
    for v in vals:
        for f in facs[:8] + facs[8 + len(mc) % 5::5]:
            raw = RI.Struct("RawDistortion", {"0": RI.TInt(v, "u64")})
            dis = RI.Struct("Distortion", {"0": RI.TInt(v, "u64")})
            mc.append((v, f))
            mr.append(u64(I.binop("*", raw, f)))
            md.append(u64(I.binop("*", dis, f)))
    out["mul_value"] = np.array([c[0] for c in mc], np.uint64)
    out["mul_factor"] = np.array([c[1] for c in mc], np.float64)
    out["mul_raw"] = np.array(mr, np.uint64)
    out["mul_dist"] = np.array(md, np.uint64)
    rc, rv = [], []
    for k in range(40):
        rate = int(rng.integers(0, 1 << 32)) if k % 3 else int(rng.integers(0, 4000))
        dist = vals[k % len(vals)]
        lam = float(rng.random() * 500) if k % 4 else 0.0
        f2 = make_fi(imp, 8, 0, (1, 1, 1), lam)
        sd = RI.Struct("ScaledDistortion", {"0": RI.TInt(dist, "u64")})
        rc.append((rate, dist, lam))
        rv.append(float(V["compute_rd_cost"](f2, RI.TInt(rate, "u32"), sd, generics={"T": G.prim(8)})))
    out["rd_rate"] = np.array([c[0] for c in rc], np.uint32)
    out["rd_dist"] = np.array([c[1] for c in rc], np.uint64)
    out["rd_lambda"] = np.array([c[2] for c in rc], np.float64)
    out["rd_cost"] = np.array(rv, np.float64)
    print("mul: %d, rd: %d" % (len(mc), len(rc)), flush=True)

    # ---- compute_distortion / compute_tx_distortion, whole
    SETTINGS = [(8, 1, 1), (8, 0, 0), (8, 1, 0), (10, 1, 1), (12, 1, 1)]
    TILES = [(0, 0, 128, 64), (64, 0, 64, 64)]
    dc, dv = [], []
    for si, (bd, xdec, ydec) in enumerate(SETTINGS):
        src = synth_planes(si, bd, xdec, ydec, FW, FH, PAD)
        rec = synth_planes(si + 100, bd, xdec, ydec, FW, FH, PAD, noise_of=src)
        hs, hr = host_planes(src, xdec, ydec), host_planes(rec, xdec, ydec)
        sizes = [3, 6] if si else [3, 4, 5, 6, 9, 12]
        for b in sizes:
            bs = H.BlockSizeV(b)
            if xdec == 1 and ydec == 0 and bs.h == 2 * bs.w:
                continue
            for ti, bo in [(0, (0, 0)), (1, (0, 0)), (0, ((64 // bs.w - 1) * bs.w // 4, 0))][:2 if b == 12 else 3]:
                tile = TILES[ti]
                if 4 * bo[0] + bs.w > tile[2] or 4 * bo[1] + bs.h > tile[3]:
                    continue
                ts = make_ts(hs, hr, tile, xdec, ydec)
                tbo = block_offset("TileBlockOffset", *bo)
                for tune in (0, 1):
                    scale = (1.0, 1.0, 1.0) if tune == 0 and b == 3 else (0.9375, 1.28125, 1.6171875)
                    fi = make_fi(imp, bd, tune, scale, 1)
                    d = V["compute_distortion"](fi, ts, bs, True, tbo, False, generics={"T": G.prim(bd)})
                    dc.append((si, b, ti, bo[0], bo[1], tune, 0) + tuple(int(v * 1e7) for v in scale))
                    dv.append(u64(d))
                    if tune == 0:  # the skip arm of compute_tx_distortion (it asserts Psnr)
                        zero = RI.Struct("ScaledDistortion", {"0": RI.TInt(0, "u64")})
                        d = V["compute_tx_distortion"](fi, ts, bs, True, tbo, zero, True, False,
                                                       generics={"T": G.prim(bd)})
                        dc.append((si, b, ti, bo[0], bo[1], tune, 1) + tuple(int(v * 1e7) for v in scale))
                        dv.append(u64(d))
            print("setting %d size %s: %d cases" % (si, H.BLOCK_NAMES[b], len(dc)), flush=True)
    out["settings"] = np.array(SETTINGS, np.int32)
    out["tiles"] = np.array(TILES, np.int32)
    out["dist_cases"] = np.array(dc, np.int64)
    out["dist_value"] = np.array(dv, np.uint64)

    # ---- the per-transform-block product of encode_tx_block, composed
    fi = make_fi(imp, 8, 0, (0.9375, 1.28125, 1.6171875), 1)
    tc, tv = [], []
    for b in (3, 6, 9, 12):
        bs = H.BlockSizeV(b)
        for (x, y) in [(0, 0), (8, 4), (16, 8), (12, 0)]:
            for p in range(3):
                d = int(rng.integers(0, 1 << 30))
                bias = V["compute_distortion_bias"](fi, block_offset("PlaneBlockOffset", x, y), bs,
                                                    generics={"T": G.prim(8)})
                raw = RI.Struct("RawDistortion", {"0": RI.TInt(d, "u64")})
                r = I.binop("*", I.binop("*", raw, bias), fi.dist_scale[p])
                tc.append((b, x, y, p, d))
                tv.append(u64(r))
    out["txb_cases"] = np.array(tc, np.int64)
    out["txb_scale"] = np.array(fi.dist_scale, np.float64)
    out["txb_value"] = np.array(tv, np.uint64)

    gen_walks(rng, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

"""Golden vectors for the transform-block loops, produced by RUNNING the
reference's own Rust function text (rsinterp.py) -- needs the reference
checkout that gen_golden_ref.py reads:

    python tools/refeval/gen_tx_blocks_ref.py

Functions evaluated: write_tx_blocks (src/encoder.rs:1757-1903) and
write_tx_tree (:1907-2037) with encode_tx_block replaced by a recording stub
that returns a scripted has_coeff (luma_ac, get_qidx and the quantizer's
update are stubs too: no transform runs here); under them BlockSize::
subsampled_size / largest_chroma_tx_size (src/partition.rs:245-297),
av1_get_coded_tx_size and get_log_tx_scale, has_chroma and
uv_intra_mode_to_tx_type_context (src/context.rs), BlockOffset::plane_offset.
What is recorded per run is the sequence of encode_tx_block calls: p, bx, by,
tx_bo, po, tx_size, tx_type, mode, alpha.  Also recorded, over their whole
domains: largest_chroma_tx_size, av1_get_coded_tx_size, get_log_tx_scale and
uv_intra_mode_to_tx_type_context.  Only numbers are written
(tests/golden/ref_tx_blocks.npz); tests/test_tx_blocks.py checks
tests/tx_blocks_ref.py and rv_tx_blocks_layout against them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402
from gen_cfl_ref import plane_cfg, usz  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "ref_tx_blocks.npz")
SIZES = list(range(3, 13))  # BLOCK_8X8 .. BLOCK_64X64 without the 4xN / Nx4 and 4:1 sizes
FORMATS = ((0, 0), (1, 0), (1, 1))
TX_TYPE_NAMES = ["DCT_DCT", "ADST_DCT", "DCT_ADST", "ADST_ADST", "FLIPADST_DCT", "DCT_FLIPADST",
                 "FLIPADST_FLIPADST", "ADST_FLIPADST", "FLIPADST_ADST", "IDTX", "V_DCT", "H_DCT",
                 "V_ADST", "H_ADST", "V_FLIPADST", "H_FLIPADST"]


class TxTypeV(int):
    pass


class _Invalid:
    """BlockSize::BLOCK_INVALID: the last variant, equal to nothing else."""

    def __lt__(self, o):
        return False

    def __gt__(self, o):
        return True

    __le__, __ge__ = __lt__, __gt__

    def __repr__(self):
        return "BLOCK_INVALID"


class _NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def field(s, *names):
    v = s
    for n in names:
        v = RI.deref(v)
        v = v._f[n] if isinstance(v, RI.Struct) else getattr(v, n)
    return v


class Recorder:
    """encode_tx_block's stand-in."""

    def __init__(self):
        self.calls, self.has_coeff = [], True

    def __call__(self, fi, ts, cw, w, p, partition_bo, bx, by, tile_bo, mode, tx_size, tx_type,
                 bsize, po, skip, ac, alpha, rdo_type, need_recon_pixel):
        po = RI.deref(po)
        self.calls.append((int(p), int(bx), int(by), int(field(tile_bo, "0", "x")),
                           int(field(tile_bo, "0", "y")), int(field(po, "x")), int(field(po, "y")),
                           int(tx_size), int(tx_type), int(mode), int(RI.deref(alpha))))
        return (self.has_coeff, RI.TInt(0, "u64"))


class _Dist:
    @staticmethod
    def zero():
        return RI.TInt(0, "u64")


def interp():
    I = G.make_interp()
    I.release = True
    G.intra_env(I)
    enc = RI.Source(G.REF + "encoder.rs")
    ctx = RI.Source(G.REF + "context.rs")
    I.sources += [enc, ctx]
    part = G.src_of(I, "partition.rs")
    I.globals.vars["BLOCK_INVALID"] = _Invalid()
    I.globals.vars["TxType"] = type("TxTypeNS", (), {n: TxTypeV(i) for i, n in
                                                     enumerate(TX_TYPE_NAMES)})
    for i, n in enumerate(TX_TYPE_NAMES):  # `use TxType::*`
        I.globals.vars[n] = TxTypeV(i)
    for i in range(19):  # `use TxSize::*`
        t = G.TxSizeV(i)
        I.globals.vars["TX_%dX%d" % (t.w, t.h)] = t
    for i, n in enumerate(G.INTRA_MODE_NAMES):  # `use PredictionMode::*`
        I.globals.vars[n] = G.PModeV(i)
    G.PModeV.is_cfl = lambda self: int(self) == 13
    G.TxSizeV.width_mi = lambda self: usz(self.w >> 2)
    G.TxSizeV.height_mi = lambda self: usz(self.h >> 2)
    # BlockSize's own methods, from the reference's text, on the host value
    for m in ("subsampled_size", "largest_chroma_tx_size"):
        f = I.make_fn(part.fn(m, "impl BlockSize"), I.globals)
        setattr(H.BlockSizeV, m, (lambda self, *a, _f=f: _f(self, *a)))
    for n in ("BlockOffset", "TileBlockOffset"):
        I.define_impl(n, ctx.impl(n))
    I.globals.vars["ScaledDistortion"] = _Dist
    I.globals.vars["get_qidx"] = lambda *a: RI.TInt(100, "u8")
    for n in ("has_chroma", "uv_intra_mode_to_tx_type_context", "av1_get_coded_tx_size"):
        G.F(I, n, "context.rs")
    G.F(I, "get_log_tx_scale", "quantize.rs")
    return I


def run(I, fn, rec, b, ts, tt, lm, cm, xdec, ydec, bo_x, bo_y, luma_only, alphas, has_coeff):
    rec.calls, rec.has_coeff = [], has_coeff
    I.globals.vars["encode_tx_block"] = rec
    I.globals.vars["luma_ac"] = lambda *a, **k: None
    cfgs = [_NS(cfg=plane_cfg(0, 0)), _NS(cfg=plane_cfg(xdec, ydec)), _NS(cfg=plane_cfg(xdec, ydec))]
    ts_ = _NS(input=_NS(planes=cfgs), qc=_NS(update=lambda *a: None))
    fi = _NS(sequence=_NS(bit_depth=usz(8)), dc_delta_q=[0, 0, 0], ac_delta_q=[0, 0, 0])
    bo = I.ev(RI.Parser("TileBlockOffset(BlockOffset { x: %d, y: %d })" % (bo_x, bo_y)).parse_expr(),
              I.globals)
    cfl = _NS(alpha=lambda i: RI.TInt(alphas[int(i)], "i16"))
    common = (fi, ts_, None, None, G.PModeV(lm))
    if fn == "write_tx_blocks":
        I.globals.vars[fn](*common, G.PModeV(cm), bo, H.BlockSizeV(b), G.TxSizeV(ts), TxTypeV(tt),
                           False, cfl, bool(luma_only), 0, True, generics={"T": G.prim(8)})
    else:
        I.globals.vars[fn](*common, bo, H.BlockSizeV(b), G.TxSizeV(ts), TxTypeV(tt), False,
                           bool(luma_only), 0, True, generics={"T": G.prim(8)})
    return list(rec.calls)


def main():
    I = interp()
    for n in ("write_tx_blocks", "write_tx_tree"):
        G.F(I, n, "encoder.rs")
    rec = Recorder()
    out = {}
    # ---- the tables, over their whole domains
    lct = []
    for b in range(22):
        for xdec, ydec in FORMATS:
            bs = H.BlockSizeV(b)
            sub = bs.subsampled_size(usz(xdec), usz(ydec))
            if isinstance(sub, _Invalid):
                lct.append((b, xdec, ydec, -1))
            else:
                lct.append((b, xdec, ydec, int(bs.largest_chroma_tx_size(usz(xdec), usz(ydec)))))
    out["largest_chroma_tx_size"] = np.array(lct, np.int32)
    out["coded_tx_size"] = np.array([int(I.globals.vars["av1_get_coded_tx_size"](G.TxSizeV(i)))
                                     for i in range(19)], np.int32)
    out["log_tx_scale"] = np.array([int(I.globals.vars["get_log_tx_scale"](G.TxSizeV(i)))
                                    for i in range(19)], np.int32)
    out["uv_tx_type"] = np.array([int(I.globals.vars["uv_intra_mode_to_tx_type_context"](G.PModeV(m)))
                                  for m in range(14)], np.int32)
    # ---- the call sequences
    meta, calls, off = [], [], [0]

    def record(fn, *a):
        rows = run(I, fn, rec, *a)
        meta.append(a[:9] + (int(a[9]),) + tuple(a[10]) + (int(a[11]),))
        calls.extend(rows)
        off.append(off[-1] + len(rows))
    k = 0
    for b in SIZES:
        bs = H.BlockSizeV(b)
        for xdec, ydec in FORMATS:
            invalid = isinstance(bs.subsampled_size(usz(xdec), usz(ydec)), _Invalid)
            # a partition position: aligned to the block, not the tile's origin
            bo_x, bo_y = (bs.w // 4) * (1 + k % 3), (bs.h // 4) * (k % 2)
            k += 1
            for ts in range(19):
                t = G.TxSizeV(ts)
                if t.w > bs.w or t.h > bs.h:
                    continue
                whole = (t.w, t.h) == (bs.w, bs.h)
                for luma_only in (False, True):
                    if invalid and not luma_only:
                        continue  # the reference panics (largest_chroma_tx_size)
                    # intra: DC / V / H / PAETH / CFL chroma where the luma block is whole
                    cms = (0, 1, 2, 12, 13) if whole and not luma_only else (0,)
                    for cm in cms:
                        if cm == 13 and b > 9:
                            continue  # cfl_allowed
                        record("write_tx_blocks", b, ts, 0, 12 if cm else 3, cm, xdec, ydec, bo_x,
                               bo_y, luma_only, (5, -3), True)
                    if whole:  # write_tx_tree codes one luma block at the origin
                        tt = 0 if max(t.w, t.h) == 64 else 3
                        for hc in (True, False):
                            record("write_tx_tree", b, ts, tt, 19, 0, xdec, ydec, bo_x, bo_y,
                                   luma_only, (0, 0), hc)
        print("%s: %d runs, %d calls" % (H.BLOCK_NAMES[b], len(meta), len(calls)), flush=True)
    out["seq_meta"] = np.array(meta, np.int32)
    out["seq_calls"] = np.array(calls, np.int32)
    out["seq_off"] = np.array(off, np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

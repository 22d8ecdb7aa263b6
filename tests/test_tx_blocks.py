"""A partition's transform blocks as one launch (rv_tx_blocks.hip,
rav1e_amd.tx_blocks_batch): write_tx_blocks / write_tx_tree (src/encoder.rs:
1757-2037) over encode_tx_block (:1077-1237) without the bitstream writer.

CPU: tests/tx_blocks_ref.py (the numpy restatement, the GPU tests' checker)
against the call sequences the reference's own text produced (tools/refeval/
gen_tx_blocks_ref.py -> tests/golden/ref_tx_blocks.npz), rv_tx_blocks_layout
against the same vectors, its error codes, the exported symbols.  GPU: levels,
eobs, distortions and dst pixels bit for bit (tolerance 0) against the
restatement.

The GPU setting: one 128x128 luma tile at (16, 8) of a 160x152 frame in padded
planes, random rec and src, at most 64 jobs a launch: the tile's corners,
every edge and interior positions."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rav1e_amd as R
from tests import tx_blocks_ref as T

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_tx_blocks.npz")
B, TS, TT, PM = R.BlockSize, R.TxSize, R.TxType, R.PredictionMode
EINVAL, ENOTSUP = R.RV_EINVAL, R.RV_ENOTSUP
FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}


@functools.lru_cache(None)
def gold():
    return dict(np.load(GOLD))


def bsize_tx(b):
    return T.X.tx_size_of(T.BLK_W[b], T.BLK_H[b])


# ---------------------------------------------------------------- CPU: golden
def test_call_sequences_equal_reference():
    """Every recorded write_tx_blocks / write_tx_tree run: the restated loops
    make the same encode_tx_block calls, entry for entry."""
    g = gold()
    meta, off, calls = g["seq_meta"], g["seq_off"], g["seq_calls"]
    assert len(meta) + 1 == len(off) and len(meta) > 500
    cov = set()
    for k, row in enumerate(meta.tolist()):
        (b, ts, tt, lm, cm, xd, yd, bo_x, bo_y, luma_only, au, av, has_coeff) = row
        got = T.call_sequence(b, ts, tt, lm, cm, xd, yd, bo_x, bo_y, bool(luma_only), (au, av),
                              bool(has_coeff))
        want = [tuple(r) for r in calls[off[k]:off[k + 1]].tolist()]
        assert got == want, row
        cov.add(("size", b, xd, yd))
        cov.add(("inter", lm >= 14, bool(luma_only), bool(has_coeff)))
        cov.add(("cm", cm if lm < 14 else -1))
    for b in T.SIZES:
        for xd, yd in T.FORMATS:
            if T.subsampled_wh(b, xd, yd) is not None:
                assert ("size", b, xd, yd) in cov
    for inter in (False, True):
        for lo in (False, True):
            assert any(c[:3] == ("inter", inter, lo) for c in cov)
    assert ("inter", True, False, False) in cov and ("inter", True, False, True) in cov
    for cm in (0, 1, 2, 12, 13):  # DC / V / H / PAETH / CFL
        assert ("cm", cm) in cov


def test_size_tables_equal_reference():
    """largest_chroma_tx_size, av1_get_coded_tx_size, get_log_tx_scale and
    uv_intra_mode_to_tx_type_context over their whole domains."""
    g = gold()
    for b, xd, yd, ts in g["largest_chroma_tx_size"].tolist():
        if ts < 0:
            assert T.subsampled_wh(b, xd, yd) is None
        elif b in T.SIZES:
            assert T.largest_chroma_tx_size(b, xd, yd) == ts
    assert len(g["coded_tx_size"]) == 19
    for ts, cts in enumerate(g["coded_tx_size"].tolist()):
        assert T.coded_wh(ts) == (T.TX_W[cts], T.TX_H[cts])
    assert [T.log_tx_scale(ts) for ts in range(19)] == g["log_tx_scale"].tolist()
    assert T.UV_TX_TYPE == g["uv_tx_type"].tolist()


def _layout_or_code(b, ts, xd, yd, lo):
    try:
        return R.tx_blocks_layout(b, ts, xd, yd, lo), 0
    except R.Rav1eHipError as e:
        return None, e.code


def test_layout_equals_reference():
    """rv_tx_blocks_layout for every supported combination: the counts, sizes
    and offsets the recorded sequences show; the stated code for every other."""
    g = gold()
    meta, off, calls = g["seq_meta"], g["seq_off"], g["seq_calls"]
    seen = set()
    for k, row in enumerate(meta.tolist()):
        b, ts, _, _, _, xd, yd, bo_x, bo_y, luma_only = row[:10]
        if (b, ts, xd, yd, luma_only) in seen:
            continue
        seen.add((b, ts, xd, yd, luma_only))
        L, code = _layout_or_code(b, ts, xd, yd, luma_only)
        assert code == 0, row
        rows = calls[off[k]:off[k + 1]].tolist()
        assert L.planes == (1 if luma_only else 3)
        assert L.blocks_per_job == len(rows)
        levels = 0
        for p in range(L.planes):
            mine = [r for r in rows if r[0] == p]
            assert L.n_blocks[p] == len(mine) == L.cols[p] * L.rows[p]
            assert all(r[7] == L.tx_size[p] for r in mine)
            cw, ch = T.coded_wh(L.tx_size[p])
            assert L.coded_area[p] == cw * ch
            assert L.first_block[p] == rows.index(mine[0]) and L.level_off[p] == levels
            levels += len(mine) * cw * ch
            # po minus the partition's own plane offset
            px, py = ((bo_x >> xd) << 2, (bo_y >> yd) << 2) if p else (4 * bo_x, 4 * bo_y)
            assert [(L.blk_x[p][i], L.blk_y[p][i]) for i in range(len(mine))] == \
                [(r[5] - px, r[6] - py) for r in mine]
            assert (L.plane_w[p], L.plane_h[p]) == ((T.BLK_W[b] >> xd, T.BLK_H[b] >> yd) if p else
                                                    (T.BLK_W[b], T.BLK_H[b]))
        assert L.levels_per_job == levels
    # every supported (bsize, layout) and every luma tx_size that divides it was recorded
    for b in T.SIZES:
        for xd, yd in T.FORMATS:
            for ts in range(19):
                for lo in (0, 1):
                    if T.check_args(b, ts, xd, yd, lo) == 0:
                        assert (b, ts, xd, yd, lo) in seen


def test_layout_error_codes():
    for b in range(-1, 23):
        for ts in range(-1, 20):
            for xd, yd in list(T.FORMATS) + [(0, 1), (2, 0)]:
                for lo in (0, 1):
                    L, code = _layout_or_code(b, ts, xd, yd, lo)
                    assert code == T.check_args(b, ts, xd, yd, lo), (b, ts, xd, yd, lo)
    # the cases the contract names
    assert _layout_or_code(B.BLOCK_4X4, TS.TX_4X4, 1, 1, 0)[1] == ENOTSUP
    assert _layout_or_code(B.BLOCK_8X4, TS.TX_4X4, 1, 1, 0)[1] == ENOTSUP
    assert _layout_or_code(B.BLOCK_16X4, TS.TX_4X4, 1, 1, 0)[1] == ENOTSUP
    assert _layout_or_code(B.BLOCK_64X16, TS.TX_16X16, 1, 1, 0)[1] == ENOTSUP
    assert _layout_or_code(B.BLOCK_128X128, TS.TX_64X64, 1, 1, 0)[1] == ENOTSUP
    assert _layout_or_code(B.BLOCK_8X16, TS.TX_8X16, 1, 0, 0)[1] == ENOTSUP  # no subsampled_size
    assert _layout_or_code(B.BLOCK_8X16, TS.TX_8X16, 1, 0, 1)[1] == 0        # luma only: not asked
    assert _layout_or_code(B.BLOCK_8X8, TS.TX_16X16, 1, 1, 0)[1] == EINVAL
    assert R.lib().rv_tx_blocks_layout(3, 1, 1, 1, 0, None) == EINVAL
    assert b"rv_tx_blocks" in R.lib().rv_last_error()


def test_symbols_exported():
    names = R.exported_symbols_from_header()
    assert "rv_tx_blocks_batch" in names and "rv_tx_blocks_layout" in names
    L = R.lib()
    assert L.rv_tx_blocks_batch and L.rv_tx_blocks_layout
    assert C.sizeof(R.RvTxBlocksParams) == 16 * 4
    assert C.sizeof(R.RvTxBlocksLayout) == (1 + 9 * 3 + 2) * 4 + 2 * 3 * R.TX_BLOCKS_MAX


def test_python_raises_the_job_preconditions():
    """Checked before anything is allocated on a device."""
    class FakePlane:
        def __init__(self, xdec=0, ydec=0):
            self.desc = R.RvPlane()
            d = self.desc
            d.stride, d.alloc_height, d.width, d.height = 192 >> xdec, 192 >> ydec, 160 >> xdec, 152 >> ydec
            d.xorigin, d.yorigin, d.xdec, d.ydec = 16 >> xdec, 16 >> ydec, xdec, ydec
            self.dtype = np.uint8
    planes = [FakePlane(), FakePlane(1, 1), FakePlane(1, 1)]
    tiles = np.array([(16, 8, 128, 128)], R.INTRA_TILE)

    def job(**kw):
        j = np.zeros(1, R.TX_BLOCKS_JOB)
        j["qindex"] = 100
        for k, v in kw.items():
            j[k] = v
        return j
    for bad in (job(tile=1), job(bo_x=-4), job(bo_x=2), job(bo_y=32), job(qindex=0), job(qindex=256)):
        with pytest.raises(R.Rav1eHipError):
            R.tx_blocks_batch(planes, planes, tiles, bad, B.BLOCK_16X16, TS.TX_16X16, PM.DC_PRED)
    with pytest.raises(R.Rav1eHipError):  # the tile leaves the planes
        R.tx_blocks_batch(planes, planes, np.array([(64, 64, 128, 128)], R.INTRA_TILE), job(),
                          B.BLOCK_16X16, TS.TX_16X16, PM.DC_PRED)


# ---------------------------------------------------------------------- GPU
FW, FH = 160, 152
TILE = (16, 8, 128, 128)
TILES = np.array([TILE], R.INTRA_TILE)
QS = (255, 40, 100, 180, 12)  # per-job qindex: get_qidx is per block


@functools.lru_cache(None)
def _planes(bd, fmt, seed):
    """Three random visible planes with saturated regions."""
    xdec, ydec = FMT[fmt]
    rng = np.random.default_rng(7000 * seed + 10 * bd + 2 * xdec + ydec)
    out = []
    for p in range(3):
        w, h = (FW >> xdec, FH >> ydec) if p else (FW, FH)
        maxv = (1 << bd) - 1
        # smooth-ish content plus noise: coefficients of every magnitude
        base = rng.integers(0, maxv + 1, (h // 8 + 2, w // 8 + 2)).repeat(8, 0).repeat(8, 1)[:h, :w]
        a = np.clip(base + rng.integers(-(maxv // 6), maxv // 6 + 1, (h, w)), 0, maxv)
        a[h // 4:h // 2, w // 3:w // 2 + 5] = maxv
        a[h // 2:h // 2 + 7, :w // 6] = 0
        a = a.astype(np.uint16 if bd > 8 else np.uint8)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def _device(planes, fmt, bd):
    xdec, ydec = FMT[fmt]
    return [R.DevicePlane.from_array(a, xpad=16, ypad=16, xdec=xdec if p else 0,
                                     ydec=ydec if p else 0, bit_depth=bd)
            for p, a in enumerate(planes)]


def _jobs(b, limit=20, seed=0):
    """The tile's corners, every edge and interior positions, at most
    `limit`; qindex and alphas vary per job."""
    bw4, bh4 = T.BLK_W[b] // 4, T.BLK_H[b] // 4
    nx, ny = 32 // bw4, 32 // bh4
    xs = sorted({0, 1 % nx, nx // 2, nx - 1})
    ys = sorted({0, 1 % ny, ny // 2, ny - 1})
    pos = [(x, y) for y in ys for x in xs]
    rng = np.random.default_rng(500 + 13 * b + seed)
    while len(pos) < min(limit, nx * ny):
        c = (int(rng.integers(nx)), int(rng.integers(ny)))
        if c not in pos:
            pos.append(c)
    pos = pos[:limit]
    jobs = np.zeros(len(pos), R.TX_BLOCKS_JOB)
    for k, (x, y) in enumerate(pos):
        jobs[k] = (0, x * bw4, y * bh4, QS[k % len(QS)], (3, -7, 16, -16, 1)[k % 5],
                   (-2, 9, -16, 5, -1)[(k + 2) % 5])
    return jobs


def _run(dev, host, jobs, b, ts, lm, cm=0, tt=0, fmt="420", bd=8, dst_fill=None, **kw):
    """One launch against the restatement, bit for bit; returns the
    restatement's per-job results."""
    rec_d, src_d, pred_d = dev
    rec, src, pred = host
    xdec, ydec = FMT[fmt]
    luma_only = kw.get("luma_only", False)
    count = 1 if luma_only else 3
    fill = (1 << bd) - 3
    dst_d = [R.DevicePlane.from_array(np.full_like(a, fill), xpad=16, ypad=16,
                                      xdec=xdec if p else 0, ydec=ydec if p else 0, bit_depth=bd)
             for p, a in enumerate(rec[:count])]
    lay, levels, eobs, dists = R.tx_blocks_batch(rec_d, src_d, TILES, jobs, b, ts, lm, cm, tt,
                                                 bit_depth=bd, pred=pred_d, dst=dst_d, **kw)
    want_dst = [np.full_like(a, fill) for a in rec[:count]]
    refs = []
    for k, j in enumerate(jobs):
        r = T.run_job(rec, src, pred, TILE, int(j["bo_x"]), int(j["bo_y"]), b, ts, tt, lm, cm,
                      int(j["qindex"]), (int(j["alpha_u"]), int(j["alpha_v"])), bd, **kw)
        refs.append(r)
        for p in range(count):
            if p in r.levels:
                assert (levels[p][k] == r.levels[p]).all(), ("levels", k, p, j)
                assert (eobs[p][k] == r.eobs[p]).all(), ("eob", k, p, j, eobs[p][k], r.eobs[p])
                assert (dists[p][k] == r.dists[p]).all(), ("dist", k, p, j)
            else:  # skip: nothing coded
                assert not levels[p][k].any() and not eobs[p][k].any() and not dists[p][k].any()
            if p in r.pixels:
                xd, yd = (xdec, ydec) if p else (0, 0)
                x = (TILE[0] >> xd) + ((int(j["bo_x"]) >> xd) << 2)
                y = (TILE[1] >> yd) + ((int(j["bo_y"]) >> yd) << 2)
                h, w = r.pixels[p].shape
                want_dst[p][y:y + h, x:x + w] = r.pixels[p]
    for p in range(count):
        assert (dst_d[p].download_visible() == want_dst[p]).all(), ("dst", p)
        # rec is never written
        assert (rec_d[p].download_visible() == rec[p]).all()
    return refs


def _setting(bd=8, fmt="420"):
    host = (_planes(bd, fmt, 1), _planes(bd, fmt, 2), _planes(bd, fmt, 3))
    return [_device(h, fmt, bd) for h in host], host


# (luma_mode, chroma_mode): a directional pair, PAETH, CfL with non-zero
# alphas (the jobs'), smooth / H, D207 (bottom-left) with D45 (top-right)
PAIRS = [(PM.DC_PRED, PM.DC_PRED), (PM.D135_PRED, PM.V_PRED), (PM.PAETH_PRED, PM.UV_CFL_PRED),
         (PM.SMOOTH_PRED, PM.PAETH_PRED), (PM.D207_PRED, PM.D45_PRED)]


@pytest.mark.gpu
@pytest.mark.parametrize("recon", [0, 1])
@pytest.mark.parametrize("b", T.SIZES, ids=["%dx%d" % (T.BLK_W[b], T.BLK_H[b]) for b in T.SIZES])
def test_gpu_every_block_size(b, recon):
    """4:2:0 8-bit, luma tx_size = bsize.tx_size(): intra, inter, both skips.
    TX_64X64's 32x32 coded area and the 64x32 / 32x64 types are among them."""
    R.require_device(0)
    dev, host = _setting()
    jobs = _jobs(b, 16)
    ts = bsize_tx(b)
    eobs = []
    for lm, cm in PAIRS:
        if cm == PM.UV_CFL_PRED and b > B.BLOCK_32X32:
            cm = PM.H_PRED
        refs = _run(dev, host, jobs, b, ts, lm, cm, need_recon_pixel=bool(recon))
        eobs += [int(e) for r in refs for p in r.eobs for e in r.eobs[p]]
    refs = _run(dev, host, jobs, b, ts, PM.NEWMV, need_recon_pixel=bool(recon))
    eobs += [int(e) for r in refs for p in r.eobs for e in r.eobs[p]]
    assert max(eobs) > 1  # filled blocks were compared
    _run(dev, host, jobs, b, ts, PM.NEWMV, skip=True, need_recon_pixel=bool(recon))
    _run(dev, host, jobs, b, ts, PM.V_PRED, PM.PAETH_PRED, skip=True, need_recon_pixel=bool(recon))
    _run(dev, host, jobs, b, ts, PM.H_PRED, luma_only=True, need_recon_pixel=bool(recon))


@pytest.mark.gpu
@pytest.mark.parametrize("b,ts", [(B.BLOCK_16X16, TS.TX_8X8), (B.BLOCK_16X16, TS.TX_4X4),
                                  (B.BLOCK_32X16, TS.TX_16X8)], ids=["16x16-8x8", "16x16-4x4",
                                                                      "32x16-16x8"])
def test_gpu_intra_chain(b, ts):
    """Later transform blocks see earlier reconstructions, with the top-right
    and bottom-left availability inside the partition."""
    R.require_device(0)
    dev, host = _setting()
    jobs = _jobs(b, 24)
    for lm, cm in PAIRS + [(PM.D45_PRED, PM.D207_PRED), (PM.D63_PRED, PM.D117_PRED),
                           (PM.SMOOTH_H_PRED, PM.SMOOTH_V_PRED)]:
        refs = _run(dev, host, jobs, b, ts, lm, cm, need_recon_pixel=True)
        # the chain matters: a block's reconstruction differs from its prediction
        assert any(e for r in refs for e in r.eobs[0])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["444", "422"])
def test_gpu_chroma_chain_without_recon(fmt):
    """64x64 without need_recon_pixel: four (4:4:4) / two (4:2:2) 32x32 chroma
    blocks per plane predicted from un-reconstructed neighbours."""
    R.require_device(0)
    dev, host = _setting(8, fmt)
    jobs = _jobs(B.BLOCK_64X64)
    for lm, cm in [(PM.DC_PRED, PM.D45_PRED), (PM.V_PRED, PM.D207_PRED), (PM.H_PRED, PM.PAETH_PRED),
                   (PM.PAETH_PRED, PM.V_PRED)]:
        for recon in (False, True):
            refs = _run(dev, host, jobs, B.BLOCK_64X64, TS.TX_64X64, lm, cm, fmt=fmt,
                        need_recon_pixel=recon)
            assert len(refs[0].eobs[1]) == (4 if fmt == "444" else 2)


LAYOUT_CASES = [(f, bd) for f in ("444", "422") for bd in (8, 10, 12)] + [("420", 10), ("420", 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("b", [B.BLOCK_8X8, B.BLOCK_16X8, B.BLOCK_32X32, B.BLOCK_64X64],
                         ids=["8x8", "16x8", "32x32", "64x64"])
@pytest.mark.parametrize("fmt,bd", LAYOUT_CASES, ids=["%s-%d" % c for c in LAYOUT_CASES])
def test_gpu_layouts_and_depths(fmt, bd, b):
    """8x8 at 4:2:0 gives 4x4 chroma, 64x64 at 4:2:2 two 32x32 chroma blocks
    per plane; non-zero delta_q: the luma quantizer takes ac delta 0 and
    dequantize ac_delta_q[0]."""
    R.require_device(0)
    dev, host = _setting(bd, fmt)
    jobs = _jobs(b, 9)
    ts = bsize_tx(b)
    dq = dict(dc_delta_q=(-3, 5, 2), ac_delta_q=(4, -6, 7))
    cfl = PM.UV_CFL_PRED if b <= B.BLOCK_32X32 else PM.SMOOTH_PRED
    for recon in (False, True):
        _run(dev, host, jobs, b, ts, PM.PAETH_PRED, cfl, fmt=fmt, bd=bd, need_recon_pixel=recon, **dq)
        _run(dev, host, jobs, b, ts, PM.D63_PRED, PM.D153_PRED, fmt=fmt, bd=bd,
             need_recon_pixel=recon, **dq)
        _run(dev, host, jobs, b, ts, PM.GLOBALMV, fmt=fmt, bd=bd, need_recon_pixel=recon, **dq)


# TxType -> 1-D kinds of the columns / rows (src/transform/mod.rs:158-219): 0 Id,
# 1 Dct, 2 Adst, 3 FlipAdst
TX_COL = [1, 2, 1, 2, 3, 1, 3, 2, 3, 0, 1, 0, 2, 0, 3, 0]
TX_ROW = [1, 1, 2, 2, 1, 3, 3, 3, 2, 0, 0, 1, 0, 2, 0, 3]


def _type_taken(ts, tt, recon):
    """What the reference's transforms implement: Id up to 32 points, Adst /
    FlipAdst up to 16, no flipped rows forward, no FlipAdst in the native
    inverse."""
    def fwd(kind, n):
        return n <= 32 if kind == 0 else True if kind == 1 else n <= 16
    ck, rk = TX_COL[tt], TX_ROW[tt]
    ok = rk != 3 and fwd(ck, T.TX_H[ts]) and fwd(rk, T.TX_W[ts])
    return ok and not (recon and 3 in (ck, rk))


@pytest.mark.gpu
@pytest.mark.parametrize("b", [B.BLOCK_8X8, B.BLOCK_16X16, B.BLOCK_16X32], ids=["8x8", "16x16", "16x32"])
def test_gpu_transform_types(b):
    """Every luma type the transforms implement for the size, flipped columns
    included (those without the inverse); an inter job's chroma takes the luma
    type."""
    R.require_device(0)
    dev, host = _setting()
    jobs = _jobs(b, 8)
    ts = bsize_tx(b)
    ran = 0
    for tt in range(1, 16):
        if _type_taken(ts, tt, True):
            _run(dev, host, jobs, b, ts, PM.V_PRED, PM.H_PRED, tt=tt)
            _run(dev, host, jobs, b, ts, PM.NEARESTMV, tt=tt)
        elif _type_taken(ts, tt, False):
            _run(dev, host, jobs, b, ts, PM.DC_PRED, PM.DC_PRED, tt=tt, need_recon_pixel=False)
        else:
            continue
        ran += 1
    assert ran >= 3


@functools.lru_cache(None)
def _uv_type_setting():
    """Inter 16x16 with ADST_ADST: half the jobs predicted within +-1 of the
    source at qindex 255 (luma eob 0), half from a random plane."""
    bd, fmt = 8, "420"
    rec, src, rnd = _planes(bd, fmt, 1), _planes(bd, fmt, 2), _planes(bd, fmt, 3)
    jobs = _jobs(B.BLOCK_16X16, 24)
    rng = np.random.default_rng(99)
    pred = [a.copy() for a in rnd]
    for k, j in enumerate(jobs):
        if k % 2:
            continue
        jobs["qindex"][k] = 255
        for p in range(3):
            xd, yd = FMT[fmt] if p else (0, 0)
            x = (TILE[0] >> xd) + ((int(j["bo_x"]) >> xd) << 2)
            y = (TILE[1] >> yd) + ((int(j["bo_y"]) >> yd) << 2)
            w, h = 16 >> xd, 16 >> yd
            s = src[p][y:y + h, x:x + w].astype(np.int64)
            pred[p][y:y + h, x:x + w] = np.clip(s + rng.choice((-1, 1), (h, w)), 0, 255)
    return (rec, src, tuple(pred)), jobs


def _uv_branches(refs):
    return {bool(r.eobs[0][0]) for r in refs}, {r.uv_tx_type for r in refs}


def test_uv_tx_type_both_branches_on_the_reference_side():
    """The seed's choice, checked without a GPU: the restatement alone sees
    empty and non-empty luma blocks and both chroma types."""
    host, jobs = _uv_type_setting()
    refs = [T.run_job(*host, TILE, int(j["bo_x"]), int(j["bo_y"]), B.BLOCK_16X16, TS.TX_16X16,
                      TT.ADST_ADST, PM.NEWMV, 0, int(j["qindex"]), (0, 0), 8, need_recon_pixel=False,
                      coeff_rate=True) for j in jobs]
    assert _uv_branches(refs) == ({False, True}, {int(TT.DCT_DCT), int(TT.ADST_ADST)})


@pytest.mark.gpu
def test_gpu_inter_uv_tx_type_branch():
    R.require_device(0)
    host, jobs = _uv_type_setting()
    dev = [_device(h, "420", 8) for h in host]
    for recon in (False, True):
        refs = _run(dev, host, jobs, B.BLOCK_16X16, TS.TX_16X16, PM.NEWMV, tt=TT.ADST_ADST,
                    need_recon_pixel=recon, coeff_rate=True)
        assert _uv_branches(refs) == ({False, True}, {int(TT.DCT_DCT), int(TT.ADST_ADST)})
    # without a coefficient rate and without reconstruction has_coeff is always true
    refs = _run(dev, host, jobs, B.BLOCK_16X16, TS.TX_16X16, PM.NEWMV, tt=TT.ADST_ADST,
                need_recon_pixel=False, coeff_rate=False)
    assert _uv_branches(refs) == ({False, True}, {int(TT.ADST_ADST)})


@pytest.mark.gpu
def test_gpu_qindex_per_job_and_independence():
    """One launch mixes qindex values; the same jobs in another order give the
    same per-job results; rec is unchanged byte for byte (in _run)."""
    R.require_device(0)
    dev, host = _setting()
    b, ts = B.BLOCK_16X16, TS.TX_8X8
    jobs = _jobs(b, 40)
    assert len(set(jobs["qindex"].tolist())) >= 3
    _run(dev, host, jobs, b, ts, PM.D45_PRED, PM.UV_CFL_PRED)
    perm = np.random.default_rng(5).permutation(len(jobs))
    full_before = [d.download_full() for d in dev[0]]
    a = R.tx_blocks_batch(dev[0], dev[1], TILES, jobs, b, ts, PM.D45_PRED, PM.UV_CFL_PRED)
    c = R.tx_blocks_batch(dev[0], dev[1], TILES, jobs[perm], b, ts, PM.D45_PRED, PM.UV_CFL_PRED)
    for k in range(1, 4):
        for p in range(3):
            assert (a[k][p][perm] == c[k][p]).all()
    for before, d in zip(full_before, dev[0]):
        assert (d.download_full() == before).all()  # the padding too


@pytest.mark.gpu
def test_gpu_argument_errors():
    """Every RV_EINVAL / RV_ENOTSUP case returns before a launch."""
    R.require_device(0)
    dev, host = _setting()
    rec, src, pred = ([(R.RvPlane * 3)(*[p.desc for p in d]) for d in dev])
    jobs = R.DeviceBuffer.from_array(_jobs(B.BLOCK_16X16, 4))
    tiles = R.DeviceBuffer.from_array(TILES)
    out = [R.DeviceBuffer(1 << 16) for _ in range(3)]
    for o in out:
        o.zero()

    def call(bsize=B.BLOCK_16X16, ts=TS.TX_16X16, tt=0, lm=0, cm=0, recon=1, bd=8, rec=rec, src=src,
             pred=pred, dst=None, jobs=jobs.ptr, tiles=tiles.ptr, n_tiles=1, n=4, levels=out[0].ptr,
             luma_only=0, prm=True):
        p = R.RvTxBlocksParams(int(bsize), int(ts), int(tt), int(lm), int(cm), 0, luma_only, recon, 1,
                               bd)
        return R.lib().rv_tx_blocks_batch(rec, src, pred, dst, tiles, n_tiles, jobs, n,
                                          C.byref(p) if prm else None, levels, out[1].ptr,
                                          out[2].ptr, None)
    for b in (B.BLOCK_4X4, B.BLOCK_4X8, B.BLOCK_8X4, B.BLOCK_4X16, B.BLOCK_16X4, B.BLOCK_8X32,
              B.BLOCK_32X8, B.BLOCK_16X64, B.BLOCK_64X16, B.BLOCK_128X128):
        assert call(bsize=b, ts=TS.TX_4X4) == ENOTSUP
    assert call(bsize=22) == EINVAL and call(ts=19) == EINVAL and call(tt=16) == EINVAL
    assert call(ts=TS.TX_32X32) == EINVAL                       # larger than the partition
    assert call(bsize=B.BLOCK_64X64, ts=TS.TX_64X64, cm=13) == EINVAL  # CfL above 32x32
    assert call(bsize=B.BLOCK_64X64, ts=TS.TX_64X64, tt=TT.ADST_DCT) == EINVAL
    assert call(bsize=B.BLOCK_64X64, ts=TS.TX_64X16, tt=TT.DCT_ADST) == EINVAL
    assert call(bsize=B.BLOCK_32X32, ts=TS.TX_32X32, tt=TT.ADST_ADST) == ENOTSUP  # no 32-point ADST
    assert call(tt=TT.DCT_FLIPADST) == ENOTSUP                  # no flipped row transform
    assert call(tt=TT.FLIPADST_DCT) == ENOTSUP                  # the inverse has no FlipAdst ...
    assert call(lm=PM.NEWMV, ts=TS.TX_8X8) == EINVAL            # inter: tx_size.block_size() == bsize
    assert call(lm=PM.NEWMV, pred=None) == EINVAL
    assert call(ts=TS.TX_8X8, recon=0) == EINVAL                # encode_tx_block's debug_assert
    assert call(lm=13) == EINVAL and call(lm=28) == EINVAL and call(cm=14) == EINVAL
    assert call(bd=9) == EINVAL and call(bd=10) == EINVAL      # u8 planes
    assert call(rec=None) == EINVAL and call(src=None) == EINVAL and call(prm=False) == EINVAL
    assert call(jobs=None) == EINVAL and call(tiles=None) == EINVAL and call(n_tiles=0) == EINVAL
    assert call(levels=None) == EINVAL and call(n=-1) == EINVAL
    assert call(dst=rec) == EINVAL                              # dst aliases rec
    assert b"rv_tx_blocks_batch" in R.lib().rv_last_error()
    mixed = (R.RvPlane * 3)(dev[0][0].desc, dev[0][1].desc, dev[0][0].desc)
    assert call(rec=mixed) == EINVAL                            # plane sets of different subsampling
    # 4:2:2 has no subsampled size for the 1:2 blocks
    d422 = [_device(h, "422", 8) for h in (_planes(8, "422", 1),)][0]
    p422 = (R.RvPlane * 3)(*[p.desc for p in d422])
    assert call(bsize=B.BLOCK_8X16, ts=TS.TX_8X16, rec=p422, src=p422, pred=p422) == ENOTSUP
    assert call(n=0, jobs=None, tiles=None, levels=None) == 0   # nothing to do is not an error
    # no launch happened: the outputs were never written
    assert not any(o.download(np.uint8).any() for o in out)
    assert call(tt=TT.FLIPADST_DCT, recon=0) == 0               # without the inverse it is taken
    assert call() == 0
    assert out[2].download(np.uint64, 12).any()

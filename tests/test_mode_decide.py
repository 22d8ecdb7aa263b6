"""A block's mode decision on the device (rv_mode_decide.hip, rav1e_amd.
mode_decide_batch / block_segments_batch / segmentation_data): a candidate's
ScaledDistortion, compute_rd_cost, the walk of rdo_mode_decision with its
early-outs, the winner (src/rdo.rs:338-568, 634-780, 784-1259).

CPU: tests/mode_decide_ref.py (the numpy restatement, the GPU tests' checker)
against the vectors the reference's own text produced (tools/refeval/
gen_mode_decide_ref.py -> tests/golden/ref_mode_decide.npz); every error code
without a device; the exports; rv_segmentation_data.  GPU: every output word
against the restatement, tolerance 0.

The GPU setting: a 68x36 luma frame (w_in_b = 17, h_in_b = 9) in planes padded
by 64, tiles (0, 0, 64, 64) and (64, 0, 64, 64): a block at the second tile's
origin has its importance area clipped at the frame's right edge while the
divisor stays the full area, and a block further right lies outside it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rav1e_amd as R
from tests import mode_decide_ref as M
from tests import tx_blocks_ref as T

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_mode_decide.npz")
B, TS, PM = R.BlockSize, R.TxSize, R.PredictionMode
EINVAL, ENOTSUP = R.RV_EINVAL, R.RV_ENOTSUP
FMT = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}
FW, FH, PAD = 68, 36, 64
W_IN_B, H_IN_B = 17, 9
TILE_LIST = [(0, 0, 64, 64), (64, 0, 64, 64)]
TILES = np.array(TILE_LIST, R.INTRA_TILE)
SCALE = (0.9375, 1.28125, 1.6171875)
LAMBDA = 37.5
SIZES = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12]  # the ten sizes rv_tx_blocks_batch takes


def block_tx(b):
    return next(t for t in range(19) if (M.TX_W[t], M.TX_H[t]) == (M.BLK_W[b], M.BLK_H[b]))


@functools.lru_cache(None)
def gold():
    return dict(np.load(GOLD))


# ------------------------------------------------------------ CPU: the vectors
def test_checker_importance_and_bias_equal_reference():
    g = gold()
    fr = M.Frame(int(g["frame"][0]), int(g["frame"][1]), g["importance"])
    assert len(g["bias_cases"]) > 100
    for (b, x, y), mean, bias in zip(g["bias_cases"], g["bias_mean"], g["bias_value"]):
        mw, mh = M.BLK_W[b] // 4, M.BLK_H[b] // 4
        got = M.mean_importance(fr, int(x), int(y), mw, mh)
        assert got.dtype == np.float32 and got == mean, (b, x, y)
        assert M.distortion_bias(fr, int(x), int(y), mw, mh) == bias, (b, x, y)
    # the cases the contract names: a clipped area divided by the full one, an area outside
    cases = {tuple(c): m for c, m in zip(g["bias_cases"].tolist(), g["bias_mean"])}
    imp = g["importance"]
    assert cases[(6, 16, 8)] == np.float32(imp[4, 8] / np.float32(16))
    assert cases[(3, 18, 10)] == 0


def test_checker_mul_and_rd_cost_equal_reference():
    g = gold()
    assert len(g["mul_value"]) > 200 and len(g["rd_cost"]) == 40
    for v, f, raw, dist in zip(g["mul_value"], g["mul_factor"], g["mul_raw"], g["mul_dist"]):
        assert M.mul(int(v), float(f)) == int(raw) == int(dist), (v, f)
    assert int(g["mul_raw"].max()) == (1 << 64) - 1  # the saturating cast occurs
    fr = M.Frame(1, 1)
    for rate, dist, lam, want in zip(g["rd_rate"], g["rd_dist"], g["rd_lambda"], g["rd_cost"]):
        fr.lambda_ = float(lam)
        assert M.rd_cost(fr, int(rate), int(dist)) == want
    for (b, x, y, p, d), want in zip(g["txb_cases"], g["txb_value"]):
        fr = M.Frame(int(g["frame"][0]), int(g["frame"][1]), g["importance"], dist_scale=g["txb_scale"])
        bias = M.distortion_bias(fr, int(x), int(y), M.BLK_W[b] // 4, M.BLK_H[b] // 4)
        assert M.mul(M.mul(int(d), bias), fr.dist_scale[p]) == int(want)


def test_checker_distortions_equal_reference():
    """compute_distortion and compute_tx_distortion's skip arm, run whole."""
    g = gold()
    w_in_b, h_in_b, _, fw, fh, pad = (int(v) for v in g["frame"])
    seen = set()
    planes = {}
    for row, want in zip(g["dist_cases"].tolist(), g["dist_value"]):
        si, b, ti, bo_x, bo_y, tune, kind = row[:7]
        bd, xdec, ydec = (int(v) for v in g["settings"][si])
        if si not in planes:
            src = M.synth_planes(si, bd, xdec, ydec, fw, fh, pad)
            planes[si] = (src, M.synth_planes(si + 100, bd, xdec, ydec, fw, fh, pad, noise_of=src))
        src, rec = planes[si]
        fr = M.Frame(w_in_b, h_in_b, g["importance"], dist_scale=[v / 1e7 for v in row[7:10]],
                     bit_depth=bd, psy=tune == 1, use_tx=kind == 1)
        got = M.pixel_distortion(fr, src, rec, tuple(g["tiles"][ti]), bo_x, bo_y, b, xdec, ydec,
                                 luma_sse=kind == 1)
        assert got == int(want), row
        seen.add((bd, xdec, ydec, b, tune, kind))
    assert len(seen) >= 40 and len(g["dist_value"]) > 100
    # 8x8 at 4:2:0 is there with both tunes: 2x2 chroma sub-blocks biased as BLOCK_4X4
    assert (8, 1, 1, 3, 0, 0) in seen and (8, 1, 1, 3, 1, 0) in seen and (8, 1, 0, 3, 1, 0) in seen


def test_tx_layout_equals_the_library_layout():
    """The checker's transform-block counts and sizes are rv_tx_blocks_layout's."""
    for b in SIZES:
        for fmt, (xdec, ydec) in FMT.items():
            for ts in range(19):
                if M.TX_W[ts] > M.BLK_W[b] or M.TX_H[ts] > M.BLK_H[b]:
                    continue
                if T.check_args(b, ts, xdec, ydec, 0) != 0:
                    continue
                lay = R.tx_blocks_layout(b, ts, xdec, ydec)
                for p, (tw, th, cols, rows) in enumerate(M.tx_layout(b, ts, xdec, ydec)):
                    assert (cols, rows) == (lay.cols[p], lay.rows[p]), (b, ts, fmt, p)
                    assert (tw, th) == (M.TX_W[lay.tx_size[p]], M.TX_H[lay.tx_size[p]])
                assert M.n_tx_blocks(b, ts, xdec, ydec) == lay.blocks_per_job


# ------------------------------------------------------------- CPU: the walk
def _row(group, flags, rate, dist, lam=8.0, hc=True, rejected=False):
    return (group, flags, rate, dist, float(dist) + lam * (rate / 8.0), hc, rejected)


def test_walk_hand_built_lists():
    S, I = M.SKIP, M.INTRA
    E, GZ, GS = M.EVALUATED, M.GATED_ZERO_DIST, M.GATED_SKIP
    # two equal candidates: the first wins
    best, st = M.walk([_row(0, 0, 100, 50), _row(1, 0, 100, 50)])
    assert best.cand == 0 and st == [E, E]
    assert M.walk([_row(0, 0, 100, 50), _row(1, 0, 100, 50)], replace_on_equal=True)[0].cand == 1
    # a skip candidate with zero distortion that replaces best: its group's non-skip is gated out
    best, st = M.walk([_row(0, S, 10, 0), _row(0, 0, 5, 0)])
    assert best.cand == 0 and best.skip and st == [E, GZ]
    # a zero-distortion skip candidate that does not replace best: the non-skip is evaluated
    rows = [_row(0, S, 8, 0), _row(0, 0, 1, 7), _row(1, S, 50, 0), _row(1, 0, 1, 3)]
    best, st = M.walk(rows)
    assert st == [E, GZ, E, E] and best.cand == 3
    assert M.walk(rows, zero_from_any_skip=True)[1] == [E, GZ, E, GZ]
    # a winning skip candidate: intra groups are gated out
    best, st = M.walk([_row(0, S, 8, 0), _row(0, 0, 1, 0), _row(1, I, 1, 0), _row(2, I, 1, 0)])
    assert best.cand == 0 and st == [E, GZ, GS, GS]
    # an intra winner
    best, st = M.walk([_row(0, S, 4000, 9), _row(0, 0, 3000, 9), _row(1, I, 10, 0)])
    assert best.cand == 2 and not best.skip and st == [E, E, E]
    # an empty list, a seed that stays, a seed that is replaced
    assert M.walk([]) == (None, [])
    assert M.walk([_row(0, I, 10, 5)], seed=(15.0, False))[0] is None  # 15 < 15 is false
    assert M.walk([_row(0, I, 10, 4)], seed=(15.0, False))[0].cand == 0
    assert M.walk([_row(0, I, 10, 4)], seed=(15.0, True))[1] == [GS]
    # a rejected candidate is passed over and starts no group
    best, st = M.walk([_row(0, S, 8, 0), _row(0, 0, 1, 0, rejected=True), _row(0, 0, 1, 0)])
    assert st == [E, M.REJECTED, GZ]


def test_walk_equals_the_transliterated_control_flow():
    """300 random lists in the reference's order through the generator's
    transliteration of rdo_mode_decision / luma_chroma_mode_rdo (nested
    closures, the intra gate once) against the checker's flat loop."""
    g = gold()
    off, rows, cost = g["walk_off"], g["walk_rows"], g["walk_cost"]
    assert len(off) == 301
    gated = {M.GATED_ZERO_DIST: 0, M.GATED_SKIP: 0}
    ties = 0
    for i, win in enumerate(g["walk_winner"]):
        r = rows[off[i]:off[i + 1]]
        c = cost[off[i]:off[i + 1]]
        lst = [(int(a[0]), int(a[1]), int(a[2]), int(a[3]), float(co), True, False) for a, co in zip(r, c)]
        best, states = M.walk(lst)
        assert (best.cand if best else -1) == int(win), i
        assert [s == M.EVALUATED for s in states] == [bool(a[4]) for a in r], i
        for s in states:
            if s in gated:
                gated[s] += 1
        ties += best is not None and (c == best.rd_cost).sum() > 1
        for a, co in zip(r, c):  # compute_rd_cost with lambda 2.5
            assert co == float(a[3]) + 2.5 * (float(a[2]) / 8.0)
    assert gated[M.GATED_ZERO_DIST] > 20 and gated[M.GATED_SKIP] > 20 and ties > 10


# ------------------------------------------------------- CPU: the C interface
def test_symbols_and_records():
    names = R.exported_symbols_from_header()
    L = R.lib()
    for n, nargs in (("rv_segmentation_data", 2), ("rv_block_segment_batch", 16),
                     ("rv_mode_decide_check", 7), ("rv_mode_decide_batch", 22),
                     ("rv_mode_decide_batch_lanes", 23)):
        assert n in names and len(getattr(L, n).argtypes) == nargs, n
        hdr = open(R.HEADER_PATH).read()
        decl = hdr[hdr.index("int %s(" % n):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs, n
    assert R.MODE_PAYLOAD.itemsize == 40 and R.MODE_CAND.itemsize == 68
    assert R.MODE_BLOCK.itemsize == 20 and R.MODE_DECISION.itemsize == 80
    assert C.sizeof(R.RvModeDecideParams) == 8 * 4 + 4 * 8
    assert (R.MODE_CAND_SKIP, R.MODE_CAND_INTRA, R.MODE_CAND_NEED_RECON_PIXEL) == (M.SKIP, M.INTRA, M.NEED_RECON)
    assert (R.MODE_STATE_EVALUATED, R.MODE_STATE_GATED_ZERO_DIST, R.MODE_STATE_GATED_SKIP,
            R.MODE_STATE_REJECTED) == (M.EVALUATED, M.GATED_ZERO_DIST, M.GATED_SKIP, M.REJECTED)
    assert R.RD_COST_MAX == M.RD_MAX
    rec = np.zeros(1, R.MODE_DECISION)[0]
    rec["cand"], rec["rd_cost"], rec["pay"]["luma_mode"], rec["pay"]["mvs"] = 3, 2.5, 13, [[1, -2], [3, 4]]
    d = R.ModeDecision.from_record(rec)
    assert (d.cand, d.rd_cost, d.pred_mode_luma, d.mvs) == (3, 2.5, 13, ((1, -2), (3, 4)))


def test_segmentation_data():
    for q, want in ((1, [0, 21, 0]), (21, [0, 21, -20]), (22, [0, 21, -21]), (255, [0, 21, -21])):
        assert R.segmentation_data(q).tolist() == want == M.segmentation_data(q)
    out = (C.c_int16 * 3)()
    assert R.lib().rv_segmentation_data(-1, out) == EINVAL
    assert R.lib().rv_segmentation_data(256, out) == EINVAL
    assert R.lib().rv_segmentation_data(100, None) == EINVAL
    with pytest.raises(R.Rav1eHipError) as e:
        R.segmentation_data(300)
    assert e.value.code == EINVAL


def _fake_sets(n, base, fmt="420", hbd=0, **change):
    """n plane sets of descriptors whose data pointers are never dereferenced."""
    xdec, ydec = FMT[fmt]
    arr = (R.RvPlane * (3 * n))()
    for s in range(n):
        for p in range(3):
            d = arr[3 * s + p]
            xd, yd = (xdec, ydec) if p else (0, 0)
            R.lib().rv_plane_geometry(C.byref(d), FW >> xd, FH >> yd, xd, yd, PAD, PAD, hbd)
            d.data = base + (3 * s + p) * (1 << 20)
    for k, v in change.items():
        setattr(arr[1], k, v)
    return arr


def _params(bsize=B.BLOCK_16X16, bd=8, tune=0, use_tx=0, coeff_rate=1, w_in_b=W_IN_B, h_in_b=H_IN_B,
            w_imp=9):
    p = R.RvModeDecideParams(int(bsize), bd, tune, use_tx, coeff_rate, w_in_b, h_in_b, w_imp, LAMBDA)
    for k in range(3):
        p.dist_scale[k] = SCALE[k]
    return p


def test_every_error_code_without_a_device():
    L = R.lib()
    fake = C.c_void_p(0x1000)

    def check(fmt="420", hbd=0, src=None, cands=None, commit=None, n_sets=2, has_imp=1, lanes=0,
              params=True, **kw):
        src = _fake_sets(1, 0x10000000, fmt, hbd) if src is None else src
        cands = _fake_sets(2, 0x20000000, fmt, hbd) if cands is None else cands
        prm = _params(**kw)
        return L.rv_mode_decide_check(src, cands, n_sets, commit, C.byref(prm) if params else None,
                                      has_imp, lanes)
    assert check() == 0
    assert check(commit=_fake_sets(1, 0x30000000)) == 0
    for b in SIZES:
        assert check(bsize=b) == 0
        assert check(bsize=b, fmt="444", tune=1) == 0
    # the sizes, layouts and depths of rv_tx_blocks_batch, with its codes
    for b in (B.BLOCK_4X4, B.BLOCK_4X8, B.BLOCK_8X4, B.BLOCK_4X16, B.BLOCK_16X4, B.BLOCK_64X16,
              B.BLOCK_64X128, B.BLOCK_128X128):
        assert check(bsize=b) == ENOTSUP
    for b in (B.BLOCK_8X16, B.BLOCK_16X32, B.BLOCK_32X64):
        assert check(bsize=b, fmt="422") == ENOTSUP and check(bsize=b, fmt="420") == 0
    assert check(bsize=-1) == EINVAL and check(bsize=22) == EINVAL
    assert check(bd=9) == EINVAL and check(bd=10) == EINVAL and check(bd=10, hbd=1) == 0
    assert check(bd=12, hbd=1) == 0 and check(bd=8, hbd=1) == EINVAL
    # tune and the tx-domain assert
    assert check(tune=2) == EINVAL and check(tune=-1) == EINVAL
    assert check(tune=1, use_tx=1) == EINVAL and check(tune=0, use_tx=1) == 0
    assert b"rv_mode_decide_batch" in L.rv_last_error()
    # plane sets
    assert check(n_sets=0) == EINVAL and check(n_sets=21) == EINVAL
    assert check(cands=_fake_sets(2, 0x20000000, "444")) == EINVAL
    assert check(cands=_fake_sets(2, 0x20000000, stride=512)) == EINVAL
    assert check(cands=_fake_sets(2, 0x20000000, yorigin=8)) == EINVAL
    assert check(commit=_fake_sets(1, 0x30000000, alloc_height=400)) == EINVAL
    assert check(commit=_fake_sets(1, 0x20000000 + 3 * (1 << 20))) == EINVAL   # commit is set 1
    assert check(commit=_fake_sets(1, 0x20000000 + 64)) == EINVAL              # a partial overlap
    nul = _fake_sets(2, 0x20000000)
    nul[4].data = None
    assert check(cands=nul) == EINVAL
    odd = _fake_sets(1, 0x10000000)
    odd[1].xdec, odd[1].ydec = 0, 1
    odd[2].xdec, odd[2].ydec = 0, 1
    assert check(src=odd) == EINVAL                                             # 4:4:0
    assert check(params=False) == EINVAL
    assert L.rv_mode_decide_check(None, _fake_sets(2, 0x20000000), 2, None, C.byref(_params()), 0, 0) == EINVAL
    # the frame
    assert check(w_in_b=0) == EINVAL and check(h_in_b=0) == EINVAL
    assert check(w_imp=8) == EINVAL and check(w_imp=8, has_imp=0) == 0
    # lanes: a power of two 8 .. 256, and enough of them for the LDS
    assert check(lanes=4) == EINVAL and check(lanes=48) == EINVAL and check(lanes=512) == EINVAL
    assert check(lanes=8) == 0 and check(lanes=256) == 0
    assert check(bsize=B.BLOCK_64X64, lanes=32, fmt="444") == EINVAL
    # the launch itself: counts and device pointers, refused before any HIP call
    src, cands, prm = _fake_sets(1, 0x10000000), _fake_sets(2, 0x20000000), _params()

    def launch(n=1, n_tiles=1, n_cands=1, n_tx=1, tiles=fake, blocks=fake, cl=fake, dist=fake, eob=fake,
               out=fake, cd=fake, cc=fake, cs=fake, status=fake):
        return L.rv_mode_decide_batch(src, cands, 2, None, tiles, n_tiles, blocks, n, cl, n_cands, None,
                                      dist, eob, n_tx, None, C.byref(prm), out, cd, cc, cs, status, None)
    assert launch(n=-1) == EINVAL and launch(n_cands=-1) == EINVAL and launch(n_tx=-1) == EINVAL
    assert launch(n_tiles=-1) == EINVAL and launch(n_tiles=0) == EINVAL
    for name in ("tiles", "blocks", "cl", "dist", "eob", "out", "cd", "cc", "cs", "status"):
        assert launch(**{name: None}) == EINVAL, name
    # block segments
    dq = (C.c_int16 * 3)(0, 21, -21)

    def seg(bsize=6, q=100, w_in_b=17, h_in_b=9, w_imp=9, imp=fake, n=1, data=dq, status=fake, tiles=fake):
        return L.rv_block_segment_batch(tiles, 1, fake, n, bsize, q, data, imp, w_imp, w_in_b, h_in_b,
                                        fake, fake, fake, status, None)
    assert seg(bsize=-1) == EINVAL and seg(bsize=22) == EINVAL and seg(bsize=13) == ENOTSUP
    assert seg(bsize=21) == ENOTSUP and seg(q=-1) == EINVAL and seg(q=256) == EINVAL
    assert seg(w_in_b=0) == EINVAL and seg(w_imp=8) == EINVAL and seg(n=-1) == EINVAL
    assert seg(data=None) == EINVAL and seg(status=None) == EINVAL and seg(tiles=None) == EINVAL
    assert b"rv_block_segment_batch" in L.rv_last_error()


def test_python_raises_the_codes_before_allocating():
    class FakePlane:
        def __init__(self, xdec=0, ydec=0, base=0x1000000):
            self.desc = R.RvPlane()
            R.lib().rv_plane_geometry(C.byref(self.desc), FW >> xdec, FH >> ydec, xdec, ydec, PAD, PAD, 0)
            self.desc.data = base
    src = [FakePlane(0, 0, 0x1000000), FakePlane(1, 1, 0x2000000), FakePlane(1, 1, 0x3000000)]
    sets = [[FakePlane(0, 0, 0x4000000), FakePlane(1, 1, 0x5000000), FakePlane(1, 1, 0x6000000)]]
    blocks, cands = np.zeros(1, R.MODE_BLOCK), np.zeros(1, R.MODE_CAND)

    def call(bsize=B.BLOCK_16X16, **kw):
        with pytest.raises(R.Rav1eHipError) as e:
            R.mode_decide_batch(src, sets, TILES, blocks, cands, bsize, LAMBDA, SCALE, W_IN_B, H_IN_B, **kw)
        return getattr(e.value, "code", None)
    assert call(B.BLOCK_4X8) == ENOTSUP and call(B.BLOCK_64X16) == ENOTSUP and call(22) == EINVAL
    assert call(tune=R.Tune.Psychovisual, use_tx_domain_distortion=True) == EINVAL
    assert call(bit_depth=10) == EINVAL and call(lanes=3) == EINVAL
    assert call(importance=np.zeros((5, 8), np.float32)) == EINVAL
    assert call(commit=sets[0]) == EINVAL
    with pytest.raises(R.Rav1eHipError) as e:
        R.block_segments_batch(TILES, blocks, B.BLOCK_16X64, 100, W_IN_B, H_IN_B)
    assert e.value.code == ENOTSUP
    with pytest.raises(R.Rav1eHipError) as e:
        R.block_segments_batch(TILES, blocks, B.BLOCK_16X16, 256, W_IN_B, H_IN_B)
    assert e.value.code == EINVAL


# ---------------------------------------------------------------------- GPU
def _host_planes(seed, bd, fmt, noise_of=None):
    xdec, ydec = FMT[fmt]
    return M.synth_planes(seed, bd, xdec, ydec, FW, FH, PAD, noise_of=noise_of)


def _device(planes, bd, fmt):
    xdec, ydec = FMT[fmt]
    out = []
    for p, (a, xo, yo) in enumerate(planes):
        xd, yd = (xdec, ydec) if p else (0, 0)
        d = R.DevicePlane.from_full(a.astype(np.uint8) if bd == 8 else a, xo, yo, FW >> xd, FH >> yd,
                                    bit_depth=bd)
        d.desc.xdec, d.desc.ydec = xd, yd
        out.append(d)
    return out


def _importance(seed):
    rng = np.random.default_rng(seed)
    imp = (rng.random((5, 9)) * 6).astype(np.float32)
    imp[0, 0] = 0
    return imp


def _positions(b, limit=6):
    """(tile, bo_x, bo_y): the first tile's corners, the second tile's origin
    (the importance area clipped at w_in_b) and, where the size allows, a block
    wholly right of the frame."""
    bw4, bh4 = M.BLK_W[b] // 4, M.BLK_H[b] // 4
    nx, ny = 16 // bw4, 16 // bh4
    pos = [(0, 0, 0), (1, 0, 0), (0, (nx - 1) * bw4, (ny - 1) * bh4)]
    if nx > 1:
        pos += [(1, bw4, 0), (0, bw4, 0)]
    if ny > 1:
        pos += [(0, 0, bh4), (1, 0, (ny - 1) * bh4)]
    return pos[:limit]


def _cand(group, flags, set_, rate, ts, off=0, **pay):
    c = np.zeros(1, R.MODE_CAND)[0]
    c["group"], c["flags"], c["set"], c["rate"], c["tx_size"] = group, flags, set_, rate, ts
    c["dist_off"] = c["eob_off"] = off
    for k, v in pay.items():
        c["pay"][k] = v
    return c


def _compare(res, fr, src, sets, blocks, cands, b, fmt, tx_dist=None, tx_eob=None, seed=None, **mut):
    """Every output word of a launch against the checker; returns the
    checker's (best, dists, costs, states) per block."""
    xdec, ydec = FMT[fmt]
    out = []
    seen = np.zeros(len(cands), bool)
    for i, blk in enumerate(blocks):
        f, n = int(blk["cand_first"]), int(blk["cand_count"])
        sd = None if seed is None else (float(seed[i]["rd_cost"]), bool(seed[i]["skip"]))
        best, dists, costs, states = M.decide_block(
            fr, src, sets, TILE_LIST[int(blk["tile"])], (int(blk["bo_x"]), int(blk["bo_y"])),
            cands[f:f + n], b, xdec, ydec, tx_dist, tx_eob, sd)
        out.append((best, dists, costs, states))
        seen[f:f + n] = True
        assert res.cand_state[f:f + n].tolist() == states, ("state", i)
        assert res.cand_dist[f:f + n].tolist() == dists, ("dist", i, res.cand_dist[f:f + n], dists)
        assert res.cand_cost[f:f + n].tolist() == costs, ("cost", i)
        d = res.decisions[i]
        if best is None:
            want = np.zeros(1, R.MODE_DECISION)[0] if seed is None else seed[i].copy()
            if seed is None:
                want["rd_cost"] = M.RD_MAX
            want["cand"] = -1
            assert d.tobytes() == want.tobytes(), ("no winner", i, d, want)
        else:
            c = cands[f + best.cand]
            assert (int(d["cand"]), float(d["rd_cost"]), int(d["distortion"]), int(d["rate"])) == \
                (f + best.cand, best.rd_cost, best.distortion, best.rate), ("winner", i, d, best)
            assert (int(d["skip"]), int(d["has_coeff"]), int(d["tx_size"]), int(d["reserved"])) == \
                (int(best.skip), int(best.has_coeff), int(c["tx_size"]), 0), ("flags", i, d, best)
            assert d["pay"].tobytes() == c["pay"].tobytes(), ("payload", i)
    assert not res.cand_state[~seen].any()
    return out


@pytest.mark.gpu
def test_gpu_block_segments():
    R.require_device(0)
    below2, below4 = np.nextafter(np.float32(2), np.float32(0)), np.nextafter(np.float32(4), np.float32(0))
    want_interior = {0.0: 1, float(below2): 1, 2.0: 0, float(below4): 0, 4.0: 2, 1000.0: 2}
    planes = [np.full((5, 9), v, np.float32) for v in want_interior] + [_importance(3), None]
    seen = set()
    for b in SIZES:
        blocks = np.zeros(len(_positions(b, 7)), R.MODE_BLOCK)
        for k, (t, x, y) in enumerate(_positions(b, 7)):
            blocks[k]["tile"], blocks[k]["bo_x"], blocks[k]["bo_y"] = t, x, y
        for q in (1, 21, 22, 120):
            for imp in planes if q == 120 or b == 6 else planes[-2:]:
                sidx, qidx, mean, rej = R.block_segments_batch(TILES, blocks, b, q, W_IN_B, H_IN_B, imp)
                assert rej == 0
                fr = M.Frame(W_IN_B, H_IN_B, imp)
                for k, blk in enumerate(blocks):
                    tl = TILE_LIST[int(blk["tile"])]
                    w = M.block_segment(fr, tl[0] // 4 + int(blk["bo_x"]), tl[1] // 4 + int(blk["bo_y"]), b, q)
                    assert (int(sidx[k]), int(qidx[k])) == w[:2] and mean[k] == w[2], (b, q, k)
                    seen.add((w[0], q))
                if imp is not None and imp.min() == imp.max() and M.BLK_H[b] <= 32 and q == 120:
                    # an interior block's mean is the plane's value exactly
                    assert mean[0] == imp[0, 0] and sidx[0] == want_interior[float(imp[0, 0])]
                    assert qidx[0] == 120 + M.segmentation_data(120)[int(sidx[0])]
                # the second tile's origin: one column of the block inside the frame
                if imp is not None and imp.min() == imp.max() and imp[0, 0] == 1000 and b == 6:
                    assert mean[1] == np.float32(1000 * 4 / 16) and mean[3] == 0
    assert {s for s, q in seen if q == 120} == {0, 1, 2}
    assert (0, 1) in seen and (1, 1) in seen and (2, 1) not in seen and (2, 21) not in seen
    # a bad tile and a negative offset are counted and read nothing
    blocks = np.zeros(3, R.MODE_BLOCK)
    blocks[1]["tile"], blocks[2]["bo_x"] = 2, -4
    sidx, qidx, mean, rej = R.block_segments_batch(TILES, blocks, 6, 120, W_IN_B, H_IN_B, _importance(3))
    assert rej == 2 and sidx[1:].tolist() == [0, 0] and qidx[1:].tolist() == [120, 120] and not mean[1:].any()


PIXEL_CASES = [(b, fmt, bd) for b in (3, 5, 4, 6, 9, 12) for fmt in ("420", "444", "422")
               for bd in (8, 10) if not (fmt == "422" and b == 4)] + [(6, "420", 12), (6, "444", 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("b,fmt,bd", PIXEL_CASES,
                         ids=["%dx%d-%s-%d" % (M.BLK_W[b], M.BLK_H[b], f, d) for b, f, d in PIXEL_CASES])
def test_gpu_pixel_path(b, fmt, bd):
    """compute_distortion under both tunes: per-candidate distortions and
    costs, random importances."""
    R.require_device(0)
    xdec, ydec = FMT[fmt]
    src = _host_planes(1, bd, fmt)
    sets = [_host_planes(10 + s, bd, fmt, noise_of=src) for s in range(3)]
    src_d, sets_d = _device(src, bd, fmt), [_device(s, bd, fmt) for s in sets]
    imp = _importance(b)
    ts = block_tx(b)
    nb = M.n_tx_blocks(b, ts, xdec, ydec)
    pos = _positions(b, 3 if b >= 9 else 5)
    rng = np.random.default_rng(b)
    blocks, cands = np.zeros(len(pos), R.MODE_BLOCK), []
    for k, (t, x, y) in enumerate(pos):
        blocks[k] = (t, x, y, len(cands), 3)
        for s in range(3):  # three intra groups on three sets
            cands.append(_cand(s, M.INTRA | (M.NEED_RECON if s == 1 else 0), s, int(rng.integers(0, 4000)), ts,
                               len(cands) * nb, luma_mode=s, sidx=k))
    cands = np.array(cands, R.MODE_CAND)
    tx_eob = rng.integers(0, 2, len(cands) * nb).astype(np.uint32) * rng.integers(0, 2, len(cands) * nb)
    tx_dist = rng.integers(0, 1 << 20, len(cands) * nb).astype(np.uint64)
    for tune in (R.Tune.Psnr, R.Tune.Psychovisual):
        fr = M.Frame(W_IN_B, H_IN_B, imp, LAMBDA, SCALE, bd, psy=tune == R.Tune.Psychovisual)
        res = R.mode_decide_batch(src_d, sets_d, TILES, blocks, cands, b, LAMBDA, SCALE, W_IN_B, H_IN_B,
                                  imp, tune, bit_depth=bd, tx_dist=tx_dist, tx_eob=tx_eob)
        assert (res.rejected_blocks, res.rejected_cands) == (0, 0)
        ref = _compare(res, fr, src, sets, blocks, cands, b, fmt, tx_dist, tx_eob)
        assert all(sum(r[1]) > 0 for r in ref)
        # neighbouring sub-blocks have different biases, and the scales are per plane
        blk = blocks[0]
        other = M.pixel_distortion(fr, src, sets[0], TILE_LIST[0], int(blk["bo_x"]), int(blk["bo_y"]), b,
                                   xdec, ydec, scale_sum=True)
        assert other != ref[0][1][0]
        if (b, fmt) == (3, "420"):
            # the 2x2 chroma sub-blocks are BLOCK_4X4 areas, not BLOCK_8X8: at the frame's right
            # edge (the second tile's origin) the two means differ, one area being clipped
            assert tuple(blocks[1])[:3] == (1, 0, 0)
            other = M.pixel_distortion(fr, src, sets[0], TILE_LIST[1], 0, 0, b, xdec, ydec, chroma_area=(2, 2))
            assert other != ref[1][1][0]
    # without an importance plane every bias is 0.65
    res = R.mode_decide_batch(src_d, sets_d, TILES, blocks, cands, b, LAMBDA, SCALE, W_IN_B, H_IN_B, None,
                              R.Tune.Psychovisual, bit_depth=bd, tx_dist=tx_dist, tx_eob=tx_eob)
    _compare(res, M.Frame(W_IN_B, H_IN_B, None, LAMBDA, SCALE, bd, psy=True), src, sets, blocks, cands, b,
             fmt, tx_dist, tx_eob)


@pytest.mark.gpu
def test_gpu_lanes_do_not_change_the_result():
    R.require_device(0)
    b, fmt, bd = 6, "420", 8
    src = _host_planes(1, bd, fmt)
    sets = [_host_planes(10 + s, bd, fmt, noise_of=src) for s in range(2)]
    src_d, sets_d = _device(src, bd, fmt), [_device(s, bd, fmt) for s in sets]
    pos = _positions(b, 7)
    blocks = np.zeros(len(pos), R.MODE_BLOCK)
    cands = []
    for k, (t, x, y) in enumerate(pos):  # more than one chunk of eight candidates
        blocks[k] = (t, x, y, len(cands), 11 if k == 2 else 2)
        for s in range(11 if k == 2 else 2):
            cands.append(_cand(s, M.SKIP, s % 2, 100 * s + k, block_tx(b)))
    cands = np.array(cands, R.MODE_CAND)
    fr = M.Frame(W_IN_B, H_IN_B, _importance(1), LAMBDA, SCALE, bd, psy=True)
    outs = []
    for lanes in (0, 8, 16, 64, 256):
        res = R.mode_decide_batch(src_d, sets_d, TILES, blocks, cands, b, LAMBDA, SCALE, W_IN_B, H_IN_B,
                                  fr.imp, R.Tune.Psychovisual, lanes=lanes)
        outs.append(res)
        _compare(res, fr, src, sets, blocks, cands, b, fmt)
    for r in outs[1:]:
        assert r.decisions.tobytes() == outs[0].decisions.tobytes()


@pytest.mark.gpu
def test_gpu_tx_path():
    """compute_tx_distortion with d_dist / d_eob from real tx_blocks_batch
    launches: a 32x32 block in TX_8X8 (16 luma transform blocks) biased by the
    partition's size at every tx_bo, a whole-block intra and an inter
    candidate, a skip candidate and one with need_recon_pixel."""
    R.require_device(0)
    b, fmt, bd = B.BLOCK_32X32, "420", 8
    xdec, ydec = FMT[fmt]
    src = _host_planes(1, bd, fmt)
    rec = _host_planes(20, bd, fmt, noise_of=src)
    pred = _host_planes(21, bd, fmt, noise_of=src)
    src_d, rec_d, pred_d = (_device(p, bd, fmt) for p in (src, rec, pred))
    fill = [(np.full_like(a, 7), xo, yo) for a, xo, yo in src]
    dst_d = [_device(fill, bd, fmt) for _ in range(3)]
    pos = [(0, 0, 0), (0, 8, 8), (1, 0, 0)]
    jobs = np.array([(t, x, y, 60 + 40 * k, 0, 0) for k, (t, x, y) in enumerate(pos)], R.TX_BLOCKS_JOB)
    runs = [  # (tx_size, luma_mode, need_recon_pixel, pred)
        (TS.TX_8X8, PM.DC_PRED, True, None), (TS.TX_32X32, PM.V_PRED, False, None),
        (TS.TX_32X32, PM.NEARESTMV, False, pred_d)]
    tx_dist, tx_eob, first = [], [], []
    for k, (ts, lm, recon, pr) in enumerate(runs):
        lay, _, eobs, dists = R.tx_blocks_batch(rec_d, src_d, TILES, jobs, b, ts, lm, lm if lm < 13 else 0,
                                                need_recon_pixel=recon, bit_depth=bd, pred=pr, dst=dst_d[k])
        first.append(sum(len(a) for a in tx_dist))
        for i in range(len(jobs)):
            tx_dist.append(np.concatenate([dists[p][i] for p in range(3)]))
            tx_eob.append(np.concatenate([eobs[p][i] for p in range(3)]))
        assert lay.blocks_per_job == M.n_tx_blocks(b, int(ts), xdec, ydec)
    assert M.n_tx_blocks(b, int(TS.TX_8X8), xdec, ydec) == 16 + 2
    tx_dist, tx_eob = np.concatenate(tx_dist), np.concatenate(tx_eob)
    assert tx_dist.any() and tx_eob.any()
    sets_d = dst_d + [pred_d]
    sets = [[(pl.download_full().astype(np.uint16), PAD, PAD) for pl in s] for s in sets_d]
    imp = _importance(9)
    blocks, cands = np.zeros(len(pos), R.MODE_BLOCK), []
    for i, (t, x, y) in enumerate(pos):
        blocks[i] = (t, x, y, len(cands), 5)
        off = [first[k] + i * M.n_tx_blocks(b, int(runs[k][0]), xdec, ydec) for k in range(3)]
        cands += [_cand(0, M.SKIP, 3, 90, TS.TX_32X32, luma_mode=PM.NEARESTMV),
                  _cand(0, 0, 2, 400, TS.TX_32X32, off[2], luma_mode=PM.NEARESTMV),
                  _cand(1, M.INTRA, 0, 700, TS.TX_8X8, off[0], luma_mode=PM.DC_PRED),
                  _cand(2, M.INTRA | M.NEED_RECON, 0, 700, TS.TX_8X8, off[0], luma_mode=PM.DC_PRED),
                  _cand(3, M.INTRA, 1, 500, TS.TX_32X32, off[1], luma_mode=PM.V_PRED)]
    cands = np.array(cands, R.MODE_CAND)
    for coeff_rate in (True, False):
        fr = M.Frame(W_IN_B, H_IN_B, imp, LAMBDA, SCALE, bd, use_tx=True, coeff_rate=coeff_rate)
        res = R.mode_decide_batch(src_d, sets_d, TILES, blocks, cands, b, LAMBDA, SCALE, W_IN_B, H_IN_B, imp,
                                  use_tx_domain_distortion=True, coeff_rate=coeff_rate, bit_depth=bd,
                                  tx_dist=tx_dist, tx_eob=tx_eob)
        assert (res.rejected_blocks, res.rejected_cands) == (0, 0)
        ref = _compare(res, fr, src, sets, blocks, cands, b, fmt, tx_dist, tx_eob)
    # the same transform blocks, two paths: the tx sum and the pixels differ
    assert all(r[1][2] != r[1][3] for r in ref)
    # the bias is the partition's at tx_bo: a bias by the transform block's size differs here
    for i, (t, x, y) in enumerate(pos[:2]):
        c = cands[5 * i + 2]
        row = tx_dist[int(c["dist_off"]):int(c["dist_off"]) + 18]
        by_tx = M.tx_distortion(fr, TILE_LIST[t], x, y, b, int(TS.TX_8X8), xdec, ydec, row, bias_by_tx_size=True)
        assert by_tx != ref[i][1][2] == M.tx_distortion(fr, TILE_LIST[t], x, y, b, int(TS.TX_8X8), xdec, ydec, row)


def _walk_setting():
    b, fmt, bd = B.BLOCK_8X8, "420", 8
    src = _host_planes(1, bd, fmt)
    sets = [src, _host_planes(11, bd, fmt, noise_of=src), _host_planes(12, bd, fmt, noise_of=src)]
    # the block at (4, 0) of tile 0: set 1 is exact there as well
    for p in range(3):
        x, w = (PAD + 8, 4) if p else (PAD + 16, 8)
        sets[1][p][0][PAD:PAD + w, x:x + w] = src[p][0][PAD:PAD + w, x:x + w]
    return b, fmt, bd, src, sets, _device(src, bd, fmt), [_device(s, bd, fmt) for s in sets]


@pytest.mark.gpu
def test_gpu_walk_hand_built_lists():
    R.require_device(0)
    b, fmt, bd, src, sets, src_d, sets_d = _walk_setting()
    ts = block_tx(b)
    S, I = M.SKIP, M.INTRA
    E, GZ, GS = M.EVALUATED, M.GATED_ZERO_DIST, M.GATED_SKIP
    lists = [
        [_cand(0, 0, 1, 100, ts), _cand(1, 0, 1, 100, ts)],                         # equal: the first
        [_cand(0, S, 0, 10, ts), _cand(0, 0, 1, 5, ts)],                            # zero skip gates
        [_cand(0, S, 0, 8, ts), _cand(0, 0, 1, 1, ts), _cand(1, S, 0, 50, ts), _cand(1, 0, 2, 1, ts)],
        [_cand(0, S, 0, 8, ts), _cand(0, 0, 1, 1, ts), _cand(1, I, 1, 1, ts), _cand(2, I, 2, 1, ts)],
        [_cand(0, S, 1, 4000, ts), _cand(0, 0, 1, 3000, ts), _cand(1, I, 0, 10, ts, luma_mode=PM.PAETH_PRED)],
        [],
    ]
    want_states = [[E, E], [E, GZ], [E, GZ, E, E], [E, GZ, GS, GS], [E, E, E], []]
    want_winner = [0, 0, 0, 0, 2, None]
    blocks, cands = np.zeros(len(lists), R.MODE_BLOCK), []
    for k, ls in enumerate(lists):
        blocks[k] = (0, 2 * k, 4, len(cands), len(ls))
        cands += ls
    cands = np.array(cands, R.MODE_CAND)
    nb = M.n_tx_blocks(b, ts, 1, 1)
    tx_dist, tx_eob = np.zeros(nb, np.uint64), np.array([0, 3, 0], np.uint32)
    fr = M.Frame(W_IN_B, H_IN_B, _importance(2), LAMBDA, SCALE, bd)
    kw = dict(tx_dist=tx_dist, tx_eob=tx_eob)
    fill = [(np.full_like(a, 9), xo, yo) for a, xo, yo in src]
    commit_d = _device(fill, bd, fmt)
    res = R.mode_decide_batch(src_d, sets_d, TILES, blocks, cands, b, LAMBDA, SCALE, W_IN_B, H_IN_B, fr.imp,
                              commit=commit_d, **kw)
    ref = _compare(res, fr, src, sets, blocks, cands, b, fmt, tx_dist, tx_eob)
    for k, r in enumerate(ref):
        assert r[3] == want_states[k], k
        assert (r[0].cand if r[0] else None) == want_winner[k], k
    assert ref[1][1][0] == 0 and ref[2][1][2] == 0 and res.decisions[5]["cand"] == -1
    assert res.decisions[4]["pay"]["luma_mode"] == PM.PAETH_PRED and res.decisions[4]["has_coeff"] == 1
    assert res.decisions[1]["skip"] == 1 and res.decisions[1]["has_coeff"] == 0
    # the empty list committed nothing
    x = PAD + 4 * 2 * 5
    assert (commit_d[0].download_full()[PAD + 16:PAD + 24, x:x + 8] == 9).all()
    # a second launch seeded with the first one's decisions (the CfL trial): one candidate per
    # block, better than the winner at some blocks and worse at others
    seed = res.decisions.copy()
    blocks2, cands2 = blocks.copy(), []
    for k in range(len(lists)):
        blocks2[k]["cand_first"], blocks2[k]["cand_count"] = k, 1
        cands2.append(_cand(0, I, 0 if k % 2 else 2, 1 if k % 2 else 4000, ts, chroma_mode=PM.UV_CFL_PRED,
                            alpha_u=k))
    cands2 = np.array(cands2, R.MODE_CAND)
    res2 = R.mode_decide_batch(src_d, sets_d, TILES, blocks2, cands2, b, LAMBDA, SCALE, W_IN_B, H_IN_B, fr.imp,
                               seed=seed, **kw)
    ref2 = _compare(res2, fr, src, sets, blocks2, cands2, b, fmt, tx_dist, tx_eob, seed=seed)
    won = [r[0] is not None for r in ref2]
    assert True in won and False in won
    assert [r[3] for r in ref2[:4]] == [[E], [GS], [GS], [GS]]  # seeds with skip gate the intra trial
    assert won[4] is False and won[5] is True and res2.decisions[5]["pay"]["alpha_u"] == 5
    assert res2.decisions[0]["cand"] == -1 and res2.decisions[0]["rd_cost"] == seed[0]["rd_cost"]


@pytest.mark.gpu
def test_gpu_walk_random_lists():
    """200 random blocks with random lists: every state and both gates occur."""
    R.require_device(0)
    b, fmt, bd, src, sets, src_d, sets_d = _walk_setting()
    ts = block_tx(b)
    rng = np.random.default_rng(77)
    blocks, cands = np.zeros(200, R.MODE_BLOCK), []
    for k in range(200):
        first = len(cands)
        g = 0
        for _ in range(int(rng.integers(0, 4))):  # inter groups: the skip candidates first
            for flags in [M.SKIP] * int(rng.integers(0, 3)) + [0] * int(rng.integers(0, 3)):
                cands.append(_cand(g, flags, int(rng.integers(0, 3)), int(rng.choice([1, 8, 40, 40, 900])), ts,
                                   luma_mode=14 + g, sidx=len(cands) % 3))
            g += 1
        for _ in range(int(rng.integers(0, 4))):  # intra groups
            for _ in range(int(rng.integers(1, 3))):
                cands.append(_cand(g, M.INTRA, int(rng.integers(0, 4 if rng.random() < 0.1 else 3)),
                                   int(rng.choice([1, 8, 40, 40, 900])), ts, luma_mode=g % 13))
            g += 1
        t = int(rng.integers(0, 2))
        # the block at (16, 0) of tile 0 is the one both set 0 and set 1 match
        x, y = (4, 0) if rng.random() < 0.3 else (2 * int(rng.integers(0, 8)), 2 * int(rng.integers(0, 8)))
        blocks[k] = (0 if (x, y) == (4, 0) else t, x, y, first, len(cands) - first)
    cands = np.array(cands, R.MODE_CAND)
    nb = M.n_tx_blocks(b, ts, 1, 1)
    tx_dist, tx_eob = np.zeros(nb, np.uint64), np.array([0, 0, 1], np.uint32)
    fr = M.Frame(W_IN_B, H_IN_B, _importance(5), LAMBDA, SCALE, bd, psy=True)
    res = R.mode_decide_batch(src_d, sets_d, TILES, blocks, cands, b, LAMBDA, SCALE, W_IN_B, H_IN_B, fr.imp,
                              R.Tune.Psychovisual, tx_dist=tx_dist, tx_eob=tx_eob)
    ref = _compare(res, fr, src, sets[:3], blocks, cands, b, fmt, tx_dist, tx_eob)
    states = [s for r in ref for s in r[3]]
    assert {M.EVALUATED, M.GATED_ZERO_DIST, M.GATED_SKIP, M.REJECTED} <= set(states)
    assert res.rejected_blocks == 0 and res.rejected_cands == states.count(M.REJECTED) > 0
    assert sum(r[0] is None for r in ref) > 0 and sum(r[0] is not None and r[0].skip for r in ref) > 10
    # equal costs occur, and the two walk mutations would change a result on these lists
    diff = {"replace_on_equal": 0, "zero_from_any_skip": 0}
    for i, blk in enumerate(blocks):
        f, n = int(blk["cand_first"]), int(blk["cand_count"])
        rows = [(int(c["group"]), int(c["flags"]), int(c["rate"]), d, co, True, s == M.REJECTED)
                for c, d, co, s in zip(cands[f:f + n], ref[i][1], ref[i][2], ref[i][3])]
        for m in diff:
            bm, sm = M.walk(rows, **{m: True})
            diff[m] += sm != ref[i][3] or (bm.cand if bm else None) != (ref[i][0].cand if ref[i][0] else None)
    assert diff["replace_on_equal"] > 0 and diff["zero_from_any_skip"] > 0, diff


@pytest.mark.gpu
def test_gpu_commit():
    """The winners' pixels land in commit, padding included; other pixels stay."""
    R.require_device(0)
    b, fmt, bd = B.BLOCK_16X16, "422", 10
    xdec, ydec = FMT[fmt]
    src = _host_planes(1, bd, fmt)
    sets = [_host_planes(10 + s, bd, fmt, noise_of=src) for s in range(3)]
    src_d, sets_d = _device(src, bd, fmt), [_device(s, bd, fmt) for s in sets]
    fill = [(np.full_like(a, 1000 + p), xo, yo) for p, (a, xo, yo) in enumerate(src)]
    commit_d = _device(fill, bd, fmt)
    ts = block_tx(b)
    # (1, 4, 8) lies in the padding right of and below the frame; the last block has no candidates
    pos = [(0, 0, 0), (0, 4, 4), (0, 12, 12), (1, 0, 0), (1, 4, 8), (0, 8, 0)]
    blocks, cands = np.zeros(len(pos), R.MODE_BLOCK), []
    for k, (t, x, y) in enumerate(pos):
        n = 0 if k == 5 else 3
        blocks[k] = (t, x, y, len(cands), n)
        for s in range(n):  # the cheapest rate decides: a different set per block
            cands.append(_cand(s, M.SKIP, s, 8 if s == k % 3 else 8000, ts))
    cands = np.array(cands, R.MODE_CAND)
    fr = M.Frame(W_IN_B, H_IN_B, None, 1e6, SCALE, bd)
    res = R.mode_decide_batch(src_d, sets_d, TILES, blocks, cands, b, 1e6, SCALE, W_IN_B, H_IN_B, None,
                              bit_depth=bd, commit=commit_d)
    ref = _compare(res, fr, src, sets, blocks, cands, b, fmt)
    want = [a.copy() for a, _, _ in fill]
    winners = set()
    for k, (t, x, y) in enumerate(pos[:5]):
        s = int(cands[int(res.decisions[k]["cand"])]["set"])
        assert s == k % 3 == ref[k][0].cand
        winners.add(s)
        for p in range(3):
            xd, yd = (xdec, ydec) if p else (0, 0)
            px, py = M.block_origin(TILE_LIST[t], x, y, xd, yd)
            w, h = 16 >> xd, 16 >> yd
            want[p][PAD + py:PAD + py + h, PAD + px:PAD + px + w] = \
                sets[s][p][0][PAD + py:PAD + py + h, PAD + px:PAD + px + w]
    assert winners == {0, 1, 2}
    for p in range(3):
        assert (commit_d[p].download_full() == want[p]).all(), p
        assert (sets_d[0][p].download_full() == sets[0][p][0]).all()


@pytest.mark.gpu
def test_gpu_per_job_errors_are_counted_and_isolated():
    """Argument errors the kernel rejects before touching memory."""
    R.require_device(0)
    b, fmt, bd = B.BLOCK_16X16, "420", 8
    src = _host_planes(1, bd, fmt)
    sets = [_host_planes(10 + s, bd, fmt, noise_of=src) for s in range(2)]
    src_d, sets_d = _device(src, bd, fmt), [_device(s, bd, fmt) for s in sets]
    ts = block_tx(b)
    nb = M.n_tx_blocks(b, ts, 1, 1)
    tx_dist, tx_eob = np.arange(2 * nb, dtype=np.uint64) * 1000, np.ones(2 * nb, np.uint32)
    good = [_cand(0, M.SKIP, 0, 50, ts), _cand(0, 0, 1, 20, ts, nb), _cand(1, M.INTRA, 0, 700, ts, 0)]
    bad = [_cand(1, M.INTRA, 2, 1, ts), _cand(1, M.INTRA, -1, 1, ts),            # no such set
           _cand(1, M.INTRA, 0, 1, ts, nb + 1), _cand(1, M.INTRA, 0, 1, ts, -1),  # the row leaves the arrays
           _cand(1, M.INTRA, 0, 1, 19), _cand(1, M.INTRA, 0, 1, TS.TX_32X32)]     # no TxSize / larger than bsize
    cands = np.array(good + bad + good + [bad[-1]] + good[:2], R.MODE_CAND)
    n1 = len(good) + len(bad)
    blocks = np.array([(0, 4, 4, 0, n1), (2, 0, 0, n1, 3), (0, 8, 4, n1, 3), (0, 2, 0, n1, 3),
                       (0, 16, 0, n1, 3), (1, 0, 0, n1 + 3, 4), (-1, 0, 0, n1, 3), (0, 0, -4, n1, 3),
                       (1, 4, 4, n1 + 3, 3)], R.MODE_BLOCK)
    fr = M.Frame(W_IN_B, H_IN_B, _importance(4), LAMBDA, SCALE, bd, use_tx=True)
    fill = [(np.full_like(a, 5), xo, yo) for a, xo, yo in src]
    commit_d = _device(fill, bd, fmt)
    kw = dict(use_tx_domain_distortion=True, tx_dist=tx_dist, tx_eob=tx_eob)
    res = R.mode_decide_batch(src_d, sets_d, TILES, blocks, cands, b, LAMBDA, SCALE, W_IN_B, H_IN_B, fr.imp,
                              commit=commit_d, **kw)
    bad_blocks = [1, 3, 4, 5, 6, 7]
    assert res.rejected_blocks == len(bad_blocks) and res.rejected_cands == len(bad) + 1
    for k in bad_blocks:
        d = res.decisions[k]
        assert d["cand"] == -1 and d["rd_cost"] == M.RD_MAX and not d["pay"].tobytes().strip(b"\0")
    assert res.cand_state[len(good):n1].tolist() == [M.REJECTED] * len(bad)
    assert not res.cand_dist[len(good):n1].any()
    # the good blocks are what a launch of them alone gives
    keep = [0, 2]
    ref = _compare(res._replace(decisions=res.decisions[keep + [8]]), fr, src, sets, blocks[keep + [8]], cands,
                   b, fmt, tx_dist, tx_eob)
    assert ref[0][0] is not None and ref[1][0] is not None
    alone = R.mode_decide_batch(src_d, sets_d, TILES, blocks[keep], cands, b, LAMBDA, SCALE, W_IN_B, H_IN_B,
                                fr.imp, **kw)
    assert alone.decisions.tobytes() == res.decisions[keep].tobytes()
    assert (alone.rejected_blocks, alone.rejected_cands) == (0, len(bad))
    # only the good blocks' winners were committed
    got = commit_d[0].download_full()
    touched = np.zeros_like(got, bool)
    for k in keep + [8]:
        px, py = M.block_origin(TILE_LIST[int(blocks[k]["tile"])], int(blocks[k]["bo_x"]), int(blocks[k]["bo_y"]), 0, 0)
        touched[PAD + py:PAD + py + 16, PAD + px:PAD + px + 16] = True
    assert (got[~touched] == 5).all() and (got[touched] != 5).any()


@pytest.mark.gpu
def test_gpu_chain_stacks_to_decision():
    """find_mvrefs_batch -> inter_mode_set_batch -> motion_compensate_batch ->
    tx_blocks_batch -> candidate_rates -> mode_decide_batch on a 64x64 tile of
    16x16 blocks at 4:2:0 8 bit: the winner, its cost and the committed pixels
    equal the checker fed the same intermediate arrays."""
    R.require_device(0)
    b, fmt, bd = B.BLOCK_16X16, "420", 8
    rng = np.random.default_rng(11)
    tile = TILE_LIST[0]
    cells = R.default_block_grid(1, 16, 16)
    for y in range(0, 16, 2):
        for x in range(0, 16, 2):
            c = cells[0, y:y + 2, x:x + 2]
            c["ref"] = (1, 8) if rng.random() < 0.6 else (5, 8)
            c["n4_w"] = c["n4_h"] = 2
            c["newmv"] = rng.random() < 0.5
            c["mv"] = rng.integers(-24, 25, (2, 2))
    grid = R.BlockGrid.from_array(cells, [(16, 16, 0, 0)], frame_cols=32, frame_rows=16, sign_bias=1 << 4)
    sets = R.inter_ref_sets([1, 2, 3, 4, 5, 6, 7], [0, 0, 0, 0, 1, 1, 1], False, b)
    assert (sets.n_single, sets.compound) == (2, 0)
    pos = [(4 * x, 4 * y) for y in range(4) for x in range(4)]
    n = len(pos)
    iblocks = np.array([(0, x, y) for x, y in pos], R.INTER_BLK)
    q = [(0, x, y, 4, 4, r0, 8) for x, y in pos for r0 in (1, 5)]
    ctx, ln, st, rej = R.find_mvrefs_batch(grid, q)
    assert rej == 0
    stacks = np.zeros(n * 2, R.MVREF_RESULT)
    stacks["mode_context"], stacks["n"], stacks["stack"] = ctx, ln, st
    stacks = stacks.reshape(n, 2)
    me = rng.integers(-30, 31, (n, 2, 2)).astype(np.int16)
    lists, mc_jobs, rej = R.inter_mode_set_batch(stacks, me, sets, False, iblocks)
    assert rej == 0
    # the planes: two references, the source, one destination set per candidate
    src = _host_planes(1, bd, fmt)
    refs = [_host_planes(30 + s, bd, fmt, noise_of=src) for s in range(2)]
    src_d, refs_d = _device(src, bd, fmt), [_device(r, bd, fmt) for r in refs]
    nd = int(lists["n"].max())
    fill = [(np.full_like(a, 3), xo, yo) for a, xo, yo in src]
    pred_d = [_device(fill, bd, fmt) for _ in range(nd)]
    assert R.motion_compensate_batch(refs_d, pred_d, TILES, mc_jobs.reshape(-1), b, 0, False, bd) == 0
    # every candidate's transform blocks from its prediction: one launch per candidate index
    ts = TS.TX_16X16
    xdec, ydec = FMT[fmt]
    nb = M.n_tx_blocks(b, int(ts), xdec, ydec)
    imp = _importance(6)
    sidx, qidx, _, rej = R.block_segments_batch(TILES, np.array([(0, x, y, 0, 0) for x, y in pos], R.MODE_BLOCK),
                                                b, 90, W_IN_B, H_IN_B, imp)
    assert rej == 0 and len(set(sidx.tolist())) > 1
    tj = np.array([(0, x, y, int(qidx[i]), 0, 0) for i, (x, y) in enumerate(pos)], R.TX_BLOCKS_JOB)
    tx_dist = np.zeros((nd, n, nb), np.uint64)
    tx_eob = np.zeros((nd, n, nb), np.uint32)
    coeffs, coeff_off = [], {}
    for k in range(nd):
        lay, levels, eobs, dists = R.tx_blocks_batch(src_d, src_d, TILES, tj, b, ts, PM.NEARESTMV, bit_depth=bd,
                                                     pred=pred_d[k], need_recon_pixel=False)
        for i in range(n):
            tx_dist[k, i] = np.concatenate([dists[p][i] for p in range(3)])
            tx_eob[k, i] = np.concatenate([eobs[p][i] for p in range(3)])
            for p in range(3):
                coeff_off[(k, i, p)] = sum(len(c) for c in coeffs)
                coeffs.append(levels[p][i].reshape(-1))
    coeffs = np.concatenate(coeffs).astype(np.int32)
    # the candidates, in the reference's order: per inter mode its skip candidate, then the coded one
    ec, recs, blocks = [], [], np.zeros(n, R.MODE_BLOCK)
    for i, (x, y) in enumerate(pos):
        blocks[i] = (0, x, y, len(recs), 2 * int(lists[i]["n"]))
        for k in range(int(lists[i]["n"])):
            c = lists[i]["cand"][k]
            s = stacks[i, int(c["set"])]
            for skip in (1, 0):
                j = np.zeros(1, R.EC_MODE_JOB)[0]
                j["bx"], j["by"], j["bsize"], j["skip"] = x, y, int(b), skip
                j["luma_mode"] = j["chroma_mode"] = int(c["luma_mode"])
                j["ref0"], j["ref1"] = int(c["ref"][0]), int(c["ref"][1])
                j["mv0_row"], j["mv0_col"] = int(c["mv"][0][0]), int(c["mv"][0][1])
                j["ref_mv0_row"], j["ref_mv0_col"] = (int(v) for v in s["stack"][0]["this_mv"])
                j["mode_context"], j["num_mv_found"] = int(c["mode_context"]), int(s["n"])
                for w in range(4):
                    j["weight%d" % w] = int(s["stack"][w]["weight"])
                rows = [] if skip else \
                    [(0, 0, x, y, 2, 0, 1, 4, 4, coeff_off[(k, i, 0)])] + \
                    [(0, p, x, y, 1, 0, 1, 3, 3, coeff_off[(k, i, p)]) for p in (1, 2)]
                ec.append((None, j, rows))
                recs.append(_cand(k, M.SKIP if skip else 0, k, 0, ts, (k * n + i) * nb,
                                  luma_mode=int(c["luma_mode"]), chroma_mode=int(c["luma_mode"]),
                                  ref_frames=c["ref"], mvs=c["mv"], sidx=int(sidx[i])))
    # priced after one committed block: a GLOBALMV skip block at the tile's origin
    prm = R.EcModeParams(reference_mode=0, tile_dims=((16, 16),))
    done = np.zeros(1, R.EC_MODE_JOB)
    done["bsize"], done["skip"], done["luma_mode"], done["chroma_mode"] = int(b), 1, PM.GLOBALMV, PM.GLOBALMV
    done["ref0"], done["ref1"] = 1, 8
    rates, _, _ = R.candidate_rates(done, [(3, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0, 4, 4, 0)],
                                    coeffs, ec, prm, R.ec_default_cdf_all(0))
    cands = np.array(recs, R.MODE_CAND)
    cands["rate"] = rates
    assert len(set(rates.tolist())) > 4
    lam = 120.0
    commit_d = _device(fill, bd, fmt)
    res = R.mode_decide_batch(src_d, pred_d, TILES, blocks, cands, b, lam, SCALE, W_IN_B, H_IN_B, imp,
                              use_tx_domain_distortion=True, bit_depth=bd, tx_dist=tx_dist.reshape(-1),
                              tx_eob=tx_eob.reshape(-1), commit=commit_d)
    assert (res.rejected_blocks, res.rejected_cands) == (0, 0)
    fr = M.Frame(W_IN_B, H_IN_B, imp, lam, SCALE, bd, use_tx=True)
    preds = [[(pl.download_full().astype(np.uint16), PAD, PAD) for pl in s] for s in pred_d]
    ref = _compare(res, fr, src, preds, blocks, cands, b, fmt, tx_dist.reshape(-1), tx_eob.reshape(-1))
    want = [a.copy() for a, _, _ in fill]
    for i, (x, y) in enumerate(pos):
        assert ref[i][0] is not None
        s = int(cands[int(res.decisions[i]["cand"])]["set"])
        for p in range(3):
            xd, yd = (xdec, ydec) if p else (0, 0)
            px, py = M.block_origin(tile, x, y, xd, yd)
            w, h = 16 >> xd, 16 >> yd
            want[p][PAD + py:PAD + py + h, PAD + px:PAD + px + w] = \
                preds[s][p][0][PAD + py:PAD + py + h, PAD + px:PAD + px + w]
    for p in range(3):
        assert (commit_d[p].download_full() == want[p]).all()
    assert len({int(d["pay"]["luma_mode"]) for d in res.decisions}) > 1

"""rv_motion_estimation_batch / rv_save_block_motion_batch / rv_me_pmv_index
(rav1e_amd/csrc/rv_motion_est.hip) against tests/motion_est_ref.py, which
composes the pinned oracle pieces, and that module against the vectors the
reference's own text produced (tests/golden/ref_motion_est.npz).  Every
comparison has tolerance 0 on MV and cost.

The GPU cases share one 136 x 104 luma frame (w_in_b 34, h_in_b 26) per bit
depth: a smooth scene, the references the same scene moved by a sub-pel amount
plus noise, so a search has a trend to follow.  Two tile layouts: one tile,
and 64-pixel tile columns (a tile with an origin, and a last column 8 pixels
wide).  The motion fields are random per 4x4 cell, about half the cells zero.
A case's inputs and its reference outputs are built once (functools.cache)
and shared by the GPU test and the CPU test of the vacuity conditions."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rav1e_amd as R
from tests import motion_est_ref as M

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_motion_est.npz")
B = R.BlockSize
FW, FH, W4, H4, PAD = 136, 104, 34, 26, 88
GEOM = (PAD, PAD, FW, FH)
LAYOUTS = {"one": [(0, 0, FW, FH)], "cols": [(0, 0, 64, FH), (64, 0, 64, FH), (128, 0, 8, FH)]}
SIZES = [B.BLOCK_8X8, B.BLOCK_8X16, B.BLOCK_16X8, B.BLOCK_16X16, B.BLOCK_16X32, B.BLOCK_32X16,
         B.BLOCK_32X32, B.BLOCK_32X64, B.BLOCK_64X32, B.BLOCK_64X64]
# single reference sets (RefType, DPB slot): 1, 2 and 3 sets, no slot shared
SETS = {1: [(1, 0)], 2: [(1, 0), (5, 1)], 3: [(1, 0), (4, 1), (5, 2)]}
# the scene's displacement in each DPB slot's plane, 1/8 pel (row, col)
# (slot 1's is far to the left: inside get_mv_range of the frame, outside the
# range a tile's own rectangle would give for blocks near a tile's left edge)
TRUE_MV = [(20, -26), (-11, -420), (6, 29)]
LAMBDA = R.me_lambda_u32(1.37) if hasattr(R, "me_lambda_u32") else 175


# ---- shared inputs -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pixels(bd):
    """(org_full, [ref_full per slot]): padded arrays of geometry GEOM."""
    rng = np.random.default_rng(1000 + bd)
    S = 8  # the scene at 1/8 pel
    hr = rng.random((FH * S + 1280, FW * S + 1280))
    for _ in range(2):  # two box blurs of 5 pixels: smooth, with texture left
        for ax in (0, 1):
            c = np.cumsum(hr, axis=ax)
            k = 5 * S
            hr = np.take(c, np.arange(k, c.shape[ax]), axis=ax) - np.take(
                c, np.arange(0, c.shape[ax] - k), axis=ax)
    hr = (hr - hr.min()) / (hr.max() - hr.min())
    mx = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8

    def cut(dy, dx, noise):
        a = hr[560 + dy:560 + dy + FH * S:S, 560 + dx:560 + dx + FW * S:S] * mx
        if noise:
            a = a + rng.integers(-2, 3, a.shape) * (1 << (bd - 8))
        return np.pad(np.clip(np.rint(a), 0, mx).astype(dt), PAD, mode="edge")

    # a plane cut at (-r, -c) shows the scene moved so that a block's MV is (r, c)
    return cut(0, 0, False), [cut(-r, -c, True) for r, c in TRUE_MV]


def _near(rng, true, full):
    """The scene's MV with a full-pel jitter (quantized when `full`)."""
    r, c = true
    if full:
        r, c = M._qfull((r, c))
    return (r + 8 * int(rng.integers(-1, 2)), c + 8 * int(rng.integers(-1, 2)))


def _field(rng, sets):
    """A (7, H4, W4, 2) field: per 4x4 cell zero (half), near the scene's MV
    of that reference (a third) or anything."""
    f = np.zeros((7, H4, W4, 2), np.int16)
    true = {ref - 1: TRUE_MV[slot] for ref, slot in sets}
    for ridx in range(7):
        for y in range(H4):
            for x in range(W4):
                u = rng.random()
                if u < 0.5:
                    continue
                if u < 0.83 and ridx in true:
                    f[ridx, y, x] = _near(rng, true[ridx], rng.random() < 0.7)
                else:
                    f[ridx, y, x] = rng.integers(-160, 161, 2)
    return f


def _positions(rng, bsize, tiles, limit=48):
    """(tile, bo_x, bo_y) of up to `limit` aligned blocks inside their tiles:
    each tile's first and last column and row first, then a random fill."""
    bw4, bh4 = M.BLK_W[bsize] // 4, M.BLK_H[bsize] // 4
    must, rest = [], []
    for t, (_, _, tw, th) in enumerate(tiles):
        xs = list(range(0, (tw >> 2) - bw4 + 1, bw4))
        ys = list(range(0, (th >> 2) - bh4 + 1, bh4))
        for y in ys:
            for x in xs:
                edge = (x in (xs[0], xs[-1])) + (y in (ys[0], ys[-1]))
                (must if edge == 2 else rest).append((t, x, y))
    rng.shuffle(rest)
    return (must + rest)[:limit]


def _ref_sets(ns, compound=0):
    s = R.RvInterRefSets()
    s.n_single, s.compound, s.fwd, s.bwd = ns, compound, 0, -1
    for i, (ref, slot) in enumerate(SETS[ns]):
        s.ref[i], s.slot[i] = ref, slot
        if ref >= 5 and s.bwd < 0:
            s.bwd = i
    return s


@functools.lru_cache(maxsize=None)
def _case(bsize, layout, bd=8, satd=True, hp=False, ns=2, prev=True, seed=0, limit=48):
    """Inputs of one batch and the reference's outputs for it."""
    rng = np.random.default_rng([int(bsize), len(layout), bd, satd, hp, ns, prev, seed])
    tiles = LAYOUTS[layout]
    sets = SETS[ns]
    pos = _positions(rng, int(bsize), tiles, limit)
    n = len(pos)
    tile_mvs, prev_mvs = _field(rng, sets), (_field(rng, sets) if prev else None)
    stacks = np.zeros((n, ns), R.MVREF_RESULT)
    cmv = np.zeros((n, ns, 2), np.int16)
    for b in range(n):
        for i, (ref, slot) in enumerate(sets):
            ln = int(rng.integers(0, 5)) if (b + i) % 5 else (b // 5) % 2  # empty / one entry
            stacks[b, i]["n"] = ln
            stacks[b, i]["mode_context"] = int(rng.integers(0, 200))
            for k in range(9):  # entries past n hold values that must not be read as pmv
                stacks[b, i]["stack"][k]["this_mv"] = _near(rng, TRUE_MV[slot], False) \
                    if rng.random() < 0.6 else rng.integers(-90, 91, 2)
                stacks[b, i]["stack"][k]["comp_mv"] = rng.integers(-90, 91, 2)
            u = rng.random()
            if u < 0.35:
                cmv[b, i] = _near(rng, TRUE_MV[slot], False)
            elif u < 0.6:
                cmv[b, i] = rng.integers(-200, 201, 2)
            elif u < 0.7:
                cmv[b, i] = (3000, -3000)  # its quantized form is out of range
    org, refs = _pixels(bd)
    want_mv = np.zeros((n, ns, 2), np.int16)
    want_cost = np.zeros((n, ns), np.uint64)
    infos = []
    for b, (t, bx, by) in enumerate(pos):
        for i, (ref, slot) in enumerate(sets):
            info = {}
            mv, cost = M.motion_estimation(
                org, refs[slot], GEOM, W4, H4, tiles[t], bx, by, int(bsize), int(stacks[b, i]["n"]),
                stacks[b, i]["stack"]["this_mv"], tuple(int(v) for v in cmv[b, i]),
                tile_mvs[ref - 1], prev_mvs[ref - 1] if prev else None, LAMBDA, satd, hp, bd, info)
            want_mv[b, i], want_cost[b, i] = mv, cost
            infos.append(info)
    return dict(tiles=tiles, pos=pos, n=n, ns=ns, tile_mvs=tile_mvs, prev_mvs=prev_mvs,
                stacks=stacks, cmv=cmv, want_mv=want_mv, want_cost=want_cost, infos=infos,
                bsize=bsize, bd=bd, satd=satd, hp=hp)


def _size_cases():
    out = []
    for k, b in enumerate(SIZES):
        for j, layout in enumerate(("one", "cols")):
            for satd in (False, True):
                m = 2 * k + j + satd
                # prev None and the three n_single values rotate through the grid
                out.append((b, layout, 8, satd, bool(m & 1), 1 + m % 3, m % 4 != 3))
    return out


SIZE_CASES = _size_cases()
HBD_CASES = [(B.BLOCK_8X8, "cols", 10, True, False, 2, True), (B.BLOCK_16X8, "one", 12, True, True, 3, True),
             (B.BLOCK_64X64, "cols", 10, False, True, 2, True), (B.BLOCK_64X64, "one", 12, True, False, 1, True),
             (B.BLOCK_8X8, "one", 12, False, True, 2, False)]


# ---- CPU: the reference against the reference's own text ------------------------
def test_ref_glue_vs_reference_text():
    """get_mv_range, save_block_motion and the pmv_idx expression of
    motion_est_ref.py against what the reference's text gave."""
    g = np.load(GOLD)
    for w_in_b, h_in_b, fx, fy, bw, bh, a, b, c, d in g["range"]:
        assert M.mv_range(int(w_in_b), int(h_in_b), int(fx), int(fy), int(bw), int(bh)) == \
            (a, b, c, d)
    for bsize, x, y, idx in g["pmv_idx"]:
        assert M.pmv_index(int(bsize), int(x), int(y)) == idx
    off = 0
    for k, (tx, ty, tw, th, rows, cols, nj) in enumerate(g["sbm_case"]):
        jobs = [(0, int(j[0]), int(j[1]), int(j[2]), int(j[3]), (int(j[4]), int(j[5])))
                for j in g["sbm_jobs"][off:off + nj]]
        off += nj
        # the golden field is the tile's own (7, rows, cols): a frame of that size
        f = np.zeros((7, int(rows), int(cols), 2), np.int16)
        M.save_block_motion(f, [(0, 0, int(tw), int(th))], jobs)
        want = g["sbm_out"][g["sbm_off"][k]:g["sbm_off"][k + 1]].reshape(f.shape)
        assert (f == want).all(), k
    assert off == len(g["sbm_jobs"])


def test_ref_chain_vs_reference_text():
    """motion_estimation of motion_est_ref.py (orc_subset_predictors ->
    orc_diamond_search full-pel -> sub-pel) against the reference's
    get_mv_range / get_subset_predictors / diamond_me_search run in that
    order on small planes at 8x8, 16x8, 8x16 and 32x32."""
    g = np.load(GOLD)
    org, ref = g["me_org"], g["me_ref"]
    xo, yo, w, h = (int(v) for v in g["me_geom"])
    seen = set()
    for k, c in enumerate(g["me_cases"]):
        (bsize, tx, ty, tw, th, bx, by, has_prev, satd, hp, lam, sn, p0r, p0c, p1r, p1c, cr,
         cc) = (int(v) for v in c)
        tf = g["me_tile_field"][k]
        pf = g["me_prev_field"][k] if has_prev else None
        stack = np.array([[p0r, p0c], [p1r, p1c]], np.int16)
        info = {}
        mv, cost = M.motion_estimation(org, ref, (xo, yo, w, h), w // 4, h // 4, (tx, ty, tw, th), bx,
                                       by, bsize, sn, stack, (cr, cc), tf, pf, lam, bool(satd),
                                       bool(hp), 8, info)
        assert info["full"] == tuple(int(v) for v in g["me_full"][k]), k
        assert mv == tuple(int(v) for v in g["me_mv"][k]) and cost == int(g["me_cost"][k]), k
        seen.add(bsize)
    assert seen >= {int(B.BLOCK_8X8), int(B.BLOCK_16X8), int(B.BLOCK_8X16), int(B.BLOCK_32X32)}


# ---- CPU: the library's host side -------------------------------------------------
def test_symbols_exported():
    L = R.lib()
    for name in ("rv_motion_estimation_batch", "rv_save_block_motion_batch",
                 "rv_save_block_motion_scratch_bytes", "rv_me_pmv_index"):
        assert hasattr(L, name), name
    for name in ("motion_estimation_batch", "save_block_motion_batch", "me_pmv_index",
                 "me_lambda_u32", "ME_SAVE_JOB", "RvMeParams"):
        assert hasattr(R, name), name
    with open(R.HEADER_PATH) as f:
        h = f.read()
    assert "rv_motion_estimation_batch" in h and "rv_me_save_job" in h and "rv_me_params" in h
    assert C.sizeof(R.RvMeParams) == 32 and R.ME_SAVE_JOB.itemsize == 24


def test_me_lambda_u32():
    assert R.me_lambda_u32(1.37) == int(1.37 * 256.0 * 0.5) == 175
    assert R.me_lambda_u32(0.0) == 0 and R.me_lambda_u32(-3.0) == 0
    assert R.me_lambda_u32(float("nan")) == 0 and R.me_lambda_u32(1e12) == 0xFFFFFFFF
    assert R.me_lambda_u32(2.0 ** -7 * 3) == 3


def test_pmv_index():
    """Every supported size, offsets either side of 32 and 64 (4x4 units)."""
    for b in SIZES:
        for x in (0, 8, 24, 31, 32, 33, 40, 63, 64, 65, 96):
            for y in (0, 16, 31, 32, 33, 63, 64, 65):
                want = M.pmv_index(int(b), x, y)
                assert R.me_pmv_index(b, x, y) == want
                big = M.BLK_W[b] > 32 or M.BLK_H[b] > 32
                assert want == (0 if big else 1 + ((x >> 5) & 1) + 2 * ((y >> 5) & 1))
    assert R.lib().rv_me_pmv_index(22, 0, 0) == -1 and R.lib().rv_me_pmv_index(-1, 0, 0) == -1
    assert R.lib().rv_me_pmv_index(int(B.BLOCK_16X64), 0, 0) == -1


def _host_plane(bd=8, pad=PAD, w=FW, h=FH):
    p = R.RvPlane()
    p.data = 0x1000  # never dereferenced: every call below fails before a launch
    p.stride, p.alloc_height = w + 2 * pad, h + 2 * pad
    p.width, p.height, p.xorigin, p.yorigin = w, h, pad, pad
    p.hbd, p.bit_depth = int(bd > 8), bd
    return p


def _call(org=None, refs=None, n_refs=2, n=4, sets=None, bsize=B.BLOCK_16X16, bd=8, ptr=0x1000,
          status=0x1000, w_in_b=W4, h_in_b=H4, n_tiles=1):
    org = _host_plane(bd) if org is None else org
    if refs is None:
        refs = (R.RvPlane * 6)()
        for k in (0, 3):
            refs[k] = _host_plane(bd)
    prm = R.RvMeParams(int(bsize), bd, 1, 0, w_in_b, h_in_b, 100, 0)
    sets = _ref_sets(2) if sets is None else sets
    return R.lib().rv_motion_estimation_batch(
        C.byref(org) if org else None, refs, n_refs, ptr, n_tiles, ptr, n, sets, ptr, ptr, ptr, None,
        C.byref(prm), ptr, None, status, None)


def test_errors_before_launch():
    """Every code the entry points return before a launch, without a device."""
    assert _call(bsize=B.BLOCK_4X8) == R.RV_ENOTSUP and _call(bsize=B.BLOCK_8X4) == R.RV_ENOTSUP
    assert _call(bsize=B.BLOCK_4X4) == R.RV_ENOTSUP
    for b in (B.BLOCK_16X64, B.BLOCK_64X16, B.BLOCK_8X32, B.BLOCK_4X16, B.BLOCK_64X128,
              B.BLOCK_128X128):
        assert _call(bsize=b) == R.RV_ENOTSUP, b
    assert _call(bsize=22) == R.RV_EINVAL and _call(bsize=-1) == R.RV_EINVAL
    assert _call(n=-1) == R.RV_EINVAL
    assert _call(ptr=None) == R.RV_EINVAL and _call(status=None) == R.RV_EINVAL
    assert _call(org=False) == R.RV_EINVAL
    assert _call(n_refs=0) == R.RV_EINVAL and _call(n_refs=9) == R.RV_EINVAL
    assert _call(n_refs=1) == R.RV_EINVAL  # set 1's slot is not in refs
    assert _call(bd=9) == R.RV_EINVAL
    assert _call(org=_host_plane(10)) == R.RV_EINVAL  # u16 pixels at 8 bit
    bad = _ref_sets(2)
    bad.n_single = 0
    assert _call(sets=bad) == R.RV_EINVAL
    bad = _ref_sets(2)
    bad.ref[1] = 8
    assert _call(sets=bad) == R.RV_EINVAL
    bad = _ref_sets(2)
    bad.compound, bad.bwd = 1, -1
    assert _call(sets=bad) == R.RV_EINVAL
    assert _call(w_in_b=0) == R.RV_EINVAL
    # padding: 64x64 needs 80 pixels around the frame; 16x16 is served by 40
    small = (R.RvPlane * 6)()
    for k in (0, 3):
        small[k] = _host_plane(8, pad=40)
    assert _call(refs=small, bsize=B.BLOCK_64X64) == R.RV_EINVAL
    shifted = (R.RvPlane * 6)()
    shifted[0], shifted[3] = _host_plane(8), _host_plane(8, pad=96)
    assert _call(refs=shifted) == R.RV_EINVAL  # geometries differ
    assert _call(org=_host_plane(8, pad=0, w=FW - 8)) == R.RV_EINVAL  # the source does not hold the frame
    L = R.lib()
    assert L.rv_save_block_motion_scratch_bytes(W4, H4) == 7 * W4 * H4 * 4
    assert L.rv_save_block_motion_scratch_bytes(0, H4) == 0
    assert L.rv_save_block_motion_batch(0x1000, -1, 0x1000, 1, W4, H4, 0x1000, 0x1000, 0x1000,
                                        None) == R.RV_EINVAL
    assert L.rv_save_block_motion_batch(0x1000, 1, 0x1000, 1, W4, H4, None, 0x1000, 0x1000,
                                        None) == R.RV_EINVAL
    assert L.rv_save_block_motion_batch(0x1000, 1, 0x1000, 1, 0, H4, 0x1000, 0x1000, 0x1000,
                                        None) == R.RV_EINVAL
    assert L.rv_save_block_motion_batch(0x1000, 1, 0x1000, 1, W4, H4, 0x1000, 0x1000, None,
                                        None) == R.RV_EINVAL


def test_vacuity_conditions():
    """The GPU cases' seeded inputs exercise what they are meant to, judged on
    the reference's outputs."""
    items, starts, flags = [], set(), {"one": [], "cols": []}
    for spec in SIZE_CASES + HBD_CASES:
        c = _case(*spec)
        for k, info in enumerate(c["infos"]):
            items.append((tuple(int(v) for v in c["want_mv"].reshape(-1, 2)[k]), info["full"]))
            starts.add(info["start"])
            flags[spec[1]].append(info["flags"])
    n = len(items)
    assert sum(1 for mv, _ in items if mv[0] & 7 or mv[1] & 7) * 4 >= n
    assert sum(1 for _, full in items if full != (0, 0)) * 4 >= n
    assert starts == set(M.SOURCES), set(M.SOURCES) - starts
    for layout, fl in flags.items():
        for j in range(3):
            assert any(not f[j] for f in fl), (layout, j)
    # the previous field differs inside 8x8 cells: an 8x8-granular read changes sets
    c = _case(*SIZE_CASES[0])
    p = c["prev_mvs"] if c["prev_mvs"] is not None else _case(*SIZE_CASES[1])["prev_mvs"]
    assert (p[:, 0::2, 0::2] != p[:, 1::2, 1::2]).any()


# ---- GPU --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dev_planes(bd):
    org, refs = _pixels(bd)
    po = R.DevicePlane.from_full(org, PAD, PAD, FW, FH, bit_depth=bd)
    pr = [[R.DevicePlane.from_full(r, PAD, PAD, FW, FH, bit_depth=bd)] for r in refs]
    return po, pr


def _run(c, blocks=None, stacks=None, tile_mvs=None, device=False, compound=0):
    po, pr = _dev_planes(c["bd"])
    blk = np.array(c["pos"], np.int32).view(R.INTER_BLK).reshape(-1) if blocks is None else blocks
    return R.motion_estimation_batch(
        po, pr, np.array(c["tiles"], np.int32).view(R.INTRA_TILE).reshape(-1), blk,
        _ref_sets(c["ns"], compound), c["stacks"] if stacks is None else stacks, c["cmv"],
        c["tile_mvs"] if tile_mvs is None else tile_mvs, c["prev_mvs"], c["bsize"], W4, H4, LAMBDA,
        c["satd"], c["hp"], c["bd"], device)


def _check(c, me, res):
    assert (me == c["want_mv"]).all(), np.argwhere((me != c["want_mv"]).any(axis=2))[:4]
    assert (res["mv_row"] == c["want_mv"][..., 0]).all() and (res["mv_col"] == c["want_mv"][..., 1]).all()
    assert (res["cost"] == c["want_cost"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("spec", SIZE_CASES + HBD_CASES, ids=lambda s: "%s-%s-%dbit-%s-hp%d-ns%d-prev%d" % (
    B(s[0]).name[6:], s[1], s[2], "satd" if s[3] else "sad", s[4], s[5], s[6]))
def test_gpu_motion_estimation(spec):
    """Every supported size at 8 bit on both tile layouts with SAD and SATD,
    allow_hp on and off, 1 / 2 / 3 reference sets, with and without the
    previous frame's field; three sizes at 10 / 12 bit."""
    R.require_device(0)
    c = _case(*spec)
    me, res, rej = _run(c)
    assert rej == 0
    _check(c, me, res)


@pytest.mark.gpu
def test_gpu_rejection_mixed_into_a_batch():
    """Rejected items write nothing and are counted; the valid ones around
    them are unchanged."""
    R.require_device(0)
    c = _case(B.BLOCK_16X16, "cols", 8, True, False, 2, True)
    blk = np.array(c["pos"], np.int32).view(R.INTER_BLK).reshape(-1).copy()
    stacks = c["stacks"].copy()
    bad = {0: ("tile", 3), 3: ("tile", -1), 5: ("bo_x", -4), 8: ("bo_x", blk[8]["bo_x"] + 1),
           11: ("bo_y", 24), 13: ("bo_x", 16)}  # 24 + 4 > 26 rows; 16 + 4 > a tile's 16 columns
    for b, (f, v) in bad.items():
        blk[b][f] = v
    stacks[20, 1]["n"], stacks[21, 0]["n"] = 10, -1
    me, res, rej = _run(c, blocks=blk, stacks=stacks)
    assert rej == 2 * len(bad) + 2
    want_mv, want_cost = c["want_mv"].copy(), c["want_cost"].copy()
    for b in bad:
        want_mv[b], want_cost[b] = 0, 0
    want_mv[20, 1], want_cost[20, 1], want_mv[21, 0], want_cost[21, 0] = 0, 0, 0, 0
    assert (me == want_mv).all() and (res["cost"] == want_cost).all()


def _sbm_jobs(rng, tiles, n=60):
    jobs = np.zeros(n, R.ME_SAVE_JOB)
    for k in range(n):
        t = int(rng.integers(0, len(tiles)))
        cols, rows = tiles[t][2] >> 2, tiles[t][3] >> 2
        jobs[k] = (t, int(rng.integers(0, cols)), int(rng.integers(0, rows)),
                   int(rng.choice([0, 3, 4, 5, 6, 9, 12, 15, 18])),
                   int(rng.choice([-1, 0, 0, 3, 4, 4, 6])), _near(rng, TRUE_MV[0], False))
    return jobs


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["one", "cols"])
def test_gpu_save_block_motion_then_search(layout):
    """save_block_motion_batch with overlapping jobs, rectangles that cross
    their tile's visible edge and skipped intra entries, equal to the
    reference's loop; a search over the painted field then differs from the
    search over the field before it."""
    R.require_device(0)
    c = _case(B.BLOCK_8X8, layout, 8, True, False, 2, True)
    tiles = c["tiles"]
    rng = np.random.default_rng(77)
    jobs = _sbm_jobs(rng, tiles)
    jobs[-1] = (len(tiles), 0, 0, 3, 0, (8, 8))  # rejected: no such tile
    jobs[-2] = (0, tiles[0][2] >> 2, 0, 3, 0, (8, 8))  # rejected: outside its tile
    want = c["tile_mvs"].copy()
    M.save_block_motion(want, tiles, [(int(j["tile"]), int(j["bo_x"]), int(j["bo_y"]), int(j["bsize"]),
                                      int(j["ref_index"]), tuple(int(v) for v in j["mv"]))
                                     for j in jobs[:-2]])
    dt = np.array(tiles, np.int32).view(R.INTRA_TILE).reshape(-1)
    dfield, rej = R.save_block_motion_batch(jobs, dt, c["tile_mvs"], W4, H4)
    got = dfield.download(np.int16, want.size).reshape(want.shape)
    assert rej == 2 and (got == want).all()
    assert (want != c["tile_mvs"]).any() and (jobs["ref_index"] < 0).any()
    clipped = [j for j in jobs[:-2] if j["ref_index"] >= 0 and
               j["bo_x"] + M.BLK_W[j["bsize"]] // 4 > tiles[j["tile"]][2] >> 2]
    assert clipped
    # the second batch reads the painted field, on the device
    me2, res2, rej2 = _run(c, tile_mvs=dfield)
    assert rej2 == 0
    org, refs = _pixels(8)
    differs = 0
    for b, (t, bx, by) in enumerate(c["pos"]):
        for i, (ref, slot) in enumerate(SETS[2]):
            mv, cost = M.motion_estimation(
                org, refs[slot], GEOM, W4, H4, tiles[t], bx, by, int(c["bsize"]),
                int(c["stacks"][b, i]["n"]), c["stacks"][b, i]["stack"]["this_mv"],
                tuple(int(v) for v in c["cmv"][b, i]), want[ref - 1], c["prev_mvs"][ref - 1], LAMBDA,
                True, False, 8)
            assert tuple(me2[b, i]) == mv and int(res2[b, i]["cost"]) == cost, (b, i)
            differs += tuple(me2[b, i]) != tuple(c["want_mv"][b, i])
    assert differs > 0


@pytest.mark.gpu
def test_gpu_chain_stacks_to_prediction():
    """find_mvrefs_batch -> motion_estimation_batch -> inter_mode_set_batch ->
    motion_compensate_batch, d_me staying on the device, against the same
    chain through the references."""
    from tests import inter_front_ref as F
    from tests.test_inter_front import _expected_lists
    R.require_device(0)
    b, bd = B.BLOCK_16X16, 8
    rng = np.random.default_rng(9)
    tiles = LAYOUTS["one"]
    cells = R.default_block_grid(1, 32, 48)
    for y in range(0, H4, 2):
        for x in range(0, W4, 2):
            cc = cells[0, y:y + 2, x:x + 2]
            cc["ref"] = (1, 5) if rng.random() < 0.4 else ((1, 8) if rng.random() < 0.6 else (5, 8))
            cc["n4_w"] = cc["n4_h"] = 2
            cc["newmv"] = rng.random() < 0.5
            cc["mv"] = rng.integers(-40, 41, (2, 2))
    grid = R.BlockGrid.from_array(cells, [(W4, H4, 0, 0)], frame_cols=W4, frame_rows=H4,
                                  sign_bias=1 << 4)
    sets = R.inter_ref_sets([1, 2, 3, 4, 5, 6, 7], [0, 0, 0, 0, 1, 1, 1], True, b)
    assert (sets.n_single, sets.compound) == (2, 1)
    pos = [(x, y) for y in range(4, 20, 4) for x in range(0, 32, 4)][:24]
    n = len(pos)
    blocks = np.array([(0, x, y) for x, y in pos], R.INTER_BLK)
    q = [(0, x, y, 4, 4, r0, r1) for x, y in pos for r0, r1 in [(1, 8), (5, 8), (1, 5)]]
    ctx, ln, st, rej = R.find_mvrefs_batch(grid, q)
    assert rej == 0
    stacks = np.zeros(n * 3, R.MVREF_RESULT)
    stacks["mode_context"], stacks["n"], stacks["stack"] = ctx, ln, st
    stacks = stacks.reshape(n, 3)
    c = _case(b, "one", bd, True, False, 2, True)
    cmv = c["cmv"][:n]
    po, pr = _dev_planes(bd)
    dtiles = np.array(tiles, np.int32).view(R.INTRA_TILE).reshape(-1)
    dme, res, rej = R.motion_estimation_batch(po, pr, dtiles, blocks, sets, stacks, cmv, c["tile_mvs"],
                                              c["prev_mvs"], b, W4, H4, LAMBDA, True, False, bd,
                                              device=True)
    assert rej == 0 and isinstance(dme, R.DeviceBuffer)
    lists, jobs, rej = R.inter_mode_set_batch(stacks, dme, sets, True, blocks)
    assert rej == 0
    # the references: the searches, then the mode set over their MVs
    org, refs = _pixels(bd)
    want_me = np.zeros((n, 2, 2), np.int16)
    for k, (x, y) in enumerate(pos):
        for i, (ref, slot) in enumerate([(1, 0), (5, 1)]):
            want_me[k, i], cost = M.motion_estimation(
                org, refs[slot], GEOM, W4, H4, tiles[0], x, y, int(b), int(stacks[k, i]["n"]),
                stacks[k, i]["stack"]["this_mv"], tuple(int(v) for v in cmv[k, i]),
                c["tile_mvs"][ref - 1], c["prev_mvs"][ref - 1], LAMBDA, True, False, bd)
            assert int(res[k, i]["cost"]) == cost
    assert (dme.download(np.int16, n * 4).reshape(n, 2, 2) == want_me).all()
    assert (want_me != 0).any()
    wl, wj, wr = _expected_lists(stacks, want_me, sets, True, blocks)
    assert wr == 0 and lists.tobytes() == wl.tobytes() and jobs.tobytes() == wj.tobytes()
    assert (lists["cand"]["luma_mode"] == R.PredictionMode.NEWMV).any()
    # luma prediction of every candidate, candidate k into destination set k
    nd = int(lists["n"].max())
    dsts = [[R.DevicePlane.from_full(np.zeros_like(org), PAD, PAD, FW, FH, bit_depth=bd)]
            for _ in range(nd)]
    assert R.motion_compensate_batch(pr, dsts, dtiles, jobs.reshape(-1), b, 0, True, bd) == 0
    host = [[F.RefPlane(r, PAD, PAD, FW, FH)] for r in refs]
    for k in range(nd):
        got = dsts[k][0].download_visible()
        for i, (x, y) in enumerate(pos):
            j = wj[i, k]
            if j["tile"] < 0:
                continue
            w = F.motion_compensate(host, tiles[0], (x, y), int(b), tuple(int(v) for v in j["ref_slot"]),
                                    [tuple(int(v) for v in m) for m in j["mv"]], 0, bd, luma_only=True)
            px, py, blk = w[0]
            assert (got[py:py + 16, px:px + 16] == blk).all(), (k, i)

"""The inter front of rdo_mode_decision on the device (rv_inter.hip): the
reference sets, the inter mode set and motion_compensate.

CPU: tests/inter_front_ref.py (the checker) against every vector of
tests/golden/ref_inter_front.npz, which tools/refeval/gen_inter_front_ref.py
made from the reference's text; rv_inter_ref_sets_build against the vectors
and hand cases; every error code of rv_motion_compensate_batch without a
device; the exports.

GPU (tolerance 0): rv_motion_compensate_batch and rv_inter_mode_set_batch
against the checker, and the chain find_mvrefs -> mode set -> motion
compensation -> transform blocks.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rav1e_amd as R
from tests import inter_front_ref as F
from tests import tx_blocks_ref as T

B, PM = R.BlockSize, R.PredictionMode
EINVAL, ENOTSUP = R.RV_EINVAL, R.RV_ENOTSUP
GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_inter_front.npz")


@functools.lru_cache(None)
def gold():
    return dict(np.load(GOLD))


# ------------------------------------------------------------------ CPU
def test_get_params_and_clamp_equal_reference():
    g = gold()["gp_cases"]
    res16 = {(0, 0): set(), (1, 1): set(), (1, 0): set()}
    clamps = set()
    for xd, yd, w, h, xo, yo, tx, ty, px, py, r, c, rf, cf, x, y in g.tolist():
        po = ((tx >> xd) + px, (ty >> yd) + py)
        got = F.get_params((r, c), po, xd, yd, w, h, xo, yo)
        assert got == (rf, cf, x, y), (xd, yd, po, r, c, got, (rf, cf, x, y))
        res16[(xd, yd)].add((r % 16, r < 0))
        res16[(xd, yd)].add((c % 16, c < 0))
        clamps.add((x == w + 3, x == 3 - xo, y == h + 3, y == 3 - yo))
    for k, v in res16.items():  # every residue mod 16 with both signs, per decimation
        assert {a for a, neg in v if neg} == set(range(16)) == {a for a, neg in v if not neg}, k
    assert {-32768, -32767, 32767} <= set(g[:, 10].tolist()) | set(g[:, 11].tolist())
    # each of the four clamps alone and the four corners
    for want in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 0), (1, 0, 0, 1),
                 (0, 1, 1, 0), (0, 1, 0, 1), (0, 0, 0, 0)):
        assert tuple(bool(v) for v in want) in clamps, want


def _vector_planes(bd, fmt):
    """The two reference frames of a pixel case, padded like the encoder's."""
    g = gold()
    W_, H_, pad = (int(v) for v in g["px_geom"][:3])
    xdec, ydec = ((1, 1), (0, 0))[fmt]
    flat = g["px_bd%d_f%d" % (bd, fmt)].astype(np.uint16 if bd > 8 else np.uint8)
    sets, off = [], 0
    for _ in range(2):
        planes = []
        for p in range(3):
            xd, yd = (xdec, ydec) if p else (0, 0)
            w, h = W_ >> xd, H_ >> yd
            vis = flat[off:off + w * h].reshape(h, w)
            off += w * h
            px, py = pad >> xd, pad >> yd
            planes.append(F.RefPlane(np.pad(vis, ((py, py), (px, px)), mode="edge"), px, py, w, h,
                                     xd, yd))
        sets.append(planes)
    return sets


def test_motion_compensate_pixels_equal_reference():
    g = gold()
    tile = tuple(int(v) for v in g["px_geom"][3:7])
    pred, off = g["px_pred"], 0
    seen = set()
    for bd, fmt, b, comp, mode, bx, by, r0, c0, r1, c1 in g["px_cases"].tolist():
        sets = _vector_planes(bd, fmt)
        got = F.motion_compensate(sets, tile, (bx, by), b, (0, 1 if comp else -1),
                                  [(r0, c0), (r1, c1)], mode, bd)
        for p in range(3):
            x, y, blk = got[p]
            want = pred[off:off + blk.size].reshape(blk.shape)
            off += blk.size
            assert (blk == want).all(), (bd, fmt, b, comp, p)
        seen.add((bd, b, comp, fmt))
    assert off == len(pred)
    assert seen == {(bd, b, comp, 0 if b != 6 else 1) for bd in (8, 10) for b in (3, 4, 5, 6)
                    for comp in (0, 1)}


def _vector_mode_case(k):
    g = gold()
    cfg = g["ms_cfg"][k].tolist()
    ns, comp, fwd, bwd, near = cfg[:5]
    refs, slots = cfg[5:5 + ns], cfg[12:12 + ns]
    st = g["ms_stacks"][k]
    stacks = []
    for i in range(ns + comp):
        n = int(st[i, 1])
        e = st[i, 2:2 + 4 * n].reshape(n, 4)
        stacks.append((int(st[i, 0]), [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in e]))
    me = [tuple(int(v) for v in m) for m in g["ms_me"][k][:ns]]
    return ns, comp, fwd, bwd, near, refs, slots, stacks, me


def test_mode_set_equals_reference():
    g = gold()
    counts = g["ms_count"]
    lens, rejected = set(), 0
    for k in range(len(counts)):
        ns, comp, fwd, bwd, near, refs, slots, stacks, me = _vector_mode_case(k)
        got = F.mode_set(stacks, me, refs, fwd, bwd, bool(comp), bool(near))
        if counts[k] < 0:
            assert got is None, k
            rejected += 1
            continue
        assert got is not None and len(got) == counts[k], k
        want = g["ms_cands"][k][:counts[k]].tolist()
        flat = [[m, s, r[0], r[1], mv[0][0], mv[0][1], mv[1][0], mv[1][1], ctx]
                for m, s, r, mv, ctx in got]
        assert flat == want, k
        lens |= {len(s[1]) for s in stacks}
    assert lens == {0, 1, 2, 3, 4, 9} and rejected >= 2


def _lib_sets(allowed, rf, rm, b):
    s = R.inter_ref_sets(allowed, rf, rm, b)
    return (list(s.ref[:s.n_single]), list(s.slot[:s.n_single]), s.fwd, s.bwd, bool(s.compound))


def test_ref_sets_equal_reference_and_hand_cases():
    for row in gold()["rs_cases"].tolist():
        na = row[0]
        allowed, rf, rm, b, ns = row[1:1 + na], row[8:15], row[15], row[16], row[17]
        want = (row[18:18 + ns], row[25:25 + ns], row[32], row[33], bool(row[34]))
        assert F.ref_sets(allowed, rf, rm, b) == want, row
        assert _lib_sets(allowed, rf, rm, b) == want, row
    ALL = [1, 2, 3, 4, 5, 6, 7]
    # LAST3 skipped although its slot is its own
    assert _lib_sets(ALL, [0, 1, 2, 3, 4, 5, 6], 1, B.BLOCK_16X16) == \
        ([1, 2, 4, 5, 6, 7], [0, 1, 3, 4, 5, 6], 0, 3, True)
    # two RefTypes on one slot are one set; the first backward set moves up
    assert _lib_sets(ALL, [0, 0, 2, 1, 1, 3, 3], 1, B.BLOCK_16X16) == \
        ([1, 4, 6], [0, 1, 3], 0, 2, True)
    # no backward reference: no compound set
    assert _lib_sets([1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 6], 1, B.BLOCK_16X16) == \
        ([1, 2, 4], [0, 1, 3], 0, -1, False)
    # 8x8 takes compound, 8x4 / 4x8 / 4x4 do not; nor does reference_mode SINGLE
    assert _lib_sets(ALL, [0, 1, 2, 3, 4, 5, 6], 1, B.BLOCK_8X8)[4] is True
    for b in (B.BLOCK_8X4, B.BLOCK_4X8, B.BLOCK_4X4, B.BLOCK_16X4):
        assert _lib_sets(ALL, [0, 1, 2, 3, 4, 5, 6], 1, b)[4] is False
    assert _lib_sets(ALL, [0, 1, 2, 3, 4, 5, 6], 0, B.BLOCK_16X16)[4] is False
    for bad in (([3], [0] * 7, 1, 6), ([0], [0] * 7, 1, 6), ([1], [8] + [0] * 6, 1, 6),
                ([1], [0] * 7, 1, 22)):
        with pytest.raises(R.Rav1eHipError) as e:
            R.inter_ref_sets(*bad)
        assert e.value.code == EINVAL


def test_symbols_exported():
    names = R.exported_symbols_from_header()
    L = R.lib()
    for n in ("rv_inter_ref_sets_build", "rv_inter_mode_set_batch", "rv_motion_compensate_batch"):
        assert n in names and getattr(L, n)
    assert C.sizeof(R.RvInterRefSets) == 18 * 4 and C.sizeof(R.RvInterMcParams) == 16
    assert R.INTER_CAND.itemsize == 28 and R.INTER_LIST.itemsize == 4 + 20 * 28
    assert R.INTER_MC_JOB.itemsize == 32 and R.INTER_BLK.itemsize == 12


FW, FH, PAD = 160, 152, 88  # the frame; SB_SIZE + FRAME_MARGIN of padding (src/frame/mod.rs:60)


def _fake_sets(n, base, fmt="420", hbd=0, **change):
    """n plane sets of descriptors whose data pointers are never dereferenced:
    every call made with them is refused before a launch."""
    xdec, ydec = F.LAYOUTS[fmt]
    arr = (R.RvPlane * (3 * n))()
    for s in range(n):
        for p in range(3):
            d = arr[3 * s + p]
            xd, yd = (xdec, ydec) if p else (0, 0)
            R.lib().rv_plane_geometry(C.byref(d), FW >> xd, FH >> yd, xd, yd, PAD >> xd, PAD >> yd, hbd)
            d.data = base + (3 * s + p) * (1 << 20)
    for k, v in change.items():
        setattr(arr[1], k, v)
    return arr


def test_motion_compensate_error_codes_without_a_device():
    L = R.lib()
    fake = C.c_void_p(0x1000)

    def call(bsize=B.BLOCK_16X16, mode=0, bd=8, luma_only=0, refs=None, dsts=None, n_refs=3,
             n_dsts=2, n=1, jobs=fake, tiles=fake, status=fake, params=True, lanes=0, fmt="420"):
        refs = _fake_sets(3, 0x10000000, fmt, bd > 8) if refs is None else refs
        dsts = _fake_sets(2, 0x20000000, fmt, bd > 8) if dsts is None else dsts
        prm = R.RvInterMcParams(int(bsize), mode, luma_only, bd)
        return L.rv_motion_compensate_batch_lanes(refs, n_refs, dsts, n_dsts, tiles, 1, jobs, n,
                                                  C.byref(prm) if params else None, status, lanes,
                                                  None)
    for b in (B.BLOCK_4X4, B.BLOCK_4X8, B.BLOCK_8X4):            # 4xN / Nx4
        assert call(bsize=b) == ENOTSUP
    for b in (B.BLOCK_4X16, B.BLOCK_16X4, B.BLOCK_64X16, B.BLOCK_64X128, B.BLOCK_128X128):
        assert call(bsize=b) == ENOTSUP                          # 4:1 / 1:4, above 64x64
    for b in (B.BLOCK_8X16, B.BLOCK_16X32, B.BLOCK_32X64):      # no subsampled_size at 4:2:2
        assert call(bsize=b, fmt="422") == ENOTSUP
    assert b"rv_motion_compensate_batch" in L.rv_last_error()
    assert call(bsize=-1) == EINVAL and call(bsize=22) == EINVAL
    assert call(mode=4) == EINVAL and call(mode=-1) == EINVAL
    assert call(bd=9) == EINVAL
    assert call(bd=10, refs=_fake_sets(3, 0x10000000)) == EINVAL     # u8 planes at 10 bit
    assert call(bd=8, dsts=_fake_sets(2, 0x20000000, hbd=1)) == EINVAL
    assert call(dsts=_fake_sets(2, 0x20000000, "444")) == EINVAL     # subsampling differs
    assert call(dsts=_fake_sets(2, 0x20000000, stride=512)) == EINVAL  # geometry differs
    assert call(refs=_fake_sets(3, 0x10000000, xorigin=40)) == EINVAL
    assert call(dsts=_fake_sets(2, 0x10000000 + 2 * 3 * (1 << 20))) == EINVAL  # dst aliases ref 2
    assert call(dsts=_fake_sets(2, 0x10000000 + 100)) == EINVAL      # a partial overlap
    assert call(refs=None, dsts=None, params=False) == EINVAL
    assert call(jobs=None) == EINVAL and call(tiles=None) == EINVAL and call(status=None) == EINVAL
    assert L.rv_motion_compensate_batch(None, 3, _fake_sets(2, 0x20000000), 2, fake, 1, fake, 1,
                                        C.byref(R.RvInterMcParams(6, 0, 0, 8)), fake, None) == EINVAL
    nul = _fake_sets(3, 0x10000000)
    nul[4].data = None
    assert call(refs=nul) == EINVAL
    assert call(n_refs=0) == EINVAL and call(n_refs=9) == EINVAL
    assert call(n_dsts=0) == EINVAL and call(n_dsts=21) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(lanes=48) == EINVAL and call(lanes=8) == EINVAL and call(lanes=512) == EINVAL
    # a reference whose padding cannot hold the furthest clamped window:
    # 64 pixels of padding end before column width + 64 + 6 of a 64x64 block
    def thin(n, base, pad):
        arr = (R.RvPlane * (3 * n))()
        for k in range(3 * n):
            xd = 1 if k % 3 else 0
            L.rv_plane_geometry(C.byref(arr[k]), FW >> xd, FH >> xd, xd, xd, pad >> xd, pad >> xd, 0)
            arr[k].data = base + k * (1 << 20)
        return arr
    assert call(bsize=B.BLOCK_64X64, refs=thin(3, 0x10000000, 64), dsts=thin(2, 0x20000000, 64)) == EINVAL
    assert call(bsize=B.BLOCK_64X64, refs=thin(3, 0x10000000, 64), dsts=thin(2, 0x20000000, 64),
                luma_only=1) == EINVAL


def test_mode_set_argument_errors_without_a_device():
    L = R.lib()
    fake = C.c_void_p(0x1000)
    s = R.inter_ref_sets([1, 5], [0, 0, 0, 0, 1, 1, 1], 1, B.BLOCK_16X16)
    assert L.rv_inter_mode_set_batch(None, fake, None, 4, s, 0, fake, None, fake, None) == EINVAL
    assert L.rv_inter_mode_set_batch(fake, fake, None, 4, s, 0, fake, fake, fake, None) == EINVAL
    assert L.rv_inter_mode_set_batch(fake, fake, None, -1, s, 0, fake, None, fake, None) == EINVAL
    assert L.rv_inter_mode_set_batch(fake, fake, None, 4, s, 0, fake, None, None, None) == EINVAL
    bad = R.RvInterRefSets()
    assert L.rv_inter_mode_set_batch(fake, fake, None, 4, bad, 0, fake, None, fake, None) == EINVAL
    s.bwd = 5
    assert L.rv_inter_mode_set_batch(fake, fake, None, 4, s, 0, fake, None, fake, None) == EINVAL


# ------------------------------------------------------------------ GPU
TILE_LIST = [(16, 8, 128, 128), (144, 8, 16, 128)]  # the second: the rest to the first's right
TILES = np.array(TILE_LIST, R.INTRA_TILE)
N_REFS = 3


@functools.lru_cache(None)
def _ref_pixels(bd, fmt):
    xdec, ydec = F.LAYOUTS[fmt]
    rng = np.random.default_rng(900 + 10 * bd + 2 * xdec + ydec)
    out = []
    for s in range(N_REFS):
        planes = []
        for p in range(3):
            xd, yd = (xdec, ydec) if p else (0, 0)
            a = rng.integers(0, 1 << bd, (FH >> yd, FW >> xd))
            a[:3, :] = (1 << bd) - 1  # saturated edges: what the clamp replicates
            a[:, -2:] = 0
            planes.append(a.astype(np.uint16 if bd > 8 else np.uint8))
        out.append(planes)
    return out


@functools.lru_cache(None)
def _refs(bd, fmt):
    """(device plane sets, the checker's RefPlanes of the same memory)"""
    xdec, ydec = F.LAYOUTS[fmt]
    dev = [[R.DevicePlane.from_array(a, xpad=PAD >> (xdec if p else 0), ypad=PAD >> (ydec if p else 0),
                                     xdec=xdec if p else 0, ydec=ydec if p else 0, bit_depth=bd)
            for p, a in enumerate(s)] for s in _ref_pixels(bd, fmt)]
    host = [[F.RefPlane.from_device(pl) for pl in s] for s in dev]
    return dev, host


def _dsts(n, bd, fmt):
    xdec, ydec = F.LAYOUTS[fmt]
    fill = (1 << bd) - 3
    dt = np.uint16 if bd > 8 else np.uint8
    return [[R.DevicePlane.from_array(np.full((FH >> (ydec if p else 0), FW >> (xdec if p else 0)), fill, dt),
                                      xpad=PAD >> (xdec if p else 0), ypad=PAD >> (ydec if p else 0),
                                      xdec=xdec if p else 0, ydec=ydec if p else 0, bit_depth=bd)
             for p in range(3)] for _ in range(n)]


def _check_launch(jobs, b, bd, fmt, n_dsts, mode=0, luma_only=False, want_rejected=0, valid=None,
                  lanes=0):
    """One launch against the checker: every destination plane whole, padding
    included, so the sentinel is seen to survive outside the blocks."""
    dev, host = _refs(bd, fmt)
    dsts = _dsts(n_dsts, bd, fmt)
    before = [[pl.download_full() for pl in s] for s in dsts]
    rej = R.motion_compensate_batch(dev, dsts, TILES, jobs, b, mode, luma_only, bd, lanes)
    assert rej == want_rejected
    for k, j in enumerate(jobs):
        if int(j["tile"]) < 0 or (valid is not None and not valid[k]):
            continue
        got = F.motion_compensate(host, TILE_LIST[int(j["tile"])], (int(j["bo_x"]), int(j["bo_y"])),
                                  int(b), tuple(int(v) for v in j["ref_slot"]),
                                  [tuple(int(v) for v in m) for m in j["mv"]], int(mode), bd, luma_only)
        for p, (x, y, blk) in got.items():
            d = dsts[int(j["dst_set"])][p].desc
            before[int(j["dst_set"])][p][d.yorigin + y:d.yorigin + y + blk.shape[0],
                                         d.xorigin + x:d.xorigin + x + blk.shape[1]] = blk
    for s in range(n_dsts):
        for p in range(3):
            assert (dsts[s][p].download_full() == before[s][p]).all(), ("dst", s, p)
    for s in range(N_REFS):  # the references are only read
        assert (dev[s][0].download_full() == host[s][0].full).all()


# MVs (row, col) in 1/8 pel: zero; whole pixels in every plane; one axis
# fractional; far outside on each side and corner (the clamp); the extremes
FIXED_MVS = [(0, 0), (32, -48), (-16, 16), (5, 16), (-32, 3), (-3, -16), (48, -7),
             (3200, 0), (-3200, 0), (0, 3200), (0, -3200), (3203, 3205), (3203, -3205),
             (-3203, 3205), (-3203, -3205), (32767, -32768), (-32768, 32767)]


def _mv(k):
    if k < len(FIXED_MVS):
        return FIXED_MVS[k]
    # every residue mod 16 on both axes (every chroma frac), both signs
    return ((k % 16) - 16 * (k % 5), ((7 * k + 3) % 16) + 16 * ((k % 7) - 3))


def _jobs(b, n_dsts, limit=64):
    """Positions of both tiles, each (position, dst_set) used once; single
    and compound jobs alternate."""
    bw4, bh4 = F.BLK_W[b] // 4, F.BLK_H[b] // 4
    slots = []
    for t, (tx, ty, tw, th) in enumerate(TILE_LIST):
        nx, ny = tw // 4 // bw4, th // 4 // bh4
        pos = [(x, y) for y in range(ny) for x in range(nx)]
        rng = np.random.default_rng(31 * b + t)
        rng.shuffle(pos)
        keep = pos[:max(1, (limit // n_dsts) * (3 if t == 0 else 1) // 4)]
        slots += [(t, x * bw4, y * bh4) for x, y in keep]
    jobs = np.zeros(min(limit, len(slots) * n_dsts), R.INTER_MC_JOB)
    for k in range(len(jobs)):
        t, x, y = slots[k // n_dsts]
        comp = k % 2
        jobs[k] = (t, x, y, k % n_dsts, (k % N_REFS, (k // 3 + 1) % N_REFS if comp else -1),
                   (_mv(k), _mv(3 * k + 1)))
    return jobs


CASES = [(b, fmt) for b in F.SIZES for fmt in ("444", "422", "420")
         if F.has_subsampled_size(b, *F.LAYOUTS[fmt])]


@pytest.mark.gpu
@pytest.mark.parametrize("b,fmt", CASES, ids=["%dx%d-%s" % (F.BLK_W[b], F.BLK_H[b], f) for b, f in CASES])
def test_gpu_motion_compensate_every_size_and_layout(b, fmt):
    R.require_device(0)
    assert len(CASES) == 27
    jobs = _jobs(b, 4)
    assert 0 < len(jobs) <= 64 and (jobs["ref_slot"][:, 1] >= 0).any() and (jobs["ref_slot"][:, 1] < 0).any()
    if F.BLK_W[b] <= 16:
        assert (jobs["tile"] == 1).any()  # the tile translation
    for bd in (8, 10, 12):
        _check_launch(jobs, b, bd, fmt, 4)
    _check_launch(jobs, b, 8, fmt, 4, luma_only=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["regular", "smooth", "sharp", "bilinear"])
def test_gpu_filter_modes(mode):
    """8x8 and 16x8 at 4:2:0 have 4-long chroma sides: the 4-tap sets."""
    R.require_device(0)
    for b in (B.BLOCK_8X8, B.BLOCK_16X8, B.BLOCK_32X32):
        _check_launch(_jobs(b, 2, 32), b, 8, "420", 2, mode=mode)
    _check_launch(_jobs(B.BLOCK_16X8, 2, 32), B.BLOCK_16X8, 10, "420", 2, mode=mode)


@pytest.mark.gpu
def test_gpu_lanes_per_job_do_not_change_the_result():
    R.require_device(0)
    for b in (B.BLOCK_8X8, B.BLOCK_32X16):
        for lanes in (16, 32, 64, 128, 256):
            if b == B.BLOCK_32X16 and lanes == 16:  # 16 jobs' windows exceed a workgroup's LDS
                with pytest.raises(R.Rav1eHipError) as e:
                    _check_launch(_jobs(b, 2, 40), b, 8, "420", 2, lanes=lanes)
                assert e.value.code == EINVAL
                continue
            _check_launch(_jobs(b, 2, 40), b, 8, "420", 2, lanes=lanes)


@pytest.mark.gpu
def test_gpu_candidates_at_one_position():
    """Twenty candidates of one block go to twenty destination sets."""
    R.require_device(0)
    for b, bd in ((B.BLOCK_16X16, 8), (B.BLOCK_8X8, 10)):
        jobs = np.zeros(40, R.INTER_MC_JOB)
        for k in range(40):
            jobs[k] = (k // 20, 4 if k < 20 else 0, 8, k % 20, (k % 3, (k + 1) % 3 if k % 4 == 1 else -1),
                       (_mv(k + 2), _mv(5 * k)))
        _check_launch(jobs, b, bd, "420", 20)


@pytest.mark.gpu
def test_gpu_rejected_jobs_write_nothing():
    R.require_device(0)
    b = B.BLOCK_16X16
    good = _jobs(b, 2, 12)
    bad = np.zeros(9, R.INTER_MC_JOB)
    bad[:] = good[0]
    bad["dst_set"] = 1
    bad[0]["tile"] = 2                   # no such tile
    bad[1]["ref_slot"] = (N_REFS, -1)    # no such reference set
    bad[2]["ref_slot"] = (0, N_REFS)
    bad[3]["ref_slot"] = (-1, -1)
    bad[4]["dst_set"] = 2                # no such destination set
    bad[5]["dst_set"] = -1
    bad[6]["bo_x"] = 2                   # not a multiple of the block
    bad[7]["bo_y"] = 32                  # leaves the tile (128 rows)
    bad[8]["bo_x"] = -4
    skip = good[:2].copy()
    skip["tile"] = -1                    # skipped, not counted
    jobs = np.concatenate([good[:5], bad[:4], skip, good[5:], bad[4:]])
    valid = np.concatenate([np.ones(5, bool), np.zeros(4, bool), np.zeros(2, bool),
                            np.ones(len(good) - 5, bool), np.zeros(5, bool)])
    _check_launch(jobs, b, 8, "420", 2, want_rejected=9, valid=valid)
    only_bad = bad.copy()
    _check_launch(only_bad, b, 10, "444", 2, want_rejected=9, valid=np.zeros(9, bool))


def _results_to_stacks(row):
    return [(int(r["mode_context"]), [(tuple(int(v) for v in r["stack"][k]["this_mv"]),
                                        tuple(int(v) for v in r["stack"][k]["comp_mv"]))
                                       for k in range(int(r["n"]))]) for r in row]


def _expected_lists(stacks, me, sets, near, blocks=None):
    n = len(stacks)
    ns = sets.n_single
    refs, slots = list(sets.ref[:ns]), list(sets.slot[:ns])
    lists = np.zeros(n, R.INTER_LIST)
    jobs = np.zeros((n, R.INTER_MAX_CANDS), R.INTER_MC_JOB)
    jobs["tile"] = -1
    jobs["ref_slot"][:, :, 1] = -1
    rejected = 0
    for i in range(n):
        got = F.mode_set(_results_to_stacks(stacks[i]), [tuple(int(v) for v in m) for m in me[i]],
                         refs, sets.fwd, sets.bwd, bool(sets.compound), near)
        if got is None:
            rejected += 1
            continue
        lists[i]["n"] = len(got)
        for k, (mode, s, r, mv, ctx) in enumerate(got):
            lists[i]["cand"][k] = (mode, s, r, mv, ctx)
            if blocks is not None:
                sl = (slots[s], -1) if s < ns else (slots[sets.fwd], slots[sets.bwd])
                jobs[i, k] = (blocks[i]["tile"], blocks[i]["bo_x"], blocks[i]["bo_y"], k, sl, mv)
    return lists, jobs, rejected


def _random_stacks(rng, n, nsets, ns):
    st = np.zeros((n, nsets), R.MVREF_RESULT)
    me = rng.integers(-6, 7, (n, ns, 2)).astype(np.int16)
    me[rng.random((n, ns)) < 0.15] = 0
    st["mode_context"] = rng.integers(0, 512, (n, nsets))
    st["n"] = rng.choice([0, 1, 2, 3, 4, 9], (n, nsets))
    st["stack"]["this_mv"] = rng.integers(-6, 7, (n, nsets, 9, 2))
    st["stack"]["comp_mv"] = rng.integers(-300, 300, (n, nsets, 9, 2))
    st["stack"]["weight"] = rng.integers(0, 1000, (n, nsets, 9))
    for i in range(n):  # the search's MV somewhere in its stack, often
        for s in range(ns):
            if rng.random() < 0.5:
                st["stack"]["this_mv"][i, s, int(rng.integers(0, 5))] = me[i, s]
    live = np.arange(9)[None, None, :] < st["n"][:, :, None]
    for f in ("this_mv", "comp_mv"):
        st["stack"][f] *= live[..., None]
    st["stack"]["weight"] *= live
    return st, me


@pytest.mark.gpu
@pytest.mark.parametrize("near", [False, True])
def test_gpu_mode_set_random_blocks(near):
    R.require_device(0)
    rng = np.random.default_rng(77 + near)
    ALL = [1, 2, 3, 4, 5, 6, 7]
    total_rejected = 0
    for allowed, rf, rm in ((ALL, [0, 0, 0, 0, 1, 1, 1], 1), (ALL, [0, 1, 0, 0, 2, 2, 2], 1),
                            ([1], [0] * 7, 1), (ALL, [0, 1, 2, 3, 4, 5, 6], 0)):
        sets = R.inter_ref_sets(allowed, rf, rm, B.BLOCK_16X16)
        n = 300
        st, me = _random_stacks(rng, n, sets.n_sets, sets.n_single)
        blocks = np.zeros(n, R.INTER_BLK)
        blocks["tile"], blocks["bo_x"], blocks["bo_y"] = rng.integers(0, 2, n), 4 * rng.integers(0, 8, n), \
            4 * rng.integers(0, 8, n)
        lists, jobs, rej = R.inter_mode_set_batch(st, me, sets, near, blocks)
        wl, wj, wr = _expected_lists(st, me, sets, near, blocks)
        assert rej == wr
        total_rejected += wr
        assert lists.tobytes() == wl.tobytes()
        assert jobs.tobytes() == wj.tobytes()
        # without the jobs
        lists2, none, rej2 = R.inter_mode_set_batch(st, me, sets, near)
        assert none is None and rej2 == wr and lists2.tobytes() == wl.tobytes()
    assert total_rejected > 0 or not near  # three single sets with near MVs overflow the list


@pytest.mark.gpu
def test_gpu_mode_set_reference_cases():
    """The vectors' hand cases, both rejections among them, one block a launch
    group: cases of one configuration share a launch."""
    R.require_device(0)
    g = gold()
    groups = {}
    for k in range(len(g["ms_count"])):
        groups.setdefault(tuple(g["ms_cfg"][k].tolist()), []).append(k)
    rejected = 0
    for cfg, ks in groups.items():
        ns, comp, fwd, bwd, near = cfg[:5]
        sets = R.RvInterRefSets(ns, (C.c_int32 * 7)(*cfg[5:12]), (C.c_int32 * 7)(*cfg[12:19]), fwd,
                                bwd, comp)
        st = np.zeros((len(ks), ns + comp), R.MVREF_RESULT)
        me = np.zeros((len(ks), ns, 2), np.int16)
        for i, k in enumerate(ks):
            v = g["ms_stacks"][k]
            for s in range(ns + comp):
                st["mode_context"][i, s], st["n"][i, s] = v[s, 0], v[s, 1]
                e = v[s, 2:38].reshape(9, 4)
                st["stack"]["this_mv"][i, s], st["stack"]["comp_mv"][i, s] = e[:, :2], e[:, 2:]
            me[i] = g["ms_me"][k][:ns]
        lists, _, rej = R.inter_mode_set_batch(st, me, sets, bool(near))
        want_rej = 0
        for i, k in enumerate(ks):
            c = int(g["ms_count"][k])
            if c < 0:
                want_rej += 1
                assert lists[i]["n"] == 0
                continue
            assert lists[i]["n"] == c
            got = lists[i]["cand"][:c]
            flat = np.concatenate([got["luma_mode"][:, None], got["set"][:, None], got["ref"],
                                   got["mv"].reshape(c, 4), got["mode_context"][:, None]], axis=1)
            assert (flat == g["ms_cands"][k][:c]).all(), k
        assert rej == want_rej
        rejected += rej
    assert rejected == int((g["ms_count"] < 0).sum()) >= 2


@pytest.mark.gpu
def test_gpu_chain_stacks_to_levels():
    """find_mvrefs_batch on a painted grid -> inter_mode_set_batch with its MC
    jobs -> motion_compensate_batch -> tx_blocks_batch with pred = one
    destination set; the levels equal tests/tx_blocks_ref.py on the checker's
    prediction."""
    R.require_device(0)
    b, bd, fmt = B.BLOCK_16X16, 8, "420"
    rng = np.random.default_rng(5)
    tile = TILE_LIST[0]
    # the tile's grid: 8x8 inter blocks on LAST / BWDREF with small MVs
    cells = R.default_block_grid(1, 32, 32)
    for y in range(0, 32, 2):
        for x in range(0, 32, 2):
            c = cells[0, y:y + 2, x:x + 2]
            two = rng.random() < 0.4
            c["ref"] = (1, 5) if two else ((1, 8) if rng.random() < 0.6 else (5, 8))
            c["n4_w"] = c["n4_h"] = 2
            c["newmv"] = rng.random() < 0.5
            c["mv"] = rng.integers(-40, 41, (2, 2))
    grid = R.BlockGrid.from_array(cells, [(32, 32, tile[0] // 4, tile[1] // 4)], frame_cols=FW // 4,
                                  frame_rows=FH // 4, sign_bias=1 << 4)
    sets = R.inter_ref_sets([1, 2, 3, 4, 5, 6, 7], [0, 0, 0, 0, 1, 1, 1], True, b)
    assert (sets.n_single, sets.compound, sets.fwd, sets.bwd) == (2, 1, 0, 1)
    pos = [(4 * x, 4 * y) for y in range(1, 8, 2) for x in range(0, 8, 2)]
    n = len(pos)
    blocks = np.array([(0, x, y) for x, y in pos], R.INTER_BLK)
    set_refs = [(1, 8), (5, 8), (1, 5)]
    q = [(0, x, y, 4, 4, r0, r1) for x, y in pos for r0, r1 in set_refs]
    ctx, ln, st, rej = R.find_mvrefs_batch(grid, q)
    assert rej == 0 and ln.max() >= 2
    res = np.zeros(n * 3, R.MVREF_RESULT)
    res["mode_context"], res["n"], res["stack"] = ctx, ln, st
    res = res.reshape(n, 3)
    me = rng.integers(-60, 61, (n, 2, 2)).astype(np.int16)
    lists, jobs, rej = R.inter_mode_set_batch(res, me, sets, True, blocks)
    wl, wj, wr = _expected_lists(res, me, sets, True, blocks)
    assert rej == wr == 0 and lists.tobytes() == wl.tobytes() and jobs.tobytes() == wj.tobytes()
    assert lists["n"].max() > 8
    # every candidate of every block in one launch, candidate k into set k
    dev, host = _refs(bd, fmt)
    nd = int(lists["n"].max())
    dsts = _dsts(nd, bd, fmt)
    assert R.motion_compensate_batch(dev, dsts, TILES, jobs.reshape(-1), b, 0, False, bd) == 0
    k = 0  # candidate 0 is NEARESTMV of set 0 for every block
    assert (lists["cand"][:, k]["luma_mode"] == PM.NEARESTMV).all()
    pred = [pl.download_visible() for pl in dsts[k]]
    want_pred = [np.full_like(a, (1 << bd) - 3) for a in pred]
    for i in range(n):
        j = jobs[i, k]
        got = F.motion_compensate(host, tile, pos[i], int(b), tuple(int(v) for v in j["ref_slot"]),
                                  [tuple(int(v) for v in m) for m in j["mv"]], 0, bd)
        for p, (x, y, blk) in got.items():
            want_pred[p][y:y + blk.shape[0], x:x + blk.shape[1]] = blk
    for p in range(3):
        assert (pred[p] == want_pred[p]).all()
    # the candidate's transform blocks from that prediction
    src = [a for a in _ref_pixels(bd, fmt)[2]]
    src_d = dev[2]
    tj = np.array([(0, x, y, 60 + 9 * i, 0, 0) for i, (x, y) in enumerate(pos)], R.TX_BLOCKS_JOB)
    ts = R.TxSize.TX_16X16
    lay, levels, eobs, dists = R.tx_blocks_batch(src_d, src_d, TILES[:1], tj, b, ts, PM.NEARESTMV,
                                                 bit_depth=bd, pred=dsts[k])
    nz = 0
    for i in range(n):
        r = T.run_job(src, src, want_pred, tile, pos[i][0], pos[i][1], int(b), int(ts), 0,
                      int(PM.NEARESTMV), 0, int(tj[i]["qindex"]), (0, 0), bd)
        for p in range(3):
            assert (levels[p][i] == r.levels[p]).all(), ("levels", i, p)
            assert (eobs[p][i] == r.eobs[p]).all() and (dists[p][i] == r.dists[p]).all()
            nz += int(np.count_nonzero(r.levels[p]))
    assert nz > 0

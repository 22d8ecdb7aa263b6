"""Intra edges and mode screening for every block size: the general
get_intra_edges (src/partition.rs:500-693) with has_top_right /
has_bottom_left (src/recon_intra.rs) and the fused screening (src/rdo.rs:
1029-1127).

CPU: tests/intra_screen_ref.py (the numpy restatement, the GPU tests'
checker) against the vectors the reference's own text produced
(tools/refeval/gen_intra_screen_ref.py -> tests/golden/ref_intra_screen.npz),
against the oracle's superblock-level form, on hand-built ties, and the
entry points' argument checks.  GPU: both entry points bit for bit against
the restatement."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import rav1e_amd as R
from tests import intra_screen_ref as X
from tests import oracle_lib as O

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_intra_screen.npz")


@functools.lru_cache(None)
def gold():
    return dict(np.load(GOLD))


# ---------------------------------------------------------------- CPU: golden
def _avail_cases():
    """The enumeration tools/refeval/gen_intra_screen_ref.py records: every
    required size, every aligned position of a 64x64 superblock, the three
    formats, the plane block and its half as transform size with every
    offset that fits."""
    for b in X.SIZES:
        for xdec, ydec in X.FORMATS:
            pw, ph = max(4, X.BLK_W[b] >> xdec), max(4, X.BLK_H[b] >> ydec)
            txs = [(pw, ph)]
            half = (max(4, pw // 2), max(4, ph // 2))
            if half != (pw, ph):
                txs.append(half)
            for tw, th in txs:
                for mi_row in range(0, 16, X.BLK_H[b] // 4):
                    for mi_col in range(0, 16, X.BLK_W[b] // 4):
                        for by in range(ph // th):
                            for bx in range(pw // tw):
                                yield (b, mi_col, mi_row, xdec, ydec, tw, th, by * (th // 4),
                                       bx * (tw // 4))


def test_availability_equals_reference():
    a = gold()["avail"]
    want = list(_avail_cases())
    assert len(a) == len(want) == 4263  # the enumerated total
    assert [tuple(r[:9]) for r in a.tolist()] == want
    seen_tr, seen_bl = set(), set()
    for (b, c, r, xd, yd, tw, th, ro, co, tr, bl) in a.tolist():
        sw, sh = X.supersample(X.BLK_W[b], X.BLK_H[b], xd, yd)
        for k in range(4):  # the four combinations of the two outer availabilities
            a0, a1 = bool(k & 1), bool(k & 2)
            got_tr = X.has_top_right(sw, sh, c, r, a0, a1, tw, ro, co, xd)
            got_bl = X.has_bottom_left(sw, sh, c, r, a0, a1, th, ro, co, yd)
            assert got_tr == bool(tr >> k & 1), ("tr", b, c, r, xd, yd, tw, th, ro, co, k)
            assert got_bl == bool(bl >> k & 1), ("bl", b, c, r, xd, yd, tw, th, ro, co, k)
        seen_tr.add((ro > 0, bool(tr >> 3 & 1)))
        seen_bl.add((co > 0, bool(bl >> 3 & 1)))
    # both answers in the row_off > 0 / == 0 branches; col_off > 0 is never available
    assert seen_tr == {(False, False), (False, True), (True, False), (True, True)}
    assert seen_bl == {(False, False), (False, True), (True, False)}


def _edge_region(g, pi):
    bd, xdec, ydec, pw, ph = (int(v) for v in g["edge_plane%d_cfg" % pi])
    full = g["edge_plane%d" % pi].astype(np.int64)
    pad = (full.shape[0] - ph) // 2
    tx0, ty0, tw, th = (int(v) for v in g["edge_tile"])
    x0, y0 = pad + (tx0 >> xdec), pad + (ty0 >> ydec)
    return bd, xdec, ydec, full[y0:y0 + (th >> ydec), x0:x0 + (tw >> xdec)]


def test_edges_equal_reference():
    g = gold()
    meta, out = g["edge_meta"], g["edge_out"]
    assert len(meta) == len(out) > 1000
    regions = {pi: _edge_region(g, pi) for pi in sorted(set(meta[:, 0].tolist()))}
    cov = set()
    for row, want in zip(meta.tolist(), out):
        pi, b, bo_x, bo_y, bx, by, po_x, po_y, tw, th, mode = row
        bd, xdec, ydec, reg = regions[pi]
        ts = X.tx_size_of(tw, th)
        got = X.get_intra_edges(reg, bo_x, bo_y, bx, by, b, po_x, po_y, ts, xdec, ydec, bd, mode)
        assert (got == want).all(), row
        # what the case exercises
        cov.add(("pos", po_x == 0, po_y == 0))
        cov.add(("fmt", xdec, ydec))
        cov.add(("bd", bd))
        cov.add(("mode", mode))
        cov.add(("size", b))
        if mode in (-1, 3, 8) and po_y != 0:
            avail = reg.shape[1] - po_x - tw
            sw, sh = X.supersample(X.BLK_W[b], X.BLK_H[b], xdec, ydec)
            has = X.has_top_right(sw, sh, bo_x, bo_y, True, avail > 0, tw, by * (th // 4),
                                  bx * (tw // 4), xdec)
            cov.add(("tr", has, 0 < avail < tw))
        if mode in (-1, 7) and po_x != 0:
            avail = reg.shape[0] - po_y - th
            sw, sh = X.supersample(X.BLK_W[b], X.BLK_H[b], xdec, ydec)
            has = X.has_bottom_left(sw, sh, bo_x, bo_y, avail > 0, True, th, by * (th // 4),
                                    bx * (tw // 4), ydec)
            cov.add(("bl", has, 0 < avail < th))
        if (xdec, ydec, b, tw, th) == (1, 1, 3, 4, 4):
            cov.add("420 8x8 partition's 4x4 chroma")
        if (xdec, ydec, b, tw, th) == (0, 0, 12, 32, 32) and bx and by:
            cov.add("444 64x64 partition's 32x32 blocks, row_off and col_off > 0")
    # a thin golden cannot pass quietly
    for x0 in (False, True):
        for y0 in (False, True):
            assert ("pos", x0, y0) in cov
    for f in X.FORMATS:
        assert ("fmt",) + f in cov
    for bd in (8, 10, 12):
        assert ("bd", bd) in cov
    for m in (-1, 0, 1, 2, 3, 4, 7, 8, 12, 13):
        assert ("mode", m) in cov
    for b in X.SIZES:
        assert ("size", b) in cov
    # top-right / bottom-left: available unclipped, clipped below the
    # transform size by the tile's edge, and unavailable
    for k in ("tr", "bl"):
        assert (k, True, False) in cov and (k, True, True) in cov and (k, False, False) in cov
    assert "420 8x8 partition's 4x4 chroma" in cov
    assert "444 64x64 partition's 32x32 blocks, row_off and col_off > 0" in cov


def _scr_regions(g, pi):
    tx0, ty0, tw, th = (int(v) for v in g["scr_tile"])
    rec, src = g["scr_rec%d" % pi], g["scr_src%d" % pi]
    pad = 8
    sl = (slice(pad + ty0, pad + ty0 + th), slice(pad + tx0, pad + tx0 + tw))
    return rec[sl].astype(np.int64), src[sl].astype(np.int64)


def test_screening_equals_reference():
    g = gold()
    meta = g["scr_meta"]
    cov = set()
    cache = {}
    for row, want_s, cdf_row, want_m in zip(meta.tolist(), g["scr_satd"], g["scr_row"],
                                            g["scr_modes"]):
        pi, b, bo_x, bo_y, kf, off, pert, num = row
        bd = (8, 10, 12)[pi]
        key = (pi, b, bo_x, bo_y)
        if key not in cache:
            rec, src = _scr_regions(g, pi)
            cache[key] = X.screen(rec, src, bo_x, bo_y, b, bd, cdf_row, num)[1]
        s = cache[key]
        assert s == want_s.tolist(), row
        modes = X.select(s, cdf_row, num)
        assert modes == [int(v) for v in want_m if v != 255], row
        assert R.intra_screen_select(s, cdf_row, num) == modes
        if not pert:  # the default row sits where intra_mode_cdf_offset says
            assert (_default_cdf()[off:off + 14] == cdf_row).all()
        cov |= {("size", b), ("kf", kf), ("num", num), ("pert", pert), ("bd", bd)}
    for b in X.SIZES:
        assert ("size", b) in cov
    for k in ("kf", "pert"):
        assert (k, 0) in cov and (k, 1) in cov
    assert ("num", 3) in cov and ("num", 7) in cov
    assert {("bd", 8), ("bd", 10), ("bd", 12)} <= cov


@functools.lru_cache(None)
def _default_cdf():
    """The combined default table (coefficient CDFs zero: not read here)."""
    hdr = open(os.path.join(os.path.dirname(R.__file__), "csrc", "rv_ec_mode_tables.h")).read()
    base = int(re.search(r"#define RV_ECM_PARTITION (\d+)", hdr).group(1))
    body = hdr[hdr.index("RV_ECM_DEFAULT_CDF["):]
    vals = [int(v) for v in re.findall(r"\d+", body[body.index("{"):body.index("}")])]
    return np.array([0] * base + vals, np.uint16)


def test_cdf_offsets_match_the_table_header():
    hdr = open(os.path.join(os.path.dirname(R.__file__), "csrc", "rv_ec_mode_tables.h")).read()
    assert int(re.search(r"#define RV_ECM_KF_Y (\d+)", hdr).group(1)) == R.ECM_KF_Y
    assert int(re.search(r"#define RV_ECM_Y_MODE (\d+)", hdr).group(1)) == R.ECM_Y_MODE
    B = R.BlockSize
    assert R.intra_mode_cdf_offset(R.FRAME_TYPE_INTER, B.BLOCK_4X8) == R.ECM_Y_MODE
    assert R.intra_mode_cdf_offset(R.FRAME_TYPE_INTER, B.BLOCK_8X8) == R.ECM_Y_MODE + 14
    assert R.intra_mode_cdf_offset(R.FRAME_TYPE_INTER, B.BLOCK_32X16) == R.ECM_Y_MODE + 28
    assert R.intra_mode_cdf_offset(R.FRAME_TYPE_INTER, B.BLOCK_64X64) == R.ECM_Y_MODE + 42
    # kf_y_cdf[above_ctx][left_ctx]: D45 -> 3, SMOOTH_H -> 2
    assert R.intra_mode_cdf_offset(R.FRAME_TYPE_KEY, B.BLOCK_8X8, 3, 11) == \
        R.ECM_KF_Y + (3 * 5 + 2) * 14
    assert R.intra_mode_cdf_offset(R.FRAME_TYPE_KEY, B.BLOCK_8X8) == R.ECM_KF_Y
    with pytest.raises(R.Rav1eHipError):
        R.intra_mode_cdf_offset(R.FRAME_TYPE_KEY, B.BLOCK_8X8, 14, 0)
    assert R.intra_plane_offset(5, 3, 1, 1) == (8, 4)
    assert R.intra_plane_offset(4, 8, 0, 0, 1, 1, R.TxSize.TX_32X32) == (48, 64)
    assert R.INTRA_BLK_JOB.itemsize == 32 and R.INTRA_TILE.itemsize == 16


# ------------------------------------------------- CPU: ties to the old checker
def test_superblock_level_equals_the_replay_checker():
    """At 64x64 superblock level the restatement equals orc_intra_edges_sb,
    and with the default y_mode row and 3 modes the selection is the
    replay's rule: DC_PRED first, then the lowest SATDs."""
    L = O.lib()
    L.orc_intra_edges_sb.restype = None
    L.orc_intra_edges_sb.argtypes = [C.c_void_p, C.c_ssize_t] + [C.c_int] * 9 + [C.c_void_p]
    rng = np.random.default_rng(5)
    for bd, (xdec, ydec) in ((8, (0, 0)), (10, (1, 1)), (12, (0, 0)), (8, (1, 1))):
        dt = np.uint16 if bd > 8 else np.uint8
        tw, th = 200 >> xdec, 136 >> ydec  # a tile of 3 x 2 superblocks and a bit
        reg = rng.integers(0, 1 << bd, (th, tw)).astype(dt)
        n = 64 >> xdec
        for sy in range(2):
            for sx in range(3):
                x, y = sx * n, sy * (64 >> ydec)
                want = np.zeros(257, dt)
                L.orc_intra_edges_sb(O.ptr(reg), tw, int(bd > 8), bd, tw, th, x, y, n,
                                     int(sy > 0), int(sx > 0), O.ptr(want))
                got = X.get_intra_edges(reg.astype(np.int64), sx * 16, sy * 16, 0, 0, 12, x, y,
                                        X.tx_size_of(n, n), xdec, ydec, bd)
                assert (got == want).all(), (bd, xdec, sx, sy)
    row = _default_cdf()[R.intra_mode_cdf_offset(R.FRAME_TYPE_INTER, 12):][:14]
    for _ in range(200):
        s = rng.integers(0, 50, 13).tolist()  # many equal values
        order = sorted(range(13), key=lambda k: s[k])
        want = [0]
        for k in order[:3]:
            if X.RAV1E_INTRA_MODES[k] not in want:
                want.append(X.RAV1E_INTRA_MODES[k])
        assert X.select(s, row, 3) == want[:3]


def test_ties_keep_the_stable_orders():
    # a flat source over a flat reconstruction: every mode predicts the same
    # block, all SATDs are equal, the SATD order is RAV1E_INTRA_MODES' own
    reg = np.full((64, 64), 77, np.int64)
    row = _default_cdf()[R.ECM_KF_Y:][:14]
    e, s, modes7 = X.screen(reg, reg, 4, 4, 6, 8, row, 7)
    assert len(set(s)) == 1 and s[0] == 0
    # a row with equal probabilities: the probability order is the set's too
    flat = np.array([32768 - 2520 * (i + 1) for i in range(13)] + [0], np.uint16)
    assert X.select(s, flat, 7) == X.RAV1E_INTRA_MODES[:7]
    assert X.select(s, flat, 3) == X.RAV1E_INTRA_MODES[:3]
    # default row: its 3 most probable modes first, then the set's order
    z, probs = 32768, []
    for a in row[:13]:
        probs.append(z - int(a))
        z = int(a)
    top = sorted(X.RAV1E_INTRA_MODES, key=lambda m: -probs[m])[:3]
    rest = [m for m in X.RAV1E_INTRA_MODES if m not in top]
    assert modes7 == (top + rest)[:7]
    # equal SATDs among the lowest: the earlier of RAV1E_INTRA_MODES wins
    s2 = [9, 5, 5, 5, 9, 9, 9, 5, 9, 9, 9, 9, 9]
    assert X.select(s2, flat, 3) == [0, 2, 1]  # 1 by probability order, then H, V (5, 5)
    assert X.select(s2, flat, 7)[:3] == [0, 2, 1]


# ---------------------------------------------------------- CPU: argument checks
def _call_edges(plane, bsize, tx, bd=8, mode=-1, n=1, out=1, tiles=1, jobs=1, n_tiles=1):
    return R.lib().rv_intra_edges_batch(C.byref(plane), tiles, n_tiles, jobs, n, bsize, tx, bd,
                                        mode, out, None)


def _call_screen(rec, src, bsize, num=3, bd=8, n=1, modes=1, cdf=1, tiles=1, jobs=1):
    return R.lib().rv_intra_screen_batch(C.byref(rec), C.byref(src), tiles, 1, jobs, n, bsize, bd,
                                         cdf, 6000, num, modes, None, None, None)


def _host_plane(xdec=0, ydec=0, hbd=0):
    p = R.RvPlane()
    R.lib().rv_plane_geometry(C.byref(p), 128, 128, xdec, ydec, 8, 8, hbd)
    p.data = 4096  # never dereferenced: every call below is refused before a launch
    return p


def test_invalid_arguments_return_their_code_without_a_launch():
    """No device is needed: the pointers are not device memory, so a launch
    would not come back with these codes."""
    B, T = R.BlockSize, R.TxSize
    p, pc = _host_plane(), _host_plane(1, 1)
    EINVAL, ENOTSUP = -1, -3
    # bad size
    assert _call_edges(p, 22, T.TX_4X4) == EINVAL
    assert _call_edges(p, -1, T.TX_4X4) == EINVAL
    assert _call_edges(p, B.BLOCK_8X8, 19) == EINVAL
    assert _call_screen(p, p, 22) == EINVAL
    # 4:1 / 1:4 sizes and sizes above 64x64
    for b in (B.BLOCK_4X16, B.BLOCK_16X4, B.BLOCK_8X32, B.BLOCK_32X8, B.BLOCK_16X64,
              B.BLOCK_64X16, B.BLOCK_64X128, B.BLOCK_128X64, B.BLOCK_128X128):
        assert _call_edges(p, b, T.TX_4X4) == ENOTSUP
        assert _call_screen(p, p, b) == ENOTSUP
    # num_modes_rdo 5
    for num in (5, 0, 13):
        assert _call_screen(p, p, B.BLOCK_8X8, num=num) == EINVAL
    # tx_size larger than the partition's plane block
    assert _call_edges(p, B.BLOCK_8X8, T.TX_16X16) == EINVAL
    assert _call_edges(p, B.BLOCK_16X8, T.TX_16X16) == EINVAL
    assert _call_edges(pc, B.BLOCK_16X16, T.TX_16X16) == EINVAL  # 8x8 in a 4:2:0 chroma plane
    assert _call_edges(pc, B.BLOCK_4X4, T.TX_8X8) == EINVAL  # supersampled to 8x8, 4x4 there
    # null outputs / inputs
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, out=None) == EINVAL
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, jobs=None) == EINVAL
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, tiles=None) == EINVAL
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, n_tiles=0) == EINVAL
    assert _call_screen(p, p, B.BLOCK_8X8, modes=None) == EINVAL
    assert _call_screen(p, p, B.BLOCK_8X8, cdf=None) == EINVAL
    assert R.lib().rv_intra_edges_batch(None, 1, 1, 1, 1, 3, 1, 8, -1, 1, None) == EINVAL
    # the rest of the header's list
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, n=-1) == EINVAL
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, bd=9) == EINVAL
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, bd=10) == EINVAL  # a u8 plane
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, mode=14) == EINVAL
    assert _call_edges(_host_plane(0, 1), B.BLOCK_8X8, T.TX_8X8) == EINVAL  # 4:4:0
    assert _call_screen(pc, pc, B.BLOCK_8X8) == EINVAL  # luma only
    assert _call_screen(p, _host_plane(hbd=1), B.BLOCK_8X8) == EINVAL
    assert b"rv_intra_screen_batch" in R.lib().rv_last_error()
    # nothing to do is not an error
    assert _call_edges(p, B.BLOCK_8X8, T.TX_8X8, n=0, out=None, jobs=None, tiles=None) == 0
    assert _call_screen(p, p, B.BLOCK_8X8, n=0, modes=None, jobs=None, tiles=None) == 0
    names = R.exported_symbols_from_header()
    assert "rv_intra_edges_batch" in names and "rv_intra_screen_batch" in names


def test_python_raises_the_reference_preconditions():
    """Checked before anything is allocated on a device."""
    class FakePlane:
        desc = _host_plane()
        dtype = np.uint8
    tiles = np.array([(0, 0, 64, 64)], R.INTRA_TILE)

    def job(**kw):
        j = np.zeros(1, R.INTRA_BLK_JOB)
        for k, v in kw.items():
            j[k] = v
        return j
    for bad in (job(tile=1), job(po_x=60, bo_x=15), job(po_y=-4), job(bo_x=-1)):
        with pytest.raises(R.Rav1eHipError):
            R._intra_blk_args("t", FakePlane, tiles, bad, R.BlockSize.BLOCK_8X8, R.TxSize.TX_8X8, 8)
    with pytest.raises(R.Rav1eHipError):  # the tile leaves the plane's allocation
        R._intra_blk_args("t", FakePlane, np.array([(0, 0, 256, 64)], R.INTRA_TILE), job(),
                          R.BlockSize.BLOCK_8X8, R.TxSize.TX_8X8, 8)
    R._intra_blk_args("t", FakePlane, tiles, job(po_x=56, bo_x=14), R.BlockSize.BLOCK_8X8,
                      R.TxSize.TX_8X8, 8)


# ---------------------------------------------------------------------- GPU
FW, FH = 136, 104
TILES = np.array([(0, 0, 64, FH), (64, 0, 72, FH)], R.INTRA_TILE)  # two tile columns


@functools.lru_cache(None)
def _frame(bd, xdec, ydec, seed):
    """Random pixels with saturated regions, plane size of the format."""
    rng = np.random.default_rng(1000 * seed + 10 * bd + 2 * xdec + ydec)
    w, h = FW >> xdec, FH >> ydec
    maxv = (1 << bd) - 1
    a = rng.integers(0, maxv + 1, (h, w))
    a[h // 4:h // 2, w // 3:w // 2 + 5] = maxv
    a[h // 2:h // 2 + 7, :w // 6] = 0
    a[:, (64 >> xdec) - 2:(64 >> xdec) + 1] = maxv  # across the tile edge
    a = a.astype(np.uint16 if bd > 8 else np.uint8)
    a.setflags(write=False)
    return a


def _regions(a, xdec, ydec):
    return [a[t["y"] >> ydec:(t["y"] + t["height"]) >> ydec,
              t["x"] >> xdec:(t["x"] + t["width"]) >> xdec].astype(np.int64) for t in TILES]


def _edge_jobs(b, xdec, ydec, tw, th):
    """Every transform block of every partition position of both tiles that
    lies inside its tile's region."""
    bw, bh = X.BLK_W[b], X.BLK_H[b]
    pw, ph = max(4, bw >> xdec), max(4, bh >> ydec)
    rows = []
    for ti, t in enumerate(TILES):
        rw, rh = t["width"] >> xdec, t["height"] >> ydec
        for mi_row in range(0, t["height"] // 4, bh // 4):
            for mi_col in range(0, t["width"] // 4, bw // 4):
                # a sub-8x8 block has its chroma at the odd position (has_chroma)
                ox = mi_col | (1 if xdec and bw == 4 else 0)
                oy = mi_row | (1 if ydec and bh == 4 else 0)
                for by in range(ph // th):
                    for bx in range(pw // tw):
                        po_x, po_y = R.intra_plane_offset(ox, oy, xdec, ydec, bx, by,
                                                          X.tx_size_of(tw, th))
                        if po_x + tw <= rw and po_y + th <= rh:
                            rows.append((ti, ox, oy, bx, by, int(po_x), int(po_y), 0))
    return np.array(rows, R.INTRA_BLK_JOB)


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("fmt", X.FORMATS, ids=["444", "422", "420"])
def test_gpu_edges_every_size(fmt, bd):
    R.require_device(0)
    xdec, ydec = fmt
    a = _frame(bd, xdec, ydec, 1)
    plane = R.DevicePlane.from_array(a, xpad=16, ypad=16, xdec=xdec, ydec=ydec, bit_depth=bd)
    regs = _regions(a, xdec, ydec)
    total = 0
    for b in X.SIZES:
        pw, ph = max(4, X.BLK_W[b] >> xdec), max(4, X.BLK_H[b] >> ydec)
        half = (max(4, pw // 2), max(4, ph // 2))
        # opt_mode None and four modes: D45 (top-right), D207 (bottom-left),
        # PAETH (the demotion), UV_CFL_PRED (the DC rule); the half-size
        # transform blocks (bx, by > 0) with None and D45 / D207
        runs = [((pw, ph), m) for m in (None, 3, 7, 12, 13)]
        if half != (pw, ph):
            runs += [(half, m) for m in (None, 3, 7)]
        for (tw, th), mode in runs:
            ts = X.tx_size_of(tw, th)
            jobs = _edge_jobs(b, xdec, ydec, tw, th)
            assert len(jobs)
            got = R.intra_edges_batch(plane, TILES, jobs, b, ts, bd, mode)
            for j, g in zip(jobs, got):
                want = X.get_intra_edges(regs[j["tile"]], j["bo_x"], j["bo_y"], j["bx"], j["by"],
                                         b, j["po_x"], j["po_y"], ts, xdec, ydec, bd,
                                         -1 if mode is None else mode)
                assert (g == want).all(), (b, tw, th, mode, j)
            total += len(jobs)
    assert total > 5000
    assert (plane.download_visible() == a).all()


def _screen_jobs(b, rng, cdf_len_default, limit=301):
    bw, bh = X.BLK_W[b], X.BLK_H[b]
    rows = []
    for ti, t in enumerate(TILES):
        for mi_row in range(0, (t["height"] - bh) // 4 + 1, bh // 4):
            for mi_col in range(0, (t["width"] - bw) // 4 + 1, bw // 4):
                rows.append((ti, mi_col, mi_row, 0, 0, 4 * mi_col, 4 * mi_row, 0))
    if len(rows) > limit:  # corners kept, the rest sampled; 301 is odd: a partial last wave
        keep = sorted(set([0, len(rows) - 1]) | set(
            int(v) for v in rng.choice(len(rows), limit - 2, replace=False)))[:limit]
        rows = [rows[i] for i in keep]
    jobs = np.array(rows, R.INTRA_BLK_JOB)
    # a row per job: key-frame rows by random neighbour modes, the size's
    # y_mode row, and the same rows of an adapted copy of the table
    for k in range(len(jobs)):
        kind = k % 4
        off = R.intra_mode_cdf_offset(R.FRAME_TYPE_KEY, b, int(rng.integers(13)),
                                      int(rng.integers(13))) if kind & 1 else \
            R.intra_mode_cdf_offset(R.FRAME_TYPE_INTER, b)
        jobs["cdf_off"][k] = off + (cdf_len_default if kind & 2 else 0)
    return jobs


@functools.lru_cache(None)
def _cdf_tables():
    """The default combined table followed by an adapted copy: every intra
    mode row replaced by a valid perturbed one."""
    d = _default_cdf()
    rng = np.random.default_rng(77)
    a = d.copy()
    for off in [R.ECM_KF_Y + 14 * i for i in range(25)] + [R.ECM_Y_MODE + 14 * i for i in range(4)]:
        p = rng.integers(1, 2400, 13)  # the 13 probabilities: positive, sum < 32768
        if off % 3 == 0:  # some of them equal
            p[3] = p[7] = p[1]
        a[off:off + 13] = 32768 - np.cumsum(p)
    t = np.concatenate([d, a])
    t.setflags(write=False)
    return t


@functools.lru_cache(None)
def _screen_reference(b, bd):
    """(jobs, edges, satds) of the size's jobs, computed once."""
    rec, src = _frame(bd, 0, 0, 2), _frame(bd, 0, 0, 3)
    rr, sr = _regions(rec, 0, 0), _regions(src, 0, 0)
    jobs = _screen_jobs(b, np.random.default_rng(100 + b), len(_default_cdf()))
    edges, satds = [], []
    for j in jobs:
        e, s, _ = X.screen(rr[j["tile"]], sr[j["tile"]], int(j["bo_x"]), int(j["bo_y"]), b, bd,
                           _default_cdf()[:14], 3)
        edges.append(e)
        satds.append(s)
    return jobs, np.array(edges), np.array(satds)


# every size at 8 and 10 bit; at 12 bit one size per work split
SCREEN_CASES = [(b, bd) for bd in (8, 10) for b in X.SIZES] + [(b, 12) for b in (0, 2, 3, 6, 9, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("b,bd", SCREEN_CASES,
                         ids=["%dx%d-%d" % (X.BLK_W[b], X.BLK_H[b], bd) for b, bd in SCREEN_CASES])
def test_gpu_screening_every_size(b, bd):
    R.require_device(0)
    rec_a, src_a = _frame(bd, 0, 0, 2), _frame(bd, 0, 0, 3)
    rec = R.DevicePlane.from_array(rec_a, xpad=16, ypad=16, bit_depth=bd)
    src = R.DevicePlane.from_array(src_a, xpad=16, ypad=16, bit_depth=bd)
    cdf = _cdf_tables()
    jobs, edges, satds = _screen_reference(b, bd)
    # jobs per workgroup (and per wavefront): 64 / the number of Hadamard
    # chunks (rv_intra_screen.hip)
    nh = min(X.BLK_W[b], X.BLK_H[b], 8)
    packing = 64 // ((X.BLK_W[b] // nh) * (X.BLK_H[b] // nh))
    for num in (3, 7):
        # all jobs; 0; 1; a count that is no multiple of the jobs per workgroup
        for n in (len(jobs), 0, 1, min(len(jobs), packing + 3)):
            got_m, got_s, got_e = R.intra_mode_screen_batch(rec, src, TILES, jobs[:n], b, cdf, num,
                                                            bd, with_satd=True, with_edges=True)
            assert len(got_m) == n and got_s.shape == (n, 13) and got_e.shape == (n, 257)
            assert (got_e == edges[:n]).all()
            assert (got_s == satds[:n]).all()
            for k in range(n):
                row = cdf[jobs["cdf_off"][k]:][:14]
                assert got_m[k] == X.select(satds[k], row, num), (b, bd, num, k)
    # the reconstruction is left untouched
    assert (rec.download_visible() == rec_a).all()
    assert (src.download_visible() == src_a).all()


@pytest.mark.gpu
def test_gpu_modes_without_optional_outputs():
    R.require_device(0)
    b, bd = 3, 8
    rec = R.DevicePlane.from_array(_frame(bd, 0, 0, 2), xpad=16, ypad=16, bit_depth=bd)
    src = R.DevicePlane.from_array(_frame(bd, 0, 0, 3), xpad=16, ypad=16, bit_depth=bd)
    cdf = _cdf_tables()
    jobs, _, satds = _screen_reference(b, bd)
    got = R.intra_mode_screen_batch(rec, src, TILES, jobs, b, R.DeviceBuffer.from_array(cdf), 7, bd)
    assert got == [X.select(satds[k], cdf[jobs["cdf_off"][k]:][:14], 7) for k in range(len(jobs))]


@pytest.mark.gpu
@pytest.mark.parametrize("b", [3, 5, 9], ids=["8x8", "16x8", "32x32"])
def test_gpu_fused_equals_composed_operators(b):
    """intra_edges_batch -> 13 x predict_intra_batch -> 13 x satd_batch ->
    the host selection gives what the fused launch gives."""
    R.require_device(0)
    bd = 8
    w, h = X.BLK_W[b], X.BLK_H[b]
    ts = X.tx_size_of(w, h)
    rec = R.DevicePlane.from_array(_frame(bd, 0, 0, 2), xpad=16, ypad=16, bit_depth=bd)
    src = R.DevicePlane.from_array(_frame(bd, 0, 0, 3), xpad=16, ypad=16, bit_depth=bd)
    cdf = _cdf_tables()
    jobs = _screen_reference(b, bd)[0]
    n = len(jobs)
    fm, fs, fe = R.intra_mode_screen_batch(rec, src, TILES, jobs, b, cdf, 7, bd, with_satd=True,
                                           with_edges=True)
    edges = R.intra_edges_batch(rec, TILES, jobs, b, ts, bd, None)
    assert (edges == fe).all()
    # predictions side by side in a scratch plane, one block per job
    per_row = 16
    scratch = R.DevicePlane(per_row * w, ((n + per_row - 1) // per_row) * h, bit_depth=bd)
    sx, sy = (np.arange(n) % per_row) * w, (np.arange(n) // per_row) * h
    px = TILES["x"][jobs["tile"]] + jobs["po_x"]
    py = TILES["y"][jobs["tile"]] + jobs["po_y"]
    var = np.array([X.variant_of(int(x), int(y)) for x, y in zip(jobs["po_x"], jobs["po_y"])])
    satd = np.zeros((n, 13), np.uint32)
    for k, m in enumerate(R.RAV1E_INTRA_MODES):
        ij = np.zeros(n, R.INTRA_JOB)
        ij["x"], ij["y"], ij["mode"], ij["variant"] = sx, sy, m, var
        R.predict_intra_batch(scratch, ij, edges, ts, bd)
        dj = np.zeros(n, R.DIST_JOB)
        dj["org_x"], dj["org_y"], dj["ref_x"], dj["ref_y"] = px, py, sx, sy
        satd[:, k] = R.satd_batch(src, scratch, dj, w, h)
    assert (satd == fs).all()
    for k in range(n):
        assert fm[k] == R.intra_screen_select(satd[k], cdf[jobs["cdf_off"][k]:][:14], 7)

"""Chroma from luma: luma_ac_batch, predict_cfl_batch, cfl_alpha_search_batch
and the CFLParams helpers against tests/cfl_ref.py (a numpy restatement of
src/encoder.rs:1714-1755, src/predict.rs:836-892 and src/rdo.rs:1261-1336
over the C oracle's DC_PRED), which itself is pinned to the vectors the
reference's own text produced (tests/golden/ref_cfl.npz, written by
tools/refeval/gen_cfl_ref.py).  CPU tests first, GPU tests (bit for bit)
after."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rav1e_amd as R
from tests import cfl_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_cfl.npz")
PAD = 16  # padding of the search planes (the neighbours of a block at 0)


# ---------------------------------------------------------------- restatement
@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def test_restatement_predict_cfl_equals_reference_vectors():
    g = golden()
    meta, off = g["pred_meta"], g["pred_off"]
    assert len(meta) >= 30
    for k, (tx, variant, alpha, bd) in enumerate(meta):
        w, h = R.TxSize(int(tx)).width(), R.TxSize(int(tx)).height()
        ac = g["pred_ac"][off[k]:off[k + 1]].reshape(h, w)
        want = g["pred_out"][off[k]:off[k + 1]].reshape(h, w)
        got = CR.predict_cfl(int(variant), w, h, g["pred_edge"][k], ac, int(alpha), int(bd))
        assert (got == want).all(), (k, tx, variant, alpha, bd)


def test_restatement_luma_ac_equals_reference_vectors():
    g = golden()
    meta, off = g["ac_meta"], g["ac_off"]
    assert len(meta) >= 30
    for k, (bsize, xdec, ydec, bd, x, y) in enumerate(meta):
        full = g["ac_luma_bd%d" % bd]
        yo, xo = g["ac_origin"]
        w, h = CR.subsampled_size(int(bsize), int(xdec), int(ydec))
        got = CR.luma_ac(full, int(yo), int(xo), int(x), int(y), int(bsize), int(xdec), int(ydec))
        assert (got.reshape(-1) == g["ac_out"][off[k]:off[k + 1]]).all(), tuple(meta[k])
        assert got.shape == (h, w)


def test_restatement_rdo_cfl_alpha_equals_reference_vectors():
    g = golden()
    if "rdo_meta" not in g:
        pytest.fail("ref_cfl.npz holds no rdo_cfl_alpha vectors")
    meta = g["rdo_meta"]
    assert len(meta) >= 12
    yo, xo = (int(v) for v in g["rdo_origin"])
    stops, variants = [], set()
    for k, (cfg, bsize, xdec, ydec, bd, x, y) in enumerate(meta):
        rec = [(g["rdo_rec%d_p%d" % (cfg, p)], yo, xo, xdec if p else 0, ydec if p else 0)
               for p in range(3)]
        src = [(g["rdo_src%d_p%d" % (cfg, p)], yo, xo, xdec if p else 0, ydec if p else 0)
               for p in range(3)]
        cx, cy = CR.chroma_pos(int(x), int(y), int(xdec), int(ydec))
        variant = (1 if cx else 0) | (2 if cy else 0)  # PredictionVariant::new of a tile at 0
        got = CR.rdo_cfl_alpha(rec, src, int(x), int(y), variant, int(bsize), int(bd))
        assert [got[0][0], got[1][0]] == list(g["rdo_alpha"][k]), tuple(meta[k])
        stops += [got[0][2], got[1][2]]
        variants.add(variant)
    # the vectors hold scans that break early and scans that run to 16
    assert min(stops) < 16 and max(stops) == 16 and variants == {0, 1, 2, 3}


def break_case_luma(w, h, xdec, ydec, dtype):
    """A luma block whose ac is +d at chroma (0, 0), -d at (h - 1, w - 1) and
    0 elsewhere, d = 1 << (3 - xdec - ydec)."""
    blk = np.full((h << ydec, w << xdec), 100, dtype)
    blk[0, 0] = 101
    blk[(h - 1) << ydec, (w - 1) << xdec] = 99
    return blk


def test_scan_break_case():
    """4:2:0, 8 bit, BLOCK_8X8: ac +2 at (0, 0), -2 at (3, 3); DC 60; source
    60 + sign(ac).  The prediction reaches the source only at alpha 16, but
    the scan gives up after a = 3 and returns 0."""
    luma = np.zeros((16, 16), np.uint8)
    luma[:8, :8] = break_case_luma(4, 4, 1, 1, np.uint8)
    assert luma[0, 0] == 101 and luma[6, 6] == 99
    ac = CR.luma_ac(luma, 0, 0, 0, 0, R.BlockSize.BLOCK_8X8, 1, 1)
    want_ac = np.zeros((4, 4), np.int16)
    want_ac[0, 0], want_ac[3, 3] = 2, -2
    assert (ac == want_ac).all()
    dc = np.full((4, 4), 60, np.uint8)
    src = (60 + np.sign(ac)).astype(np.uint8)
    costs = CR.alpha_costs(src, dc, ac, 8)
    assert costs[1:32] == [2] * 31 and costs[32] == 0
    alpha, cost, stop = CR.alpha_scan(costs)
    assert (alpha, cost, stop) == (0, 2, 3)
    assert int(np.argmin(costs)) - 16 == 16


# ---------------------------------------------------------------- validation
class FakePlane:
    """A plane descriptor without device memory: enough for the checks that
    come before any launch."""

    def __init__(self, w, h, xdec=0, ydec=0, hbd=0, pad=16):
        self.desc = R.RvPlane()
        R.lib().rv_plane_geometry(C.byref(self.desc), w, h, xdec, ydec, pad, pad, hbd)


def fake_planes(xdec, ydec, hbd=0):
    return [FakePlane(128, 96), FakePlane(128 >> xdec, 96 >> ydec, xdec, ydec, hbd),
            FakePlane(128 >> xdec, 96 >> ydec, xdec, ydec, hbd)]


def test_python_validation_rejects_without_launch():
    p420, p422 = fake_planes(1, 1), fake_planes(1, 0)
    job = np.array([(8, 8, 3, 0)], R.CFL_JOB)
    odd = np.array([(12, 12, 3, 0)], R.CFL_JOB)
    B = R.BlockSize
    with pytest.raises(R.Rav1eHipError, match="cfl_allowed"):
        R.cfl_alpha_search_batch(p420, p420, job, B.BLOCK_64X64)
    with pytest.raises(R.Rav1eHipError, match="cfl_allowed"):
        R.luma_ac_batch(p420[0], job, B.BLOCK_4X16, 1, 1)
    with pytest.raises(R.Rav1eHipError, match="no subsampled size"):
        R.cfl_alpha_search_batch(p422, p422, job, B.BLOCK_8X16)
    with pytest.raises(R.Rav1eHipError, match="no subsampled size"):
        R.luma_ac_batch(p422[0], job, B.BLOCK_8X16, 1, 0)
    # an even-position BLOCK_4X4 at 4:2:0 carries no chroma
    with pytest.raises(R.Rav1eHipError, match="has_chroma"):
        R.cfl_alpha_search_batch(p420, p420, job, B.BLOCK_4X4)
    with pytest.raises(R.Rav1eHipError, match="has_chroma"):
        R.luma_ac_batch(p420[0], job, B.BLOCK_4X4, 1, 1)
    # ... and the odd one would pass that check: it fails later, on its position
    far = np.array([((1 << 20) + 4, 12, 3, 0)], R.CFL_JOB)
    with pytest.raises(R.Rav1eHipError, match="leave"):
        R.luma_ac_batch(p420[0], far, B.BLOCK_4X4, 1, 1)
    assert R.has_chroma(odd["x"], odd["y"], B.BLOCK_4X4, 1, 1).all()
    with pytest.raises(R.Rav1eHipError, match="variant"):
        R.cfl_alpha_search_batch(p420, p420, np.array([(8, 8, 4, 0)], R.CFL_JOB), B.BLOCK_8X8)

    dst = FakePlane(64, 64)
    ij = np.array([(0, 0, 13, 3)], R.INTRA_JOB)
    e, a = np.zeros((1, 257), np.uint8), np.zeros((1, 8, 8), np.int16)
    with pytest.raises(R.Rav1eHipError, match="64-point"):
        R.predict_cfl_batch(dst, ij, e, np.zeros((1, 64, 64), np.int16), [1], R.TxSize.TX_64X64)
    with pytest.raises(R.Rav1eHipError, match="64-point"):
        R.predict_cfl_batch(dst, ij, e, np.zeros((1, 64, 16), np.int16), [1], R.TxSize.TX_16X64)
    with pytest.raises(R.Rav1eHipError, match="edges"):
        R.predict_cfl_batch(dst, ij, e[:, :256], a, [1], R.TxSize.TX_8X8)
    with pytest.raises(R.Rav1eHipError, match="ac must"):
        R.predict_cfl_batch(dst, ij, e, a.reshape(1, 4, 16), [1], R.TxSize.TX_8X8)
    with pytest.raises(R.Rav1eHipError, match="ac must"):
        R.predict_cfl_batch(dst, ij, e, a.astype(np.int32), [1], R.TxSize.TX_8X8)
    with pytest.raises(R.Rav1eHipError, match="alpha"):
        R.predict_cfl_batch(dst, ij, e, a, [17], R.TxSize.TX_8X8)
    with pytest.raises(R.Rav1eHipError, match="UV_CFL_PRED"):
        R.predict_cfl_batch(dst, np.array([(0, 0, 0, 3)], R.INTRA_JOB), e, a, [1], R.TxSize.TX_8X8)
    # predict_intra_batch keeps refusing CfL
    with pytest.raises(R.Rav1eHipError, match="CfL"):
        R.predict_intra_batch(dst, ij, e, R.TxSize.TX_8X8)


def test_c_abi_validation_rejects_without_launch():
    """n = 0 tells a rejected call from an accepted one with no launch either
    way: the argument checks come before the n == 0 return."""
    L = R.lib()
    p420, p422, p444 = (fake_planes(1, 1), fake_planes(1, 0), fake_planes(0, 0))
    for pl in (p420, p422, p444):
        for p in pl:
            p.desc.data = 4096  # never dereferenced: n = 0
    arr = lambda pl: (R.RvPlane * 3)(*(p.desc for p in pl))
    search = lambda pl, bsize, bd=8: L.rv_cfl_alpha_search_batch(arr(pl), arr(pl), None, 0, bsize,
                                                                  bd, None, None, None)
    B = R.BlockSize
    assert search(p420, B.BLOCK_32X32) == R.RV_OK
    assert search(p420, B.BLOCK_64X64) == R.RV_EINVAL
    assert search(p420, B.BLOCK_4X16) == R.RV_EINVAL
    assert search(p422, B.BLOCK_8X16) == R.RV_EINVAL
    assert search(p422, B.BLOCK_16X16) == R.RV_OK
    assert search(p444, B.BLOCK_8X16) == R.RV_OK
    assert search(p420, B.BLOCK_8X8, 10) == R.RV_EINVAL  # u8 planes at 10 bit
    p420[0].desc.stride += 2  # pixel runs are loaded as aligned vectors
    assert search(p420, B.BLOCK_32X32) == R.RV_EINVAL
    p420[0].desc.stride -= 2
    ac = lambda bsize, xd, yd: L.rv_cfl_luma_ac_batch(C.byref(p420[0].desc), None, 0, bsize, xd, yd,
                                                      None, None)
    assert ac(B.BLOCK_8X8, 1, 1) == R.RV_OK
    assert ac(B.BLOCK_32X64, 1, 1) == R.RV_EINVAL
    assert ac(B.BLOCK_16X32, 1, 0) == R.RV_EINVAL
    assert ac(B.BLOCK_8X8, 0, 1) == R.RV_EINVAL  # 4:4:0 is no subsampling of the reference
    pred = lambda tx: L.rv_predict_cfl_batch(C.byref(p420[0].desc), None, None, None, None, 0, tx,
                                             8, None)
    for tx in R.TxSize:
        want = R.RV_ENOTSUP if max(tx.width(), tx.height()) == 64 else R.RV_OK
        assert pred(int(tx)) == want, tx
    assert sum(pred(int(tx)) == R.RV_OK for tx in R.TxSize) == 14
    assert pred(19) == R.RV_EINVAL


def test_cfl_params_helpers():
    """CFLParams (src/context.rs:1866-1915) for every alpha pair but (0, 0)."""
    seen = set()
    for u in range(-16, 17):
        for v in range(-16, 17):
            if (u, v) == (0, 0):
                continue
            p = R.CFLParams.from_alpha(u, v)
            assert (p.alpha(0), p.alpha(1)) == (u, v)
            js = p.joint_sign()
            assert 0 <= js <= 7
            seen.add(js)
            for uv, a in ((0, u), (1, v)):
                if a != 0:
                    assert 0 <= p.index(uv) <= 15 and p.index(uv) == abs(a) - 1
                    assert 0 <= p.context(uv) <= 5
    assert seen == set(range(8))
    d = R.CFLParams()  # Default: sign (NEG, ZERO), scale (1, 0)
    assert (d.alpha(0), d.alpha(1)) == (-1, 0)
    assert R.PredictionMode.UV_CFL_PRED == 13


def test_kernels_use_no_scratch(tmp_path):
    """Every kernel of rv_cfl.hip keeps its arrays in registers: the compiler
    reports 0 bytes of scratch per lane."""
    mk = open(os.path.join(ROOT, "rav1e_amd", "csrc", "Makefile")).read()
    hipcc = re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1)
    hipcc = os.environ.get("HIPCC", hipcc)
    if shutil.which(hipcc) is None:
        pytest.skip("hipcc absent")
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= ((?:.*\\\n)*.*)$", mk, re.M).group(1)
    flags = flags.replace("\\\n", " ").replace("$(ARCH)", arch).split()
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "rv_cfl.hip",
                                          "-o", str(tmp_path / "rv_cfl.o")],
                       cwd=os.path.join(ROOT, "rav1e_amd", "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(names) == len(scratch) >= 3
    assert any("cfl_search_kernel" in n for n in names)
    assert any("cfl_luma_ac_kernel" in n for n in names) and any("cfl_pred_kernel" in n for n in names)
    spilled = [(n, s) for n, s in zip(names, scratch) if s != "0"]
    assert not spilled, spilled


# ---------------------------------------------------------------- the search grid
def _need_odd(bsize, xdec, ydec):
    bw, bh = CR.BLOCK_WH[bsize]
    return (xdec != 0 and bw == 4), (ydec != 0 and bh == 4)


@functools.lru_cache(maxsize=None)
def search_cell(bsize, xdec, ydec, bd):
    """One cell of the alpha-search grid: 64 jobs on an 8 x 8 lattice, their
    planes (whole padded arrays, PAD pixels of replicated border) and the
    restatement's answers.  Job 9 is the break case, job 10 a flat-luma job;
    the source chroma of every other job is clip(dc + scaled(a*, ac) + noise)
    with a* uniform in -20 .. 20 and noise in -3 .. 3."""
    rng = np.random.default_rng([bsize, xdec, ydec, bd])
    dtype = np.uint16 if bd > 8 else np.uint8
    maxv = (1 << bd) - 1
    bw, bh = CR.BLOCK_WH[bsize]
    w, h = CR.subsampled_size(bsize, xdec, ydec)
    px, py = max(bw, 8), max(bh, 8)
    ox, oy = _need_odd(bsize, xdec, ydec)
    LW, LH = 8 * px, 8 * py
    vis = [rng.integers(0, maxv + 1, (LH, LW)).astype(dtype),
           rng.integers(0, maxv + 1, (LH >> ydec, LW >> xdec)).astype(dtype),
           rng.integers(0, maxv + 1, (LH >> ydec, LW >> xdec)).astype(dtype)]
    jobs = np.zeros(64, R.CFL_JOB)
    for k in range(64):
        jobs[k] = ((k % 8) * px + (4 if ox else 0), (k // 8) * py + (4 if oy else 0),
                   int(rng.integers(0, 4)), 0)
    for k in (9, 10):  # the two special jobs
        x, y = int(jobs[k]["x"]), int(jobs[k]["y"])
        lx, ly = CR.luma_origin(x, y, bsize, xdec, ydec)
        blk = break_case_luma(w, h, xdec, ydec, dtype) if k == 9 else \
            np.full((h << ydec, w << xdec), 77, dtype)
        vis[0][ly:ly + (h << ydec), lx:lx + (w << xdec)] = blk
        if k == 9:
            jobs[k]["variant"] = 3
            cx, cy = CR.chroma_pos(x, y, xdec, ydec)
            for p in (1, 2):  # DC 60
                vis[p][cy - 1, cx:cx + w] = 60
                vis[p][cy:cy + h, cx - 1] = 60
    rec = [(np.pad(v, PAD, mode="edge"), PAD, PAD, xdec if p else 0, ydec if p else 0)
           for p, v in enumerate(vis)]
    srcv = [vis[0].copy(), np.zeros_like(vis[1]), np.zeros_like(vis[2])]
    astar = rng.integers(-20, 21, (64, 2))
    for k in range(64):
        x, y, variant = int(jobs[k]["x"]), int(jobs[k]["y"]), int(jobs[k]["variant"])
        ac = CR.luma_ac(rec[0][0], PAD, PAD, x, y, bsize, xdec, ydec)
        cx, cy = CR.chroma_pos(x, y, xdec, ydec)
        for p in (1, 2):
            edge = CR.cfl_edges(rec[p][0], PAD, PAD, cx, cy, w, h, variant)
            dc = int(CR.O.predict_intra(0, variant, w, h, edge, bd)[0, 0])
            if k == 9:
                assert dc == 60
                s = dc + np.sign(ac)
            elif k == 10:
                s = dc + rng.integers(-3, 4, (h, w))
            else:
                s = dc + CR.scaled_luma_q0(int(astar[k, p - 1]), ac) + rng.integers(-3, 4, (h, w))
            srcv[p][cy:cy + h, cx:cx + w] = np.clip(s, 0, maxv)
    src = [(np.pad(v, PAD, mode="edge"), PAD, PAD, xdec if p else 0, ydec if p else 0)
           for p, v in enumerate(srcv)]
    alpha = np.zeros((64, 2), np.int16)
    cost = np.zeros((64, 2), np.uint64)
    stop = np.zeros((64, 2), np.int32)
    argmin = np.zeros((64, 2), np.int32)
    for k in range(64):
        res = CR.rdo_cfl_alpha(rec, src, int(jobs[k]["x"]), int(jobs[k]["y"]),
                               int(jobs[k]["variant"]), bsize, bd)
        for p in range(2):
            alpha[k, p], cost[k, p], stop[k, p] = res[p][:3]
            argmin[k, p] = int(np.argmin(res[p][3])) - 16
    return dict(rec=rec, src=src, jobs=jobs, alpha=alpha, cost=cost, stop=stop, argmin=argmin,
                dims=(LW, LH))


def test_search_grid_is_honest():
    """What keeps the search test from passing for the wrong reason, asserted
    on the restatement's answers (fractions are over the 128 scans of a cell:
    64 jobs, two chroma planes)."""
    wanted = set()
    for bd in (8, 10, 12):
        for bsize, xdec, ydec in CR.allowed_cells():
            c = search_cell(bsize, xdec, ydec, bd)
            wanted |= set(int(a) for a in c["alpha"].reshape(-1))
            early = float((c["stop"] < 16).mean())
            assert early >= 0.10, (bsize, xdec, ydec, bd, early)
            assert 1 - early >= 0.10, (bsize, xdec, ydec, bd, early)
            zeros = float((c["alpha"] == 0).all(axis=1).mean())
            assert zeros <= 0.10, (bsize, xdec, ydec, bd, zeros)
            # the break case: the scan stops after a = 3 at alpha 0, short of the minimum
            assert list(c["alpha"][9]) == [0, 0] and list(c["stop"][9]) == [3, 3]
            assert (c["argmin"][9] > 0).all() and (c["cost"][9] == 2).all()
            # flat luma: ac == 0, every cost ties
            assert list(c["alpha"][10]) == [0, 0]
    assert wanted == set(range(-16, 17))


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def device():
    R.require_device(0)


def device_plane(full, yo, xo, xdec, ydec, bd):
    """Upload a whole padded array as a plane of the given decimation."""
    h, w = full.shape[0] - 2 * yo, full.shape[1] - 2 * xo
    p = R.DevicePlane.from_full(np.ascontiguousarray(full), xo, yo, w, h, bit_depth=bd)
    p.desc.xdec, p.desc.ydec = xdec, ydec
    return p


def ac_jobs(bsize, xdec, ydec):
    """Positions in a 128 x 96 luma plane with 32 pixels of padding: a few
    inside (odd block offsets where a sub-8x8 block needs them), the
    all-maximum block at (32, 32), one block over the right padding and one
    over the bottom padding."""
    bw, bh = CR.BLOCK_WH[bsize]
    ox, oy = _need_odd(bsize, xdec, ydec)
    dx, dy = (4 if ox else 0), (4 if oy else 0)
    pos = [(0 + dx, 0 + dy), (32 + dx, 32 + dy), (64 + dx, 8 + dy), (96 + dx, 64 + dy),
           (40 + dx, 56 + dy), (8 + dx, 64 + dy)]
    right = (124, 16 + dy) if bw > 4 else (128 + dx, 16 + dy)
    bottom = (16 + dx, 92) if bh > 4 else (16 + dx, 96 + dy)
    jobs = np.zeros(len(pos) + 2, R.CFL_JOB)
    for k, (x, y) in enumerate(pos + [right, bottom]):
        jobs[k] = (x, y, 0, 0)
        assert CR.has_chroma(x, y, bsize, xdec, ydec)
    return jobs


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_luma_ac_batch(device, bd):
    rng = np.random.default_rng(bd)
    maxv = (1 << bd) - 1
    img = rng.integers(0, maxv + 1, (96, 128)).astype(np.uint16 if bd > 8 else np.uint8)
    img[32:64, 32:64] = maxv  # an all-maximum block: ac == 0
    img[60:, 100:] = rng.integers(maxv - 3, maxv + 1, (36, 28))  # a bright border to replicate
    luma = R.DevicePlane.from_array(img, xpad=32, ypad=32, bit_depth=bd)
    full = luma.download_full()  # with the padding rv_plane_pad wrote
    yo, xo = luma.desc.yorigin, luma.desc.xorigin
    for bsize, xdec, ydec in CR.allowed_cells():
        jobs = ac_jobs(bsize, xdec, ydec)
        got = R.luma_ac_batch(luma, jobs, bsize, xdec, ydec)
        w, h = CR.subsampled_size(bsize, xdec, ydec)
        assert got.shape == (len(jobs), h, w) and got.dtype == np.int16
        for k, j in enumerate(jobs):
            want = CR.luma_ac(full, yo, xo, int(j["x"]), int(j["y"]), bsize, xdec, ydec)
            assert (got[k] == want).all(), (bsize, xdec, ydec, k)
        assert not got[1].any()
        assert got[0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_predict_cfl_batch(device, bd):
    """All 14 sizes x 4 variants x alpha in {-16, -1, 0, 1, 7, 16} x three
    kinds of edge buffer (random, saturated, zero), so both clamps fire."""
    rng = np.random.default_rng(100 + bd)
    dtype = np.uint16 if bd > 8 else np.uint8
    maxv = (1 << bd) - 1
    amax = min(32767, maxv << 3)  # luma_ac's range at this depth
    dst = R.DevicePlane(9 * 32, 8 * 32, hbd=bd > 8, bit_depth=bd)
    sizes = [tx for tx in R.TxSize if max(tx.width(), tx.height()) <= 32]
    assert len(sizes) == 14
    lo_clamp = hi_clamp = False
    for tx in sizes:
        w, h = tx.width(), tx.height()
        combos = [(v, a, e) for v in range(4) for a in (-16, -1, 0, 1, 7, 16) for e in range(3)]
        n = len(combos)
        jobs = np.zeros(n, R.INTRA_JOB)
        edges = np.zeros((n, 257), dtype)
        alpha = np.zeros(n, np.int16)
        ac = rng.integers(-amax, amax + 1, (n, h, w)).astype(np.int16)
        ac[:, 0, 0] = np.where(rng.integers(0, 2, n) == 1, amax, -amax)
        for k, (v, a, e) in enumerate(combos):
            jobs[k] = ((k % 9) * 32, (k // 9) * 32, R.PredictionMode.UV_CFL_PRED, v)
            alpha[k] = a
            edges[k] = rng.integers(0, maxv + 1, 257) if e == 0 else (maxv if e == 1 else 0)
        R.predict_cfl_batch(dst, jobs, edges, ac, alpha, tx, bd)
        out = dst.download_visible()
        for k, (v, a, e) in enumerate(combos):
            want = CR.predict_cfl(v, w, h, edges[k], ac[k], a, bd)
            x, y = int(jobs[k]["x"]), int(jobs[k]["y"])
            assert (out[y:y + h, x:x + w] == want).all(), (tx, v, a, e)
            if a != 0:
                lo_clamp |= bool((want == 0).any())
                hi_clamp |= bool((want == maxv).any())
    assert lo_clamp and hi_clamp


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("xdec,ydec", CR.SUBSAMPLINGS)
def test_cfl_alpha_search_batch(device, xdec, ydec, bd):
    for bsize, xd, yd in CR.allowed_cells():
        if (xd, yd) != (xdec, ydec):
            continue
        c = search_cell(bsize, xdec, ydec, bd)
        rec = [device_plane(*pl, bd) for pl in c["rec"]]
        src = [device_plane(*pl, bd) for pl in c["src"]]
        before = [p.download_full() for p in rec]
        alpha, cost = R.cfl_alpha_search_batch(rec, src, c["jobs"], bsize, bd, with_cost=True)
        assert (alpha == c["alpha"]).all(), (bsize, np.argwhere(alpha != c["alpha"])[:4])
        assert (cost == c["cost"]).all(), (bsize, np.argwhere(cost != c["cost"])[:4])
        assert (R.cfl_alpha_search_batch(rec, src, c["jobs"][:5], bsize, bd) == c["alpha"][:5]).all()
        for p in range(3):  # rec is left untouched
            assert (rec[p].download_full() == before[p]).all()

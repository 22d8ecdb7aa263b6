"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and
the reference's own known answers, bit for bit.

Marked `gpu`: runs on a real MI355X (gpurun).  Sources of truth:
  - SAD/SATD: the 88 KATs of src/dist.rs:379-460 on the reference fixture;
  - transforms: tests/golden/tx2d_golden.npz (vectors from the reference's
    own transform source) plus the oracle on random residuals;
  - MC, SSE, cdef moments, full search, pad, downsample: the oracle
    (oracle/, a restatement of the cited reference functions) on seeded
    random planes, including edge cases (max values, 10/12-bit, u8
    overshoot, ties in the motion search).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import rav1e_amd as R
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BLOCKS = [O.block_wh(b) for b in O.BLOCKS]


@pytest.fixture(scope="module", autouse=True)
def hip():
    R.require_device(0)


def rand_plane(rng, h, w, bd):
    dt = np.uint8 if bd == 8 else np.uint16
    return rng.integers(0, 1 << bd, (h, w)).astype(dt)


def blk(a, y, x, h, w):
    return np.ascontiguousarray(a[y:y + h, x:x + w])


def full_of(a, pad):
    """Host copy of a padded plane the way DevicePlane.from_array lays it out."""
    p = R.DevicePlane.from_array(a, xpad=pad, ypad=pad)
    return p, p.download_full()


# ---- SAD / SATD -----------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_sad_satd_reference_kats(dtype):
    with open(os.path.join(GOLD, "dist_kat.json")) as f:
        kat = json.load(f)
    (inp, ix, iy), (rec, rx, ry) = O.dist_kat_planes(dtype)
    pi = R.DevicePlane.from_full(inp, ix, iy, 640, 480)
    pr = R.DevicePlane.from_full(rec, rx, ry, 640, 480)
    for i, name in enumerate(kat["blocks"]):
        w, h = O.block_wh(name)
        job = np.array([(32, 40, 32, 40)], dtype=R.DIST_JOB)
        assert int(R.sad_batch(pi, pr, job, w, h)[0]) == kat["sad"][i], name
        assert int(R.satd_batch(pi, pr, job, w, h)[0]) == kat["satd"][i], name


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_sad_satd_random_vs_oracle(bd):
    rng = np.random.default_rng(100 + bd)
    a = rand_plane(rng, 300, 320, bd)
    b = rand_plane(rng, 300, 320, bd)
    pa, fa = full_of(a, 16)
    pb, fb = full_of(b, 16)
    xo, yo = pa.desc.xorigin, pa.desc.yorigin
    for w, h in BLOCKS:
        n = 23
        jobs = np.zeros(n, dtype=R.DIST_JOB)
        jobs["org_x"] = rng.integers(-8, 320 - w + 8, n)
        jobs["org_y"] = rng.integers(-8, 300 - h + 8, n)
        jobs["ref_x"] = rng.integers(-8, 320 - w + 8, n)
        jobs["ref_y"] = rng.integers(-8, 300 - h + 8, n)
        sad = R.sad_batch(pa, pb, jobs, w, h)
        satd = R.satd_batch(pa, pb, jobs, w, h)
        for k, j in enumerate(jobs):
            args = (fa, yo + j["org_y"], xo + j["org_x"], fb, yo + j["ref_y"], xo + j["ref_x"], w, h)
            assert sad[k] == O.get_sad(*args), (w, h, k)
            assert satd[k] == O.get_satd(*args), (w, h, k)


def test_satd_max_residual_10bit():
    """|diff| = 1023 everywhere: the 8x8 Hadamard hits 65472 (> i16), which
    the generated kernels wrap; the declared ground truth does not."""
    a = np.full((64, 64), 1023, np.uint16)
    b = np.zeros((64, 64), np.uint16)
    pa, pb = R.DevicePlane.from_array(a), R.DevicePlane.from_array(b)
    job = np.array([(0, 0, 0, 0)], dtype=R.DIST_JOB)
    for w, h in [(8, 8), (64, 64), (4, 4), (16, 4)]:
        got = int(R.satd_batch(pa, pb, job, w, h)[0])
        assert got == O.get_satd(a, 0, 0, b, 0, 0, w, h, 0)
        assert got != O.get_satd(a, 0, 0, b, 0, 0, w, h, 1) or min(w, h) == 4


# ---- SSE / cdef moments ---------------------------------------------------
@pytest.mark.parametrize("bd,xdec,ydec", [(8, 0, 0), (8, 1, 1), (10, 0, 0), (10, 1, 0),
                                           (12, 0, 0), (12, 1, 1)])
def test_sse_vs_oracle(bd, xdec, ydec):
    rng = np.random.default_rng(7 + bd + xdec)
    a = rand_plane(rng, 160, 160, bd)
    b = rand_plane(rng, 160, 160, bd)
    pa = R.DevicePlane(160, 160, xdec, ydec, 8, 8, bd > 8)
    pa.upload_visible(a)
    pb = R.DevicePlane(160, 160, xdec, ydec, 8, 8, bd > 8)
    pb.upload_visible(b)
    for w, h in [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (32, 16), (8, 32), (128, 128)]:
        if (min(w, 8) >> xdec) == 0 or (min(h, 8) >> ydec) == 0:
            continue
        jobs = np.array([(0, 0, 0, 0), (5, 3, 17, 9), (160 - w, 160 - h, 1, 2)], dtype=R.DIST_JOB)
        got = R.sse_batch(pa, pb, jobs, w, h)
        for k, j in enumerate(jobs):
            want = O.sse_wxh(blk(a, j["org_y"], j["org_x"], h, w),
                             blk(b, j["ref_y"], j["ref_x"], h, w), w, h, xdec, ydec)
            np.testing.assert_array_equal(got[k], want, err_msg=str((w, h, k)))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_cdef_moments_vs_oracle(bd):
    rng = np.random.default_rng(11 + bd)
    a = rand_plane(rng, 130, 140, bd)
    b = rand_plane(rng, 130, 140, bd)
    pa, pb = R.DevicePlane.from_array(a), R.DevicePlane.from_array(b)
    for w, h in [(8, 8), (64, 64), (16, 32), (128, 64)]:
        jobs = np.array([(0, 0, 0, 0), (3, 1, 7, 2), (140 - w, 130 - h, 0, 0)], dtype=R.DIST_JOB)
        got = R.cdef_moments_batch(pa, pb, jobs, w, h)
        for k, j in enumerate(jobs):
            for s in range((w // 8) * (h // 8)):
                by, bx = divmod(s, w // 8)
                want = O.cdef_moments(blk(a, j["org_y"] + 8 * by, j["org_x"] + 8 * bx, 8, 8),
                                      blk(b, j["ref_y"] + 8 * by, j["ref_x"] + 8 * bx, 8, 8))
                np.testing.assert_array_equal(got[k, s], want)
                assert R.cdef_dist_from_moments(got[k, s], bd) == O.cdef_dist(want, bd)


# ---- MC -------------------------------------------------------------------
MC_SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (4, 16), (64, 16), (128, 128),
            (2, 4), (8, 2)]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_put_prep_vs_oracle(bd):
    rng = np.random.default_rng(200 + bd)
    src = rand_plane(rng, 200, 200, bd)
    # saturated stripes exercise the clamp (u8 overshoot, src/mc.rs:244-245)
    src[:, 40:48] = np.array([0, 1, 0, 1, 1, 0, 1, 0]) * ((1 << bd) - 1)
    ps = R.DevicePlane.from_array(src, xpad=16, ypad=16)
    fs = ps.download_full()
    xo, yo = ps.desc.xorigin, ps.desc.yorigin
    for (w, h) in MC_SIZES:
        fr = [(0, 0), (0, 6), (10, 0), (2, 14), (8, 8), (15, 1)]
        for mx, my in [(0, 0), (1, 2), (2, 2), (3, 3), (2, 1)]:
            jobs = np.zeros(len(fr), dtype=R.MC_JOB)
            for k, (cf, rf) in enumerate(fr):
                jobs[k] = (36 + 3 * k, 20 + 5 * k, 0, h * k, cf, rf)
            dst = R.DevicePlane(w, h * len(fr), 0, 0, 0, 0, bd > 8)
            R.put_8tap_batch(dst, ps, jobs, w, h, mx, my, bd)
            got = dst.download_visible()
            prep = R.prep_8tap_batch(ps, jobs, w, h, mx, my, bd)
            for k, (cf, rf) in enumerate(fr):
                want = O.put_8tap(fs, yo + jobs[k]["src_y"], xo + jobs[k]["src_x"], w, h, cf, rf,
                                  mx, my, bd=bd)
                np.testing.assert_array_equal(got[h * k:h * k + h], want,
                                              err_msg=str((w, h, cf, rf, mx, my)))
                wantp = O.prep_8tap(fs, yo + jobs[k]["src_y"], xo + jobs[k]["src_x"], w, h, cf,
                                    rf, mx, my, bd=bd)
                np.testing.assert_array_equal(prep[k], wantp)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_mc_avg_vs_oracle(bd):
    rng = np.random.default_rng(300 + bd)
    src = rand_plane(rng, 120, 120, bd)
    ps = R.DevicePlane.from_array(src, xpad=16, ypad=16)
    for w, h in [(8, 8), (16, 16), (64, 64), (32, 8)]:
        jobs = np.array([(20, 20, 0, 0, 6, 10), (24, 31, 0, h, 0, 12)], dtype=R.MC_JOB)
        t1 = R.prep_8tap_batch(ps, jobs, w, h, 0, 0, bd)
        t2 = R.prep_8tap_batch(ps, jobs[::-1].copy(), w, h, 2, 1, bd)
        dst = R.DevicePlane(w, 2 * h, 0, 0, 0, 0, bd > 8)
        R.mc_avg_batch(dst, t1, t2, jobs, w, h, bd)
        got = dst.download_visible()
        for k in range(2):
            want = O.mc_avg(t1[k], t2[k], bd=bd, hbd=1 if bd > 8 else 0)
            np.testing.assert_array_equal(got[h * k:h * k + h], want)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_mc_dist_fused_vs_oracle(bd):
    rng = np.random.default_rng(400 + bd)
    ref = rand_plane(rng, 200, 200, bd)
    org = rand_plane(rng, 200, 200, bd)
    pr = R.DevicePlane.from_array(ref, xpad=16, ypad=16)
    po = R.DevicePlane.from_array(org, xpad=16, ypad=16)
    fr = pr.download_full()
    xo, yo = pr.desc.xorigin, pr.desc.yorigin
    for w, h in [(8, 8), (16, 16), (64, 64), (32, 16), (4, 4), (16, 4)]:
        jobs = np.zeros(9, dtype=R.MC_JOB)
        for k in range(9):
            jobs[k] = (30 + k, 40 + 2 * k, 50, 60, (2 * k) % 16, (14 - 2 * k) % 16)
        for metric in (0, 1):
            got = R.mc_dist_batch(po, pr, jobs, w, h, 0, 0, bd, metric)
            for k in range(9):
                pred = O.put_8tap(fr, yo + jobs[k]["src_y"], xo + jobs[k]["src_x"], w, h,
                                  jobs[k]["col_frac"], jobs[k]["row_frac"], bd=bd)
                o = blk(org, 60, 50, h, w)
                want = O.get_sad(o, 0, 0, pred, 0, 0, w, h) if metric == 0 else \
                    O.get_satd(o, 0, 0, pred, 0, 0, w, h)
                assert got[k] == want, (w, h, k, metric)


# ---- transforms -----------------------------------------------------------
def test_fwd_inv_golden():
    g = np.load(os.path.join(GOLD, "tx2d_golden.npz"))
    keys = sorted({k.rsplit("_", 1)[0] for k in g.files if k.endswith("_out")})
    for key in keys:
        tag, s, t, bd = key.split("_")
        s, t, bd = int(s[1:]), int(t[1:]), int(bd[2:])
        w, h = 1 << O.TX_W_LOG2[s], 1 << O.TX_H_LOG2[s]
        if tag == "fwd":
            got = R.fwd_txfm_batch(g[key + "_in"].reshape(1, h, w), s, t, bd)[0]
        else:
            dst = g[key + "_dst"].astype(np.uint8 if bd == 8 else np.uint16).reshape(h, w)
            pd = R.DevicePlane.from_array(dst)
            R.inv_txfm_add_batch(g[key + "_coeffs"].reshape(1, -1), pd,
                                 np.array([(0, 0, 0, 0)], dtype=R.TX_JOB), s, t, bd)
            got = pd.download_visible()
        np.testing.assert_array_equal(np.asarray(got).ravel(), g[key + "_out"].ravel(),
                                      err_msg=key)


def _fwd_supported(s, t):
    return O.fwd_txfm2d(np.zeros((1 << O.TX_H_LOG2[s]) * (1 << O.TX_W_LOG2[s]), np.int16),
                        s, t, 8) is not None


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_fwd_random_vs_oracle(bd):
    rng = np.random.default_rng(500 + bd)
    for s in range(19):
        w, h = 1 << O.TX_W_LOG2[s], 1 << O.TX_H_LOG2[s]
        for t in range(16):
            if not _fwd_supported(s, t):
                with pytest.raises(R.Rav1eHipError):
                    R.fwd_txfm_batch(np.zeros((1, h, w), np.int16), s, t, bd)
                continue
            m = (1 << bd) - 1
            res = rng.integers(-m, m + 1, (5, h, w)).astype(np.int16)
            res[0] = m  # extremes
            res[1] = -m
            got = R.fwd_txfm_batch(res, s, t, bd)
            for k in range(5):
                np.testing.assert_array_equal(got[k], O.fwd_txfm2d(res[k], s, t, bd),
                                              err_msg=str((s, t, bd, k)))


def _inv_supported(s, t):
    w, h = 1 << O.TX_W_LOG2[s], 1 << O.TX_H_LOG2[s]
    return O.inv_txfm2d_add(np.zeros(min(w, 32) * min(h, 32), np.int32),
                            np.zeros((h, w), np.uint8), s, t, 8) is not None


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_inv_random_vs_oracle(bd):
    rng = np.random.default_rng(600 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    for s in range(19):
        w, h = 1 << O.TX_W_LOG2[s], 1 << O.TX_H_LOG2[s]
        cw, ch = min(w, 32), min(h, 32)
        for t in range(16):
            if not _inv_supported(s, t):
                continue
            n = 4
            co = rng.integers(-3000, 3000, (n, ch * cw)).astype(np.int32)
            co[0] = rng.integers(-(1 << 20), 1 << 20, ch * cw)  # exercise the clamps
            dst = rng.integers(0, 1 << bd, (h * n, w)).astype(dt)
            pd = R.DevicePlane.from_array(dst, xpad=8, ypad=8)
            jobs = np.array([(0, 0, 0, h * k) for k in range(n)], dtype=R.TX_JOB)
            R.inv_txfm_add_batch(co, pd, jobs, s, t, bd)
            got = pd.download_visible()
            for k in range(n):
                want = O.inv_txfm2d_add(co[k], dst[h * k:h * k + h], s, t, bd)
                np.testing.assert_array_equal(got[h * k:h * k + h], want, err_msg=str((s, t, k)))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_diff_fwd_fused_vs_oracle(bd):
    rng = np.random.default_rng(700 + bd - 8)
    src = rand_plane(rng, 140, 140, bd)
    pred = rand_plane(rng, 140, 140, bd)
    ps, pp = R.DevicePlane.from_array(src), R.DevicePlane.from_array(pred)
    for s, t in [(4, 0), (3, 0), (0, 3), (7, 2), (1, 9), (18, 0)]:
        w, h = 1 << O.TX_W_LOG2[s], 1 << O.TX_H_LOG2[s]
        jobs = np.array([(0, 0, 3, 5), (140 - w, 140 - h, 0, 0)], dtype=R.TX_JOB)
        got = R.diff_fwd_txfm_batch(ps, pp, jobs, s, t, bd)
        for k, j in enumerate(jobs):
            res = src[j["src_y"]:j["src_y"] + h, j["src_x"]:j["src_x"] + w].astype(np.int16) - \
                pred[j["pred_y"]:j["pred_y"] + h, j["pred_x"]:j["pred_x"] + w].astype(np.int16)
            np.testing.assert_array_equal(got[k], O.fwd_txfm2d(res, s, t, bd),
                                          err_msg=str((s, t, k)))


# ---- motion search --------------------------------------------------------
def _fs_case(rng, hbd, blk, nj, flat=False):
    bd = 10 if hbd else 8
    org = rand_plane(rng, 180, 260, bd)
    ref = np.roll(org, (3, -5), (0, 1)) if not flat else np.full_like(org, 77)
    if flat:
        org[:] = 77
    po_, pr_ = R.DevicePlane.from_array(org, xpad=40, ypad=40, bit_depth=bd), \
        R.DevicePlane.from_array(ref, xpad=40, ypad=40, bit_depth=bd)
    fo, fr = po_.download_full(), pr_.download_full()
    xo, yo = po_.desc.xorigin, po_.desc.yorigin
    jobs = np.zeros(nj, dtype=R.FS_JOB)
    for k in range(nj):
        px, py = int(rng.integers(0, 260 - blk)), int(rng.integers(0, 180 - blk))
        rx, ry = int(rng.integers(4, 60)), int(rng.integers(4, 20))
        jobs[k] = (px, py, max(px - rx, -30), min(px + rx, 260 - blk + 30),
                   max(py - ry, -30), min(py + ry, 180 - blk + 30),
                   int(rng.integers(-40, 40)), int(rng.integers(-40, 40)), 0, 0,
                   int(rng.integers(0, 3000)), 0)
    return po_, pr_, fo, fr, xo, yo, jobs


@pytest.mark.parametrize("hbd,blk,step", [(False, 16, 1), (False, 32, 1), (True, 16, 1),
                                          (False, 8, 2), (False, 16, 3)])
@pytest.mark.parametrize("sea", [False, True])
def test_full_search_vs_oracle(hbd, blk, step, sea):
    """Exhaustive kernels and (16x16, step 1) the successive-elimination
    path over box-sum tables vs orc_full_search."""
    if sea and (blk, step) != (16, 1):
        pytest.skip("the SEA entry point is 16x16, step 1")
    rng = np.random.default_rng(800 + blk + step)
    po_, pr_, fo, fr, xo, yo, jobs = _fs_case(rng, hbd, blk, 12)
    if sea:
        got = R.full_search_sea_batch(po_, pr_, jobs)
    else:
        got = R.full_search_batch(po_, pr_, jobs, blk, blk, step, allow_hp=False)
    for k, j in enumerate(jobs):
        mv, cost = O.full_search(fo, fr, xo, yo, j, blk, blk, step, 0)
        assert (got[k]["mv_row"], got[k]["mv_col"], got[k]["cost"]) == (mv[0], mv[1], cost), k


@pytest.mark.parametrize("sea", [False, True])
@pytest.mark.parametrize("scale", [4, 2, 1])
def test_full_search_replay_windows_vs_oracle(scale, sea):
    """The quarter-res coarse search of the replay (estimate_motion_ss4
    windows at me_range_scale 4/2/1, natural-ish content): the exact
    successive-elimination path must return the oracle's exhaustive
    argmin (cost and first raster index)."""
    from rav1e_amd import replay as RP
    W, H = 640, 384
    q = []
    for t in (0, 1):
        y = RP.synth_frame(W, H, t)[:W * H].reshape(H, W).astype(np.int32)
        for _ in range(2):
            y = (y[0::2, 0::2] + y[1::2, 0::2] + y[0::2, 1::2] + y[1::2, 1::2] + 2) >> 2
        q.append(y.astype(np.uint8))
    po_, pr_ = R.DevicePlane.from_array(q[0], xpad=22, ypad=22), R.DevicePlane.from_array(
        q[1], xpad=22, ypad=22)
    fo, fr = po_.download_full(), pr_.download_full()
    xo, yo = po_.desc.xorigin, po_.desc.yorigin
    qw, qh = W // 4, H // 4
    jobs = np.zeros(12, dtype=R.FS_JOB)
    rng = np.random.default_rng(1500 + scale)
    for k in range(len(jobs)):
        px, py = 16 * int(rng.integers(0, qw // 16)), 16 * int(rng.integers(0, qh // 16))
        rx, ry = 48 * scale, 16 * scale
        jobs[k] = (px, py, max(px - rx, -20), min(px + rx, qw - 16 + 20), max(py - ry, -20),
                   min(py + ry, qh - 16 + 20), int(rng.integers(-40, 40)),
                   int(rng.integers(-40, 40)), 0, 0, int(rng.integers(0, 200)), 0)
    if sea:
        got = R.full_search_sea_batch(po_, pr_, jobs)
    else:
        got = R.full_search_batch(po_, pr_, jobs, 16, 16, 1)
    for k, j in enumerate(jobs):
        mv, cost = O.full_search(fo, fr, xo, yo, j, 16, 16, 1, 0)
        assert (got[k]["mv_row"], got[k]["mv_col"], got[k]["cost"]) == (mv[0], mv[1], cost), k


@pytest.mark.parametrize("sea", [False, True])
def test_full_search_ties_keep_first_raster_candidate(sea):
    rng = np.random.default_rng(900)
    po_, pr_, fo, fr, xo, yo, jobs = _fs_case(rng, False, 16, 6, flat=True)
    jobs["lambda_"] = 0  # every candidate costs 0: the first raster one wins
    if sea:
        got = R.full_search_sea_batch(po_, pr_, jobs)
    else:
        got = R.full_search_batch(po_, pr_, jobs, 16, 16, 1)
    for k, j in enumerate(jobs):
        mv, cost = O.full_search(fo, fr, xo, yo, j, 16, 16, 1, 0)
        assert cost == 0
        assert (got[k]["mv_row"], got[k]["mv_col"]) == mv
        assert mv == (8 * (j["y_lo"] - j["po_y"]), 8 * (j["x_lo"] - j["po_x"]))


@pytest.mark.parametrize("hbd", [False, True])
def test_plane_box_sums_vs_numpy(hbd):
    """rv_plane_box_sums over the whole allocation (padding included) vs an
    integral-image box sum of 4-tall x KW-wide blocks, paired as
    S(x, y) | S(x + KW, y) << 16 for KW = 8 then 4; a half whose block
    leaves the allocation is 0."""
    rng = np.random.default_rng(950 + hbd)
    a = rand_plane(rng, 70, 90, 10 if hbd else 8)
    p = R.DevicePlane.from_array(a, xpad=12, ypad=12, bit_depth=10 if hbd else 8)
    full = p.download_full().astype(np.int64)
    got = R.plane_box_sums(p).download(np.uint32).reshape((2,) + full.shape).astype(np.int64)
    ii = np.zeros((full.shape[0] + 1, full.shape[1] + 1), np.int64)
    ii[1:, 1:] = full.cumsum(0).cumsum(1)
    kh = 4
    for t, kw in enumerate((8, 4)):
        sk = np.zeros(full.shape, np.int64)
        sk[:1 - kh, :1 - kw] = ii[kh:, kw:] - ii[:-kh, kw:] - ii[kh:, :-kw] + ii[:-kh, :-kw]
        hi = np.zeros_like(sk)
        hi[:, :-kw] = sk[:, kw:]
        np.testing.assert_array_equal(got[t] & 0xFFFF, sk, err_msg=f"KW={kw} low")
        np.testing.assert_array_equal(got[t] >> 16, hi, err_msg=f"KW={kw} high")


@pytest.mark.parametrize("hbd", [False, True])
def test_full_search_sea_pruning_edge_cases(hbd):
    """SEA path: flat + textured mixes, huge lambdas (exhaustive fallback),
    windows clipped into the padding, the mv-0 probe outside the window."""
    rng = np.random.default_rng(960 + hbd)
    bd = 10 if hbd else 8
    org = rand_plane(rng, 120, 200, bd)
    org[:, :100] = org[:, :100] // 64 * 64  # quantised half: many LB ties
    ref = np.roll(org, (2, 7), (0, 1))
    po_, pr_ = R.DevicePlane.from_array(org, xpad=24, ypad=24, bit_depth=bd), \
        R.DevicePlane.from_array(ref, xpad=24, ypad=24, bit_depth=bd)
    fo, fr = po_.download_full(), pr_.download_full()
    xo, yo = po_.desc.xorigin, po_.desc.yorigin
    jobs = np.zeros(12, dtype=R.FS_JOB)
    for k in range(len(jobs)):
        px, py = int(rng.integers(0, 200 - 16)), int(rng.integers(0, 120 - 16))
        lam = [0, 40, 3000, (1 << 23) - 1, 1 << 23, (1 << 26) + 5][k % 6]
        if k == 7:  # window far from mv 0: the probe finds nothing
            jobs[k] = (px, py, -24, -24 + 30, -24, -24 + 9, 0, 0, 0, 0, lam, 0)
            continue
        if k in (10, 11):  # mv 0 on a window corner: the 4x4 probe mostly clamped away
            x_lo, y_lo = (px, py) if k == 10 else (px - 30, py - 9)
            jobs[k] = (px, py, x_lo, x_lo + 30, y_lo, y_lo + 9, 0, 0, 0, 0, lam, 0)
            continue
        jobs[k] = (px, py, max(px - 40, -24), min(px + 40, 200 - 16 + 24), max(py - 12, -24),
                   min(py + 12, 120 - 16 + 24), int(rng.integers(-40, 40)),
                   int(rng.integers(-40, 40)), 0, 0, lam, 0)
    got = R.full_search_sea_batch(po_, pr_, jobs)
    for k, j in enumerate(jobs):
        mv, cost = O.full_search(fo, fr, xo, yo, j, 16, 16, 1, 0)
        assert (got[k]["mv_row"], got[k]["mv_col"], got[k]["cost"]) == (mv[0], mv[1], cost), k


def test_full_search_sea_rejects_12bit_and_unstated_depth():
    """The packed 16-bit box sums overflow for 12-bit pixels: the SEA entry
    points refuse u16 planes that do not state bit_depth 9 or 10."""
    a = np.full((64, 64), 4000, np.uint16)
    for bd in (12, None):
        p = R.DevicePlane.from_array(a, xpad=16, ypad=16, bit_depth=bd)
        with pytest.raises(R.Rav1eHipError):
            R.plane_box_sums(p)
        jobs = np.zeros(1, dtype=R.FS_JOB)
        jobs[0] = (0, 0, 0, 4, 0, 4, 0, 0, 0, 0, 1, 0)
        box = R.DeviceBuffer(8 * p.desc.stride * p.desc.alloc_height)
        with pytest.raises(R.Rav1eHipError):
            R.full_search_sea_batch(p, p, jobs, s8=box)


def test_full_search_empty_window():
    a = np.zeros((64, 64), np.uint8)
    pa = R.DevicePlane.from_array(a, xpad=16, ypad=16)
    jobs = np.zeros(1, dtype=R.FS_JOB)
    jobs[0] = (0, 0, 5, 4, 0, 0, 0, 0, 0, 0, 1, 0)  # x_hi < x_lo
    got = R.full_search_batch(pa, pa, jobs, 16, 16)
    assert got[0]["cost"] == 2 ** 64 - 1 and got[0]["mv_row"] == 0 and got[0]["mv_col"] == 0


def _ds_case(rng, bd, w, h, nj, subpel, edge=False):
    H, W = 200, 280
    org = rand_plane(rng, H, W, bd) if not edge else np.zeros((H, W), np.uint16 if bd > 8
                                                             else np.uint8)
    # reference = org moved by a sub-pel-ish amount plus noise, so the search has a trend
    ref = np.roll(org, (2, -3), (0, 1))
    if not edge:
        noise = rng.integers(-3, 4, ref.shape)
        ref = np.clip(ref.astype(np.int32) + noise, 0, (1 << bd) - 1).astype(org.dtype)
    else:  # 0 / max step edges: the MC overshoot cases
        ref[:, ::2] = (1 << bd) - 1
    po_ = R.DevicePlane.from_array(org, xpad=88, ypad=88)
    pr_ = R.DevicePlane.from_array(ref, xpad=88, ypad=88)
    fo, fr = po_.download_full(), pr_.download_full()
    jobs = np.zeros(nj, dtype=R.DS_JOB)
    for k in range(nj):
        px = int(rng.integers(-8, W - w + 8)) if k % 3 else 0
        py = int(rng.integers(-8, H - h + 8)) if k % 3 else H - h
        span = 8 * int(rng.integers(2, 24))
        jobs[k]["po_x"], jobs[k]["po_y"] = px, py
        jobs[k]["mvx_min"], jobs[k]["mvx_max"] = -span, span
        jobs[k]["mvy_min"], jobs[k]["mvy_max"] = -span // 2, span // 2
        jobs[k]["pmv0_row"], jobs[k]["pmv0_col"] = rng.integers(-40, 40, 2)
        jobs[k]["lambda_"] = int(rng.integers(0, 4000))
        n = int(rng.integers(1, 9))
        jobs[k]["n_pred"] = n
        step = 1 if subpel else 8
        jobs[k]["pred"][:n] = rng.integers(-12, 12, (n, 2)) * step
        if k % 4 == 1:  # a predictor out of range
            jobs[k]["pred"][0] = (span + 8, 0)
    return po_, pr_, fo, fr, jobs, W, H


@pytest.mark.parametrize("bd,w,h,subpel,satd", [
    (8, 64, 64, False, False), (8, 64, 64, True, False), (8, 32, 32, False, False),
    (8, 32, 32, True, False), (8, 16, 32, True, False), (8, 64, 32, True, False),
    (10, 64, 64, False, False), (10, 64, 64, True, False), (10, 32, 32, True, False),
    (8, 8, 8, True, False), (8, 16, 16, True, True), (10, 32, 32, False, True),
    # lane-group kernel: SATD sub-pel at every square size, small full-pel
    (8, 8, 8, True, True), (10, 8, 8, True, True), (12, 16, 16, True, True),
    (10, 32, 32, True, True), (8, 64, 64, True, True), (10, 64, 64, True, True),
    (8, 8, 8, False, False), (10, 16, 16, False, False), (12, 8, 8, False, True),
    (10, 16, 16, True, False),
])
def test_diamond_search_vs_oracle(bd, w, h, subpel, satd):
    """Fast (wavefront-per-candidate) and generic paths vs orc_diamond_search."""
    rng = np.random.default_rng(1100 + w + 7 * h + bd + subpel)
    po_, pr_, fo, fr, jobs, W, H = _ds_case(rng, bd, w, h, 24, subpel)
    xo, yo = po_.desc.xorigin, po_.desc.yorigin
    for hp in (False, True) if subpel else (False,):
        got = R.diamond_search_batch(po_, pr_, jobs, w, h, subpel, satd, hp, bd)
        for k, j in enumerate(jobs):
            mv, cost = O.diamond_search(fo, fr, xo, yo, W, H, j, w, h, subpel, satd, hp, bd)
            assert (got[k]["mv_row"], got[k]["mv_col"], got[k]["cost"]) == (mv[0], mv[1], cost), \
                (k, hp, got[k], mv, cost)


@pytest.mark.parametrize("bd,n,satd", [(8, 64, False), (10, 64, False), (10, 8, True),
                                       (12, 32, True)])
def test_diamond_subpel_edges_vs_oracle(bd, n, satd):
    """0/max column stripes (8-tap overshoot) and blocks clamped at the frame edge."""
    rng = np.random.default_rng(1200 + bd + n)
    po_, pr_, fo, fr, jobs, W, H = _ds_case(rng, bd, n, n, 16, True, edge=True)
    xo, yo = po_.desc.xorigin, po_.desc.yorigin
    got = R.diamond_search_batch(po_, pr_, jobs, n, n, True, satd, False, bd)
    for k, j in enumerate(jobs):
        mv, cost = O.diamond_search(fo, fr, xo, yo, W, H, j, n, n, True, satd, False, bd)
        assert (got[k]["mv_row"], got[k]["mv_col"], got[k]["cost"]) == (mv[0], mv[1], cost), k


@pytest.mark.parametrize("bd,w,h,satd", [
    (8, 64, 64, False), (8, 32, 32, False), (10, 64, 64, False), (8, 16, 32, False),
    (8, 16, 16, True), (10, 8, 8, True), (8, 8, 16, False),
])
def test_telescopic_subpel_vs_oracle(bd, w, h, satd):
    """telescopic_subpel_search (src/me.rs:858-941): fast and generic paths."""
    rng = np.random.default_rng(1300 + w + 3 * h + bd + satd)
    po_, pr_, fo, fr, jobs, W, H = _ds_case(rng, bd, w, h, 20, False)
    xo, yo = po_.desc.xorigin, po_.desc.yorigin
    start = np.zeros(len(jobs), dtype=R.FS_RESULT)
    for k in range(len(jobs)):  # full-pel starting points, some out of range
        start[k]["mv_row"], start[k]["mv_col"] = 8 * rng.integers(-3, 4), 8 * rng.integers(-3, 4)
        start[k]["cost"] = int(rng.integers(0, 1 << 22)) if k % 5 else 2 ** 64 - 1
    for hp in (False, True):
        got = R.telescopic_subpel_batch(po_, pr_, jobs, start, w, h, satd, hp, bd)
        for k, j in enumerate(jobs):
            mv, cost = O.telescopic_subpel(fo, fr, xo, yo, W, H, j, w, h, satd, hp, bd,
                                           (start[k]["mv_row"], start[k]["mv_col"]),
                                           start[k]["cost"])
            assert (got[k]["mv_row"], got[k]["mv_col"], got[k]["cost"]) == (mv[0], mv[1], cost), \
                (k, hp, got[k], mv, cost)


@pytest.mark.parametrize("tx_size", [0, 1, 2, 3, 4, 9, 12, 17])
def test_tx_dist_vs_oracle(tx_size):
    """tx-domain distortion (src/encoder.rs:1210-1224), incl. i32-wrapping squares."""
    rng = np.random.default_rng(1400 + tx_size)
    tw, th = R.TxSize(tx_size).width(), R.TxSize(tx_size).height()
    area = min(tw, 32) * min(th, 32)
    n = 9
    co = rng.integers(-40000, 40000, (n, tw * th)).astype(np.int32)
    rc = (co[:, :area] // 8 * 8 + rng.integers(-3, 4, (n, area))).astype(np.int32)
    co[0, :4] = [2 ** 31 - 1, -2 ** 31, 70000, -70000]  # wrapping squares
    rc[0, :4] = [-2 ** 31, 2 ** 31 - 1, 0, 0]
    got = R.tx_dist_batch(co, rc, tx_size)
    for b in range(n):
        assert int(got[b]) == O.tx_dist(co[b, :area], rc[b], tw, th), b


# ---- frame layout -----------------------------------------------------------
@pytest.mark.parametrize("hbd", [False, True])
def test_pad_and_downsample_vs_oracle(hbd):
    rng = np.random.default_rng(1000)
    bd = 10 if hbd else 8
    a = rand_plane(rng, 120, 200, bd)
    p = R.DevicePlane.from_array(a, xpad=88, ypad=88)
    full = p.download_full()
    want = np.zeros_like(full)
    d = p.desc
    want[d.yorigin:d.yorigin + 120, d.xorigin:d.xorigin + 200] = a
    O.lib().orc_plane_pad(O.ptr(want), d.stride, d.alloc_height, d.xorigin, d.yorigin, 0, 0,
                          200, 120, 1 if hbd else 0)
    np.testing.assert_array_equal(full, want)
    q = R.DevicePlane(100, 60, 1, 1, 44, 44, hbd)
    R._check(R.lib().rv_plane_downsample(C.byref(q.desc), C.byref(p.desc), None), "ds")
    R._sync()
    got = q.download_visible()
    exp = np.zeros((60, 100), dtype=a.dtype)
    O.lib().orc_downsample(O.ptr(exp), 100, 100, 60, O.ptr(a), 200, 1 if hbd else 0)
    np.testing.assert_array_equal(got, exp)


# ---- drop-in asm-shaped entry points ---------------------------------------
def test_asm_shims_match_oracle():
    L = R.lib()
    rng = np.random.default_rng(1100)
    a = rng.integers(0, 256, (80, 96)).astype(np.uint8)
    b = rng.integers(0, 256, (80, 96)).astype(np.uint8)
    for bs in (R.BlockSize.BLOCK_4X4, R.BlockSize.BLOCK_16X16, R.BlockSize.BLOCK_64X16,
               R.BlockSize.BLOCK_8X32):
        w, h = bs.width(), bs.height()
        f = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t)(
            L.rv_sad_fn(int(R.CpuFeatureLevel.HIP), int(bs), 0))
        g = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t)(
            L.rv_satd_fn(int(R.CpuFeatureLevel.HIP), int(bs), 0))
        pa, pb = O.ptr(a, 3 * 96 + 5), O.ptr(b, 7 * 96 + 2)
        assert f(pa, 96, pb, 96) == O.get_sad(a, 3, 5, b, 7, 2, w, h)
        assert g(pa, 96, pb, 96) == O.get_satd(a, 3, 5, b, 7, 2, w, h)
    assert L.rv_sad_fn(int(R.CpuFeatureLevel.AVX2), 6, 0) is None
    # put / prep / avg with the NASM argument order (src/asm/x86/mc.rs:17-78)
    dst = np.zeros((16, 16), np.uint8)
    L.rav1e_put_8tap_sharp_smooth_hip(O.ptr(dst), C.c_ssize_t(16), O.ptr(a, 20 * 96 + 20),
                                      C.c_ssize_t(96), 16, 16, 6, 10)
    np.testing.assert_array_equal(dst, O.put_8tap(a, 20, 20, 16, 16, 6, 10, 2, 1))
    tmp = np.zeros((8, 8), np.int16)
    L.rav1e_prep_8tap_regular_regular_hip(O.ptr(tmp), O.ptr(a, 30 * 96 + 30), C.c_ssize_t(96),
                                          8, 8, 4, 0)
    np.testing.assert_array_equal(tmp, O.prep_8tap(a, 30, 30, 8, 8, 4, 0))
    avg = np.zeros((8, 8), np.uint8)
    L.rav1e_avg_hip(O.ptr(avg), C.c_ssize_t(8), O.ptr(tmp), O.ptr(tmp), 8, 8)
    np.testing.assert_array_equal(avg, O.mc_avg(tmp, tmp))
    # transforms
    res = rng.integers(-255, 256, (32, 32)).astype(np.int16)
    co = np.zeros(32 * 32, np.int32)
    assert L.rav1e_fwd_txfm_hip(O.ptr(res), O.ptr(co), 3, 0, 8) == 0
    np.testing.assert_array_equal(co, O.fwd_txfm2d(res, 3, 0, 8))
    d = rng.integers(0, 256, (32, 32)).astype(np.uint8)
    want = O.inv_txfm2d_add(co // 8, d, 3, 0, 8)
    assert L.rav1e_inv_txfm_add_hip(O.ptr((co // 8).astype(np.int32)), O.ptr(d), 32, 3, 0, 8) == 0
    np.testing.assert_array_equal(d, want)


# ---- quantize / dequantize (src/quantize.rs) ----------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_lookahead_intra_costs_vs_oracle(bd):
    """rv_lookahead_intra_costs vs the oracle on the same padded plane, with
    sizes that leave partial last blocks (read from the padding)."""
    rng = np.random.default_rng(2000 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    for w, h in ((64, 64), (100, 60), (1920, 1080)):
        a = rng.integers(0, 1 << bd, (h, w)).astype(dt)
        p = R.DevicePlane.from_array(a, xpad=16, ypad=16)
        got = R.lookahead_intra_costs(p, bd)
        full = p.download_full()
        want = O.lookahead_intra_costs(full, p.desc.yorigin, p.desc.xorigin, w, h, bd)
        np.testing.assert_array_equal(got, want, err_msg=f"{bd} {w}x{h}")


@pytest.mark.gpu
@pytest.mark.parametrize("bd,n_unique", [(8, 1), (8, 2), (10, 3)])
def test_propagate_importances_vs_oracle(bd, n_unique):
    """rv_propagate_importances vs the oracle, f32 bit patterns: 1080p-sized
    importance grid (32400 blocks), sub-pel and negative MVs, zero intra
    costs, many sources per target (a constant MV field piles four sources
    onto most targets) -- the sort-and-ordered-sum must reproduce the
    reference's += sequence exactly."""
    rng = np.random.default_rng(2100 + bd + n_unique)
    dt = np.uint8 if bd == 8 else np.uint16
    w, h = 1920, 1080
    a = rng.integers(0, 1 << bd, (h, w)).astype(dt)
    b = np.roll(a, (3, -5), axis=(0, 1)) + rng.integers(0, 4, (h, w)).astype(dt)
    b = np.minimum(b, (1 << bd) - 1).astype(dt)
    po = R.DevicePlane.from_array(a, xpad=88, ypad=88)
    pr = R.DevicePlane.from_array(b, xpad=88, ypad=88)
    nbx, nby = w // 8, h // 8
    mvs = np.zeros((nby, nbx), dtype=R.MOTION_VECTOR)
    mvs["row"] = rng.integers(-512, 513, (nby, nbx))
    mvs["col"] = rng.integers(-512, 513, (nby, nbx))
    # the true motion (b is a rolled by (3, -5)) with sub-pel parts: small
    # inter costs, so these blocks propagate
    mvs[: nby // 2, : nbx // 2] = (np.int16(3 * 8 + 5), np.int16(-5 * 8 + 3))
    intra = R.lookahead_intra_costs(po, bd)
    intra[0, :50] = 0
    imp = (rng.random((nby, nbx)) * 1000).astype(np.float32)
    ref0 = (rng.random((nby, nbx)) * 300).astype(np.float32)
    got = R.propagate_importances(po, pr, mvs, intra, imp, n_unique, ref0)
    of, rf = po.download_full(), pr.download_full()
    mv2 = np.stack([mvs["row"], mvs["col"]], axis=-1)
    want = O.propagate_importances(of, po.desc.yorigin, po.desc.xorigin, rf, pr.desc.yorigin,
                                   pr.desc.xorigin, w, h, mv2, intra, imp, n_unique, ref0)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got != ref0).mean() > 0.2


@pytest.mark.gpu
def test_estimate_rate_vs_oracle():
    """rv_estimate_rate_batch vs orc_estimate_rate, every TxSize at several
    base qindices, over bin edges, the clamped top bins and large values."""
    rng = np.random.default_rng(1900)
    fd = np.concatenate([np.array([0, 1, 1999, 2000, 97999, 98000, 99999, 100000, 10 ** 7, 2 ** 40],
                                  dtype=np.uint64),
                         rng.integers(0, 120000, 54).astype(np.uint64)])
    for qi in (0, 60, 100, 255):
        for ts in range(19):
            got = R.estimate_rate_batch(fd, ts, qi)
            want = [O.estimate_rate(qi, ts, int(v)) for v in fd]
            np.testing.assert_array_equal(got, np.array(want, dtype=np.uint64), err_msg=f"{qi} {ts}")
    assert R.estimate_rate_batch(np.zeros(0, np.uint64), 0, 0).size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("tx_size,tx_type", [(4, 0), (3, 0), (0, 0), (1, 3), (2, 9), (5, 0),
                                              (11, 0), (17, 0), (2, 11), (3, 10)])
def test_quantize_vs_oracle(tx_size, tx_type):
    """rv_quantize_batch / rv_dequantize_batch vs orc_quantize /
    orc_dequantize: levels, dequantized values and eob, bit for bit, over
    8/10/12 bits, several qindices, intra and inter; the input is the
    forward transform's full W*H raster as encode_tx_block hands it over."""
    rng = np.random.default_rng(1500 + 16 * tx_size + tx_type)
    t = R.TxSize(tx_size)
    area, coded = t.width() * t.height(), R.coded_tx_area(tx_size)
    for bd in (8, 10, 12):
        for qi in (1, 40, 120, 255):
            acq = O.lib().orc_ac_q(qi, 0, bd)
            for is_intra in (False, True):
                n = 12
                c = rng.integers(-4 * acq, 4 * acq, (n, area)).astype(np.int32)
                c[rng.random((n, area)) < 0.6] = 0
                c[0] = 0                                    # eob = 1, all zero
                c[1, :] = 0
                c[1, 0] = 5 * acq                           # DC only
                c[2] = rng.integers(-(1 << 18), 1 << 18, area)  # large values
                q, r, eob = R.quantize_batch(c, tx_size, tx_type, qi, bd, is_intra)
                for k in range(n):
                    wq, weob = O.quantize(c[k], tx_size, tx_type, qi, bd, is_intra)
                    assert int(eob[k]) == weob, (bd, qi, is_intra, k)
                    np.testing.assert_array_equal(q[k], wq, err_msg=f"{bd} {qi} {is_intra} {k}")
                    np.testing.assert_array_equal(r[k], O.dequantize(wq, tx_size, qi, bd))
                np.testing.assert_array_equal(R.dequantize_batch(q, tx_size, qi, bd), r)


# ---- intra prediction (src/predict.rs:202-241, 538-1035) -------------------
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_predict_intra_vs_oracle(bd):
    """Every intra mode (PAETH through its variant remap) x every
    PredictionVariant x all 19 TxSizes, random and saturated edge buffers."""
    rng = np.random.default_rng(900 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    for tx in range(19):
        w, h = 1 << O.TX_W_LOG2[tx], 1 << O.TX_H_LOG2[tx]
        combos = [(m, v) for m in range(13) for v in range(4)]
        edges = rng.integers(0, 1 << bd, (len(combos) + 2, R.EDGE_PX)).astype(dt)
        edges[-2] = (1 << bd) - 1
        edges[-1, ::2] = 0
        edges[-1, 1::2] = (1 << bd) - 1
        combos += [(9, 3), (5, 3)]
        jobs = np.zeros(len(combos), dtype=R.INTRA_JOB)
        for k, (m, v) in enumerate(combos):
            jobs[k] = (0, k * h, m, v)
        dst = R.DevicePlane(w, h * len(combos), 0, 0, 0, 0, bd > 8)
        R.predict_intra_batch(dst, jobs, edges, tx, bd)
        got = dst.download_visible()
        for k, (m, v) in enumerate(combos):
            want = O.predict_intra(m, v, w, h, edges[k], bd)
            np.testing.assert_array_equal(got[k * h:(k + 1) * h], want, err_msg=str((tx, m, v)))


def test_predict_intra_reference_kats():
    """The reference's own 4x4 known answers (src/predict.rs:1047-1107)
    through the HIP path."""
    eb = [max(i + 32 - 64, 0) for i in range(129)]
    e = np.zeros(R.EDGE_PX, np.uint8)
    e[124:128], e[128], e[129:133] = eb[60:64], eb[64], eb[65:69]
    kats = [(0, 3, [32] * 16), (0, 2, [35] * 16), (0, 1, [30] * 16), (0, 0, [128] * 16),
            (1, 3, [33, 34, 35, 36] * 4), (2, 3, [31] * 4 + [30] * 4 + [29] * 4 + [28] * 4),
            (12, 3, [32, 34, 35, 36, 30, 32, 32, 36, 29, 32, 32, 32, 28, 28, 32, 32]),
            (9, 3, [32, 34, 35, 35, 30, 32, 33, 34, 29, 31, 32, 32, 29, 30, 32, 32]),
            (11, 3, [31, 33, 34, 35, 30, 33, 34, 35, 29, 32, 34, 34, 28, 31, 33, 34]),
            (10, 3, [33, 34, 35, 36, 31, 31, 32, 33, 30, 30, 30, 31, 29, 30, 30, 30])]
    jobs = np.zeros(len(kats), dtype=R.INTRA_JOB)
    for k, (m, v, _) in enumerate(kats):
        jobs[k] = (0, 4 * k, m, v)
    dst = R.DevicePlane(4, 4 * len(kats), 0, 0, 0, 0, False)
    R.predict_intra_batch(dst, jobs, np.tile(e, (len(kats), 1)), 0, 8)
    got = dst.download_visible()
    for k, (m, v, want) in enumerate(kats):
        assert got[4 * k:4 * k + 4].ravel().tolist() == want, (m, v)

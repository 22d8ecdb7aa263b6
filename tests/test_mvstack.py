"""rav1e's MV reference stacks for blocks of every size as a device operator
(rav1e_amd/csrc/rv_mvstack.hip: grid paint, find_mvrefs for a batch of
queries, the stack fields of rv_ec_mode_job) against the reference-evaluated
vectors (tests/golden/ref_mvref.npz, ref_mvref_rect.npz) and the oracle
(oracle/orc_mvref.c).  Every comparison is integer and exact.

The scenes are random partitions with PARTITION_HORZ / VERT leaves on ragged
tiles; their seeds are fixed, chosen on the CPU so that the oracle alone shows
every feature the tests assert (an empty stack, a long one, the 16-step of a
64x64 block, the clamp, the extra search with a sign flip and the compound
completion)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rav1e_amd as R
from tests import oracle_lib as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PAIRS = ((1, 8), (2, 8), (1, 2))
# (w4, h4) -> BlockSize (src/partition.rs:116-140)
BSIZE = {(2, 2): 3, (2, 4): 4, (4, 2): 5, (4, 4): 6, (4, 8): 7, (8, 4): 8, (8, 8): 9, (8, 16): 10,
         (16, 8): 11, (16, 16): 12}
N4_OF = {v: k for k, v in BSIZE.items()}
NEWMV_MODES = (19, 22, 23, 24, 25, 27)  # NEWMV, NEAREST_NEWMV, NEW_NEARESTMV, NEAR_NEWMV, NEW_NEARMV, NEW_NEWMV
# two tiles of 3 x 2 superblocks with ragged edges inside a 92 x 58 frame: tile 0
# ends at the frame's right edge and starts at its top, tile 1 at its left and bottom
TILES = ((44, 30, 48, 0), (48, 26, 0, 32))
FRAME = (92, 58)
SIGN_BIAS = 0b1010010  # LAST2, BWDREF and ALTREF look backwards from the others
SCENE_SEED, TOKEN_SEED = 3, 5


def bias_list(mask):
    return [(mask >> i) & 1 for i in range(7)]


def default_grid(h, w):
    g = np.zeros((h, w), O.BLK)
    g["n4_w"] = g["n4_h"] = 16
    return g


def load_vectors(name):
    """[(grid (Hh, W) BLK, (cols, rows, tx, ty), (fcols, frows), sign-bias mask,
    queries (k, 9), entries (k, 9, 5))] per case"""
    g = np.load(os.path.join(GOLD, name))
    out, off = [], 0
    for (case, tx, ty, cols, rows, fcols, frows, W, Hh, sb0, sb1) in g["grids"]:
        c = g["cells"][off:off + W * Hh]
        off += W * Hh
        b = np.zeros(W * Hh, O.BLK)
        b["ref"] = c[:, 0:2]
        b["mv"][:, 0] = c[:, 2:4]
        b["mv"][:, 1] = c[:, 4:6]
        b["n4_w"], b["n4_h"], b["newmv"] = c[:, 6], c[:, 7], c[:, 8]
        sel = g["query"][:, 0] == case
        out.append((b.reshape(Hh, W), (int(cols), int(rows), int(tx), int(ty)),
                    (int(fcols), int(frows)), int(sb0) | int(sb1) << 1, g["query"][sel],
                    g["entries"][sel]))
    assert off == len(g["cells"])
    return out


def oracle_results(grid, tile, frame, mask, queries):
    """R.MVREF_RESULT of rows (bx, by, bw4, bh4, r0, r1) on one tile's grid"""
    res = np.zeros(len(queries), R.MVREF_RESULT)
    for i, (bx, by, bw4, bh4, r0, r1) in enumerate(queries):
        ctx, st = O.find_mvrefs(grid, tile[0], tile[1], tile[2], tile[3], frame[0], frame[1],
                                int(bx), int(by), int(bw4), int(bh4), (int(r0), int(r1)),
                                bias_list(mask))
        res[i]["mode_context"], res[i]["n"] = ctx, len(st)
        res[i]["stack"][:len(st)] = st
    return res


# ----------------------------------------------------------------- scenes
def partition(rng, cols, rows, rect=True, p_split=0.5):
    """Coding-order leaves (x, y, w4, h4) and partition nodes (x, y, n4, split)
    of one tile: NONE / SPLIT / HORZ / VERT down to 8x8, SPLIT wherever a block
    crosses the tile's edge (encode_partition_topdown); `order`: both, in
    coding order, as ("node", ...) / ("leaf", ...)."""
    order = []

    def tree(x, y, n4):
        if x >= cols or y >= rows:
            return
        h = n4 // 2
        crossing = x + n4 > cols or y + n4 > rows
        r = rng.random()
        if n4 > 2 and (crossing or r < p_split):
            order.append(("node", x, y, n4, 3))
            for dy in (0, h):
                for dx in (0, h):
                    tree(x + dx, y + dy, h)
        elif rect and n4 > 2 and r < p_split + 0.15:
            order.append(("leaf", x, y, n4, h))
            order.append(("leaf", x, y + h, n4, h))
        elif rect and n4 > 2 and r < p_split + 0.3:
            order.append(("leaf", x, y, h, n4))
            order.append(("leaf", x + h, y, h, n4))
        else:
            order.append(("node", x, y, n4, 0))
            order.append(("leaf", x, y, n4, n4))
    for sy in range(0, rows, 16):
        for sx in range(0, cols, 16):
            tree(sx, sy, 16)
    return order


def rand_mv(rng, pool):
    if rng.random() < 0.7:
        return pool[int(rng.integers(0, len(pool)))]
    return (int(rng.integers(-300, 301)), int(rng.integers(-300, 301)))


def rand_block_job(rng, pool, t, x, y, w4, h4):
    """An intra, single-reference or compound leaf as an EC_MODE_JOB row with
    zeroed stack fields"""
    j = np.zeros(1, R.EC_MODE_JOB)[0]
    j["tile"], j["bx"], j["by"], j["bsize"] = t, x, y, BSIZE[(w4, h4)]
    r = rng.random()
    if r < 0.25:
        j["luma_mode"], j["ref1"] = int(rng.integers(0, 13)), 8
        return j
    if r < 0.5:
        j["ref0"], j["ref1"], mode = 1, 2, int(rng.integers(20, 28))
        m0, m1 = rand_mv(rng, pool), rand_mv(rng, pool)
    else:
        j["ref0"], j["ref1"], mode = int(rng.integers(1, 3)), 8, int(rng.integers(14, 20))
        m0, m1 = rand_mv(rng, pool), (0, 0)
    j["luma_mode"] = j["chroma_mode"] = mode
    j["mv0_row"], j["mv0_col"], j["mv1_row"], j["mv1_col"] = m0 + m1
    return j


def np_paint(jobs, tiles, grid_h, grid_w):
    """The paint's rules on the host: (n_tiles, grid_h, grid_w) BLK"""
    g = np.stack([default_grid(grid_h, grid_w) for _ in tiles])
    for j in jobs:
        if j["kind"] != 0 or not 0 <= j["tile"] < len(tiles):
            continue
        cols, rows = tiles[j["tile"]][:2]
        w4, h4 = N4_OF[int(j["bsize"])]
        x, y = int(j["bx"]), int(j["by"])
        if not (0 <= x < cols and 0 <= y < rows):
            continue
        c = g[j["tile"], y:min(y + h4, rows), x:min(x + w4, cols)]
        c["ref"] = (j["ref0"], j["ref1"])
        c["n4_w"], c["n4_h"] = w4, h4
        c["newmv"] = int(j["luma_mode"]) in NEWMV_MODES
        c["mv"] = ((j["mv0_row"], j["mv0_col"]), (j["mv1_row"], j["mv1_col"]))
    return g


@functools.lru_cache(maxsize=None)
def scene():
    """The whole-tile scene: jobs (coding order, blocks only), the numpy-painted
    grids, every leaf x PAIRS as queries (tile, bx, by, bw4, bh4, r0, r1) and the
    oracle's results."""
    rng = np.random.default_rng(SCENE_SEED)
    pool = [(int(rng.integers(-300, 301)), int(rng.integers(-300, 301))) for _ in range(4)]
    jobs, queries = [], []
    for t, (cols, rows, _, _) in enumerate(TILES):
        for it in partition(rng, cols, rows, p_split=0.35):
            if it[0] != "leaf":
                continue
            _, x, y, w4, h4 = it
            jobs.append(rand_block_job(rng, pool, t, x, y, w4, h4))
            queries += [(t, x, y, w4, h4, r0, r1) for (r0, r1) in PAIRS]
    jobs = np.array(jobs, R.EC_MODE_JOB)
    grids = np_paint(jobs, TILES, 32, 48)
    queries = np.array(queries, np.int64)
    want = np.zeros(len(queries), R.MVREF_RESULT)
    for t, tile in enumerate(TILES):
        sel = np.nonzero(queries[:, 0] == t)[0]
        want[sel] = oracle_results(grids[t], tile, FRAME, SIGN_BIAS, queries[sel, 1:])
    return jobs, grids, queries, want


def scene_features(queries, want, grids):
    """What the oracle alone shows on the scene"""
    f = set()
    for q, w in zip(queries, want):
        t, bx, by, bw4, bh4, r0, r1 = (int(v) for v in q)
        n = int(w["n"])
        st = w["stack"][:n]
        if n == 0:
            f.add("empty")
        if n >= 4:
            f.add("long")
        if (bw4, bh4) == (16, 16) and n:
            f.add("64x64")
        extra = n and (st["weight"] == 2).any()  # the scans' weights start at 4
        if extra and r1 != 8:
            f.add("compound extra")
        tile = TILES[t]
        if n:  # the same query far inside a huge frame: no clamp
            far = oracle_results(grids[t], (tile[0], tile[1], 4096, 4096), (16384, 16384), SIGN_BIAS,
                                 [(bx, by, bw4, bh4, r0, r1)])[0]
            if far["stack"].tobytes() != w["stack"].tobytes():
                f.add("clamp")
        if extra and r1 == 8:  # without sign biases no MV is flipped
            flat = oracle_results(grids[t], tile, FRAME, 0, [(bx, by, bw4, bh4, r0, r1)])[0]
            if flat["stack"].tobytes() != w["stack"].tobytes():
                f.add("sign flip")
    return f


FEATURES = {"empty", "long", "64x64", "clamp", "sign flip", "compound extra"}


# -------------------------------------------------------------------- CPU
def test_oracle_find_mvrefs_vs_rect_reference():
    kinds = set()
    nq = 0
    for grid, tile, frame, mask, query, entries in load_vectors("ref_mvref_rect.npz"):
        got = oracle_results(grid, tile, frame, mask, query[:, 1:7])
        for q, ent, g in zip(query, entries, got):
            case, bx, by, bw4, bh4, r0, r1, ctx, n = (int(v) for v in q)
            assert (int(g["mode_context"]), int(g["n"])) == (ctx, n), (case, bx, by, bw4, bh4, r0, r1)
            st = g["stack"][:n]
            np.testing.assert_array_equal(st["this_mv"], ent[:n, 0:2])
            np.testing.assert_array_equal(st["comp_mv"], ent[:n, 2:4])
            np.testing.assert_array_equal(st["weight"], ent[:n, 4])
            nq += 1
            if bw4 == 2 * bh4:
                kinds.add("2:1")
            if bh4 == 2 * bw4:
                kinds.add("1:2")
            # Block::default() is the only cell with ref_frames [INTRA_FRAME; 2]
            nb = [grid[by - 1, bx]] if by else []
            nb += [grid[by, bx - 1]] if bx else []
            if any(tuple(c["ref"]) == (0, 0) for c in nb):
                kinds.add("default cell")
            if r1 != 8 and (ent[:n, 4] == 2).any():  # the scans' weights start at 4
                kinds.add("compound extra")
    assert nq >= 200
    assert kinds == {"2:1", "1:2", "default cell", "compound extra"}


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_leaves_never_read_cells_coded_at_or_after_them(seed):
    """For the leaves of a final partition the stack on the fully painted grid
    is the stack on the grid as it was when the leaf was coded: one launch over
    a painted grid serves every block."""
    rng = np.random.default_rng(seed)
    sbw, sbh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    cols = sbw * 16 - 2 * int(rng.integers(0, 4))
    rows = sbh * 16 - 2 * int(rng.integers(0, 4))
    tile, frame = (cols, rows, 16, 32), (cols + 32, rows + 32)
    pool = [(int(rng.integers(-300, 301)), int(rng.integers(-300, 301))) for _ in range(3)]
    leaves = [it[1:] for it in partition(rng, cols, rows, p_split=0.55) if it[0] == "leaf"]
    jobs = np.array([rand_block_job(rng, pool, 0, *lf) for lf in leaves], R.EC_MODE_JOB)
    grid = np_paint(jobs, (tile,), sbh * 16, sbw * 16)[0]
    index = np.full(grid.shape, len(leaves), np.int64)  # cells no leaf covers: never coded
    for k, (x, y, w4, h4) in enumerate(leaves):
        index[y:min(y + h4, rows), x:min(x + w4, cols)] = k
    blank = default_grid(*grid.shape)
    mask = int(rng.integers(0, 128))
    n = 0
    for k, (x, y, w4, h4) in enumerate(leaves):
        before = np.where(index < k, grid, blank)
        q = [(x, y, w4, h4, r0, r1) for (r0, r1) in PAIRS]
        full, seen = (oracle_results(g, tile, frame, mask, q) for g in (grid, before))
        assert full.tobytes() == seen.tobytes(), (seed, k, x, y, w4, h4)
        n += 3
    assert n >= 30


def test_scene_shows_every_feature_on_the_oracle():
    jobs, grids, queries, want = scene()
    assert 200 <= len(queries) <= 900
    assert scene_features(queries, want, grids) == FEATURES
    sizes = {(int(q[3]), int(q[4])) for q in queries}
    assert {(16, 16), (2, 2), (4, 2), (2, 4)} <= sizes
    kinds = {(int(j["ref0"]) != 0, int(j["ref1"]) != 8) for j in jobs}
    assert kinds == {(False, False), (True, False), (True, True)}
    assert max(abs(int(jobs[f].max())) for f in ("mv0_row", "mv0_col")) > 200


def _geom(**kw):
    g = dict(n_tiles=2, grid_w=48, grid_h=32, frame_cols=92, frame_rows=58, sign_bias=SIGN_BIAS)
    g.update(kw)
    return R.RvMvrefGeom(**g)


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    L = R.lib()
    p = C.c_void_p(0x10000)  # never dereferenced: the checks come first
    bad_geoms = [_geom(n_tiles=0), _geom(n_tiles=1025), _geom(grid_w=40), _geom(grid_h=24),
                 _geom(grid_w=0), _geom(grid_h=8), _geom(frame_cols=0), _geom(sign_bias=128)]

    def paint(items=p, n=4, g=None, tiles=p, grid=p, scratch=p, status=p):
        return L.rv_mvref_grid_paint(items, n, g or _geom(), tiles, grid, scratch, status, None)

    def batch(items=p, n=4, g=None, tiles=p, grid=p, results=p, status=p):
        return L.rv_find_mvrefs_batch(items, n, g or _geom(), tiles, grid, results, status, None)

    def fill(items=p, n=4, g=None, tiles=p, grid=p, status=p):
        return L.rv_ec_mode_fill_stacks(items, n, g or _geom(), tiles, grid, None, status, None)

    for f, extra in ((paint, ("scratch",)), (batch, ("results",)), (fill, ())):
        assert f(n=0) == R.RV_OK
        assert f(n=0, items=None) == R.RV_OK
        assert f(n=-1) == R.RV_EINVAL
        assert b"bad arguments" in L.rv_last_error()
        for name in ("items", "tiles", "grid", "status") + extra:
            assert f(**{name: None}) == R.RV_EINVAL, (f.__name__, name)
        assert f(grid=C.c_void_p(0x10008)) == R.RV_EINVAL  # records are 16-byte aligned
        for g in bad_geoms:
            assert f(g=g) == R.RV_EINVAL, (f.__name__, g.n_tiles, g.grid_w, g.grid_h)
            assert f(g=g, n=0) == R.RV_EINVAL
    assert L.rv_mvref_paint_scratch_bytes(_geom()) == 2 * 48 * 32 * 4


def test_python_mirror_rejects_a_grid_smaller_than_a_tile():
    with pytest.raises(R.Rav1eHipError, match="holds every tile"):
        R.BlockGrid(TILES, grid_w=32, grid_h=32)
    with pytest.raises(R.Rav1eHipError, match="multiple of 16"):
        R.BlockGrid(TILES, grid_w=50, grid_h=32)
    with pytest.raises(R.Rav1eHipError, match="tiles"):
        R.BlockGrid(np.zeros((0, 4), np.int32))
    assert R.MV_BLK.itemsize == 16 and R.MV_CAND.itemsize == 12
    assert R.MVREF_QUERY.itemsize == 32 and R.MVREF_RESULT.itemsize == 116
    assert R.MV_BLK == O.BLK and R.MV_CAND == O.CAND


# -------------------------------------------------------------------- GPU
def assert_results_equal(got_ctx, got_n, got_st, want):
    np.testing.assert_array_equal(got_ctx, want["mode_context"])
    np.testing.assert_array_equal(got_n, want["n"])
    for f in ("this_mv", "comp_mv", "weight"):
        np.testing.assert_array_equal(got_st[f], want["stack"][f])


@pytest.mark.gpu
@pytest.mark.parametrize("name,count", [("ref_mvref.npz", 960), ("ref_mvref_rect.npz", 219)])
def test_device_find_mvrefs_equals_reference(name, count):
    R.require_device(0)
    nq = 0
    for cells, tile, frame, mask, query, entries in load_vectors(name):
        grid = R.BlockGrid.from_array(cells, [tile], frame_cols=frame[0], frame_rows=frame[1],
                                      sign_bias=mask)
        rows = np.concatenate([np.zeros((len(query), 1), np.int64), query[:, 1:7]], axis=1)
        ctx, n, st, rejected = R.find_mvrefs_batch(grid, rows)
        assert rejected == 0
        np.testing.assert_array_equal(ctx, query[:, 7])
        np.testing.assert_array_equal(n, query[:, 8])
        live = np.arange(9)[None, :] < query[:, 8:9]
        want = entries * live[:, :, None]  # the slots past the stack's length are zero
        np.testing.assert_array_equal(st["this_mv"], want[:, :, 0:2])
        np.testing.assert_array_equal(st["comp_mv"], want[:, :, 2:4])
        np.testing.assert_array_equal(st["weight"], want[:, :, 4])
        nq += len(query)
    assert nq == count


@pytest.mark.gpu
def test_device_whole_tiles_equal_oracle():
    R.require_device(0)
    jobs, grids, queries, want = scene()
    assert scene_features(queries, want, grids) == FEATURES
    grid = R.paint_block_grid(jobs, TILES, FRAME[0], FRAME[1], SIGN_BIAS)
    assert grid.rejected == 0 and grid.shape == grids.shape
    assert grid.download().tobytes() == grids.tobytes()
    ctx, n, st, rejected = R.find_mvrefs_batch(grid, queries)
    assert rejected == 0
    assert_results_equal(ctx, n, st, want)


@pytest.mark.gpu
def test_device_paint_equals_numpy_paint():
    R.require_device(0)
    rng = np.random.default_rng(21)
    pool = [(300, -300), (-7, 12)]
    rows = [(0, 0, 0, 4, 4), (0, 2, 2, 4, 4), (0, 2, 2, 2, 2),  # overlapping: the later job wins
            (0, 40, 24, 8, 8),        # clipped at the ragged right and bottom edge (44 x 30)
            (0, 16, 0, 16, 8), (0, 16, 8, 16, 8), (0, 32, 0, 4, 8),
            (1, 0, 0, 16, 16), (1, 44, 24, 4, 2), (1, 46, 24, 2, 4)]
    rows += [(1, 16 + 2 * (k % 8), 8 + 2 * (k // 8), 2, 2) for k in range(24)]
    rows += [(1, 16, 8, 8, 8)]  # over all of them
    jobs = np.array([rand_block_job(rng, pool, *r) for r in rows], R.EC_MODE_JOB)
    node = np.zeros(1, R.EC_MODE_JOB)
    node["kind"], node["bsize"], node["partition"] = 1, 12, 3  # a partition node paints nothing
    outside = jobs[:3].copy()
    outside["tile"] = (2, -1, 0)
    outside["bx"][2] = 44  # past tile 0's columns
    jobs = np.concatenate([jobs[:5], node, jobs[5:], outside])
    want = np_paint(jobs, TILES, 32, 48)
    grid = R.paint_block_grid(jobs, TILES, FRAME[0], FRAME[1], SIGN_BIAS)
    got = grid.download()
    assert grid.rejected == 3
    assert got.tobytes() == want.tobytes()
    assert (want["n4_w"] == 16).any() and tuple(want[0, 31, 47]["ref"]) == (0, 0)  # untouched cells
    assert want[0, 2, 2]["n4_w"] == 2 and want[0, 29, 43]["n4_w"] == 8
    # an empty job list is a grid of Block::default()
    empty = R.paint_block_grid(jobs[:0], TILES).download()
    assert empty.tobytes() == np_paint(jobs[:0], TILES, 32, 48).tobytes()


def _host_filled(jobs, grids, mask):
    """The four stack fields of every inter job from the oracle's stacks"""
    out = jobs.copy()
    stacks = np.zeros(len(jobs), R.MVREF_RESULT)
    for i, j in enumerate(jobs):
        if j["kind"] != 0 or j["luma_mode"] < 14:
            continue
        t = int(j["tile"])
        w4, h4 = N4_OF[int(j["bsize"])]
        r = oracle_results(grids[t], TILES[t], FRAME, mask,
                           [(j["bx"], j["by"], w4, h4, j["ref0"], j["ref1"])])[0]
        stacks[i] = r
        n = int(r["n"])
        out[i]["mode_context"], out[i]["num_mv_found"] = r["mode_context"], n
        for k in range(4):
            out[i]["weight%d" % k] = r["stack"][k]["weight"] if k < n else 0
        if n:
            (out[i]["ref_mv0_row"], out[i]["ref_mv0_col"]) = r["stack"][0]["this_mv"]
            (out[i]["ref_mv1_row"], out[i]["ref_mv1_col"]) = r["stack"][0]["comp_mv"]
    return out, stacks


STACK_FIELDS = ["mode_context", "num_mv_found", "weight0", "weight1", "weight2", "weight3",
                "ref_mv0_row", "ref_mv0_col", "ref_mv1_row", "ref_mv1_col"]


@functools.lru_cache(maxsize=None)
def token_scene():
    """The same tiles inside the tokenizer's limits (square blocks, NONE /
    SPLIT, compound blocks bidirectional), built in coding order: each block's
    mode is one its stack allows, and an MV that is not coded is the stack's.
    Returns (jobs with zeroed stack fields, the host-filled jobs, the grids)."""
    rng = np.random.default_rng(TOKEN_SEED)
    pool = [(int(rng.integers(-300, 301)), int(rng.integers(-300, 301))) for _ in range(4)]
    grids = np.stack([default_grid(32, 48) for _ in TILES])
    jobs = []
    for t, tile in enumerate(TILES):
        for it in partition(rng, tile[0], tile[1], rect=False, p_split=0.5):
            j = np.zeros(1, R.EC_MODE_JOB)[0]
            j["tile"], j["bx"], j["by"], j["ref1"] = t, it[1], it[2], 8
            if it[0] == "node":
                j["kind"], j["bsize"], j["partition"] = 1, BSIZE[(it[3], it[3])], it[4]
                jobs.append(j)
                continue
            _, x, y, w4, h4 = it
            j["bsize"], j["skip"] = BSIZE[(w4, h4)], rng.random() < 0.3
            r = rng.random()
            if r < 0.2:
                j["luma_mode"], j["chroma_mode"] = int(rng.integers(0, 13)), int(rng.integers(0, 13))
            else:
                comp = r < 0.5
                refs = (int(rng.integers(1, 3)), 5) if comp else (int(rng.choice([1, 2, 5])), 8)
                st = oracle_results(grids[t], tile, FRAME, SIGN_BIAS, [(x, y, w4, h4) + refs])[0]
                n, s = int(st["n"]), st["stack"]
                new = rand_mv(rng, pool)
                if comp:
                    mode = int(rng.choice([20, 22, 23, 26] + ([21, 27] if n >= 2 else [])))
                    mvs = {20: tuple(s[0]["this_mv"]) + tuple(s[0]["comp_mv"]),
                           21: tuple(s[1]["this_mv"]) + tuple(s[1]["comp_mv"]),
                           22: tuple(s[0]["this_mv"]) + new, 23: new + tuple(s[0]["comp_mv"]),
                           26: (0, 0, 0, 0), 27: new + rand_mv(rng, pool)}[mode]
                else:
                    mode = int(rng.choice([14, 15, 18, 19] + ([16] if n > 2 else [])))
                    near = lambda k: tuple(s[k]["this_mv"]) if n > 1 else (0, 0)  # noqa: E731
                    mvs = {14: tuple(s[0]["this_mv"]), 15: near(1), 16: near(2), 18: (0, 0),
                           19: new}[mode] + (0, 0)
                j["luma_mode"] = j["chroma_mode"] = mode
                j["ref0"], j["ref1"] = refs
                j["mv0_row"], j["mv0_col"], j["mv1_row"], j["mv1_col"] = (int(v) for v in mvs)
            jobs.append(j)
            one =np_paint(np.array([j], R.EC_MODE_JOB), TILES, 32, 48)[t]
            sel = np.zeros((32, 48), bool)
            sel[y:min(y + h4, tile[1]), x:min(x + w4, tile[0])] = True
            grids[t] = np.where(sel, one, grids[t])
    jobs = np.array(jobs, R.EC_MODE_JOB)
    filled, _ = _host_filled(jobs, grids, SIGN_BIAS)
    return jobs, filled, grids


def test_token_scene_is_what_the_reference_would_code():
    """Sequential construction and the painted grid agree (the visibility
    property), and the host-filled jobs pass the reference's assert!s."""
    jobs, filled, grids = token_scene()
    assert np_paint(jobs, TILES, 32, 48).tobytes() == grids.tobytes()
    R.check_mode_jobs(filled)
    inter = filled[(filled["kind"] == 0) & (filled["luma_mode"] >= 14)]
    assert len(inter) > 40 and (inter["num_mv_found"] == 0).any() and (inter["num_mv_found"] > 2).any()
    assert (inter["ref1"] != 8).any()


@pytest.mark.gpu
def test_device_fill_end_to_end():
    R.require_device(0)
    # the whole-tile scene (rectangular leaves too): the four fields and the stacks
    jobs, grids, _, _ = scene()
    want, want_stacks = _host_filled(jobs, grids, SIGN_BIAS)
    grid = R.paint_block_grid(jobs, TILES, FRAME[0], FRAME[1], SIGN_BIAS)
    info = {}
    filled, stack_mvs = R.ec_fill_mode_stacks(jobs, grid, info=info)
    assert info["rejected"] == 0
    assert filled.tobytes() == want.tobytes()
    assert info["stacks"].tobytes() == want_stacks.tobytes()
    np.testing.assert_array_equal(stack_mvs, want_stacks["stack"]["this_mv"][:, :4])
    intra = jobs["luma_mode"] < 14
    assert intra.any() and filled[intra].tobytes() == jobs[intra].tobytes()

    # inside the tokenizer's limits: the device-filled jobs tokenize like the host-filled ones
    tjobs, tfilled, tgrids = token_scene()
    tgrid = R.paint_block_grid(tjobs, TILES, FRAME[0], FRAME[1], SIGN_BIAS)
    assert tgrid.download().tobytes() == tgrids.tobytes()
    dfilled, dstack_mvs = R.ec_fill_mode_stacks(tjobs, tgrid)
    for f in STACK_FIELDS:
        np.testing.assert_array_equal(dfilled[f], tfilled[f], f)
    assert dfilled.tobytes() == tfilled.tobytes()
    prm = R.EcModeParams(R.FRAME_INTER, 1, 0, 0, 0, 0, [t[:2] for t in TILES])
    tok, off, bad = R.ec_tokenize_modes(dfilled, prm, dstack_mvs)
    wtok, woff, wbad = R.ec_tokenize_modes(tfilled, prm)
    assert (bad, wbad) == (0, 0) and len(tok) > len(tjobs)
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(tok, wtok)

    # candidates at one position against the committed grid, no repaint
    cands = np.zeros(5, R.EC_MODE_JOB)
    cands["tile"], cands["bx"], cands["by"], cands["ref1"] = 1, 16, 8, 8
    cands["bsize"] = (6, 6, 6, 9, 6)
    cands["luma_mode"] = (14, 19, 20, 19, 0)  # the last one intra: untouched
    cands["ref0"] = (1, 2, 1, 5, 0)
    cands["ref1"] = (8, 8, 5, 8, 8)
    cwant, _ = _host_filled(cands, tgrids, SIGN_BIAS)
    cfilled, _ = R.ec_fill_mode_stacks(cands, tgrid)
    assert cfilled.tobytes() == cwant.tobytes()
    assert cwant["num_mv_found"][:4].any()
    assert tgrid.download().tobytes() == tgrids.tobytes()


@pytest.mark.gpu
def test_device_rejected_queries_leave_their_slots():
    R.require_device(0)
    jobs, grids, _, _ = scene()
    grid = R.BlockGrid.from_array(grids, TILES, frame_cols=FRAME[0], frame_rows=FRAME[1],
                                  sign_bias=SIGN_BIAS)
    rows = [(0, 16, 16, 4, 4, 1, 8),     # fine
            (0, 16, 16, 1, 1, 1, 8),     # 4x4: not a supported size
            (0, 16, 16, 16, 4, 1, 8),    # 4:1
            (0, 44, 16, 4, 4, 1, 8),     # past the tile's 44 columns
            (1, 16, 28, 4, 4, 1, 8),     # past the tile's 26 rows
            (2, 0, 0, 4, 4, 1, 8),       # no such tile
            (0, 16, 16, 4, 4, 8, 8),     # NONE_FRAME as the first reference
            (0, 16, 16, 4, 4, 1, 9),     # no such RefType
            (0, 16, 16, 4, 4, -1, 8),
            (1, 16, 16, 8, 4, 1, 2)]     # fine
    mark = np.frombuffer(b"\x5a" * (R.MVREF_RESULT.itemsize * len(rows)), R.MVREF_RESULT)
    ctx, n, st, rejected = R.find_mvrefs_batch(grid, rows, results=mark)
    assert rejected == 8
    got = np.zeros(len(rows), R.MVREF_RESULT)
    got["mode_context"], got["n"], got["stack"] = ctx, n, st
    for i in range(1, 9):
        assert got[i].tobytes() == mark[i].tobytes(), i
    for i in (0, 9):
        t = rows[i][0]
        want = oracle_results(grids[t], TILES[t], FRAME, SIGN_BIAS, [rows[i][1:]])[0]
        assert got[i].tobytes() == want.tobytes(), i
    # the fill counts its rejected jobs and leaves them as they were
    bad = jobs[(jobs["luma_mode"] >= 14)][:3].copy()
    bad["bx"][0], bad["ref0"][1], bad["bsize"][2] = 46, 8, 0
    info = {}
    out, _ = R.ec_fill_mode_stacks(bad, grid, check=False, info=info)
    assert info["rejected"] == 3 and out.tobytes() == bad.tobytes()
    with pytest.raises(R.Rav1eHipError, match="3 inter jobs"):
        R.ec_fill_mode_stacks(bad, grid)

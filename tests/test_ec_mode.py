"""Block mode-info symbols (rav1e_amd/csrc/rv_ec_mode.hip, the mixed-stream
host coders of rv_ec.hip): the plain-Python restatement tests/ec_mode_ref.py
against vectors made by evaluating the reference's own ContextWriter /
BlockContext text (tools/refeval/gen_ec_mode_ref.py ->
tests/golden/ref_ec_mode.npz), the combined CDF table and the host coders
against the same vectors, and (-m gpu) the device tokenizer against the
restatement.  Every comparison is exact."""
import os
import re

import numpy as np
import pytest

import rav1e_amd as R
from tests import ec_mode_ref as M
from tests import ec_rate_ref as RR

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_ec_mode.npz")
F = M.F


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLD)


class Case:
    def __init__(self, g, row):
        (self.cid, self.j0, self.nj, self.o0, self.no, ft, rm, fi, hp, seg, la, self.t0, self.nt,
         self.q, self.lv0, self.nlv, self.coeffs) = (int(v) for v in row)
        self.dims = g["tile_dims"][self.t0:self.t0 + self.nt]
        self.args = (ft, rm, fi, hp, seg, la)
        self.prm = M.Params(ft, rm, fi, hp, seg, la, self.dims)
        self.rprm = R.EcModeParams(ft, rm, fi, hp, seg, la, self.dims)
        self.jobs = g["jobs"][self.j0:self.j0 + self.nj].astype(np.int64)
        self.stored = self.jobs.copy()  # seg_idx as the reference leaves it
        self.stored[:, F["seg_idx"]] = g["seg_stored"][self.j0:self.j0 + self.nj]
        self.ops = g["ops"][self.o0:self.o0 + self.no].astype(np.int64)
        self.init = g["init_cdf"][self.cid]
        self.lv = g["lv_jobs"][self.lv0:self.lv0 + self.nlv].astype(np.int64)

    def op_token(self, o):
        src, kind, a, ln, s, gather = (int(v) for v in o)
        if kind == 2:
            return 0x80000000 | a
        t = a | ln << 13 | s << 18
        if kind == 1:
            t |= gather << 23 | (M.BSIZE_LG[int(self.jobs[src, F["bsize"]])] - 3) << 25
        return t

    def tile_ops(self):
        """the ops of every tile, in stream order"""
        out = [[] for _ in range(self.nt)]
        t = 0
        for o in self.ops:
            if o[0] >= 0:
                t = int(self.jobs[o[0], F["tile"]])
            out[t].append(o)
        return out


def cases(g):
    return [Case(g, row) for row in g["cases"]]


# ------------------------------------------------------------------- CPU
def test_restatement_equals_reference_ops(ref):
    for c in cases(ref):
        got, bad, seg = M.tokenize(c.stored, c.prm)
        assert bad == 0
        for i in range(c.nj):
            want = [tuple(int(v) for v in o[2:6]) for o in c.ops[c.ops[:, 0] == i]]
            assert got[i] == want, (c.cid, i)


def test_skip_segments_resolve_to_what_the_reference_stores(ref):
    changed = 0
    for c in cases(ref):
        blk = c.jobs[:, F["kind"]] == 0
        _, _, seg = M.tokenize(c.jobs, c.prm)
        np.testing.assert_array_equal(seg[blk], c.stored[blk, F["seg_idx"]])
        got = R.resolve_skip_segments(R.ec_mode_jobs(c.jobs), c.rprm)
        np.testing.assert_array_equal(got["seg_idx"][blk], c.stored[blk, F["seg_idx"]])
        changed += int((c.jobs[blk, F["seg_idx"]] != c.stored[blk, F["seg_idx"]]).sum())
    assert changed > 0  # the vectors do exercise the rule
    # all in segment 0: the identity
    z = R.ec_mode_jobs(cases(ref)[0].jobs)
    z["seg_idx"] = 0
    np.testing.assert_array_equal(R.resolve_skip_segments(z, cases(ref)[0].rprm), z)


def test_layout_matches_the_generated_header():
    hdr = open(os.path.join(os.path.dirname(R.__file__), "csrc", "rv_ec_mode_tables.h")).read()
    for name, off in M.OFF.items():
        assert int(re.search(r"#define RV_ECM_%s (\d+)" % name, hdr).group(1)) == off, name
    assert M.EC_TOTAL == R.lib().rv_ec_cdf_total() == M.OFF["PARTITION"]
    assert M.EC_TOTAL_ALL == R.lib().rv_ec_cdf_total_all() <= 8191


def test_default_cdf_all(ref):
    for c in cases(ref):
        got = R.ec_default_cdf_all(c.q)
        np.testing.assert_array_equal(got, c.init)
        np.testing.assert_array_equal(got[:M.EC_TOTAL], R.ec_default_cdf(c.q))
    with pytest.raises(R.Rav1eHipError):
        R.ec_default_cdf_all(4)


def test_code_stream_bytes_and_final_cdfs(ref):
    by, tb, fin = ref["bytes"], ref["tile_bytes"], ref["final_cdf"]
    starts = np.concatenate([[0], np.cumsum(tb)])
    for c in cases(ref):
        for t, ops in enumerate(c.tile_ops()):
            tok = np.array([c.op_token(o) for o in ops], np.uint32)
            cdf = c.init.copy()
            got = R.ec_code_stream(tok, cdf)
            k = c.t0 + t
            np.testing.assert_array_equal(got, by[starts[k]:starts[k + 1]])
            np.testing.assert_array_equal(cdf, fin[k])


def test_count_stream_equals_counting_writer(ref):
    for c in cases(ref):
        for ops in c.tile_ops():
            tok = np.array([c.op_token(o) for o in ops], np.uint32)
            w, cdf = RR.Counter(), [int(v) for v in c.init]
            before = w.tell_frac()
            for src, kind, a, ln, s, gather in ops:
                if kind == 2:
                    w.bit(int(a))
                elif kind == 1:
                    w.symbol(int(s), M.gather_cdf(cdf[a:a + ln], int(gather)))
                else:
                    sl = cdf[a:a + ln]
                    w.symbol_with_update(int(s), sl)
                    cdf[a:a + ln] = sl
            want = (w.tell_frac() - before) & 0xFFFFFFFF
            c1 = c.init.copy()
            rate, _ = R.ec_count_stream(tok, c1)
            assert rate == want
            np.testing.assert_array_equal(c1, np.array(cdf, np.uint16))
            # counted in two pieces through the state
            c2, h = c.init.copy(), len(tok) // 2
            r1, st = R.ec_count_stream(tok[:h], c2)
            r2, _ = R.ec_count_stream(tok[h:], c2, st)
            assert r1 + r2 == want


def test_old_entry_points_reject_mode_tokens(ref):
    tok = np.array([M.OFF["SKIP"] | 3 << 13], np.uint32)
    with pytest.raises(R.Rav1eHipError):
        R.ec_code_tokens(tok, R.ec_default_cdf(0))
    with pytest.raises(R.Rav1eHipError):
        R.ec_count_tokens(tok, R.ec_default_cdf(0))
    # and the new ones a malformed edge token (a gather over an 8x8 slice, a non-partition CDF)
    for bad in (M.OFF["PARTITION"] | 5 << 13 | 1 << 23, M.OFF["KF_Y"] | 11 << 13 | 1 << 23,
                M.OFF["PARTITION"] | 11 << 13 | 3 << 23, (M.EC_TOTAL_ALL - 2) | 3 << 13):
        with pytest.raises(R.Rav1eHipError):
            R.ec_code_stream(np.array([bad], np.uint32), R.ec_default_cdf_all(0))
        with pytest.raises(R.Rav1eHipError):
            R.ec_count_stream(np.array([bad], np.uint32), R.ec_default_cdf_all(0))


def test_reset_counts_all(ref):
    """CDFContext::reset_counts: every counter a coded CDF slice adapts (its
    last entry) is cleared, nothing else moves."""
    for c in cases(ref)[:2] + cases(ref)[-1:]:
        fin = ref["final_cdf"][c.t0].copy()
        got = fin.copy()
        R.lib().rv_ec_reset_counts_all(got.ctypes.data)
        counters = {int(o[2] + o[3] - 1) for o in c.ops if o[1] == 0}
        assert any(fin[k] for k in counters)
        assert not any(got[k] for k in counters)
        moved = np.nonzero(got != fin)[0]
        assert set(moved.tolist()) <= counters


def _job(**kw):
    j = np.zeros(1, R.EC_MODE_JOB)
    j["bsize"], j["ref1"] = 6, 8
    for k, v in kw.items():
        j[k] = v
    return j


def test_python_preconditions_raise():
    P = R.PredictionMode
    inter = dict(ref0=1, mode_context=0)
    ok = _job(luma_mode=P.NEW_NEWMV, chroma_mode=P.NEW_NEWMV, ref0=1, ref1=5, num_mv_found=2)
    R.check_mode_jobs(ok)
    with pytest.raises(R.Rav1eHipError, match="NEW_NEWMV"):
        R.check_mode_jobs(_job(luma_mode=P.NEW_NEWMV, chroma_mode=P.NEW_NEWMV, ref0=1, ref1=5,
                               num_mv_found=1))
    with pytest.raises(R.Rav1eHipError, match="stack entry"):
        R.check_mode_jobs(_job(luma_mode=P.NEAR1MV, chroma_mode=P.NEAR1MV, num_mv_found=2, **inter))
    near = _job(luma_mode=P.NEAR0MV, chroma_mode=P.NEAR0MV, num_mv_found=2, mv0_row=8, mv0_col=-16,
                **inter)
    stack = np.zeros((1, 4, 2), np.int32)
    stack[0, 1] = (8, -16)
    R.check_mode_jobs(near, stack)
    stack[0, 1] = (8, -8)
    with pytest.raises(R.Rav1eHipError, match="not the stack's"):
        R.check_mode_jobs(near, stack)
    with pytest.raises(R.Rav1eHipError, match="not the stack's"):
        R.check_mode_jobs(_job(luma_mode=P.NEARESTMV, chroma_mode=P.NEARESTMV, num_mv_found=1,
                               mv0_row=8, ref_mv0_row=16, **inter))
    with pytest.raises(R.Rav1eHipError, match="below 8x8"):
        R.check_mode_jobs(_job(luma_mode=P.NEAREST_NEARESTMV, chroma_mode=P.NEAREST_NEARESTMV,
                               ref0=1, ref1=5, num_mv_found=2, bsize=1))


# ------------------------------------------------------------------- GPU
def _rand_block(rng, prm, lg):
    """A leaf's decision inside the tokenizer's restrictions."""
    j = np.zeros(M.NF, np.int64)
    j[F["bsize"]] = {3: 3, 4: 6, 5: 9, 6: 12}[lg]
    j[F["skip"]] = rng.random() < 0.3
    j[F["seg_idx"]] = rng.integers(0, prm.last_active_segid + 1) if prm.seg_enabled else 0
    if prm.frame_type == M.KEY or rng.random() < 0.25:
        lm, cm = int(rng.integers(0, 13)), int(rng.integers(0, 14))
        if lg == 6 and cm == 13:
            cm = 0
        j[F["luma_mode"]], j[F["chroma_mode"]], j[F["ref1"]] = lm, cm, 8
        if cm == 13:
            js = int(rng.integers(0, 8))
            j[F["cfl_joint_sign"]] = js
            j[F["cfl_scale_u"]] = rng.integers(1, 17) if (js + 1) // 3 else 0
            j[F["cfl_scale_v"]] = rng.integers(1, 17) if (js + 1) % 3 else 0
        return j
    comp = prm.reference_mode and rng.random() < 0.45
    lm = int(rng.integers(20, 28)) if comp else int(rng.integers(14, 20))
    j[F["luma_mode"]] = j[F["chroma_mode"]] = lm
    j[F["ref0"]] = rng.integers(1, 5) if comp else rng.integers(1, 8)
    j[F["ref1"]] = rng.integers(5, 8) if comp else 8
    nf = int(rng.integers(0, 6))
    if lm == M.NEW_NEWMV:
        nf = max(nf, 2)
    if M.has_near(lm) and lm != M.NEAR0MV:
        nf = max(nf, M.near_ref_mv_idx(lm) + 1)
    j[F["num_mv_found"]] = nf
    j[F["weight0"]:F["weight0"] + 4] = rng.integers(0, 1280, 4)
    j[F["mode_context"]] = int(rng.integers(0, 7)) | int(rng.integers(0, 2)) << 3 | \
        int(rng.integers(0, 6)) << 4
    rm = rng.integers(-512, 512, 4) if nf else np.zeros(4, np.int64)
    j[F["ref_mv0_row"]:F["ref_mv0_row"] + 4] = rm
    # differences of every magnitude class (log-uniform up to 2^14), zero components too
    d = (2 ** rng.uniform(0, 14, 4)).astype(np.int64) * rng.choice([-1, 1], 4) * (rng.random(4) < 0.8)
    coded = np.repeat([lm in (M.NEWMV, M.NEW_NEWMV, M.NEW_NEARESTMV),
                       lm in (M.NEW_NEWMV, M.NEAREST_NEWMV)], 2)
    j[F["mv0_row"]:F["mv0_row"] + 4] = rm + d * coded  # an MV that is not coded is the stack's
    return j


def _rand_jobs(rng, prm):
    """Coding-order jobs of every tile: a random quadtree down to 8x8, split
    where a block crosses the tile edge (encode_partition_topdown)."""
    jobs = []

    def tree(t, x, y, lg, cols, rows):
        if x >= cols or y >= rows:
            return
        n4 = 1 << (lg - 2)
        split = lg > 3 and (x + n4 > cols or y + n4 > rows or rng.random() < 0.55)
        node = np.zeros(M.NF, np.int64)
        node[[F["kind"], F["tile"], F["bx"], F["by"], F["bsize"], F["partition"]]] = (
            1, t, x, y, {3: 3, 4: 6, 5: 9, 6: 12}[lg], 3 if split else 0)
        jobs.append(node)
        if split:
            for dy in (0, n4 // 2):
                for dx in (0, n4 // 2):
                    tree(t, x + dx, y + dy, lg - 1, cols, rows)
        else:
            j = _rand_block(rng, prm, lg)
            j[[F["tile"], F["bx"], F["by"]]] = (t, x, y)
            jobs.append(j)
    for t, (cols, rows) in enumerate(prm.tile_dims):
        for sy in range(0, rows, 16):
            for sx in range(0, cols, 16):
                tree(t, sx, sy, 6, cols, rows)
    jobs = np.array(jobs, np.int64)
    _, _, seg = M.tokenize(jobs, prm)  # skip blocks' stored segment ids
    jobs[:, F["seg_idx"]] = seg
    return jobs


def _device(jobs, prm, check=True):
    rprm = R.EcModeParams(prm.frame_type, prm.reference_mode, prm.force_integer_mv,
                          prm.allow_high_precision_mv, prm.seg_enabled, prm.last_active_segid,
                          prm.tile_dims)
    return R.ec_tokenize_modes(R.ec_mode_jobs(jobs), rprm, check=check)


def _assert_device_equals_ref(jobs, prm, check=True):
    want_tok, want_off, want_bad = M.tokens(jobs, prm)
    tok, off, bad = _device(jobs, prm, check)
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(tok, want_tok)
    assert bad == want_bad
    return tok, off, bad


@pytest.mark.gpu
def test_device_tokens_equal_restatement_on_golden_tiles(ref):
    for c in cases(ref):
        tok, off, bad = _assert_device_equals_ref(c.stored, c.prm)
        assert bad == 0
        # and the reference's ops directly
        want = np.array([c.op_token(o) for o in c.ops if o[0] >= 0], np.uint32)
        np.testing.assert_array_equal(tok, want)


# two tiles of 2x2 superblocks; a frame edge cutting the last superblock both
# ways (136x104 luma); key and inter; SINGLE and not; the three MV precisions
FRESH = [
    dict(frame_type=1, reference_mode=1, tile_dims=((32, 32), (32, 32))),
    dict(frame_type=1, reference_mode=0, allow_high_precision_mv=1, tile_dims=((34, 26),)),
    dict(frame_type=1, reference_mode=1, force_integer_mv=1, seg_enabled=1, last_active_segid=2,
         tile_dims=((34, 26), (18, 32))),
    dict(frame_type=0, seg_enabled=1, last_active_segid=7, tile_dims=((34, 26), (32, 32))),
]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(FRESH)))
def test_device_tokens_equal_restatement_on_fresh_tiles(k):
    rng = np.random.default_rng(100 + k)
    prm = M.Params(**FRESH[k])
    jobs = _rand_jobs(rng, prm)
    tok, off, bad = _assert_device_equals_ref(jobs, prm)
    assert bad == 0 and len(tok) > len(jobs)
    if k == 0:  # a list of one job, and an empty one
        first = jobs[1:2].copy()  # the first leaf or node below the root
        _assert_device_equals_ref(jobs[:1], prm)
        _assert_device_equals_ref(first, prm)
        tok, off, bad = _device(jobs[:0], prm)
        assert len(tok) == 0 and off.tolist() == [0] and bad == 0


def _violations(jobs, prm):
    """(name, job) pairs, one per restriction, made from valid jobs of the list."""
    blk = jobs[jobs[:, F["kind"]] == 0]
    lm = blk[:, F["luma_mode"]]
    pick = lambda m: blk[np.nonzero(m)[0][0]].copy()
    any_b, node = blk[0], jobs[jobs[:, F["kind"]] == 1][0]
    intra, single, comp = pick(lm < 13), pick((lm >= 14) & (lm < 20)), pick(lm >= 20)
    out = []

    def add(name, base, **kw):
        j = base.copy()
        for f, v in kw.items():
            j[F[f]] = v
        out.append((name, j))
    add("4x4", any_b, bsize=0)
    add("8x16", any_b, bsize=4)
    add("128x128", any_b, bsize=15, bx=0, by=0)
    add("kind", any_b, kind=2)
    add("tile", any_b, tile=len(prm.tile_dims))
    add("tile negative", any_b, tile=-1)
    add("misaligned", any_b, bsize=12, bx=8, by=0)
    add("outside", any_b, bsize=3, bx=1 << 20, by=0)
    add("negative", any_b, bsize=3, bx=-2, by=0)
    add("PARTITION_HORZ", node, partition=1)
    add("PARTITION_VERT_4", node, partition=9)
    add("edge node not split", node, tile=0, bsize=6, bx=28, by=24, partition=0)  # rows end at 26
    add("skip 2", any_b, skip=2)
    add("segment past last_active", any_b, seg_idx=prm.last_active_segid + 1)
    add("luma UV_CFL", intra, luma_mode=13)
    add("luma 28", single, luma_mode=28, chroma_mode=28)
    add("luma negative", intra, luma_mode=-1)
    add("chroma 14", intra, chroma_mode=14)
    add("intra with a ref", intra, ref0=1)
    add("cfl on 64x64", intra, bsize=12, bx=0, by=0, chroma_mode=13, cfl_joint_sign=0, cfl_scale_v=1)
    add("cfl joint sign 8", intra, bsize=3, chroma_mode=13, cfl_joint_sign=8, cfl_scale_u=1,
        cfl_scale_v=1)
    add("cfl scale 17", intra, bsize=3, chroma_mode=13, cfl_joint_sign=7, cfl_scale_u=17,
        cfl_scale_v=1)
    add("chroma differs", single, chroma_mode=0)
    add("single ref 0", single, ref0=0)
    add("single ref 8", single, ref0=8)
    add("single with second ref", single, ref1=5)
    add("compound both forward", comp, ref1=2)
    add("compound backward first", comp, ref0=5)
    add("mode_context newmv 7", single, mode_context=7)
    add("mode_context refmv 6", single, mode_context=6 << 4)
    add("mode_context negative", single, mode_context=-1)
    add("num_mv_found 10", single, num_mv_found=10)
    add("NEW_NEWMV one entry", comp, luma_mode=27, chroma_mode=27, num_mv_found=1)
    add("NEAR2MV three entries", single, luma_mode=17, chroma_mode=17, num_mv_found=3)
    add("mv difference", single, luma_mode=19, chroma_mode=19, mv0_row=(1 << 14) + 1, ref_mv0_row=0)
    return out


@pytest.mark.gpu
def test_jobs_outside_the_restrictions_are_counted_and_emit_nothing():
    rng = np.random.default_rng(7)
    prm = M.Params(frame_type=1, reference_mode=1, seg_enabled=1, last_active_segid=3,
                   tile_dims=((34, 26), (32, 32)))
    jobs = _rand_jobs(rng, prm)
    tok0, off0, bad0 = _assert_device_equals_ref(jobs, prm)
    assert bad0 == 0
    bad_jobs = _violations(jobs, prm)
    for name, j in bad_jobs:
        assert not M.job_ok(j, prm), name
    # each alone ...
    for name, j in bad_jobs:
        tok, off, bad = _device(j[None], prm, check=False)
        assert (len(tok), off.tolist(), bad) == (0, [0, 0], 1), name
    # ... and all of them spread through the valid list
    at = np.sort(rng.integers(0, len(jobs) + 1, len(bad_jobs)))
    mixed = np.insert(jobs, at, np.array([j for _, j in bad_jobs]), axis=0)
    is_bad = np.ones(len(mixed), bool)
    is_bad[np.setdiff1d(np.arange(len(mixed)), at + np.arange(len(at)))] = False
    tok, off, bad = _assert_device_equals_ref(mixed, prm, check=False)
    assert bad == len(bad_jobs)
    np.testing.assert_array_equal(tok, tok0)
    n = np.diff(off.astype(np.int64))
    assert not n[is_bad].any()
    np.testing.assert_array_equal(n[~is_bad], np.diff(off0.astype(np.int64)))
    # the frame-level restrictions: inter blocks on a key frame, compound under SINGLE, tile
    # sizes that are odd or empty.  A rejected leaf stores no record, so its neighbours' contexts
    # are not the reference's: the counts (which no context changes) and the rejections are compared.
    def counts(p, want_bad):
        _, want_off, ref_bad = M.tokens(jobs, p)
        _, off, bad = _device(jobs, p, check=False)
        np.testing.assert_array_equal(off, want_off)
        assert bad == ref_bad == want_bad
    lm, blk = jobs[:, F["luma_mode"]], jobs[:, F["kind"]] == 0
    counts(M.Params(frame_type=0, tile_dims=prm.tile_dims), int((lm >= 14).sum()))
    counts(M.Params(frame_type=1, reference_mode=0, tile_dims=prm.tile_dims), int((lm >= 20).sum()))
    for dims in (((33, 26), (32, 32)), ((34, 0), (32, 32))):
        counts(M.Params(frame_type=1, reference_mode=1, tile_dims=dims),
               int((jobs[:, F["tile"]] == 0).sum()))


@pytest.mark.gpu
def test_code_tile_bytes_equal_reference(ref):
    c = [c for c in cases(ref) if c.coeffs][0]
    by, cdf, tok = R.code_tile(R.ec_mode_jobs(c.stored), c.lv[:, :10], ref["lv_coeffs"],
                               c.lv[:, 10], c.rprm, c.init)
    want = np.array([c.op_token(o) for o in c.ops], np.uint32)
    np.testing.assert_array_equal(tok, want)
    starts = np.concatenate([[0], np.cumsum(ref["tile_bytes"])])
    np.testing.assert_array_equal(by, ref["bytes"][starts[c.t0]:starts[c.t0 + 1]])
    np.testing.assert_array_equal(cdf, ref["final_cdf"][c.t0])

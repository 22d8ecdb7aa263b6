"""The coefficient bit counter (WriterBase<WriterCounter>, src/ec.rs): the
Python restatement tests/ec_rate_ref.py and the product's host counter
rv_ec_count_tokens against vectors made by evaluating the reference's own
text (tools/refeval/gen_ec_rate_ref.py -> tests/golden/ref_ec_rate.npz), and
(-m gpu) the device counter rv_ec_rate_batch against those vectors and
against the host counter.  Every comparison is exact."""
import os

import numpy as np
import pytest

from tests import ec_rate_ref as ER
from tests.test_ec_util import leaves, rand_coeffs

GOLD = os.path.join(os.path.dirname(__file__), "golden")
M32 = 0xFFFFFFFF
BAD = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLD, "ref_ec_rate.npz"))


@pytest.fixture(scope="module")
def ref_ec():
    return np.load(os.path.join(GOLD, "ref_ec.npz"))


def _streams(ref):
    """(q, ops, states) of every writer vector."""
    for o0, no, s0 in ref["wr_index"]:
        ops = ref["wr_ops"][o0:o0 + no]
        q = int(ops[ops[:, 0] == 0][0, 1])
        yield q, ops, ref["wr_state"][s0:s0 + no + 1]


# ------------------------------------------------------------------ CPU
def test_python_counter_matches_reference(ref):
    import rav1e_amd as R
    assert len(ref["wr_index"]) >= 24
    flushed = 0
    for q, ops, st in _streams(ref):
        assert len(ops) >= 300
        cdf = [int(v) for v in R.ec_default_cdf(q)]
        w = ER.Counter()
        got = [(w.rng, w.cnt, w.tell(), w.tell_frac())]
        for kind, a, b, c, d in ops.tolist():
            if kind == 0:
                assert a == q
                sub = cdf[b:b + c]
                w.symbol_with_update(d, sub)
                cdf[b:b + c] = sub
            elif kind == 2:
                w.bit(a)
            else:
                w.literal(a, b)
            got.append((w.rng, w.cnt, w.tell(), w.tell_frac()))
        np.testing.assert_array_equal(np.array(got, np.int64), st)
        flushed += w.bytes
    assert flushed > 24 * 50  # bytes were flushed: store's s >= 0 branches ran


def test_host_counter_matches_reference(ref):
    import rav1e_amd as R
    assert R.EC_BITRES == 3
    for si, (q, ops, st) in enumerate(_streams(ref)):
        tok, start = ER.ops_to_tokens(ops)
        tok = np.array(tok, np.uint32)
        tf = st[:, 3]
        cdf = R.ec_default_cdf(q)
        rate, state = R.ec_count_tokens(tok, cdf)
        assert rate == int(tf[-1] - tf[0])
        assert state[:2] == (int(st[-1, 0]), int(st[-1, 1]))
        assert (state[2] * 8 + state[1] + 10) == int(st[-1, 2])  # tell()
        coded = R.ec_default_cdf(q)
        R.ec_code_tokens(tok, coded)
        np.testing.assert_array_equal(cdf, coded)
        # split at op k: the second piece starts from the recorded (rng, cnt)
        # and the CDFs as adapted so far
        for k in (1, len(ops) // 3, (si * 37) % len(ops), len(ops) - 1):
            c2 = R.ec_default_cdf(q)
            r1, s1 = R.ec_count_tokens(tok[:start[k]], c2)
            assert r1 == int(tf[k] - tf[0])
            assert s1[:2] == (int(st[k, 0]), int(st[k, 1]))
            r2, s2 = R.ec_count_tokens(tok[start[k]:], c2, (int(st[k, 0]), int(st[k, 1]), 0))
            assert r2 == int(tf[-1] - tf[k])
            assert s2[:2] == state[:2] and s1[2] + s2[2] == state[2]
            np.testing.assert_array_equal(c2, coded)
            # the same through the in / out state
            c3 = R.ec_default_cdf(q)
            _, s3 = R.ec_count_tokens(tok[:start[k]], c3)
            r3, s3 = R.ec_count_tokens(tok[start[k]:], c3, s3)
            assert (r3, s3) == (r2, state)


def test_host_counter_empty_and_bad_tokens():
    import rav1e_amd as R
    total = R.ec_default_cdf(0).size
    cdf = R.ec_default_cdf(0)
    assert R.ec_count_tokens(np.zeros(0, np.uint32), cdf) == (0, (0x8000, -9, 0))
    good = 0 | 3 << 13 | 1 << 18
    for bad in ((total - 2) | 3 << 13,      # off + len > total
                8191 | 31 << 13,            # far outside
                5 | 1 << 13,                # len < 2
                5 | 0 << 13,
                5 | 3 << 13 | 2 << 18,      # s >= len - 1
                5 | 5 << 13 | 31 << 18):
        for toks in ([bad], [good, 0x80000001, bad, good]):
            with pytest.raises(R.Rav1eHipError, match=r"\(-1\).*bad token"):
                R.ec_count_tokens(np.array(toks, np.uint32), R.ec_default_cdf(0))
            with pytest.raises(R.Rav1eHipError, match=r"\(-1\).*bad token"):
                R.ec_code_tokens(np.array(toks, np.uint32), R.ec_default_cdf(0))
    with pytest.raises(R.Rav1eHipError, match=r"\(-1\).*bad state"):
        R.ec_count_tokens(np.array([good], np.uint32), cdf, (0x7FFF, -9, 0))


# ------------------------------------------------------------------ GPU
def _host_rates(R, tok, bounds, cdfs, group_cdf, init=None):
    """ec_count_tokens of tok[bounds[g]:bounds[g + 1]] from a copy of the
    group's snapshot."""
    out = []
    for g in range(len(bounds) - 1):
        c = np.array(cdfs[group_cdf[g]], np.uint16)
        st = None
        if init is not None:
            cnt = int(init[g]) >> 16
            st = (int(init[g]) & 0xFFFF, cnt - 0x10000 if cnt & 0x8000 else cnt, 0)
        out.append(R.ec_count_tokens(tok[int(bounds[g]):int(bounds[g + 1])], c, st)[0] & M32)
    return np.array(out, np.uint32)


@pytest.mark.gpu
def test_gpu_rates_match_reference_blocks(ref, ref_ec):
    """Every non-skip leaf of ref_ec.npz's five cases priced from both
    snapshots.  A call takes the case's job list twice (the copy's tiles get
    context maps of their own, so both copies tokenize alike) with the two
    snapshots alternating over the groups of each copy."""
    import rav1e_amd as R
    R.require_device()
    jobs_all, co = ref_ec["lv_jobs"], ref_ec["lv_coeffs"]
    init, fin = ref_ec["lv_init_cdf"], ref_ec["lv_final_cdf"]
    rows = ref["blk_groups"]
    t0 = 0
    for ci, (cid, j0, nj, xdec, ydec, q, ntiles) in enumerate(ref_ec["lv_cases"].tolist()):
        cdfs = np.stack([init[ci], fin[t0 + ntiles - 1]])
        t0 += ntiles
        assert not np.array_equal(cdfs[0], cdfs[1])
        grp = rows[rows[:, 0] == ci]
        want = {(int(f), int(s)): int(r) for _, f, n, s, r in grp}
        firsts = sorted({f for f, _ in want})
        assert len(want) == 2 * len(firsts) and len(firsts) > 20
        jobs = np.concatenate([jobs_all[j0:j0 + nj]] * 2)
        # a group runs from its leaf's first job to the next leaf's: the
        # skip / row / tile jobs it takes in have no tokens
        gf = np.array(firsts + [nj + f for f in firsts] + [2 * nj], np.int32)
        L = len(firsts)
        sid = np.array([i & 1 for i in range(L)] + [(i + 1) & 1 for i in range(L)], np.int32)
        exp = np.array([want[(int(f) % nj, int(s))] for f, s in zip(gf[:-1], sid)], np.uint32)
        rates, tok, off = R.coefficient_rates(jobs, co, gf, cdfs, int(xdec), int(ydec),
                                              group_cdf=sid)
        np.testing.assert_array_equal(rates, exp, err_msg=f"case {ci}")
        np.testing.assert_array_equal(tok[:off[nj]], tok[off[nj]:])
        # the call itself: no bad group, the snapshots untouched
        r2, bad, after = R.ec_rate_batch(tok, off, gf, cdfs, sid)
        assert bad == 0
        np.testing.assert_array_equal(r2, exp)
        np.testing.assert_array_equal(after, cdfs)


def _rand_jobs(rng, xdec, sbw, sbh, ntiles, scale):
    """A coding-order job list like tests/test_ec.py's: quadtree leaves 64..8
    in z-order, skip leaves, superblock rows, tiles, ragged edges."""
    vis_w4, vis_h4 = sbw * 16 - 2, sbh * 16 - 6
    jobs, co, nco = [], [], 0
    for _ in range(ntiles):
        jobs.append((3, 0, 0, 0, 0, 0, 0, 0, 0, 0))
        for sby in range(sbh):
            jobs.append((2, 0, 0, 0, 0, 0, 0, 0, 0, 0))
            for sbx in range(sbw):
                lv = []
                leaves(rng, sbx * 16, sby * 16, 6, 3, vis_w4, vis_h4, lv)
                for x4, y4, lg in lv:
                    if rng.random() < 0.3:
                        jobs.append((1, 0, x4, y4, 0, 0, 0, lg, lg, 0))
                        continue
                    intra = lg == 6 and rng.random() < 0.25
                    for p in range(3):
                        plg = lg - (xdec if p else 0)
                        tx, n_tx = min(plg - 2, 4), 1
                        if p and xdec == 0 and lg == 6:
                            tx, n_tx = 3, 4
                        cw = min(4 << tx, 32)
                        for t in range(n_tx):
                            bx = x4 + (t % 2) * 8 if n_tx == 4 else x4
                            by = y4 + (t // 2) * 8 if n_tx == 4 else y4
                            c = rand_coeffs(rng, cw, scale if p == 0 else scale / 2)
                            jobs.append((0, p, bx, by, tx, 0, 0 if intra else 1, plg, plg, nco))
                            co.append(c)
                            nco += len(c)
    return np.array(jobs, np.int64), np.concatenate(co).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("xdec,sbw,sbh,ntiles,scale", [
    (1, 3, 2, 1, 400.0), (1, 8, 2, 2, 0.3), (0, 4, 3, 2, 4.0)])
def test_gpu_rates_match_host_counter(xdec, sbw, sbh, ntiles, scale):
    """Tokenizer + device counter over groups of mixed size (random job
    boundaries: parts of a leaf, several leaves, jobs without tokens)
    against the host counter on the same tokens."""
    import rav1e_amd as R
    R.require_device()
    rng = np.random.default_rng(sbw * 11 + ntiles)
    jobs, co = _rand_jobs(rng, xdec, sbw, sbh, ntiles, scale)
    n = len(jobs)
    cdfs = np.stack([R.ec_default_cdf(0), R.ec_default_cdf(3)])
    _, tok, off = R.coefficient_rates(jobs, co, [0, n], cdfs, xdec, xdec)
    off = off.astype(np.int64)
    cut = set(np.nonzero(rng.random(n) < 0.35)[0].tolist()) | {0, n}
    b = e = 0
    if scale > 100:  # one long group: the jobs from b up to more than 1000 tokens
        b = n // 3
        e = int(np.searchsorted(off, off[b] + 1001))
        assert e <= n
        cut = {c for c in cut if not b < c < e} | {b, e}
    free = (np.arange(n) < b - 1) | (np.arange(n) > e)
    j1 = int(np.nonzero(free & (jobs[:, 0] == 0) & (np.diff(off) == 1))[0][0])  # a one-token block
    j0 = int(np.nonzero(free & (jobs[:, 0] != 0))[0][-1])  # a skip / row / tile job
    keep = {0, n, b, e, j1, j1 + 1, j0, j0 + 1}
    cut |= keep
    if (len(cut) - 1) % 4 == 0:
        cut.remove(min(cut - keep))
    gf = np.array(sorted(cut), np.int32)
    ng = len(gf) - 1
    ntok = np.diff(off[gf])
    assert ng % 4 != 0 and ng > 8
    assert np.any((ntok == 0) & (np.diff(gf) > 0)) and np.any(ntok == 1)
    if scale > 100:
        assert ntok.max() > 1000
        assert np.any(tok[off[b]:off[e]] >> 31)  # Golomb raw bits among them
    sid = rng.integers(0, 2, ng).astype(np.int32)
    rates, tok2, off2 = R.coefficient_rates(jobs, co, gf, cdfs, xdec, xdec, group_cdf=sid)
    np.testing.assert_array_equal(tok2, tok)
    np.testing.assert_array_equal(off2, off)
    want = _host_rates(R, tok, off[gf], cdfs, sid)
    np.testing.assert_array_equal(rates, want)
    assert np.all(rates[ntok == 0] == 0)
    # no group_cdf: every group from snapshot 0
    r0, _, _ = R.coefficient_rates(jobs, co, gf, cdfs, xdec, xdec)
    np.testing.assert_array_equal(r0, _host_rates(R, tok, off[gf], cdfs, np.zeros(ng, int)))


def _vector_tokens(ref, q):
    """The tokens of the writer vectors of q context q, end to end: valid
    symbols of the coefficient families and raw bits."""
    out = []
    for sq, ops, _ in _streams(ref):
        if sq == q:
            out += ER.ops_to_tokens(ops)[0]
    return np.array(out, np.uint32)


SIZES = [0, 1, 63, 64, 65, 0, 127, 128, 129, 2, 1200, 7, 64, 300, 1]


@pytest.mark.gpu
def test_gpu_group_sizes_around_the_token_load(ref):
    """A synthetic token array with the offsets given directly: groups of 0,
    1, 63, 64, 65, 127 .. 129 and 1200 tokens (the kernel loads 64 tokens at
    a time), a group count that is no multiple of the groups per block."""
    import rav1e_amd as R
    R.require_device()
    tok = _vector_tokens(ref, 1)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    assert off[-1] <= tok.size and len(SIZES) % 4 != 0
    cdfs = np.stack([R.ec_default_cdf(1), R.ec_default_cdf(2)])
    sid = np.arange(len(SIZES)) % 2
    gf = np.arange(len(SIZES) + 1)
    rates, bad, after = R.ec_rate_batch(tok, off, gf, cdfs, sid)
    assert bad == 0
    np.testing.assert_array_equal(rates, _host_rates(R, tok, off, cdfs, sid))
    np.testing.assert_array_equal(after, cdfs)
    assert rates[0] == 0 and rates[5] == 0 and rates[10] > 1200
    # groups of several "jobs": group_first strides over the offsets
    gf2 = np.array([0, 3, 4, 9, len(SIZES)])
    r2, bad, _ = R.ec_rate_batch(tok, off, gf2, cdfs, sid[:4])
    assert bad == 0
    np.testing.assert_array_equal(r2, _host_rates(R, tok, off[gf2], cdfs, sid[:4]))


@pytest.mark.gpu
def test_gpu_init_state_matches_reference_and_host(ref):
    """d_init: every writer vector from its op k on, from the recorded (rng,
    cnt) at k and the CDFs as adapted to k (one snapshot per group); the
    rate is the recorded tell_frac difference."""
    import rav1e_amd as R
    R.require_device()
    toks, off, cdfs, init, want = [], [0], [], [], []
    for si, (q, ops, st) in enumerate(_streams(ref)):
        tok, start = ER.ops_to_tokens(ops)
        k = (si * 53 + 7) % len(ops)
        c = R.ec_default_cdf(q)
        R.ec_count_tokens(np.array(tok[:start[k]], np.uint32), c)
        cdfs.append(c)
        toks += tok[start[k]:]
        off.append(len(toks))
        init.append(int(st[k, 0]) | (int(st[k, 1]) & 0xFFFF) << 16)
        want.append(int(st[-1, 3] - st[k, 3]))
    assert any(w >> 31 for w in init)  # negative cnt among them
    tok, off, cdfs = np.array(toks, np.uint32), np.array(off, np.uint32), np.stack(cdfs)
    ng = len(want)
    sid = np.arange(ng)
    rates, bad, _ = R.ec_rate_batch(tok, off, np.arange(ng + 1), cdfs, sid, init)
    assert bad == 0
    np.testing.assert_array_equal(rates, np.array(want, np.uint32))
    np.testing.assert_array_equal(rates, _host_rates(R, tok, off, cdfs, sid, init))


@pytest.mark.gpu
def test_gpu_bad_token_and_bad_snapshot_stop_their_group_only(ref):
    """Input validation: one malformed token in one group, or a snapshot
    index outside [0, n_cdfs).  The kernel tests a token before it uses its
    offset and an index before it scales it, so such a group indexes
    nothing: it reads 0xFFFFFFFF, d_status[0] counts it, and every other
    group's rate is exact."""
    import rav1e_amd as R
    R.require_device()
    tok = _vector_tokens(ref, 2)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    ng = len(SIZES)
    cdfs = np.stack([R.ec_default_cdf(2), R.ec_default_cdf(0)])
    sid = (np.arange(ng) // 2) % 2
    gf = np.arange(ng + 1)
    good = _host_rates(R, tok, off, cdfs, sid)
    total = cdfs.shape[1]
    for g, at, bad_tok in ((10, 1100, (total - 2) | 3 << 13),   # off + len > total, deep in
                           (10, 0, 8191 | 31 << 13 | 29 << 18),
                           (3, 63, 5 | 1 << 13),                # len < 2, last of a load
                           (4, 64, 5 | 3 << 13 | 2 << 18),      # s >= len - 1, first of the next
                           (1, 0, 0x7FFFFFFF)):
        t = tok.copy()
        t[off[g] + at] = bad_tok
        rates, bad, after = R.ec_rate_batch(t, off, gf, cdfs, sid)
        assert bad == 1
        assert rates[g] == BAD
        keep = np.arange(ng) != g
        np.testing.assert_array_equal(rates[keep], good[keep])
        np.testing.assert_array_equal(after, cdfs)
    s2 = sid.copy()
    s2[[2, 6, 11]] = (2, -1, 0x7FFFFFFF)
    rates, bad, _ = R.ec_rate_batch(tok, off, gf, cdfs, s2)
    assert bad == 3
    keep = ~np.isin(np.arange(ng), [2, 6, 11])
    assert np.all(rates[~keep] == BAD)
    np.testing.assert_array_equal(rates[keep], good[keep])

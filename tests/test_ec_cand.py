"""Whole RDO candidates priced on the device (rv_ec_rate.hip's mixed-stream
counter rv_ec_rate_stream_batch, rv_ec_cand.hip's candidate tokenizer and the
fused rv_ec_cand_rates): what luma_chroma_mode_rdo (src/rdo.rs:689-768) takes
as a candidate's rate.  The ground truth is the pinned pieces composed on the
host: the golden streams of tests/golden/ref_ec_mode.npz, ec_tokenize_modes
and the coefficient tokenizer over whole tiles, tests/ec_mode_ref.py and the
host counter ec_count_stream.  Every comparison is exact."""
import os

import numpy as np
import pytest

import rav1e_amd as R
from tests import ec_mode_ref as M
from tests import ec_rate_ref as ER
from tests import test_ec_mode as TM
from tests.test_ec_util import rand_coeffs

GOLD = os.path.join(os.path.dirname(__file__), "golden")
F = M.F
M32 = 0xFFFFFFFF
BAD = 0xFFFFFFFF
TOTAL, TOTAL_ALL = M.EC_TOTAL, M.EC_TOTAL_ALL


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLD, "ref_ec_mode.npz"))


@pytest.fixture(scope="module")
def ref_rate():
    return np.load(os.path.join(GOLD, "ref_ec_rate.npz"))


def _pack_state(st):
    return (int(st[0]) | (int(st[1]) & 0xFFFF) << 16)


def _unpack_state(w):
    cnt = int(w) >> 16
    return (int(w) & 0xFFFF, cnt - 0x10000 if cnt & 0x8000 else cnt, 0)


def _host_stream_rates(tok, bounds, cdfs, group_cdf, init=None):
    """ec_count_stream of tok[bounds[g]:bounds[g + 1]] from a copy of the group's snapshot"""
    out = []
    for g in range(len(bounds) - 1):
        c = np.array(cdfs[group_cdf[g]], np.uint16)
        st = None if init is None else _unpack_state(init[g])
        out.append(R.ec_count_stream(tok[int(bounds[g]):int(bounds[g + 1])], c, st)[0] & M32)
    return np.array(out, np.uint32)


def _golden_tile_streams(ref):
    """(case, tile tokens, group bounds) of every golden tile: one group per
    block, from the first op of the partition nodes ahead of it to the last
    coefficient op behind it."""
    for c in TM.cases(ref):
        for ops in c.tile_ops():
            tok = np.array([c.op_token(o) for o in ops], np.uint32)
            cuts, last = [0], -1
            for k, o in enumerate(ops):
                src = int(o[0])
                if src >= 0 and src != last:
                    if last >= 0 and c.jobs[last, F["kind"]] == 0:
                        cuts.append(k)
                    last = src
            cuts.append(len(ops))
            yield c, tok, np.array(sorted(set(cuts)), np.int64)


# ------------------------------------------------------------------- CPU
def test_new_exports_exist_with_the_declared_argument_counts():
    L = R.lib()
    names = R.exported_symbols_from_header()
    for name, nargs in (("rv_ec_rate_stream_batch", 11), ("rv_ec_rate_stream_batch_waves", 12),
                        ("rv_ec_cand_scratch_bytes", 2), ("rv_ec_cand_tokenize", 23),
                        ("rv_ec_cand_rates", 28), ("rv_ec_partition_gather", 2)):
        assert name in names
        assert len(getattr(L, name).argtypes) == nargs, name
    # the header's own parameter lists
    hdr = open(R.HEADER_PATH).read()
    for name, nargs in (("rv_ec_rate_stream_batch", 11), ("rv_ec_cand_tokenize", 23),
                        ("rv_ec_cand_rates", 28)):
        decl = hdr[hdr.index("int %s(" % name):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs, name
    assert R.EC_CAND.itemsize == 16
    assert L.rv_ec_cand_scratch_bytes(0, 0) > 0
    assert L.rv_ec_cand_scratch_bytes(1000, 5000) >= 4 * 1001 + 17 * 5000


def _block(**kw):
    j = np.zeros(1, R.EC_MODE_JOB)
    j["bsize"], j["ref1"] = 6, 8
    for k, v in kw.items():
        j[k] = v
    return j[0]


def test_python_preconditions_raise():
    blk = _block(bx=4, by=8)
    tx = [(0, 0, 4, 8, 2, 0, 0, 4, 4, 0)]
    cdfs = R.ec_default_cdf_all(0)
    R.pack_candidates([(None, blk, tx)])
    with pytest.raises(R.Rav1eHipError, match="no block"):
        R.pack_candidates([(None, None, tx)])
    with pytest.raises(R.Rav1eHipError, match="no block"):
        R.pack_candidates([(None, _block(kind=1), [])])
    for bad in ((0, 0, 8, 8, 2, 0, 0, 4, 4, 0),      # right of the block
                (0, 0, 4, 4, 2, 0, 0, 4, 4, 0),      # above it
                (1, 0, 4, 8, 2, 0, 0, 4, 4, 0)):     # no transform block
        with pytest.raises(R.Rav1eHipError, match="outside the block"):
            R.pack_candidates([(None, blk, [tx[0], bad])])
    P = R.PredictionMode
    with pytest.raises(R.Rav1eHipError, match="NEW_NEWMV"):
        R.pack_candidates([(None, _block(luma_mode=P.NEW_NEWMV, chroma_mode=P.NEW_NEWMV, ref0=1,
                                         ref1=5, num_mv_found=1), [])])
    prm = R.EcModeParams(tile_dims=((32, 32),))
    args = (np.zeros(0, R.EC_MODE_JOB), np.zeros((0, 10), np.int64), np.zeros(256, np.int32))
    with pytest.raises(R.Rav1eHipError, match="one entry per group"):
        R.candidate_rates(*args, [(None, blk, tx)], prm, cdfs, group_cdf=[0, 0])
    with pytest.raises(R.Rav1eHipError, match="one entry per group"):
        R.candidate_rates(*args, [(None, blk, tx)], prm, cdfs, init=[])
    with pytest.raises(R.Rav1eHipError, match="u16 wide"):
        R.candidate_rates(*args, [(None, blk, tx)], prm, R.ec_default_cdf(0))
    with pytest.raises(R.Rav1eHipError, match="no block"):
        R.candidate_rates(*args, [(None, None, tx)], prm, cdfs)
    tok, off = np.zeros(4, np.uint32), np.array([0, 4], np.uint32)
    with pytest.raises(R.Rav1eHipError, match="u16 wide"):
        R.ec_rate_stream_batch(tok, off, [0, 1], R.ec_default_cdf(0))
    with pytest.raises(R.Rav1eHipError, match="u16 wide"):
        R.ec_rate_stream_batch(tok, off, [0, 1], np.zeros((2, TOTAL_ALL + 1), np.uint16))
    with pytest.raises(R.Rav1eHipError, match="one entry per group"):
        R.ec_rate_stream_batch(tok, off, [0, 1], cdfs, group_cdf=[0, 0])
    with pytest.raises(R.Rav1eHipError, match="waves"):
        R.ec_rate_stream_batch(tok, off, [0, 1], cdfs, waves=3)


def test_shared_gather_equals_the_restatement():
    n = 0
    for q in range(4):
        cdf = R.ec_default_cdf_all(q)
        for i in range(20):
            part = cdf[M.OFF["PARTITION"] + 11 * i:M.OFF["PARTITION"] + 11 * (i + 1)]
            for gather in (1, 2):
                assert R.ec_partition_gather(part, gather) == M.gather_cdf(part, gather)[0]
                n += 1
    assert n == 160
    # an adapted CDF, and wrap-around arithmetic on an arbitrary one
    rng = np.random.default_rng(3)
    for _ in range(50):
        part = np.sort(rng.integers(0, 32768, 10))[::-1].astype(np.uint16)
        for gather in (1, 2):
            assert R.ec_partition_gather(part, gather) == M.gather_cdf(part, gather)[0]
    with pytest.raises(R.Rav1eHipError):
        R.ec_partition_gather(np.zeros(11, np.uint16), 3)
    with pytest.raises(R.Rav1eHipError):
        R.ec_partition_gather(np.zeros(11, np.uint16), 0)


# ------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_mixed_counter_equals_host_counter_on_golden_tiles(ref):
    """One group per block of every golden tile, the snapshot of group g being
    the CDFs after the groups before it and its init the writer state there:
    rates, and with them the chained states, equal the host's word for word."""
    R.require_device()
    toks, bounds, cdfs, init, want = [], [0], [], [], []
    kinds, gathers, interleaved = set(), set(), False
    for c, tok, cuts in _golden_tile_streams(ref):
        interleaved |= bool(c.coeffs)
        kinds |= {"raw" if t >> 31 else "edge" if (t >> 23) & 3 else "sym" for t in tok.tolist()}
        gathers |= {(t >> 23) & 3 for t in tok.tolist() if not t >> 31}
        cdf, st = c.init.copy(), (0x8000, -9, 0)
        whole, _ = R.ec_count_stream(tok, c.init.copy())
        total = 0
        for g in range(len(cuts) - 1):
            cdfs.append(cdf.copy())
            init.append(_pack_state(st))
            rate, st = R.ec_count_stream(tok[cuts[g]:cuts[g + 1]], cdf, st)
            want.append(rate & M32)
            total += rate
        assert total == whole  # the chain is the tile's count
        toks.append(tok)
        bounds += (bounds[-1] + cuts[1:]).tolist()
    assert kinds == {"sym", "raw", "edge"} and gathers == {0, 1, 2} and interleaved
    tok = np.concatenate(toks)
    ng = len(want)
    assert ng > 300
    rates, bad, after = R.ec_rate_stream_batch(tok, np.array(bounds, np.uint32), np.arange(ng + 1),
                                               np.stack(cdfs), np.arange(ng), np.array(init, np.uint32))
    assert bad == 0
    np.testing.assert_array_equal(rates, np.array(want, np.uint32))
    np.testing.assert_array_equal(after, np.stack(cdfs))


@pytest.mark.gpu
def test_code_tile_stream_is_the_golden_interleaved_stream(ref):
    """The interleaved golden case through code_tile gives the stream the
    counter test cuts up (the other cases carry mode tokens only)."""
    R.require_device()
    c = [c for c in TM.cases(ref) if c.coeffs][0]
    _, _, tok = R.code_tile(R.ec_mode_jobs(c.stored), c.lv[:, :10], ref["lv_coeffs"], c.lv[:, 10],
                            c.rprm, c.init)
    (_, want, _), = [s for s in _golden_tile_streams(ref) if s[0].coeffs]
    np.testing.assert_array_equal(tok, want)


SIZES = [0, 1, 63, 64, 65, 128, 65, 0, 129, 7, 300]


def _vector_tokens(ref_rate, q):
    out = []
    for o0, no, s0 in ref_rate["wr_index"]:
        ops = ref_rate["wr_ops"][o0:o0 + no]
        if int(ops[ops[:, 0] == 0][0, 1]) == q:
            out += ER.ops_to_tokens(ops)[0]
    return np.array(out, np.uint32)


@pytest.mark.gpu
def test_coefficient_only_streams_equal_the_coefficient_counter(ref_rate):
    R.require_device()
    tok = _vector_tokens(ref_rate, 1)
    off = np.concatenate([[0], np.cumsum(SIZES + [1200])]).astype(np.uint32)
    ng = len(off) - 1
    assert off[-1] <= tok.size
    allc = np.stack([R.ec_default_cdf_all(1), R.ec_default_cdf_all(2), R.ec_default_cdf_all(0)])
    sid = np.arange(ng) % 3
    init = np.array([0x8000 | (0xFFF7 << 16)] * ng, np.uint32)
    init[1::2] = 0xC123 | (3 << 16)
    for ini in (None, init):
        r_old, bad_old, _ = R.ec_rate_batch(tok, off, np.arange(ng + 1), allc[:, :TOTAL], sid, ini)
        r_new, bad_new, after = R.ec_rate_stream_batch(tok, off, np.arange(ng + 1), allc, sid, ini)
        assert bad_old == 0 and bad_new == 0
        np.testing.assert_array_equal(r_new, r_old)
        np.testing.assert_array_equal(after, allc)
    assert r_old[0] == 0 and r_old[-1] > 1200


@pytest.mark.gpu
def test_token_loads_and_slice_phases(ref):
    """Groups of 0, 1, 63, 64, 65 and 128 tokens (64 tokens per load), an edge
    token as the last token of one load and the first of the next, eight
    snapshots (a snapshot is 11 908 B: every 4-byte phase of the 16-byte unit
    occurs) and the snapshot table displaced by one u16 (the odd phases)."""
    R.require_device()
    tok = np.concatenate([t for _, t, _ in _golden_tile_streams(ref)])
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    assert off[-1] <= tok.size
    tok = tok[:off[-1]].copy()
    P = M.OFF["PARTITION"]
    edge = lambda ctx, s, gather, bsl: P + 11 * ctx | 11 << 13 | s << 18 | gather << 23 | bsl << 25
    g65 = [g for g, n in enumerate(SIZES) if n == 65]
    tok[off[g65[0]] + 63] = edge(5, 1, 1, 1)   # the last token of the first load
    tok[off[g65[0]] + 64] = edge(9, 0, 2, 2)   # the first of the next
    tok[off[g65[1]] + 63] = edge(14, 0, 1, 3)
    tok[off[g65[1]] + 64] = edge(6, 1, 2, 1)
    tok[off[SIZES.index(128)] + 64] = edge(12, 1, 2, 3)
    tok[off[SIZES.index(1)]] = edge(4, 1, 1, 1)  # a group that is one edge token
    ng = len(SIZES)
    cdfs = np.stack([R.ec_default_cdf_all(k % 4) for k in range(8)])
    for k in range(8):  # adapted tables: the gathers see CDFs that moved
        R.ec_count_stream(tok[:200 * k], cdfs[k])
    sid = (np.arange(ng) * 3) % 8
    assert set(sid.tolist()) == set(range(8))
    want = _host_stream_rates(tok, off, cdfs, sid)
    assert want[0] == 0 and len(set(want.tolist())) > 6
    for phase in (0, 1):
        for waves in (None, 1, 2, 4):
            rates, bad, after = R.ec_rate_stream_batch(tok, off.astype(np.uint32),
                                                       np.arange(ng + 1), cdfs, sid, None, waves,
                                                       cdf_phase=phase)
            assert bad == 0
            np.testing.assert_array_equal(rates, want, err_msg=f"phase {phase} waves {waves}")
            np.testing.assert_array_equal(after, cdfs)
    # groups of several pieces: group_first strides over the offsets
    gf = np.array([0, 3, 4, 9, ng])
    rates, bad, _ = R.ec_rate_stream_batch(tok, off.astype(np.uint32), gf, cdfs, sid[:4])
    assert bad == 0
    np.testing.assert_array_equal(rates, _host_stream_rates(tok, off[gf], cdfs, sid[:4]))


@pytest.mark.gpu
def test_bad_inputs_stop_their_own_group_only(ref):
    R.require_device()
    tok = np.concatenate([t for _, t, _ in _golden_tile_streams(ref)])
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    tok = tok[:off[-1]].copy()
    ng = len(SIZES)
    cdfs = np.stack([R.ec_default_cdf_all(2), R.ec_default_cdf_all(0)])
    sid = (np.arange(ng) // 2) % 2
    good = _host_stream_rates(tok, off, cdfs, sid)
    P = M.OFF["PARTITION"]
    cases = ((10, 250, (TOTAL_ALL - 2) | 3 << 13),            # off + len > the combined total
             (10, 0, 8191 | 31 << 13 | 29 << 18),
             (2, 62, 5 | 1 << 13),                            # len < 2
             (4, 64, 5 | 3 << 13 | 2 << 18),                  # s >= len - 1, first of a load
             (5, 63, P | 11 << 13 | 3 << 23),                 # gather field 3, last of a load
             (5, 64, M.OFF["KF_Y"] | 11 << 13 | 1 << 23),     # a gather over no partition CDF
             (8, 128, (P + 3) | 11 << 13 | 2 << 23),          # ... over a misaligned one
             (3, 1, P | 5 << 13 | 1 << 23),                   # ... over an 8x8 slice
             (1, 0, P | 11 << 13 | 2 << 18 | 1 << 23))        # an edge symbol above 1
    for g, at, bad_tok in cases:
        t = tok.copy()
        t[off[g] + at] = bad_tok
        with pytest.raises(R.Rav1eHipError):  # the host refuses the same token
            R.ec_count_stream(t[off[g]:off[g + 1]], cdfs[sid[g]].copy())
        rates, bad, after = R.ec_rate_stream_batch(t, off.astype(np.uint32), np.arange(ng + 1),
                                                   cdfs, sid)
        assert bad == 1, hex(bad_tok)
        assert rates[g] == BAD
        keep = np.arange(ng) != g
        np.testing.assert_array_equal(rates[keep], good[keep])
        np.testing.assert_array_equal(after, cdfs)
    s2 = sid.copy()
    s2[[2, 6, 9]] = (-1, len(cdfs), 0x7FFFFFFF)
    rates, bad, _ = R.ec_rate_stream_batch(tok, off.astype(np.uint32), np.arange(ng + 1), cdfs, s2)
    assert bad == 3
    keep = ~np.isin(np.arange(ng), [2, 6, 9])
    assert np.all(rates[~keep] == BAD)
    np.testing.assert_array_equal(rates[keep], good[keep])


# ---- candidates -------------------------------------------------------------
class Tile:
    """Random tiles in both job formats: test_ec_mode's quadtree of mode jobs
    (every leaf behind its PARTITION_NONE node) and, per leaf, the coefficient
    rows code_coefficients takes (a skip leaf's reset row; kind 2 / 3 rows at
    superblock-row and tile starts), with where each leaf's rows are."""

    def __init__(self, seed, prm_kw, xdec, scale=6.0):
        self.rng = rng = np.random.default_rng(seed)
        self.prm, self.xdec = M.Params(**prm_kw), xdec
        self.rprm = R.EcModeParams(**prm_kw)
        self.mode = TM._rand_jobs(rng, self.prm)
        self.co, self.nco = [], 0
        rows, self.span = [], {}
        tile, sbrow = -1, -1
        for i, j in enumerate(self.mode):
            if j[F["kind"]] != 0:
                continue
            if j[F["tile"]] != tile:
                tile, sbrow = int(j[F["tile"]]), -1
                rows.append((3, 0, 0, 0, 0, 0, 0, 0, 0, 0))
            if j[F["by"]] >> 4 != sbrow:
                sbrow = int(j[F["by"]]) >> 4
                rows.append((2, 0, 0, 0, 0, 0, 0, 0, 0, 0))
            mine = self.block_rows(j, scale)
            self.span[i] = (len(rows), len(rows) + len(mine))
            rows += mine
        self.rows = np.array(rows, np.int64)
        self.blocks = sorted(self.span)

    def coeffs(self):
        return np.concatenate(self.co).astype(np.int32)

    def tx_row(self, p, bx, by, tx, inter, plg, scale):
        cw = min(4 << tx, 32)
        c = rand_coeffs(self.rng, cw, scale if p == 0 else scale / 2)
        self.co.append(c)
        self.nco += len(c)
        return (0, p, bx, by, tx, 0, inter, plg, plg, self.nco - len(c))

    def block_rows(self, j, scale, split_luma=False):
        """The coefficient rows of mode job j: luma (one transform, or four of
        the next size down) then chroma, write_tx_blocks' order."""
        lg = M.BSIZE_LG[int(j[F["bsize"]])]
        x4, y4 = int(j[F["bx"]]), int(j[F["by"]])
        if j[F["skip"]]:
            return [(1, 0, x4, y4, 0, 0, 0, lg, lg, 0)]
        inter = int(j[F["luma_mode"]] >= M.NEARESTMV)
        out = []
        if split_luma:
            tx, h = lg - 3, 1 << (lg - 3)
            for dy in (0, h):
                for dx in (0, h):
                    out.append(self.tx_row(0, x4 + dx, y4 + dy, tx, inter, lg, scale))
        else:
            out.append(self.tx_row(0, x4, y4, min(lg - 2, 4), inter, lg, scale))
        plg = lg - self.xdec
        for p in (1, 2):
            if plg == 6:
                for t in range(4):
                    out.append(self.tx_row(p, x4 + (t % 2) * 8, y4 + (t // 2) * 8, 3, inter, plg, scale))
            else:
                out.append(self.tx_row(p, x4, y4, plg - 2, inter, plg, scale))
        return out

    def tokenize(self, mode=None, rows=None):
        """The existing entry points over the whole tile list: (mode tokens,
        their offsets, coefficient tokens, their offsets)."""
        mode = self.mode if mode is None else mode
        rows = self.rows if rows is None else rows
        mtok, moff, bad = R.ec_tokenize_modes(R.ec_mode_jobs(mode), self.rprm)
        assert bad == 0
        cdf = R.ec_default_cdf(0)
        _, ctok, coff = R.coefficient_rates(rows, self.coeffs(), [0, len(rows)], cdf, self.xdec,
                                            self.xdec)
        return mtok, moff.astype(np.int64), ctok, coff.astype(np.int64)

    def slice_of(self, toks, i, span=None):
        """Block i's tokens: its partition node, its mode info, its coefficients"""
        mtok, moff, ctok, coff = toks
        a, b = self.span[i] if span is None else span
        return np.concatenate([mtok[moff[i - 1]:moff[i + 1]], ctok[coff[a]:coff[b]]])

    def candidate(self, i, block=None, rows=None):
        assert self.mode[i - 1, F["kind"]] == 1 and self.mode[i - 1, F["partition"]] == 0
        a, b = self.span[i]
        rows = self.rows[a:b] if rows is None else np.array(rows, np.int64)
        return (self.mode[i - 1], self.mode[i] if block is None else block, rows[rows[:, 0] == 0])

    def state(self, upto=None):
        """The coding state after the blocks before mode job `upto` (None: all)"""
        if upto is None:
            return R.EcCodingState(R.ec_mode_jobs(self.mode), self.rows, self.coeffs(), self.rprm,
                                   self.xdec, self.xdec)
        return R.EcCodingState(R.ec_mode_jobs(self.mode[:upto - 1]), self.rows[:self.span[upto][0]],
                               self.coeffs(), self.rprm, self.xdec, self.xdec)


def _picks(t):
    """At least 8 blocks spread over the coding order, with the first block of
    every tile, a block at column 0 of a second superblock row, a block at the
    tile's right or bottom edge, and a skip block."""
    m, blocks = t.mode, t.blocks
    want = {blocks[0], blocks[-1]}
    for tile in range(len(t.prm.tile_dims)):
        want.add(next(i for i in blocks if m[i, F["tile"]] == tile))
    want.add(next(i for i in blocks if m[i, F["bx"]] == 0 and m[i, F["by"]] == 16))
    cols, rows = t.prm.tile_dims[0]
    n4 = lambda i: 1 << (M.BSIZE_LG[int(m[i, F["bsize"]])] - 2)
    want.add(next(i for i in blocks if m[i, F["tile"]] == 0 and
                  (m[i, F["bx"]] + n4(i) >= cols or m[i, F["by"]] + n4(i) >= rows)))
    want.add(next(i for i in blocks if m[i, F["skip"]]))
    want.add(next(i for i in blocks if not m[i, F["skip"]] and m[i, F["bx"]] > 0 and m[i, F["by"]] > 0))
    want |= set(blocks[::max(1, len(blocks) // 6)])
    return sorted(want)


TILES = [
    (1, dict(frame_type=1, reference_mode=1, tile_dims=((32, 32),)), 1),
    (2, dict(frame_type=1, reference_mode=1, force_integer_mv=1, seg_enabled=1, last_active_segid=2,
             tile_dims=((34, 26), (18, 32))), 1),
    (3, dict(frame_type=0, tile_dims=((34, 26), (32, 32))), 0),
    (4, dict(frame_type=1, reference_mode=0, allow_high_precision_mv=1, tile_dims=((32, 32),)), 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(TILES)))
def test_candidate_equals_the_committed_block(k):
    """A candidate built from block i's own jobs, against the maps of the
    blocks before it, gets block i's slice of the tile's stream; so it does
    against the maps of all blocks."""
    R.require_device()
    seed, prm_kw, xdec = TILES[k]
    t = Tile(seed, prm_kw, xdec)
    toks = t.tokenize()
    picks = _picks(t)
    assert len(picks) >= 8
    want = [t.slice_of(toks, i) for i in picks]
    assert any(len(w) > 100 for w in want)
    full = t.state()
    maps = (full.mode_map_host(), full.coef_map_host())
    tok, off, bad = R.ec_tokenize_candidates(full, [t.candidate(i) for i in picks])
    assert bad == 0
    for n, i in enumerate(picks):
        np.testing.assert_array_equal(tok[off[n]:off[n + 1]], want[n], err_msg=f"block {i}, all maps")
    assert len(tok) == off[-1] == sum(len(w) for w in want)
    np.testing.assert_array_equal(full.mode_map_host(), maps[0])
    np.testing.assert_array_equal(full.coef_map_host(), maps[1])
    for n, i in enumerate(picks):
        tok, off, bad = R.ec_tokenize_candidates(t.state(i), [t.candidate(i)])
        assert bad == 0 and off.tolist() == [0, len(want[n])]
        np.testing.assert_array_equal(tok, want[n], err_msg=f"block {i}, maps of the blocks before")
    # no candidates at all
    tok, off, bad = R.ec_tokenize_candidates(full, [])
    assert (len(tok), off.tolist(), bad) == (0, [0], 0)


def _alternatives(t, i, n=3):
    """n other decisions for the block at mode job i: mode, refs, MVs, coefficients"""
    out = []
    lg = M.BSIZE_LG[int(t.mode[i, F["bsize"]])]
    while len(out) < n:
        j = TM._rand_block(t.rng, t.prm, lg)
        j[[F["tile"], F["bx"], F["by"]]] = t.mode[i, [F["tile"], F["bx"], F["by"]]]
        if len(out) < n - 1 and j[F["skip"]]:
            continue  # at most the last one is a skip candidate
        out.append((j, t.block_rows(j, 30.0)))
    return out


def _replaced(t, i, block, rows):
    """The tile's job lists with block i replaced, and the replaced block's row span"""
    a, b = t.span[i]
    mode = t.mode.copy()
    mode[i] = block
    new_rows = np.concatenate([t.rows[:a], np.array(rows, np.int64).reshape(-1, 10), t.rows[b:]])
    return mode, new_rows, (a, a + len(rows))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2])
def test_alternatives_at_one_position(k):
    """Three different candidates at one position in one call: each equals the
    slice obtained by replacing the block in the job lists and tokenizing the
    tile again with the existing entry points; the maps are untouched."""
    R.require_device()
    seed, prm_kw, xdec = TILES[k]
    t = Tile(seed + 10, prm_kw, xdec)
    inner = [i for i in t.blocks if t.mode[i, F["bx"]] > 0 and t.mode[i, F["by"]] > 0]
    for i in (inner[len(inner) // 3], inner[-1], t.blocks[0]):
        alts = _alternatives(t, i)
        want = []
        for block, rows in alts:
            mode, new_rows, span = _replaced(t, i, block, rows)
            want.append(t.slice_of(t.tokenize(mode, new_rows), i, span))
        assert len({w.tobytes() for w in want}) == 3
        state = t.state()  # after the alternatives' coefficients were drawn
        maps = (state.mode_map_host(), state.coef_map_host())
        cands = [t.candidate(i, block, rows) for block, rows in alts] + [t.candidate(i)]
        tok, off, bad = R.ec_tokenize_candidates(state, cands)
        assert bad == 0
        for n, w in enumerate(want):
            np.testing.assert_array_equal(tok[off[n]:off[n + 1]], w, err_msg=f"block {i} alt {n}")
        np.testing.assert_array_equal(tok[off[3]:off[4]], t.slice_of(t.tokenize(), i))
        assert state.mode_map_host().tobytes() == maps[0].tobytes()
        assert state.coef_map_host().tobytes() == maps[1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("xdec", [1, 0])
def test_sibling_transform_blocks_see_each_other(xdec):
    """A 32x32 candidate coded as four 16x16 luma transforms plus chroma, and a
    16x16 one as four 8x8: the later siblings read the txb_skip / dc_sign
    contexts the earlier ones set."""
    R.require_device()
    t = Tile(41 + xdec, dict(frame_type=1, reference_mode=1, tile_dims=((32, 32),)), xdec)
    done = set()
    for i in t.blocks:
        lg = M.BSIZE_LG[int(t.mode[i, F["bsize"]])]
        if lg not in (4, 5) or lg in done or t.mode[i, F["bx"]] == 0 or t.mode[i, F["by"]] == 0:
            continue
        done.add(lg)
        block = t.mode[i].copy()
        block[F["skip"]] = 0
        rows = t.block_rows(block, 40.0, split_luma=True)
        assert sum(r[1] == 0 for r in rows) == 4
        mode, new_rows, span = _replaced(t, i, block, rows)
        want = t.slice_of(t.tokenize(mode, new_rows), i, span)
        # the siblings matter: with the later three reading the committed map
        # alone the stream would differ
        tok, off, bad = R.ec_tokenize_candidates(t.state(), [t.candidate(i, block, rows)])
        assert bad == 0
        np.testing.assert_array_equal(tok, want, err_msg=f"log2 size {lg}")
    assert done == {4, 5}


@pytest.mark.gpu
def test_candidate_rates_end_to_end():
    """candidate_rates = ec_count_stream of the ground-truth slice from the
    group's snapshot, with and without init."""
    R.require_device()
    seed, prm_kw, xdec = TILES[1]
    t = Tile(seed + 20, prm_kw, xdec)
    toks = t.tokenize()
    picks = _picks(t)
    want_tok = [t.slice_of(toks, i) for i in picks]
    n = len(picks)
    cdfs = np.stack([R.ec_default_cdf_all(q) for q in (0, 3, 1)])
    R.ec_count_stream(np.concatenate(want_tok), cdfs[2])  # an adapted snapshot
    sid = np.arange(n) % 3
    init = np.array([0x8000 | (0xFFF7 << 16), 0xC123 | (3 << 16), 0x9ABC | (0xFFFE << 16)] * n,
                    np.uint32)[:n]
    bounds = np.concatenate([[0], np.cumsum([len(w) for w in want_tok])])
    cands = [t.candidate(i) for i in picks]
    for ini in (None, init):
        want = _host_stream_rates(np.concatenate(want_tok), bounds, cdfs, sid, ini)
        rates, tok, off = R.candidate_rates(R.ec_mode_jobs(t.mode), t.rows, t.coeffs(), cands,
                                            t.rprm, cdfs, sid, ini, xdec, xdec)
        np.testing.assert_array_equal(off, bounds)
        np.testing.assert_array_equal(tok, np.concatenate(want_tok))
        np.testing.assert_array_equal(rates, want)
    # no group_cdf: snapshot 0
    rates, _, _ = R.candidate_rates(R.ec_mode_jobs(t.mode), t.rows, t.coeffs(), cands, t.rprm, cdfs,
                                    xdec=xdec, ydec=xdec)
    np.testing.assert_array_equal(
        rates, _host_stream_rates(np.concatenate(want_tok), bounds, cdfs, np.zeros(n, int)))


@pytest.mark.gpu
def test_candidates_outside_the_restrictions_are_counted_and_emit_nothing():
    R.require_device()
    seed, prm_kw, xdec = TILES[0]
    t = Tile(seed + 30, prm_kw, xdec)
    state = t.state()
    picks = [i for i in _picks(t) if not t.mode[i, F["skip"]]][:5]
    good = [t.candidate(i) for i in picks]
    cdfs = R.ec_default_cdf_all(1)
    rates0, tok0, off0, rej0, bad0 = R.ec_candidate_rates(state, good, cdfs)
    assert (rej0, bad0) == (0, 0) and rates0.min() > 0
    i = picks[1]
    node, block, rows = t.candidate(i)

    def blk(**kw):
        j = block.copy()
        for f, v in kw.items():
            j[F[f]] = v
        return j
    far = rows.copy()
    far[0, 2] += 64  # a transform block outside its block
    off_map = rows.copy()
    off_map[:, 2] = 1 << 20
    wrong_node = node.copy()
    wrong_node[F["bx"]] += 16
    horz = node.copy()
    horz[F["partition"]] = 1
    bad_cands = [
        (node, blk(bsize=0), rows),               # 4x4
        (node, blk(bsize=4), rows),               # 8x16
        (node, blk(luma_mode=28, chroma_mode=28), rows),
        (node, blk(tile=7), rows),
        (node, blk(skip=1), rows),                # a skip block with transform blocks
        (node, blk(kind=1), rows),                # no block
        (block, block, rows),                     # a block where the node belongs
        (wrong_node, block, rows),                # a node somewhere else
        (horz, block, rows),                      # PARTITION_HORZ
        (node, block, far),
        (node, block, off_map),
    ]
    for bad_c in bad_cands:
        tok, off, rej = R.ec_tokenize_candidates(state, [bad_c], check=False)
        assert (len(tok), off.tolist(), rej) == (0, [0, 0], 1)
    mixed, is_bad = [], []
    for n, c in enumerate(good):
        mixed += [c] + bad_cands[2 * n:2 * n + 2] + ([bad_cands[10]] if n == 4 else [])
        is_bad += [False] + [True] * (len(mixed) - len(is_bad) - 1)
    assert sum(is_bad) == len(bad_cands)
    is_bad = np.array(is_bad)
    rates, tok, off, rej, bad = R.ec_candidate_rates(state, mixed, cdfs, check=False)
    assert (rej, bad) == (len(bad_cands), 0)
    np.testing.assert_array_equal(tok, tok0)
    cnt = np.diff(off.astype(np.int64))
    assert not cnt[is_bad].any() and not rates[is_bad].any()
    np.testing.assert_array_equal(cnt[~is_bad], np.diff(off0.astype(np.int64)))
    np.testing.assert_array_equal(rates[~is_bad], rates0)

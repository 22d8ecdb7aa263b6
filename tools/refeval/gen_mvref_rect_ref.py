"""Reference-evaluated vectors for the MV reference stack on the ground
tests/golden/ref_mvref.npz leaves out (tests/golden/ref_mvref_rect.npz).

    python tools/refeval/gen_mvref_rect_ref.py        (in the build container)

gen_mvref_ref.py's environment and file format, with other grids and queries:

  * partitions that also hold PARTITION_HORZ and PARTITION_VERT leaves
    (2:1 and 1:2 blocks, n4 2..16), so n4_w != n4_h in the cells;
  * superblocks left uncoded: their cells are Block::default()
    (src/context.rs:1425-1442: ref_frames [INTRA_FRAME; 2], 64x64);
  * queries at the coded leaves' positions with the leaves' own sizes,
    square and 2:1 / 1:2, for the single and the compound stacks.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_mvref_ref as M  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402

OUT = os.path.join(M.ROOT, "tests", "golden", "ref_mvref_rect.npz")
CASES, QUERIES = 12, 32


class FreshBlocks(M.Blocks):
    """M.Blocks whose cells are (mode, refs, mv0, mv1, w4, h4) tuples, each read
    a new Block: the evaluated clamp assigns into the stack entries' MVs, which
    would otherwise be the cell's own objects (Rust copies them)."""

    def index_any(self, bo):
        b = bo._f["0"]
        mode, refs, m0, m1, w4, h4 = self.grid[int(b._f["y"])][int(b._f["x"])]
        return RI.Struct("Block", {
            "mode": mode, "ref_frames": [M.RefT(refs[0]), M.RefT(refs[1])],
            "mv": [M.mv(*m0), M.mv(*m1)], "n4_w": M.usz(w4), "n4_h": M.usz(h4)})


def gen_case(rng, I, case, out):
    sbw, sbh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    cols = sbw * 16 - (int(rng.integers(0, 4)) * 2 if rng.random() < 0.4 else 0)
    rows = sbh * 16 - (int(rng.integers(0, 4)) * 2 if rng.random() < 0.4 else 0)
    tx, ty = int(rng.integers(0, 3)) * 16, int(rng.integers(0, 3)) * 16
    fcols, fr = tx + cols + int(rng.integers(0, 2)) * 16, ty + rows + int(rng.integers(0, 2)) * 16
    pool = [(int(rng.integers(-200, 200)), int(rng.integers(-200, 200))) for _ in range(3)]
    W, Hh = sbw * 16, sbh * 16
    default = (M.PM["DC_PRED"], (0, 0), (0, 0), (0, 0), 16, 16)
    cells = [[default] * W for _ in range(Hh)]
    recs = np.zeros((Hh, W, 9), np.int32)
    recs[:, :, 6:8] = 16
    leaves = []

    def leaf(x, y, w4, h4):
        r = rng.random()
        if r < 0.2:
            refs, mode = (0, 8), M.PM["DC_PRED"]
        elif r < 0.45:
            refs, mode = (1, 2), M.PM[M.MODES[20 + int(rng.integers(0, 8))]]
        else:
            refs = (1 + int(rng.integers(0, 2)), 8)
            mode = M.PM[M.MODES[14 + int(rng.integers(0, 6))]]
        m0, m1 = M.rand_mv(rng, pool), M.rand_mv(rng, pool)
        if refs[1] == 8:
            m1 = (0, 0)
        if refs[0] == 0:
            m0 = m1 = (0, 0)
        b = (mode, refs, m0, m1, w4, h4)
        for j in range(y, min(y + h4, Hh)):
            for i in range(x, min(x + w4, W)):
                cells[j][i] = b
                recs[j, i] = (refs[0], refs[1], m0[0], m0[1], m1[0], m1[1], w4, h4,
                              int(mode in M.NEWMV_MODES))
        if x < cols and y < rows:
            leaves.append((x, y, w4, h4))

    def node(x, y, n4):
        # PARTITION_NONE / SPLIT / HORZ / VERT (the last two from 16x16 up:
        # their halves stay at 8 pixels or more)
        r = rng.random()
        h = n4 // 2
        if n4 > 2 and r < 0.4:
            for (dx, dy) in ((0, 0), (h, 0), (0, h), (h, h)):
                node(x + dx, y + dy, h)
        elif n4 > 2 and r < 0.6:
            leaf(x, y, n4, h)
            leaf(x, y + h, n4, h)
        elif n4 > 2 and r < 0.8:
            leaf(x, y, h, n4)
            leaf(x + h, y, h, n4)
        else:
            leaf(x, y, n4, n4)
    for sy in range(sbh):
        for sx in range(sbw):
            if sbw * sbh > 1 and rng.random() < 0.3:
                continue  # an uncoded superblock: Block::default() cells
            node(sx * 16, sy * 16, 16)
    blocks = FreshBlocks(cells, cols, rows, tx, ty, fcols, fr)
    sbias = [bool(rng.random() < 0.5) for _ in range(7)]
    fi = RI.Struct("FrameInvariants", {"ref_frame_sign_bias": sbias})
    cw = RI.Struct("ContextWriter", {"bc": RI.Struct("BlockContext", {"blocks": blocks})})
    out["grids"].append((case, tx, ty, cols, rows, fcols, fr, W, Hh, int(sbias[0]), int(sbias[1])))
    out["cells"].append(recs.reshape(-1, 9))
    nq = 0
    order = rng.permutation(len(leaves))[:QUERIES]
    for k in order:
        bx, by, w4, h4 = leaves[int(k)]
        kind = int(rng.integers(0, 3))
        rf = (1, 8) if kind == 0 else (2, 8) if kind == 1 else (1, 2)
        bs = H.BlockSizeV(H.BLOCK_NAMES.index("%dX%d" % (w4 * 4, h4 * 4)))
        stack = []
        ctxv = M.call(I, cw, "find_mvrefs", M.tile_bo(bx, by), [M.RefT(rf[0]), M.RefT(rf[1])],
                      stack, bs, fi, rf[1] != 8)
        ent = np.zeros((9, 5), np.int32)
        for i, c in enumerate(stack):
            ent[i] = (int(c.this_mv.row), int(c.this_mv.col), int(c.comp_mv.row),
                      int(c.comp_mv.col), int(c.weight))
        out["query"].append((case, bx, by, w4, h4, rf[0], rf[1], int(ctxv), len(stack)))
        out["entries"].append(ent)
        nq += 1
    return nq


def main():
    t0 = time.time()
    rng = np.random.default_rng(0x7EC7)
    I = M.make()
    out = {"grids": [], "cells": [], "query": [], "entries": []}
    nq = 0
    for case in range(CASES):
        nq += gen_case(rng, I, case, out)
    np.savez_compressed(OUT, grids=np.array(out["grids"], np.int32),
                        cells=np.concatenate(out["cells"]).astype(np.int32),
                        query=np.array(out["query"], np.int32),
                        entries=np.array(out["entries"], np.int32))
    print("wrote %s: %d cases, %d queries in %.0f s" % (OUT, len(out["grids"]), nq, time.time() - t0))


if __name__ == "__main__":
    main()

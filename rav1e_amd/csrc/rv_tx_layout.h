// rv_tx_layout.h -- internal: how a partition's transform blocks are laid out
// (write_tx_blocks / write_tx_tree, src/encoder.rs:1757-2037), shared by the
// launch that codes them (rv_tx_blocks.hip) and the one that reads their
// distortions and eobs back per candidate (rv_mode_decide.hip).
#pragma once
#include <cstdio>

#include "rv_device.h"

namespace rv {

constexpr uint8_t kTxbTxW[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kTxbTxH[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
// BlockSize in pixels; the sizes above 64x64 are not taken
constexpr uint8_t kTxbBlkW[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 0, 0, 0, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kTxbBlkH[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 0, 0, 0, 16, 4, 32, 8, 64, 16};

// The geometry both entry points share (and the launch's argument checks that
// depend on it alone); RV_OK, or the code with the message set.
static inline int txb_layout(int bsize, int tx_size, int xdec, int ydec, int luma_only,
                      rv_tx_blocks_layout_t *o) {
  auto fail = [](int code, const char *what) {
    char msg[160];
    snprintf(msg, sizeof msg, "rv_tx_blocks: %s", what);
    return rv_set_error(code, msg);
  };
  if (!o) return fail(RV_EINVAL, "null layout");
  if (bsize < 0 || bsize > 21) return fail(RV_EINVAL, "bsize is no BlockSize");
  if (tx_size < 0 || tx_size > 18) return fail(RV_EINVAL, "tx_size is no TxSize");
  if (!((xdec == 0 && ydec == 0) || (xdec == 1 && (ydec == 0 || ydec == 1))))
    return fail(RV_EINVAL, "subsampling must be 4:4:4, 4:2:2 or 4:2:0");
  if (bsize > 12) return fail(RV_ENOTSUP, "4:1 / 1:4 partitions and sizes above 64x64 are not supported");
  const int bw = kTxbBlkW[bsize], bh = kTxbBlkH[bsize];
  if (bw == 4 || bh == 4) return fail(RV_ENOTSUP, "4xN / Nx4 partitions are not supported");
  // subsampled_size (src/partition.rs:245-286): no 1:2 size at 4:2:2
  if (!luma_only && xdec == 1 && ydec == 0 && bh == 2 * bw)
    return fail(RV_ENOTSUP, "the block size has no subsampled size at 4:2:2 (BLOCK_INVALID)");
  const int tw = kTxbTxW[tx_size], th = kTxbTxH[tx_size];
  if (tw > bw || th > bh) return fail(RV_EINVAL, "tx_size does not divide the partition");
  *o = rv_tx_blocks_layout_t{};
  o->planes = luma_only ? 1 : 3;
  int blocks = 0, levels = 0;
  for (int p = 0; p < o->planes; p++) {
    int pw = bw, ph = bh, ts = tx_size;
    if (p) {
      // largest_chroma_tx_size (src/partition.rs:288-297): the plane block's
      // transform, 64-point sides coded as 32 (av1_get_coded_tx_size)
      pw = bw >> xdec, ph = bh >> ydec;
      const int uw = pw < 32 ? pw : 32, uh = ph < 32 ? ph : 32;
      for (ts = 0; ts < 19; ts++)
        if (kTxbTxW[ts] == uw && kTxbTxH[ts] == uh) break;
    }
    const int w = kTxbTxW[ts], h = kTxbTxH[ts];
    o->tx_size[p] = ts;
    o->plane_w[p] = pw, o->plane_h[p] = ph;
    // bw x bh, bw_uv x bh_uv (src/encoder.rs:1764-1765, 1823-1832)
    o->cols[p] = pw / w, o->rows[p] = ph / h;
    o->n_blocks[p] = o->cols[p] * o->rows[p];
    o->coded_area[p] = (w < 32 ? w : 32) * (h < 32 ? h : 32);
    o->first_block[p] = blocks;
    o->level_off[p] = levels;
    for (int i = 0; i < o->n_blocks[p]; i++) {
      o->blk_x[p][i] = (uint8_t)((i % o->cols[p]) * w);
      o->blk_y[p][i] = (uint8_t)((i / o->cols[p]) * h);
    }
    blocks += o->n_blocks[p];
    levels += o->n_blocks[p] * o->coded_area[p];
  }
  o->blocks_per_job = blocks;
  o->levels_per_job = levels;
  return RV_OK;
}

}  // namespace rv

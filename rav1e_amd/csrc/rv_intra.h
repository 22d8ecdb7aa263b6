// rv_intra.h -- intra prediction and get_intra_edges on the device, shared by
// the batched predictor (rv_intra.hip), the intra-mode screening of the
// replay (rv_intra_pass.hip) and the intra RDO chains (rv_rdo.hip).
//
// Edge buffer (rav1e's edge_buf, 4 * MAX_TX_SIZE + 1 pixels, built by
// get_intra_edges, src/partition.rs:500-693): left pixels bottom-to-top and
// right-aligned in [0, 128), the top-left pixel at 128, the above row (and
// above-right) from 129.  On the device it lives in LDS as i32.
#pragma once

#include "rv_device.h"

namespace rv {

constexpr int kIntraEdge = 4 * 64 + 1;
constexpr int kIntraModes = 13;
// RAV1E_INTRA_MODES (src/predict.rs:32-46) as PredictionMode values
static __constant__ uint8_t kIntraModeOrder[kIntraModes] = {0, 2, 1, 9, 11, 10, 12,
                                                             3, 4, 5, 6, 7, 8};

// sm_weight_arrays (src/predict.rs:406-424)
static __constant__ uint8_t kSmW[128] = {
    0,   0,   255, 128, 255, 149, 85,  64,  255, 197, 146, 105, 73,  50,  37,  32,
    255, 225, 196, 170, 145, 123, 102, 84,  68,  54,  43,  33,  26,  20,  17,  16,
    255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92,  83,  74,
    66,  59,  52,  45,  39,  34,  29,  25,  21,  17,  14,  12,  10,  9,   8,   8,
    255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150,
    144, 138, 133, 127, 121, 116, 111, 106, 101, 96,  91,  86,  82,  77,  73,  69,
    65,  61,  57,  54,  50,  47,  44,  41,  38,  35,  32,  29,  27,  25,  22,  20,
    18,  16,  15,  13,  12,  10,  9,   8,   7,   6,   6,   5,   5,   4,   4,   4};

// dr_intra_derivative (src/predict.rs:912-944) of the angles rav1e's six
// directional modes reach (45, 23, 67)
__device__ __forceinline__ int intra_dr_deriv(int a) {
  return a == 45 ? 64 : a == 23 ? 151 : a == 67 ? 27 : 0;
}

// predict_intra's remaps (src/predict.rs:214-236): PAETH by variant, and the
// directional angle of a mode.  variant: PredictionVariant (0 NONE, 1 LEFT,
// 2 TOP, 3 BOTH) of the block's tile position.
__device__ __forceinline__ int intra_remap(int mode, int variant) {
  return mode == 12 ? (variant == 0 ? 0 : variant == 1 ? 2 : variant == 2 ? 1 : 12) : mode;
}
__device__ __forceinline__ int intra_angle(int mode) {
  return mode == 3 ? 45 : mode == 4 ? 135 : mode == 5 ? 113 : mode == 6 ? 157
       : mode == 7 ? 203 : mode == 8 ? 67 : 0;
}

// Per-block constants of a (remapped) mode: DC value (needs the edge sums),
// derivatives.
struct IntraSetup {
  int mode, angle, dx, dy;
  int32_t dcv;
};

// The DC value of the remapped DC_PRED (pred_dc / _top / _left / _128,
// src/predict.rs:603-661): sums over the first h left / w above pixels,
// reduced over the G lanes of this lane's group.
template <int G>
__device__ __forceinline__ int32_t intra_dc(const int32_t *e, int variant, int w, int h, int bd,
                                            int lane) {
  const int L0 = 128 - h, A0 = 129;
  uint32_t s = 0;
  if (variant & 1)
    for (int k = lane; k < h; k += G) s += (uint32_t)e[L0 + k];
  if (variant & 2)
    for (int k = lane; k < w; k += G) s += (uint32_t)e[A0 + k];
  s = group_sum<G>(s);
  const uint32_t len = (variant & 1 ? h : 0) + (variant & 2 ? w : 0);
  return variant == 0 ? (128 << (bd - 8)) : (int32_t)((s + (len >> 1)) / len);
}

__device__ __forceinline__ IntraSetup intra_setup(int mode, int variant) {
  IntraSetup s;
  s.mode = intra_remap(mode, variant);
  s.angle = intra_angle(s.mode);
  const int a = s.angle;
  s.dx = a < 90 ? intra_dr_deriv(a) : (a > 90 && a < 180 ? intra_dr_deriv(180 - a) : 0);
  s.dy = (a > 90 && a < 180) ? intra_dr_deriv(a - 90) : (a > 180 ? intra_dr_deriv(270 - a) : 0);
  s.dcv = 0;
  return s;
}

// Pixel (r, c) of the w x h prediction (the native Intra trait,
// src/predict.rs:599-1034; no edge filter or upsampling, as rav1e).
__device__ __forceinline__ int32_t intra_px(const IntraSetup &s, const int32_t *e, int w, int h,
                                            int r, int c, int maxv) {
  const int L0 = 128 - h, LB = 128 - h - w, A0 = 129;
  switch (s.mode) {
    case 0: return s.dcv;                          // DC_PRED
    case 1: return e[A0 + c];                      // V_PRED
    case 2: return e[L0 + h - 1 - r];              // H_PRED
    case 12: {                                     // PAETH_PRED
      const int32_t tl = e[128], l = e[L0 + h - 1 - r], t = e[A0 + c];
      const int32_t base = t + l - tl;
      const int32_t pl = abs(base - l), pt = abs(base - t), ptl = abs(base - tl);
      return (pl <= pt && pl <= ptl) ? l : (pt <= ptl ? t : tl);
    }
    case 9: {  // SMOOTH_PRED: weights scaled by 2^8, log2_scale 9
      const uint32_t wh = kSmW[h + r], ww = kSmW[w + c];
      const uint32_t v = wh * (uint32_t)e[A0 + c] + (256 - wh) * (uint32_t)e[L0] +
                         ww * (uint32_t)e[L0 + h - 1 - r] + (256 - ww) * (uint32_t)e[A0 + w - 1];
      return (int32_t)((v + 256) >> 9);
    }
    case 11: {  // SMOOTH_H_PRED
      const uint32_t ww = kSmW[w + c];
      return (int32_t)((ww * (uint32_t)e[L0 + h - 1 - r] + (256 - ww) * (uint32_t)e[A0 + w - 1] +
                        128) >> 8);
    }
    case 10: {  // SMOOTH_V_PRED
      const uint32_t wh = kSmW[h + r];
      return (int32_t)((wh * (uint32_t)e[A0 + c] + (256 - wh) * (uint32_t)e[L0] + 128) >> 8);
    }
    default: {  // pred_directional (src/predict.rs:894-1034)
      int32_t v;
      if (s.angle < 90) {
        const int idx = (r + 1) * s.dx, base = (idx >> 6) + c, sh = (idx >> 1) & 31;
        const int mb = h + w - 1;
        v = base < mb ? round_shift(e[A0 + base] * (32 - sh) + e[A0 + base + 1] * sh, 5) : e[A0 + mb];
      } else if (s.angle < 180) {
        const int idx = (c << 6) - (r + 1) * s.dx, base = idx >> 6;
        if (base >= -1) {
          const int sh = (idx >> 1) & 31;
          const int32_t a = base < 0 ? e[128] : e[A0 + base];
          v = round_shift(a * (32 - sh) + e[A0 + base + 1] * sh, 5);
        } else {
          const int idy = (r << 6) - (c + 1) * s.dy, bl = idy >> 6, sh = (idy >> 1) & 31;
          const int32_t a = bl < 0 ? e[128] : e[LB + w + h - 1 - bl];
          v = round_shift(a * (32 - sh) + e[LB + w + h - 2 - bl] * sh, 5);
        }
      } else {
        const int idx = (c + 1) * s.dy, base = (idx >> 6) + r, sh = (idx >> 1) & 31;
        v = round_shift(e[LB + w + h - 1 - base] * (32 - sh) + e[LB + w + h - 2 - base] * sh, 5);
      }
      return v < 0 ? 0 : (v > maxv ? maxv : v);
    }
  }
}

// get_intra_edges (src/partition.rs:500-693) with opt_mode None for the
// transform block of a superblock-level partition (an n x n block at
// tile-relative pixel (x, y) of a tw-wide tile region whose pixel (0, 0) is
// plane pixel (tx, ty)): has_top_right holds iff the top row and the right
// neighbour exist, has_bottom_left never (src/recon_intra.rs:174-470 for
// the first transform block of a 64x64 partition).  The G lanes of a group
// fill e (i32, LDS); entries no branch of the reference writes are zero.
// The caller orders the writes before any read (a barrier).
template <typename Px, int G>
__device__ __forceinline__ void intra_edges_sb(const rv_plane &p, int tx, int ty, int tw, int x,
                                               int y, int n, int have_top, int bd, int32_t *e,
                                               int lane) {
  const int base = 128 << (bd - 8);
  const int L = 128, A = 129;
  auto D = [&](int r, int c) -> int32_t { return (int32_t)*plane_ptr<Px>(p, tx + c, ty + r); };
  const int na = (y != 0 && have_top && x + n < tw) ? (n < tw - x - n ? n : tw - x - n) : 0;
  for (int i = lane; i < kIntraEdge; i += G) {
    int32_t v = 0;
    if (i >= L - n && i < L) {  // left
      const int k = i - (L - n);
      v = x != 0 ? D(y + n - 1 - k, x - 1) : (y != 0 ? D(y - 1, 0) : base + 1);
    } else if (i == L) {  // top-left
      v = x == 0 && y == 0 ? base : y == 0 ? D(0, x - 1) : x == 0 ? D(y - 1, 0) : D(y - 1, x - 1);
    } else if (i >= A && i < A + n) {  // top
      const int k = i - A;
      v = y != 0 ? D(y - 1, x + k) : (x != 0 ? D(0, x - 1) : base - 1);
    } else if (i >= A + n && i < A + 2 * n) {  // top-right: available, else the last one
      const int k = i - A - n;
      const int kk = k < na ? k : na - 1;
      if (kk >= 0)
        v = D(y - 1, x + n + kk);
      else  // none available: above[n - 1]
        v = y != 0 ? D(y - 1, x + n - 1) : (x != 0 ? D(0, x - 1) : base - 1);
    } else if (i >= L - 2 * n && i < L - n) {  // bottom-left: left[L - n] replicated
      v = x != 0 ? D(y + n - 1, x - 1) : (y != 0 ? D(y - 1, 0) : base + 1);
    }
    e[i] = v;
  }
}

// ---- get_intra_edges, general form (src/partition.rs:500-693) --------------
// BlockSize (src/partition.rs:116-140) in 4x4 units; 0 past BLOCK_64X64 and
// for the 4:1 / 1:4 sizes, which the general form does not take.
static __constant__ uint8_t kBlkW4[22] = {1, 1, 2, 2, 2, 4, 4, 4, 8, 8, 8, 16, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static __constant__ uint8_t kBlkH4[22] = {1, 2, 1, 2, 4, 2, 4, 8, 4, 8, 16, 8, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// The general case of has_top_right / has_bottom_left (src/recon_intra.rs:
// 233-241, 448-456): whether the block of the same size to the top right /
// bottom left of the bw4 x bh4 block at (mi_row, mi_col) of a 64x64
// superblock is coded before it.  Blocks are coded in the recursive
// top-left, top-right, bottom-left, bottom-right order; a 2:1 block is the
// top / bottom half and a 1:2 block the left / right half of the square s =
// max(bw4, bh4).  Walking up the quadtree from that square:
//   top right:   a bottom-left quadrant sees its top-right sibling, a
//                bottom-right one would need the next square to the right, a
//                top-left one the square above; a top-right one asks its
//                parent.
//   bottom left: a top-left quadrant sees the square to its left, a right
//                quadrant would need its own bottom-left sibling, coded
//                later; a bottom-left one asks its parent.
// The reference reads the same answers from tables indexed by position.
__device__ __forceinline__ bool intra_tr_coded(int mi_row, int mi_col, int bw4, int bh4) {
  const int r = mi_row & 15, c = mi_col & 15;
  if (bw4 > bh4 && (r & bh4)) return false;  // bottom half: the square to the right
  if (bw4 < bh4 && !(c & bw4)) return true;  // left half: above the right half
  for (int s = bw4 > bh4 ? bw4 : bh4; s < 16; s <<= 1) {
    if (r & s) return !(c & s);
    if (!(c & s)) return true;
  }
  return true;  // the superblock's top row
}
__device__ __forceinline__ bool intra_bl_coded(int mi_row, int mi_col, int bw4, int bh4) {
  const int r = mi_row & 15, c = mi_col & 15;
  if (bw4 > bh4 && !(r & bh4)) return true;  // top half: beside the square to the left
  if (bw4 < bh4 && (c & bw4)) return false;  // right half: below the left half
  for (int s = bw4 > bh4 ? bw4 : bh4; s < 16; s <<= 1) {
    if (c & s) return false;
    if (!(r & s)) return true;
  }
  return false;  // the superblock's bottom row
}

// has_top_right (src/recon_intra.rs:174-243), 64x64 superblocks.  bw4 / bh4:
// the partition after supersample_chroma_bsize; txw4: tx_size.width_mi().
__device__ __forceinline__ bool intra_has_top_right(int bw4, int bh4, int mi_col, int mi_row,
                                                    bool top, bool right, int txw4, int row_off,
                                                    int col_off, int ss_x) {
  if (!top || !right) return false;
  const int plane_bw = max(bw4 >> ss_x, 1);
  if (row_off > 0) return col_off + txw4 < plane_bw;
  if (col_off + txw4 < plane_bw) return true;
  const int lw = 31 - __builtin_clz(bw4), lh = 31 - __builtin_clz(bh4);
  const int br = (mi_row & 15) >> lh, bc = (mi_col & 15) >> lw;
  if (br == 0) return true;
  if (((bc + 1) << lw) >= 16) return false;
  return intra_tr_coded(mi_row, mi_col, bw4, bh4);
}

// has_bottom_left (src/recon_intra.rs:376-458), 64x64 superblocks.
__device__ __forceinline__ bool intra_has_bottom_left(int bw4, int bh4, int mi_col, int mi_row,
                                                      bool bottom, bool left, int txh4,
                                                      int row_off, int col_off, int ss_y) {
  if (!bottom || !left) return false;
  if (col_off > 0) return false;
  const int plane_bh = max(bh4 >> ss_y, 1);
  if (row_off + txh4 < plane_bh) return true;
  const int lw = 31 - __builtin_clz(bw4), lh = 31 - __builtin_clz(bh4);
  const int br = (mi_row & 15) >> lh, bc = (mi_col & 15) >> lw;
  if (bc == 0) return ((br << lh) >> ss_y) + row_off + txh4 < (16 >> ss_y);
  if (((br + 1) << lh) >= 16) return false;
  return intra_bl_coded(mi_row, mi_col, bw4, bh4);
}

// supersample_chroma_bsize (src/partition.rs:459-498) on 4x4-unit sizes: a
// 4-pixel side doubles on a decimated axis.  Of the sizes taken here only
// 4x4, 4x8 and 8x4 change.
__device__ __forceinline__ void intra_supersample(int &bw4, int &bh4, int ss_x, int ss_y) {
  const int w = bw4, h = bh4;
  if (w == 1 && h == 1) {
    bw4 <<= ss_x;
    bh4 <<= ss_y;
  } else if (w == 1 && h == 2) {  // BLOCK_4X8 -> 8X8 where x is decimated
    bw4 <<= ss_x;
  } else if (w == 2 && h == 1) {  // BLOCK_8X4 -> 8X8 where y is decimated
    bh4 <<= ss_y;
  }
}

// What one call of get_intra_edges depends on besides the pixels.
struct IntraEdgeGeo {
  int tx, ty, tw, th;  // the tile's region of this plane: origin (plane pixels) and size
  int x, y;            // po: the block's tile-relative pixel offset in this plane
  int w, h;            // tx_size
  int ntr, nbl;        // num_avail of the top-right / bottom-left branch
  uint32_t needs;      // bit 0 left, 1 top-left, 2 top, 3 top-right, 4 bottom-left
};

// The needs_* masks under opt_mode (src/partition.rs:525-557); mode < 0: None.
__device__ __forceinline__ uint32_t intra_edge_needs(int mode, int x, int y) {
  if (mode < 0) return 31u;
  if (mode == 12) mode = x == 0 && y == 0 ? 0 : y == 0 ? 2 : x == 0 ? 1 : 12;
  const bool dc_or_cfl = mode == 0 || mode == 13;
  const bool left = mode != 1 && (!dc_or_cfl || x != 0) && !(mode == 3 || mode == 8);
  const bool topleft = mode == 12 || mode == 5 || mode == 4 || mode == 6;
  const bool top = mode != 2 && (!dc_or_cfl || y != 0);
  const bool topright = mode == 3 || mode == 8;
  const bool bottomleft = mode == 7;
  return (uint32_t)left | (uint32_t)topleft << 1 | (uint32_t)top << 2 | (uint32_t)topright << 3 |
         (uint32_t)bottomleft << 4;
}

// The geometry of get_intra_edges (src/partition.rs:597-674) for transform
// block (bx, by) of the partition at (mi_col, mi_row) (tile-relative 4x4
// units) of size bw4 x bh4 (before supersample_chroma_bsize).
__device__ __forceinline__ IntraEdgeGeo intra_edge_geo(int tx, int ty, int tw, int th, int mi_col,
                                                       int mi_row, int bw4, int bh4, int bx, int by,
                                                       int x, int y, int w, int h, int xdec,
                                                       int ydec, int mode) {
  IntraEdgeGeo g;
  g.tx = tx, g.ty = ty, g.tw = tw, g.th = th, g.x = x, g.y = y, g.w = w, g.h = h;
  g.needs = intra_edge_needs(mode, x, y);
  const int bx4 = bx * (w >> 2), by4 = by * (h >> 2);
  const bool have_top = by4 != 0 || mi_row > (ydec ? 1 : 0);
  const bool have_left = bx4 != 0 || mi_col > (xdec ? 1 : 0);
  const bool right = x + w < tw, bottom = y + h < th;
  intra_supersample(bw4, bh4, xdec, ydec);
  g.ntr = (y != 0 && intra_has_top_right(bw4, bh4, mi_col, mi_row, have_top, right, w >> 2, by4,
                                         bx4, xdec))
              ? min(w, tw - x - w) : 0;
  g.nbl = (x != 0 && intra_has_bottom_left(bw4, bh4, mi_col, mi_row, bottom, have_left, h >> 2,
                                           by4, bx4, ydec))
              ? min(h, th - y - h) : 0;
  return g;
}

// Entry i of edge_buf (src/partition.rs:559-690); entries no branch writes
// are zero.  Each entry is computed from the pixels alone, so any lane may
// produce any entry.  D(r, c): the pixel at row r, column c of the tile's
// region of the plane (the fused transform-block kernel reads the partition's
// own pixels from its working copy, rv_tx_blocks.hip).
template <typename Rd>
__device__ __forceinline__ int32_t intra_edge_rd(const IntraEdgeGeo &g, int bd, int i, Rd D) {
  const int base = 128 << (bd - 8);
  const int L = 128, A = 129;
  const int x = g.x, y = g.y, w = g.w, h = g.h;
  auto left = [&](int k) -> int32_t {  // left[2 * MAX_TX_SIZE - h + k]
    return x != 0 ? D(y + h - 1 - k, x - 1) : (y != 0 ? D(y - 1, 0) : base + 1);
  };
  auto above = [&](int k) -> int32_t {  // above[k], k < w
    return y != 0 ? D(y - 1, x + k) : (x != 0 ? D(0, x - 1) : base - 1);
  };
  if (i >= L - h && i < L) return (g.needs & 1) ? left(i - (L - h)) : 0;
  if (i == L)
    return (g.needs & 2) ? (x == 0 && y == 0 ? base : y == 0 ? D(0, x - 1) : x == 0 ? D(y - 1, 0)
                                                                                   : D(y - 1, x - 1))
                         : 0;
  if (i >= A && i < A + w) return (g.needs & 4) ? above(i - A) : 0;
  // top-right: num_avail pixels (up to w, which may exceed h), then the last
  // one up to h
  if (i >= A + w && i < A + w + max(h, g.ntr)) {
    if (!(g.needs & 8)) return 0;
    const int k = i - A - w;
    if (k < g.ntr) return D(y - 1, x + w + k);
    if (g.ntr > 0) return D(y - 1, x + w + g.ntr - 1);
    return (g.needs & 4) ? above(w - 1) : 0;  // above[w - 1] as the top branch left it
  }
  if (i >= L - h - max(w, g.nbl) && i < L - h) {  // bottom-left: likewise, downwards
    if (!(g.needs & 16)) return 0;
    const int k = L - h - 1 - i;
    if (k < g.nbl) return D(y + h + k, x - 1);
    if (g.nbl > 0) return D(y + h + g.nbl - 1, x - 1);
    return (g.needs & 1) ? left(0) : 0;  // left[2 * MAX_TX_SIZE - h] as the left branch left it
  }
  return 0;
}

// The same from a plane: pixel (0, 0) of the region is plane pixel (g.tx, g.ty).
template <typename Px>
__device__ __forceinline__ int32_t intra_edge_px(const rv_plane &p, const IntraEdgeGeo &g, int bd,
                                                 int i) {
  return intra_edge_rd(g, bd, i, [&](int r, int c) -> int32_t {
    return (int32_t)*plane_ptr<Px>(p, g.tx + c, g.ty + r);
  });
}

// get_scaled_luma_q0 (src/predict.rs:485-493)
__device__ __forceinline__ int32_t cfl_scaled(int32_t alpha, int32_t ac) {
  const int32_t q6 = alpha * ac;
  const int32_t a0 = ((q6 < 0 ? -q6 : q6) + 32) >> 6;
  return q6 < 0 ? -a0 : a0;
}

}  // namespace rv

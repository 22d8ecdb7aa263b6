// rv_mvstack.hip -- rav1e's MV reference stacks for blocks of every size, as
// an operator (ContextWriter::find_mvrefs / setup_mvref_list,
// src/context.rs:2308-2965; has_tr, src/partition.rs:695-750).
//
// rv_mvref.hip holds the replay's own stacks: 64x64 blocks on a superblock
// grid, re-evaluated in rounds.  This file is the general function over a
// tile's grid of 4x4-unit block records, the one oracle/orc_mvref.c states
// for the tests:
//
//   paint   a coding-order rv_ec_mode_job array into per-tile grids;
//   batch   find_mvrefs for an array of queries against the grids;
//   fill    the stack fields of every inter job of an rv_ec_mode_job array
//           from the grids (what encode_block_post_cdef passes on,
//           src/encoder.rs:1531-1557).
//
// One launch serves a whole tile set: for the leaves of a final partition
// find_mvrefs reads no cell that is coded at or after the querying block
// (the rows above, the columns to the left, the top-right block only where
// has_tr says it is coded, the top-left block), so the painted grid shows
// every block what the reference saw when it coded that block (DESIGN.md §5;
// tests/test_mvstack.py holds the property test).
//
// One query per lane.  A query is a short serial walk -- at most three rows
// and three columns of at most eight neighbours, each pushed into or matched
// against a stack of at most nine entries -- with nothing for 64 lanes to
// share, and a frame has hundreds of thousands of them.  The stack is indexed
// at run time, so it lives in LDS rather than in a private array (which
// would be scratch memory): entry e's word f of lane l is at
// ((e * 3 + f) * kLanes + l), the 64 lanes of one access on consecutive
// words, hence on different banks.
//
// Paint: jobs may overlap (a candidate list over committed blocks), and the
// later job of the array must win whatever the scheduling.  Pass 1, one lane
// per job: atomicMax of the job's index into a per-cell owner word.  Pass 2,
// one lane per cell: the owner's record, or Block::default() without one.
#include <cstdint>

#include "rv_device.h"

namespace rv {
namespace {

constexpr int kLanes = 256;      // lanes (queries) per workgroup
constexpr int kSlots = 9;        // MAX_REF_MV_STACK_SIZE (8) and the extra search's write past a short stack
constexpr int kStackMax = 8;     // src/context.rs:89
constexpr int kRefCatLevel = 640;  // src/context.rs:90
constexpr int kRowCols = 3;      // MVREF_ROW_COLS, src/partition.rs:98
constexpr int kIntra = 0, kNone = 8;
constexpr int kNearestMv = 14;   // PredictionMode::NEARESTMV

struct Grid {
  const rv_mv_blk *g;  // the tile's cells
  int gw, gh;          // the grid's pitch and height
  int cols, rows;      // the tile
};

// One cell: a 16-byte load; the sizes are held to 1..16 so that a scan over a
// grid the caller filled with anything still advances and ends.
struct Cell {
  int r0, r1, n4w, n4h, newmv;
  uint32_t mv0, mv1;  // row | col << 16
};
__device__ __forceinline__ Cell cell_at(const Grid &t, int x, int y) {
  x = min(max(x, 0), t.gw - 1);
  y = min(max(y, 0), t.gh - 1);
  const uint4 v = *reinterpret_cast<const uint4 *>(t.g + (size_t)y * t.gw + x);
  Cell c;
  c.r0 = (int8_t)(v.x & 255u);
  c.r1 = (int8_t)((v.x >> 8) & 255u);
  c.n4w = min(max((int)((v.x >> 16) & 255u), 1), 16);
  c.n4h = min(max((int)(v.x >> 24), 1), 16);
  c.newmv = (int)(v.y & 255u);
  c.mv0 = v.z;
  c.mv1 = v.w;
  return c;
}

__device__ __forceinline__ uint32_t mv_neg(uint32_t m) {
  const uint32_t r = (0u - (m & 0xFFFFu)) & 0xFFFFu, c = (0u - (m >> 16)) & 0xFFFFu;
  return r | c << 16;
}
__device__ __forceinline__ uint32_t mv_clamp(uint32_t m, int xmin, int xmax, int ymin, int ymax) {
  const int r = min(max((int)(int16_t)(m & 0xFFFFu), ymin), ymax);
  const int c = min(max((int)(int16_t)(m >> 16), xmin), xmax);
  return ((uint32_t)r & 0xFFFFu) | ((uint32_t)c & 0xFFFFu) << 16;
}

// The lane's stack in LDS
struct Stk {
  uint32_t *p;
  int n;
  __device__ __forceinline__ uint32_t &t(int i) { return p[(i * 3 + 0) * kLanes]; }
  __device__ __forceinline__ uint32_t &c(int i) { return p[(i * 3 + 1) * kLanes]; }
  __device__ __forceinline__ uint32_t &w(int i) { return p[(i * 3 + 2) * kLanes]; }
  __device__ __forceinline__ void set(int i, uint32_t tv, uint32_t cv, uint32_t wv) {
    t(i) = tv;
    c(i) = cv;
    w(i) = wv;
  }
};

// find_matching_mv_and_update_weight / find_matching_comp_mv_and_update_weight
// and the push (src/context.rs:2326-2364)
__device__ __forceinline__ void push_or_add(Stk &s, uint32_t tv, uint32_t cv, uint32_t w, bool comp) {
  for (int i = 0; i < s.n; i++)
    if (s.t(i) == tv && (!comp || s.c(i) == cv)) {
      s.w(i) += w;
      return;
    }
  if (s.n < kStackMax) {
    s.set(s.n, tv, comp ? cv : 0u, w);
    s.n++;
  }
}

// add_ref_mv_candidate (src/context.rs:2366-2435)
__device__ __forceinline__ bool add_ref(Stk &s, const Cell &b, int rf0, int rf1, bool comp,
                                        uint32_t w, int &newmv) {
  if (b.r0 == kIntra) return false;  // Block::is_inter
  if (comp) {
    if (b.r0 != rf0 || b.r1 != rf1) return false;
    push_or_add(s, b.mv0, b.mv1, w, true);
    if (b.newmv) newmv++;
    return true;
  }
  bool found = false;
  if (b.r0 == rf0) {
    push_or_add(s, b.mv0, 0u, w, false);
    if (b.newmv) newmv++;
    found = true;
  }
  if (b.r1 == rf0) {
    push_or_add(s, b.mv1, 0u, w, false);
    if (b.newmv) newmv++;
    found = true;
  }
  return found;
}

// scan_row_mbmi (src/context.rs:2491-2555)
__device__ __forceinline__ bool scan_row(const Grid &t, int bx, int by, int row_offset,
                                         int max_row_offs, int &processed_rows, int rf0, int rf1,
                                         bool comp, Stk &s, int &newmv, int bw4) {
  const int end_mi = min(min(bw4, t.cols - bx), 16);
  int col_offset = 0;
  if (abs(row_offset) > 1) {
    col_offset = 1;
    if ((bx & 1) && bw4 < 2) col_offset -= 1;
  }
  const bool step16 = bw4 >= 16;
  bool found = false;
  for (int i = 0; i < end_mi;) {
    const Cell c = cell_at(t, bx + col_offset + i, by + row_offset);
    int len = min(bw4, c.n4w);
    if (step16)
      len = max(4, len);
    else if (abs(row_offset) > 1)
      len = max(len, 2);
    int weight = 2;
    if (bw4 >= 2 && bw4 <= c.n4w) {
      const int inc = min(-max_row_offs + row_offset + 1, c.n4h);
      weight = max(weight, inc);
      processed_rows = inc - row_offset - 1;
    }
    if (add_ref(s, c, rf0, rf1, comp, (uint32_t)(len * weight), newmv)) found = true;
    i += len;
  }
  return found;
}

// scan_col_mbmi (src/context.rs:2557-2621)
__device__ __forceinline__ bool scan_col(const Grid &t, int bx, int by, int col_offset,
                                         int max_col_offs, int &processed_cols, int rf0, int rf1,
                                         bool comp, Stk &s, int &newmv, int bh4) {
  const int end_mi = min(min(bh4, t.rows - by), 16);
  int row_offset = 0;
  if (abs(col_offset) > 1) {
    row_offset = 1;
    if ((by & 1) && bh4 < 2) row_offset -= 1;
  }
  const bool step16 = bh4 >= 16;
  bool found = false;
  for (int i = 0; i < end_mi;) {
    const Cell c = cell_at(t, bx + col_offset, by + row_offset + i);
    int len = min(bh4, c.n4h);
    if (step16)
      len = max(4, len);
    else if (abs(col_offset) > 1)
      len = max(len, 2);
    int weight = 2;
    if (bh4 >= 2 && bh4 <= c.n4h) {
      const int inc = min(-max_col_offs + col_offset + 1, c.n4w);
      weight = max(weight, inc);
      processed_cols = inc - col_offset - 1;
    }
    if (add_ref(s, c, rf0, rf1, comp, (uint32_t)(len * weight), newmv)) found = true;
    i += len;
  }
  return found;
}

// scan_blk_mbmi (src/context.rs:2623-2642)
__device__ __forceinline__ bool scan_blk(const Grid &t, int x, int y, int rf0, int rf1, bool comp,
                                         Stk &s, int &newmv) {
  if (x >= t.cols || y >= t.rows) return false;
  return add_ref(s, cell_at(t, x, y), rf0, rf1, comp, 2 * 2, newmv);
}

// has_tr (src/partition.rs:695-750), 64x64 superblocks
__device__ __forceinline__ bool has_tr(int bx, int by, int bw4, int bh4) {
  const int mask_row = by & 15, mask_col = bx & 15;
  int bs = max(bw4, bh4);
  if (bs > 16) return false;
  bool tr = !((mask_row & bs) && (mask_col & bs));
  while (bs < 16) {
    if (mask_col & bs) {
      if ((mask_col & (2 * bs)) && (mask_row & (2 * bs))) {
        tr = false;
        break;
      }
    } else {
      break;
    }
    bs <<= 1;
  }
  if (bw4 < bh4 && (bx & bw4) == 0) tr = true;
  if (bw4 > bh4 && (by & bh4) != 0) tr = false;
  return tr;
}

// find_valid_row_offs / find_valid_col_offs (src/context.rs:2308-2324)
__device__ __forceinline__ int valid_offs(int off, int mi, int n) { return min(max(off, -mi), n - mi - 1); }

__device__ __forceinline__ bool sign_of(uint32_t sbias, int r) { return (sbias >> ((r - 1) & 31)) & 1u; }

// The compound extra search's lists of one reference list (add_extra_mv_candidate,
// src/context.rs:2437-2489): up to two same-reference MVs and two others,
// in named words (a run-time index into a private array would be scratch)
struct ExtraList {
  uint32_t id0 = 0, id1 = 0, df0 = 0, df1 = 0;
  int idc = 0, dfc = 0;
  __device__ __forceinline__ void add(int cr, uint32_t m, int rf, uint32_t sbias) {
    if (cr == rf && idc < 2) {
      if (idc == 0) id0 = m; else id1 = m;
      idc++;
    } else if (dfc < 2) {
      const uint32_t v = sign_of(sbias, cr) != sign_of(sbias, rf) ? mv_neg(m) : m;
      if (dfc == 0) df0 = v; else df1 = v;
      dfc++;
    }
  }
  // combined_mvs[0] / [1] of the list: the same-reference MVs, then the others
  __device__ __forceinline__ uint32_t comb0() const { return idc > 0 ? id0 : dfc > 0 ? df0 : 0u; }
  __device__ __forceinline__ uint32_t comb1() const {
    if (idc > 1) return id1;
    if (idc == 1) return dfc > 0 ? df0 : 0u;
    return dfc > 1 ? df1 : 0u;
  }
};

// setup_mvref_list for a valid query: the stack into s (sorted, completed,
// clamped), the mode context returned
__device__ __forceinline__ int mvrefs(const Grid &t, const rv_mvref_tile &tl, int fcols, int frows,
                                      uint32_t sbias, int bx, int by, int bw4, int bh4, int rf0,
                                      int rf1, Stk &s) {
  s.n = 0;
  if (rf0 == kIntra) return 0;  // find_mvrefs, :2957-2962
  const bool comp = rf1 != kNone;
  int max_row_offs = 0, max_col_offs = 0;
  // (the odd-position adjustments row_adj / col_adj are zero from 8x8 up)
  int processed_rows = 0, processed_cols = 0;
  const bool up = by > 0, left = bx > 0;
  if (up) max_row_offs = valid_offs(-2 * kRowCols, by, t.rows);
  if (left) max_col_offs = valid_offs(-2 * kRowCols, bx, t.cols);
  bool row_match = false, col_match = false;
  int newmv = 0;
  if (abs(max_row_offs) >= 1)
    row_match |= scan_row(t, bx, by, -1, max_row_offs, processed_rows, rf0, rf1, comp, s, newmv, bw4);
  if (abs(max_col_offs) >= 1)
    col_match |= scan_col(t, bx, by, -1, max_col_offs, processed_cols, rf0, rf1, comp, s, newmv, bh4);
  if (has_tr(bx, by, bw4, bh4) && by > 0)
    row_match |= scan_blk(t, bx + bw4, by - 1, rf0, rf1, comp, s, newmv);
  const int nearest_match = (int)row_match + (int)col_match;
  for (int i = 0; i < s.n; i++) s.w(i) += kRefCatLevel;  // add_offset
  int far_newmv = 0;
  if (bx > 0 && by > 0) row_match |= scan_blk(t, bx - 1, by - 1, rf0, rf1, comp, s, far_newmv);
  for (int idx = 2; idx <= kRowCols; idx++) {
    const int off = -2 * idx + 1;
    if (abs(off) <= abs(max_row_offs) && abs(off) > processed_rows)
      row_match |= scan_row(t, bx, by, off, max_row_offs, processed_rows, rf0, rf1, comp, s, far_newmv, bw4);
    if (abs(off) <= abs(max_col_offs) && abs(off) > processed_cols)
      col_match |= scan_col(t, bx, by, off, max_col_offs, processed_cols, rf0, rf1, comp, s, far_newmv, bh4);
  }
  const int total_match = (int)row_match + (int)col_match;
  int mode_context;
  if (nearest_match == 0)
    mode_context = min(total_match, 1) + (total_match << 4);
  else if (nearest_match == 1)
    mode_context = 3 - min(newmv, 1) + ((2 + total_match) << 4);
  else
    mode_context = 5 - min(newmv, 1) + (5 << 4);
  // 7.10.2.11: sort by weight, descending, stable
  for (int i = 1; i < s.n; i++)
    for (int j = i; j > 0 && s.w(j) > s.w(j - 1); j--) {
      const uint32_t a = s.t(j), b = s.c(j), c = s.w(j);
      s.set(j, s.t(j - 1), s.c(j - 1), s.w(j - 1));
      s.set(j - 1, a, b, c);
    }
  if (s.n < 2) {
    // 7.10.2.12: the extra search over the row above, then the column to the left
    const int w4 = min(min(bw4, 16), t.cols - bx), h4 = min(min(bh4, 16), t.rows - by);
    const int num4x4 = min(w4, h4);
    ExtraList l0, l1;
    for (int pass = up ? 0 : 1; pass < (left ? 2 : 1); pass++) {
      for (int idx = 0; idx < num4x4 && s.n < 2;) {
        const Cell b = pass == 0 ? cell_at(t, bx + idx, by - 1) : cell_at(t, bx - 1, by + idx);
#pragma unroll
        for (int cl = 0; cl < 2; cl++) {
          const int cr = cl ? b.r1 : b.r0;
          const uint32_t m = cl ? b.mv1 : b.mv0;
          if (cr == kIntra || cr == kNone) continue;
          if (comp) {
            l0.add(cr, m, rf0, sbias);
            l1.add(cr, m, rf1, sbias);
          } else {
            const uint32_t v = sign_of(sbias, cr) != sign_of(sbias, rf0) ? mv_neg(m) : m;
            bool found = false;
            for (int i = 0; i < s.n; i++) found |= s.t(i) == v;
            if (!found) {
              s.set(s.n, v, 0u, 2u);
              s.n++;
            }
          }
        }
        idx += pass == 0 ? b.n4w : b.n4h;
      }
    }
    if (comp) {
      if (s.n == 1) {
        const bool same = l0.comb0() == s.t(0) && l1.comb0() == s.c(0);
        s.set(1, same ? l0.comb1() : l0.comb0(), same ? l1.comb1() : l1.comb0(), 2u);
      } else {
        s.set(0, l0.comb0(), l1.comb0(), 2u);
        s.set(1, l0.comb1(), l1.comb1(), 2u);
      }
      s.n = 2;
    }
  }
  // clamp (src/context.rs:2911-2941)
  const int fx = tl.mi_x + bx, fy = tl.mi_y + by;
  const int border_w = 128 + bw4 * 4 * 8, border_h = 128 + bh4 * 4 * 8;
  const int xmin = -fx * 32 - border_w, xmax = (fcols - fx - bw4) * 32 + border_w;
  const int ymin = -fy * 32 - border_h, ymax = (frows - fy - bh4) * 32 + border_h;
  for (int i = 0; i < s.n; i++) {
    s.t(i) = mv_clamp(s.t(i), xmin, xmax, ymin, ymax);
    s.c(i) = mv_clamp(s.c(i), xmin, xmax, ymin, ymax);
  }
  return mode_context;
}

__device__ __forceinline__ bool tile_ok(const rv_mvref_tile &t, const rv_mvref_geom &g) {
  return t.cols >= 1 && t.cols <= g.grid_w && t.rows >= 1 && t.rows <= g.grid_h && t.mi_x >= 0 &&
         t.mi_y >= 0 && t.mi_x <= (1 << 20) && t.mi_y <= (1 << 20);
}
__device__ __forceinline__ bool size_ok(int bw4, int bh4) {
  auto one = [](int v) { return v == 2 || v == 4 || v == 8 || v == 16; };
  return one(bw4) && one(bh4) && bw4 <= 2 * bh4 && bh4 <= 2 * bw4;
}

// The query's checks, then its tile; false: rejected
__device__ __forceinline__ bool query_ok(const rv_mvref_geom &g, const rv_mvref_tile *tiles,
                                         const rv_mv_blk *grid, int tile, int bx, int by, int bw4,
                                         int bh4, int rf0, int rf1, rv_mvref_tile &tl, Grid &t) {
  if (tile < 0 || tile >= g.n_tiles || !size_ok(bw4, bh4)) return false;
  if (rf0 < 0 || rf0 > 7 || rf1 < 1 || rf1 > 8) return false;
  tl = tiles[tile];
  if (!tile_ok(tl, g)) return false;
  if (bx < 0 || by < 0 || bx >= tl.cols || by >= tl.rows || (bx & (bw4 - 1)) || (by & (bh4 - 1)))
    return false;
  t.g = grid + (size_t)tile * g.grid_w * g.grid_h;
  t.gw = g.grid_w;
  t.gh = g.grid_h;
  t.cols = tl.cols;
  t.rows = tl.rows;
  return true;
}

__device__ __forceinline__ rv_mv mv_of(uint32_t m) { return rv_mv{(int16_t)(m & 0xFFFFu), (int16_t)(m >> 16)}; }

__device__ __forceinline__ void store_result(rv_mvref_result *r, int ctx, Stk &s) {
  r->mode_context = ctx;
  r->n = s.n;
  for (int i = 0; i < s.n; i++) r->stack[i] = rv_mv_cand{mv_of(s.t(i)), mv_of(s.c(i)), s.w(i)};
  for (int i = s.n; i < kSlots; i++) r->stack[i] = rv_mv_cand{rv_mv{0, 0}, rv_mv{0, 0}, 0u};
}

__global__ __launch_bounds__(kLanes) void mvstack_batch_kernel(const rv_mvref_query *q, int n,
                                                               rv_mvref_geom g,
                                                               const rv_mvref_tile *tiles,
                                                               const rv_mv_blk *grid,
                                                               rv_mvref_result *out,
                                                               uint32_t *status) {
  __shared__ uint32_t lds[kSlots * 3 * kLanes];
  const int i = blockIdx.x * kLanes + threadIdx.x;
  if (i >= n) return;
  const rv_mvref_query v = q[i];
  rv_mvref_tile tl;
  Grid t;
  if (!query_ok(g, tiles, grid, v.tile, v.bx, v.by, v.bw4, v.bh4, v.ref[0], v.ref[1], tl, t)) {
    atomicAdd(status, 1u);
    return;
  }
  Stk s{lds + threadIdx.x, 0};
  const int ctx = mvrefs(t, tl, g.frame_cols, g.frame_rows, g.sign_bias, v.bx, v.by, v.bw4, v.bh4,
                         v.ref[0], v.ref[1], s);
  store_result(out + i, ctx, s);
}

// BlockSize -> (width, height) in 4x4 units: BLOCK_4X4 .. BLOCK_64X64 and
// BLOCK_4X16 .. BLOCK_64X16; false for the 128 sizes and anything else
__device__ __forceinline__ bool bsize_n4(int bsize, int &w, int &h) {
  switch (bsize) {
    case 0: w = 1, h = 1; return true;
    case 1: w = 1, h = 2; return true;
    case 2: w = 2, h = 1; return true;
    case 3: w = 2, h = 2; return true;
    case 4: w = 2, h = 4; return true;
    case 5: w = 4, h = 2; return true;
    case 6: w = 4, h = 4; return true;
    case 7: w = 4, h = 8; return true;
    case 8: w = 8, h = 4; return true;
    case 9: w = 8, h = 8; return true;
    case 10: w = 8, h = 16; return true;
    case 11: w = 16, h = 8; return true;
    case 12: w = 16, h = 16; return true;
    case 16: w = 1, h = 4; return true;
    case 17: w = 4, h = 1; return true;
    case 18: w = 2, h = 8; return true;
    case 19: w = 8, h = 2; return true;
    case 20: w = 4, h = 16; return true;
    case 21: w = 16, h = 4; return true;
    default: w = h = 0; return false;
  }
}

// NEWMV, NEAREST_NEWMV, NEW_NEARESTMV, NEAR_NEWMV, NEW_NEARMV, NEW_NEWMV
// (PredictionMode 19, 22, 23, 24, 25, 27)
__device__ __forceinline__ bool is_newmv_mode(int m) {
  return m >= 0 && m < 32 && ((1u << m) & (1u << 19 | 1u << 22 | 1u << 23 | 1u << 24 | 1u << 25 | 1u << 27));
}

__device__ __forceinline__ bool paint_job_ok(const rv_ec_mode_job &j, const rv_mvref_geom &g,
                                             const rv_mvref_tile *tiles, rv_mvref_tile &tl, int &w,
                                             int &h) {
  if (j.tile < 0 || j.tile >= g.n_tiles || !bsize_n4(j.bsize, w, h)) return false;
  if (j.ref[0] < 0 || j.ref[0] > 8 || j.ref[1] < 0 || j.ref[1] > 8) return false;
  for (int k = 0; k < 4; k++)
    if (j.mv[k] < -32768 || j.mv[k] > 32767) return false;
  tl = tiles[j.tile];
  if (!tile_ok(tl, g)) return false;
  return j.bx >= 0 && j.by >= 0 && j.bx < tl.cols && j.by < tl.rows;
}

// Paint, pass 1: one lane per job, the largest job index of every cell it covers
__global__ __launch_bounds__(256) void mvstack_owner_kernel(const rv_ec_mode_job *jobs, int n,
                                                            rv_mvref_geom g,
                                                            const rv_mvref_tile *tiles, int *owner,
                                                            uint32_t *status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const rv_ec_mode_job j = jobs[i];
  if (j.kind != 0) return;
  rv_mvref_tile tl;
  int w, h;
  if (!paint_job_ok(j, g, tiles, tl, w, h)) {
    atomicAdd(status, 1u);
    return;
  }
  int *o = owner + (size_t)j.tile * g.grid_w * g.grid_h;
  const int xe = min(j.bx + w, tl.cols), ye = min(j.by + h, tl.rows);
  for (int y = j.by; y < ye; y++)
    for (int x = j.bx; x < xe; x++) atomicMax(o + (size_t)y * g.grid_w + x, i);
}

// Paint, pass 2: one lane per cell
__global__ __launch_bounds__(256) void mvstack_cell_kernel(const rv_ec_mode_job *jobs, int n,
                                                           size_t cells, const int *owner,
                                                           rv_mv_blk *grid) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  // Block::default(): ref {INTRA, INTRA}, 64x64, zero MVs
  uint4 v = make_uint4(16u << 16 | 16u << 24, 0u, 0u, 0u);
  const int i = owner[c];
  if (i >= 0 && i < n) {
    const rv_ec_mode_job j = jobs[i];
    int w = 16, h = 16;
    bsize_n4(j.bsize, w, h);
    v.x = ((uint32_t)j.ref[0] & 255u) | ((uint32_t)j.ref[1] & 255u) << 8 | (uint32_t)w << 16 |
          (uint32_t)h << 24;
    v.y = is_newmv_mode(j.luma_mode) ? 1u : 0u;
    v.z = ((uint32_t)j.mv[0] & 0xFFFFu) | ((uint32_t)j.mv[1] & 0xFFFFu) << 16;
    v.w = ((uint32_t)j.mv[2] & 0xFFFFu) | ((uint32_t)j.mv[3] & 0xFFFFu) << 16;
  }
  *reinterpret_cast<uint4 *>(grid + c) = v;
}

// Fill: one lane per job
__global__ __launch_bounds__(kLanes) void mvstack_fill_kernel(rv_ec_mode_job *jobs, int n,
                                                              rv_mvref_geom g,
                                                              const rv_mvref_tile *tiles,
                                                              const rv_mv_blk *grid,
                                                              rv_mvref_result *stacks,
                                                              uint32_t *status) {
  __shared__ uint32_t lds[kSlots * 3 * kLanes];
  const int i = blockIdx.x * kLanes + threadIdx.x;
  if (i >= n) return;
  rv_ec_mode_job *jp = jobs + i;
  const int kind = jp->kind, mode = jp->luma_mode;
  if (kind != 0 || mode < kNearestMv) return;  // a partition node, an intra block
  const int tile = jp->tile, bx = jp->bx, by = jp->by, rf0 = jp->ref[0], rf1 = jp->ref[1];
  int bw4, bh4;
  rv_mvref_tile tl;
  Grid t;
  if (!bsize_n4(jp->bsize, bw4, bh4) ||
      !query_ok(g, tiles, grid, tile, bx, by, bw4, bh4, rf0, rf1, tl, t)) {
    atomicAdd(status, 1u);
    return;
  }
  Stk s{lds + threadIdx.x, 0};
  const int ctx = mvrefs(t, tl, g.frame_cols, g.frame_rows, g.sign_bias, bx, by, bw4, bh4, rf0, rf1, s);
  jp->mode_context = ctx;
  jp->num_mv_found = s.n;
  for (int k = 0; k < 4; k++) jp->weight[k] = k < s.n ? (int32_t)s.w(k) : 0;
  const rv_mv t0 = s.n ? mv_of(s.t(0)) : rv_mv{0, 0}, c0 = s.n ? mv_of(s.c(0)) : rv_mv{0, 0};
  jp->ref_mv[0] = t0.row;
  jp->ref_mv[1] = t0.col;
  jp->ref_mv[2] = c0.row;
  jp->ref_mv[3] = c0.col;
  if (stacks) store_result(stacks + i, ctx, s);
}

// The checks the three entry points share, before any HIP call
bool args_ok(const void *items, int n, const rv_mvref_geom &g, const void *tiles, const void *grid,
             const void *status) {
  const bool dim_ok = g.grid_w >= 16 && g.grid_h >= 16 && g.grid_w <= 16384 && g.grid_h <= 16384 &&
                      g.grid_w % 16 == 0 && g.grid_h % 16 == 0;
  return n >= 0 && n <= (1 << 22) && g.n_tiles >= 1 && g.n_tiles <= 1024 && dim_ok &&
         (size_t)g.n_tiles * g.grid_w * g.grid_h <= ((size_t)1 << 28) && g.frame_cols >= 1 &&
         g.frame_rows >= 1 && g.frame_cols <= (1 << 20) && g.frame_rows <= (1 << 20) &&
         g.sign_bias <= 127u && tiles && grid && !((uintptr_t)grid & 15) && status && (!n || items);
}

}  // namespace
}  // namespace rv

using namespace rv;

extern "C" {

size_t rv_mvref_paint_scratch_bytes(rv_mvref_geom geom) {
  if (geom.n_tiles < 1 || geom.grid_w < 1 || geom.grid_h < 1) return 0;
  return (size_t)geom.n_tiles * geom.grid_w * geom.grid_h * sizeof(int);
}

int rv_mvref_grid_paint(const rv_ec_mode_job *d_jobs, int n, rv_mvref_geom geom,
                        const rv_mvref_tile *d_tiles, rv_mv_blk *d_grid, void *d_scratch,
                        uint32_t *d_status, void *stream) {
  if (!args_ok(d_jobs, n, geom, d_tiles, d_grid, d_status) || !d_scratch)
    return rv_set_error(RV_EINVAL, "rv_mvref_grid_paint: bad arguments");
  if (n == 0) return RV_OK;
  hipStream_t st = rv_resolve_stream(stream);
  const size_t cells = (size_t)geom.n_tiles * geom.grid_w * geom.grid_h;
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess ||
      hipMemsetAsync(d_scratch, 0xFF, cells * sizeof(int), st) != hipSuccess)
    return rv_set_error(RV_EHIP, "rv_mvref_grid_paint: clear");
  mvstack_owner_kernel<<<(n + 255) / 256, 256, 0, st>>>(d_jobs, n, geom, d_tiles, (int *)d_scratch,
                                                        d_status);
  mvstack_cell_kernel<<<(unsigned)((cells + 255) / 256), 256, 0, st>>>(d_jobs, n, cells,
                                                                       (const int *)d_scratch, d_grid);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

int rv_find_mvrefs_batch(const rv_mvref_query *d_queries, int n, rv_mvref_geom geom,
                         const rv_mvref_tile *d_tiles, const rv_mv_blk *d_grid,
                         rv_mvref_result *d_results, uint32_t *d_status, void *stream) {
  if (!args_ok(d_queries, n, geom, d_tiles, d_grid, d_status) || (n && !d_results))
    return rv_set_error(RV_EINVAL, "rv_find_mvrefs_batch: bad arguments");
  if (n == 0) return RV_OK;
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess)
    return rv_set_error(RV_EHIP, "rv_find_mvrefs_batch: clear");
  mvstack_batch_kernel<<<(n + kLanes - 1) / kLanes, kLanes, 0, st>>>(d_queries, n, geom, d_tiles,
                                                                    d_grid, d_results, d_status);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

int rv_ec_mode_fill_stacks(rv_ec_mode_job *d_jobs, int n, rv_mvref_geom geom,
                           const rv_mvref_tile *d_tiles, const rv_mv_blk *d_grid,
                           rv_mvref_result *d_stacks, uint32_t *d_status, void *stream) {
  if (!args_ok(d_jobs, n, geom, d_tiles, d_grid, d_status))
    return rv_set_error(RV_EINVAL, "rv_ec_mode_fill_stacks: bad arguments");
  if (n == 0) return RV_OK;
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess)
    return rv_set_error(RV_EHIP, "rv_ec_mode_fill_stacks: clear");
  mvstack_fill_kernel<<<(n + kLanes - 1) / kLanes, kLanes, 0, st>>>(d_jobs, n, geom, d_tiles, d_grid,
                                                                   d_stacks, d_status);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

}  // extern "C"

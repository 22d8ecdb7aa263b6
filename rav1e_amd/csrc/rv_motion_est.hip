// rv_motion_est.hip -- DiamondSearch::motion_estimation (src/me.rs:193-278,
// :391-463) of rdo_mode_decision (src/rdo.rs:858-878) for n blocks of one
// bsize x the single reference sets, in one launch, and save_block_motion
// (src/encoder.rs:1432-1444), which writes the field the searches read.
//
// One item is a (block, reference set).  Its whole chain stays on chip: the
// pmv pair from the MV stack (rdo.rs:859-865), get_mv_range (me.rs:64-80),
// get_subset_predictors (me.rs:82-174) into eleven fixed slots with a validity
// mask (rv_epzs.h keeps its sets the same way: nothing is indexed at run
// time), the full-pel diamond (me.rs:693-785, SAD, radius 16 -> 8) and the
// sub-pel diamond from the full-pel winner, which is handed over in
// registers (radius 4 -> 2, 1 under allow_hp; SATD under use_satd_subpel).
// No rv_ds_job record exists anywhere.
//
// No recost.  motion_estimation recomputes lowest_cost with SATD between the
// two searches (me.rs:232-253), but the sub-pel diamond_me_search starts with
// get_best_predictor, which resets the centre and its cost (me.rs:663-664)
// before it looks at anything: the recomputed value is never read.  It is
// not computed here.
//
// Lanes.  A candidate's block is cut into 8x8 chunks; a lane owns whole chunks
// (CPL of them in turn), so SATD's Hadamard runs inside the lane and the only
// exchanges are two short shuffle trees: a candidate's chunk sums over its C
// lanes, and the round's four costs over the item's 4 C lanes (the four
// candidates of a diamond step, or four predictors, run side by side as in
// ds_grp_kernel).  C = min(chunks, 16): an 8x8 item takes 4 lanes (16 items
// per wavefront), 16x8 / 8x16 take 8, 16x16 takes 16, 32x16 / 16x32 take 32
// and 32x32 upwards a whole wavefront.  Squares and rectangles go the same
// way.  Items of one wavefront diverge freely: a shuffle only reads lanes of
// its own item.  No LDS, no barrier.
#include <cstdio>

#include "rv_epzs.h"
#include "rv_mc.h"
#include "rv_me.h"

namespace rv {

// BlockSize in pixels (src/partition.rs:85-108 order), every size
constexpr uint8_t kMeBlkW[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kMeBlkH[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16};

constexpr int kMeMaxSets = 7;
constexpr int kMeSlots = 11;  // zero, coarse, left, top, top-right, mean, 5 of subset C

struct MeGeom {
  int32_t stride, width, height, xorigin, yorigin;
};
struct MeArgs {
  rv_plane org;
  MeGeom rg;                       // the reference planes' common geometry
  const void *refp[kMeMaxSets];    // luma plane of single set i
  int32_t ref_idx[kMeMaxSets];     // sets.ref[i].to_index()
  const rv_intra_tile *tiles;
  const rv_inter_blk *blocks;
  const rv_mvref_result *stacks;
  const rv_mv *cmv, *tile_mvs, *prev_mvs;
  rv_mv *me;
  rv_fs_result *res;
  uint32_t *status;
  int n_items, n_tiles, ns, nsets, w_in_b, h_in_b, hp, bd;
  uint32_t lambda;
};

// What a candidate's cost needs of the item, all in registers
struct MeItem {
  int px, py;  // the block's frame position (pixels)
  int mvx_min, mvx_max, mvy_min, mvy_max;
  rv_mv pmv0, pmv1;
};

template <typename T>
__device__ __forceinline__ T me_pick(T const (&tab)[kMeMaxSets], int i) {
  T p = tab[0];
#pragma unroll
  for (int s = 1; s < kMeMaxSets; s++) p = i == s ? tab[s] : p;
  return p;
}

__device__ __forceinline__ bool me_in_range(rv_mv mv, const MeItem &it) {
  return !(mv.col < it.mvx_min || mv.col > it.mvx_max || mv.row < it.mvy_min ||
           mv.row > it.mvy_max);
}

// compute_mv_rd_cost (src/me.rs:840-856) given the distortion
__device__ __forceinline__ uint64_t me_cost(uint32_t dist, rv_mv mv, const MeItem &it,
                                            uint32_t lambda, int hp) {
  const uint32_t r1 = ds_diff_to_rate((int16_t)(mv.row - it.pmv0.row), hp) +
                      ds_diff_to_rate((int16_t)(mv.col - it.pmv0.col), hp);
  const uint32_t r2 = ds_diff_to_rate((int16_t)(mv.row - it.pmv1.row), hp) +
                      ds_diff_to_rate((int16_t)(mv.col - it.pmv1.col), hp);
  const uint32_t rate = r1 < r2 + 1 ? r1 : r2 + 1;
  return 256ull * dist + (uint64_t)rate * lambda;
}

template <int W, int H>
struct MeLanes {
  static constexpr int NCX = W / 8;
  static constexpr int NCH = NCX * (H / 8);      // 8x8 chunks of a candidate
  static constexpr int C = NCH < 16 ? NCH : 16;  // lanes per candidate
  static constexpr int L = 4 * C;                // lanes per item
  static constexpr int CPL = NCH / C;            // chunks per lane
  static constexpr int IPW = 64 / L;             // items per wavefront
};

// The distortion of candidate mv, summed over the C lanes of its subgroup
// (lane c of it); ok = false: no pixel is read and the value is unused.
// Full-pel (SUB = false): SAD against the region at po + mv / 8.  Sub-pel:
// put_8tap REGULAR of predict_inter (src/predict.rs:255-338, PlaneSlice::clamp
// of the window's origin) and SAD, or get_satd's 8x8 Hadamards (src/dist.rs:
// 208-328) with one rounding of the block's sum.  The filter runs branch-free
// over the fractions: a zero fraction takes the identity taps (128 at tap 3),
// whose round trips through the two shifts are exact, so the four cases of
// put_8tap (src/mc.rs:213-274) come out bit for bit; the intermediates fit i16
// at 8 / 10 / 12 bit as ds_grp_kernel's do.
template <typename Px, int W, int H, bool SUB, bool SATD>
__device__ __forceinline__ uint32_t me_dist(const MeArgs &a, const Px *ref, const MeItem &it,
                                            rv_mv mv, bool ok, int c) {
  using G = MeLanes<W, H>;
  const MeGeom &g = a.rg;
  const int ib = a.bd == 12 ? 2 : 4, maxv = (1 << a.bd) - 1;
  uint32_t acc = 0;
  if (ok) {
    int cf = 0, rf = 0, sx, sy;
    if (SUB) {
      const int roff = (int)mv.row >> 3, coff = (int)mv.col >> 3;
      rf = ((int)mv.row - (roff << 3)) << 1;
      cf = ((int)mv.col - (coff << 3)) << 1;
      sx = clampi(it.px + coff - 3, -g.xorigin, g.width);  // window origin (-3, -3)
      sy = clampi(it.py + roff - 3, -g.yorigin, g.height);
    } else {
      sx = it.px + mv.col / 8;  // Rust `/` truncates toward zero
      sy = it.py + mv.row / 8;
    }
    const Px *rbase = ref + (int64_t)(g.yorigin + sy) * g.stride + g.xorigin + sx;
    // horizontal taps as i16 pairs for v_dot2: odd outputs (1,2) (3,4) (5,6),
    // even outputs (0,1) (2,3) (4,5) (6,7); REGULAR taps 0 and 7 are zero
    uint32_t xp[7];
    int32_t fy[8];
    if (SUB) {
      int32_t fx[8];
      const int8_t *xf = kSubpel[0][cf];
      const int8_t *yf = kSubpel[0][rf];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        fx[u] = cf ? (int32_t)xf[u] : (u == 3 ? 128 : 0);
        fy[u] = rf ? (int32_t)yf[u] : (u == 3 ? 128 : 0);
      }
      auto pk = [](int lo, int hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16); };
      xp[0] = pk(fx[1], fx[2]), xp[1] = pk(fx[3], fx[4]), xp[2] = pk(fx[5], fx[6]);
      xp[3] = pk(fx[0], fx[1]), xp[4] = pk(fx[2], fx[3]), xp[5] = pk(fx[4], fx[5]);
      xp[6] = pk(fx[6], fx[7]);
    }
    const int32_t hround = (1 << (7 - ib)) >> 1, vround = (1 << (7 + ib)) >> 1;
#pragma unroll 1
    for (int j = 0; j < G::CPL; j++) {
      const int q = c + j * G::C;
      const int x0 = (q % G::NCX) * 8, y0 = (q / G::NCX) * 8;
      const Px *o0 = plane_ptr<Px>(a.org, it.px + x0, it.py + y0);
      const Px *r0 = rbase + (int64_t)y0 * g.stride + x0;
      if (!SUB) {  // 8-pixel rows: unaligned vector loads + v_sad
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const Px *o = o0 + (int64_t)i * a.org.stride, *r = r0 + (int64_t)i * g.stride;
          if constexpr (sizeof(Px) == 1) {
            uint2 ov, rv;
            __builtin_memcpy(&ov, o, 8);
            __builtin_memcpy(&rv, r, 8);
            acc = __builtin_amdgcn_sad_u8(ov.x, rv.x, acc);
            acc = __builtin_amdgcn_sad_u8(ov.y, rv.y, acc);
          } else {
            uint4 ov, rv;
            __builtin_memcpy(&ov, o, 16);
            __builtin_memcpy(&rv, r, 16);
            acc = __builtin_amdgcn_sad_u16(ov.x, rv.x, acc);
            acc = __builtin_amdgcn_sad_u16(ov.y, rv.y, acc);
            acc = __builtin_amdgcn_sad_u16(ov.z, rv.z, acc);
            acc = __builtin_amdgcn_sad_u16(ov.w, rv.w, acc);
          }
        }
      } else {
        // output rows 0 .. 7 take window rows 1 .. 13 (taps 1 .. 6): the
        // horizontal pass streams row by row into the rows' vertical sums
        int32_t v[8][8];
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
          for (int t = 0; t < 8; t++) v[i][t] = vround;
#pragma unroll
        for (int m = 1; m < 14; m++) {
          const Px *w = r0 + (int64_t)m * g.stride;
          uint32_t pp[7];  // pixel pairs (2j, 2j + 1) as packed i16, pixels 0 .. 13
          if constexpr (sizeof(Px) == 1) {
            uint4 lv;
            __builtin_memcpy(&lv, w, 16);
            const uint32_t wd[4] = {lv.x, lv.y, lv.z, lv.w};
#pragma unroll
            for (int jj = 0; jj < 7; jj++)
              pp[jj] = __builtin_amdgcn_perm(0u, wd[jj >> 1], jj & 1 ? 0x0c030c02u : 0x0c010c00u);
          } else {
            uint4 v0, v1;
            __builtin_memcpy(&v0, w, 16);
            __builtin_memcpy(&v1, w + 8, 16);
            const uint32_t wd[7] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z};
#pragma unroll
            for (int jj = 0; jj < 7; jj++) pp[jj] = wd[jj];
          }
          int32_t mid[8];
#pragma unroll
          for (int t = 0; t < 8; t++) {
            int32_t hs = hround;
            if (t & 1) {
#pragma unroll
              for (int u = 0; u < 3; u++) hs = dot2_i16(pp[(t + 1) / 2 + u], xp[u], hs);
            } else {
#pragma unroll
              for (int u = 0; u < 4; u++) hs = dot2_i16(pp[t / 2 + u], xp[3 + u], hs);
            }
            mid[t] = hs >> (7 - ib);
          }
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const int kk = m - i;
            if (kk >= 1 && kk < 7) {
#pragma unroll
              for (int t = 0; t < 8; t++) v[i][t] += __mul24(fy[kk], mid[t]);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const Px *o = o0 + (int64_t)i * a.org.stride;
#pragma unroll
          for (int t = 0; t < 8; t++) v[i][t] = (int32_t)o[t] - clampi(v[i][t] >> (7 + ib), 0, maxv);
        }
        if (SATD) {
#pragma unroll
          for (int i = 0; i < 8; i++) had1d<8>(&v[i][0], 1);  // rows
#pragma unroll
          for (int t = 0; t < 8; t++) had1d<8>(&v[0][t], 8);  // columns
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
          for (int t = 0; t < 8; t++) acc += (uint32_t)(v[i][t] < 0 ? -v[i][t] : v[i][t]);
      }
    }
  }
#pragma unroll
  for (int m = G::C / 2; m; m >>= 1) acc += __shfl_xor(acc, m, 64);
  return SUB && SATD ? (acc + 4) >> 3 : acc;  // get_satd: (sum + (1 << ln >> 1)) >> ln, ln = 3
}

// diamond_me_search (src/me.rs:693-785): get_best_predictor over the valid
// ones of NS predictor slots in slot order, four to a round, then the diamond
// steps; the round loop and its exactness arguments are ds_grp_kernel's.
// (k, c): this lane's candidate subgroup and its lane in it; gbase: the
// item's first lane.  center / center_cost: out.
template <typename Px, int W, int H, bool SUB, bool SATD, int NS>
__device__ __forceinline__ void me_diamond(const MeArgs &a, const Px *ref, const MeItem &it,
                                           const rv_mv (&slot)[NS], uint32_t valid, int k, int c,
                                           int gbase, rv_mv &center, uint64_t &center_cost) {
  using G = MeLanes<W, H>;
  center = rv_mv{0, 0};
  center_cost = ~0ull;
  const int np = __popc(valid);
  int16_t radius = SUB ? 4 : 16;
  const int16_t radius_end = SUB ? (a.hp ? 1 : 2) : 8;
  int p0 = 0, back = -1;
  // Every diamond move strictly lowers center_cost, so the loop ends; the
  // bound only guarantees the grid drains whatever the inputs.
  for (int iter = 0; iter < 4096 + NS; iter++) {
    const bool pred_phase = p0 < np;
    rv_mv c4[4];
    int n;
    if (pred_phase) {
      n = np - p0 < 4 ? np - p0 : 4;
      // list position p0 + kk: the valid slot with that many valid slots
      // below it (a selection over static indices)
#pragma unroll
      for (int kk = 0; kk < 4; kk++) c4[kk] = rv_mv{0, 0};
#pragma unroll
      for (int i = 0; i < NS; i++) {
        const bool v = (valid >> i) & 1;
        const int pos = __popc(valid & ((1u << i) - 1)) - p0;
#pragma unroll
        for (int kk = 0; kk < 4; kk++)
          if (v && pos == kk) c4[kk] = slot[i];
      }
    } else {
      n = 4;
      c4[0] = rv_mv{(int16_t)(center.row + radius), center.col};  // diamond_pattern
      c4[1] = rv_mv{center.row, (int16_t)(center.col + radius)};
      c4[2] = rv_mv{(int16_t)(center.row - radius), center.col};
      c4[3] = rv_mv{center.row, (int16_t)(center.col - radius)};
    }
    const int skip = pred_phase ? -1 : back;
    rv_mv mine = c4[0];
#pragma unroll
    for (int kk = 1; kk < 4; kk++)
      if (k == kk) mine = c4[kk];
    const bool okm = k < n && k != skip && me_in_range(mine, it);
    const uint32_t dv = me_dist<Px, W, H, SUB, SATD>(a, ref, it, mine, okm, c);
    const uint64_t cm = okm ? me_cost(dv, mine, it, a.lambda, a.hp) : ~0ull;
    const uint32_t lo = (uint32_t)cm, hi = (uint32_t)(cm >> 32);
    uint64_t best = ~0ull;
    int bp = 0;
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      const uint32_t l = __shfl(lo, gbase + kk * G::C, 64), h = __shfl(hi, gbase + kk * G::C, 64);
      const uint64_t cv = ((uint64_t)h << 32) | l;
      if (cv < best) {  // strict <: the first minimum, as the sequential scan
        best = cv;
        bp = kk;
      }
    }
    rv_mv bmv = c4[0];
#pragma unroll
    for (int kk = 1; kk < 4; kk++)
      if (bp == kk) bmv = c4[kk];
    if (pred_phase) {
      if (best < center_cost) {
        center = bmv;
        center_cost = best;
      }
      p0 += 4;
    } else if (center_cost <= best) {
      if (radius == radius_end) break;
      radius /= 2;
      back = -1;
    } else {
      // the step after a move contains the old centre again, whose cost the
      // move strictly undercut: it cannot win and is not evaluated
      back = center_cost != ~0ull ? (bp + 2) & 3 : -1;
      center = bmv;
      center_cost = best;
    }
  }
}

template <typename Px, int W, int H, bool SATD>
__global__ __launch_bounds__(256) void motion_est_kernel(MeArgs a) {
  using G = MeLanes<W, H>;
  const int lane = threadIdx.x & 63;
  const int gl = lane % G::L, k = gl / G::C, c = gl % G::C, gbase = lane - gl;
  const int item = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * G::IPW + lane / G::L;
  if (item >= a.n_items) return;  // whole items: a shuffle never reads a lane that left
  const int b = item / a.ns, i = item - b * a.ns;
  constexpr int bw4 = W / 4, bh4 = H / 4;

  // ---- the item's checks: a rejected item reads no pixel, writes nothing ----
  const rv_inter_blk blk = a.blocks[b];
  const rv_mvref_result *st = a.stacks + (int64_t)b * a.nsets + i;
  const int len = st->n;
  bool ok = blk.tile >= 0 && blk.tile < a.n_tiles && blk.bo_x >= 0 && blk.bo_y >= 0 &&
            blk.bo_x <= (1 << 20) && blk.bo_y <= (1 << 20) && blk.bo_x % bw4 == 0 &&
            blk.bo_y % bh4 == 0 && len >= 0 && len <= 9;
  rv_intra_tile tl = {};
  if (ok) {
    tl = a.tiles[blk.tile];
    // the tile inside the frame on 4x4 units, the block inside the tile
    // (so inside the frame: get_mv_range's usize subtraction cannot underflow)
    ok = tl.x >= 0 && tl.y >= 0 && tl.width > 0 && tl.height > 0 && (tl.x & 3) == 0 &&
         (tl.y & 3) == 0 && tl.x <= 4 * a.w_in_b - tl.width && tl.y <= 4 * a.h_in_b - tl.height &&
         4 * (blk.bo_x + bw4) <= tl.width && 4 * (blk.bo_y + bh4) <= tl.height;
  }
  if (!ok) {
    if (gl == 0) atomicAdd(a.status, 1u);
    return;
  }
  const int tx4 = tl.x >> 2, ty4 = tl.y >> 2, cols = tl.width >> 2;  // tile_mvs.cols()
  const int bx = blk.bo_x, by = blk.bo_y, fx4 = tx4 + bx, fy4 = ty4 + by;

  MeItem it;
  it.px = 4 * fx4, it.py = 4 * fy4;
  // get_mv_range (src/me.rs:64-80) of the frame block offset
  it.mvx_min = -fx4 * 32 - (128 + W * 8);
  it.mvx_max = (a.w_in_b - fx4 - bw4) * 32 + (128 + W * 8);
  it.mvy_min = -fy4 * 32 - (128 + H * 8);
  it.mvy_max = (a.h_in_b - fy4 - bh4) * 32 + (128 + H * 8);
  // the pmv pair (src/rdo.rs:859-865)
  const rv_mv z{0, 0};
  // Every conditional value below is loaded from an address that is valid
  // either way and then selected: `cond ? *p : zero` on structs becomes a
  // select between p and a private copy of zero, i.e. scratch and flat loads.
  const rv_mv e0 = st->stack[0].this_mv, e1 = st->stack[1].this_mv;
  it.pmv0 = len > 0 ? e0 : z;
  it.pmv1 = len > 1 ? e1 : z;

  // ---- get_subset_predictors (src/me.rs:82-174), fixed slots ----------------
  const int ridx = me_pick(a.ref_idx, i);
  rv_mv s[kMeSlots];
  uint32_t valid = 3;  // zero and the coarse MV are always pushed
  s[0] = z;
  s[1] = epzs_qfull(a.cmv[item]);
  {
    const rv_mv *tm = a.tile_mvs + ((int64_t)ridx * a.h_in_b + fy4) * a.w_in_b + fx4;
    // (bx < tile_mvs.cols() - 1 holds for every accepted item: a block of two
    // or more units inside its tile ends at cols at most.  Kept as written.)
    const bool hl = bx > 0, ht = by > 0, htr = ht && bx < cols - 1;
    const rv_mv vl = tm[hl ? -1 : 0], vt = tm[ht ? -a.w_in_b : 0], vtr = tm[htr ? 1 - a.w_in_b : 0];
    const rv_mv l = hl ? vl : z, t = ht ? vt : z, tr = htr ? vtr : z;
    s[2] = l, s[3] = t, s[4] = tr;
    valid |= (uint32_t)(hl && !epzs_zero(l)) << 2;
    valid |= (uint32_t)(ht && !epzs_zero(t)) << 3;
    valid |= (uint32_t)(htr && !epzs_zero(tr)) << 4;
    // the mean: MotionVector Add / Div<i16> (i16 arithmetic, truncating)
    const int nm = (int)hl + (int)ht + (int)htr;
    const int16_t sr = (int16_t)((int16_t)(l.row + t.row) + tr.row);
    const int16_t sc = (int16_t)((int16_t)(l.col + t.col) + tr.col);
    const int d = nm ? nm : 1;
    s[5] = epzs_qfull(rv_mv{(int16_t)(sr / d), (int16_t)(sc / d)});
    valid |= (uint32_t)(nm && !epzs_zero(s[5])) << 5;
  }
  if (a.prev_mvs) {  // subset C: the previous frame's field at 4x4 granularity
    const rv_mv *pm = a.prev_mvs + ((int64_t)ridx * a.h_in_b + fy4) * a.w_in_b + fx4;
    const bool cl = fx4 > 0, ct = fy4 > 0, cr = fx4 < a.w_in_b - 1, cb = fy4 < a.h_in_b - 1;
    const rv_mv vl = pm[cl ? -1 : 0], vt = pm[ct ? -a.w_in_b : 0], vr = pm[cr ? 1 : 0],
                vb = pm[cb ? a.w_in_b : 0];
    s[6] = cl ? vl : z, s[7] = ct ? vt : z, s[8] = cr ? vr : z, s[9] = cb ? vb : z;
    s[10] = pm[0];
#pragma unroll
    for (int p = 6; p < kMeSlots; p++) valid |= (uint32_t)!epzs_zero(s[p]) << p;
  } else {
#pragma unroll
    for (int p = 6; p < kMeSlots; p++) s[p] = z;
  }
  const Px *ref = (const Px *)me_pick(a.refp, i);
  rv_mv best;
  uint64_t cost;
  me_diamond<Px, W, H, false, false, kMeSlots>(a, ref, it, s, valid, k, c, gbase, best, cost);
  const rv_mv one[1] = {best};  // the full-pel winner, sub_pixel_me's only predictor (me.rs:441)
  me_diamond<Px, W, H, true, SATD, 1>(a, ref, it, one, 1u, k, c, gbase, best, cost);
  if (gl == 0) {
    a.me[item] = best;
    if (a.res) {
      rv_fs_result r;
      r.best_mv = best, r.reserved = 0, r.cost = cost;
      a.res[item] = r;
    }
  }
}


// ---- save_block_motion -------------------------------------------------------
// Two passes over (job, cell): the latest job that covers a cell claims it
// (atomicMax of the job's index into the scratch grid), then each job writes
// the cells it owns -- the result of running the list in order.
struct SbmArgs {
  const rv_me_save_job *jobs;
  const rv_intra_tile *tiles;
  rv_mv *field;
  int32_t *owner;
  uint32_t *status;
  int n, n_tiles, w_in_b, h_in_b;
};

// The job's clipped rectangle on frame 4x4 units; false: skipped or rejected
__device__ __forceinline__ bool sbm_rect(const SbmArgs &a, const rv_me_save_job &jb, bool count,
                                         int &x0, int &y0, int &x1, int &y1) {
  if (jb.ref_index < 0) return false;  // an intra winner (src/encoder.rs:2171)
  bool ok = jb.ref_index < 7 && jb.bsize >= 0 && jb.bsize < 22 && jb.tile >= 0 &&
            jb.tile < a.n_tiles && jb.bo_x >= 0 && jb.bo_y >= 0;
  rv_intra_tile tl = {};
  if (ok) {
    tl = a.tiles[jb.tile];
    ok = tl.x >= 0 && tl.y >= 0 && tl.width > 0 && tl.height > 0 && (tl.x & 3) == 0 &&
         (tl.y & 3) == 0 && tl.x <= 4 * a.w_in_b - tl.width && tl.y <= 4 * a.h_in_b - tl.height &&
         jb.bo_x < (tl.width >> 2) && jb.bo_y < (tl.height >> 2);
  }
  if (!ok) {
    if (count) atomicAdd(a.status, 1u);
    return false;
  }
  const int mi_w = tl.width >> 2, mi_h = tl.height >> 2;  // ts.mi_width / mi_height
  const int ex = jb.bo_x + (kMeBlkW[jb.bsize] >> 2), ey = jb.bo_y + (kMeBlkH[jb.bsize] >> 2);
  x0 = (tl.x >> 2) + jb.bo_x, y0 = (tl.y >> 2) + jb.bo_y;
  x1 = (tl.x >> 2) + (ex < mi_w ? ex : mi_w), y1 = (tl.y >> 2) + (ey < mi_h ? ey : mi_h);
  return true;
}

// One 64-lane group per job: the largest block is 32 x 32 cells
template <bool WRITE>
__global__ __launch_bounds__(256) void save_block_motion_kernel(SbmArgs a) {
  const int j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= a.n) return;
  const rv_me_save_job jb = a.jobs[j];
  int x0, y0, x1, y1;
  if (!sbm_rect(a, jb, !WRITE && lane == 0, x0, y0, x1, y1)) return;
  const int w = x1 - x0, cells = w * (y1 - y0);
  for (int i = lane; i < cells; i += 64) {
    const int64_t cell = ((int64_t)jb.ref_index * a.h_in_b + y0 + i / w) * a.w_in_b + x0 + i % w;
    if (!WRITE)
      atomicMax(a.owner + cell, j);
    else if (a.owner[cell] == j)
      a.field[cell] = jb.mv;
  }
}

static int me_fail(int code, const char *who, const char *what) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return rv_set_error(code, msg);
}

static bool me_sets_ok(const rv_inter_ref_sets &s) {
  if (s.n_single < 1 || s.n_single > 7 || (s.compound != 0 && s.compound != 1)) return false;
  for (int i = 0; i < s.n_single; i++)
    if (s.ref[i] < 1 || s.ref[i] > 7 || s.slot[i] < 0 || s.slot[i] > 7) return false;
  if (s.fwd < -1 || s.fwd >= s.n_single || s.bwd < -1 || s.bwd >= s.n_single) return false;
  if (s.compound && (s.fwd < 0 || s.bwd < 0)) return false;
  return true;
}

template <typename Px, bool SATD>
static bool me_launch(const MeArgs &a, int bw, int bh, hipStream_t st) {
#define RV_ME_CASE(W, H)                                                            \
  if (bw == W && bh == H) {                                                         \
    constexpr int ipw = MeLanes<W, H>::IPW;                                         \
    const unsigned grid = (unsigned)((a.n_items + 4 * ipw - 1) / (4 * ipw));        \
    motion_est_kernel<Px, W, H, SATD><<<grid, 256, 0, st>>>(a);                     \
    return true;                                                                    \
  }
  RV_ME_CASE(8, 8)
  RV_ME_CASE(8, 16)
  RV_ME_CASE(16, 8)
  RV_ME_CASE(16, 16)
  RV_ME_CASE(16, 32)
  RV_ME_CASE(32, 16)
  RV_ME_CASE(32, 32)
  RV_ME_CASE(32, 64)
  RV_ME_CASE(64, 32)
  RV_ME_CASE(64, 64)
#undef RV_ME_CASE
  return false;
}

}  // namespace rv

using namespace rv;

extern "C" int rv_me_pmv_index(int bsize, int bo_x, int bo_y) {
  // src/rdo.rs:1532-1536 compares in enum order, src/encoder.rs:2160-2166 with
  // BlockSize::greater_than: they agree on every size but the 4:1 / 1:4 ones
  if (bsize < 0 || bsize > 15) return -1;
  if (bsize > 9) return 0;  // above BLOCK_32X32
  return ((bo_x & 32) >> 5) + ((bo_y & 32) >> 4) + 1;
}

extern "C" int rv_motion_estimation_batch(const rv_plane *org, const rv_plane *refs, int n_refs,
                                          const rv_intra_tile *d_tiles, int n_tiles,
                                          const rv_inter_blk *d_blocks, int n,
                                          rv_inter_ref_sets sets, const rv_mvref_result *d_stacks,
                                          const rv_mv *d_cmv, const rv_mv *d_tile_mvs,
                                          const rv_mv *d_prev_mvs, const rv_me_params *params,
                                          rv_mv *d_me, rv_fs_result *d_res, uint32_t *d_status,
                                          void *stream) {
  const char *who = "rv_motion_estimation_batch";
  if (!params || !org || !refs || !d_status || n < 0 || n_tiles < 0)
    return me_fail(RV_EINVAL, who, "null argument or negative count");
  const rv_me_params &P = *params;
  if (P.bsize < 0 || P.bsize > 21) return me_fail(RV_EINVAL, who, "bsize is no BlockSize");
  const int bd = P.bit_depth;
  if (bd != 8 && bd != 10 && bd != 12) return me_fail(RV_EINVAL, who, "bit_depth must be 8, 10 or 12");
  if (n_refs < 1 || n_refs > 8) return me_fail(RV_EINVAL, who, "n_refs is 1 .. 8");
  if (!me_sets_ok(sets)) return me_fail(RV_EINVAL, who, "sets is no rv_inter_ref_sets_build result");
  if (P.w_in_b < 1 || P.h_in_b < 1 || P.w_in_b > (1 << 14) || P.h_in_b > (1 << 14))
    return me_fail(RV_EINVAL, who, "w_in_b / h_in_b outside 1 .. 2^14");
  if (n > (1 << 22)) return me_fail(RV_EINVAL, who, "n above 2^22");
  const int bw = kMeBlkW[P.bsize], bh = kMeBlkH[P.bsize];
  if (P.bsize > 12)
    return me_fail(RV_ENOTSUP, who, "4:1 / 1:4 partitions and sizes above 64x64 are not supported");
  if (bw == 4 || bh == 4) return me_fail(RV_ENOTSUP, who, "4xN / Nx4 partitions are not supported");

  MeArgs a = {};
  if (!org->data || org->hbd != (bd > 8) || org->xdec || org->ydec)
    return me_fail(RV_EINVAL, who, "the source plane: no data, subsampled, or a pixel type that does not fit bit_depth");
  if (org->stride <= 0 || org->xorigin < 0 || org->yorigin < 0 ||
      (int64_t)org->stride - org->xorigin < 4 * (int64_t)P.w_in_b ||
      (int64_t)org->alloc_height - org->yorigin < 4 * (int64_t)P.h_in_b)
    return me_fail(RV_EINVAL, who, "the source plane does not hold the frame");
  const rv_plane &g0 = refs[0];
  for (int i = 0; i < sets.n_single; i++) {
    if (sets.slot[i] >= n_refs) return me_fail(RV_EINVAL, who, "a reference set's slot is not in refs");
    const rv_plane &pl = refs[3 * sets.slot[i]];
    if (!pl.data) return me_fail(RV_EINVAL, who, "a plane without data");
    if (pl.hbd != (bd > 8) || pl.xdec || pl.ydec)
      return me_fail(RV_EINVAL, who, "a reference plane is subsampled or its pixel type does not fit bit_depth");
    if (pl.stride != g0.stride || pl.alloc_height != g0.alloc_height || pl.width != g0.width ||
        pl.height != g0.height || pl.xorigin != g0.xorigin || pl.yorigin != g0.yorigin)
      return me_fail(RV_EINVAL, who, "the reference planes differ in geometry");
    a.refp[i] = pl.data;
    a.ref_idx[i] = sets.ref[i] - 1;
  }
  for (int i = sets.n_single; i < kMeMaxSets; i++) a.refp[i] = a.refp[0], a.ref_idx[i] = a.ref_idx[0];
  if (g0.stride <= 0 || g0.alloc_height <= 0 || g0.width <= 0 || g0.height <= 0 || g0.xorigin < 0 ||
      g0.yorigin < 0)
    return me_fail(RV_EINVAL, who, "a plane's geometry is not positive");
  // Full-pel: get_mv_range lets a candidate's region start 16 + w pixels left
  // of / above the frame and end as far right of / below it.  Sub-pel:
  // PlaneSlice::clamp leaves the window's origin in [-xorigin, width] x
  // [-yorigin, height]; the filter reads 14 rows of 16 pixels per 8x8 chunk.
  const int64_t fw = 4 * (int64_t)P.w_in_b, fh = 4 * (int64_t)P.h_in_b;
  if (g0.xorigin < 16 + bw || g0.yorigin < 16 + bh || (int64_t)g0.stride - g0.xorigin < fw + 16 + bw ||
      (int64_t)g0.alloc_height - g0.yorigin < fh + 16 + bh ||
      (int64_t)g0.xorigin + g0.width + bw + 8 > g0.stride ||
      (int64_t)g0.yorigin + g0.height + bh + 7 > g0.alloc_height)
    return me_fail(RV_EINVAL, who, "a reference plane's padding does not hold the furthest clamped sub-pel window");
  if (n > 0 && (!d_tiles || n_tiles == 0 || !d_blocks || !d_stacks || !d_cmv || !d_tile_mvs || !d_me))
    return me_fail(RV_EINVAL, who, "null argument");

  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess) return rv_set_hip_error(hipGetLastError(), who);
  if (n == 0) return RV_OK;
  a.org = *org;
  a.rg = MeGeom{g0.stride, g0.width, g0.height, g0.xorigin, g0.yorigin};
  a.tiles = d_tiles, a.blocks = d_blocks, a.stacks = d_stacks;
  a.cmv = d_cmv, a.tile_mvs = d_tile_mvs, a.prev_mvs = d_prev_mvs;
  a.me = d_me, a.res = d_res, a.status = d_status;
  a.ns = sets.n_single, a.nsets = sets.n_single + sets.compound, a.n_items = n * a.ns;
  a.n_tiles = n_tiles, a.w_in_b = P.w_in_b, a.h_in_b = P.h_in_b;
  a.hp = P.allow_hp != 0, a.bd = bd, a.lambda = P.lambda;
  const bool launched = bd > 8 ? (P.use_satd ? me_launch<uint16_t, true>(a, bw, bh, st)
                                             : me_launch<uint16_t, false>(a, bw, bh, st))
                               : (P.use_satd ? me_launch<uint8_t, true>(a, bw, bh, st)
                                             : me_launch<uint8_t, false>(a, bw, bh, st));
  if (!launched) return me_fail(RV_ENOTSUP, who, "no kernel for this block size");
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" size_t rv_save_block_motion_scratch_bytes(int w_in_b, int h_in_b) {
  if (w_in_b < 1 || h_in_b < 1 || w_in_b > (1 << 14) || h_in_b > (1 << 14)) return 0;
  return (size_t)7 * w_in_b * h_in_b * sizeof(int32_t);
}

extern "C" int rv_save_block_motion_batch(const rv_me_save_job *d_jobs, int n,
                                          const rv_intra_tile *d_tiles, int n_tiles, int w_in_b,
                                          int h_in_b, rv_mv *d_tile_mvs, void *d_scratch,
                                          uint32_t *d_status, void *stream) {
  const char *who = "rv_save_block_motion_batch";
  if (!d_status || n < 0 || n > (1 << 22) || n_tiles < 0)
    return me_fail(RV_EINVAL, who, "null status, or a count that is negative or above 2^22");
  const size_t sb = rv_save_block_motion_scratch_bytes(w_in_b, h_in_b);
  if (!sb) return me_fail(RV_EINVAL, who, "w_in_b / h_in_b outside 1 .. 2^14");
  if (n > 0 && (!d_jobs || !d_tiles || n_tiles == 0 || !d_tile_mvs || !d_scratch))
    return me_fail(RV_EINVAL, who, "null argument");
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess) return rv_set_hip_error(hipGetLastError(), who);
  if (n == 0) return RV_OK;
  if (hipMemsetAsync(d_scratch, 0xFF, sb, st) != hipSuccess)  // every owner -1
    return rv_set_hip_error(hipGetLastError(), who);
  SbmArgs a = {d_jobs, d_tiles, d_tile_mvs, (int32_t *)d_scratch, d_status, n, n_tiles, w_in_b, h_in_b};
  const unsigned grid = (unsigned)((n + 3) / 4);
  save_block_motion_kernel<false><<<grid, 256, 0, st>>>(a);
  save_block_motion_kernel<true><<<grid, 256, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

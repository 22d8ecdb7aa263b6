// rv_ec_mode_sym.h -- the symbol-forming device functions of the block mode
// info (encode_block_pre_cdef, encode_block_post_cdef's symbols,
// write_partition), shared by the tokenizer of committed blocks
// (rv_ec_mode.hip: the restrictions, the map's record layout and the token
// format are described there) and the tokenizer of RDO candidates
// (rv_ec_cand.hip).  mode_symbols only reads the neighbour-record map.
#pragma once

#include "rv_device.h"
#include "rv_ec.h"
#include "rv_ec_tables.h"
#include "rv_ec_mode_tables.h"

namespace rv {

constexpr int kNearestMv = 14, kNear0Mv = 15, kNear2Mv = 17, kGlobalMv = 18, kNewMv = 19;
constexpr int kNearestNearestMv = 20, kNearNearMv = 21, kNearestNewMv = 22, kNewNearestMv = 23;
constexpr int kNearNewMv = 24, kNewNearMv = 25, kNewNewMv = 27;
constexpr int kUvCfl = 13, kVPred = 1, kD63Pred = 8;
constexpr int kRefCatLevel = 640;  // REF_CAT_LEVEL (src/context.rs:90)

// intra_mode_context (src/context.rs:2206-2207)
__constant__ uint8_t kIntraModeContext[13] = {0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0};

struct ModeArgs {
  const rv_ec_mode_job *jobs;
  int n;
  rv_ec_mode_params prm;
  int n_tiles;
  const int32_t *tile_dims;  // [n_tiles][2] cols, rows (luma 4x4 units)
  const uint32_t *map;  // read only here; mode_prep_kernel stores through its own pointer
  int map_w8, map_h8;
  uint32_t *count;  // [n] token counts, then exclusive offsets [n + 1]
  uint32_t *tokens;
  uint32_t cap;
  uint32_t *status;  // [0] total tokens, [1] overflow flag, [2] rejected jobs
};

__device__ inline int bsize_lg(int bsize) {  // BLOCK_8X8 3, 16X16 6, 32X32 9, 64X64 12
  return bsize == 3 ? 3 : bsize == 6 ? 4 : bsize == 9 ? 5 : bsize == 12 ? 6 : 0;
}
__device__ inline bool mode_has_near(int m) {
  return (m >= kNear0Mv && m <= kNear2Mv) || m == kNearNearMv || m == kNearNewMv || m == kNewNearMv;
}
__device__ inline int near_ref_mv_idx(int m) {
  return (m >= kNear0Mv && m <= kNear2Mv) ? m - kNear0Mv + 1 : 1;
}
__device__ inline bool mv_coded(int m, int k) {  // src/encoder.rs:1567-1577
  return k == 0 ? (m == kNewMv || m == kNewNewMv || m == kNewNearestMv)
                : (m == kNewNewMv || m == kNearestNewMv);
}

// The restrictions of the header comment; cols / rows: the job's tile.
__device__ bool mode_job_ok(const rv_ec_mode_job &j, const ModeArgs &a, int &cols, int &rows) {
  if ((j.kind != 0 && j.kind != 1) || j.tile < 0 || j.tile >= a.n_tiles) return false;
  const int lg = bsize_lg(j.bsize);
  if (!lg) return false;
  cols = a.tile_dims[2 * j.tile];
  rows = a.tile_dims[2 * j.tile + 1];
  if (cols < 2 || rows < 2 || ((cols | rows) & 1) || cols > 2 * a.map_w8 || rows > 2 * a.map_h8)
    return false;
  const int n4 = 1 << (lg - 2);
  if (j.bx < 0 || j.by < 0 || j.bx >= cols || j.by >= rows || ((j.bx | j.by) & (n4 - 1)))
    return false;
  if (j.kind == 1) {
    if (j.partition != 0 && j.partition != 3) return false;
    const int hbs = n4 >> 1;
    if ((j.bx + hbs < cols) != (j.by + hbs < rows)) return j.partition == 3 && lg > 3;
    return true;
  }
  if ((j.skip & ~1) || j.seg_idx < 0 || j.seg_idx > 7) return false;
  if (a.prm.seg_enabled && (a.prm.last_active_segid < 0 || a.prm.last_active_segid > 7 ||
                            j.seg_idx > a.prm.last_active_segid))
    return false;
  const int lm = j.luma_mode, cm = j.chroma_mode;
  if (lm < 0 || lm > 27 || lm == kUvCfl) return false;
  if (lm < kNearestMv) {
    if (cm < 0 || cm > kUvCfl || j.ref[0] != 0 || (j.ref[1] != 0 && j.ref[1] != 8)) return false;
    if (cm == kUvCfl) {
      const int js = j.cfl_joint_sign;
      if (lg > 5 || js < 0 || js > 7) return false;
      const int su = (js + 1) / 3, sv = (js + 1) % 3;
      if (su && (j.cfl_scale[0] < 1 || j.cfl_scale[0] > 16)) return false;
      if (sv && (j.cfl_scale[1] < 1 || j.cfl_scale[1] > 16)) return false;
    }
    return true;
  }
  if (a.prm.frame_type != 1 || cm != lm) return false;
  const int ctx = j.mode_context;
  if (ctx < 0 || (ctx & 7) > 6 || ((ctx >> 4) & 15) > 5) return false;
  if (j.num_mv_found < 0 || j.num_mv_found > 9) return false;
  if (lm >= kNearestNearestMv) {
    if (!a.prm.reference_mode || j.ref[0] < 1 || j.ref[0] > 4 || j.ref[1] < 5 || j.ref[1] > 7)
      return false;
  } else if (j.ref[0] < 1 || j.ref[0] > 7 || (j.ref[1] != 0 && j.ref[1] != 8)) {
    return false;
  }
  if (lm == kNewNewMv && j.num_mv_found < 2) return false;
  if (mode_has_near(lm) && lm != kNear0Mv && j.num_mv_found <= near_ref_mv_idx(lm)) return false;
#pragma unroll
  for (int k = 0; k < 2; k++)
    if (mv_coded(lm, k)) {
      // 64-bit: the fields are unchecked int32 until here
      const long long dr = (long long)j.mv[2 * k] - j.ref_mv[2 * k];
      const long long dc = (long long)j.mv[2 * k + 1] - j.ref_mv[2 * k + 1];
      if (dr < -(1 << 14) || dr > (1 << 14) || dc < -(1 << 14) || dc > (1 << 14)) return false;
    }
  return true;
}

struct CountSink {
  uint32_t n = 0;
  __device__ inline void put(uint32_t) { n++; }
};
struct WriteSink {
  uint32_t *t;
  uint32_t o, cap;
  uint32_t *status;
  __device__ inline void put(uint32_t v) {
    if (o < cap)
      t[o] = v;
    else
      status[1] = 1;
    o++;
  }
};

// neighbour record fields
__device__ inline int rec_skip(uint32_t r) { return r & 1; }
__device__ inline int rec_mode(uint32_t r) { return (r >> 1) & 31; }
__device__ inline int rec_ref0(uint32_t r) { return (r >> 6) & 15; }
__device__ inline int rec_ref1(uint32_t r) { return (r >> 10) & 15; }
__device__ inline int rec_seg(uint32_t r) { return (r >> 14) & 7; }
__device__ inline int rec_pc(uint32_t r) { return (r >> 17) & 31; }

__device__ inline int ref_count_ctx(int c0, int c1) { return c0 < c1 ? 0 : c0 == c1 ? 1 : 2; }
// neighbors_ref_counts as 7 nibbles (a run-time indexed array would live in scratch)
__device__ inline uint32_t ref_counts_add(uint32_t c, uint32_t rec) {
  if (rec_mode(rec) >= kNearestMv) {
    c += 1u << (4 * (rec_ref0(rec) - 1));
    const int r1 = rec_ref1(rec);
    if (r1 != 0 && r1 != 8) c += 1u << (4 * (r1 - 1));
  }
  return c;
}
__device__ inline int rc(uint32_t c, int ref) { return (c >> (4 * (ref - 1))) & 15; }
__device__ inline bool samedir(int r0, int r1) {  // is_samedir_ref_pair
  return (r0 >= 5 && r0 != 8) == (r1 >= 5 && r1 != 8);
}

// neg_interleave (src/context.rs:3507-3534)
__device__ inline int neg_interleave(int x, int r, int mx) {
  if (r == 0) return x;
  if (r >= mx - 1) return -x + mx - 1;
  const int diff = x - r, ad = diff < 0 ? -diff : diff;
  if (2 * r < mx) {
    if (ad <= r) return diff > 0 ? (diff << 1) - 1 : (-diff) << 1;
    return x;
  }
  if (ad < mx - r) return diff > 0 ? (diff << 1) - 1 : (-diff) << 1;
  return (mx - x) - 1;
}

// encode_mv_component (src/context.rs:4319-4370); precision -1 NONE, 0 LOW, 1 HIGH
template <class S>
__device__ inline void mv_component(S &s, int comp, int base, int precision) {
  const int sign = comp < 0;
  const uint32_t z = (uint32_t)(sign ? -comp : comp) - 1;
  const int c = z >= 8192u ? 10 : ((z >> 3) ? 31 - __clz((int)(z >> 3)) : 0);
  const uint32_t offset = z - (c ? (2u << (c + 2)) : 0u);
  const int d = (int)(offset >> 3), fr = (int)(offset >> 1) & 3, hp = (int)offset & 1;
  s.put(ec_sym(base + RV_ECM_MVC_SIGN, 3, sign));
  s.put(ec_sym(base + RV_ECM_MVC_CLASSES, 12, c));
  if (c == 0) {
    s.put(ec_sym(base + RV_ECM_MVC_CLASS0, 3, d));
  } else {
    for (int i = 0; i < c; i++) s.put(ec_sym(base + RV_ECM_MVC_BITS + 3 * i, 3, (d >> i) & 1));
  }
  if (precision > -1)
    s.put(ec_sym(base + (c == 0 ? RV_ECM_MVC_CLASS0_FP + 5 * d : RV_ECM_MVC_FP), 5, fr));
  if (precision > 0) s.put(ec_sym(base + (c == 0 ? RV_ECM_MVC_CLASS0_HP : RV_ECM_MVC_HP), 3, hp));
}

// A valid job's symbols in the reference's order.  The same function counts
// (CountSink: the neighbour values do not change the count) and writes.
template <class S>
__device__ inline void mode_symbols(const rv_ec_mode_job &j, const ModeArgs &a, int cols, int rows,
                                    S &s) {
  const int lg = bsize_lg(j.bsize), n4 = 1 << (lg - 2);
  const int x8 = j.bx >> 1, y8 = j.by >> 1;
  const bool has_above = j.by > 0, has_left = j.bx > 0;
  const uint32_t *m = a.map + (size_t)j.tile * a.map_w8 * a.map_h8;
  const uint32_t ra = has_above ? m[(size_t)(y8 - 1) * a.map_w8 + x8] : 0;
  const uint32_t rl = has_left ? m[(size_t)y8 * a.map_w8 + x8 - 1] : 0;
  if (j.kind == 1) {  // write_partition
    const int hbs = n4 >> 1, bsl = lg - 3;
    const bool has_cols = j.bx + hbs < cols, has_rows = j.by + hbs < rows;
    const int ctx = ((rec_pc(rl) >> bsl) & 1) * 2 + ((rec_pc(ra) >> bsl) & 1) + bsl * 4;
    const int off = RV_ECM_PARTITION + ctx * 11, len = lg == 3 ? 5 : 11;
    if (has_rows && has_cols)
      s.put(ec_sym(off, len, j.partition));
    else if (has_rows != has_cols)  // !has_rows: vert_alike (1), !has_cols: horz_alike (2)
      s.put(ec_edge(off, len, j.partition == 3, has_cols ? 1 : 2, bsl));
    return;
  }
  const int lm = j.luma_mode, cm = j.chroma_mode;
  const bool is_inter = lm >= kNearestMv;
  // encode_block_pre_cdef: write_skip, write_segmentation (preskip false)
  s.put(ec_sym(RV_ECM_SKIP + 3 * ((has_above && rec_skip(ra)) + (has_left && rec_skip(rl))), 3,
               j.skip));
  if (a.prm.seg_enabled && !j.skip) {
    // get_segment_pred (src/context.rs:3465-3505)
    const int ul = (has_above && has_left) ? rec_seg(m[(size_t)(y8 - 1) * a.map_w8 + x8 - 1]) : -1;
    const int u = has_above ? rec_seg(ra) : -1, l = has_left ? rec_seg(rl) : -1;
    int ci, pred;
    if (ul < 0 || u < 0 || l < 0)
      ci = 0;
    else if (ul == u && ul == l)
      ci = 2;
    else if (ul == u || ul == l || u == l)
      ci = 1;
    else
      ci = 0;
    if (u == -1)
      pred = l == -1 ? 0 : l;
    else if (l == -1)
      pred = u;
    else
      pred = ul == u ? u : l;
    s.put(ec_sym(RV_ECM_SEG + 9 * ci, 9,
                 neg_interleave(j.seg_idx, pred, a.prm.last_active_segid + 1)));
  }
  // encode_block_post_cdef
  if (a.prm.frame_type == 1) {
    const bool ai = has_above && rec_mode(ra) < kNearestMv, li = has_left && rec_mode(rl) < kNearestMv;
    int ictx;  // intra_inter_context (src/context.rs:1744-1774)
    if (has_above && has_left)
      ictx = (ai && li) ? 3 : (ai || li);
    else
      ictx = (ai || li) ? 2 : 0;
    s.put(ec_sym(RV_ECM_INTRA_INTER + 3 * ictx, 3, is_inter));
    if (is_inter) {
      const int rf0 = j.ref[0], rf1 = j.ref[1];
      uint32_t cnt = 0;  // fill_neighbours_ref_counts
      if (has_above) cnt = ref_counts_add(cnt, ra);
      if (has_left) cnt = ref_counts_add(cnt, rl);
      const int a0 = has_above ? rec_ref0(ra) : 0, a1 = has_above ? rec_ref1(ra) : 8;
      const int l0 = has_left ? rec_ref0(rl) : 0, l1 = has_left ? rec_ref1(rl) : 8;
      const int ll2_l3g = ref_count_ctx(rc(cnt, 1) + rc(cnt, 2), rc(cnt, 3) + rc(cnt, 4));
      const int l_l2 = ref_count_ctx(rc(cnt, 1), rc(cnt, 2));
      const int l3_g = ref_count_ctx(rc(cnt, 3), rc(cnt, 4));
      const int bf2_a = ref_count_ctx(rc(cnt, 5) + rc(cnt, 6), rc(cnt, 7));
      const int b_a2 = ref_count_ctx(rc(cnt, 5), rc(cnt, 6));
      const bool comp = rf1 != 0 && rf1 != 8;
      const bool ls = l1 == 8, as = a1 == 8, lin = l0 == 0, ain = a0 == 0;
      // write_ref_frames (src/context.rs:3189-3334)
      if (a.prm.reference_mode) {  // sz >= 2 holds for every size in scope
        const bool lb = l0 >= 5, ab = a0 >= 5;
        int c;  // get_comp_mode_ctx
        if (has_left && has_above)
          c = (as && ls) ? (ab ^ lb) : as ? 2 + (ab || ain) : ls ? 2 + (lb || lin) : 4;
        else if (has_above)
          c = as ? ab : 3;
        else if (has_left)
          c = ls ? lb : 3;
        else
          c = 1;
        s.put(ec_sym(RV_ECM_COMP_MODE + 3 * c, 3, comp));
      }
      if (comp) {
        const bool aci = has_above && !ain && !as, lci = has_left && !lin && !ls;
        const bool auc = aci && samedir(a0, a1), luc = lci && samedir(l0, l1);
        int c;  // get_comp_ref_type_ctx
        if (has_above && !ain && has_left && !lin) {
          const int sd = samedir(a0, l0);
          if (!aci && !lci)
            c = 1 + 2 * sd;
          else if (!aci)
            c = !luc ? 1 : 3 + sd;
          else if (!lci)
            c = !auc ? 1 : 3 + sd;
          else if (!auc && !luc)
            c = 0;
          else if (!auc || !luc)
            c = 2;
          else
            c = 3 + ((a0 == 5) == (l0 == 5));
        } else if (has_above && has_left) {
          c = aci ? 1 + 2 * auc : lci ? 1 + 2 * luc : 2;
        } else if (aci) {
          c = 4 * auc;
        } else if (lci) {
          c = 4 * luc;
        } else {
          c = 2;
        }
        s.put(ec_sym(RV_ECM_COMP_REF_TYPE + 3 * c, 3, 1));  // bidirectional
        const bool cr = rf0 == 4 || rf0 == 3;
        s.put(ec_sym(RV_ECM_COMP_REF + (ll2_l3g * 3 + 0) * 3, 3, cr));
        if (!cr)
          s.put(ec_sym(RV_ECM_COMP_REF + (l_l2 * 3 + 1) * 3, 3, rf0 == 2));
        else
          s.put(ec_sym(RV_ECM_COMP_REF + (l3_g * 3 + 2) * 3, 3, rf0 == 4));
        const bool cb = rf1 == 7;
        s.put(ec_sym(RV_ECM_COMP_BWD_REF + (bf2_a * 2 + 0) * 3, 3, cb));
        if (!cb) s.put(ec_sym(RV_ECM_COMP_BWD_REF + (b_a2 * 2 + 1) * 3, 3, rf1 == 6));
      } else {
        const int b0c = ref_count_ctx(rc(cnt, 1) + rc(cnt, 2) + rc(cnt, 3) + rc(cnt, 4),
                                      rc(cnt, 5) + rc(cnt, 6) + rc(cnt, 7));
        const bool b0 = rf0 >= 5;
        s.put(ec_sym(RV_ECM_SINGLE_REF + (b0c * 6 + 0) * 3, 3, b0));
        if (b0) {
          const bool b1 = rf0 == 7;
          s.put(ec_sym(RV_ECM_SINGLE_REF + (bf2_a * 6 + 1) * 3, 3, b1));
          if (!b1) s.put(ec_sym(RV_ECM_SINGLE_REF + (b_a2 * 6 + 5) * 3, 3, rf0 == 6));
        } else {
          const bool b2 = rf0 == 3 || rf0 == 4;
          s.put(ec_sym(RV_ECM_SINGLE_REF + (ll2_l3g * 6 + 2) * 3, 3, b2));
          if (!b2)
            s.put(ec_sym(RV_ECM_SINGLE_REF + (l_l2 * 6 + 3) * 3, 3, rf0 != 1));
          else
            s.put(ec_sym(RV_ECM_SINGLE_REF + (l3_g * 6 + 4) * 3, 3, rf0 != 3));
        }
      }
      const int ctx = j.mode_context, newmv_ctx = ctx & 7, refmv_ctx = (ctx >> 4) & 15;
      if (lm >= kNearestNearestMv) {  // write_compound_mode
        const int c = refmv_ctx < 2   ? min(newmv_ctx, 1)
                      : refmv_ctx < 4 ? min(newmv_ctx + 1, 4)
                                      : min(max(newmv_ctx, 1) + 3, 7);
        s.put(ec_sym(RV_ECM_COMPOUND_MODE + 9 * c, 9, lm - kNearestNearestMv));
      } else {  // write_inter_mode
        s.put(ec_sym(RV_ECM_NEWMV + 3 * newmv_ctx, 3, lm != kNewMv));
        if (lm != kNewMv) {
          s.put(ec_sym(RV_ECM_ZEROMV + 3 * ((ctx >> 3) & 1), 3, lm != kGlobalMv));
          if (lm != kGlobalMv) s.put(ec_sym(RV_ECM_REFMV + 3 * refmv_ctx, 3, lm != kNearestMv));
        }
      }
      const int nf = j.num_mv_found;
      const int w0 = j.weight[0] < kRefCatLevel, w1 = j.weight[1] < kRefCatLevel;
      const int w2 = j.weight[2] < kRefCatLevel, w3 = j.weight[3] < kRefCatLevel;
      // the first DRL loop (ref_mv_idx 0: one symbol at the first idx that has a successor)
      if ((lm == kNewMv || lm == kNewNewMv) && nf > 1) s.put(ec_sym(RV_ECM_DRL + 3 * (w0 + w1), 3, 0));
      const int precision =
          a.prm.force_integer_mv ? -1 : a.prm.allow_high_precision_mv ? 1 : 0;
#pragma unroll
      for (int k = 0; k < 2; k++)
        if (mv_coded(lm, k)) {  // write_mv (src/context.rs:3391-3417)
          const int dr = j.mv[2 * k] - j.ref_mv[2 * k], dc = j.mv[2 * k + 1] - j.ref_mv[2 * k + 1];
          const int jt = dr == 0 ? (dc == 0 ? 0 : 1) : (dc == 0 ? 2 : 3);
          s.put(ec_sym(RV_ECM_MV_JOINTS, 5, jt));
          if (jt >= 2) mv_component(s, dr, RV_ECM_MV_COMP, precision);
          if (jt & 1) mv_component(s, dc, RV_ECM_MV_COMP + 69, precision);
        }
      if (mode_has_near(lm)) {  // the second DRL loop, idx 1..2
        const int rmi = near_ref_mv_idx(lm);
        if (nf > 2) {
          s.put(ec_sym(RV_ECM_DRL + 3 * (w1 + w2), 3, rmi > 1));
          if (rmi > 1 && nf > 3) s.put(ec_sym(RV_ECM_DRL + 3 * (w2 + w3), 3, rmi > 2));
        }
      }
    } else {
      // write_intra_mode: size_group_lookup of 8x8 1, 16x16 2, 32x32 / 64x64 3
      s.put(ec_sym(RV_ECM_Y_MODE + 14 * min(lg - 2, 3), 14, lm));
    }
  } else {  // write_intra_mode_kf
    const int am = has_above ? rec_mode(ra) : 0, lmode = has_left ? rec_mode(rl) : 0;
    // a neighbour of a key frame is intra (mode < 13); min keeps the index in the table
    const int actx = kIntraModeContext[min(am, 12)], lctx = kIntraModeContext[min(lmode, 12)];
    s.put(ec_sym(RV_ECM_KF_Y + (actx * 5 + lctx) * 14, 14, lm));
  }
  if (!is_inter) {
    if (lm >= kVPred && lm <= kD63Pred)  // write_angle_delta(0): symbol MAX_ANGLE_DELTA
      s.put(ec_sym(RV_ECM_ANGLE_DELTA + 8 * (lm - kVPred), 8, 3));
    const int cfl_ok = lg <= 5;  // BlockSize::cfl_allowed
    s.put(ec_sym(RV_ECM_UV_MODE + (cfl_ok * 13 + lm) * 15, cfl_ok ? 15 : 14, cm));
    if (cm == kUvCfl) {  // write_cfl_alphas
      const int js = j.cfl_joint_sign, su = (js + 1) / 3, sv = (js + 1) % 3;
      s.put(ec_sym(RV_ECM_CFL_SIGN, 9, js));
      if (su) s.put(ec_sym(RV_ECM_CFL_ALPHA + 17 * ((su - 1) * 3 + sv), 17, j.cfl_scale[0] - 1));
      if (sv) s.put(ec_sym(RV_ECM_CFL_ALPHA + 17 * ((sv - 1) * 3 + su), 17, j.cfl_scale[1] - 1));
    }
    if (cm >= kVPred && cm <= kD63Pred) s.put(ec_sym(RV_ECM_ANGLE_DELTA + 8 * (cm - kVPred), 8, 3));
  }
}

}  // namespace rv

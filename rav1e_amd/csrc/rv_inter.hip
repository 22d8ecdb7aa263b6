// rv_inter.hip -- the inter front of rdo_mode_decision (src/rdo.rs:784-1259):
// the reference sets (:815-835, :914-927, host), the inter mode set with each
// candidate's MVs (:858-986) and motion_compensate of the candidates (src/
// encoder.rs:1239-1430 through predict_inter, src/predict.rs:255-338).
//
// Mode set.  One lane per block.  A first pass over the sets counts the
// candidates (the two inputs on which the reference panics are rejected
// there), a second pass writes the records and the MC jobs straight to global
// memory through a running pointer: no local array is indexed at run time, so
// nothing lands in scratch (as rv_epzs.h keeps its sets).
//
// Motion compensation.  A job takes a group of G lanes of a 256-lane
// workgroup (G a power of two, 16 .. 256; 256 / G jobs share the workgroup)
// and walks its coded planes one after the other.  Per plane and reference:
// get_params and PlaneSlice::clamp, the (h + 7) x (w + 7) window into LDS with
// row-contiguous reads, the horizontal pass into LDS, the vertical pass.  A
// single reference writes put_8tap's pixel; a compound job keeps prep_8tap's
// i16 tile of the first reference in LDS and folds mc_avg into the vertical
// pass of the second, so no intermediate touches HBM.  The fracs differ per
// job, so the barriers sit outside every per-job condition.
//
// The plane tables are kernel arguments: one geometry per plane (the sets must
// agree in it) and one pointer per (set, plane).  A job's set is a per-lane
// value; the pointer is picked by a select chain over constant indices, which
// keeps the table in SGPRs (a run-time index into a by-value argument is
// copied to scratch).
#include <cstdio>

#include "rv_mc.h"

namespace rv {

// BlockSize in pixels (src/partition.rs:85-108 order); 0: not taken here
constexpr uint8_t kInterBlkW[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 0, 0, 0, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kInterBlkH[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 0, 0, 0, 16, 4, 32, 8, 64, 16};
// every BlockSize, for width_mi / height_mi (128 sizes included)
constexpr uint8_t kInterAllW[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kInterAllH[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16};

constexpr int kMcbThreads = 256;
constexpr int kMcbMaxRefs = 8;

// PredictionMode (src/predict.rs:73-107 order)
enum : int32_t {
  kNearestMv = 14, kNear0Mv = 15, kNear1Mv = 16, kNear2Mv = 17, kGlobalMv = 18, kNewMv = 19,
  kNearestNearestMv = 20, kNearNearMv = 21, kNearestNewMv = 22, kNewNearestMv = 23,
  kGlobalGlobalMv = 26, kNewNewMv = 27
};
constexpr int32_t kNoneFrame = 8;

// ---- the mode set -----------------------------------------------------------
struct ImsArgs {
  const rv_mvref_result *stacks;
  const rv_mv *me;
  const rv_inter_blk *blocks;
  rv_inter_list *lists;
  rv_inter_mc_job *jobs;
  uint32_t *status;
  rv_inter_ref_sets sets;
  int n, near;
};

// An MV travels as one register (row in the low half): equal MVs are equal
// words, and no rv_mv local has its address taken.
typedef uint32_t mvw;
__device__ __forceinline__ mvw mv_ld(const rv_mv *p) {
  return (uint32_t)(uint16_t)p->row | ((uint32_t)(uint16_t)p->col << 16);
}
__device__ __forceinline__ void mv_st(rv_mv *p, mvw v) {
  p->row = (int16_t)(v & 0xFFFFu);
  p->col = (int16_t)(v >> 16);
}

// NEWMV's condition (src/rdo.rs:898-909) on single set i's stack
__device__ __forceinline__ bool ims_has_new(const rv_mvref_result *st, mvw me, int near) {
  if (me == 0) return false;
  const int take = near ? 4 : 2, len = st->n;
  for (int k = 0; k < take && k < len; k++)
    if (mv_ld(&st->stack[k].this_mv) == me) return false;
  return true;
}

__global__ __launch_bounds__(256) void inter_mode_set_kernel(ImsArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.n) return;
  const int ns = a.sets.n_single, nsets = ns + a.sets.compound;
  const rv_mvref_result *st = a.stacks + (int64_t)b * nsets;
  const rv_mv *me = a.me + (int64_t)b * ns;
  rv_inter_list *L = a.lists + b;
  rv_inter_mc_job *J = a.jobs ? a.jobs + (int64_t)b * RV_INTER_MAX_CANDS : nullptr;

  // pass 1: the list's length, and the inputs the reference panics on
  int count = 0;
  bool bad = false;
  for (int i = 0; i < nsets; i++) bad |= st[i].n < 0 || st[i].n > 9;
  if (!bad) {
    for (int i = 0; i < ns; i++) {
      const int len = st[i].n;
      count += 1 + (len >= 1) + (len >= 2);
      if (a.near) count += (len >= 3) + (len >= 4);
      count += ims_has_new(st + i, mv_ld(me + i), a.near);
    }
    if (a.sets.compound) {
      count += 6;
      bad |= st[ns].n == 0;  // mv_stacks[i][0] of NEAREST_NEWMV (:974-979)
    }
    bad |= count > RV_INTER_MAX_CANDS;  // the ArrayVec's capacity (:837)
  }
  if (bad) {
    atomicAdd(a.status, 1u);
    count = 0;
  }
  L->n = count;
  rv_inter_blk blk = {-1, 0, 0};
  if (J && !bad) blk = a.blocks[b];

  // pass 2: the records in push order
  int k = 0;
  auto emit = [&](int mode, int set, int r0, int r1, int s0, int s1, mvw m0, mvw m1, int ctx) {
    rv_inter_cand *c = L->cand + k;  // field by field: no local record to index
    c->luma_mode = mode, c->set = set, c->ref[0] = r0, c->ref[1] = r1;
    mv_st(&c->mv[0], m0), mv_st(&c->mv[1], m1), c->mode_context = ctx;
    if (J) {
      rv_inter_mc_job *j = J + k;
      j->tile = blk.tile, j->bo_x = blk.bo_x, j->bo_y = blk.bo_y, j->dst_set = k;
      j->ref_slot[0] = s0, j->ref_slot[1] = s1, mv_st(&j->mv[0], m0), mv_st(&j->mv[1], m1);
    }
    k++;
  };
  const mvw zero = 0;
  if (!bad) {
    for (int i = 0; i < ns; i++) {
      const rv_mvref_result *s = st + i;
      const int len = s->n, ctx = s->mode_context, r = a.sets.ref[i], sl = a.sets.slot[i];
      const mvw m = mv_ld(me + i);
      emit(kNearestMv, i, r, kNoneFrame, sl, -1, len > 0 ? mv_ld(&s->stack[0].this_mv) : zero,
           len > 0 ? mv_ld(&s->stack[0].comp_mv) : zero, ctx);
      if (len >= 1)
        emit(kNear0Mv, i, r, kNoneFrame, sl, -1, len > 1 ? mv_ld(&s->stack[1].this_mv) : zero,
             len > 1 ? mv_ld(&s->stack[1].comp_mv) : zero, ctx);
      if (len >= 2) emit(kGlobalMv, i, r, kNoneFrame, sl, -1, zero, zero, ctx);
      if (a.near && len >= 3)
        emit(kNear1Mv, i, r, kNoneFrame, sl, -1, mv_ld(&s->stack[2].this_mv), mv_ld(&s->stack[2].comp_mv), ctx);
      if (a.near && len >= 4)
        emit(kNear2Mv, i, r, kNoneFrame, sl, -1, mv_ld(&s->stack[3].this_mv), mv_ld(&s->stack[3].comp_mv), ctx);
      if (ims_has_new(s, m, a.near)) emit(kNewMv, i, r, kNoneFrame, sl, -1, m, zero, ctx);
    }
    if (a.sets.compound) {
      const rv_mvref_result *s = st + ns;
      const int f = a.sets.fwd, w = a.sets.bwd, len = s->n, ctx = s->mode_context;
      const int r0 = a.sets.ref[f], r1 = a.sets.ref[w], s0 = a.sets.slot[f], s1 = a.sets.slot[w];
      const mvw m0 = mv_ld(me + f), m1 = mv_ld(me + w);  // mvs_from_me of the compound set (:925-927)
      const mvw e0t = mv_ld(&s->stack[0].this_mv), e0c = mv_ld(&s->stack[0].comp_mv);  // len >= 1 here
      emit(kGlobalGlobalMv, ns, r0, r1, s0, s1, zero, zero, ctx);
      emit(kNearestNearestMv, ns, r0, r1, s0, s1, e0t, e0c, ctx);
      emit(kNewNewMv, ns, r0, r1, s0, s1, m0, m1, ctx);
      emit(kNearestNewMv, ns, r0, r1, s0, s1, e0t, m1, ctx);
      emit(kNewNearestMv, ns, r0, r1, s0, s1, m0, e0c, ctx);
      emit(kNearNearMv, ns, r0, r1, s0, s1, len > 1 ? mv_ld(&s->stack[1].this_mv) : zero,
           len > 1 ? mv_ld(&s->stack[1].comp_mv) : zero, ctx);
    }
  }
  // the unused entries: zero records, skipped jobs
  for (; k < RV_INTER_MAX_CANDS; k++) {
    rv_inter_cand *c = L->cand + k;
    c->luma_mode = 0, c->set = 0, c->ref[0] = 0, c->ref[1] = 0;
    mv_st(&c->mv[0], zero), mv_st(&c->mv[1], zero), c->mode_context = 0;
    if (J) {
      rv_inter_mc_job *j = J + k;
      j->tile = -1, j->bo_x = 0, j->bo_y = 0, j->dst_set = 0;
      j->ref_slot[0] = 0, j->ref_slot[1] = -1, mv_st(&j->mv[0], zero), mv_st(&j->mv[1], zero);
    }
  }
}

// ---- motion compensation ----------------------------------------------------
struct McbGeom {
  int32_t stride, alloc_height, width, height, xorigin, yorigin;
};
struct McbArgs {
  McbGeom g[3];
  const void *ref[3][kMcbMaxRefs];         // [plane][set]
  void *dst[3][RV_INTER_MAX_CANDS];
  const rv_intra_tile *tiles;
  const rv_inter_mc_job *jobs;
  uint32_t *status;
  int n_tiles, n, n_refs, n_dsts, planes;
  int bw, bh, xdec, ydec;  // the luma block, the chroma planes' decimation
  int mode, bit_depth;
  int lanes_log2;          // lanes per job
  int lds_per_job;         // i16 elements
};

// tab[set] for a per-lane set < N: constant indices only
template <typename T, int N>
__device__ __forceinline__ T mcb_pick(T const (&tab)[N], int set) {
  T p = tab[0];
#pragma unroll
  for (int s = 1; s < N; s++) p = set == s ? tab[s] : p;
  return p;
}

template <typename Px>
__global__ __launch_bounds__(kMcbThreads) void motion_compensate_kernel(McbArgs a) {
  extern __shared__ __align__(16) int16_t lds[];
  const int tid = threadIdx.x, G = 1 << a.lanes_log2;
  const int lane = tid & (G - 1), slot = tid >> a.lanes_log2;
  const int job = blockIdx.x * (kMcbThreads >> a.lanes_log2) + slot;
  const int bw4 = a.bw >> 2, bh4 = a.bh >> 2;

  // ---- the job and its checks: a rejected job touches no pixel --------------
  bool ok = false;
  rv_inter_mc_job jb = {};
  rv_intra_tile tl = {};
  if (job < a.n) {
    jb = a.jobs[job];
    if (jb.tile >= 0) {
      ok = jb.tile < a.n_tiles && jb.ref_slot[0] >= 0 && jb.ref_slot[0] < a.n_refs &&
           jb.ref_slot[1] < a.n_refs && jb.dst_set >= 0 && jb.dst_set < a.n_dsts &&
           jb.bo_x >= 0 && jb.bo_y >= 0 && jb.bo_x <= (1 << 20) && jb.bo_y <= (1 << 20) &&
           jb.bo_x % bw4 == 0 && jb.bo_y % bh4 == 0;
      if (ok) {
        tl = a.tiles[jb.tile];
        ok = tl.x >= 0 && tl.y >= 0 && tl.x <= (1 << 24) && tl.y <= (1 << 24) &&
             tl.width >= 0 && tl.height >= 0 && 4 * (jb.bo_x + bw4) <= tl.width &&
             4 * (jb.bo_y + bh4) <= tl.height;
        for (int p = 0; ok && p < a.planes; p++) {  // the block inside the destination
          const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
          const int fx = (tl.x >> xd) + ((4 * jb.bo_x) >> xd), fy = (tl.y >> yd) + ((4 * jb.bo_y) >> yd);
          ok = fx + (a.bw >> xd) <= a.g[p].stride - a.g[p].xorigin &&
               fy + (a.bh >> yd) <= a.g[p].alloc_height - a.g[p].yorigin;
        }
      }
      if (!ok && lane == 0) atomicAdd(a.status, 1u);
    }
  }
  const bool compound = ok && jb.ref_slot[1] >= 0;
  const int passes = __syncthreads_or(compound) ? 2 : 1;  // uniform over the workgroup

  int16_t *win = lds + slot * a.lds_per_job;        // [sh][sw] source pixels
  int16_t *mid = win + (a.bh + 7) * (a.bw + 7);     // [sh][w] horizontal pass
  int16_t *t0 = mid + (a.bh + 7) * a.bw;            // [h][w] prep tile of reference 0
  const int ib = a.bit_depth == 12 ? 2 : 4;         // intermediate_bits
  const int maxv = (1 << a.bit_depth) - 1;

  for (int p = 0; p < a.planes; p++) {
    const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
    const int w = a.bw >> xd, h = a.bh >> yd;
    const McbGeom g = a.g[p];
    // frame_po (src/encoder.rs:1264-1266, src/predict.rs:261)
    const int fx = (tl.x >> xd) + ((4 * jb.bo_x) >> xd), fy = (tl.y >> yd) + ((4 * jb.bo_y) >> yd);
    const int dset = jb.dst_set;
    Px *dbase = (Px *)(p == 0 ? mcb_pick(a.dst[0], dset)
                              : p == 1 ? mcb_pick(a.dst[1], dset) : mcb_pick(a.dst[2], dset));
    for (int r = 0; r < passes; r++) {
      const bool act = ok && (r == 0 || compound);
      // get_params (src/predict.rs:267-284)
      const rv_mv mv = r ? jb.mv[1] : jb.mv[0];
      const int sr = 3 + yd, sc = 3 + xd;
      const int roff = (int)mv.row >> sr, coff = (int)mv.col >> sc;
      const int rf = act ? ((int)mv.row - (roff << sr)) << (4 - sr) : 0;
      const int cf = act ? ((int)mv.col - (coff << sc)) << (4 - sc) : 0;
      // PlaneSlice::clamp (src/frame/plane.rs:521-533) of the window's origin, then + 3
      const int sx = clampi(fx + coff - 3, -g.xorigin, g.width) + 3;
      const int sy = clampi(fy + roff - 3, -g.yorigin, g.height) + 3;
      const int ox = cf ? 3 : 0, oy = rf ? 3 : 0;   // window margins
      const int sw = w + (cf ? 7 : 0), sh = h + (rf ? 7 : 0);
      const int rs = act ? (r ? jb.ref_slot[1] : jb.ref_slot[0]) : 0;
      const Px *sbase = (const Px *)(p == 0 ? mcb_pick(a.ref[0], rs)
                                            : p == 1 ? mcb_pick(a.ref[1], rs) : mcb_pick(a.ref[2], rs));

      // 1. source window -> LDS (row-contiguous)
      if (act) {
        const Px *sp = sbase + (int64_t)(g.yorigin + sy - oy) * g.stride + g.xorigin + sx - ox;
        for (int i = lane; i < sh * sw; i += G) {
          const int rr = i / sw, c = i - rr * sw;
          win[i] = (int16_t)sp[(int64_t)rr * g.stride + c];
        }
      }
      __syncthreads();

      // 2. horizontal pass: mid = round_shift(sum xf * src, 7 - ib)
      if (act && cf) {
        const int8_t *xf = kSubpel[filter_set(a.mode, w)][cf];
        int32_t f[8];
#pragma unroll
        for (int k = 0; k < 8; k++) f[k] = xf[k];
        for (int i = lane; i < sh * w; i += G) {
          const int rr = i / w, c = i - rr * w;
          const int16_t *q = win + rr * sw + c;  // column c - 3 .. c + 4
          int32_t s = 0;
#pragma unroll
          for (int k = 0; k < 8; k++) s += f[k] * q[k];
          mid[i] = (int16_t)round_shift(s, 7 - ib);
        }
      }
      __syncthreads();

      // 3. vertical pass; put_8tap's pixel, or prep_8tap's value and mc_avg
      if (act) {
        const int8_t *yf = kSubpel[filter_set(a.mode, h)][rf];
        int32_t fyv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) fyv[k] = yf[k];
        Px *dp = dbase + (int64_t)(g.yorigin + fy) * g.stride + g.xorigin + fx;
        for (int i = lane; i < w * h; i += G) {
          const int rr = i / w, c = i - rr * w;
          int32_t v;  // put: before the clamp; prep: the i16 intermediate
          if (!cf && !rf) {
            v = win[rr * sw + c];
            if (compound) v = (int32_t)(int16_t)(v << ib);
          } else if (!cf) {
            const int16_t *q = win + rr * sw + c;  // rows rr - 3 .. rr + 4
            int32_t s = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) s += fyv[k] * q[k * sw];
            v = compound ? round_shift(s, 7 - ib) : round_shift(s, 7);
          } else if (!rf) {
            const int32_t m = mid[rr * w + c];
            v = compound ? m : round_shift(m, ib);
          } else {
            const int16_t *q = mid + rr * w + c;
            int32_t s = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) s += fyv[k] * q[k * w];
            v = compound ? round_shift(s, 7) : round_shift(s, 7 + ib);
          }
          if (compound && r == 0) {
            t0[i] = (int16_t)v;  // read back by this lane only
          } else {
            // mc_avg (src/mc.rs:389-408): round_shift(t1 + t2, ib + 1)
            if (compound) v = round_shift((int32_t)t0[i] + (int32_t)(int16_t)v, ib + 1);
            dp[(int64_t)rr * g.stride + c] = (Px)clampi(v, 0, maxv);
          }
        }
      }
      __syncthreads();  // the next window overwrites win / mid
    }
  }
}

static int inter_fail(int code, const char *who, const char *what) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return rv_set_error(code, msg);
}

static bool ref_sets_ok(const rv_inter_ref_sets &s) {
  if (s.n_single < 1 || s.n_single > 7 || (s.compound != 0 && s.compound != 1)) return false;
  for (int i = 0; i < s.n_single; i++)
    if (s.ref[i] < 1 || s.ref[i] > 7 || s.slot[i] < 0 || s.slot[i] > 7) return false;
  if (s.fwd < -1 || s.fwd >= s.n_single || s.bwd < -1 || s.bwd >= s.n_single) return false;
  if (s.compound && (s.fwd < 0 || s.bwd < 0)) return false;
  return true;
}

// Default lanes per job: one lane per eight luma pixels, 16 at least.  Measured
// on the squares: 16 lanes at 8x8, 32 at 16x16, 128 at 32x32 and
// 256 at 64x64 were the fastest packings; the rectangles follow the same rule.
static int mcb_default_lanes(int bw, int bh) {
  int l = bw * bh / 8;
  return l < 16 ? 16 : (l > kMcbThreads ? kMcbThreads : l);
}

}  // namespace rv

using namespace rv;

extern "C" int rv_inter_ref_sets_build(const int32_t *allowed, int n_allowed,
                                       const int32_t *ref_frames, int reference_mode_not_single,
                                       int bsize, rv_inter_ref_sets *out) {
  const char *who = "rv_inter_ref_sets_build";
  if (!allowed || !ref_frames || !out) return inter_fail(RV_EINVAL, who, "null argument");
  if (n_allowed < 1 || n_allowed > 7) return inter_fail(RV_EINVAL, who, "n_allowed is 1 .. 7");
  if (bsize < 0 || bsize > 21) return inter_fail(RV_EINVAL, who, "bsize is no BlockSize");
  for (int k = 0; k < n_allowed; k++)
    if (allowed[k] < 1 || allowed[k] > 7) return inter_fail(RV_EINVAL, who, "a RefType outside 1 .. 7");
  for (int k = 0; k < 7; k++)
    if (ref_frames[k] < 0 || ref_frames[k] > 7) return inter_fail(RV_EINVAL, who, "a slot outside 0 .. 7");
  rv_inter_ref_sets s = {};
  s.fwd = s.bwd = -1;
  for (int k = 0; k < n_allowed; k++) {
    const int r = allowed[k];
    if (r == 3) continue;  // LAST3_FRAME is used only for probs (:817-820)
    const int slot = ref_frames[r - 1];
    bool seen = false;
    for (int i = 0; i < s.n_single; i++) seen |= s.slot[i] == slot;
    if (seen) continue;
    if (s.fwd < 0 && r < 5) s.fwd = s.n_single;   // is_fwd_ref
    if (s.bwd < 0 && r >= 5) s.bwd = s.n_single;  // is_bwd_ref
    s.ref[s.n_single] = r;
    s.slot[s.n_single] = slot;
    s.n_single++;
  }
  if (s.n_single == 0) return inter_fail(RV_EINVAL, who, "no reference set (only LAST3_FRAME allowed)");
  const int w_mi = kInterAllW[bsize] >> 2, h_mi = kInterAllH[bsize] >> 2;
  const int sz = w_mi < h_mi ? w_mi : h_mi;
  s.compound = reference_mode_not_single && sz >= 2 && s.fwd >= 0 && s.bwd >= 0;
  *out = s;
  return RV_OK;
}

extern "C" int rv_inter_mode_set_batch(const rv_mvref_result *d_stacks, const rv_mv *d_me,
                                       const rv_inter_blk *d_blocks, int n, rv_inter_ref_sets sets,
                                       int include_near_mvs, rv_inter_list *d_lists,
                                       rv_inter_mc_job *d_mc_jobs, uint32_t *d_status,
                                       void *stream) {
  const char *who = "rv_inter_mode_set_batch";
  if (n < 0 || n > (1 << 24)) return inter_fail(RV_EINVAL, who, "n outside 0 .. 2^24");
  if (!ref_sets_ok(sets)) return inter_fail(RV_EINVAL, who, "sets is no rv_inter_ref_sets_build result");
  if (!d_status || (n && (!d_stacks || !d_me || !d_lists)) || (n && d_mc_jobs && !d_blocks))
    return inter_fail(RV_EINVAL, who, "null argument");
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess)
    return rv_set_hip_error(hipGetLastError(), who);
  if (n == 0) return RV_OK;
  ImsArgs a = {d_stacks, d_me, d_blocks, d_lists, d_mc_jobs, d_status, sets, n, include_near_mvs != 0};
  inter_mode_set_kernel<<<(n + 255) / 256, 256, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_motion_compensate_batch_lanes(const rv_plane *refs, int n_refs,
                                                const rv_plane *dsts, int n_dsts,
                                                const rv_intra_tile *d_tiles, int n_tiles,
                                                const rv_inter_mc_job *d_jobs, int n,
                                                const rv_inter_mc_params *params,
                                                uint32_t *d_status, int lanes, void *stream) {
  const char *who = "rv_motion_compensate_batch";
  if (!params || !refs || !dsts || !d_status || n < 0 || n_tiles < 0)
    return inter_fail(RV_EINVAL, who, "null argument or negative count");
  const rv_inter_mc_params &P = *params;
  if (P.bsize < 0 || P.bsize > 21) return inter_fail(RV_EINVAL, who, "bsize is no BlockSize");
  if (P.filter_mode < 0 || P.filter_mode > 3) return inter_fail(RV_EINVAL, who, "filter_mode is no FilterMode");
  const int bd = P.bit_depth;
  if (bd != 8 && bd != 10 && bd != 12) return inter_fail(RV_EINVAL, who, "bit_depth must be 8, 10 or 12");
  if (n_refs < 1 || n_refs > kMcbMaxRefs) return inter_fail(RV_EINVAL, who, "n_refs is 1 .. 8");
  if (n_dsts < 1 || n_dsts > RV_INTER_MAX_CANDS) return inter_fail(RV_EINVAL, who, "n_dsts is 1 .. 20");
  if (lanes != 0 && (lanes < 16 || lanes > kMcbThreads || (lanes & (lanes - 1))))
    return inter_fail(RV_EINVAL, who, "lanes is 0 or a power of two 16 .. 256");
  const int luma_only = P.luma_only != 0, planes = luma_only ? 1 : 3;
  const int xdec = luma_only ? 0 : refs[1].xdec, ydec = luma_only ? 0 : refs[1].ydec;
  if (!((xdec == 0 && ydec == 0) || (xdec == 1 && (ydec == 0 || ydec == 1))))
    return inter_fail(RV_EINVAL, who, "subsampling must be 4:4:4, 4:2:2 or 4:2:0");
  if (P.bsize > 12)
    return inter_fail(RV_ENOTSUP, who, "4:1 / 1:4 partitions and sizes above 64x64 are not supported");
  const int bw = kInterBlkW[P.bsize], bh = kInterBlkH[P.bsize];
  if (bw == 4 || bh == 4)
    return inter_fail(RV_ENOTSUP, who, "4xN / Nx4 partitions are not supported (their chroma reads the neighbours' MVs)");
  // subsampled_size (src/partition.rs:245-286): no 1:2 size at 4:2:2
  if (!luma_only && xdec == 1 && ydec == 0 && bh == 2 * bw)
    return inter_fail(RV_ENOTSUP, who, "the block size has no subsampled size at 4:2:2 (BLOCK_INVALID)");

  McbArgs a = {};
  const size_t px = bd > 8 ? 2 : 1;
  for (int p = 0; p < planes; p++) {
    const rv_plane &g0 = refs[p];
    for (int k = 0; k < n_refs + n_dsts; k++) {
      const rv_plane &pl = k < n_refs ? refs[3 * k + p] : dsts[3 * (k - n_refs) + p];
      if (!pl.data) return inter_fail(RV_EINVAL, who, "a plane without data");
      if (pl.hbd != (bd > 8)) return inter_fail(RV_EINVAL, who, "pixel type does not fit bit_depth");
      if (pl.xdec != (p ? xdec : 0) || pl.ydec != (p ? ydec : 0))
        return inter_fail(RV_EINVAL, who, "the plane sets differ in subsampling");
      if (pl.stride != g0.stride || pl.alloc_height != g0.alloc_height || pl.width != g0.width ||
          pl.height != g0.height || pl.xorigin != g0.xorigin || pl.yorigin != g0.yorigin)
        return inter_fail(RV_EINVAL, who, "the plane sets differ in geometry");
    }
    if (g0.stride <= 0 || g0.alloc_height <= 0 || g0.width <= 0 || g0.height <= 0 ||
        g0.xorigin < 0 || g0.yorigin < 0)
      return inter_fail(RV_EINVAL, who, "a plane's geometry is not positive");
    // the furthest clamped window: PlaneSlice::clamp leaves the origin in
    // [-xorigin, width] x [-yorigin, height]; the filters read 7 past the block
    const int w = bw >> (p ? xdec : 0), h = bh >> (p ? ydec : 0);
    if ((int64_t)g0.xorigin + g0.width + w + 6 >= g0.stride ||
        (int64_t)g0.yorigin + g0.height + h + 6 >= g0.alloc_height)
      return inter_fail(RV_EINVAL, who, "a reference plane's padding does not hold the furthest clamped window");
    // no destination may overlap a reference or another destination
    const size_t bytes = (size_t)g0.stride * g0.alloc_height * px;
    for (int d = 0; d < n_dsts; d++) {
      const char *d0 = (const char *)dsts[3 * d + p].data;
      for (int k = 0; k < n_refs + d; k++) {
        const char *r0 = (const char *)(k < n_refs ? refs[3 * k + p].data : dsts[3 * (k - n_refs) + p].data);
        if (d0 < r0 + bytes && r0 < d0 + bytes)
          return inter_fail(RV_EINVAL, who, k < n_refs ? "a destination set aliases a reference set"
                                                       : "two destination sets overlap");
      }
    }
    a.g[p] = McbGeom{g0.stride, g0.alloc_height, g0.width, g0.height, g0.xorigin, g0.yorigin};
    for (int k = 0; k < kMcbMaxRefs; k++) a.ref[p][k] = refs[3 * (k < n_refs ? k : 0) + p].data;
    for (int k = 0; k < RV_INTER_MAX_CANDS; k++) a.dst[p][k] = dsts[3 * (k < n_dsts ? k : 0) + p].data;
  }
  if (n > 0 && (!d_jobs || !d_tiles || n_tiles == 0))
    return inter_fail(RV_EINVAL, who, "null jobs or tiles");
  if (n > (1 << 24)) return inter_fail(RV_EINVAL, who, "n above 2^24");

  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess)
    return rv_set_hip_error(hipGetLastError(), who);
  if (n == 0) return RV_OK;
  a.tiles = d_tiles, a.jobs = d_jobs, a.status = d_status;
  a.n_tiles = n_tiles, a.n = n, a.n_refs = n_refs, a.n_dsts = n_dsts, a.planes = planes;
  a.bw = bw, a.bh = bh, a.xdec = xdec, a.ydec = ydec;
  a.mode = P.filter_mode, a.bit_depth = bd;
  const int L = lanes ? lanes : mcb_default_lanes(bw, bh);
  a.lanes_log2 = 31 - __builtin_clz((unsigned)L);
  // window, horizontal pass and one prep tile of the luma block (the largest)
  a.lds_per_job = ((bh + 7) * (bw + 7) + (bh + 7) * bw + bw * bh + 7) & ~7;
  const int jpw = kMcbThreads / L;
  const size_t lds = (size_t)a.lds_per_job * jpw * sizeof(int16_t);
  if (lds > 64 * 1024) return inter_fail(RV_EINVAL, who, "too few lanes per job for this block size (LDS)");
  const unsigned grid = (unsigned)((n + jpw - 1) / jpw);
  if (bd > 8)
    motion_compensate_kernel<uint16_t><<<grid, kMcbThreads, lds, st>>>(a);
  else
    motion_compensate_kernel<uint8_t><<<grid, kMcbThreads, lds, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_motion_compensate_batch(const rv_plane *refs, int n_refs, const rv_plane *dsts,
                                          int n_dsts, const rv_intra_tile *d_tiles, int n_tiles,
                                          const rv_inter_mc_job *d_jobs, int n,
                                          const rv_inter_mc_params *params, uint32_t *d_status,
                                          void *stream) {
  return rv_motion_compensate_batch_lanes(refs, n_refs, dsts, n_dsts, d_tiles, n_tiles, d_jobs, n,
                                          params, d_status, 0, stream);
}

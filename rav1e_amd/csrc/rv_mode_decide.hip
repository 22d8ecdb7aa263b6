// rv_mode_decide.hip -- the end of rdo_mode_decision (src/rdo.rs:784-1259) as
// device operators: a candidate's ScaledDistortion as luma_chroma_mode_rdo
// takes it (:736-751: compute_distortion :338-411 or compute_tx_distortion
// :414-475), compute_rd_cost (:563-568), the walk over a block's candidates
// with the reference's early-outs (:752-780, :1008), and the winner's
// PartitionParameters; beside it the heuristic segment index and get_qidx of a
// block (:655-679, src/encoder.rs:1061-1072).  The contract is in
// include/rav1e_hip.h.
//
// Work split.  A block takes G lanes of a 256-lane workgroup (256 / G blocks
// share it).  The block's source pixels (u16) and the f64 bias of each of its
// importance sub-blocks go to LDS once and serve every candidate.  Candidates
// are taken eight at a time; the lanes run over (candidate, sub-block): one
// lane sums one sub-block's moments (an 8x8 luma sub-block, or a chroma
// sub-block of at most 8x8) against the candidate's pixels, finishes it in f64
// (cdef_dist_finish / the bias product, truncated as the reference truncates)
// and adds the u64 to the candidate's per-plane sum in LDS -- integer adds, so
// their order does not matter.  One lane per candidate then scales the three
// sums (or walks the candidate's transform blocks on the tx path) and forms
// the cost; one lane per block walks the list.  Every barrier is outside the
// per-candidate conditions: the chunk loop runs to the workgroup's longest
// list.
#include <cfloat>
#include <cstdio>

#include "rv_distortion.h"
#include "rv_tx_layout.h"

namespace rv {

constexpr int kMdThreads = 256;
constexpr int kMdChunk = 8;  // candidates in flight per block
// a candidate's word in LDS: its set, and how it is taken
constexpr int kMdValid = 1 << 8, kMdPixels = 1 << 9;

struct MdGeom {
  int32_t stride, alloc_height, xorigin, yorigin;
};
// What the tx path reads of rv_tx_blocks_layout(bsize, tx_size) per plane:
// the blocks, their columns and the transform's size in 4x4 units.
struct MdTx {
  uint16_t nb[3];
  uint8_t cols[3], tw4[3], th4[3];
  uint8_t valid;
};
struct MdArgs {
  const void *src[3];
  const void *cand[3][RV_INTER_MAX_CANDS];  // [plane][set]
  void *commit[3];
  MdGeom g[3];
  const rv_intra_tile *tiles;
  const rv_mode_block *blocks;
  const rv_mode_cand *cands;
  const rv_mode_decision *seed;
  const uint64_t *dist;
  const uint32_t *eob;
  const float *imp;
  rv_mode_decision *out;
  uint64_t *cand_dist;
  double *cand_cost;
  int32_t *cand_state;
  uint32_t *status;
  double lambda, scale[3];
  int n_tiles, n, n_cands, n_sets, n_tx;
  int bw, bh, xdec, ydec, bd;
  int psy, use_tx, coeff_rate, has_commit;
  int w_in_b, h_in_b, w_imp;
  int lanes_log2;
  int lsx, L;                      // luma 8x8 sub-blocks: per row, in all
  int cbw, cbh, csx, C, cmw, cmh;  // chroma sub-blocks: pixels, per row, per plane, bias area
  int items;                       // L + 2 * C
  // byte offsets in a block's LDS: biases f64 [L + C], sums u64 [chunk][3],
  // candidate words i32 [chunk], the winner's set, the source planes u16
  int off_acc, off_info, off_src[3], lds_per_block;
  MdTx tx[19];
};

// `(x as u64)` of Rust: saturating, NaN -> 0
__device__ __forceinline__ uint64_t f64_as_u64(double v) {
  if (!(v > 0.0)) return 0;
  return v >= 18446744073709551616.0 ? ~0ull : (uint64_t)v;
}

template <typename Px, int N>
__device__ __forceinline__ void md_row(const Px *p, int32_t *o) {
  struct V {
    Px v[N];
  } t;
  __builtin_memcpy(&t, p, sizeof t);
#pragma unroll
  for (int i = 0; i < N; i++) o[i] = (int32_t)t.v[i];
}

// sse_wxh's inner sum (src/rdo.rs:304-321) of a W-wide sub-block of h rows
template <typename Px, int W>
__device__ __forceinline__ uint64_t md_sse(const uint16_t *s, int ss, const Px *c, int64_t cs, int h) {
  uint64_t v = 0;
  for (int r = 0; r < h; r++) {
    int32_t a[W], b[W];
    md_row<uint16_t, W>(s + r * ss, a);
    md_row<Px, W>(c + r * cs, b);
    uint32_t row = 0;
#pragma unroll
    for (int q = 0; q < W; q++) {
      const int32_t d = (int32_t)(int16_t)a[q] - (int32_t)(int16_t)b[q];
      row += (uint32_t)(d * d);
    }
    v += row;
  }
  return v;
}

// has_coeff of a candidate (src/encoder.rs:1140-1142, 1173-1189, 1812, 1914-1916)
__device__ __forceinline__ int md_has_coeff(const MdArgs &a, int flags, int eob_off, const MdTx &t) {
  if (flags & RV_MODE_CAND_SKIP) return 0;
  if (!((flags & RV_MODE_CAND_NEED_RECON_PIXEL) || a.coeff_rate)) return 1;
  const int nb = t.nb[0] + t.nb[1] + t.nb[2];
  int any = 0;
  for (int i = 0; i < nb; i++) any |= a.eob[eob_off + i] != 0;
  return any;
}

template <typename Px>
__global__ __launch_bounds__(kMdThreads) void mode_decide_kernel(MdArgs a) {
  extern __shared__ __align__(16) unsigned char md_lds[];
  __shared__ const void *cand_tab[3][RV_INTER_MAX_CANDS];
  __shared__ MdTx tx_tab[19];
  __shared__ int wg_max;
  const int tid = threadIdx.x, G = 1 << a.lanes_log2;
  const int lane = tid & (G - 1), slot = tid >> a.lanes_log2;
  const int blk = blockIdx.x * (kMdThreads >> a.lanes_log2) + slot;
  const int bw4 = a.bw >> 2, bh4 = a.bh >> 2;

  // the tables a lane indexes by its own values go to LDS, read as memory from
  // the kernel's argument segment (indexing `a` itself by a lane's value would
  // hold all of it in registers)
  {
    typedef const MdArgs __attribute__((address_space(4))) *KArgs;
    KArgs ka = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    if (tid < 3 * RV_INTER_MAX_CANDS)
      cand_tab[tid / RV_INTER_MAX_CANDS][tid % RV_INTER_MAX_CANDS] =
          ka->cand[tid / RV_INTER_MAX_CANDS][tid % RV_INTER_MAX_CANDS];
    if (tid >= 64 && tid < 64 + 19) {
      const MdTx __attribute__((address_space(4))) *t = &ka->tx[tid - 64];
      MdTx v;
      for (int p = 0; p < 3; p++) v.nb[p] = t->nb[p], v.cols[p] = t->cols[p], v.tw4[p] = t->tw4[p], v.th4[p] = t->th4[p];
      v.valid = t->valid;
      tx_tab[tid - 64] = v;
    }
  }
  if (tid == 0) wg_max = 0;
  __syncthreads();

  unsigned char *lds = md_lds + (size_t)slot * a.lds_per_block;
  double *bias = (double *)lds;
  unsigned long long *acc = (unsigned long long *)(lds + a.off_acc);
  int32_t *info = (int32_t *)(lds + a.off_info);
  int32_t *winner = info + kMdChunk;

  // ---- the block and its checks: a rejected block touches no pixel ----------
  bool ok = false;
  rv_mode_block b = {};
  rv_intra_tile tl = {};
  if (blk < a.n) {
    b = a.blocks[blk];
    ok = b.tile >= 0 && b.tile < a.n_tiles && b.bo_x >= 0 && b.bo_y >= 0 && b.bo_x <= (1 << 20) &&
         b.bo_y <= (1 << 20) && b.bo_x % bw4 == 0 && b.bo_y % bh4 == 0 && b.cand_first >= 0 &&
         b.cand_count >= 0 && b.cand_count <= a.n_cands && b.cand_first <= a.n_cands - b.cand_count;
    if (ok) {
      tl = a.tiles[b.tile];
      ok = tl.x >= 0 && tl.y >= 0 && tl.x <= (1 << 24) && tl.y <= (1 << 24) && tl.width >= 0 &&
           tl.height >= 0 && 4 * (b.bo_x + bw4) <= tl.width && 4 * (b.bo_y + bh4) <= tl.height;
#pragma unroll
      for (int p = 0; p < 3; p++) {  // the block inside the planes' allocations
        const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
        const int fx = (tl.x >> xd) + ((b.bo_x >> xd) << 2), fy = (tl.y >> yd) + ((b.bo_y >> yd) << 2);
        ok = ok && fx + (a.bw >> xd) <= a.g[p].stride - a.g[p].xorigin &&
             fy + (a.bh >> yd) <= a.g[p].alloc_height - a.g[p].yorigin;
      }
    }
    if (!ok && lane == 0) atomicAdd(a.status, 1u);
  }
  const int count = ok ? b.cand_count : 0;
  if (lane == 0 && count) atomicMax(&wg_max, count);

  // ---- the source pixels and the sub-blocks' biases, once per block ---------
  if (ok) {
#pragma unroll
    for (int p = 0; p < 3; p++) {
      const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
      const int w = a.bw >> xd, h = a.bh >> yd;
      const int fx = (tl.x >> xd) + ((b.bo_x >> xd) << 2), fy = (tl.y >> yd) + ((b.bo_y >> yd) << 2);
      const Px *sp = (const Px *)a.src[p] + (int64_t)(a.g[p].yorigin + fy) * a.g[p].stride +
                     a.g[p].xorigin + fx;
      uint16_t *d = (uint16_t *)(lds + a.off_src[p]);
      for (int i = lane; i < w * h; i += G) {
        const int r = i / w, q = i - r * w;
        d[i] = (uint16_t)sp[(int64_t)r * a.g[p].stride + q];
      }
    }
    for (int i = lane; i < a.L + a.C; i += G) {
      if (i < a.L) {  // BLOCK_8X8 at the 8x8 sub-block (src/rdo.rs:268-281, 302-331)
        const int sx = i % a.lsx, sy = i / a.lsx;
        bias[i] = distortion_bias(a.imp, a.w_imp, a.w_in_b, a.h_in_b, (tl.x >> 2) + b.bo_x + 2 * sx,
                                  (tl.y >> 2) + b.bo_y + 2 * sy, 2, 2);
      } else {  // imp_bsize at the chroma sub-block's frame_block_offset
        const int j = i - a.L, sx = j % a.csx, sy = j / a.csx;
        const int px = (tl.x >> a.xdec) + ((b.bo_x >> a.xdec) << 2) + sx * a.cbw;
        const int py = (tl.y >> a.ydec) + ((b.bo_y >> a.ydec) << 2) + sy * a.cbh;
        bias[i] = distortion_bias(a.imp, a.w_imp, a.w_in_b, a.h_in_b, px >> (2 - a.xdec),
                                  py >> (2 - a.ydec), a.cmw, a.cmh);
      }
    }
  }
  __syncthreads();

  const int nchunks = (wg_max + kMdChunk - 1) / kMdChunk;
  for (int ch = 0; ch < nchunks; ch++) {
    const int c0 = ch * kMdChunk;
    const int nc = count - c0 < kMdChunk ? (count - c0 > 0 ? count - c0 : 0) : kMdChunk;
    // ---- 1. the chunk's candidates and their checks -------------------------
    if (lane < kMdChunk) {
      int32_t w = 0;
      if (lane < nc) {
        const rv_mode_cand c = a.cands[b.cand_first + c0 + lane];
        const bool skip = (c.flags & RV_MODE_CAND_SKIP) != 0;
        bool v = c.set >= 0 && c.set < a.n_sets && c.tx_size >= 0 && c.tx_size < 19;
        if (v) {
          const MdTx t = tx_tab[c.tx_size];
          const int nb = t.nb[0] + t.nb[1] + t.nb[2];
          v = t.valid && (skip || (c.dist_off >= 0 && c.eob_off >= 0 && nb <= a.n_tx &&
                                   c.dist_off <= a.n_tx - nb && c.eob_off <= a.n_tx - nb));
        }
        if (v) {
          const bool pixels = !a.use_tx || (c.flags & RV_MODE_CAND_NEED_RECON_PIXEL) || skip;
          w = c.set | kMdValid | (pixels ? kMdPixels : 0);
        } else {
          atomicAdd(a.status + 1, 1u);
        }
      }
      info[lane] = w;
      acc[lane * 3 + 0] = 0, acc[lane * 3 + 1] = 0, acc[lane * 3 + 2] = 0;
    }
    __syncthreads();

    // ---- 2. (candidate, sub-block): the biased distortion of a sub-block -----
    for (int t = lane; t < nc * a.items; t += G) {
      const int c = t / a.items, it = t - c * a.items;
      const int32_t w = info[c];
      if (!(w & kMdPixels)) continue;
      const int set = w & 0xff;
      uint64_t v;
      int p = 0;
      if (it < a.L) {
        const int sx = it % a.lsx, sy = it / a.lsx;
        const int fx = tl.x + 4 * b.bo_x + 8 * sx, fy = tl.y + 4 * b.bo_y + 8 * sy;
        const Px *cp = (const Px *)cand_tab[0][set] + (int64_t)(a.g[0].yorigin + fy) * a.g[0].stride +
                       a.g[0].xorigin + fx;
        const uint16_t *sp = (const uint16_t *)(lds + a.off_src[0]) + sy * 8 * a.bw + sx * 8;
        if (a.psy) {  // cdef_dist_wxh_8x8's sums (src/rdo.rs:229-244)
          int32_t ss = 0, sd = 0;
          uint32_t ss2 = 0, sd2 = 0, ssd = 0;
          for (int r = 0; r < 8; r++) {
            int32_t x[8], y[8];
            md_row<uint16_t, 8>(sp + r * a.bw, x);
            md_row<Px, 8>(cp + (int64_t)r * a.g[0].stride, y);
#pragma unroll
            for (int q = 0; q < 8; q++) {
              ss += x[q], sd += y[q];
              ss2 += (uint32_t)(x[q] * x[q]), sd2 += (uint32_t)(y[q] * y[q]);
              ssd += (uint32_t)(x[q] * y[q]);
            }
          }
          v = cdef_dist_finish(ss, sd, ss2, sd2, ssd, a.bd);
        } else {
          v = md_sse<Px, 8>(sp, a.bw, cp, a.g[0].stride, 8);
        }
        v = distortion_biased(v, bias[it]);
      } else {
        int j = it - a.L;
        p = j < a.C ? 1 : 2;
        j -= (p - 1) * a.C;
        const MdGeom g = p == 1 ? a.g[1] : a.g[2];
        const int sx = j % a.csx, sy = j / a.csx, cw = a.bw >> a.xdec;
        const int fx = (tl.x >> a.xdec) + ((b.bo_x >> a.xdec) << 2) + sx * a.cbw;
        const int fy = (tl.y >> a.ydec) + ((b.bo_y >> a.ydec) << 2) + sy * a.cbh;
        const Px *cp = (const Px *)cand_tab[p][set] + (int64_t)(g.yorigin + fy) * g.stride + g.xorigin + fx;
        const uint16_t *sp =
            (const uint16_t *)(lds + (p == 1 ? a.off_src[1] : a.off_src[2])) + sy * a.cbh * cw + sx * a.cbw;
        if (a.cbw == 8) v = md_sse<Px, 8>(sp, cw, cp, g.stride, a.cbh);
        else if (a.cbw == 4) v = md_sse<Px, 4>(sp, cw, cp, g.stride, a.cbh);
        else v = md_sse<Px, 2>(sp, cw, cp, g.stride, a.cbh);
        v = distortion_biased(v, bias[a.L + j]);
      }
      atomicAdd(acc + c * 3 + p, (unsigned long long)v);
    }
    __syncthreads();

    // ---- 3. one lane per candidate: the ScaledDistortion and the cost ---------
    if (lane < nc) {
      const int idx = b.cand_first + c0 + lane;
      const int32_t w = info[lane];
      uint64_t dist = 0;
      double cost = DBL_MAX;
      int state = RV_MODE_STATE_REJECTED;
      if (w & kMdValid) {
        const rv_mode_cand c = a.cands[idx];
        if (w & kMdPixels) {  // each plane `* fi.dist_scale[p]` on its own (src/rdo.rs:375, 406)
          dist = f64_as_u64((double)acc[lane * 3 + 0] * a.scale[0]) +
                 f64_as_u64((double)acc[lane * 3 + 1] * a.scale[1]) +
                 f64_as_u64((double)acc[lane * 3 + 2] * a.scale[2]);
        } else {  // RawDistortion(d) * bias * dist_scale[p] per transform block (src/encoder.rs:1234-1236)
          const MdTx t = tx_tab[c.tx_size];
          int o = c.dist_off;
#pragma unroll
          for (int p = 0; p < 3; p++) {
            const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
            for (int i = 0; i < t.nb[p]; i++) {
              const int bx = i % t.cols[p], by = i / t.cols[p];
              // tx_bo (src/encoder.rs:1785-1788, 1864-1869); the partition's bsize
              const double bs = distortion_bias(a.imp, a.w_imp, a.w_in_b, a.h_in_b,
                                                (tl.x >> 2) + b.bo_x + ((bx * t.tw4[p]) << xd),
                                                (tl.y >> 2) + b.bo_y + ((by * t.th4[p]) << yd), bw4, bh4);
              dist += f64_as_u64((double)distortion_biased(a.dist[o++], bs) * a.scale[p]);
            }
          }
        }
        // compute_rd_cost (src/rdo.rs:563-568)
        cost = (double)dist + a.lambda * ((double)c.rate / 8.0);
        state = RV_MODE_STATE_EVALUATED;
      }
      a.cand_dist[idx] = dist, a.cand_cost[idx] = cost, a.cand_state[idx] = state;
    }
    __syncthreads();
  }

  // ---- the walk: one lane per block ------------------------------------------
  if (lane == 0 && blk < a.n) {
    // best: the seed's (or the default's) until a candidate replaces it; only
    // what the walk reads is kept, the record is formed once at the end
    double best_rd = DBL_MAX;
    bool best_skip = false;
    if (ok && a.seed) best_rd = a.seed[blk].rd_cost, best_skip = a.seed[blk].skip != 0;
    uint64_t best_dist = 0;
    int best_cand = -1, wset = -1;
    bool first = true, zero = false, gate = false;
    int group = 0;
    for (int k = 0; k < count; k++) {
      const int idx = b.cand_first + k;
      if (a.cand_state[idx] == RV_MODE_STATE_REJECTED) continue;
      const rv_mode_cand *c = a.cands + idx;
      const int flags = c->flags, grp = c->group;
      const bool intra = (flags & RV_MODE_CAND_INTRA) != 0, skip = (flags & RV_MODE_CAND_SKIP) != 0;
      if (first || grp != group) {  // a luma_chroma_mode_rdo call begins
        first = false, group = grp, zero = false;
        gate = intra && best_skip;  // src/rdo.rs:1008
      }
      if (intra ? gate : (!skip && zero)) {  // :774-780
        a.cand_state[idx] = intra ? RV_MODE_STATE_GATED_SKIP : RV_MODE_STATE_GATED_ZERO_DIST;
        continue;
      }
      const double rd = a.cand_cost[idx];
      if (rd < best_rd) {  // :752-765
        best_rd = rd, best_dist = a.cand_dist[idx], best_cand = idx, best_skip = skip;
        wset = c->set;
        if (!intra && skip) zero = best_dist == 0;
      }
    }
    rv_mode_decision *o = a.out + blk;
    if (best_cand >= 0) {
      const rv_mode_cand *c = a.cands + best_cand;
      o->pay = c->pay;
      o->rd_cost = best_rd, o->distortion = best_dist, o->rate = c->rate, o->cand = best_cand;
      o->skip = best_skip, o->tx_size = c->tx_size, o->reserved = 0;
      o->has_coeff = md_has_coeff(a, c->flags, c->eob_off, tx_tab[c->tx_size]);
    } else if (ok && a.seed) {
      *o = a.seed[blk];
      o->cand = -1;
    } else {
      *o = rv_mode_decision{};
      o->rd_cost = DBL_MAX, o->cand = -1;
    }
    winner[0] = wset;
  }
  __syncthreads();

  // ---- commit: the winner's partition pixels of every plane ------------------
  if (!a.has_commit || !ok) return;
  const int wset = winner[0];
  if (wset < 0) return;
#pragma unroll
  for (int p = 0; p < 3; p++) {
    const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
    const int w = a.bw >> xd, h = a.bh >> yd;
    const int fx = (tl.x >> xd) + ((b.bo_x >> xd) << 2), fy = (tl.y >> yd) + ((b.bo_y >> yd) << 2);
    const int64_t o = (int64_t)(a.g[p].yorigin + fy) * a.g[p].stride + a.g[p].xorigin + fx;
    const Px *cp = (const Px *)cand_tab[p][wset] + o;
    Px *dp = (Px *)a.commit[p] + o;
    for (int i = lane; i < w * h; i += G) {
      const int r = i / w, q = i - r * w;
      dp[(int64_t)r * a.g[p].stride + q] = cp[(int64_t)r * a.g[p].stride + q];
    }
  }
}

struct SegArgs {
  const rv_intra_tile *tiles;
  const rv_mode_block *blocks;
  const float *imp;
  int32_t *sidx, *qindex;
  float *mean;
  uint32_t *status;
  int n_tiles, n, bw4, bh4, base_q_idx, w_imp, w_in_b, h_in_b;
  int data[3];
};

__global__ __launch_bounds__(256) void block_segment_kernel(SegArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const rv_mode_block b = a.blocks[i];
  bool ok = b.tile >= 0 && b.tile < a.n_tiles && b.bo_x >= 0 && b.bo_y >= 0 && b.bo_x <= (1 << 20) &&
            b.bo_y <= (1 << 20);
  rv_intra_tile tl = {};
  if (ok) {
    tl = a.tiles[b.tile];
    ok = tl.x >= 0 && tl.y >= 0 && tl.x <= (1 << 24) && tl.y <= (1 << 24);
  }
  int sidx = 0;
  float mean = 0.f;
  if (ok) {
    mean = mean_importance(a.imp, a.w_imp, a.w_in_b, a.h_in_b, (tl.x >> 2) + b.bo_x,
                           (tl.y >> 2) + b.bo_y, a.bw4, a.bh4);
    // src/rdo.rs:664-679 (an importance that is no number >= 0 is unreachable!() there)
    sidx = mean >= 4.f ? 2 : mean >= 2.f ? 0 : 1;
    const int d = sidx == 2 ? a.data[2] : sidx == 1 ? a.data[1] : a.data[0];
    if (a.base_q_idx + d < 2) sidx = 0;
  } else {
    atomicAdd(a.status, 1u);
  }
  const int d = sidx == 2 ? a.data[2] : sidx == 1 ? a.data[1] : a.data[0];
  a.sidx[i] = sidx;
  a.qindex[i] = clampi(a.base_q_idx + d, 0, 255);  // get_qidx (src/encoder.rs:1061-1072)
  a.mean[i] = mean;
}

static int md_fail(int code, const char *who, const char *what) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return rv_set_error(code, msg);
}

// Default lanes per block: one lane per eight luma pixels, 8 .. 256.  Measured
// on the squares at 4:2:0: 8 lanes at 8x8, 32 at 16x16, 128 at
// 32x32 and 256 at 64x64 were the fastest packings; the rectangles follow the
// same rule.
static int md_default_lanes(int bw, int bh) {
  const int l = bw * bh / 8;
  return l < kMdChunk ? kMdChunk : (l > kMdThreads ? kMdThreads : l);
}

// Everything about a launch that can be checked without one, and the launch's
// geometry in `a`.
static int md_prepare(const rv_plane *src, const rv_plane *cands, int n_sets, const rv_plane *commit,
                      const rv_mode_decide_params *params, bool has_importance, int lanes, MdArgs &a) {
  const char *who = "rv_mode_decide_batch";
  if (!params || !src || !cands) return md_fail(RV_EINVAL, who, "null argument");
  const rv_mode_decide_params &P = *params;
  const int bd = P.bit_depth;
  if (bd != 8 && bd != 10 && bd != 12) return md_fail(RV_EINVAL, who, "bit_depth must be 8, 10 or 12");
  const int xdec = src[1].xdec, ydec = src[1].ydec;
  // the sizes and layouts rv_tx_blocks_batch takes, with its codes
  rv_tx_blocks_layout_t lay;
  const int rc = txb_layout(P.bsize, 0, xdec, ydec, 0, &lay);
  if (rc != RV_OK) return rc;
  if (P.tune != RV_TUNE_PSNR && P.tune != RV_TUNE_PSYCHOVISUAL) return md_fail(RV_EINVAL, who, "tune is no RV_TUNE_*");
  if (P.use_tx_domain_distortion && P.tune != RV_TUNE_PSNR)  // compute_tx_distortion's assert (src/rdo.rs:419)
    return md_fail(RV_EINVAL, who, "use_tx_domain_distortion needs RV_TUNE_PSNR");
  if (n_sets < 1 || n_sets > RV_INTER_MAX_CANDS) return md_fail(RV_EINVAL, who, "n_sets is 1 .. 20");
  if (lanes != 0 && (lanes < kMdChunk || lanes > kMdThreads || (lanes & (lanes - 1))))
    return md_fail(RV_EINVAL, who, "lanes is 0 or a power of two 8 .. 256");
  if (P.w_in_b < 1 || P.h_in_b < 1) return md_fail(RV_EINVAL, who, "w_in_b / h_in_b below 1");
  if (has_importance && P.w_imp < (P.w_in_b + 1) / 2)
    return md_fail(RV_EINVAL, who, "w_imp below ceil(w_in_b / 2)");

  const size_t px = bd > 8 ? 2 : 1;
  for (int p = 0; p < 3; p++) {
    const rv_plane &g0 = src[p];
    for (int k = 0; k < n_sets + 2; k++) {
      if (k == n_sets + 1 && !commit) continue;
      const rv_plane &pl = k == 0 ? src[p] : k <= n_sets ? cands[3 * (k - 1) + p] : commit[p];
      if (!pl.data) return md_fail(RV_EINVAL, who, "a plane without data");
      if (pl.hbd != (bd > 8)) return md_fail(RV_EINVAL, who, "pixel type does not fit bit_depth");
      if (pl.xdec != (p ? xdec : 0) || pl.ydec != (p ? ydec : 0))
        return md_fail(RV_EINVAL, who, "the plane sets differ in subsampling");
      if (pl.stride != g0.stride || pl.alloc_height != g0.alloc_height || pl.xorigin != g0.xorigin ||
          pl.yorigin != g0.yorigin)
        return md_fail(RV_EINVAL, who, "the plane sets differ in geometry");
    }
    if (g0.stride <= 0 || g0.alloc_height <= 0 || g0.xorigin < 0 || g0.yorigin < 0)
      return md_fail(RV_EINVAL, who, "a plane's geometry is not positive");
    if (commit) {  // a candidate set is read while commit is written
      const size_t bytes = (size_t)g0.stride * g0.alloc_height * px;
      const char *d0 = (const char *)commit[p].data;
      for (int k = 0; k < n_sets; k++) {
        const char *r0 = (const char *)cands[3 * k + p].data;
        if (d0 < r0 + bytes && r0 < d0 + bytes) return md_fail(RV_EINVAL, who, "commit overlaps a candidate set");
      }
      a.commit[p] = commit[p].data;
    }
    a.g[p] = MdGeom{g0.stride, g0.alloc_height, g0.xorigin, g0.yorigin};
    a.src[p] = g0.data;
    for (int k = 0; k < RV_INTER_MAX_CANDS; k++) a.cand[p][k] = cands[3 * (k < n_sets ? k : 0) + p].data;
  }
  const int bw = kTxbBlkW[P.bsize], bh = kTxbBlkH[P.bsize];
  a.bw = bw, a.bh = bh, a.xdec = xdec, a.ydec = ydec, a.bd = bd;
  a.psy = P.tune == RV_TUNE_PSYCHOVISUAL, a.use_tx = P.use_tx_domain_distortion != 0;
  a.coeff_rate = P.coeff_rate != 0, a.has_commit = commit != nullptr;
  a.w_in_b = P.w_in_b, a.h_in_b = P.h_in_b, a.w_imp = P.w_imp;
  a.lambda = P.lambda;
  for (int p = 0; p < 3; p++) a.scale[p] = P.dist_scale[p];
  // sse_wxh's sub-blocks (src/rdo.rs:293-299) of luma and of w_uv x h_uv (:380-382)
  const int w_uv = bw >> xdec, h_uv = bh >> ydec;
  const int iw = w_uv < 8 ? w_uv : 8, ih = h_uv < 8 ? h_uv : 8;
  a.lsx = bw / 8, a.L = (bw / 8) * (bh / 8);
  a.cbw = iw >> xdec, a.cbh = ih >> ydec, a.cmw = iw >> 2, a.cmh = ih >> 2;
  a.csx = w_uv / a.cbw, a.C = a.csx * (h_uv / a.cbh);
  a.items = a.L + 2 * a.C;
  for (int ts = 0; ts < 19; ts++) {
    if (kTxbTxW[ts] > bw || kTxbTxH[ts] > bh) continue;
    if (txb_layout(P.bsize, ts, xdec, ydec, 0, &lay) != RV_OK) continue;
    MdTx &t = a.tx[ts];
    t.valid = 1;
    for (int p = 0; p < 3; p++) {
      t.nb[p] = (uint16_t)lay.n_blocks[p], t.cols[p] = (uint8_t)lay.cols[p];
      t.tw4[p] = kTxbTxW[lay.tx_size[p]] >> 2, t.th4[p] = kTxbTxH[lay.tx_size[p]] >> 2;
    }
  }
  int off = (a.L + a.C) * 8;
  a.off_acc = off, off += kMdChunk * 3 * 8;
  a.off_info = off, off += (kMdChunk + 8) * 4;
  for (int p = 0; p < 3; p++) {
    off = (off + 15) & ~15;
    a.off_src[p] = off, off += (p ? w_uv * h_uv : bw * bh) * 2;
  }
  a.lds_per_block = (off + 15) & ~15;
  const int L = lanes ? lanes : md_default_lanes(bw, bh);
  a.lanes_log2 = 31 - __builtin_clz((unsigned)L);
  const int bpw = kMdThreads / L;
  const size_t lds = (size_t)a.lds_per_block * bpw;
  if (lds > 60 * 1024) {
    if (lanes) return md_fail(RV_EINVAL, who, "too few lanes per block for this block size (LDS)");
    return md_fail(RV_EHIP, who, "internal: the default packing exceeds the LDS");
  }
  return RV_OK;
}

}  // namespace rv

using namespace rv;

extern "C" int rv_segmentation_data(int base_q_idx, int16_t data[3]) {
  if (!data || base_q_idx < 0 || base_q_idx > 255)
    return md_fail(RV_EINVAL, "rv_segmentation_data", "null data or base_q_idx outside 0 .. 255");
  // segmentation_optimize (src/segmentation.rs:29-48)
  const int lo = 1 - base_q_idx;
  data[0] = 0, data[1] = 21, data[2] = (int16_t)(lo > -21 ? lo : -21);
  return RV_OK;
}

extern "C" int rv_block_segment_batch(const rv_intra_tile *d_tiles, int n_tiles,
                                      const rv_mode_block *d_blocks, int n, int bsize, int base_q_idx,
                                      const int16_t data[3], const float *d_importance, int w_imp,
                                      int w_in_b, int h_in_b, int32_t *d_sidx, int32_t *d_qindex,
                                      float *d_mean, uint32_t *d_status, void *stream) {
  const char *who = "rv_block_segment_batch";
  if (!data || !d_status || n < 0 || n_tiles < 0) return md_fail(RV_EINVAL, who, "null argument or negative count");
  if (bsize < 0 || bsize > 21) return md_fail(RV_EINVAL, who, "bsize is no BlockSize");
  if (bsize > 12) return md_fail(RV_ENOTSUP, who, "4:1 / 1:4 partitions and sizes above 64x64 are not supported");
  if (base_q_idx < 0 || base_q_idx > 255) return md_fail(RV_EINVAL, who, "base_q_idx outside 0 .. 255");
  if (w_in_b < 1 || h_in_b < 1) return md_fail(RV_EINVAL, who, "w_in_b / h_in_b below 1");
  if (d_importance && w_imp < (w_in_b + 1) / 2)
    return md_fail(RV_EINVAL, who, "w_imp below ceil(w_in_b / 2)");
  if (n > 0 && (!d_tiles || n_tiles == 0 || !d_blocks || !d_sidx || !d_qindex || !d_mean))
    return md_fail(RV_EINVAL, who, "null blocks, tiles or outputs");
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess) return rv_set_hip_error(hipGetLastError(), who);
  if (n == 0) return RV_OK;
  SegArgs a = {};
  a.tiles = d_tiles, a.blocks = d_blocks, a.imp = d_importance;
  a.sidx = d_sidx, a.qindex = d_qindex, a.mean = d_mean, a.status = d_status;
  a.n_tiles = n_tiles, a.n = n, a.bw4 = kTxbBlkW[bsize] >> 2, a.bh4 = kTxbBlkH[bsize] >> 2;
  a.base_q_idx = base_q_idx, a.w_imp = w_imp, a.w_in_b = w_in_b, a.h_in_b = h_in_b;
  for (int i = 0; i < 3; i++) a.data[i] = data[i];
  block_segment_kernel<<<(n + 255) / 256, 256, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_mode_decide_check(const rv_plane *src, const rv_plane *cands, int n_sets,
                                    const rv_plane *commit, const rv_mode_decide_params *params,
                                    int has_importance, int lanes) {
  MdArgs a = {};
  return md_prepare(src, cands, n_sets, commit, params, has_importance != 0, lanes, a);
}

extern "C" int rv_mode_decide_batch_lanes(
    const rv_plane *src, const rv_plane *cands, int n_sets, const rv_plane *commit,
    const rv_intra_tile *d_tiles, int n_tiles, const rv_mode_block *d_blocks, int n,
    const rv_mode_cand *d_cands, int n_cands, const rv_mode_decision *d_seed, const uint64_t *d_dist,
    const uint32_t *d_eob, int n_tx, const float *d_importance, const rv_mode_decide_params *params,
    rv_mode_decision *d_out, uint64_t *d_cand_dist, double *d_cand_cost, int32_t *d_cand_state,
    uint32_t *d_status, int lanes, void *stream) {
  const char *who = "rv_mode_decide_batch";
  if (!d_status || n < 0 || n_tiles < 0 || n_cands < 0 || n_tx < 0)
    return md_fail(RV_EINVAL, who, "null argument or negative count");
  MdArgs a = {};
  const int rc = md_prepare(src, cands, n_sets, commit, params, d_importance != nullptr, lanes, a);
  if (rc != RV_OK) return rc;
  if (n > 0 && (!d_blocks || !d_tiles || n_tiles == 0 || !d_out)) return md_fail(RV_EINVAL, who, "null blocks, tiles or output");
  if (n_cands > 0 && (!d_cands || !d_cand_dist || !d_cand_cost || !d_cand_state))
    return md_fail(RV_EINVAL, who, "null candidates or candidate outputs");
  if (n_tx > 0 && (!d_dist || !d_eob)) return md_fail(RV_EINVAL, who, "null d_dist or d_eob");
  if (n > (1 << 24) || n_cands > (1 << 28)) return md_fail(RV_EINVAL, who, "n above 2^24 or n_cands above 2^28");

  const int bpw = kMdThreads >> a.lanes_log2;
  const size_t lds = (size_t)a.lds_per_block * bpw;

  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 8, st) != hipSuccess) return rv_set_hip_error(hipGetLastError(), who);
  if (n_cands > 0 &&
      (hipMemsetAsync(d_cand_dist, 0, (size_t)n_cands * 8, st) != hipSuccess ||
       hipMemsetAsync(d_cand_cost, 0, (size_t)n_cands * 8, st) != hipSuccess ||
       hipMemsetAsync(d_cand_state, 0, (size_t)n_cands * 4, st) != hipSuccess))
    return rv_set_hip_error(hipGetLastError(), who);
  if (n == 0) return RV_OK;
  a.tiles = d_tiles, a.blocks = d_blocks, a.cands = d_cands, a.seed = d_seed;
  a.dist = d_dist, a.eob = d_eob, a.imp = d_importance;
  a.out = d_out, a.cand_dist = d_cand_dist, a.cand_cost = d_cand_cost, a.cand_state = d_cand_state;
  a.status = d_status;
  a.n_tiles = n_tiles, a.n = n, a.n_cands = n_cands, a.n_sets = n_sets, a.n_tx = n_tx;
  const unsigned grid = (unsigned)((n + bpw - 1) / bpw);
  if (a.bd > 8)
    mode_decide_kernel<uint16_t><<<grid, kMdThreads, lds, st>>>(a);
  else
    mode_decide_kernel<uint8_t><<<grid, kMdThreads, lds, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_mode_decide_batch(const rv_plane *src, const rv_plane *cands, int n_sets,
                                    const rv_plane *commit, const rv_intra_tile *d_tiles, int n_tiles,
                                    const rv_mode_block *d_blocks, int n, const rv_mode_cand *d_cands,
                                    int n_cands, const rv_mode_decision *d_seed, const uint64_t *d_dist,
                                    const uint32_t *d_eob, int n_tx, const float *d_importance,
                                    const rv_mode_decide_params *params, rv_mode_decision *d_out,
                                    uint64_t *d_cand_dist, double *d_cand_cost, int32_t *d_cand_state,
                                    uint32_t *d_status, void *stream) {
  return rv_mode_decide_batch_lanes(src, cands, n_sets, commit, d_tiles, n_tiles, d_blocks, n, d_cands,
                                    n_cands, d_seed, d_dist, d_eob, n_tx, d_importance, params, d_out,
                                    d_cand_dist, d_cand_cost, d_cand_state, d_status, 0, stream);
}

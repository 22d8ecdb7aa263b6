// rv_replay_frame.hip -- one coded frame of the replay (rv_replay.hip's header
// names the stages F0 .. F8).  The kernels only a frame launches: scoring,
// candidate lists, the partition levels, the partition, the block map, the
// importance SATD; the intra pass's host side; the frame's state and stages
// (FrameRun); and rv_replay_frame, the order of those stages.
#include "rv_replay.h"

namespace rv {

// One candidate's rd costs: skip (rs, distortion ds) and non-skip (rn, dn);
// live = rav1e pushes it and it repeats no earlier candidate's MVs.
struct CandCost {
  double rs, rn;
  uint64_t ds, dn;
  int live;
};
__device__ inline CandCost cand_cost(const CandGeo &cg, double lambda, double ds_u, double ds_v,
                                     const rv_fs_result *sub, const uint64_t *lout,
                                     const uint64_t *uout, const uint64_t *vout, int ntx_c, int sb,
                                     int c) {
  CandCost k{0.0, 0.0, 0, 0, 0};
  const int ns = cg.R * cg.M;  // single-reference candidates; compound ones follow
  rv_mv mv;
  if (c < ns ? !cand_live(cg, sub, sb, c, &mv) : !comp_live(cg, sub, sb, c - ns)) return k;
  k.live = 1;
  const int64_t o = (int64_t)c * cg.nsb + sb;
  uint64_t su = 0, sv = 0, nu = 0, nv = 0;
  uint32_t rate = (uint32_t)lout[o * 3 + 2];
  for (int j = 0; j < ntx_c; j++) {
    const int64_t t = (o * ntx_c + j) * 3;
    su += uout[t];
    sv += vout[t];
    nu += uout[t + 1];
    nv += vout[t + 1];
    rate += (uint32_t)uout[t + 2] + (uint32_t)vout[t + 2];
  }
  // Distortion * dist_scale[p] -> ScaledDistortion, summed over planes
  k.ds = (uint64_t)((double)lout[o * 3 + 0] * 1.0) + (uint64_t)((double)su * ds_u) +
         (uint64_t)((double)sv * ds_v);
  k.dn = (uint64_t)((double)lout[o * 3 + 1] * 1.0) + (uint64_t)((double)nu * ds_u) +
         (uint64_t)((double)nv * ds_v);
  k.rs = (double)k.ds + lambda * (0.0 / 8.0);
  k.rn = (double)k.dn + lambda * ((double)rate / 8.0);
  return k;
}
// The argmin step of candidate k after the ones before it (strict <; skip
// first, non-skip unless the skip variant became the best at zero distortion)
__device__ inline void argmin_step(RdoWinner &w, const CandCost &k, int c) {
  if (!k.live) return;
  bool zero_dist = false;
  if (k.rs < w.cost) {
    w = RdoWinner{c, 1, k.rs, k.ds};
    zero_dist = k.ds == 0;
  }
  if (!zero_dist && k.rn < w.cost) w = RdoWinner{c, 0, k.rn, k.dn};
}

// compute_rd_cost + the per-superblock argmin (rdo_mode_decision): the
// candidates in rav1e's order (reference-major: NEARESTMV, NEAR0MV,
// GLOBALMV, NEWMV, then the compound modes), each skip first, then non-skip
// unless the skip variant became the best with zero distortion
// (luma_chroma_mode_rdo, src/rdo.rs:690-700); strict `<`.  ScaledDistortion
// = luma + U + V (dist_scale 1.0); rate = the estimate_rate bits of every
// transform block (the rate model of RDOType::TxDistEstRate,
// src/encoder.rs:1226-1231; the entropy coder's mode and MV bits are out of
// scope); rd = dist as f64 + lambda * rate / 8 (src/rdo.rs:563-569).
__device__ inline RdoWinner block_argmin(const CandGeo &cg, double lambda, double ds_u,
                                         double ds_v, const rv_fs_result *sub,
                                         const uint64_t *lout, const uint64_t *uout,
                                         const uint64_t *vout, int ntx_c, int sb) {
  RdoWinner w{0, 0, 1.7976931348623157e308, 0};  // f64::MAX
  for (int c = 0; c < cg.R * cg.M + cg.comp; c++)
    argmin_step(w, cand_cost(cg, lambda, ds_u, ds_v, sub, lout, uout, vout, ntx_c, sb, c), c);
  return w;
}

// The scoring of the superblocks a round evaluated, one wavefront per
// superblock: lane c costs candidate c (the loads of every candidate in
// flight at once), lane 0 walks the argmin in rav1e's order over the
// wavefront's LDS copy, then the wavefront writes the superblock's winner,
// decision record and result words.  The superblocks: every one (alist
// null, round 0) or the list the round's check wrote (alist[0 .. *acount)).
// A fixed pool of workgroups loops over them.  Block 0 also resets the
// candidate lists' counts (consumed) and, on round 0, the frame's counters.
constexpr int kScoreMaxCands = 2 * kCandModes + kCompModes;
__global__ __launch_bounds__(256) void score_wave_kernel(
    Geo g, CandGeo cg, double lambda, double ds_u, double ds_v, const rv_fs_result *sub,
    const uint64_t *lout, const uint64_t *uout, const uint64_t *vout, int ntx_c, RdoWinner *win,
    const rv_fs_result *coarse, const rv_fs_result *half, const rv_fs_result *full,
    const rv_fs_result *look, const rv_fs_result *half_l, uint64_t *words, int32_t *cand_count,
    unsigned long long *imp_sum, uint32_t *evals, int32_t *leaf_count, const int32_t *alist,
    const int32_t *acount, BlkDec *dec, int round) {
  __shared__ CandCost kc[4][kScoreMaxCands];
  __shared__ RdoWinner ws[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = alist ? __builtin_amdgcn_readfirstlane(*acount) : g.nsb;
  const int nc = cg.R * cg.M + cg.comp;
  const int per = kWordsPerRef * g.R + 4;
  for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    const int sb = alist ? __builtin_amdgcn_readfirstlane(alist[i]) : i;
    if (lane < nc)
      kc[wave][lane] = cand_cost(cg, lambda, ds_u, ds_v, sub, lout, uout, vout, ntx_c, sb, lane);
    wave_sync();
    if (lane == 0) {
      RdoWinner w{0, 0, 1.7976931348623157e308, 0};  // f64::MAX
      for (int c = 0; c < nc; c++) argmin_step(w, kc[wave][c], c);
      ws[wave] = w;
      win[sb] = w;
      if (dec) dec[sb] = blk_dec_of(cg, sub, sb, w.c);
    }
    wave_sync();
    const RdoWinner w = ws[wave];
    uint64_t *base = words + (int64_t)sb * per;
    for (int wi = lane; wi < per; wi += 64) {
      uint64_t v;
      if (wi < kWordsPerRef * g.R) {
        const int r = wi / kWordsPerRef, k = wi - r * kWordsPerRef, e = k >> 1;
        const int64_t o = (int64_t)r * g.nsb + sb;
        // [coarse, 4 half-res quadrants, full-pel, sub-pel, 16 lookahead, the
        // lookahead's 4 half-res quadrants]
        const rv_fs_result &f = e == 0 ? coarse[o] : e < 5 ? half[o * 4 + e - 1] : e == 5 ? full[o]
                                : e == 6 ? sub[o] : e < 23 ? look[o * 16 + e - 7]
                                : half_l[o * 4 + e - 23];
        v = (k & 1) ? f.cost : pack_mv(f.best_mv);
      } else {
        const int j = wi - kWordsPerRef * g.R;
        if (j == 0) {
          v = (uint64_t)w.c;
        } else if (j == 1) {
          v = (uint64_t)w.skip;
        } else if (j == 2) {
          __builtin_memcpy(&v, &w.cost, 8);
        } else {
          v = w.dist;
        }
      }
      base[wi] = v;
    }
    wave_sync();  // kc / ws of this superblock are read before the next one's writes
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // F4's lists are consumed: ready for the next round / frame.  Round 0:
    // the single-reference and compound candidates of the frame's first F4
    // launch (the one the roofline times; later rounds are counted by
    // rv_replay_counters' [15]); F5 sums next; the partition decision
    // appends next (the rounds the intra pass triggers may run after it)
    if (!round) {
      evals[0] = (uint32_t)cand_count[0];
      evals[1] = (uint32_t)cand_count[1];
      if (imp_sum) *imp_sum = 0;  // F5's sum
      if (leaf_count)
        for (int l = 0; l < 4; l++) leaf_count[l] = 0;
    }
    cand_count[0] = cand_count[1] = 0;
  }
}

// The searches' predictor lists (get_subset_predictors, src/me.rs:82-96:
// zero, then the coarse MVs quantize_to_fullpel'd): slot p >= 1 of job i
// takes source src[8 i + p] (-1: none) = 2 * index + kind, kind 0 a coarse
// result (estimate_motion_ss4's MV * 4), 1 a half-res result
// (estimate_motion_ss2's MV * 2); `shr`: me_ss2 halves every predictor.
__global__ void fill_preds_kernel(rv_ds_job *jobs, const int32_t *src, int n,
                                  const rv_fs_result *coarse, const rv_fs_result *half, int shr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int p = 1; p < 8; p++) {  // src: 8 entries per job, [0] unused
    const int v = src[8 * i + p];
    if (v < 0) break;
    const rv_mv m = (v & 1) ? half[v >> 1].best_mv : coarse[v >> 1].best_mv;
    const int sc = (v & 1) ? 2 : 4;
    rv_mv q = qfull(rv_mv{(int16_t)(m.row * sc), (int16_t)(m.col * sc)});
    if (shr) q = rv_mv{(int16_t)(q.row >> 1), (int16_t)(q.col >> 1)};
    jobs[i].pred[p] = q;
  }
}

struct CandKeys {
  CandKey *key;  // [nsingle + nsb * kCompModes]
  uint32_t tag;
  int reuse;     // 0: record only (round 0); 1: skip a slot whose key matches
};
__device__ inline uint32_t mv_bits(rv_mv m) {
  return (uint32_t)(uint16_t)m.row | ((uint32_t)(uint16_t)m.col << 16);
}
// v: the candidate is live; returns whether F4 must evaluate it
__device__ inline bool cand_key_step(const CandKeys &k, int slot, bool v, rv_mv m0, rv_mv m1) {
  if (!v || !k.key) return v;
  const CandKey n{k.tag, mv_bits(m0), mv_bits(m1)};
  const CandKey o = k.key[slot];
  if (k.reuse && o.tag == n.tag && o.mv0 == n.mv0 && o.mv1 == n.mv1) return false;
  k.key[slot] = n;
  return true;
}

// The valid candidates (cand_mv true) of every superblock, compacted for
// the F4 launch: rav1e evaluates only the modes it pushes (about half of
// the 4 per reference on smooth motion: NEWMV often repeats a neighbour's
// MV).  One thread per candidate c * nsb + sb; wave-aggregated appends
// (the order of the list does not matter: every output is indexed by the
// candidate).
__global__ __launch_bounds__(256) void cand_list_kernel(CandGeo cg, const rv_fs_result *sub,
                                                         int n, int32_t *list, int32_t *count,
                                                         const uint8_t *active = nullptr,
                                                         CandKeys keys = CandKeys{nullptr, 0, 0}) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool v = false;
  if (i < n) {
    rv_mv mv;
    const int c = i / cg.nsb, sb = i - c * cg.nsb;
    v = (!active || active[sb]) && cand_live(cg, sub, sb, c, &mv);
    v = cand_key_step(keys, i, v, mv, rv_mv{0, 0});
  }
  const uint64_t m = __ballot(v);
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0 && m) base = atomicAdd(count, (int)__popcll(m));
  base = __shfl(base, 0, 64);
  if (v) list[base + __popcll(m & ((1ull << lane) - 1))] = i;
}
// The compound candidates (all pushed on SELECT frames) without repeated
// MV pairs: entries are absolute candidate indices nsingle + m * nsb + sb.
__global__ __launch_bounds__(256) void comp_list_kernel(CandGeo cg, const rv_fs_result *sub,
                                                         int nsingle, int32_t *list, int32_t *count,
                                                         const uint8_t *active = nullptr,
                                                         CandKeys keys = CandKeys{nullptr, 0, 0}) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool v = false;
  if (i < cg.comp * cg.nsb) {
    const int mm = i / cg.nsb, sb = i - mm * cg.nsb;
    v = (!active || active[sb]) && comp_live(cg, sub, sb, mm);
    if (v && keys.key) {
      rv_mv a0, a1;
      comp_mvs(cg, sub, sb, mm, &a0, &a1);
      v = cand_key_step(keys, nsingle + i, v, a0, a1);
    }
  }
  const uint64_t m = __ballot(v);
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0 && m) base = atomicAdd(count, (int)__popcll(m));
  base = __shfl(base, 0, 64);
  if (v) list[base + __popcll(m & ((1ull << lane) - 1))] = nsingle + i;
}

// The rounds after the first: both candidate lists (single-reference, then
// compound from nsingle on) of the superblocks the round's check listed,
// over a fixed pool of workgroups; wave-aggregated appends as above.
__global__ __launch_bounds__(256) void round_lists_kernel(CandGeo cg, const rv_fs_result *sub,
                                                          int nsingle, int32_t *list,
                                                          int32_t *count, const int32_t *alist,
                                                          const int32_t *acount, CandKeys keys) {
  const int cnt = __builtin_amdgcn_readfirstlane(*acount);
  const int ns = cg.R * cg.M, total = cnt * (ns + cg.comp);
  const int lane = threadIdx.x & 63;
  for (int b0 = blockIdx.x * 256; b0 < total; b0 += gridDim.x * 256) {
    const int i = b0 + (int)threadIdx.x;
    bool v = false;
    int c = 0, sb = 0;
    if (i < total) {
      c = i / cnt;
      sb = alist[i - c * cnt];
      rv_mv mv, m1{0, 0};
      if (c < ns) {
        v = cand_live(cg, sub, sb, c, &mv);
      } else {
        v = comp_live(cg, sub, sb, c - ns);
        if (v) comp_mvs(cg, sub, sb, c - ns, &mv, &m1);
      }
      const int slot = c < ns ? c * cg.nsb + sb : nsingle + (c - ns) * cg.nsb + sb;
      v = cand_key_step(keys, slot, v, mv, m1);
    }
    const bool comp = c >= ns;  // uniform per wavefront only where the split falls between them
    const uint64_t ms = __ballot(v && !comp), mc = __ballot(v && comp);
    int bs = 0, bc = 0;
    if (lane == 0) {
      if (ms) bs = atomicAdd(count, (int)__popcll(ms));
      if (mc) bc = atomicAdd(count + 1, (int)__popcll(mc));
    }
    bs = __shfl(bs, 0, 64);
    bc = __shfl(bc, 0, 64);
    const uint64_t below = (1ull << lane) - 1;
    if (v && !comp) list[bs + __popcll(ms & below)] = c * cg.nsb + sb;
    if (v && comp) list[nsingle + bc + __popcll(mc & below)] = nsingle + (c - ns) * cg.nsb + sb;
  }
}

// F5: get_satd of every 8x8 luma block of the group inside the frame
// against reference 0's original frame at the full-pel part of its
// lookahead MV (the 16x16 block's, fi.lookahead_mvs[y * 2][x * 2];
// compute_block_importances, src/api/internal.rs:823-1010) plus its
// lookahead intra cost (get_satd against pred_dc_128,
// src/api/internal.rs:680-765), summed.  One lane per block; the source
// block is read once for both.
template <typename Px>
__global__ __launch_bounds__(256) void importance_kernel(Geo g, rv_plane org, rv_plane ref,
                                                          const rv_fs_result *look, int nbx,
                                                          int nby, unsigned long long *sum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t v = 0;
  if (i < nbx * nby) {
    const int bx = i % nbx, by = i / nbx;
    const int sb = (by / 8) * g.tw + (bx / 8), q = ((by % 8) / 2) * 4 + (bx % 8) / 2;
    const rv_mv mv = look[sb * 16 + q].best_mv;  // reference 0
    const int x = g.tx0 * kSb + bx * 8, y = g.ty0 * kSb + by * 8;
    const Px *o = plane_ptr<Px>(org, x, y);
    const Px *r = plane_ptr<Px>(ref, x + ((int)mv.col >> 3), y + ((int)mv.row >> 3));
    const int32_t base = 128 << (g.bd - 8);
    int32_t d[64], e[64];
#pragma unroll
    for (int rr = 0; rr < 8; rr++)
#pragma unroll
      for (int cc = 0; cc < 8; cc++) {
        const int32_t ov = (int32_t)o[(int64_t)rr * org.stride + cc];
        d[rr * 8 + cc] = ov - (int32_t)r[(int64_t)rr * ref.stride + cc];
        e[rr * 8 + cc] = ov - base;
      }
    // (sum + (1 << ln >> 1)) >> ln, ln = 3
    v = ((satd_chunk<8>(d) + 4) >> 3) + ((satd_chunk<8>(e) + 4) >> 3);
  }
  block_atomic_add(v, sum);
}

// The full-pel jobs of a level take their pmvs entry as the coarse
// predictor, quantize_to_fullpel'd (get_subset_predictors, src/me.rs:82-96):
// a 32x32 block the half-res search of its quadrant (build_half_res_pmvs),
// a 16x16 / 8x8 block the sub-pel winner of its 32x32 (rdo_mode_decision
// stores b_me into pmvs for 32x32 and 64x64 blocks, src/rdo.rs:866-876).
__global__ void seed_level_kernel(rv_ds_job *jobs, int n, int gw, int R,
                                  const rv_fs_result *parent, int pn, int pgw, int f, int ex0,
                                  int ey0, int tw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * R) return;
  const int k = i / n, b = i - k * n, bx = b % gw, by = b / gw;
  if (pgw == 0) {  // 32x32: the half-res search of its quadrant (pmvs[1..4], MV * 2)
    // the group superblock of the level grid's block (the grid starts at
    // group superblock (ex0, ey0))
    const int sb = (ey0 + (by >> 1)) * tw + ex0 + (bx >> 1), q = (by & 1) * 2 + (bx & 1);
    const rv_mv m = parent[((int64_t)k * pn + sb) * 4 + q].best_mv;
    jobs[i].pred[1] = qfull(rv_mv{(int16_t)(m.row * 2), (int16_t)(m.col * 2)});
    return;
  }
  jobs[i].pred[1] = qfull(parent[k * pn + (by / f) * pgw + bx / f].best_mv);
}

// rdo_mode_decision's winner of every block of a level + its result words
// (the level's full-pel / sub-pel searches, winner, skip, cost, distortion).
__global__ __launch_bounds__(64) void score_level(CandGeo cg, double lambda, double ds_u,
                                                  double ds_v, const rv_fs_result *full,
                                                  const rv_fs_result *sub, const uint64_t *lout,
                                                  const uint64_t *uout, const uint64_t *vout,
                                                  RdoWinner *win, uint64_t *words,
                                                  int32_t *cand_count, uint32_t *evals) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b == 0) {
    evals[0] = (uint32_t)cand_count[0];
    evals[1] = (uint32_t)cand_count[1];
    cand_count[0] = cand_count[1] = 0;
  }
  if (b >= cg.nsb) return;
  const RdoWinner w = block_argmin(cg, lambda, ds_u, ds_v, sub, lout, uout, vout, 1, b);
  win[b] = w;
  uint64_t *wd = words + (int64_t)b * (4 * cg.R + 4);
  for (int k = 0; k < cg.R; k++) {
    const rv_fs_result f = full[k * cg.nsb + b], s = sub[k * cg.nsb + b];
    wd[4 * k + 0] = pack_mv(f.best_mv);
    wd[4 * k + 1] = f.cost;
    wd[4 * k + 2] = pack_mv(s.best_mv);
    wd[4 * k + 3] = s.cost;
  }
  uint64_t cb;
  __builtin_memcpy(&cb, &w.cost, 8);
  wd[4 * cg.R + 0] = (uint64_t)w.c;
  wd[4 * cg.R + 1] = (uint64_t)w.skip;
  wd[4 * cg.R + 2] = cb;
  wd[4 * cg.R + 3] = w.dist;
}

struct PartArgs {
  const RdoWinner *win[kLevels];
  int gw[kLevels];          // level grid width (blocks)
  int x0[kLevels], y0[kLevels];  // level grid origin (frame pixels)
  int ex0, ey0, ew, eh;     // the group superblocks the level grids cover
  int forced;               // speed 10: must_split only (the minimum block is 64x64)
  int32_t *leaf[kLevels];   // the committed blocks of each level
  int32_t *leaf_count;      // [kLevels], zeroed by score_candidates
  uint64_t *words;          // one partition mask per superblock
};

// encode_partition_topdown (src/encoder.rs:2392-2470) over every superblock
// of the group: a block past the frame edge must split; a block that fits
// compares PARTITION_NONE (its mode decision's rd cost) with
// PARTITION_SPLIT (the sum of its four children's, rdo_partition_decision,
// src/rdo.rs:1500-1668; strict `<`; the partition symbol's rate is not
// modelled) and recurses into a split; 8x8 blocks are leaves.  One thread
// per superblock; the leaves go to per-level lists (wave-aggregated
// appends, order irrelevant: every output is indexed by block).
__global__ __launch_bounds__(64) void partition_kernel(Geo g, PartArgs p) {
  const int sb = blockIdx.x * 64 + threadIdx.x;
  const bool live = sb < g.nsb;
  const int gx0 = g.tx0 * kSb, gy0 = g.ty0 * kSb;  // the group (level 0 grid)
  const int X = gx0 + (live ? sb % g.tw : 0) * kSb, Y = gy0 + (live ? sb / g.tw : 0) * kSb;
  const int sx = live ? sb % g.tw - p.ex0 : -1, sy = live ? sb / g.tw - p.ey0 : -1;
  const bool in_rect = sx >= 0 && sy >= 0 && sx < p.ew && sy < p.eh;
  auto idx = [&](int l, int x, int y) {
    const int B = kSb >> l;
    return ((y - p.y0[l]) / B) * p.gw[l] + (x - p.x0[l]) / B;
  };
  auto cost = [&](int l, int x, int y) { return p.win[l][idx(l, x, y)].cost; };
  auto split = [&](int l, int x, int y) -> bool {
    const int B = kSb >> l;
    if (!in_rect) return false;  // no level grid here: the superblock is a leaf
    if (x + B > g.W || y + B > g.H) return true;  // must_split
    if (l == kLevels - 1 || p.forced) return false;
    const int h = B / 2;
    double s = 0.0;
    s += cost(l + 1, x, y);
    s += cost(l + 1, x + h, y);
    s += cost(l + 1, x, y + h);
    s += cost(l + 1, x + h, y + h);
    return 0.0 + s < cost(l, x, y);
  };
  uint32_t mask = 0;
  auto walk = [&](auto emit) {
    if (!live) return;
    if (!split(0, X, Y)) {
      emit(0, X, Y);
      return;
    }
    mask |= 1u;
    for (int q = 0; q < 4; q++) {
      const int x1 = X + (q & 1) * 32, y1 = Y + (q >> 1) * 32;
      if (x1 >= g.W || y1 >= g.H) continue;
      if (!split(1, x1, y1)) {
        emit(1, x1, y1);
        continue;
      }
      mask |= 2u << q;
      for (int r = 0; r < 4; r++) {
        const int x2 = x1 + (r & 1) * 16, y2 = y1 + (r >> 1) * 16;
        if (x2 >= g.W || y2 >= g.H) continue;
        if (!split(2, x2, y2)) {
          emit(2, x2, y2);
          continue;
        }
        mask |= 1u << (5 + ((y2 - Y) / 16) * 4 + (x2 - X) / 16);
        for (int t = 0; t < 4; t++) {
          const int x3 = x2 + (t & 1) * 8, y3 = y2 + (t >> 1) * 8;
          if (x3 < g.W && y3 < g.H) emit(3, x3, y3);
        }
      }
    }
  };
  int cnt[kLevels] = {0, 0, 0, 0};
  walk([&](int l, int, int) { cnt[l]++; });
  const int lane = threadIdx.x & 63;
  int base[kLevels];
  for (int l = 0; l < kLevels; l++) {
    int v = cnt[l];
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    const int total = __shfl(v, 63, 64);
    int b0 = 0;
    if (lane == 63 && total) b0 = atomicAdd(&p.leaf_count[l], total);
    b0 = __shfl(b0, 63, 64);
    base[l] = b0 + v - cnt[l];
  }
  walk([&](int l, int x, int y) { p.leaf[l][base[l]++] = idx(l, x, y); });
  if (live) p.words[sb] = mask;
}

// The deblocking filter's block map: every 4x4 of a committed block gets
// the block's log2 size (4x4 units) and skip flag.  One thread per 4x4 row
// of a block: block i = list ? list[i] : i of the level grid (gw wide,
// origin (x0, y0) in blocks), lg = 4 - level.
__global__ void block_map_kernel(const int32_t *list, const int32_t *count, int n, int gw, int x0,
                                 int y0, int level, const RdoWinner *win, uint8_t *lg,
                                 uint8_t *skip, int mi_stride, int mi_cols, int mi_rows) {
  const int n4 = 16 >> level;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nb = count ? *count : n;
  if (i >= nb * n4) return;
  const int j = i / n4, r = i - j * n4;
  const int b = list ? list[j] : j;
  const int mx = (x0 + b % gw) * n4, my = (y0 + b / gw) * n4 + r;
  if (my >= mi_rows) return;
  const uint8_t sk = (uint8_t)win[b].skip;
  for (int c = 0; c < n4 && mx + c < mi_cols; c++) {
    lg[(int64_t)my * mi_stride + mx + c] = (uint8_t)(4 - level);
    skip[(int64_t)my * mi_stride + mx + c] = sk;
  }
}

}  // namespace rv

// F6b: rdo_mode_decision's intra-mode screening and intra RDO of every
// superblock whose inter winner is not skip (rv_intra_pass.hip), round by
// round until no decision changes.  la / ca: the F6 commit arguments.
// The eligible superblocks (they need only the inter winners): queued right
// after the argmin, so the host's read of their count completes while the
// commit (F6) runs instead of draining the stream.
static int intra_begin(rv_replay *r) {
  const Geo &g = r->g;
  hipStream_t st = r->stream;
  const IntraGeo ig{g.W, g.H, g.bd, g.nsb, g.tw, g.tx0, g.ty0, g.tws, g.ths};
  RV_H(hipMemsetAsync(r->i_cnt, 0, 4 * sizeof(int32_t), st));
  RV_R(rv_intra_elig(ig, r->win, r->i_elig, r->i_was, r->i_mark, r->i_list[0], r->i_cnt, st));
  RV_H(hipMemcpyAsync(r->h_cnt, r->i_cnt, 4, hipMemcpyDeviceToHost, st));
  RV_H(hipEventRecord(r->ev_ielig, st));
  return RV_OK;
}

static int intra_pass(rv_replay *r, const RdoArgs &la, const RdoArgs &ca, const RvInput &cur,
                      const RvSlot &S, const rv_replay::Level &L, int slot, int *nrounds) {
  const Geo &g = r->g;
  hipStream_t st = r->stream;
  const IntraGeo ig{g.W, g.H, g.bd, g.nsb, g.tw, g.tx0, g.ty0, g.tws, g.ths};
  uint32_t *stats = r->i_stats + (size_t)slot * 3;
  RV_H(hipEventSynchronize(r->ev_ielig));  // intra_begin's count
  int n = *r->h_cnt, round = 0;
  // the rounds are bounded by the longest dependency chain of a tile (its
  // anti-diagonals: right, below-left)
  const int max_rounds = g.tws + 2 * g.ths + 4;
  while (n > 0) {
    if (round >= max_rounds)
      return rv_set_error(RV_EHIP, "rv_replay_frame: the intra rounds did not converge");
    const int ci = round & 1;
    int32_t *list = r->i_list[ci], *cnt = r->i_cnt + ci;
    RV_H(hipMemsetAsync(r->i_cnt + (ci ^ 1), 0, sizeof(int32_t), st));
    RV_H(hipMemsetAsync(r->i_cnt + 2, 0, 2 * sizeof(int32_t), st));
    // screening: edges + the modes to try
    IntraScreenArgs sa;
    sa.g = ig;
    sa.rec[0] = S.y;
    sa.rec[1] = S.u;
    sa.rec[2] = S.v;
    sa.org = cur.y;
    sa.list = list;
    sa.count = cnt;
    sa.edges = r->i_edges;
    sa.modes = r->i_modes;
    RV_R(rv_intra_screen(sa, n, g.hbd, st));
    // the intra chains: 3 luma modes, 6 chroma chains per plane
    RdoArgs li = la, cl = ca;
    li.commit = cl.commit = 0;
    li.list = cl.list = list;
    li.count = cl.count = cnt;
    // grids sized by the round's count (the host read it): the lists hold
    // n superblocks, the commit / revert lists at most n
    li.ntx_per_cand = 3;
    li.n_tx = n * 3;
    cl.ntx_per_cand = 6;
    cl.n_tx = n * 6;
    li.iedges = cl.iedges = r->i_edges;
    li.imodes = cl.imodes = r->i_modes;
    li.iwin = cl.iwin = r->i_win;
    li.p[0].q = L.qil;
    li.p[0].out = r->i_lout;
    cl.p[0].q = L.qiu;
    cl.p[1].q = L.qiv;
    cl.p[0].out = r->i_cout;
    cl.p[1].out = r->i_cout + (size_t)g.nsb * 6 * 3;
    RV_R(rv_rdo_intra(li, cl, g.hbd, st));
    // the decisions, the commit / revert lists, the next round
    IntraDecideArgs da;
    da.g = ig;
    da.win = r->win;
    da.modes = r->i_modes;
    da.lout = r->i_lout;
    da.uout = r->i_cout;
    da.vout = r->i_cout + (size_t)g.nsb * 6 * 3;
    da.lambda = L.lambda;
    da.ds_u = L.ds[1];
    da.ds_v = L.ds[2];
    da.list = list;
    da.count = cnt;
    da.iwin = r->i_win;
    da.iwas = r->i_was;
    da.elig = r->i_elig;
    da.mark = r->i_mark;
    da.round = round;
    da.words = r->words;
    da.words_per_sb = kWordsPerRef * g.R + 4;
    da.win_off = kWordsPerRef * g.R;
    da.commit_list = r->i_commit;
    da.commit_count = r->i_cnt + 2;
    da.revert_list = r->i_revert;
    da.revert_count = r->i_cnt + 3;
    da.next_list = r->i_list[ci ^ 1];
    da.next_count = r->i_cnt + (ci ^ 1);
    RV_R(rv_intra_decide(da, st));
    // intra winners into the frame; superblocks back to inter: the F6 chain
    li.commit = cl.commit = 1;
    li.list = cl.list = r->i_commit;
    li.count = cl.count = r->i_cnt + 2;
    li.ntx_per_cand = cl.ntx_per_cand = 1;
    li.n_tx = cl.n_tx = n;
    li.p[0].out = cl.p[0].out = cl.p[1].out = nullptr;
    RV_R(rv_rdo_intra(li, cl, g.hbd, st));
    RdoArgs lr = la, cr = ca;
    lr.list = cr.list = r->i_revert;
    lr.count = cr.count = r->i_cnt + 3;
    lr.n_tx = n;
    cr.n_tx = n * cr.ntx_per_cand;
    RV_R(rv_rdo_candidates(lr, cr, g.hbd, st));
    RV_H(hipMemcpyAsync(r->h_cnt, r->i_cnt + (ci ^ 1), 4, hipMemcpyDeviceToHost, st));
    RV_H(hipStreamSynchronize(st));
    n = *r->h_cnt;
    round++;
  }
  RV_R(rv_intra_stats(g.nsb, r->i_elig, r->i_was, stats, st));
  RV_H(hipMemcpyAsync(stats + 2, &round, 4, hipMemcpyHostToDevice, st));
  if (nrounds) *nrounds = round;
  return RV_OK;
}

// ---- one coded frame ----------------------------------------------------------
namespace {

// Where the 32x32 .. 8x8 levels' searches, candidates and scores run (their
// partition and commit follow from it)
enum class LvPlace {
  kNone,    // no level grids: speed 10, every superblock inside the frame
  kEdge,    // speed 10: on the edge stream, forked before the first check
  kEarly,   // speed 10 without an edge stream: on the main stream before the
            // first check (the stack rounds may read their leaves: a
            // top-right neighbour past the right frame edge)
  kRound0,  // interleaved with round 0's stages on the main stream (speed 6,
            // and speed 10's stand-in stacks without an edge stream)
};

// The levels a stage covers, in order: `only`, or 32x32 .. 8x8; those with
// use[l] set (rv_replay::lv_me: the motion search runs; lv_used: leaves exist)
struct Levels {
  const bool *use;
  int only;
  struct It {
    const Levels *s;
    int l;
    int operator*() const { return l; }
    It &operator++() {
      l = s->next(l + 1);
      return *this;
    }
    bool operator!=(const It &o) const { return l != o.l; }
  };
  int last() const { return only ? only + 1 : kLevels; }
  int next(int l) const {
    while (l < last() && !use[l]) l++;
    return l;
  }
  It begin() const { return It{this, next(only ? only : 1)}; }
  It end() const { return It{this, last()}; }
};

// An error return must not leave the frame-edge levels (edge streams)
// running: the next frame rewrites the MVs they read, and rv_replay_destroy
// frees them.  Armed from before the fork; disarmed once the main stream has
// joined them.
struct SideJoin {
  rv_replay *r;
  bool armed;
  ~SideJoin() {
    for (int l = 1; l < kLevels; l++)
      if (armed && r->edge[l]) (void)hipStreamSynchronize(r->edge[l]);
  }
};

// RAV1E_HIP_HOST_TRACE=1: the host's time per frame phase (stderr)
struct HostTrace {
  using hclock = std::chrono::steady_clock;
  hclock::time_point h0 = hclock::now(), take = h0, r0 = h0, mv = h0, intra = h0;
  static hclock::time_point now() { return hclock::now(); }
  void report(long frame, int lv) const {
    static const bool host_trace = getenv("RAV1E_HIP_HOST_TRACE") != nullptr;
    if (!host_trace) return;
    auto us = [](hclock::time_point a, hclock::time_point b) {
      return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count();
    };
    static thread_local hclock::time_point prev_end = h0;
    const auto h1 = hclock::now();
    fprintf(stderr, "host frame %ld level %d: since-last-exit %ld take %ld r0 %ld mv %ld intra %ld tail %ld us\n",
            frame, lv, us(prev_end, h0), us(h0, take), us(take, r0), us(r0, mv), us(mv, intra),
            us(intra, h1));
    prev_end = h1;
  }
};

// The kernel probes' brackets (rv_replay.h, kp_*) around a probed launch on
// stream xs: open, the launch with acc(p) / ts(p), close.  Off: no-ops, nulls.
struct KProbe {
  rv_replay *r;
  bool on;
  uint32_t *acc(int p) const { return on ? r->kp_cnt[p] : nullptr; }
  int open(hipStream_t xs, int p = 0) const {
    if (!on) return RV_OK;
    if (r->kp_n[p] >= r->kp_init[p]) {
      // the next kKpInit launches' device-clock span slots: start = max,
      // end = 0, in one or two copies; their previous pairs harvested first
      constexpr long K = rv_replay::kKp, C = rv_replay::kKpInit;
      static_assert(C <= K, "the initialised slots fit the ring");
      const long need = r->kp_n[p] + C - K;
      if (r->kp_done[p] < need) RV_H(kp_harvest(r, p, need));
      static const std::vector<unsigned long long> init = [] {
        std::vector<unsigned long long> v(2 * (size_t)C, 0ull);
        for (long i = 0; i < C; i++) v[2 * (size_t)i] = ~0ull;
        return v;
      }();
      const long s0 = r->kp_n[p] % K, first = std::min(C, K - s0);
      RV_H(hipMemcpyAsync(r->kp_ts[p] + 2 * s0, init.data(), 2 * sizeof(unsigned long long) * first,
                          hipMemcpyHostToDevice, xs));
      if (C > first)
        RV_H(hipMemcpyAsync(r->kp_ts[p], init.data(), 2 * sizeof(unsigned long long) * (C - first),
                            hipMemcpyHostToDevice, xs));
      r->kp_init[p] = r->kp_n[p] + C;
    }
    RV_H(hipEventRecord(r->kp_ev[p][2 * (size_t)(r->kp_n[p] % rv_replay::kKp)], xs));
    return RV_OK;
  }
  unsigned long long *ts(int p = 0) const {
    return on ? r->kp_ts[p] + 2 * (size_t)(r->kp_n[p] % rv_replay::kKp) : nullptr;
  }
  int close(hipStream_t xs, int p = 0) const {
    if (!on) return RV_OK;
    RV_H(hipEventRecord(r->kp_ev[p][2 * (size_t)(r->kp_n[p] % rv_replay::kKp) + 1], xs));
    r->kp_n[p]++;
    return RV_OK;
  }
};

// One inter frame's state and stages; rv_replay_frame below is their order.
// Everything a launch's asynchronous argument copy reads (f4h) lives here, to
// the end of rv_replay_frame.
struct FrameRun {
  rv_replay *const r;
  const Geo &g;
  const rv_replay_frame_info &fi;
  HostTrace &tr;
  const int lv;
  const rv_replay::Level &L;
  hipStream_t const st;
  const RvInput &cur;
  const RvSlot &S;
  CandGeo cg;
  const RvSlot *ref[RV_MAX_REFS];
  // the references' reconstructions, their inputs' half-res planes and (the
  // lookahead searches the original frames) their inputs
  rv_plane refs_y[RV_MAX_REFS], refs_h[RV_MAX_REFS], refs_o[RV_MAX_REFS];
  const int nr;        // jobs per reference
  const long ncoded;   // non-key frames before this one
  const int slot;      // the frame's slot of the per-frame rings
  uint32_t *ev_full, *ev_sub;
  ChainNext to_sub;
  const EpzsGeo eg;
  const LvPlace place;
  const bool tm;       // an instrumented frame: e is its event set
  hipEvent_t *e;
  const KProbe kp;     // F3 sub-pel (probe 0) and the F4 lists (probe 1), speed 10
  const float *imp = nullptr;
  const uint8_t *const act;  // speed 10: the superblocks a round re-evaluates
  const int nsingle, ntx_c;
  const int64_t nct;   // output blocks per chroma plane
  const bool f4_list;  // 12-bit keeps the full-grid launches
  // F4's arguments, also the list launches' in device memory: luma, chroma,
  // compound luma, compound chroma; la / ca: F6's commit of the winners
  RdoArgs f4h[4], la, ca;
  RdoArgs ll[kLevels], lc6[kLevels];  // the used levels' luma / chroma F4 arguments
  MvrefArgs ma;
  uint32_t q_first = 0;  // the run's first check: its list is the run's first round
  int mv_runs = 0;
  // The MV-stack rounds' budget, per run.  Termination: within
  // a tile a superblock's stacks read its left, top-left, top and top-right
  // neighbours, and its EPZS sets read fields of its left and top neighbours,
  // so its dependency depth is at most x + 2 y <= (tws - 1) + 2 (ths - 1).  A
  // superblock of depth d is settled (evaluated with its final inputs) after
  // evaluation round d + 1: its predecessors are settled after round d, so
  // check d + 1 gives its final inputs.  Hence every run ends by evaluation
  // round tws + 2 ths - 2 and the check after it lists nothing.
  const int budget;

  static LvPlace placement(const rv_replay *r) {
    if (!r->lvl) return LvPlace::kNone;
    if (!r->s6 && r->edge[1]) return LvPlace::kEdge;
    return r->exact ? LvPlace::kEarly : LvPlace::kRound0;
  }

  FrameRun(rv_replay *r_, const rv_replay_frame_info &fi_, HostTrace &tr_)
      : r(r_), g(r_->g), fi(fi_), tr(tr_), lv(fi_.level), L(r_->lv[fi_.level]), st(r_->stream),
        cur(r_->inputs[fi_.display % r_->inputs.size()]), S(r_->slots[fi_.display % kSlots]),
        cg(r_->cg), nr(r_->g.nsb), ncoded(r_->coded - 1),
        slot((int)((r_->coded - 1) % rv_replay::kRing)),
        to_sub{kChainFullToSub, r_->jobs_sub[fi_.level]},
        eg{g.tx0, g.ty0, g.tw, g.th, g.tws, g.ths, g.W, g.H, g.w_in_b, g.h_in_b},
        place(placement(r_)),
        tm(r_->timing_stride > 0 && (ncoded / r_->timing_block) % r_->timing_stride == 0),
        e(r_->evs[r_->timed % rv_replay::kRing]), kp{r_, tm && r_->kprobe && !r_->s6},
        act(r_->exact ? r_->mv_active : nullptr), nsingle(g.nsb * g.R * g.M), ntx_c(r_->ntx_c),
        nct((int64_t)g.nsb * g.C * r_->ntx_c), f4_list(g.bd != 12),
        budget(g.tws + 2 * g.ths - 2) {
    cg.comp = fi.compound ? kCompModes : 0;
    cg.stk = r->exact ? r->stk : nullptr;  // speed 10: rav1e's stacks (rv_mvref.hip)
    for (int k = 0; k < g.R; k++) {
      ref[k] = &r->slots[fi.ref_display[k] % kSlots];
      refs_y[k] = ref[k]->y;
      const RvInput &ri = r->inputs[fi.ref_display[k] % r->inputs.size()];
      refs_h[k] = ri.hres;
      refs_o[k] = ri.y;
    }
    ev_full = r->ds_evals + (size_t)slot * 2 * nr * g.R;
    ev_sub = ev_full + (size_t)nr * g.R;
    if (tm) r->timed++;
    memset(&ma, 0, sizeof(ma));
  }

  int ev(StageEv i, hipStream_t xs) const {
    if (tm) RV_H(hipEventRecord(e[i], xs));
    return RV_OK;
  }
  int ev(StageEv i) const { return ev(i, st); }
  Levels searched(int only) const { return Levels{r->lv_me, only}; }
  Levels used(int only = 0) const { return Levels{r->lv_used, only}; }
  int32_t *slot_cnt(uint32_t q) const { return r->rr.slot(q); }
  // check q's list (two halves: an incremental check reads the previous one)
  int32_t *mvl(uint32_t q) const { return r->mv_list + (size_t)(q & 1) * g.nsb; }

  // F0 .. FL: the frame's lookahead (lookahead_frame), or with an importance
  // window the engine's, run W frames ahead, and the window's importances
  int take_lookahead() {
    imp = r->imp;
    if (r->eng) {
      RV_R(la_encode_exchange(r, r->coded, st));
      RV_R(la_engine_take(r, r->coded, st, &imp));
      // F0 .. FL ran on the engine: empty stages here
      for (StageEv i : {kEvF0, kEvF1, kEvF2, kEvLaBegin, kEvLaEnd}) RV_R(ev(i));
    } else {
      LaRefs er;  // without a window: the encode's references only
      memset(&er, 0, sizeof(er));
      er.n = g.R;
      for (int k = 0; k < g.R; k++) er.disp[k] = fi.ref_display[k], er.order[k] = k;
      RV_R(lookahead_frame(r, r->rr, st, fi, er, ncoded, LaOut{r->coarse, r->half_l, r->look}, r->la_list,
                           true, &r->la_round_sum, &r->la_reeval, tm ? e : nullptr));
      r->la_frames++;
    }
    r->imp_last = imp;
    tr.take = HostTrace::now();
    return RV_OK;
  }

  // A used level's luma and chroma F4 arguments, from the superblocks' (a, c)
  void level_args(int l, RdoArgs a, RdoArgs c) {
    const rv_replay::PLevel &P = r->pl[l];
    CandGeo cgl = P.cg;
    cgl.comp = cg.comp;
    const int ns = P.n * g.R * g.M;
    a.p[0].levels = P.l_lev;
    a.p[0].out = P.l_out;
    a.p[0].q = L.qs[l][0];
    a.g = cgl;
    a.sub = P.sub;
    a.win = P.win;
    a.n_tx = ns;
    a.list = P.cand_list;
    a.count = P.cand_count;
    a.ntx_per_cand = 1;
    a.bsize = P.B;
    a.mb_w = a.mb_h = P.B;
    a.q_tx_index = P.txl * 16;  // DCT_DCT
    a.tx_size = P.txl;
    for (int q = 0; q < 2; q++) {
      c.p[q].levels = P.c_lev + (size_t)q * P.n * P.bc * P.bch;
      c.p[q].out = P.c_out + (size_t)q * P.n * g.C * 3;
      c.p[q].q = L.qs[l][1 + q];
    }
    c.g = cgl;
    c.sub = P.sub;
    c.win = P.win;
    c.n_tx = ns;
    c.list = P.cand_list;
    c.count = P.cand_count;
    c.ntx_per_cand = 1;
    c.bsize = P.B;
    c.mb_w = P.bc;
    c.mb_h = P.bch;
    c.sub_w = (P.bc < 8 ? P.bc : 8) >> g.xdec;   // sse_wxh's importance blocks
    c.sub_h = (P.bch < 8 ? P.bch : 8) >> g.ydec;
    c.q_tx_index = P.txc * 16;
    c.tx_size = P.txc;
    ll[l] = a;
    lc6[l] = c;
  }

  // Every RDO argument set of the frame, before any stage reads one: the
  // superblocks' F4 candidates -- luma (N = 64, cdef distortion) and both
  // chroma planes (N = 32, SSE) -- their compound sets (all pushed; distinct
  // MV pairs from the list), every used level's, and F6's commit
  void build_args() {
    memset(&la, 0, sizeof(la));
    la.p[0].org = cur.y;
    for (int k = 0; k < g.R; k++) la.p[0].ref[k] = ref[k]->y;
    la.p[0].dst = S.y;
    la.p[0].levels = r->l_lev;
    la.p[0].out = r->l_out;
    la.g = cg;
    la.sub = r->sub;
    la.win = r->win;
    la.imp = imp;
    la.w_in_b = g.w_in_b;
    la.h_in_b = g.h_in_b;
    la.w_imp = g.w_imp;
    la.n_tx = nsingle;
    la.list = r->cand_list;
    la.count = r->cand_count;
    la.ntx_per_cand = 1;
    la.bd = g.bd;
    la.bsize = kSb;
    la.mb_w = la.mb_h = kSb;
    la.sub_w = la.sub_h = 8;
    la.p[0].q = L.ql;
    la.q_tx_index = 4 * 16 + 0;  // TX_64X64, DCT_DCT
    la.tx_size = 4;
    la.qindex = L.qidx;
    ca = la;
    const rv_plane cur_c[2] = {cur.u, cur.v}, s_c[2] = {S.u, S.v};
    for (int p = 0; p < 2; p++) {
      ca.p[p].org = cur_c[p];
      for (int k = 0; k < g.R; k++) ca.p[p].ref[k] = p ? ref[k]->v : ref[k]->u;
      ca.p[p].dst = s_c[p];
      ca.p[p].levels = r->c_lev + (size_t)p * g.nsb * ntx_c * 1024;
      ca.p[p].out = r->c_out + (size_t)p * nct * 3;
      ca.p[p].q = p ? L.qv : L.qu;
    }
    ca.n_tx = nsingle * ntx_c;
    ca.ntx_per_cand = ntx_c;
    ca.mb_w = g.cw;
    ca.mb_h = g.ch;
    ca.xdec = g.xdec;
    ca.ydec = g.ydec;
    ca.sub_w = (g.cw < 8 ? g.cw : 8) >> g.xdec;
    ca.sub_h = (g.ch < 8 ? g.ch : 8) >> g.ydec;
    ca.q_tx_index = 3 * 16 + 0;  // TX_32X32, DCT_DCT
    ca.tx_size = 3;
    f4h[0] = f4h[2] = la;
    f4h[1] = f4h[3] = ca;
    f4h[2].list = f4h[3].list = r->cand_list + nsingle;
    f4h[2].count = f4h[3].count = r->cand_count + 1;
    f4h[2].cand_base = f4h[3].cand_base = 0;
    f4h[2].n_tx = g.nsb * cg.comp;
    f4h[3].n_tx = g.nsb * cg.comp * ntx_c;
    if (place != LvPlace::kNone)
      for (int l : used()) level_args(l, la, ca);
    la.commit = ca.commit = 1;
    la.list = ca.list = r->lvl ? r->pl[0].leaf : nullptr;  // with levels: the unsplit superblocks
    la.count = ca.count = r->lvl ? r->leaf_count : nullptr;
    la.n_tx = g.nsb;
    ca.n_tx = g.nsb * ntx_c;
    la.ntx_per_cand = 1;
  }

  // ---- the 32x32 .. 8x8 levels (speed 6: every block; speed 10: the frame-
  // edge rectangle), in pieces the schedule places (LvPlace); levels with no
  // leaf are skipped
  // motion_estimation of every block (sub-pel by SATD at speed 6,
  // use_satd_subpel, src/api/config.rs:429-431; SAD at speed 10), seeded with
  // the pmvs entry: a 32x32 its half-res quadrant search, a 16x16 / 8x8 its
  // 32x32's sub-pel winner
  int lv_me(hipStream_t es, int only = 0) {
    for (int l : searched(only)) {
      rv_replay::PLevel &P = r->pl[l];
      if (l == 1)
        seed_level_kernel<<<(P.n * g.R + 255) / 256, 256, 0, es>>>(
            P.jobs_full[lv], P.n, P.gw, g.R, r->half_l, g.nsb, 0, 0, r->ex0, r->ey0, g.tw);
      else
        seed_level_kernel<<<(P.n * g.R + 255) / 256, 256, 0, es>>>(
            P.jobs_full[lv], P.n, P.gw, g.R, r->pl[1].sub, r->pl[1].n, r->pl[1].gw, 1 << (l - 1),
            0, 0, 0);
      ChainNext to_s{kChainFullToSub, P.jobs_sub[lv]};
      RV_R(rv_diamond_search_multi(&cur.y, refs_y, g.R, P.jobs_full[lv], P.n, P.B, P.B, 0, 0, 0,
                                   g.bd, P.full, nullptr, &to_s, es));
      RV_R(rv_diamond_search_multi(&cur.y, refs_y, g.R, P.jobs_sub[lv], P.n, P.B, P.B, 1,
                                   r->s6 ? 1 : 0, 0, g.bd, P.sub, nullptr, nullptr, es));
    }
    return RV_OK;
  }
  // the candidate lists of every used level (single, or compound)
  void lv_lists(hipStream_t es, bool comp, int only = 0) {
    for (int l : used(only)) {
      rv_replay::PLevel &P = r->pl[l];
      const int ns = P.n * g.R * g.M;
      if (!comp) {
        cand_list_kernel<<<(ns + 255) / 256, 256, 0, es>>>(P.cg, P.sub, ns, P.cand_list,
                                                            P.cand_count);
      } else {
        CandGeo cgl = P.cg;
        cgl.comp = cg.comp;
        comp_list_kernel<<<(P.n * cg.comp + 255) / 256, 256, 0, es>>>(
            cgl, P.sub, ns, P.cand_list + ns, P.cand_count + 1);
      }
    }
  }
  // the single-reference candidates of every used level: luma (cdef
  // distortion) and chroma launches
  int lv_rdo(hipStream_t es, int only = 0) {
    for (int l : used(only))
      RV_R(rv_rdo_blocks2(ll[l], lc6[l], r->pl[l].B, r->pl[l].bc, g.hbd, es, 0));
    return RV_OK;
  }
  // the compound candidates of every used level (all pushed)
  int lv_rdo_comp(hipStream_t es, int only = 0) {
    for (int l : used(only)) {
      const rv_replay::PLevel &P = r->pl[l];
      RdoArgs a = ll[l], c = lc6[l];
      a.list = c.list = P.cand_list + P.n * g.R * g.M;
      a.count = c.count = P.cand_count + 1;
      a.cand_base = c.cand_base = 0;
      a.n_tx = c.n_tx = P.n * cg.comp;
      RV_R(rv_rdo_blocks2(a, c, P.B, P.bc, g.hbd, es, 1));
    }
    return RV_OK;
  }
  // every used level's winners and result words
  void lv_score(hipStream_t es, int only = 0) {
    for (int l : used(only)) {
      rv_replay::PLevel &P = r->pl[l];
      CandGeo cgl = P.cg;
      cgl.comp = cg.comp;
      score_level<<<(P.n + 63) / 64, 64, 0, es>>>(cgl, L.lambda, L.ds[1], L.ds[2], P.full, P.sub,
                                                  P.l_out, P.c_out, P.c_out + (size_t)P.n * g.C * 3,
                                                  P.win, r->words + P.woff, P.cand_count,
                                                  r->cand_evals + 2 * (slot * kLevels + l));
    }
  }
  // the leaves of every used level into the frame
  int lv_commit(hipStream_t es, int only = 0) {
    for (int l : used(only)) {
      const rv_replay::PLevel &P = r->pl[l];
      RdoArgs a = ll[l], c = lc6[l];
      a.commit = c.commit = 1;
      a.list = c.list = P.leaf;
      a.count = c.count = r->leaf_count + l;
      a.n_tx = c.n_tx = P.n;
      RV_R(rv_rdo_blocks2(a, c, P.B, P.bc, g.hbd, es, 2));
    }
    return RV_OK;
  }
  // the levels' candidates, F4 and winners, stage by stage (after lv_me)
  int lv_decide(hipStream_t es, int only = 0) {
    lv_lists(es, false, only);
    if (cg.comp) lv_lists(es, true, only);
    RV_R(lv_rdo(es, only));
    if (cg.comp) RV_R(lv_rdo_comp(es, only));
    lv_score(es, only);
    return RV_OK;
  }

  // kEarly: the levels' searches, candidates and winners on the main stream
  int levels_on_main() {
    RV_R(lv_me(st));
    return lv_decide(st);
  }
  // kEdge: the levels on the edge stream, forked here: the 32x32 searches
  // first (the smaller levels seed from them), then each level's candidates
  // and scores.  Without an edge stream: an empty span.
  int fork_edge_levels() {
    if (place != LvPlace::kEdge) {
      RV_R(ev(kEvEdgeBegin));
      return ev(kEvEdgeEnd);
    }
    hipStream_t e1 = r->edge[1];
    RV_H(hipEventRecord(r->ev_efork, st));
    for (int l = 1; l < kLevels; l++) RV_H(hipStreamWaitEvent(r->edge[l], r->ev_efork, 0));
    RV_R(ev(kEvEdgeBegin, e1));
    RV_R(lv_me(e1, 1));
    RV_H(hipEventRecord(r->ev_l1me, e1));
    for (int l = 1; l < kLevels; l++) {
      hipStream_t es = r->edge[l];
      if (l > 1 && r->lv_me[l]) {
        RV_H(hipStreamWaitEvent(es, r->ev_l1me, 0));
        RV_R(lv_me(es, l));
      }
      if (!r->lv_used[l]) continue;
      RV_R(lv_decide(es, l));
      RV_H(hipEventRecord(r->ev_ejoin[l], es));
    }
    for (int l : used())
      if (l > 1) RV_H(hipStreamWaitEvent(e1, r->ev_ejoin[l], 0));
    return ev(kEvEdgeEnd, e1);
  }
  // kEdge: the main stream waits for the levels' winners
  int join_edge_scores() {
    if (place != LvPlace::kEdge) return RV_OK;
    for (int l : used()) RV_H(hipStreamWaitEvent(st, r->ev_ejoin[l], 0));
    return RV_OK;
  }

  // The MV-stack checks' arguments (rv_mvref.hip), as the first check takes
  // them: EPZS sets from the coding-order field, guessed from the previous
  // decisions of this level and the lookahead's quadrants; the frame-edge
  // leaves are not read (they may be in flight)
  MvrefArgs mvref_args() const {
    MvrefArgs a;
    memset(&a, 0, sizeof(a));
    a.nsb = g.nsb;
    a.tw = g.tw;
    a.th = g.th;
    a.tx0 = g.tx0;
    a.ty0 = g.ty0;
    a.tws = g.tws;
    a.ths = g.ths;
    a.W = g.W;
    a.H = g.H;
    a.w_in_b = g.w_in_b;
    a.h_in_b = g.h_in_b;
    a.R = g.R;
    a.comp = cg.comp ? 1 : 0;
    for (int k = 0; k < g.R; k++) a.sign_bias |= (uint32_t)(fi.ref_display[k] > fi.display) << k;
    a.dec = r->dec_lv[lv];
    a.stk = r->stk;
    a.active = r->mv_active;
    a.jf = r->jobs_full[lv];
    a.js = r->jobs_sub[lv];
    a.init = 1;
    a.lvl = r->lvl ? 1 : 0;
    if (r->lvl)
      for (int l : used()) {
        a.lwin[l] = r->pl[l].win;
        a.lsub[l] = r->pl[l].sub;
        a.lcg[l] = r->pl[l].cg;
      }
    a.epzs = 1;
    a.eg = eg;
    a.jh = r->jobs_half[lv];
    a.coarse = r->coarse;
    a.hq = r->half_l;
    a.prev = r->slots[fi.ref_display[0] % kSlots].fmv;  // the LAST reference's frame_mvs
    a.edge_ok = 0;
    a.f3dirty = r->f3dirty;
    a.f2dirty = r->f2dirty;
    return a;
  }
  int check(uint32_t q) {
    ma.count = slot_cnt(q);
    ma.pub = r->rr.pub(q);
    ma.list = mvl(q);
    return rv_mvref_round(ma, st);
  }
  // speed 10: rav1e's MV stacks in coding-order rounds (rv_mvref.hip): round
  // 0 evaluates every superblock with the stacks of this level's previous
  // frame's decisions (a guess), each later round re-evaluates the
  // superblocks whose stacks changed, until none does.  The first check
  // marks every superblock (its count is not read).
  int check0() {
    ma = mvref_args();
    if (r->edge_tr) RV_R(join_edge_scores());  // the leaves the stacks read
    return check(r->rr.seq++);
  }

  // F2: build_half_res_pmvs of the encode (speed 10: the sets the check
  // stored; otherwise the lookahead's quadrants stand in) and the F3
  // full-pel predictors (otherwise zero + the coarse MV)
  int f2() {
    if (r->exact)
      return rv_diamond_search_multi(&cur.hres, refs_h, g.R, r->jobs_half[lv], nr * 4, 16, 16, 0, 0,
                                     0, g.bd, r->half, nullptr, nullptr, st);
    RV_H(hipMemcpyAsync(r->half, r->half_l, (size_t)nr * g.R * 4 * sizeof(rv_fs_result),
                        hipMemcpyDeviceToDevice, st));
    fill_preds_kernel<<<(nr * g.R + 255) / 256, 256, 0, st>>>(r->jobs_full[lv], r->src_full,
                                                              nr * g.R, r->coarse, r->half, 0);
    return RV_OK;
  }

  // Round 0: every superblock, full grids.  F3 full-res full-pel diamond ->
  // sub-pel predictor; sub-pel diamond (speed 10: SAD, no hp) -> NEWMV of
  // every superblock and reference; the candidates; F4; the argmin.  kRound0:
  // each stage is followed by the levels'.
  int round0() {
    const bool with_lv = place == LvPlace::kRound0;
    // the list launches' arguments into device memory
    if (f4_list) RV_R(rv_rdo_args_put(f4h, cg.comp ? 4 : 2, r->f4_args, st));
    RV_R(rv_diamond_search_multi(&cur.y, refs_y, g.R, r->jobs_full[lv], nr, 64, 64, 0, 0, 0, g.bd,
                                 r->full, ev_full, &to_sub, st, act));
    RV_R(ev(kEvF3Full));
    RV_R(kp.open(st));
    RV_R(rv_diamond_search_multi(&cur.y, refs_y, g.R, r->jobs_sub[lv], nr, 64, 64, 1,
                                 r->s6 ? 1 : 0, 0, g.bd, r->sub, ev_sub, nullptr, st, act, nullptr,
                                 nullptr, 1, nullptr, 0, kp.acc(0), kp.ts()));
    RV_R(kp.close(st));
    if (with_lv) RV_R(lv_me(st));
    // the valid candidates (a few microseconds; bracketed with F3 sub-pel;
    // the count was zeroed by the previous argmin or at creation)
    const CandKeys keys0{r->cand_key, (uint32_t)(r->coded + 1), 0};
    cand_list_kernel<<<(nsingle + 255) / 256, 256, 0, st>>>(cg, r->sub, nsingle, r->cand_list,
                                                            r->cand_count, act, keys0);
    if (with_lv) lv_lists(st, false);
    if (cg.comp) {  // the compound lists (after the single ones in the same arrays)
      comp_list_kernel<<<(g.nsb * cg.comp + 255) / 256, 256, 0, st>>>(
          cg, r->sub, nsingle, r->cand_list + nsingle, r->cand_count + 1, act, keys0);
      if (with_lv) lv_lists(st, true);
    }
    RV_R(ev(kEvF3Sub));
    // F4 every valid candidate, luma + both chroma planes in one fused launch
    if (f4_list) {
      RV_R(kp.open(st, 1));
      RV_R(rv_rdo_candidates_list(f4h, r->f4_args, 1, 0, g.hbd, st, 0, kp.acc(1), kp.ts(1)));
      RV_R(kp.close(st, 1));
    } else
      RV_R(rv_rdo_candidates(f4h[0], f4h[1], g.hbd, st));
    if (with_lv) RV_R(lv_rdo(st));
    RV_R(ev(kEvF4Single));
    if (cg.comp) {  // the compound candidates (all pushed), distinct MV pairs from the list
      if (f4_list) {
        RV_R(kp.open(st, 1));
        RV_R(rv_rdo_candidates_list(f4h + 2, r->f4_args + 2, 1, 1, g.hbd, st, 0, kp.acc(1), kp.ts(1)));
        RV_R(kp.close(st, 1));
      } else
        RV_R(rv_rdo_candidates(f4h[2], f4h[3], g.hbd, st, true));
      if (with_lv) RV_R(lv_rdo_comp(st));
    }
    RV_R(ev(kEvF4Comp));
    score_wave_kernel<<<(g.nsb + 3) / 4, 256, 0, st>>>(
        g, cg, L.lambda, L.ds[1], L.ds[2], r->sub, r->l_out, r->c_out, r->c_out + nct * 3, ntx_c,
        r->win, r->coarse, r->half, r->full, r->look, r->half_l, r->words, r->cand_count,
        r->tail + 2, r->cand_evals + 2 * slot * kLevels, r->leaf_count, nullptr, nullptr,
        r->exact ? r->dec_lv[lv] : nullptr, 0);
    return RV_OK;
  }

  // A later round: the same stages over the superblocks check q listed
  // (r->mv_list, its count in the ring), each launch a fixed pool of
  // workgroups that loops over the device count -- a round of a few dozen
  // superblocks costs their latency, not a full grid of early exits.
  // the first round of a run lists most superblocks (check 1 after round 0:
  // 70-80 % at 2160p): its searches take full grids, later ones the pool
  int round_of(uint32_t q) {
    const int32_t *acnt = slot_cnt(q);
    int lg = q == q_first ? nr * g.R : 0;
    // A later round's grids from the last count the host read (a check one
    // or two rounds back): twice that many superblocks, so the launches
    // carry the live work and few empty workgroups (a round's fixed pools
    // put ~12 k waves through the dispatcher for a few dozen superblocks).
    // A list longer than the hint loops over the grid, so the hint only
    // sizes, never decides.
    const int hint = q == q_first ? -1 : r->rr.last_count;
    const int hsb = hint >= 0 ? std::max(2 * hint, 16) : 0;
    int f4_grid = 0;
    if (hsb) {
      lg = std::min(hsb * g.R, 512);
      f4_grid = std::min(6 * hsb, 1024);
    }
    // F2 and F3 full-pel of the listed superblocks in one launch (the check's
    // sets came from the state before this round, so they are independent;
    // only the jobs whose set or pmv changed run), with F3's sub-pel search
    // fused into it: each F3 workgroup runs its job's sub-pel search right
    // after the full-pel one.  The probe brackets the launch (its sub-pel
    // candidates, its span).  (The rounds are speed 10's: SAD, no half-pel.)
    RV_R(kp.open(st));
    RV_R(rv_diamond_f2_f3(&cur.hres, refs_h, r->jobs_half[lv], r->half, ma.f2dirty, &cur.y,
                          refs_y, r->jobs_full[lv], r->full, ma.f3dirty, &to_sub, g.R, nr, g.bd,
                          mvl(q), acnt, lg, st, r->jobs_sub[lv], r->sub, kp.acc(0), kp.ts()));
    RV_R(kp.close(st));
    // the pools of the small per-round kernels: kRoundGrid unless the hint sizes them
    const int rg = hsb ? std::min(kRoundGrid, std::max((14 * hsb + 255) / 256, (hsb + 3) / 4))
                       : kRoundGrid;
    round_lists_kernel<<<rg, 256, 0, st>>>(
        cg, r->sub, nsingle, r->cand_list, r->cand_count, mvl(q), acnt,
        CandKeys{r->cand_key, (uint32_t)(r->coded + 1), 1});
    // F4: a pool of workgroups over the live list entries (rdo_quad_list_kernel),
    // on a compound frame the single and compound candidates in one launch;
    // 12-bit: full grids whose workgroups past the device counts exit at once
    if (f4_list) {
      RV_R(kp.open(st, 1));
      RV_R(rv_rdo_candidates_list(f4h, r->f4_args, cg.comp ? 2 : 1, 0, g.hbd, st, f4_grid,
                                  kp.acc(1), kp.ts(1)));
      RV_R(kp.close(st, 1));
    } else {
      RV_R(rv_rdo_candidates(f4h[0], f4h[1], g.hbd, st));
      if (cg.comp) RV_R(rv_rdo_candidates(f4h[2], f4h[3], g.hbd, st, true));
    }
    score_wave_kernel<<<rg, 256, 0, st>>>(
        g, cg, L.lambda, L.ds[1], L.ds[2], r->sub, r->l_out, r->c_out, r->c_out + nct * 3, ntx_c,
        r->win, r->coarse, r->half, r->full, r->look, r->half_l, r->words, r->cand_count, nullptr,
        nullptr, nullptr, mvl(q), acnt, r->dec_lv[lv], 1);
    return RV_OK;
  }

  // A run of the MV-stack rounds after the first: a check recomputes every
  // superblock's stacks and F2 / F3 EPZS sets from the decisions and results
  // so far and lists the superblocks where one changed; the round re-runs
  // their F2, F3, candidates, F4 and argmin.  *changed: some round evaluated.
  int mv_rounds_run(const uint8_t *iwas, bool *changed) {
    mv_runs++;
    q_first = r->rr.seq;  // run_rounds' first check
    ma.init = 0;
    ma.iwas = iwas;
    return run_rounds(
        r->rr, st, budget, [this](uint32_t q) { return check(q); },
        [this](uint32_t q) { return round_of(q); }, &r->mv_round_sum, &r->mv_reeval, changed,
        "mvref", ncoded, lv);
  }
  // The first run: from here on the checks read the frame-edge leaves (the
  // EPZS field of the edge superblocks) and the encode's own F2 results
  int rounds() {
    RV_R(join_edge_scores());
    ma.hq = r->half;
    ma.edge_ok = 1;
    tr.r0 = HostTrace::now();
    RV_R(mv_rounds_run(nullptr, nullptr));
    tr.mv = HostTrace::now();
    return RV_OK;
  }

  PartArgs part_args() const {
    PartArgs pa;
    memset(&pa, 0, sizeof(pa));
    for (int l = 0; l < kLevels; l++) {
      const rv_replay::PLevel &P = r->pl[l];
      pa.win[l] = l ? P.win : r->win;
      pa.gw[l] = P.gw;
      pa.x0[l] = (g.tx0 + (l ? r->ex0 : 0)) * kSb;
      pa.y0[l] = (g.ty0 + (l ? r->ey0 : 0)) * kSb;
      pa.leaf[l] = P.leaf;
    }
    pa.ex0 = r->ex0;
    pa.ey0 = r->ey0;
    pa.ew = r->ew;
    pa.eh = r->eh;
    pa.forced = !r->s6;
    pa.leaf_count = r->leaf_count;
    pa.words = r->words + r->wpart;
    return pa;
  }
  // the levels' winners are in (kRound0: scored here), then the partition
  int partition() {
    if (place == LvPlace::kNone) return RV_OK;
    RV_R(join_edge_scores());
    if (place == LvPlace::kRound0) lv_score(st);
    partition_kernel<<<(g.nsb + 63) / 64, 64, 0, st>>>(g, part_args());
    return RV_OK;
  }

  // F6 commit the winners into the frame: the levels' leaves (kEdge: on the
  // edge stream, beside the superblocks' commit; the main stream then joins it)
  int commit() {
    const bool edge = place == LvPlace::kEdge;
    if (edge) {
      RV_H(hipEventRecord(r->ev_epart, st));
      for (int l : used()) {
        RV_H(hipStreamWaitEvent(r->edge[l], r->ev_epart, 0));
        RV_R(lv_commit(r->edge[l], l));
        RV_H(hipEventRecord(r->ev_ecommit[l], r->edge[l]));
      }
    }
    RV_R(rv_rdo_candidates(la, ca, g.hbd, st));
    if (edge) {
      for (int l : used()) RV_H(hipStreamWaitEvent(st, r->ev_ecommit[l], 0));
    } else if (place != LvPlace::kNone) {
      RV_R(lv_commit(st));
    }
    return RV_OK;
  }

  // F6b intra-mode screening + intra RDO of the non-skip superblocks.  An
  // intra winner is no MV source (add_ref_mv_candidate skips intra blocks):
  // the superblocks whose stacks it changes are re-decided, the frame
  // re-committed and the intra pass re-run, until the stacks hold (the joint
  // fixed point of the tile's coding order).
  // Bound: each pass settles at least the next superblock of every tile's
  // raster order (its predecessors' decisions, intra flags and
  // reconstruction are final, so its stacks, inter winner and intra
  // decision are too), so tws * ths passes always suffice.
  int intra_fixed_point() {
    int irounds = 0;
    if (r->intra) RV_R(intra_pass(r, la, ca, cur, S, L, slot, &irounds));
    tr.intra = HostTrace::now();
    for (int pass = 0; r->exact && r->intra; pass++) {
      if (pass > g.tws * g.ths)
        return rv_set_error(RV_EHIP, "rv_replay_frame: the MV / intra passes did not settle "
                                     "(internal error)");
      // no screened superblock (no intra round): no superblock is intra, the
      // stacks are the ones the MV rounds settled -- the check would list
      // nothing (only after the first pass: later ones follow a run whose
      // stacks saw intra blocks)
      if (pass == 0 && irounds == 0) break;
      bool changed = false;
      RV_R(mv_rounds_run(r->i_was, &changed));
      if (!changed) break;
      RV_R(rv_rdo_candidates(la, ca, g.hbd, st));  // F6 again: every inter winner
      RV_R(intra_begin(r));
      RV_R(intra_pass(r, la, ca, cur, S, L, slot, &irounds));
    }
    return RV_OK;
  }

  // speed 10: the rounds' counters, and the encode's field becomes the
  // frame's frame_mvs (the group's part; the other groups' arrive with the
  // exchange)
  int frame_mvs() {
    r->mv_round_sum++;  // round 0
    r->mv_run_sum += mv_runs;
    r->mv_frames++;
    ma.iwas = r->intra ? r->i_was : nullptr;
    return rv_mvref_field(ma, S.fmv, st);
  }

  // F5: the 8x8 importance SATD against reference 0's original frame at the
  // lookahead MVs (FL's output; the sum was zeroed by round 0's argmin)
  int f5_importance() {
    const unsigned nb = (unsigned)((r->n_imp + 255) / 256);
    if (g.hbd)
      importance_kernel<uint16_t><<<nb, 256, 0, st>>>(g, cur.y, refs_o[0], r->look, r->imp_bx,
                                                      r->imp_by, r->tail + 2);
    else
      importance_kernel<uint8_t><<<nb, 256, 0, st>>>(g, cur.y, refs_o[0], r->look, r->imp_bx,
                                                     r->imp_by, r->tail + 2);
    return RV_OK;
  }

  // The block map of the committed blocks (the deblocking filter and F8 read it)
  void block_map() {
    if (!r->lvl) {
      block_map_kernel<<<(g.nsb * 16 + 255) / 256, 256, 0, st>>>(
          nullptr, nullptr, g.nsb, g.tw, g.tx0, g.ty0, 0, r->win, r->mi_lg, r->mi_skip,
          r->mi_stride, r->mi_cols, r->mi_rows);
      return;
    }
    for (int l = 0; l < kLevels; l++) {
      const rv_replay::PLevel &P = r->pl[l];
      const int n4 = 16 >> l;
      block_map_kernel<<<(P.n * n4 + 255) / 256, 256, 0, st>>>(
          P.leaf, r->leaf_count + l, P.n, P.gw, l ? P.cg.tx0 : g.tx0, l ? P.cg.ty0 : g.ty0, l,
          l ? P.win : r->win, r->mi_lg, r->mi_skip, r->mi_stride, r->mi_cols, r->mi_rows);
    }
  }

  EcFrameArgs ec_frame_args() const {
    EcFrameArgs ea;
    ea.tx0 = g.tx0;
    ea.ty0 = g.ty0;
    ea.tw = g.tw;
    ea.th = g.th;
    ea.tws = g.tws;
    ea.ths = g.ths;
    ea.xdec = g.xdec;
    ea.ydec = g.ydec;
    ea.ntx_c = r->ntx_c;
    ea.nsb = g.nsb;
    ea.mi_lg = r->mi_lg;
    ea.mi_skip = r->mi_skip;
    ea.mi_stride = r->mi_stride;
    ea.mi_cols = r->mi_cols;
    ea.mi_rows = r->mi_rows;
    ea.lv[0].l_lev = r->l_lev;
    ea.lv[0].c_lev = r->c_lev;
    ea.lv[0].n = g.nsb;
    ea.lv[0].gw = g.tw;
    ea.lv[0].x0 = g.tx0;
    ea.lv[0].y0 = g.ty0;
    for (int l = 1; r->lvl && l < kLevels; l++) {
      const rv_replay::PLevel &P = r->pl[l];
      ea.lv[l].l_lev = P.l_lev;
      ea.lv[l].c_lev = P.c_lev;
      ea.lv[l].n = P.n;
      ea.lv[l].gw = P.gw;
      ea.lv[l].x0 = P.cg.tx0;
      ea.lv[l].y0 = P.cg.ty0;
      ea.lv[l].B = P.B;
      ea.lv[l].bc = P.bc;
    }
    ea.words = r->words;
    ea.words_per_sb = kWordsPerRef * g.R + 4;
    ea.win_off = kWordsPerRef * g.R;
    return ea;
  }
  // F8 (RV_REPLAY_ENTROPY): the committed transform blocks' symbols, in
  // coding order, into a host-mapped ring slot (once the host thread is done
  // with it); the host thread range-codes them beside the next frames
  int f8_tokens() {
    EcHost *eh = r->ech;
    const int es = (int)(r->ec_frames & 1);
    {
      std::unique_lock<std::mutex> lk(eh->mu);
      eh->cv.wait(lk, [&] { return !eh->busy[es]; });
      eh->busy[es] = true;
    }
    EcFrameBufs b = r->ecb;
    RV_H(hipHostGetDevicePointer((void **)&b.tokens, eh->tok_h[es], 0));
    RV_H(hipHostGetDevicePointer((void **)&b.stat, eh->stat_h[es], 0));
    RV_R(ev(kEvF8Begin));
    RV_R(ec_frame_tokens(ec_frame_args(), b, st));
    RV_R(ev(kEvF8End));
    RV_H(hipEventRecord(eh->ev[es], st));
    const int q = r->lv[lv].qidx;
    {
      std::lock_guard<std::mutex> lk(eh->mu);
      eh->q.push_back({es, lv, q <= 20 ? 0 : q <= 60 ? 1 : q <= 120 ? 2 : 3});
      eh->queued++;
    }
    eh->cv.notify_all();
    r->ec_frames++;
    return RV_OK;
  }

  // F7: the reconstruction becomes a reference.  One group: the loop filters
  // and the padding.  Tile groups: this group's restoration units, then its
  // region packed; over RCCL the all-gather and the import follow here
  // (otherwise the caller moves the buffers and calls rv_replay_import).
  int finish_slot() {
    if (!groups_active(r)) return filter_slot(r, S, cur, lv);
    XRect xr[9];
    int nx;
    if (r->lrf) {  // this group's units travel with its reconstruction
      LrfGeo lg;
      RV_R(lrf_geometry(g.W, g.H, g.xdec, g.ydec, g.bd, r->lv[lv].qidx, g.tws, g.ths, &lg));
      RV_R(lrf_decide_slot(r, S, cur, lv, lg, r->grects + 4 * r->my_group));
    }
    group_rects(r, r->my_group, xr, &nx);
    RV_R(xcopy(r, S, xr, nx, 0, r->xsend));
    if (!r->comm) return RV_OK;
#if RV_HAVE_RCCL
    if (ncclAllGather(r->xsend, r->xrecv, r->xbytes, ncclUint8, (ncclComm_t)r->comm, st) !=
        ncclSuccess)
      return rv_set_error(RV_EHIP, "rv_replay_frame: ncclAllGather");
    return rv_replay_import(r);
#else
    return rv_set_error(RV_EINVAL, "rv_replay_frame: built without RCCL");
#endif
  }
};

// The key frame: its input is its reconstruction (intra coding is out of
// scope); the pyramid of its input for the searches that reference it
int key_frame(rv_replay *r) {
  const Geo &g = r->g;
  hipStream_t st = r->stream;
  const RvInput &in = r->inputs[0];
  const RvSlot &s = r->slots[0];
  RV_H(hipMemcpyAsync(s.y.data, in.y.data, plane_bytes(in.y), hipMemcpyDeviceToDevice, st));
  RV_H(hipMemcpyAsync(s.u.data, in.u.data, plane_bytes(in.u), hipMemcpyDeviceToDevice, st));
  RV_H(hipMemcpyAsync(s.v.data, in.v.data, plane_bytes(in.v), hipMemcpyDeviceToDevice, st));
  if (!r->eng) {  // (the lookahead engine computes every pyramid itself)
    RV_R(rv_plane_pyramid(&in.y, &in.hres, &in.qres, st));
    if (r->sea) RV_R(rv_plane_box_sums(&in.qres, in.qres_box, st));
  }
  // an intra frame saves no motion: its frame_mvs stay zero
  RV_H(hipMemsetAsync(s.fmv, 0, (size_t)(g.w_in_b / 2) * (g.h_in_b / 2) * g.R * sizeof(rv_mv), st));
  return RV_OK;
}

}  // namespace

// One coded frame, as the order of its stages (FrameRun above; the stages'
// events: StageEv).  kEdge forks the frame-edge levels beside everything up
// to the partition; the MV-stack rounds and the intra fixed point are host
// loops over the round ring.
extern "C" int rv_replay_frame(rv_replay *r, rv_replay_frame_info *info) {
  if (!r) return rv_set_error(RV_EINVAL, "rv_replay_frame: null");
  rv_replay_frame_info fi;
  frame_info(r->coded, r->g.R, &fi);
  if (fi.is_key) {
    RV_R(key_frame(r));
    r->coded++;
    r->last = fi;
    if (info) *info = fi;
    RV_H(hipGetLastError());
    return RV_OK;
  }
  if (!r->lv[0].set || !r->lv[1].set || !r->lv[2].set)
    return rv_set_error(RV_EINVAL, "rv_replay_frame: level params not set");
  HostTrace tr;
  RV_R(ensure_jobs(r));
  FrameRun f(r, fi, tr);
  RV_R(f.ev(kEvStart));
  RV_R(f.take_lookahead());
  RV_R(f.ev(kEvFL));
  SideJoin side_join{r, r->edge[1] != nullptr};
  f.build_args();
  RV_R(f.fork_edge_levels());
  if (f.place == LvPlace::kEarly) RV_R(f.levels_on_main());
  if (r->exact) RV_R(f.check0());  // the stacks and EPZS sets round 0 runs with
  RV_R(f.f2());
  RV_R(f.round0());                // F3, candidates, F4, argmin of every superblock
  if (r->exact) RV_R(f.rounds());  // ... of those whose stacks changed, until none does
  RV_R(f.partition());
  if (r->intra) RV_R(intra_begin(r));  // its count reaches the host while F6 runs
  RV_R(f.ev(kEvArgmin));
  RV_R(f.commit());
  side_join.armed = false;  // the edge streams have joined the main one
  RV_R(f.ev(kEvCommit));
  RV_R(f.intra_fixed_point());
  if (r->exact) RV_R(f.frame_mvs());
  RV_R(f.ev(kEvIntra));
  RV_R(f.f5_importance());
  RV_R(f.ev(kEvF5));
  if (r->deblock || r->entropy) f.block_map();
  if (r->entropy) RV_R(f.f8_tokens());
  tr.report(r->coded, fi.level);
  r->coded++;
  r->last = fi;
  RV_R(f.finish_slot());
  RV_R(f.ev(kEvF7));
  if (r->eng) RV_R(la_engine_release(r, r->coded - 1, f.st));  // its lookahead entry is free
  if (info) *info = fi;
  RV_H(hipGetLastError());
  return RV_OK;
}

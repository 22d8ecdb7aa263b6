// rv_cfl.hip -- chroma from luma: luma_ac (src/encoder.rs:1714-1755), the
// CfL predictor (pred_cfl / _128 / _left / _top / _inner, src/predict.rs:
// 836-892, with predict_intra's alpha == 0 -> DC_PRED remap, :223) and the
// alpha search rdo_cfl_alpha (src/rdo.rs:1261-1336).
//
// A chroma block of W x H pixels is spread over a group of G = min(64, W*H)
// lanes, NP = W*H / G pixels per lane in runs of min(NP, 4) consecutive
// pixels of a row, so the luma rows come in with one vector load per run.
// Blocks below 64 pixels (4x4, 4x8, 8x4) share a wavefront, 64 / G jobs in
// aligned lane groups like intra_dc<G>.  The ac block, the source pixels and
// the 33 per-alpha partial sums live in registers (statically indexed: no
// scratch); sums are reduced across lanes with DPP adds and lane reads, so
// the totals of a whole-wave block and the scan over them are scalar.
//
// The search runs one wavefront per job (or lane group per job) over U and
// then V, so the ac block is computed once and shared by both planes
// without leaving the registers.  Only alpha[n][2] (and cost[n][2]) are
// written: the reference leaves the last tried prediction in `rec` as a
// side effect that encode_block_post_cdef overwrites at once; this kernel
// leaves `rec` untouched.
#include "rv_intra.h"

namespace rv {

constexpr uint8_t kCflTxW[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kCflTxH[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
// BlockSize 0 .. 9 (BLOCK_4X4 .. BLOCK_32X32): the sizes cfl_allowed() admits
// (src/partition.rs:174-177)
constexpr uint8_t kCflBsW[10] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32};
constexpr uint8_t kCflBsH[10] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32};

// Geometry of one call: the chroma-plane block (subsampled_size, src/
// partition.rs:245-286) and the luma origin's sub8x8_offset (:303-312).
struct CflGeom {
  int w, h;      // chroma block
  int lw, sh;    // log2 w, log2 (w * h)
  int xdec, ydec;
  int offx, offy;  // luma origin offset in pixels (0 or -4)
};

struct CflPlanes {
  rv_plane luma, rec_u, rec_v, src_u, src_v;
};

// Position of the run `k` of lane `gl`: pixel index, row, column.
template <int G, int NP>
__device__ __forceinline__ void cfl_run_pos(const CflGeom &g, int k, int gl, int &r, int &c) {
  constexpr int CW = NP < 4 ? NP : 4;
  const int i = (k * G + gl) * CW;
  r = i >> g.lw;
  c = i & (g.w - 1);
}

// R consecutive pixels (R = 1, 2, 4, 8) starting at a multiple of min(R, 4)
// pixels from the plane's row start, as i32: one 2 / 4 / 8-byte load per (up
// to) four pixels.  The entry points require xorigin and stride to be
// multiples of 4 pixels and the allocation 16-byte aligned, and job positions
// are multiples of 4, so every such unit is naturally aligned.
template <typename Px, int R>
__device__ __forceinline__ void cfl_load_run(const Px *p, int32_t (&o)[R]) {
  if constexpr (R == 1) {
    o[0] = p[0];
  } else if constexpr (sizeof(Px) == 1) {
    if constexpr (R == 2) {
      const uint32_t v = *reinterpret_cast<const uint16_t *>(p);
      o[0] = v & 255;
      o[1] = v >> 8;
    } else {
#pragma unroll
      for (int u = 0; u < R / 4; u++) {
        const uint32_t v = reinterpret_cast<const uint32_t *>(p)[u];
        o[4 * u] = v & 255;
        o[4 * u + 1] = (v >> 8) & 255;
        o[4 * u + 2] = (v >> 16) & 255;
        o[4 * u + 3] = v >> 24;
      }
    }
  } else {
    if constexpr (R == 2) {
      const uint32_t v = *reinterpret_cast<const uint32_t *>(p);
      o[0] = v & 0xffff;
      o[1] = v >> 16;
    } else {
#pragma unroll
      for (int u = 0; u < R / 4; u++) {
        const uint2 v = reinterpret_cast<const uint2 *>(p)[u];
        o[4 * u] = v.x & 0xffff;
        o[4 * u + 1] = v.x >> 16;
        o[4 * u + 2] = v.y & 0xffff;
        o[4 * u + 3] = v.y >> 16;
      }
    }
  }
}

// luma_ac (src/encoder.rs:1714-1755) of the block whose luma origin (after
// the sub-8x8 offset) is (lx, ly): this lane's NP samples, average removed.
template <typename Px, int G, int NP>
__device__ __forceinline__ void cfl_luma_ac(const rv_plane &luma, const CflGeom &g, int lx, int ly,
                                            int gl, int32_t (&ac)[NP]) {
  constexpr int CW = NP < 4 ? NP : 4;
  int32_t sum = 0;
#pragma unroll
  for (int k = 0; k < NP / CW; k++) {
    int r, c;
    cfl_run_pos<G, NP>(g, k, gl, r, c);
    const Px *p0 = plane_ptr<Px>(luma, lx + (c << g.xdec), ly + (r << g.ydec));
    if (g.xdec == 0) {  // 4:4:4
      int32_t v[CW];
      cfl_load_run<Px, CW>(p0, v);
#pragma unroll
      for (int j = 0; j < CW; j++) ac[k * CW + j] = v[j] << 3;
    } else {
      int32_t v[2 * CW];
      cfl_load_run<Px, 2 * CW>(p0, v);
#pragma unroll
      for (int j = 0; j < CW; j++) ac[k * CW + j] = v[2 * j] + v[2 * j + 1];
      if (g.ydec != 0) {  // 4:2:0
        cfl_load_run<Px, 2 * CW>(p0 + luma.stride, v);
#pragma unroll
        for (int j = 0; j < CW; j++)
          ac[k * CW + j] = (ac[k * CW + j] + v[2 * j] + v[2 * j + 1]) << 1;
      } else {  // 4:2:2
#pragma unroll
        for (int j = 0; j < CW; j++) ac[k * CW + j] <<= 2;
      }
    }
#pragma unroll
    for (int j = 0; j < CW; j++) sum += ac[k * CW + j];
  }
  sum = group_sum<G>(sum);  // <= 1024 * 32760
  const int32_t avg = (sum + (1 << (g.sh - 1))) >> g.sh;
#pragma unroll
  for (int j = 0; j < NP; j++) ac[j] -= avg;
}

// The sum of v over the 16 lanes of this lane's row, in every lane of the
// row: four DPP adds (xor 1, xor 2, mirror within 8, mirror within 16), no
// LDS crossbar traffic.
__device__ __forceinline__ uint32_t row_sum16(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, true);  // row_half_mirror
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xf, 0xf, true);  // row_mirror
  return v;
}

// A group's total of per-lane partials (each <= 16 * 4095^2, so a row's sum
// fits u32): G = 16 the row; G = 32 two rows; G = 64 the four rows read
// into scalars, so the total -- and the scan over the totals -- is uniform.
template <int G, typename Acc>
__device__ __forceinline__ Acc cfl_group_total(uint32_t v) {
  v = row_sum16(v);
  if constexpr (G == 16) {
    return v;
  } else if constexpr (G == 32) {
    return (Acc)v + (Acc)__shfl_xor(v, 16, RV_WAVE);
  } else {
    return (Acc)(uint32_t)__builtin_amdgcn_readlane((int)v, 0) +
           (Acc)(uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (Acc)(uint32_t)__builtin_amdgcn_readlane((int)v, 32) +
           (Acc)(uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  }
}

// bo.plane_offset / Area::BlockStartingAt (src/context.rs, src/tiling/
// plane_region.rs): (bo >> dec) << 2 of the luma pixel position 4 * bo
__device__ __forceinline__ int cfl_chroma_pos(int luma_px, int dec) {
  return ((luma_px >> 2) >> dec) << 2;
}

template <typename Px, int G, int NP>
__global__ __launch_bounds__(64) void cfl_luma_ac_kernel(rv_plane luma, const rv_cfl_job *jobs,
                                                          int n, CflGeom g, int16_t *out) {
  constexpr int CW = NP < 4 ? NP : 4;
  const int lane = threadIdx.x, u = lane / G, gl = lane % G;
  int job = blockIdx.x * (64 / G) + u;
  const bool live = job < n;
  job = live ? job : n - 1;
  const rv_cfl_job j = jobs[job];
  int32_t ac[NP];
  cfl_luma_ac<Px, G, NP>(luma, g, j.x + g.offx, j.y + g.offy, gl, ac);
  if (!live) return;
  int16_t *o = out + ((int64_t)job << g.sh);
#pragma unroll
  for (int k = 0; k < NP / CW; k++) {
    int16_t v[CW];
#pragma unroll
    for (int q = 0; q < CW; q++) v[q] = (int16_t)ac[k * CW + q];
    __builtin_memcpy(o + (k * G + gl) * CW, v, sizeof(v));  // row stride W: index = pixel index
  }
}

// rdo_cfl_alpha (src/rdo.rs:1261-1336).  Acc: the type of a block's total
// SSE (u32 where w * h * (2^bd - 1)^2 < 2^32, else u64); a lane's partial
// (<= 16 * 4095^2) always fits u32.
template <typename Px, int G, int NP, typename Acc>
__global__ __launch_bounds__(64) void cfl_search_kernel(CflPlanes P, const rv_cfl_job *jobs, int n,
                                                         CflGeom g, int bd, int16_t *alpha_out,
                                                         uint64_t *cost_out) {
  constexpr int CW = NP < 4 ? NP : 4;
  __shared__ int32_t edges[64 / G][kIntraEdge + 3];
  const int lane = threadIdx.x, u = lane / G, gl = lane % G;
  int job = blockIdx.x * (64 / G) + u;
  const bool live = job < n;
  job = live ? job : n - 1;
  const rv_cfl_job j = jobs[job];
  const int variant = j.variant & 3;
  int32_t ac[NP];
  cfl_luma_ac<Px, G, NP>(P.luma, g, j.x + g.offx, j.y + g.offy, gl, ac);

  const int cx = cfl_chroma_pos(j.x, g.xdec), cy = cfl_chroma_pos(j.y, g.ydec);
  const int maxv = (1 << bd) - 1;
  int32_t *e = edges[u];
#pragma unroll 1
  for (int p = 0; p < 2; p++) {
    const rv_plane &rec = p ? P.rec_v : P.rec_u;
    const rv_plane &src = p ? P.src_v : P.src_u;
    // get_intra_edges(.., Some(UV_CFL_PRED)) (src/partition.rs:542-595): the
    // left column when x != 0, the above row when y != 0 -- all a DC reads
    if (variant & 1)
      for (int k = gl; k < g.h; k += G) e[128 - g.h + k] = *plane_ptr<Px>(rec, cx - 1, cy + g.h - 1 - k);
    if (variant & 2)
      for (int k = gl; k < g.w; k += G) e[129 + k] = *plane_ptr<Px>(rec, cx + k, cy - 1);
    wave_sync();
    const int32_t dc = intra_dc<G>(e, variant, g.w, g.h, bd, gl);
    wave_sync();  // the next plane rewrites e

    int32_t s[NP];
#pragma unroll
    for (int k = 0; k < NP / CW; k++) {
      int r, c;
      cfl_run_pos<G, NP>(g, k, gl, r, c);
      int32_t v[CW];
      cfl_load_run<Px, CW>(plane_ptr<Px>(src, cx + c, cy + r), v);
#pragma unroll
      for (int q = 0; q < CW; q++) s[k * CW + q] = v[q];
    }

    // acc[16 + a]: this lane's sse_wxh partial (bias 1, src/rdo.rs:286-335)
    // at alpha a.  +a and -a share |a * ac| (get_scaled_luma_q0).
    uint32_t acc[33];
#pragma unroll
    for (int a = 0; a < 33; a++) acc[a] = 0;
#pragma unroll
    for (int q = 0; q < NP; q++) {
      const int32_t mag = ac[q] < 0 ? -ac[q] : ac[q];
      const bool neg = ac[q] < 0;
      const int32_t d0 = s[q] - dc;  // alpha 0: DC_PRED
      acc[16] += (uint32_t)__mul24(d0, d0);
      int32_t m = 32;
#pragma unroll
      for (int a = 1; a <= 16; a++) {
        m += mag;
        const int32_t sc = neg ? -(m >> 6) : (m >> 6);
        const int32_t dp = s[q] - clamp_med3(dc + sc, 0, maxv);
        const int32_t dm = s[q] - clamp_med3(dc - sc, 0, maxv);
        acc[16 + a] += (uint32_t)__mul24(dp, dp);
        acc[16 - a] += (uint32_t)__mul24(dm, dm);
      }
      // one pixel at a time: interleaving the unrolled pixels only multiplies
      // the live temporaries (spills at 16 pixels per lane)
      __builtin_amdgcn_sched_barrier(0);
    }
    Acc cost[33];
#pragma unroll
    for (int a = 0; a < 33; a++) cost[a] = cfl_group_total<G, Acc>(acc[a]);

    // the reference's scan (src/rdo.rs:1311-1327), uniform over the group
    Acc best = cost[16];
    int32_t best_a = 0, count = 2;
    bool done = false;
#pragma unroll
    for (int a = 1; a <= 16; a++) {
      if (!done) {
        if (cost[16 + a] < best) {
          best = cost[16 + a];
          best_a = a;
          count += 2;
        }
        if (cost[16 - a] < best) {
          best = cost[16 - a];
          best_a = -a;
          count += 2;
        }
        done = count < a;
      }
    }
    if (live && gl == 0) {
      alpha_out[job * 2 + p] = (int16_t)best_a;
      if (cost_out) cost_out[job * 2 + p] = (uint64_t)best;
    }
  }
}

// predict_intra(UV_CFL_PRED) (src/predict.rs:202-241, 836-892): DC of the
// job's variant from the edge buffer, plus the scaled ac.  One wavefront per
// block as intra_kernel.
template <typename Px>
__global__ __launch_bounds__(64) void cfl_pred_kernel(rv_plane dst, const rv_intra_job *jobs,
                                                       const Px *edges, const int16_t *ac,
                                                       const int16_t *alphas, int w, int h,
                                                       int bd) {
  __shared__ int32_t e[kIntraEdge + 3];
  const int lane = threadIdx.x;
  const rv_intra_job j = jobs[blockIdx.x];
  const Px *eb = edges + (int64_t)blockIdx.x * kIntraEdge;
  for (int i = lane; i < kIntraEdge; i += 64) e[i] = eb[i];
  __syncthreads();
  const int32_t dc = intra_dc<64>(e, j.variant & 3, w, h, bd, lane);
  const int32_t alpha = alphas[blockIdx.x];
  const int16_t *a = ac + (int64_t)blockIdx.x * w * h;
  const int maxv = (1 << bd) - 1;
  for (int i = lane; i < w * h; i += 64) {
    const int r = i / w, c = i - r * w;
    *plane_ptr_mut<Px>(dst, j.x + c, j.y + r) = (Px)clampi(dc + cfl_scaled(alpha, a[i]), 0, maxv);
  }
}

// The chroma block of (bsize, xdec, ydec), or false where cfl_allowed()
// fails or subsampled_size is BLOCK_INVALID.
static bool cfl_geometry(int bsize, int xdec, int ydec, CflGeom *g) {
  if (bsize < 0 || bsize > 9) return false;
  if (!((xdec == 0 && ydec == 0) || (xdec == 1 && (ydec == 0 || ydec == 1)))) return false;
  const int bw = kCflBsW[bsize], bh = kCflBsH[bsize];
  // 4:2:2: BLOCK_4X8, BLOCK_8X16 and BLOCK_16X32 have no subsampled size
  if (xdec == 1 && ydec == 0 && bh == 2 * bw) return false;
  g->w = xdec && bw > 4 ? bw >> 1 : bw;
  g->h = ydec && bh > 4 ? bh >> 1 : bh;
  g->lw = 31 - __builtin_clz((unsigned)g->w);
  g->sh = g->lw + (31 - __builtin_clz((unsigned)g->h));
  g->xdec = xdec;
  g->ydec = ydec;
  g->offx = xdec && bw == 4 ? -4 : 0;
  g->offy = ydec && bh == 4 ? -4 : 0;
  return true;
}

template <typename Px>
static void launch_luma_ac(const rv_plane &luma, const rv_cfl_job *jobs, int n, const CflGeom &g,
                           int16_t *out, hipStream_t s) {
#define RV_CFL_AC(G, NP) \
  cfl_luma_ac_kernel<Px, G, NP><<<(n + 64 / G - 1) / (64 / G), 64, 0, s>>>(luma, jobs, n, g, out)
  switch (g.sh) {
    case 4: RV_CFL_AC(16, 1); break;
    case 5: RV_CFL_AC(32, 1); break;
    case 6: RV_CFL_AC(64, 1); break;
    case 7: RV_CFL_AC(64, 2); break;
    case 8: RV_CFL_AC(64, 4); break;
    case 9: RV_CFL_AC(64, 8); break;
    default: RV_CFL_AC(64, 16); break;
  }
#undef RV_CFL_AC
}

template <typename Px>
static void launch_search(const CflPlanes &P, const rv_cfl_job *jobs, int n, const CflGeom &g,
                          int bd, int16_t *alpha, uint64_t *cost, hipStream_t s) {
#define RV_CFL_S(G, NP, Acc)                                                                   \
  cfl_search_kernel<Px, G, NP, Acc><<<(n + 64 / G - 1) / (64 / G), 64, 0, s>>>(P, jobs, n, g, bd, \
                                                                               alpha, cost)
  switch (g.sh) {
    case 4: RV_CFL_S(16, 1, uint32_t); break;
    case 5: RV_CFL_S(32, 1, uint32_t); break;
    case 6: RV_CFL_S(64, 1, uint32_t); break;
    case 7: RV_CFL_S(64, 2, uint32_t); break;
    case 8: RV_CFL_S(64, 4, uint32_t); break;  // 256 * 4095^2 < 2^32
    case 9:
      if constexpr (sizeof(Px) == 2) {
        if (bd > 10) { RV_CFL_S(64, 8, unsigned long long); break; }
      }
      RV_CFL_S(64, 8, uint32_t);
      break;
    default:
      if constexpr (sizeof(Px) == 2) {
        if (bd > 10) { RV_CFL_S(64, 16, unsigned long long); break; }
      }
      RV_CFL_S(64, 16, uint32_t);  // 1024 * 1023^2 < 2^32
      break;
  }
#undef RV_CFL_S
}

// What cfl_load_run needs of a plane read in runs.
static bool cfl_plane_aligned(const rv_plane &p) {
  return p.data && ((uintptr_t)p.data & 15) == 0 && (p.xorigin & 3) == 0 && (p.stride & 3) == 0;
}

static bool cfl_bit_depth_ok(int bd, int hbd) {
  return (bd == 8 || bd == 10 || bd == 12) && hbd == (bd > 8);
}

}  // namespace rv

using namespace rv;

extern "C" int rv_cfl_luma_ac_batch(const rv_plane *luma, const rv_cfl_job *d_jobs, int n,
                                    int bsize, int xdec, int ydec, int16_t *d_ac, void *stream) {
  CflGeom g;
  if (!luma || !cfl_plane_aligned(*luma) || n < 0 || !cfl_geometry(bsize, xdec, ydec, &g) ||
      (n > 0 && (!d_jobs || !d_ac)))
    return rv_set_error(RV_EINVAL, "rv_cfl_luma_ac_batch: bad arguments");
  if (n == 0) return RV_OK;
  hipStream_t s = rv_resolve_stream(stream);
  if (luma->hbd)
    launch_luma_ac<uint16_t>(*luma, d_jobs, n, g, d_ac, s);
  else
    launch_luma_ac<uint8_t>(*luma, d_jobs, n, g, d_ac, s);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_predict_cfl_batch(const rv_plane *dst, const rv_intra_job *d_jobs,
                                    const void *d_edges, const int16_t *d_ac,
                                    const int16_t *d_alpha, int n, int tx_size, int bit_depth,
                                    void *stream) {
  if (!dst || !dst->data || n < 0 || tx_size < 0 || tx_size > 18 ||
      !cfl_bit_depth_ok(bit_depth, dst->hbd) ||
      (n > 0 && (!d_jobs || !d_edges || !d_ac || !d_alpha)))
    return rv_set_error(RV_EINVAL, "rv_predict_cfl_batch: bad arguments");
  const int w = kCflTxW[tx_size], h = kCflTxH[tx_size];
  if (w > 32 || h > 32)  // pred_cfl_inner asserts 32 >= W (src/predict.rs:843)
    return rv_set_error(RV_ENOTSUP, "rv_predict_cfl_batch: no CfL for 64-point transform sizes");
  if (n == 0) return RV_OK;
  hipStream_t s = rv_resolve_stream(stream);
  if (dst->hbd)
    cfl_pred_kernel<uint16_t><<<n, 64, 0, s>>>(*dst, d_jobs, (const uint16_t *)d_edges, d_ac,
                                               d_alpha, w, h, bit_depth);
  else
    cfl_pred_kernel<uint8_t><<<n, 64, 0, s>>>(*dst, d_jobs, (const uint8_t *)d_edges, d_ac,
                                              d_alpha, w, h, bit_depth);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_cfl_alpha_search_batch(const rv_plane *rec, const rv_plane *src,
                                         const rv_cfl_job *d_jobs, int n, int bsize,
                                         int bit_depth, int16_t *d_alpha, uint64_t *d_cost,
                                         void *stream) {
  CflGeom g;
  bool ok = rec && src && n >= 0;
  for (int p = 0; ok && p < 3; p++)
    ok = rec[p].data && cfl_plane_aligned(p ? src[p] : rec[p]) &&
         cfl_bit_depth_ok(bit_depth, rec[p].hbd) && src[p].hbd == rec[p].hbd;
  // xdec / ydec come from the chroma plane descriptor (src/rdo.rs:1265)
  ok = ok && rec[2].xdec == rec[1].xdec && rec[2].ydec == rec[1].ydec &&
       cfl_geometry(bsize, rec[1].xdec, rec[1].ydec, &g) && (n == 0 || (d_jobs && d_alpha));
  if (!ok) return rv_set_error(RV_EINVAL, "rv_cfl_alpha_search_batch: bad arguments");
  if (n == 0) return RV_OK;
  hipStream_t s = rv_resolve_stream(stream);
  const CflPlanes P = {rec[0], rec[1], rec[2], src[1], src[2]};
  if (rec[0].hbd)
    launch_search<uint16_t>(P, d_jobs, n, g, bit_depth, d_alpha, d_cost, s);
  else
    launch_search<uint8_t>(P, d_jobs, n, g, bit_depth, d_alpha, d_cost, s);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

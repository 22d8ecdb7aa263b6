// rv_intra_screen.hip -- the front of rdo_mode_decision's intra path for any
// block size, frame type and CDF state, as batched operators:
//
//   rv_intra_edges_batch   get_intra_edges (src/partition.rs:500-693) for any
//                          partition / transform block / plane, with
//                          has_top_right / has_bottom_left (src/recon_intra.rs:
//                          174-243, 376-458);
//   rv_intra_screen_batch  the fused mode screening (src/rdo.rs:1029-1127):
//                          edges, the 13 RAV1E_INTRA_MODES predicted and their
//                          get_satd (src/dist.rs:197-328), the two stable
//                          sorts and the merged mode list.
//
// The replay keeps its own superblock-level screening (rv_intra_pass.hip);
// nothing here is called by it.
//
// Screening, work split.  A W x H block has C = (W / N) * (H / N) Hadamard
// chunks of N x N, N = 4 when a side is 4, else 8.  A workgroup of four
// wavefronts serves 64 / C jobs: the 64 lanes of every wavefront are the
// (job, chunk) pairs of those jobs, chunk fastest, and wavefront v takes the
// modes v, v + 4, v + 8 (and 12 for v = 0).  For 64x64 that is the replay's
// kernel: one job per workgroup, a lane per chunk.  For 8x8 and 4x4 it is 64
// jobs per workgroup, a lane per job.  A lane keeps its chunk of the source
// in registers across its modes, and the mode is uniform over a wavefront, so
// the predictor's switch (intra_px) does not diverge.
//
// Two earlier forms are measured beside this one in DESIGN.md §5: mode slots
// x chunks inside one wavefront (up to 13 modes side by side: the switch
// serialises), and C lanes per job walking all 13 modes (a quarter of the
// wavefronts, each four times as long: latency-bound).
//
// The predictions never leave the registers; a job reads its source block
// (once per wavefront) and at most 257 edge pixels, staged in LDS as i32 --
// only the window a W x H block can have, 4 max(W, H) + 1 entries around the
// top-left pixel -- by the job's 4 C threads together.  The chunk sums
// of a mode are reduced over the job's C lanes (group_sum<C>: C <= 64,
// aligned).  The sorts and the merge are a few dozen scalar steps by the
// job's lane 0.
#include <cstdio>

#include "rv_intra.h"

namespace rv {

constexpr uint8_t kScrTxW[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kScrTxH[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
// BlockSize in pixels for the host's checks (0: not taken, see kBlkW4)
constexpr uint8_t kHostBlkW[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kHostBlkH[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct IntraBlkArgs {
  rv_plane rec;
  const rv_intra_tile *tiles;
  int n_tiles;
  const rv_intra_blk_job *jobs;
  int n;
  int bw4, bh4;  // the partition
  int w, h;      // tx_size
  int bd;
  int mode;      // opt_mode, -1 None
};

// The edge geometry of job j, or false where the job names no tile, lies
// outside its tile, or its tile's region (with the row above and the column
// to the left) leaves the plane's allocation: such a job reads nothing.
__device__ __forceinline__ bool blk_geo(const IntraBlkArgs &a, const rv_intra_blk_job &j,
                                        IntraEdgeGeo &g) {
  if (j.tile < 0 || j.tile >= a.n_tiles) return false;
  const rv_intra_tile t = a.tiles[j.tile];
  const int xdec = a.rec.xdec, ydec = a.rec.ydec;
  // TileRect::decimated (src/tiling/tiler.rs)
  const int tx = t.x >> xdec, ty = t.y >> ydec, tw = t.width >> xdec, th = t.height >> ydec;
  if (t.x < 0 || t.y < 0 || tw <= 0 || th <= 0 || tx + tw > a.rec.stride - a.rec.xorigin ||
      ty + th > a.rec.alloc_height - a.rec.yorigin)
    return false;
  if (j.bo_x < 0 || j.bo_y < 0 || j.bx < 0 || j.by < 0 || j.po_x < 0 || j.po_y < 0 ||
      j.po_x > tw - a.w || j.po_y > th - a.h)
    return false;
  g = intra_edge_geo(tx, ty, tw, th, j.bo_x, j.bo_y, a.bw4, a.bh4, j.bx, j.by, j.po_x, j.po_y, a.w,
                     a.h, xdec, ydec, a.mode);
  return true;
}

// One wavefront per job, four jobs per workgroup.
template <typename Px>
__global__ __launch_bounds__(256) void intra_edges_kernel(IntraBlkArgs a, Px *edges) {
  const int job = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (job >= a.n) return;
  IntraEdgeGeo g;
  const bool ok = blk_geo(a, a.jobs[job], g);
  Px *o = edges + (size_t)job * kIntraEdge;
  for (int i = lane; i < kIntraEdge; i += 64) o[i] = ok ? (Px)intra_edge_px<Px>(a.rec, g, a.bd, i) : (Px)0;
}

struct IntraScreenBatchArgs {
  IntraBlkArgs b;
  rv_plane src;
  const uint16_t *cdf;
  int cdf_len;
  int num_modes;
  uint8_t *modes;   // [n][8]
  uint32_t *satd;   // [n][13] or null
  void *edges;      // [n][257] or null
};

template <int W, int H>
struct ScreenShape {
  static constexpr int N = (W == 4 || H == 4) ? 4 : 8;
  static constexpr int C = (W / N) * (H / N);
  static constexpr int JPB = 64 / C;  // jobs per workgroup
  // the edge entries a W x H block can have: [OFF, OFF + STRIDE) (left and
  // bottom-left reach 2 max(W, H) below the top-left pixel at 128, above and
  // top-right as far beyond it, src/partition.rs:559-690)
  static constexpr int M = W > H ? W : H;
  static constexpr int OFF = 128 - 2 * M;
  static constexpr int STRIDE = 4 * M + 1;
};

template <typename Px, int W, int H>
__global__ __launch_bounds__(256) void intra_screen_batch_kernel(IntraScreenBatchArgs a) {
  using S = ScreenShape<W, H>;
  constexpr int N = S::N, C = S::C, JPB = S::JPB;
  constexpr int OFF = S::OFF, STRIDE = S::STRIDE;
  // job s's entry i is at es[s * STRIDE + i], i in [OFF, OFF + STRIDE): the
  // windows tile the array behind a lead of OFF words
  __shared__ int32_t es[OFF + JPB * STRIDE];
  __shared__ uint32_t satd[JPB][kIntraModes];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = lane / C, c = lane % C;  // the job of this workgroup, its chunk
  const int gl = wave * C + c;              // this thread among the job's 4 C
  constexpr int G = 4 * C;
  const int job = blockIdx.x * JPB + slot;
  const bool live = job < a.b.n;
  int32_t *e = es + slot * STRIDE;
  const int bd = a.b.bd;
  rv_intra_blk_job j = {};
  IntraEdgeGeo g = {};
  bool ok = false;
  if (live) {
    j = a.b.jobs[job];
    // the screening is of the luma block itself (src/rdo.rs:1033-1047)
    ok = blk_geo(a.b, j, g) && j.bx == 0 && j.by == 0 && j.po_x == 4 * j.bo_x &&
         j.po_y == 4 * j.bo_y;
    if (ok) {
      const rv_intra_tile t = a.b.tiles[j.tile];
      ok = t.x + j.po_x + W <= a.src.stride - a.src.xorigin &&
           t.y + j.po_y + H <= a.src.alloc_height - a.src.yorigin && j.cdf_off >= 0 &&
           j.cdf_off + kIntraModes <= a.cdf_len;
    }
  }
  for (int i = OFF + gl; i < OFF + STRIDE; i += G)
    e[i] = ok ? intra_edge_px<Px>(a.b.rec, g, bd, i) : 0;
  __syncthreads();
  if (live && a.edges)
    for (int i = gl; i < kIntraEdge; i += G)
      ((Px *)a.edges)[(size_t)job * kIntraEdge + i] = i >= OFF && i < OFF + STRIDE ? (Px)e[i] : (Px)0;
  if (ok) {
    const int var = g.x == 0 && g.y == 0 ? 0 : g.y == 0 ? 1 : g.x == 0 ? 2 : 3;
    const int maxv = (1 << bd) - 1;
    const int cy = (c / (W / N)) * N, cx = (c % (W / N)) * N;  // this lane's chunk
    const rv_intra_tile t = a.b.tiles[j.tile];
    const Px *o = plane_ptr<Px>(a.src, t.x + g.x + cx, t.y + g.y + cy);
    const int64_t os = a.src.stride;
    int32_t src[N * N];
#pragma unroll
    for (int r = 0; r < N; r++)
#pragma unroll
      for (int q = 0; q < N; q++) src[r * N + q] = (int32_t)o[(int64_t)r * os + q];
    const int32_t dcv = intra_dc<C>(e, var, W, H, bd, c);
    for (int k = wave; k < kIntraModes; k += 4) {
      IntraSetup st = intra_setup(kIntraModeOrder[k], var);
      st.dcv = dcv;
      int32_t d[N * N];
#pragma unroll
      for (int r = 0; r < N; r++)
#pragma unroll
        for (int q = 0; q < N; q++)
          d[r * N + q] = src[r * N + q] - intra_px(st, e, W, H, cy + r, cx + q, maxv);
      const uint64_t s = group_sum<C>(satd_chunk<N>(d));
      // get_satd's normalisation: ln = msb(N) (src/dist.rs:326-327)
      if (c == 0) satd[slot][k] = (uint32_t)((s + (N >> 1)) >> (N == 4 ? 2 : 3));
    }
  }
  __syncthreads();
  if (!live || gl != 0) return;
  uint8_t *wm = a.modes + (size_t)job * 8;
  if (!ok) {
    for (int i = 0; i < 8; i++) wm[i] = 0;
    if (a.satd)
      for (int i = 0; i < kIntraModes; i++) a.satd[(size_t)job * kIntraModes + i] = 0;
    return;
  }
  // satds.sort_by_key(|a| a.1): stable, over RAV1E_INTRA_MODES' order.  The
  // orders are 4-bit indices packed into a word (no indexed private array).
  const uint32_t *sj = satd[slot];
  if (a.satd)
    for (int i = 0; i < kIntraModes; i++) a.satd[(size_t)job * kIntraModes + i] = sj[i];
  auto nib = [](uint64_t v, int i) -> int { return (int)((v >> (4 * i)) & 15); };
  auto swap_adj = [](uint64_t v, int i) -> uint64_t {  // entries i - 1 and i
    const uint64_t lo = (v >> (4 * (i - 1))) & 15, hi = (v >> (4 * i)) & 15;
    v &= ~(0xffull << (4 * (i - 1)));
    return v | hi << (4 * (i - 1)) | lo << (4 * i);
  };
  uint64_t so = 0xcba9876543210ull;
  for (int i = 1; i < kIntraModes; i++)
    for (int q = i; q > 0 && sj[nib(so, q)] < sj[nib(so, q - 1)]; q--) so = swap_adj(so, q);
  // probs: d = z - a over the row's first 13 entries, z from 32768, taken per
  // mode of RAV1E_INTRA_MODES; sort_by_key(|a| !a.1): stable, descending
  const uint16_t *row = a.cdf + j.cdf_off;
  uint16_t z = 32768;
  // prob of PredictionMode m at bits [16 m, 16 m + 16) of four words
  uint64_t pw[4] = {0, 0, 0, 0};
#pragma unroll
  for (int m = 0; m < kIntraModes; m++) {
    const uint16_t av = row[m];
    pw[m >> 2] |= (uint64_t)(uint16_t)(z - av) << (16 * (m & 3));
    z = av;
  }
  auto prob = [&](int k) -> uint32_t {  // of RAV1E_INTRA_MODES[k]
    const int m = kIntraModeOrder[k];
    const uint64_t wv = (m >> 2) == 0 ? pw[0] : (m >> 2) == 1 ? pw[1] : (m >> 2) == 2 ? pw[2] : pw[3];
    return (uint32_t)((wv >> (16 * (m & 3))) & 0xffff);
  };
  uint64_t po = 0xcba9876543210ull;
  for (int i = 1; i < kIntraModes; i++)
    for (int q = i; q > 0 && prob(nib(po, q)) > prob(nib(po, q - 1)); q--) po = swap_adj(po, q);
  // modes = the num / 2 most probable, then the num lowest SATDs not yet in,
  // truncated to num (src/rdo.rs:1110-1127); a mode set as a bit mask
  const int num = a.num_modes;
  uint32_t seen = 0;
  int cnt = 0;
  uint64_t out = 0;  // byte 0 the count, then the modes
  for (int i = 0; i < num / 2; i++) {
    const int md = kIntraModeOrder[nib(po, i)];
    seen |= 1u << md;
    if (cnt < num) out |= (uint64_t)md << (8 * (1 + cnt));
    cnt++;
  }
  for (int i = 0; i < num; i++) {
    const int md = kIntraModeOrder[nib(so, i)];
    if (seen & (1u << md)) continue;
    seen |= 1u << md;
    if (cnt < num) out |= (uint64_t)md << (8 * (1 + cnt));
    cnt++;
  }
  out |= (uint64_t)(cnt < num ? cnt : num);
  for (int i = 0; i < 8; i++) wm[i] = (uint8_t)(out >> (8 * i));
}

template <typename Px, int W, int H>
static void launch_screen(const IntraScreenBatchArgs &a, hipStream_t s) {
  constexpr int JPB = ScreenShape<W, H>::JPB;
  intra_screen_batch_kernel<Px, W, H><<<(a.b.n + JPB - 1) / JPB, 256, 0, s>>>(a);
}

template <typename Px>
static bool dispatch_screen(const IntraScreenBatchArgs &a, hipStream_t s) {
  switch (a.b.w * 100 + a.b.h) {
#define RV_SCR(W, H) case W * 100 + H: launch_screen<Px, W, H>(a, s); return true;
    RV_SCR(4, 4) RV_SCR(4, 8) RV_SCR(8, 4) RV_SCR(8, 8) RV_SCR(8, 16) RV_SCR(16, 8) RV_SCR(16, 16)
    RV_SCR(16, 32) RV_SCR(32, 16) RV_SCR(32, 32) RV_SCR(32, 64) RV_SCR(64, 32) RV_SCR(64, 64)
#undef RV_SCR
  }
  return false;
}

// The checks both entry points share; RV_OK, or the code with the message set.
static int check_blk(const char *who, const rv_plane *rec, const rv_intra_tile *d_tiles,
                     int n_tiles, const rv_intra_blk_job *d_jobs, int n, int bsize, int tx_size,
                     int bit_depth) {
  char msg[160];
  auto fail = [&](int code, const char *what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return rv_set_error(code, msg);
  };
  if (!rec || n < 0 || n_tiles < 0) return fail(RV_EINVAL, "null plane or negative count");
  if (bsize < 0 || bsize > 21) return fail(RV_EINVAL, "bsize is no BlockSize");
  if (tx_size < 0 || tx_size > 18) return fail(RV_EINVAL, "tx_size is no TxSize");
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12)
    return fail(RV_EINVAL, "bit_depth must be 8, 10 or 12");
  if (rec->hbd != (bit_depth > 8)) return fail(RV_EINVAL, "pixel type does not fit bit_depth");
  if (!((rec->xdec == 0 && rec->ydec == 0) || (rec->xdec == 1 && (rec->ydec == 0 || rec->ydec == 1))))
    return fail(RV_EINVAL, "subsampling must be 4:4:4, 4:2:2 or 4:2:0");
  if (kHostBlkW[bsize] == 0)
    return fail(RV_ENOTSUP, "4:1 / 1:4 partitions and sizes above 64x64 are not supported");
  // the partition's block in this plane (after supersample_chroma_bsize)
  const int pw = kHostBlkW[bsize] >> rec->xdec > 4 ? kHostBlkW[bsize] >> rec->xdec : 4;
  const int ph = kHostBlkH[bsize] >> rec->ydec > 4 ? kHostBlkH[bsize] >> rec->ydec : 4;
  if (kScrTxW[tx_size] > pw || kScrTxH[tx_size] > ph)
    return fail(RV_EINVAL, "tx_size is larger than the partition's block in this plane");
  if (n > 0 && (!d_jobs || !d_tiles || n_tiles == 0)) return fail(RV_EINVAL, "null jobs or tiles");
  return RV_OK;
}

}  // namespace rv

using namespace rv;

extern "C" int rv_intra_edges_batch(const rv_plane *plane, const rv_intra_tile *d_tiles,
                                    int n_tiles, const rv_intra_blk_job *d_jobs, int n, int bsize,
                                    int tx_size, int bit_depth, int opt_mode, void *d_edges,
                                    void *stream) {
  const int rc = check_blk("rv_intra_edges_batch", plane, d_tiles, n_tiles, d_jobs, n, bsize,
                           tx_size, bit_depth);
  if (rc != RV_OK) return rc;
  if (opt_mode < -1 || opt_mode > 13)
    return rv_set_error(RV_EINVAL, "rv_intra_edges_batch: opt_mode is -1 (None) or an intra mode");
  if (n > 0 && !d_edges) return rv_set_error(RV_EINVAL, "rv_intra_edges_batch: null output");
  if (n == 0) return RV_OK;
  const IntraBlkArgs a = {*plane, d_tiles, n_tiles, d_jobs, n, kHostBlkW[bsize] >> 2,
                          kHostBlkH[bsize] >> 2, kScrTxW[tx_size], kScrTxH[tx_size], bit_depth,
                          opt_mode};
  hipStream_t s = rv_resolve_stream(stream);
  if (plane->hbd)
    intra_edges_kernel<uint16_t><<<(n + 3) / 4, 256, 0, s>>>(a, (uint16_t *)d_edges);
  else
    intra_edges_kernel<uint8_t><<<(n + 3) / 4, 256, 0, s>>>(a, (uint8_t *)d_edges);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_intra_screen_batch(const rv_plane *rec, const rv_plane *src,
                                     const rv_intra_tile *d_tiles, int n_tiles,
                                     const rv_intra_blk_job *d_jobs, int n, int bsize,
                                     int bit_depth, const uint16_t *d_cdf, int cdf_len,
                                     int num_modes_rdo, uint8_t *d_modes, uint32_t *d_satd,
                                     void *d_edges, void *stream) {
  // bsize.tx_size() of the 13 sizes taken: the transform of the same shape
  static const int8_t kBlkTx[13] = {0, 5, 6, 1, 7, 8, 2, 9, 10, 3, 11, 12, 4};
  const int tx_size = bsize >= 0 && bsize < 13 ? kBlkTx[bsize] : 0;
  const int rc = check_blk("rv_intra_screen_batch", rec, d_tiles, n_tiles, d_jobs, n, bsize,
                           tx_size, bit_depth);
  if (rc != RV_OK) return rc;
  if (!src || src->hbd != rec->hbd)
    return rv_set_error(RV_EINVAL, "rv_intra_screen_batch: null source or another pixel type");
  if (rec->xdec || rec->ydec || src->xdec || src->ydec)
    return rv_set_error(RV_EINVAL, "rv_intra_screen_batch: the screening is of luma planes");
  if (num_modes_rdo != 3 && num_modes_rdo != 7)
    return rv_set_error(RV_EINVAL, "rv_intra_screen_batch: num_modes_rdo is 3 or 7");
  if (cdf_len < 0 || (n > 0 && (!d_cdf || !d_modes)))
    return rv_set_error(RV_EINVAL, "rv_intra_screen_batch: null CDF table or output");
  if (n == 0) return RV_OK;
  const IntraScreenBatchArgs a = {
      {*rec, d_tiles, n_tiles, d_jobs, n, kHostBlkW[bsize] >> 2, kHostBlkH[bsize] >> 2,
       kScrTxW[tx_size], kScrTxH[tx_size], bit_depth, -1},
      *src, d_cdf, cdf_len, num_modes_rdo, d_modes, d_satd, d_edges};
  hipStream_t s = rv_resolve_stream(stream);
  const bool ok = rec->hbd ? dispatch_screen<uint16_t>(a, s) : dispatch_screen<uint8_t>(a, s);
  if (!ok) return rv_set_error(RV_ENOTSUP, "rv_intra_screen_batch: block size not supported");
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

// rv_tx_blocks.hip -- a partition's transform blocks as one RDO candidate:
// write_tx_blocks (src/encoder.rs:1757-1903, intra) and write_tx_tree
// (:1907-2037, inter) without the bitstream writer, every encode_tx_block
// (:1077-1237) of the partition in one launch over a batch of jobs:
//
//   intra: get_intra_edges (src/partition.rs:500-693) + predict_intra / CfL,
//   diff (src/encoder.rs:1044-1058) + forward transform (forward.rs:1804-1899),
//   QuantizationContext::update + quantize (src/quantize.rs:205-316),
//   dequantize (:319-333), inverse transform + add (inverse.rs:1939-2114)
//   when need_recon_pixel, and the tx-domain distortion (encoder.rs:1210-1224).
//
// Work split.  A job takes a group of G lanes of a 64-lane wavefront (= one
// workgroup): G = 8 or 16 where no transform of the launch has more points
// (64 / G jobs share the wavefront, as the transform launches pack 64 / max(W,
// H) blocks), else the whole wavefront.  The job's transform blocks run one
// after the other in the reference's order (luma by outer / bx inner, then U,
// then V), because an intra block's edges are the reconstruction of the
// blocks before it.  The modes are launch parameters, so the whole wavefront
// is on one prediction at a time (the predictor's switch diverges only where
// PAETH is demoted at a tile's edge).  Inside a W x H block the element-wise
// steps (edges, prediction, residual, quantize, distortion) use all G lanes;
// the 1-D passes use one lane per column / row with the vector in VGPRs, as
// rv_tx_fwd.hip / rv_tx_inv.hip.
//
// LDS per job: the partition's working copy of every coded plane (u16,
// dynamic: what earlier transform blocks left, the pixels the next block's
// edges read inside the partition), the CfL ac block (i16, dynamic), one
// coefficient block (i32, rows padded to W + 1) and the edge buffer.  `rec`
// is read for edges outside the partition and never written; only levels,
// eobs, distortions and (optionally) the partition's pixels leave the chip.
//
// The kernel is instantiated per pixel type and per largest transform side
// of the launch (8, 16, 32, 64): an instantiation holds the 1-D networks up
// to its side only, so a launch of 8x8 jobs is not held to the register
// budget of the 64-point DCT.
#include <cstdio>

#include "rv_intra.h"
#include "rv_quant.h"
#include "rv_tx2d.h"
#include "rv_tx_layout.h"

namespace rv {

// uv_intra_mode_to_tx_type_context (src/context.rs:615-650) by chroma mode
constexpr uint8_t kTxbUvTxType[14] = {0, 1, 2, 0, 3, 1, 2, 2, 1, 3, 1, 2, 3, 0};

struct TxbArgs {
  rv_plane rec[3], src[3], pred[3], dst[3];
  const rv_intra_tile *tiles;
  int n_tiles;
  const rv_tx_blocks_job *jobs;
  int n;
  rv_tx_blocks_params p;
  int is_inter, has_dst, planes;
  int bw4, bh4;             // the partition, 4x4 luma units
  int xdec, ydec;           // of the chroma planes
  int pw[3], ph[3];         // the partition's pixels in each plane
  int txs[3];               // TxSize of each plane
  int cols[3], rows[3];     // transform blocks of each plane
  int first_block[3], level_off[3];
  int wc_off[3], ac_off;    // u16 / i16 element offsets in a job's dynamic LDS
  int dyn_per_job;          // u16 elements of dynamic LDS per job
  int blocks_per_job, levels_per_job;
  int32_t *levels;
  uint32_t *eob;
  uint64_t *dist;
};

// What a job's transform blocks of one plane share.
struct TxbPlaneCtx {
  int job, p;
  int rtx, rty, rtw, rth;  // the tile's region of this plane (plane pixels)
  int px0, py0;            // the partition's origin inside the region
  int bo_x, bo_y;          // partition_bo (tile-relative 4x4 luma units)
  int mode, tx_type, alpha;
  QCtx q;                  // the quantizer's context
  int32_t dq_dc, dq_ac;    // dequantize's own lookups
};

// Lanes per job by the launch's largest transform side.
template <int MAXN>
struct TxbGroup {
  static constexpr int G = MAXN <= 16 ? MAXN : 64;
};

template <typename Px>
__device__ __forceinline__ bool txb_region_inside(const rv_plane &p, int x, int y, int w, int h) {
  return p.data && x >= -p.xorigin && y >= -p.yorigin && x + w <= p.stride - p.xorigin &&
         y + h <= p.alloc_height - p.yorigin;
}

// One encode_tx_block: transform block (bx, by) of the plane, blk its index
// in the plane.  Returns the eob as write_coeffs_lv_map counts it (src/
// context.rs:3987-3991): one past the last non-zero level in scan order.
template <typename Px, int W, int H, int G>
__device__ __forceinline__ int txb_block(const TxbArgs &a, const TxbPlaneCtx &c, int bx, int by,
                                         int blk, uint16_t *wc, const int16_t *ac, int32_t *buf,
                                         int32_t *e) {
  constexpr int S = W + 1;
  constexpr int CW = W < 32 ? W : 32, CH = H < 32 ? H : 32, CA = CW * CH;
  constexpr int RR = CA / W;  // raster rows the coded area spans
  constexpr int WL = tx::lg2<W>(), HL = tx::lg2<H>();
  constexpr bool RECT2 = (WL - HL == 1) || (HL - WL == 1);
  // the lane in the job's group; opaque to hoisting (rv_device.h)
  const int lane = G == 64 ? (int)rv_tid() : (int)(rv_tid() & (G - 1));
  const int p = c.p, bd = a.p.bit_depth, maxv = (1 << bd) - 1;
  const int PW = a.pw[p];
  const int x0 = bx * W, y0 = by * H;  // inside the partition
  uint16_t *w0 = wc + y0 * PW + x0;
  const int txs = a.txs[p];

  // ---- 1. intra: edges and prediction -------------------------------------
  if (!a.is_inter) {
    const rv_plane &rec = a.rec[p];
    const IntraEdgeGeo g =
        intra_edge_geo(c.rtx, c.rty, c.rtw, c.rth, c.bo_x, c.bo_y, a.bw4, a.bh4, bx, by, c.px0 + x0,
                       c.py0 + y0, W, H, p ? a.xdec : 0, p ? a.ydec : 0, c.mode);
    const int PH = a.ph[p];
    // the partition's own pixels come from the working copy, the rest from rec
    auto rd = [&](int r, int q) -> int32_t {
      const int pr = r - c.py0, pq = q - c.px0;
      if (pr >= 0 && pr < PH && pq >= 0 && pq < PW) return (int32_t)wc[pr * PW + pq];
      return (int32_t)*plane_ptr<Px>(rec, c.rtx + q, c.rty + r);
    };
    // the entries a W x H block can have (rv_intra_screen.hip)
    constexpr int M = W > H ? W : H, OFF = 128 - 2 * M;
    for (int i = OFF + lane; i < OFF + 4 * M + 1; i += G) e[i] = intra_edge_rd(g, bd, i, rd);
    wave_sync();
    const int var = g.x == 0 && g.y == 0 ? 0 : g.y == 0 ? 1 : g.x == 0 ? 2 : 3;
    const bool cfl = c.mode == 13 && c.alpha != 0;  // alpha == 0 -> DC_PRED (src/predict.rs:223)
    IntraSetup st = intra_setup(c.mode == 13 ? 0 : c.mode, var);
    if (st.mode == 0) st.dcv = intra_dc<G>(e, var, W, H, bd, lane);
    for (int i = lane; i < W * H; i += G) {
      const int r = i / W, q = i % W;
      int32_t v;
      if (cfl)  // pred_cfl_inner (src/predict.rs:836-860)
        v = clampi(st.dcv + cfl_scaled(c.alpha, ac[(y0 + r) * PW + x0 + q]), 0, maxv);
      else
        v = intra_px(st, e, W, H, r, q, maxv);
      w0[r * PW + q] = (uint16_t)v;
    }
    wave_sync();
  }
  if (a.p.skip) return 0;

  // ---- 2. residual, << -shift[0] -------------------------------------------
  const int8_t *sh = kFwdShift[txs][(bd - 8) / 2];
  const int s0 = sh[0], s1 = sh[1], s2 = sh[2];
  {
    const Px *sp = plane_ptr<Px>(a.src[p], c.rtx + c.px0 + x0, c.rty + c.py0 + y0);
    const int64_t ss = a.src[p].stride;
    for (int i = lane; i < W * H; i += G) {
      const int r = i / W, q = i % W;
      const int16_t d = (int16_t)((int16_t)sp[r * ss + q] - (int16_t)w0[r * PW + q]);
      buf[r * S + q] = rsa((int32_t)d, -s0);
    }
  }
  wave_sync();
  // ---- 3. forward: columns (Col::FLIPPED upside down), then the coded rows --
  const int ck = tx_col_kind(c.tx_type), rk = tx_row_kind(c.tx_type);
  if (lane < W) {
    int32_t v[H];
#pragma unroll
    for (int r = 0; r < H; r++) v[r] = buf[(ck == 3 ? H - 1 - r : r) * S + lane];
    fwd_kind<H>(ck, v);
    // quantize reads the first coded_tx_area entries of the W-stride raster
    // (src/encoder.rs:1152-1170), raster rows 0 .. RR - 1: only those rows of
    // the column pass are kept (16 of 64 for TX_64X64; the compiler drops the
    // other outputs' arithmetic)
#pragma unroll
    for (int r = 0; r < RR; r++) buf[r * S + lane] = rsa(v[r], -s1);
  }
  wave_sync();
  if (lane < RR) {
    int32_t v[W];
#pragma unroll
    for (int q = 0; q < W; q++) v[q] = buf[lane * S + q];
    fwd_kind<W>(rk, v);
#pragma unroll
    for (int q = 0; q < W; q++) buf[lane * S + q] = rsa(v[q], -s2);
  }
  wave_sync();
  // ---- 4. quantize; dequantize in place; the distortion of the coded slice --
  constexpr int K = CA >= G ? CA / G : 1;  // quantize_block's scan indices per lane
  const uint16_t *scan = RV_SCANS + RV_SCAN_OFF[txs * 16 + c.tx_type];
  int32_t *lv = a.levels + (int64_t)c.job * a.levels_per_job + a.level_off[p] + blk * CA;
  const int32_t roff = (1 << c.q.log_tx_scale) - 1;
  uint64_t txd = 0;
  int k = 0, last = 0;
  quantize_block<CA, G>(
      c.q, scan, [&](int pos) { return buf[(pos / W) * S + (pos % W)]; },
      [&](int pos, int32_t q, int32_t) {
        int32_t *ep = buf + (pos / W) * S + (pos % W);
        // dequantize (src/quantize.rs:319-333) with the plane's own delta_q
        const int32_t r =
            wadd(wmul(q, pos == 0 ? c.dq_dc : c.dq_ac), (q >> 31) & roff) >> c.q.log_tx_scale;
        const int32_t dd = wsub(*ep, r);
        txd += (uint64_t)(int64_t)wmul(dd, dd);  // (c * c) as u64: wrapping square, sign-extended
        *ep = r;
        lv[pos] = q;
        k++;
        if (q != 0) last = lane * K + k;
      });
  txd = group_sum<G>(txd);
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, RV_WAVE));
  if (lane == 0) {
    const int bits = 2 * (3 - c.q.log_tx_scale);
    const int64_t o = (int64_t)c.job * a.blocks_per_job + a.first_block[p] + blk;
    a.dist[o] = (txd + (1ull << (bits - 1))) >> bits;
    a.eob[o] = (uint32_t)last;
  }
  wave_sync();
  if (!a.p.need_recon_pixel) return last;

  // ---- 5. inverse: rows of the CW x CH coded block (packed entry i = raster
  // entry i), then columns + add ----------------------------------------------
  const int range = bd + 8;
  {
    int32_t v[W];
    if (lane < CH) {
#pragma unroll
      for (int q = 0; q < W; q++) {
        const int i = lane * CW + q;
        const int32_t raw = q < CW ? buf[(i / W) * S + (i % W)] : 0;
        v[q] = tx::clampv(RECT2 ? round_shift(wmul(raw, 2896), 12) : raw, range);
      }
    }
    wave_sync();  // all reads precede the in-place row writes
    if (lane < CH) {
      inv_kind<W>(rk, v, range);
#pragma unroll
      for (int q = 0; q < W; q++) buf[lane * S + q] = v[q];
    }
  }
  wave_sync();
  if (lane < W) {
    const int crange = bd + 6 > 16 ? bd + 6 : 16;
    const int shift = kInvShift[txs];
    int32_t v[H];
#pragma unroll
    for (int r = 0; r < H; r++)
      v[r] = r < CH ? tx::clampv(round_shift(buf[r * S + lane], shift), crange) : 0;
    inv_kind<H>(ck, v, crange);
#pragma unroll
    for (int r = 0; r < H; r++) {
      uint16_t *q = w0 + r * PW + lane;
      *q = (uint16_t)clampi(wadd((int32_t)*q, round_shift(v[r], 4)), 0, maxv);
    }
  }
  wave_sync();
  return last;
}

template <typename Px, int MAXN>
__global__ __launch_bounds__(64) void tx_blocks_kernel(TxbArgs a) {
  // G lanes per job: a job whose transforms have at most 16 points takes 8 or
  // 16 lanes (one per column / row), and 64 / G jobs share the wavefront
  constexpr int G = TxbGroup<MAXN>::G, JPW = 64 / G;
  extern __shared__ uint16_t txb_dyn_all[];
  __shared__ int32_t buf_all[JPW][MAXN * (MAXN + 1)];
  __shared__ int32_t e_all[JPW][kIntraEdge + 3];
  const int slot = threadIdx.x / G, lane = threadIdx.x % G;
  const int job = blockIdx.x * JPW + slot;
  if (job >= a.n) return;  // the whole lane group
  uint16_t *txb_dyn = txb_dyn_all + slot * a.dyn_per_job;
  int32_t *buf = buf_all[slot], *e = e_all[slot];
  const rv_tx_blocks_job j = a.jobs[job];
  const int bd = a.p.bit_depth;

  // the job's preconditions (the caller's; a job that breaks one reads
  // nothing and yields zeros): a tile, an aligned partition inside it, a
  // qindex, the tile's regions inside the planes
  bool ok = j.tile >= 0 && j.tile < a.n_tiles && j.bo_x >= 0 && j.bo_y >= 0 &&
            j.bo_x % a.bw4 == 0 && j.bo_y % a.bh4 == 0 && j.qindex >= 1 && j.qindex <= 255;
  rv_intra_tile t = {};
  if (ok) {
    t = a.tiles[j.tile];
    ok = t.x >= 0 && t.y >= 0 && 4 * (j.bo_x + a.bw4) <= t.width && 4 * (j.bo_y + a.bh4) <= t.height;
    for (int p = 0; ok && p < a.planes; p++) {
      const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
      const int x = t.x >> xd, y = t.y >> yd, w = t.width >> xd, h = t.height >> yd;
      ok = txb_region_inside<Px>(a.rec[p], x, y, w, h) && txb_region_inside<Px>(a.src[p], x, y, w, h) &&
           (!a.is_inter || txb_region_inside<Px>(a.pred[p], x, y, w, h)) &&
           (!a.has_dst || txb_region_inside<Px>(a.dst[p], x, y, w, h));
    }
  }
  // an inter skip job codes nothing (src/encoder.rs:1914-1916)
  if (!ok || a.p.skip) {
    int32_t *lv = a.levels + (int64_t)job * a.levels_per_job;
    for (int i = lane; i < a.levels_per_job; i += G) lv[i] = 0;
    for (int i = lane; i < a.blocks_per_job; i += G) {
      a.eob[(int64_t)job * a.blocks_per_job + i] = 0;
      a.dist[(int64_t)job * a.blocks_per_job + i] = 0;
    }
    if (!ok || a.is_inter) return;
  }

  int16_t *ac = (int16_t *)(txb_dyn + a.ac_off);
  int luma_eob = 0;
  for (int p = 0; p < a.planes; p++) {
    const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
    TxbPlaneCtx c;
    c.job = job, c.p = p;
    c.rtx = t.x >> xd, c.rty = t.y >> yd, c.rtw = t.width >> xd, c.rth = t.height >> yd;
    // bo.plane_offset (src/context.rs:1293-1298)
    c.px0 = (j.bo_x >> xd) << 2, c.py0 = (j.bo_y >> yd) << 2;
    c.bo_x = j.bo_x, c.bo_y = j.bo_y;
    const int PW = a.pw[p], PH = a.ph[p];
    uint16_t *wc = txb_dyn + a.wc_off[p];
    const int tw = kTxbTxW[a.txs[p]], th = kTxbTxH[a.txs[p]];
    if (a.is_inter) {  // the prediction is the caller's (motion_compensate)
      const Px *pp = plane_ptr<Px>(a.pred[p], c.rtx + c.px0, c.rty + c.py0);
      const int64_t ps = a.pred[p].stride;
      for (int i = lane; i < PW * PH; i += G) wc[i] = (uint16_t)pp[(i / PW) * ps + i % PW];
      wave_sync();
    }
    if (p == 0) {
      c.mode = a.p.luma_mode, c.tx_type = a.p.tx_type, c.alpha = 0;
      c.q = q_ctx(j.qindex, tw * th, !a.is_inter, bd, a.p.dc_delta_q[0], 0);
    } else if (!a.is_inter) {
      c.mode = a.p.chroma_mode;
      c.alpha = p == 1 ? j.alpha_u : j.alpha_v;
      // src/encoder.rs:1846-1850
      c.tx_type = tw >= 32 || th >= 32 ? 0 : kTxbUvTxType[c.mode];
      c.q = q_ctx(j.qindex, tw * th, 1, bd, a.p.dc_delta_q[p], a.p.ac_delta_q[p]);
    } else {
      c.mode = a.p.luma_mode, c.alpha = 0;
      // has_coeff of the luma block (src/encoder.rs:1173-1189, 1984)
      const bool has_coeff = (a.p.need_recon_pixel || a.p.coeff_rate) ? luma_eob != 0 : true;
      c.tx_type = has_coeff ? a.p.tx_type : 0;
      c.q = q_ctx(j.qindex, tw * th, 0, bd, a.p.dc_delta_q[p], a.p.ac_delta_q[p]);
    }
    c.dq_dc = q_lookup(0, j.qindex, a.p.dc_delta_q[p], bd);
    c.dq_ac = q_lookup(1, j.qindex, a.p.ac_delta_q[p], bd);
    if (p == 1 && !a.is_inter && a.p.chroma_mode == 13) {
      // luma_ac (src/encoder.rs:1714-1755) of what the luma working copy holds
      // after the luma blocks (:1834-1836)
      const uint16_t *wl = txb_dyn + a.wc_off[0];
      const int LW = a.pw[0];
      int32_t sum = 0;
      for (int i = lane; i < PW * PH; i += G) {
        const int r = i / PW, q = i % PW;
        const uint16_t *l = wl + (r << a.ydec) * LW + (q << a.xdec);
        int32_t v;
        if (!a.xdec) v = (int32_t)l[0] << 3;
        else if (!a.ydec) v = ((int32_t)l[0] + l[1]) << 2;
        else v = ((int32_t)l[0] + l[1] + l[LW] + l[LW + 1]) << 1;
        ac[i] = (int16_t)v;
        sum += v;
      }
      sum = group_sum<G>(sum);
      const int shf = 31 - __builtin_clz((unsigned)(PW * PH));
      const int32_t avg = (sum + (1 << (shf - 1))) >> shf;
      for (int i = lane; i < PW * PH; i += G) ac[i] = (int16_t)(ac[i] - avg);
      wave_sync();
    }
    for (int by = 0; by < a.rows[p]; by++)
      for (int bx = 0; bx < a.cols[p]; bx++) {
        const int blk = by * a.cols[p] + bx;
        int eob = 0;
        switch (a.txs[p]) {
#define RV_TXB(ID, W, H)                                                             \
  case ID:                                                                           \
    if constexpr (W <= MAXN && H <= MAXN)                                            \
      eob = txb_block<Px, W, H, G>(a, c, bx, by, blk, wc, ac, buf, e);                  \
    break;
          RV_TXB(0, 4, 4) RV_TXB(1, 8, 8) RV_TXB(2, 16, 16) RV_TXB(3, 32, 32) RV_TXB(4, 64, 64)
          RV_TXB(5, 4, 8) RV_TXB(6, 8, 4) RV_TXB(7, 8, 16) RV_TXB(8, 16, 8) RV_TXB(9, 16, 32)
          RV_TXB(10, 32, 16) RV_TXB(11, 32, 64) RV_TXB(12, 64, 32) RV_TXB(13, 4, 16)
          RV_TXB(14, 16, 4) RV_TXB(15, 8, 32) RV_TXB(16, 32, 8) RV_TXB(17, 16, 64)
          RV_TXB(18, 64, 16)
#undef RV_TXB
        }
        if (p == 0) luma_eob = eob;
      }
  }
  if (!a.has_dst) return;
  for (int p = 0; p < a.planes; p++) {
    const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
    const int PW = a.pw[p], PH = a.ph[p];
    const uint16_t *wc = txb_dyn + a.wc_off[p];
    Px *dp = plane_ptr_mut<Px>(a.dst[p], (t.x >> xd) + ((j.bo_x >> xd) << 2),
                               (t.y >> yd) + ((j.bo_y >> yd) << 2));
    const int64_t ds = a.dst[p].stride;
    for (int i = lane; i < PW * PH; i += G) dp[(i / PW) * ds + i % PW] = (Px)wc[i];
  }
}

// Whether the forward (and, with recon, the inverse) 2-D transform takes
// (size, type): fwd_check of rv_tx_fwd.hip, inv_supported of rv_tx_inv.hip.
static int txb_type_check(int ts, int tx_type, int recon) {
  const int w = kTxbTxW[ts], h = kTxbTxH[ts];
  if ((w == 64 || h == 64) && tx_type != 0)
    return rv_set_error(RV_EINVAL, "rv_tx_blocks_batch: a 64-point size takes DCT_DCT only");
  const int ck = tx_col_kind(tx_type), rk = tx_row_kind(tx_type);
  if (rk == 3 || !tx::fwd_supported(ck, h) || !tx::fwd_supported(rk, w))
    return rv_set_error(RV_ENOTSUP, "rv_tx_blocks_batch: the forward transform has no such type");
  if (recon && (!tx::inv_supported(ck, h) || !tx::inv_supported(rk, w)))
    return rv_set_error(RV_ENOTSUP, "rv_tx_blocks_batch: the inverse transform has no such type");
  return RV_OK;
}

template <typename Px, int MAXN>
static void txb_launch_n(const TxbArgs &a, hipStream_t s) {
  constexpr int JPW = 64 / TxbGroup<MAXN>::G;  // jobs per wavefront
  tx_blocks_kernel<Px, MAXN><<<(a.n + JPW - 1) / JPW, 64, (size_t)a.dyn_per_job * 2 * JPW, s>>>(a);
}

template <typename Px>
static void txb_launch(const TxbArgs &a, int maxn, hipStream_t s) {
  switch (maxn) {
    case 8: txb_launch_n<Px, 8>(a, s); break;
    case 16: txb_launch_n<Px, 16>(a, s); break;
    case 32: txb_launch_n<Px, 32>(a, s); break;
    default: txb_launch_n<Px, 64>(a, s); break;
  }
}

}  // namespace rv

using namespace rv;

extern "C" int rv_tx_blocks_layout(int bsize, int tx_size, int xdec, int ydec, int luma_only,
                                   rv_tx_blocks_layout_t *out) {
  return txb_layout(bsize, tx_size, xdec, ydec, luma_only, out);
}

extern "C" int rv_tx_blocks_batch(const rv_plane *rec, const rv_plane *src, const rv_plane *pred,
                                  const rv_plane *dst, const rv_intra_tile *d_tiles, int n_tiles,
                                  const rv_tx_blocks_job *d_jobs, int n,
                                  const rv_tx_blocks_params *params, int32_t *d_levels,
                                  uint32_t *d_eob, uint64_t *d_dist, void *stream) {
  auto fail = [](int code, const char *what) {
    char msg[160];
    snprintf(msg, sizeof msg, "rv_tx_blocks_batch: %s", what);
    return rv_set_error(code, msg);
  };
  if (!params || !rec || !src || n < 0 || n_tiles < 0) return fail(RV_EINVAL, "null argument or negative count");
  const rv_tx_blocks_params &P = *params;
  const int bd = P.bit_depth;
  if (bd != 8 && bd != 10 && bd != 12) return fail(RV_EINVAL, "bit_depth must be 8, 10 or 12");
  const int luma_only = P.luma_only != 0;
  const int xdec = luma_only ? 0 : rec[1].xdec, ydec = luma_only ? 0 : rec[1].ydec;
  rv_tx_blocks_layout_t L;
  const int rc = txb_layout(P.bsize, P.tx_size, xdec, ydec, luma_only, &L);
  if (rc != RV_OK) return rc;
  const bool inter = P.luma_mode >= 14 && P.luma_mode <= 27;
  if (!inter && (P.luma_mode < 0 || P.luma_mode > 12))
    return fail(RV_EINVAL, "luma_mode is an intra mode 0 .. 12 or an inter mode 14 .. 27");
  if (!inter && !luma_only && (P.chroma_mode < 0 || P.chroma_mode > 13))
    return fail(RV_EINVAL, "chroma_mode is an intra mode 0 .. 13");
  if (P.tx_type < 0 || P.tx_type > 15) return fail(RV_EINVAL, "tx_type is no TxType");
  // cfl_allowed (src/partition.rs:174-177)
  if (!inter && !luma_only && P.chroma_mode == 13 && P.bsize > 9)
    return fail(RV_EINVAL, "CfL needs a block size up to BLOCK_32X32");
  const int recon = P.need_recon_pixel != 0;
  if (inter && L.n_blocks[0] != 1)  // write_tx_tree codes one luma block at the origin
    return fail(RV_EINVAL, "an inter partition has one luma transform block: tx_size.block_size() == bsize");
  // encode_tx_block's debug_assert (src/encoder.rs:1111-1113)
  if (!inter && L.n_blocks[0] != 1 && !recon)
    return fail(RV_EINVAL, "intra luma transform blocks smaller than the partition need need_recon_pixel");
  if (inter && !pred) return fail(RV_EINVAL, "an inter launch needs the prediction planes");
  int e = txb_type_check(L.tx_size[0], P.tx_type, recon);
  if (e != RV_OK) return e;
  if (!luma_only) {
    const int uw = kTxbTxW[L.tx_size[1]], uh = kTxbTxH[L.tx_size[1]];
    const int uvt = inter ? P.tx_type : (uw >= 32 || uh >= 32 ? 0 : kTxbUvTxType[P.chroma_mode]);
    if ((e = txb_type_check(L.tx_size[1], uvt, recon)) != RV_OK) return e;
  }
  for (int p = 0; p < L.planes; p++) {
    const rv_plane *set[4] = {rec, src, inter ? pred : nullptr, dst};
    for (int k = 0; k < 4; k++) {
      if (!set[k]) continue;
      const rv_plane &pl = set[k][p];
      if (!pl.data) return fail(RV_EINVAL, "a plane without data");
      if (pl.hbd != (bd > 8)) return fail(RV_EINVAL, "pixel type does not fit bit_depth");
      if (pl.xdec != (p ? xdec : 0) || pl.ydec != (p ? ydec : 0))
        return fail(RV_EINVAL, "the plane sets differ in subsampling");
    }
    if (dst) {  // rec is never written: several candidates at one position are independent
      const size_t px = bd > 8 ? 2 : 1;
      const char *r0 = (const char *)rec[p].data, *d0 = (const char *)dst[p].data;
      const char *r1 = r0 + (size_t)rec[p].stride * rec[p].alloc_height * px;
      const char *d1 = d0 + (size_t)dst[p].stride * dst[p].alloc_height * px;
      if (d0 < r1 && r0 < d1) return fail(RV_EINVAL, "dst aliases rec");
    }
  }
  if (n > 0 && (!d_jobs || !d_tiles || n_tiles == 0 || !d_levels || !d_eob || !d_dist))
    return fail(RV_EINVAL, "null jobs, tiles or outputs");
  if (n == 0) return RV_OK;

  TxbArgs a = {};
  for (int p = 0; p < L.planes; p++) {
    a.rec[p] = rec[p], a.src[p] = src[p];
    if (inter) a.pred[p] = pred[p];
    if (dst) a.dst[p] = dst[p];
  }
  a.tiles = d_tiles, a.n_tiles = n_tiles, a.jobs = d_jobs, a.n = n;
  a.p = P;
  a.p.skip = P.skip != 0, a.p.need_recon_pixel = recon, a.p.coeff_rate = P.coeff_rate != 0;
  a.is_inter = inter, a.has_dst = dst != nullptr, a.planes = L.planes;
  a.bw4 = kTxbBlkW[P.bsize] >> 2, a.bh4 = kTxbBlkH[P.bsize] >> 2;
  a.xdec = xdec, a.ydec = ydec;
  int maxn = 8, off = 0;
  for (int p = 0; p < L.planes; p++) {
    a.pw[p] = L.plane_w[p], a.ph[p] = L.plane_h[p];
    a.txs[p] = L.tx_size[p];
    a.cols[p] = L.cols[p], a.rows[p] = L.rows[p];
    a.first_block[p] = L.first_block[p], a.level_off[p] = L.level_off[p];
    a.wc_off[p] = off;
    off += a.pw[p] * a.ph[p];
    const int w = kTxbTxW[a.txs[p]], h = kTxbTxH[a.txs[p]];
    while (maxn < w || maxn < h) maxn *= 2;
  }
  a.ac_off = off;
  if (!luma_only) off += a.pw[1] * a.ph[1];
  a.blocks_per_job = L.blocks_per_job, a.levels_per_job = L.levels_per_job;
  a.levels = d_levels, a.eob = d_eob, a.dist = d_dist;
  hipStream_t s = rv_resolve_stream(stream);
  a.dyn_per_job = (off + 1) & ~1;  // keeps every job's working copy 4-byte aligned
  if (bd > 8)
    txb_launch<uint16_t>(a, maxn, s);
  else
    txb_launch<uint8_t>(a, maxn, s);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

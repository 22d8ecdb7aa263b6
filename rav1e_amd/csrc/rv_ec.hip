// rv_ec.hip -- coefficient entropy coding: a device tokenizer for
// ContextWriter::write_coeffs_lv_map (src/context.rs:3965-4220) and the host
// range coder of WriterBase<WriterEncoder> (src/ec.rs:100-600).
//
// The work splits where the reference's data dependencies split:
//  * Everything write_coeffs_lv_map derives from a transform block's own
//    coefficients and its neighbours' final coefficient contexts -- the
//    scan, eob, eob_pt / eob_extra, the nz-map and base-range contexts, the
//    txb_skip / dc_sign contexts, the symbol values -- is data-parallel
//    across transform blocks once the blocks are committed.  The block
//    context a block reads (BlockContext::get_txb_ctx, :1776-1868) is the
//    value set_coeff_context (:1594-1609) stored for the block directly
//    above / left of it in the same tile (z-order coding never revisits a
//    column above or a row to the left; a skip leaf stores 0 through
//    reset_skip_context, :1651-1679; a tile starts from zero, the left
//    context restarts every superblock row, :1681-1688).  So one launch
//    stores every block's context value into a per-plane 4x4 map, a second
//    reads its neighbours' values and emits the block's symbols.
//  * What stays sequential is the range coder and the CDF adaptation
//    (update_cdf, src/ec.rs:891-905): the host runs them over the symbol
//    stream of each tile ("tokens": CDF offset + length + symbol, or a raw
//    bit), tiles independently.
//
// Device layout: jobs in coding order (rv_ec_job), token offsets from an
// exclusive scan of the per-job token counts, tokens u32:
//   symbol  bits 0-12 CDF offset (u16 units, rv_ec_tables.h layout),
//           bits 13-17 CDF length (nsymbs + 1), bits 18-22 symbol
//   raw bit bit 31 set, bit 0 the bit (Writer::bit, bool at 16384)
//   edge    the frame-edge partition symbol of write_partition
//           (src/context.rs:2082-2108), only in the mixed streams of
//           rv_ec_mode.hip: bits 0-22 as a symbol's (the partition CDF's
//           offset and length, the symbol is_split), bits 23-24 the gather
//           (1 partition_gather_vert_alike, 2 _horz_alike), bits 25-26 the
//           block-size class bsl the reference hands the gather (which
//           ignores it).  The 2-entry CDF is gathered from the adapting
//           partition CDF when the token is coded; nothing adapts.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rv_device.h"
#include "rv_ec.h"
#include "rv_ec_mode_tables.h"
#include "rv_ec_sym.h"

namespace rv {

struct EcArgs {
  const rv_ec_job *jobs;
  int n, xdec, ydec, map_w4, map_h4;
  const uint32_t *dn;  // non-null: the job count is *dn (<= n, device-generated jobs)
  uint8_t *map;
  uint32_t *count;  // [n] token counts, then exclusive offsets [n + 1]
  int32_t *eob;     // [n]
  uint32_t *tokens;
  uint32_t cap;
  uint32_t *status;  // [0] total tokens, [1] overflow flag
};

__device__ inline uint8_t *ec_map(const EcArgs &a, int tile, int p) {
  return a.map + ((size_t)tile * 3 + p) * a.map_h4 * a.map_w4;
}

// Pass 1, one wavefront per job: eob, the stored context value (cul_level
// with the dc sign, src/context.rs:4209-4217; 0 for eob == 0 and for a skip
// leaf's planes) into the map, and the job's token count.
__device__ void ec_prep_job(const EcArgs &a, int j, int lane);
__global__ __launch_bounds__(256) void ec_prep_kernel(EcArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = a.dn ? (int)*a.dn : a.n;
  for (int j = blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += gridDim.x * 4) ec_prep_job(a, j, lane);
}
__device__ void ec_prep_job(const EcArgs &a, int j, int lane) {
  const rv_ec_job jb = a.jobs[j];
  if (jb.kind == 1) {
    for (int p = 0; p < 3; p++) {
      const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
      const int w4 = max(1, (1 << (jb.bw_lg - 2)) >> xd), h4 = max(1, (1 << (jb.bh_lg - 2)) >> yd);
      uint8_t *m = ec_map(a, jb.tile, p);
      const int x0 = jb.bx >> xd, y0 = jb.by >> yd;
      for (int i = lane; i < w4 * h4; i += 64)
        m[(size_t)(y0 + i / w4) * a.map_w4 + x0 + i % w4] = 0;
    }
  }
  if (jb.kind != 0) {
    if (lane == 0) {
      a.count[j] = 0;
      a.eob[j] = 0;
    }
    return;
  }
  int eob;
  uint8_t val;
  uint32_t count;
  ec_job_stats(jb, lane, eob, val, count);
  const int tx = jb.tx_size;
  const int xd = jb.plane ? a.xdec : 0, yd = jb.plane ? a.ydec : 0;
  const int n4 = 1 << tx;
  uint8_t *m = ec_map(a, jb.tile, jb.plane);
  const int x0 = jb.bx >> xd, y0 = jb.by >> yd;
  for (int i = lane; i < n4 * n4; i += 64) m[(size_t)(y0 + i / n4) * a.map_w4 + x0 + i % n4] = val;
  if (lane == 0) {
    a.count[j] = count;
    a.eob[j] = eob;
  }
}

// Exclusive scan of the counts in place (n <= 1024 * 1024; dn non-null:
// the count is *dn <= n): per-1024 block scans, a scan of the block sums,
// the block offsets added.  v[count] = the total, status[0] too.
__device__ inline int scan_n(int n, const uint32_t *dn) { return dn ? (int)*dn : n; }
__global__ __launch_bounds__(1024) void ec_scan_blocks(uint32_t *v, int n, const uint32_t *dn,
                                                       uint32_t *bsum) {
  __shared__ uint32_t s[1024];
  n = scan_n(n, dn);
  const int i = blockIdx.x * 1024 + threadIdx.x;
  const uint32_t x = i < n ? v[i] : 0;
  s[threadIdx.x] = x;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const uint32_t t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  if (i < n) v[i] = s[threadIdx.x] - x;
  if (threadIdx.x == 1023) bsum[blockIdx.x] = s[1023];
}
__global__ __launch_bounds__(1024) void ec_scan_top(uint32_t *bsum, int n, const uint32_t *dn,
                                                    uint32_t *v, uint32_t *status) {
  __shared__ uint32_t s[1024];
  n = scan_n(n, dn);
  const int nb = (n + 1023) / 1024;
  const uint32_t x = (int)threadIdx.x < nb ? bsum[threadIdx.x] : 0;
  s[threadIdx.x] = x;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const uint32_t t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  if ((int)threadIdx.x < nb) bsum[threadIdx.x] = s[threadIdx.x] - x;
  if (threadIdx.x == 0) {
    v[n] = s[1023];
    if (status) {
      status[0] = s[1023];
      status[1] = 0;
    }
  }
}
__global__ __launch_bounds__(1024) void ec_scan_add(uint32_t *v, int n, const uint32_t *dn,
                                                    const uint32_t *bsum) {
  n = scan_n(n, dn);
  const int i = blockIdx.x * 1024 + threadIdx.x;
  if (i < n) v[i] += bsum[blockIdx.x];
}

void ec_scan(uint32_t *v, int n, const uint32_t *dn, uint32_t *bsum, uint32_t *status,
             hipStream_t st) {
  const int nb = (n + 1023) / 1024;
  ec_scan_blocks<<<nb, 1024, 0, st>>>(v, n, dn, bsum);
  ec_scan_top<<<1, 1024, 0, st>>>(bsum, n, dn, v, status);
  if (nb > 1) ec_scan_add<<<nb, 1024, 0, st>>>(v, n, dn, bsum);
}

// Pass 2, one wavefront per transform-block job: its symbols, in
// write_coeffs_lv_map's order, from its token offset.
__device__ void ec_token_job(const EcArgs &a, int j, int lane, uint8_t *lv);
__global__ __launch_bounds__(256) void ec_token_kernel(EcArgs a) {
  __shared__ uint8_t lds[4][kEcLds];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = a.dn ? (int)*a.dn : a.n;
  for (int j = blockIdx.x * 4 + wv; j < n; j += gridDim.x * 4) {
    ec_token_job(a, j, lane, lds[wv]);
    wave_sync();
  }
}
__device__ void ec_token_job(const EcArgs &a, int j, int lane, uint8_t *lv) {
  const rv_ec_job jb = a.jobs[j];
  if (jb.kind != 0) return;
  const int tx = jb.tx_size, p = jb.plane;
  const int xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
  // get_txb_ctx from the neighbours' stored values (zero outside the tile)
  const int n4 = 1 << tx, x0 = jb.bx >> xd, y0 = jb.by >> yd;
  const uint8_t *m = ec_map(a, jb.tile, p);
  const int ab = (lane < n4 && y0 > 0) ? m[(size_t)(y0 - 1) * a.map_w4 + x0 + lane] : 0;
  const int lf = (lane < n4 && x0 > 0) ? m[(size_t)(y0 + lane) * a.map_w4 + x0 - 1] : 0;
  ec_job_tokens(jb, a.eob[j], a.count[j], ab, lf, TokW{a.tokens, a.cap, a.status}, lane, lv);
}


// ---- the replay's job list -------------------------------------------------
// One thread per superblock of the group in coding order (tiles in raster
// order, superblocks in raster order inside a tile; encode_tile_group /
// encode_tile, src/encoder.rs:2766-2781, 3160-3340): its jobs are [tile
// start] [superblock-row start] then its leaves in z-order
// (encode_partition_topdown, :2392-2470): the Morton walk of the
// superblock's 256 luma 4x4 positions meets each leaf's top-left first.
// pass 0 counts, pass 1 writes at the scanned offsets.
__device__ inline void ec_sb_of(const EcFrameArgs &a, int i, int &sx, int &sy, int &t, int &first,
                                int &rowstart, int &t0x, int &t0y) {
  const int ntx = (a.tw + a.tws - 1) / a.tws;
  int base = 0;
  for (t = 0;; t++) {
    const int tx = t % ntx, ty = t / ntx;
    const int w = min(a.tws, a.tw - tx * a.tws), h = min(a.ths, a.th - ty * a.ths);
    if (i < base + w * h) {
      const int k = i - base;
      t0x = a.tx0 + tx * a.tws;
      t0y = a.ty0 + ty * a.ths;
      sx = t0x + k % w;
      sy = t0y + k / w;
      first = k == 0;
      rowstart = k % w == 0;
      return;
    }
    base += w * h;
  }
}

// The jobs of superblock i (coding order): count (out == nullptr) or write
// them from out[0].  Leaves in z-order: a walk over the superblock's 8x8
// cells in z-order (the depth-first order of the partition tree) that reads
// the block map's leaf size at a cell and, at a leaf's top-left cell, emits
// the leaf and steps over its cells (a 64x64 leaf costs one read).  No
// stack: the explicit depth-first stack it replaces was indexed at run time
// and lived in scratch memory (208 B per lane).
__device__ int ec_sb_jobs(const EcFrameArgs &a, int i, rv_ec_job *out, int cap) {
  int sx, sy, t, first, rowstart, t0x, t0y;
  ec_sb_of(a, i, sx, sy, t, first, rowstart, t0x, t0y);
  int n = 0;
  auto put = [&](const rv_ec_job &jb) {
    if (out && n < cap) out[n] = jb;
    n++;
  };
  rv_ec_job z{};
  z.tile = t;
  if (first) {
    rv_ec_job j3 = z;
    j3.kind = 3;
    put(j3);
  }
  if (rowstart) {
    rv_ec_job j2 = z;
    j2.kind = 2;
    put(j2);
  }
  const int sb = (sy - a.ty0) * a.tw + (sx - a.tx0);
  for (int zc = 0; zc < 64;) {
    // cell zc of the superblock in z-order: de-interleave its bits
    const int cx = (zc & 1) | ((zc >> 1) & 2) | ((zc >> 2) & 4);
    const int cy = ((zc >> 1) & 1) | ((zc >> 2) & 2) | ((zc >> 3) & 4);
    const int x4 = sx * 16 + 2 * cx, y4 = sy * 16 + 2 * cy;
    if (x4 >= a.mi_cols || y4 >= a.mi_rows) {  // outside the frame: no block starts here
      zc++;
      continue;
    }
    const int code = a.mi_lg[(size_t)y4 * a.mi_stride + x4];  // log2 of the leaf's 4x4 units
    const int n4 = 1 << code, lg = code + 2;
    if (((x4 | y4) & (n4 - 1)) != 0) {  // not the leaf's first cell (never for a consistent map)
      zc++;
      continue;
    }
    zc += (n4 >> 1) * (n4 >> 1);  // the leaf's cells
    rv_ec_job jb = z;
    jb.bx = x4 - t0x * 16;
    jb.by = y4 - t0y * 16;
    if (a.mi_skip[(size_t)y4 * a.mi_stride + x4]) {
      jb.kind = 1;
      jb.bw_lg = jb.bh_lg = lg;
      put(jb);
      continue;
    }
    const int l = 6 - lg;
    const EcGenLevel &L = a.lv[l];
    int bi, inter = 1;
    if (l == 0) {
      bi = sb;
      inter = a.words[(size_t)sb * a.words_per_sb + a.win_off] < 1000;
    } else {
      bi = (y4 / n4 - L.y0) * L.gw + (x4 / n4 - L.x0);
    }
    jb.kind = 0;
    jb.is_inter = inter;
    jb.plane = 0;
    jb.tx_size = min(lg - 2, 4);
    jb.bw_lg = jb.bh_lg = lg;
    jb.coeffs = L.l_lev + (size_t)bi * (l == 0 ? 1024 : L.B * L.B);
    put(jb);
    const int plg = lg - a.xdec;
    const int ntc = plg == 6 ? 4 : 1;
    const int ctx_ = plg == 6 ? 3 : plg - 2;
    const int carea = plg == 6 ? 1024 : L.bc * L.bc;
    for (int p = 1; p < 3; p++)
      for (int c = 0; c < ntc; c++) {
        rv_ec_job jc = jb;
        jc.plane = p;
        jc.tx_size = ctx_;
        jc.bw_lg = jc.bh_lg = plg;
        jc.bx = jb.bx + (ntc == 4 ? (c % 2) * 8 : 0);
        jc.by = jb.by + (ntc == 4 ? (c / 2) * 8 : 0);
        if (l == 0)
          jc.coeffs = L.c_lev + (size_t)(p - 1) * a.nsb * a.ntx_c * 1024 +
                      ((size_t)bi * a.ntx_c + c) * 1024;
        else
          jc.coeffs = L.c_lev + (size_t)(p - 1) * L.n * carea + (size_t)bi * carea;
        put(jc);
      }
  }
  return n;
}

// block-wide exclusive scan of one value per thread (1024 threads)
__device__ inline uint32_t block_scan_1024(uint32_t x, uint32_t *s, uint32_t &total) {
  s[threadIdx.x] = x;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const uint32_t t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  total = s[1023];
  const uint32_t r = s[threadIdx.x] - x;
  __syncthreads();
  return r;
}

// Every superblock's job count (pass 0) / its jobs at the scanned offset
// (pass 1), one thread per superblock.
__global__ __launch_bounds__(64) void ec_gen_kernel(EcFrameArgs a, EcFrameBufs b, int pass) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.nsb) return;
  if (!pass) {
    b.sb_off[i] = (uint32_t)ec_sb_jobs(a, i, nullptr, 0);
    return;
  }
  const uint32_t o = b.sb_off[i];
  if (o < (uint32_t)b.max_jobs) ec_sb_jobs(a, i, b.jobs + o, b.max_jobs - (int)o);
}

// One workgroup: the exclusive scan of the superblocks' job counts;
// sb_off[nsb] = the job count (clamped to max_jobs, overflow flagged)
__global__ __launch_bounds__(1024) void ec_sb_scan_kernel(EcFrameArgs a, EcFrameBufs b) {
  __shared__ uint32_t s[1024];
  uint32_t carry = 0;
  for (int c0 = 0; c0 < a.nsb; c0 += 1024) {
    const int i = c0 + threadIdx.x;
    const uint32_t x = i < a.nsb ? b.sb_off[i] : 0;
    uint32_t total;
    const uint32_t o = carry + block_scan_1024(x, s, total);
    if (i < a.nsb) b.sb_off[i] = o;
    carry += total;
  }
  if (threadIdx.x == 0) {
    b.sb_off[a.nsb] = carry < (uint32_t)b.max_jobs ? carry : b.max_jobs;
    if (carry > (uint32_t)b.max_jobs) b.dstat[1] = 1;
  }
}

// One workgroup: the exclusive scan of the jobs' token counts, then the
// host-mapped stat: [total, overflow, jobs, first token of every tile, total]
__global__ __launch_bounds__(1024) void ec_scan_frame_kernel(EcFrameArgs a, EcFrameBufs b) {
  __shared__ uint32_t s[1024];
  const int n = (int)b.sb_off[a.nsb];
  uint32_t carry = 0;
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int i = c0 + threadIdx.x;
    const uint32_t x = i < n ? b.offsets[i] : 0;
    uint32_t total;
    const uint32_t o = carry + block_scan_1024(x, s, total);
    if (i < n) b.offsets[i] = o;
    carry += total;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    b.offsets[n] = carry;
    b.dstat[0] = carry;
    const bool over = b.dstat[1] || carry > b.cap;
    b.dstat[1] = over;
    b.stat[0] = carry;
    b.stat[1] = over;
    b.stat[2] = (uint32_t)n;
    b.stat[3 + b.ntiles] = carry;
  }
  if ((int)threadIdx.x < b.ntiles) {  // tile t's first superblock -> its first job's token
    const int t = threadIdx.x;
    const int ntx = (a.tw + a.tws - 1) / a.tws;
    int base = 0;
    for (int k = 0; k < t; k++) {
      const int tx = k % ntx, ty = k / ntx;
      base += min(a.tws, a.tw - tx * a.tws) * min(a.ths, a.th - ty * a.ths);
    }
    // sb_off holds unclamped prefix sums: past an overflow (dstat[1]) the
    // index is clamped to the job count (the host drops the frame anyway)
    const uint32_t j = b.sb_off[base];
    b.stat[3 + t] = b.offsets[j < (uint32_t)n ? j : (uint32_t)n];
  }
}

int ec_frame_tokens(const EcFrameArgs &a, const EcFrameBufs &b, hipStream_t st) {
  if (b.ntiles > 1024) return rv_set_error(RV_EINVAL, "ec_frame_tokens: more than 1024 tiles");
  EcArgs e;
  e.jobs = b.jobs;
  e.n = b.max_jobs;
  e.dn = b.sb_off + a.nsb;
  e.xdec = a.xdec;
  e.ydec = a.ydec;
  e.map_w4 = b.map_w4;
  e.map_h4 = b.map_h4;
  e.map = b.map;  // every visible 4x4 of a tile is stored by its leaf before it is read
  e.count = b.offsets;
  e.eob = (int32_t *)b.scratch;
  e.tokens = b.tokens;
  e.cap = b.cap;
  e.status = b.dstat;
  if (hipMemsetAsync(b.dstat, 0, 8, st) != hipSuccess)
    return rv_set_error(RV_EHIP, "ec_frame_tokens: status");
  ec_gen_kernel<<<(a.nsb + 63) / 64, 64, 0, st>>>(a, b, 0);
  ec_sb_scan_kernel<<<1, 1024, 0, st>>>(a, b);
  ec_gen_kernel<<<(a.nsb + 63) / 64, 64, 0, st>>>(a, b, 1);
  // grid-stride over the device-side job count
  ec_prep_kernel<<<1024, 256, 0, st>>>(e);
  ec_scan_frame_kernel<<<1, 1024, 0, st>>>(a, b);
  ec_token_kernel<<<1024, 256, 0, st>>>(e);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

}  // namespace rv

using namespace rv;

// ------------------------------------------------------------ host coder
namespace {

// update_cdf (src/ec.rs:891-905) of a CDF of nsymbs symbols + its counter
inline void update_cdf(uint16_t *cdf, int nsymbs, uint32_t s) {
  const int rate = ec_cdf_rate(nsymbs, cdf[nsymbs]);
  cdf[nsymbs] = ec_cdf_count(cdf[nsymbs]);
  for (int i = 0; i < nsymbs - 1; i++) cdf[i] = ec_cdf_step(cdf[i], rate, (uint32_t)i < s);
}

struct EcWriter {  // WriterBase<WriterEncoder> (src/ec.rs:100-600)
  uint32_t low = 0;
  uint16_t rng = 0x8000;
  int16_t cnt = -9;
  std::vector<uint16_t> pre;

  // lr_compute + store (src/ec.rs:270-295, 339-364)
  inline void store(uint32_t fl, uint32_t fh, uint32_t nms) {
    uint32_t l, rr;
    ec_lr_compute(rng, fl, fh, nms, l, rr);
    uint32_t lo = l + low;
    int c = cnt;
    const int d = ec_norm_shift(rr);  // 16 - ilog(u16)
    int s = c + d;
    if (s >= 0) {
      c += 16;
      uint32_t m = (1u << c) - 1;
      if (s >= 8) {
        pre.push_back((uint16_t)(lo >> c));
        lo &= m;
        c -= 8;
        m >>= 8;
      }
      pre.push_back((uint16_t)(lo >> c));
      s = c + d - 24;
      lo &= m;
    }
    low = lo << d;
    rng = (uint16_t)(rr << d);
    cnt = (int16_t)s;
  }
  // symbol_with_update: cdf of len entries (nsymbs + 1), update_cdf after
  inline void symbol_update(uint32_t s, uint16_t *cdf, int len) {
    const int n = len - 1;
    const uint32_t fl = s > 0 ? cdf[s - 1] : 32768u;
    store(fl, cdf[s], (uint32_t)(n - (int)s));
    update_cdf(cdf, n, s);
  }
  inline void bit(uint32_t b) {  // bool(b, 16384): symbol over [16384, 0]
    store(b ? 16384u : 32768u, b ? 0u : 16384u, b ? 1u : 2u);
  }
  // done() (src/ec.rs:444-486)
  size_t finish() {
    int c = cnt;
    int s = 10 + c;
    const uint32_t m = 0x3FFF;
    uint32_t e = ((low + m) & ~m) | (m + 1);
    if (s > 0) {
      uint32_t n = (1u << (c + 16)) - 1;
      for (;;) {
        pre.push_back((uint16_t)(e >> (c + 16)));
        e &= n;
        s -= 8;
        c -= 8;
        n >>= 8;
        if (s <= 0) break;
      }
    }
    return pre.size();
  }
  void bytes(uint8_t *out) const {
    uint16_t cc = 0;
    for (size_t offs = pre.size(); offs > 0;) {
      offs--;
      cc = (uint16_t)(cc + pre[offs]);
      out[offs] = (uint8_t)cc;
      cc >>= 8;
    }
  }
};

// One stream through a writer W (EcWriter / EcCounter).  total: the size of
// the CDF table the tokens index; Mixed: the edge-partition token is coded
// (the combined table's streams), else bits 23-30 are not looked at.
template <bool Mixed, class W>
static bool ec_run_stream(W &w, const uint32_t *tok, size_t n, uint16_t *cdf, int total) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t t = tok[i];
    if (t >> 31) {
      w.bit(t & 1);
      continue;
    }
    int off, len, s;
    if (!ec_token_ok(t, total, off, len, s)) return false;
    uint16_t *c = cdf + off;
    const int gather = Mixed ? (int)((t >> 23) & 3) : 0;
    if (gather) {
      // partition_gather_vert_alike / _horz_alike (src/context.rs:1995-2057) of a
      // 10-type partition CDF, then Writer::symbol against [x, 0]: no adaptation
      if (!ec_edge_ok(gather, off, len, s, RV_ECM_PARTITION)) return false;
      uint32_t fl, fh, nms;
      ec_edge_store_args(ec_gather_cdf(c, gather), s, fl, fh, nms);
      w.store(fl, fh, nms);
      continue;
    }
    w.store(s > 0 ? c[s - 1] : 32768u, c[s], (uint32_t)(len - 1 - s));
    update_cdf(c, len - 1, (uint32_t)s);
  }
  return true;
}

static long ec_code(const uint32_t *tok, size_t n, uint16_t *cdf, uint8_t *out, size_t cap,
                    int total, bool mixed, const char *null_tok, const char *null_cdf,
                    const char *bad) {
  if (!tok && n) return rv_set_error(RV_EINVAL, null_tok);
  if (!cdf) return rv_set_error(RV_EINVAL, null_cdf);
  EcWriter w;
  w.pre.reserve(n / 4 + 64);
  if (!(mixed ? ec_run_stream<true>(w, tok, n, cdf, total) : ec_run_stream<false>(w, tok, n, cdf, total)))
    return rv_set_error(RV_EINVAL, bad);
  const size_t nb = w.finish();
  if (out && nb <= cap) w.bytes(out);
  return (long)nb;
}

static long ec_count(const uint32_t *tok, size_t n, uint16_t *cdf, uint32_t *state, int total,
                     bool mixed, const char *null_tok, const char *null_cdf, const char *bad_state,
                     const char *bad) {
  if (!tok && n) return rv_set_error(RV_EINVAL, null_tok);
  if (!cdf) return rv_set_error(RV_EINVAL, null_cdf);
  EcCounter w;
  if (state) {
    if (state[0] < 0x8000 || state[0] > 0xFFFF || state[1] > 0xFFFF)
      return rv_set_error(RV_EINVAL, bad_state);
    w.rng = state[0];
    w.cnt = (int16_t)state[1];
  }
  // the byte count enters the rate only through its growth: w counts from 0
  const long before = 8 * (long)w.cnt - (long)w.frac();
  if (!(mixed ? ec_run_stream<true>(w, tok, n, cdf, total) : ec_run_stream<false>(w, tok, n, cdf, total)))
    return rv_set_error(RV_EINVAL, bad);
  const long rate = 64 * (long)w.bytes + 8 * (long)w.cnt - (long)w.frac() - before;
  if (state) {
    state[0] = w.rng;
    state[1] = (uint16_t)w.cnt;
    state[2] += w.bytes;
  }
  return rate;
}

}  // namespace

extern "C" {

long rv_ec_code_tokens(const uint32_t *tok, size_t n, uint16_t *cdf, uint8_t *out, size_t cap) {
  return ec_code(tok, n, cdf, out, cap, RV_EC_TOTAL, false, "rv_ec_code_tokens: null tokens",
                 "rv_ec_code_tokens: null cdf", "rv_ec_code_tokens: bad token");
}

long rv_ec_count_tokens(const uint32_t *tok, size_t n, uint16_t *cdf, uint32_t *state) {
  return ec_count(tok, n, cdf, state, RV_EC_TOTAL, false, "rv_ec_count_tokens: null tokens",
                  "rv_ec_count_tokens: null cdf", "rv_ec_count_tokens: bad state",
                  "rv_ec_count_tokens: bad token");
}

long rv_ec_code_stream(const uint32_t *tok, size_t n, uint16_t *cdf_all, uint8_t *out, size_t cap) {
  return ec_code(tok, n, cdf_all, out, cap, RV_EC_TOTAL_ALL, true, "rv_ec_code_stream: null tokens",
                 "rv_ec_code_stream: null cdf", "rv_ec_code_stream: bad token");
}

long rv_ec_count_stream(const uint32_t *tok, size_t n, uint16_t *cdf_all, uint32_t *state) {
  return ec_count(tok, n, cdf_all, state, RV_EC_TOTAL_ALL, true, "rv_ec_count_stream: null tokens",
                  "rv_ec_count_stream: null cdf", "rv_ec_count_stream: bad state",
                  "rv_ec_count_stream: bad token");
}

int rv_ec_partition_gather(const uint16_t *cdf, int gather) {
  if (!cdf || gather < 1 || gather > 2) return rv_set_error(RV_EINVAL, "rv_ec_partition_gather");
  return (int)ec_gather_cdf(cdf, gather);
}

int rv_ec_default_cdf(int qctx, uint16_t *out) {
  if (qctx < 0 || qctx > 3 || !out) return rv_set_error(RV_EINVAL, "rv_ec_default_cdf");
  memcpy(out, RV_EC_DEFAULT_CDF[qctx], sizeof(RV_EC_DEFAULT_CDF[qctx]));
  return RV_OK;
}

int rv_ec_cdf_total(void) { return RV_EC_TOTAL; }

// CDFContext::reset_counts (src/context.rs:851-) over the coefficient CDFs
void rv_ec_reset_counts(uint16_t *cdf) {
  static const int fam[][3] = {{RV_EC_TXB_SKIP, 65, 3},   {RV_EC_EOB16, 4, 6},
                               {RV_EC_EOB32, 4, 7},       {RV_EC_EOB64, 4, 8},
                               {RV_EC_EOB128, 4, 9},      {RV_EC_EOB256, 4, 10},
                               {RV_EC_EOB512, 4, 11},     {RV_EC_EOB1024, 4, 12},
                               {RV_EC_EOB_EXTRA, 90, 3},  {RV_EC_BASE_EOB, 40, 4},
                               {RV_EC_BASE, 420, 5},      {RV_EC_BR, 210, 5},
                               {RV_EC_DC_SIGN, 6, 3},     {RV_EC_INTER_TX, 16, 17}};
  for (const auto &f : fam)
    for (int i = 0; i < f[1]; i++) cdf[f[0] + i * f[2] + f[2] - 1] = 0;
}

int rv_ec_cdf_total_all(void) { return RV_EC_TOTAL_ALL; }

int rv_ec_default_cdf_all(int qctx, uint16_t *out) {
  if (qctx < 0 || qctx > 3 || !out) return rv_set_error(RV_EINVAL, "rv_ec_default_cdf_all");
  memcpy(out, RV_EC_DEFAULT_CDF[qctx], sizeof(RV_EC_DEFAULT_CDF[qctx]));
  memcpy(out + RV_EC_TOTAL, RV_ECM_DEFAULT_CDF, sizeof(RV_ECM_DEFAULT_CDF));
  return RV_OK;
}

// CDFContext::reset_counts over both parts.  The sliced CDFs keep their
// counter where update_cdf leaves it: partition_cdf[0..4) in entry 4,
// [16..20) in entry 8, uv_mode_cdf[0] in entry UV_INTRA_MODES - 1.
void rv_ec_reset_counts_all(uint16_t *cdf) {
  rv_ec_reset_counts(cdf);
  for (int i = 0; i < 4; i++) {  // inter_tx_cdf[2][i][12], [3][i][2]: the sliced sets' counters
    cdf[RV_EC_INTER_TX + (2 * 4 + i) * 17 + 12] = 0;
    cdf[RV_EC_INTER_TX + (3 * 4 + i) * 17 + 2] = 0;
  }
  static const int fam[][3] = {{RV_ECM_KF_Y, 25, 14},         {RV_ECM_Y_MODE, 4, 14},
                               {RV_ECM_CFL_SIGN, 1, 9},       {RV_ECM_CFL_ALPHA, 6, 17},
                               {RV_ECM_NEWMV, 7, 3},          {RV_ECM_ZEROMV, 2, 3},
                               {RV_ECM_REFMV, 6, 3},          {RV_ECM_SKIP, 3, 3},
                               {RV_ECM_INTRA_INTER, 4, 3},    {RV_ECM_ANGLE_DELTA, 8, 8},
                               {RV_ECM_COMP_MODE, 5, 3},      {RV_ECM_COMP_REF_TYPE, 5, 3},
                               {RV_ECM_COMP_REF, 9, 3},       {RV_ECM_COMP_BWD_REF, 6, 3},
                               {RV_ECM_SINGLE_REF, 18, 3},    {RV_ECM_DRL, 3, 3},
                               {RV_ECM_COMPOUND_MODE, 8, 9},  {RV_ECM_MV_JOINTS, 1, 5},
                               {RV_ECM_SEG, 3, 9}};
  for (const auto &f : fam)
    for (int i = 0; i < f[1]; i++) cdf[f[0] + i * f[2] + f[2] - 1] = 0;
  for (int i = 0; i < 20; i++) cdf[RV_ECM_PARTITION + i * 11 + (i < 4 ? 4 : i < 16 ? 10 : 8)] = 0;
  for (int i = 0; i < 13; i++) {
    cdf[RV_ECM_UV_MODE + i * 15 + 13] = 0;
    cdf[RV_ECM_UV_MODE + (13 + i) * 15 + 14] = 0;
  }
  static const int mvc[][3] = {{RV_ECM_MVC_CLASSES, 1, 12}, {RV_ECM_MVC_CLASS0_FP, 2, 5},
                               {RV_ECM_MVC_FP, 1, 5},       {RV_ECM_MVC_SIGN, 1, 3},
                               {RV_ECM_MVC_CLASS0_HP, 1, 3}, {RV_ECM_MVC_HP, 1, 3},
                               {RV_ECM_MVC_CLASS0, 1, 3},   {RV_ECM_MVC_BITS, 10, 3}};
  for (int k = 0; k < 2; k++)
    for (const auto &f : mvc)
      for (int i = 0; i < f[1]; i++) cdf[RV_ECM_MV_COMP + 69 * k + f[0] + i * f[2] + f[2] - 1] = 0;
}

size_t rv_ec_scratch_bytes(int n_jobs) {
  const size_t nb = ((size_t)n_jobs + 1023) / 1024;
  return (size_t)n_jobs * 4 /* eob */ + ((size_t)n_jobs + 1) * 4 /* counts / offsets */ +
         (nb + 1) * 4 + 16;
}

int rv_ec_tokenize(const rv_ec_job *d_jobs, int n, int xdec, int ydec, int n_tiles, int map_w4,
                   int map_h4, uint8_t *d_map, void *d_scratch, uint32_t *d_offsets,
                   uint32_t *d_tokens, uint32_t token_cap, uint32_t *d_status, void *stream) {
  if (n < 0 || n > 1024 * 1024 || n_tiles < 1 || map_w4 < 1 || map_h4 < 1 || !d_map ||
      !d_scratch || !d_offsets || !d_status || (token_cap && !d_tokens) || (n && !d_jobs))
    return rv_set_error(RV_EINVAL, "rv_ec_tokenize: bad arguments");
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_map, 0, (size_t)n_tiles * 3 * map_w4 * map_h4, st) != hipSuccess)
    return rv_set_error(RV_EHIP, "rv_ec_tokenize: map clear");
  if (n == 0) {
    if (hipMemsetAsync(d_status, 0, 8, st) != hipSuccess ||
        hipMemsetAsync(d_offsets, 0, 4, st) != hipSuccess)
      return rv_set_error(RV_EHIP, "rv_ec_tokenize: status");
    return RV_OK;
  }
  EcArgs a;
  a.jobs = d_jobs;
  a.n = n;
  a.xdec = xdec;
  a.ydec = ydec;
  a.map_w4 = map_w4;
  a.map_h4 = map_h4;
  a.map = d_map;
  a.count = d_offsets;
  a.eob = (int32_t *)d_scratch;
  uint32_t *bsum = (uint32_t *)((char *)d_scratch + (size_t)n * 4);
  a.tokens = d_tokens;
  a.cap = token_cap;
  a.status = d_status;
  a.dn = nullptr;
  const int grid = (n + 3) / 4 < 4096 ? (n + 3) / 4 : 4096;
  ec_prep_kernel<<<grid, 256, 0, st>>>(a);
  ec_scan(d_offsets, n, nullptr, bsum, d_status, st);
  ec_token_kernel<<<grid, 256, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

}  // extern "C"

// rv_ec_cand.hip -- the tokens of RDO candidates against a frozen coding
// state, and their real rates: what luma_chroma_mode_rdo (src/rdo.rs:699-733)
// writes into its WriterCounter for one candidate -- write_partition where
// bsize >= BLOCK_8X8 && is_sqr (:699), encode_block_pre_cdef, then
// encode_block_post_cdef (src/encoder.rs:1446-1662): the mode info and the
// transform tree's coefficients (write_tx_tree / write_tx_blocks, :1757-2030).
//
// A candidate is an optional partition node (rv_ec_mode_job kind 1), exactly
// one block (kind 0) and the block's transform blocks (rv_ec_job kind 0, luma
// then chroma in the reference's order).  Its tokens are contiguous:
// partition, pre_cdef, the mode symbols of post_cdef, the coefficient tokens,
// the order code_tile interleaves.  They are exactly the tokens the block
// would get if it were appended to the committed job lists and tokenized by
// rv_ec_mode_tokenize / rv_ec_tokenize:
//  * the contexts come from the two maps those entry points leave behind
//    (the neighbour records per 8x8 cell, the coefficient context per 4x4
//    cell and plane), which are only read here.  A block reads the cells
//    directly above and left of it, and z-order coding never revisits a column
//    above or a row to the left (rv_ec.hip's header): those cells belong to
//    blocks coded before it whatever is coded after it.  So a map built from
//    *more* blocks than those before the candidate -- the whole frame's --
//    gives the same tokens, and a caller can keep one pair of maps per frame;
//  * candidates at one position, in one call, are independent: nothing is
//    stored into either map;
//  * a candidate's own transform blocks see each other (a 32x32 block coded as
//    four 16x16 luma transforms reads the txb_skip / dc_sign contexts its
//    earlier siblings set): a neighbour cell is looked up first among the
//    candidate's earlier transform blocks of the plane, then in the committed
//    map.  A candidate has few of them, so this is a search, not a map copy;
//  * tile edges, superblock-row starts and skip candidates are the existing
//    tokenizers' (a skip candidate has no transform blocks).
//
// Shape: one wavefront per transform block (its eob, context value and token
// count; then its symbols), one lane per candidate (the checks, the mode
// symbols counted and written by the one function with two sinks), the
// exclusive scan of the per-candidate counts through ec_scan.  The symbol
// functions are the committed tokenizers' (rv_ec_sym.h, rv_ec_mode_sym.h).
//
// A candidate outside the mode tokenizer's restrictions (rv_ec_mode.hip), or
// whose indices, partition node or transform blocks do not fit its block (a
// transform block of another tile, outside the block or the context map, a
// skip block with transform blocks), emits nothing and adds 1 to d_status[2];
// nothing of it is used as an index.  The candidates' transform-block ranges
// are disjoint: the caller's structure, trusted like every job list here.
#include "rv_device.h"
#include "rv_ec.h"
#include "rv_ec_mode_sym.h"
#include "rv_ec_sym.h"

namespace rv {

constexpr uint32_t kTxBad = 0xFFFFFFFFu;

struct CandArgs {
  const rv_ec_cand *cands;
  int n;
  const rv_ec_job *tx;
  int n_tx;
  ModeArgs m;  // the mode jobs, the frame parameters, the frozen record map, tokens, status
  int xdec, ydec, map_w4, map_h4;
  const uint8_t *cmap;  // the frozen coefficient-context map
  uint32_t *offsets;    // [n] token counts, then exclusive offsets [n + 1]
  int32_t *first;       // [n + 1] 0 .. n: one counter group per candidate
  uint32_t *txcnt;      // per transform block: token count (kTxBad: unusable)
  int32_t *txeob;
  uint32_t *txrel;      // first token, relative to its candidate's
  int32_t *txcand;      // its candidate (-1: none, or a rejected one)
  uint8_t *txval;       // the context value set_coeff_context would store
};

__device__ inline bool cand_tx_ok(const rv_ec_job &jb, const CandArgs &a) {
  if (jb.kind != 0 || jb.plane < 0 || jb.plane > 2 || jb.tx_size < 0 || jb.tx_size > 4 ||
      jb.tx_type < 0 || jb.tx_type > 15 || jb.tile < 0 || jb.tile >= a.m.n_tiles || !jb.coeffs ||
      jb.bx < 0 || jb.by < 0 || jb.bw_lg < 0 || jb.bw_lg > 7 || jb.bh_lg < 0 || jb.bh_lg > 7)
    return false;
  const int xd = jb.plane ? a.xdec : 0, yd = jb.plane ? a.ydec : 0, n4 = 1 << jb.tx_size;
  return (jb.bx >> xd) <= a.map_w4 - n4 && (jb.by >> yd) <= a.map_h4 - n4;
}

// Launch 1, one wavefront per transform block: eob, context value, token count
__global__ __launch_bounds__(256) void cand_tx_prep_kernel(CandArgs a) {
  const int lane = threadIdx.x & 63;
  for (int j = blockIdx.x * 4 + (threadIdx.x >> 6); j < a.n_tx; j += gridDim.x * 4) {
    const rv_ec_job jb = a.tx[j];
    int eob = 0;
    uint8_t val = 0;
    uint32_t count = kTxBad;
    if (cand_tx_ok(jb, a)) ec_job_stats(jb, lane, eob, val, count);
    if (lane == 0) {
      a.txcnt[j] = count;
      a.txeob[j] = eob;
      a.txval[j] = val;
    }
  }
}

// Launch 2, one lane per candidate: the checks, its token count, and where each
// of its transform blocks starts inside it.
__global__ __launch_bounds__(256) void cand_count_kernel(CandArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > a.n) return;
  a.first[c] = c;
  if (c == a.n) return;
  const rv_ec_cand cd = a.cands[c];
  const int nm = a.m.n;
  bool ok = cd.block >= 0 && cd.block < nm && cd.part >= -1 && cd.part < nm && cd.tx_first >= 0 &&
            cd.tx_count >= 0 && cd.tx_count <= a.n_tx && cd.tx_first <= a.n_tx - cd.tx_count;
  uint32_t n = 0;
  if (ok) {
    const rv_ec_mode_job blk = a.m.jobs[cd.block];
    int cols, rows;
    ok = blk.kind == 0 && mode_job_ok(blk, a.m, cols, rows);
    CountSink s;
    if (ok && cd.part >= 0) {
      const rv_ec_mode_job pj = a.m.jobs[cd.part];
      int pc, pr;
      ok = pj.kind == 1 && pj.tile == blk.tile && pj.bx == blk.bx && pj.by == blk.by &&
           pj.bsize == blk.bsize && mode_job_ok(pj, a.m, pc, pr);
      if (ok) mode_symbols(pj, a.m, cols, rows, s);
    }
    if (ok) {
      mode_symbols(blk, a.m, cols, rows, s);
      n = s.n;
      const int n4 = 1 << (bsize_lg(blk.bsize) - 2);
      if (blk.skip && cd.tx_count) ok = false;
      for (int k = cd.tx_first; ok && k < cd.tx_first + cd.tx_count; k++) {
        const rv_ec_job t = a.tx[k];
        const uint32_t cnt = a.txcnt[k];
        if (cnt == kTxBad || t.tile != blk.tile || t.bx < blk.bx || t.bx >= blk.bx + n4 ||
            t.by < blk.by || t.by >= blk.by + n4)
          ok = false;
        else
          n += cnt;
      }
    }
    if (ok) {
      uint32_t rel = s.n;
      for (int k = cd.tx_first; k < cd.tx_first + cd.tx_count; k++) {
        a.txrel[k] = rel;
        a.txcand[k] = c;
        rel += a.txcnt[k];
      }
    }
  }
  a.offsets[c] = ok ? n : 0;
  if (!ok) atomicAdd(a.m.status + 2, 1u);
}

// Launch 3, one lane per candidate: partition, pre_cdef and post_cdef's mode symbols
__global__ __launch_bounds__(256) void cand_mode_token_kernel(CandArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.n) return;
  if (a.offsets[c + 1] == a.offsets[c]) return;  // rejected (a block codes its skip flag at least)
  const rv_ec_cand cd = a.cands[c];
  const rv_ec_mode_job blk = a.m.jobs[cd.block];
  const int cols = a.m.tile_dims[2 * blk.tile], rows = a.m.tile_dims[2 * blk.tile + 1];
  WriteSink w{a.m.tokens, a.offsets[c], a.m.cap, a.m.status};
  if (cd.part >= 0) mode_symbols(a.m.jobs[cd.part], a.m, cols, rows, w);
  mode_symbols(blk, a.m, cols, rows, w);
}

// Launch 4, one wavefront per transform block of an accepted candidate
__global__ __launch_bounds__(256) void cand_tx_token_kernel(CandArgs a) {
  __shared__ uint8_t lds[4][kEcLds];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = blockIdx.x * 4 + wv; j < a.n_tx; j += gridDim.x * 4) {
    const int c = a.txcand[j];
    if (c < 0 || c >= a.n) continue;
    const rv_ec_cand cd = a.cands[c];
    const rv_ec_job jb = a.tx[j];
    const int p = jb.plane, xd = p ? a.xdec : 0, yd = p ? a.ydec : 0;
    const int n4 = 1 << jb.tx_size, x0 = jb.bx >> xd, y0 = jb.by >> yd;
    // the committed map (cand_tx_ok: the block's cells are inside it) ...
    const uint8_t *m = a.cmap + ((size_t)jb.tile * 3 + p) * a.map_h4 * a.map_w4;
    int ab = (lane < n4 && y0 > 0) ? m[(size_t)(y0 - 1) * a.map_w4 + x0 + lane] : 0;
    int lf = (lane < n4 && x0 > 0) ? m[(size_t)(y0 + lane) * a.map_w4 + x0 - 1] : 0;
    // ... under the candidate's earlier transform blocks of the plane
    for (int k = cd.tx_first; k < j; k++) {
      const rv_ec_job q = a.tx[k];
      if (q.plane != p) continue;
      const int qn = 1 << q.tx_size, qx = q.bx >> xd, qy = q.by >> yd;
      const int v = a.txval[k];
      if (lane < n4) {
        if (y0 - 1 >= qy && y0 - 1 < qy + qn && x0 + lane >= qx && x0 + lane < qx + qn) ab = v;
        if (x0 - 1 >= qx && x0 - 1 < qx + qn && y0 + lane >= qy && y0 + lane < qy + qn) lf = v;
      }
    }
    ec_job_tokens(jb, a.txeob[j], a.offsets[c] + a.txrel[j], ab, lf,
                  TokW{a.m.tokens, a.m.cap, a.m.status}, lane, lds[wv]);
    wave_sync();
  }
}

// Before the counter reads the tokens: a total past token_cap (d_status[1]
// is set, tokens were dropped) cuts every offset down to the buffer.
__global__ __launch_bounds__(256) void cand_clamp_kernel(CandArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > a.n || a.m.status[0] <= a.m.cap) return;
  if (a.offsets[i] > a.m.cap) a.offsets[i] = a.m.cap;
}

// The scratch buffer's parts (base null: only the size)
static size_t cand_layout(int n, int n_tx, char *base, CandArgs *a, uint32_t **bsum) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + o : nullptr;
    o += (bytes + 15) & ~(size_t)15;
    return p;
  };
  uint32_t *b = (uint32_t *)take((((size_t)n + 1023) / 1024 + 1) * 4);
  int32_t *first = (int32_t *)take(((size_t)n + 1) * 4);
  uint32_t *txcnt = (uint32_t *)take((size_t)n_tx * 4);
  int32_t *txeob = (int32_t *)take((size_t)n_tx * 4);
  uint32_t *txrel = (uint32_t *)take((size_t)n_tx * 4);
  int32_t *txcand = (int32_t *)take((size_t)n_tx * 4);
  uint8_t *txval = (uint8_t *)take((size_t)n_tx);
  if (a) {
    a->first = first;
    a->txcnt = txcnt;
    a->txeob = txeob;
    a->txrel = txrel;
    a->txcand = txcand;
    a->txval = txval;
  }
  if (bsum) *bsum = b;
  return o;
}

// The launches of rv_ec_cand_tokenize on st; a filled for the caller
static int cand_tokenize(const rv_ec_cand *d_cands, int n, const rv_ec_mode_job *d_mode_jobs,
                         int n_mode_jobs, const rv_ec_job *d_tx_jobs, int n_tx_jobs,
                         rv_ec_mode_params params, int n_tiles, const int32_t *d_tile_dims, int xdec,
                         int ydec, int map_w4, int map_h4, const uint8_t *d_coef_map, int map_w8,
                         int map_h8, const uint32_t *d_mode_map, void *d_scratch,
                         uint32_t *d_offsets, uint32_t *d_tokens, uint32_t token_cap,
                         uint32_t *d_status, int status_words, const char *who, hipStream_t st,
                         CandArgs &a) {
  if (n < 0 || n > 1024 * 1024 || n_mode_jobs < 0 || n_tx_jobs < 0 || n_tx_jobs > (1 << 24) ||
      n_tiles < 1 || n_tiles > 1024 || xdec < 0 || xdec > 1 || ydec < 0 || ydec > 1 || map_w4 < 1 ||
      map_h4 < 1 || map_w8 < 1 || map_h8 < 1 || map_w8 > 8192 || map_h8 > 8192 || !d_tile_dims ||
      !d_coef_map || !d_mode_map || !d_scratch || ((uintptr_t)d_scratch & 15) || !d_offsets ||
      !d_status || (token_cap && !d_tokens) || (n && (!d_cands || !d_mode_jobs)) ||
      (n_tx_jobs && !d_tx_jobs))
    return rv_set_error(RV_EINVAL, who);
  if (hipMemsetAsync(d_status, 0, 4 * (size_t)status_words, st) != hipSuccess)
    return rv_set_error(RV_EHIP, who);
  if (n == 0) {
    if (hipMemsetAsync(d_offsets, 0, 4, st) != hipSuccess) return rv_set_error(RV_EHIP, who);
    return RV_OK;
  }
  a.cands = d_cands;
  a.n = n;
  a.tx = d_tx_jobs;
  a.n_tx = n_tx_jobs;
  a.m.jobs = d_mode_jobs;
  a.m.n = n_mode_jobs;
  a.m.prm = params;
  a.m.n_tiles = n_tiles;
  a.m.tile_dims = d_tile_dims;
  a.m.map = d_mode_map;
  a.m.map_w8 = map_w8;
  a.m.map_h8 = map_h8;
  a.m.count = nullptr;
  a.m.tokens = d_tokens;
  a.m.cap = token_cap;
  a.m.status = d_status;
  a.xdec = xdec;
  a.ydec = ydec;
  a.map_w4 = map_w4;
  a.map_h4 = map_h4;
  a.cmap = d_coef_map;
  a.offsets = d_offsets;
  uint32_t *bsum;
  cand_layout(n, n_tx_jobs, (char *)d_scratch, &a, &bsum);
  const int tgrid = (n_tx_jobs + 3) / 4 < 4096 ? (n_tx_jobs + 3) / 4 : 4096;
  if (n_tx_jobs) {
    if (hipMemsetAsync(a.txcand, 0xFF, (size_t)n_tx_jobs * 4, st) != hipSuccess)
      return rv_set_error(RV_EHIP, who);
    cand_tx_prep_kernel<<<tgrid, 256, 0, st>>>(a);
  }
  cand_count_kernel<<<(n + 1 + 255) / 256, 256, 0, st>>>(a);
  // status[0] = the total; status[1] is cleared again, [2] keeps the rejections
  ec_scan(d_offsets, n, nullptr, bsum, d_status, st);
  cand_mode_token_kernel<<<(n + 255) / 256, 256, 0, st>>>(a);
  if (n_tx_jobs) cand_tx_token_kernel<<<tgrid, 256, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

}  // namespace rv

using namespace rv;

extern "C" {

size_t rv_ec_cand_scratch_bytes(int n_cands, int n_tx_jobs) {
  return cand_layout(n_cands < 0 ? 0 : n_cands, n_tx_jobs < 0 ? 0 : n_tx_jobs, nullptr, nullptr,
                     nullptr);
}

int rv_ec_cand_tokenize(const rv_ec_cand *d_cands, int n, const rv_ec_mode_job *d_mode_jobs,
                        int n_mode_jobs, const rv_ec_job *d_tx_jobs, int n_tx_jobs,
                        rv_ec_mode_params params, int n_tiles, const int32_t *d_tile_dims, int xdec,
                        int ydec, int map_w4, int map_h4, const uint8_t *d_coef_map, int map_w8,
                        int map_h8, const uint32_t *d_mode_map, void *d_scratch,
                        uint32_t *d_offsets, uint32_t *d_tokens, uint32_t token_cap,
                        uint32_t *d_status, void *stream) {
  CandArgs a;
  return cand_tokenize(d_cands, n, d_mode_jobs, n_mode_jobs, d_tx_jobs, n_tx_jobs, params, n_tiles,
                       d_tile_dims, xdec, ydec, map_w4, map_h4, d_coef_map, map_w8, map_h8,
                       d_mode_map, d_scratch, d_offsets, d_tokens, token_cap, d_status, 3,
                       "rv_ec_cand_tokenize: bad arguments", rv_resolve_stream(stream), a);
}

int rv_ec_cand_rates(const rv_ec_cand *d_cands, int n, const rv_ec_mode_job *d_mode_jobs,
                     int n_mode_jobs, const rv_ec_job *d_tx_jobs, int n_tx_jobs,
                     rv_ec_mode_params params, int n_tiles, const int32_t *d_tile_dims, int xdec,
                     int ydec, int map_w4, int map_h4, const uint8_t *d_coef_map, int map_w8,
                     int map_h8, const uint32_t *d_mode_map, void *d_scratch, uint32_t *d_offsets,
                     uint32_t *d_tokens, uint32_t token_cap, const uint16_t *d_cdfs_all, int n_cdfs,
                     const int32_t *d_group_cdf, const uint32_t *d_init, uint32_t *d_rate,
                     uint32_t *d_status, void *stream) {
  if (n_cdfs < 1 || !d_cdfs_all || ((uintptr_t)d_cdfs_all & 1) || (n > 0 && !d_rate))
    return rv_set_error(RV_EINVAL, "rv_ec_cand_rates: bad arguments");
  hipStream_t st = rv_resolve_stream(stream);
  CandArgs a;
  const int rc = cand_tokenize(d_cands, n, d_mode_jobs, n_mode_jobs, d_tx_jobs, n_tx_jobs, params,
                               n_tiles, d_tile_dims, xdec, ydec, map_w4, map_h4, d_coef_map, map_w8,
                               map_h8, d_mode_map, d_scratch, d_offsets, d_tokens, token_cap,
                               d_status, 4, "rv_ec_cand_rates: bad arguments", st, a);
  if (rc != RV_OK || n == 0) return rc;
  cand_clamp_kernel<<<(n + 1 + 255) / 256, 256, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return ec_rate_stream_launch(d_tokens, d_offsets, a.first, n, d_cdfs_all, n_cdfs, d_group_cdf,
                               d_init, d_rate, d_status + 3, 0, st);
}

}  // extern "C"

// rv_ec.h -- the replay's coefficient-coding stage (internal): the
// committed frame's transform blocks as a coding-order job list, tokenized
// on the device (rv_ec.hip), range-coded on the host.
#pragma once

#include "rv_device.h"

namespace rv {

// the committed levels of one partition level (0 = the 64x64 superblocks)
struct EcGenLevel {
  const int32_t *l_lev = nullptr, *c_lev = nullptr;  // luma / chroma levels per block
  int n = 0, gw = 0, x0 = 0, y0 = 0;  // blocks, grid width and origin (level-block units)
  int B = 64, bc = 32;                // block size, chroma transform size (luma 64: coded 32)
};

struct EcFrameArgs {
  int tx0, ty0, tw, th, tws, ths;  // the group and the uniform tile size (superblocks)
  int xdec, ydec, ntx_c, nsb;
  const uint8_t *mi_lg, *mi_skip;  // the committed block map (luma 4x4: 4 - level, skip)
  int mi_stride, mi_cols, mi_rows;
  EcGenLevel lv[4];
  const uint64_t *words;  // result words: a superblock's winner >= 1000 is intra
  int words_per_sb, win_off;
};

struct EcFrameBufs {
  int max_jobs, ntiles, map_w4, map_h4;
  rv_ec_job *jobs;
  uint32_t *sb_off;      // [nsb + 1]
  uint8_t *map;
  void *scratch;         // rv_ec_scratch_bytes(max_jobs)
  uint32_t *offsets;     // [max_jobs + 1]
  uint32_t *tokens;      // token_cap u32 (host-mapped)
  uint32_t cap;
  uint32_t *stat;        // host-mapped [total, overflow, jobs, tile token starts [ntiles + 1]]
  uint32_t *dstat;       // device [total, overflow]
};

// ---- the range coder's arithmetic, shared by the host encoder, the host
// counter (rv_ec.hip) and the device counter (rv_ec_rate.hip)
// lr_compute (src/ec.rs:339-355): the low offset and the new range
__host__ __device__ inline void ec_lr_compute(uint32_t r, uint32_t fl, uint32_t fh, uint32_t nms,
                                              uint32_t &l, uint32_t &rr) {
  if (fl < 32768) {
    const uint32_t u = (((r >> 8) * (fl >> 6)) >> 1) + 4 * nms;
    const uint32_t v = (((r >> 8) * (fh >> 6)) >> 1) + 4 * (nms - 1);
    l = r - u;
    rr = (u - v) & 0xFFFF;
  } else {
    l = 0;
    rr = (r - ((((r >> 8) * (fh >> 6)) >> 1) + 4 * (nms - 1))) & 0xFFFF;
  }
}
// 16 - ilog(u16) of a range (16 for 0, which no valid state reaches)
__host__ __device__ inline int ec_norm_shift(uint32_t rr) {
#ifdef __HIP_DEVICE_COMPILE__
  return __clz((int)rr) - 16;
#else
  return rr ? __builtin_clz(rr) - 16 : 16;
#endif
}
// update_cdf (src/ec.rs:891-905): the adaptation rate of a CDF of nsymbs
// symbols whose counter is `count`, and one entry's step.  A rate of 16
// shifts a u16 entry to 0 like every larger one (only a counter that is not
// one gives it), so the shift count stays in range.
__host__ __device__ inline int ec_cdf_rate(int nsymbs, uint32_t count) {
  const int rate = 3 + (nsymbs >> 1 < 2 ? nsymbs >> 1 : 2) + (int)(count >> 4);
  return rate < 16 ? rate : 16;
}
__host__ __device__ inline uint16_t ec_cdf_step(uint32_t v, int rate, bool below) {
  return below ? (uint16_t)(v + ((32768 - (int)v) >> rate)) : (uint16_t)(v - (v >> rate));
}
__host__ __device__ inline uint16_t ec_cdf_count(uint32_t count) {
  return (uint16_t)(count + 1 - (count >> 5));
}

// WriterBase<WriterCounter> (src/ec.rs:187-205, 366-388, 765-780)
struct EcCounter {
  uint32_t rng = 0x8000;
  int32_t cnt = -9;
  uint32_t bytes = 0;
  __host__ __device__ inline void store(uint32_t fl, uint32_t fh, uint32_t nms) {
    uint32_t l, rr;
    ec_lr_compute(rng, fl, fh, nms, l, rr);
    const int d = ec_norm_shift(rr);
    int c = cnt, s = c + d;
    if (s >= 0) {
      c += 16;
      if (s >= 8) {
        bytes++;
        c -= 8;
      }
      bytes++;
      s = c + d - 24;
    }
    rng = (rr << d) & 0xFFFF;
    cnt = (int16_t)s;
  }
  __host__ __device__ inline void bit(uint32_t b) {  // bool(b, 16384)
    store(b ? 16384u : 32768u, b ? 0u : 16384u, b ? 1u : 2u);
  }
  // frac_compute's fraction of the range (OD_BITRES = 3 bits)
  __host__ __device__ inline uint32_t frac() const {
    uint32_t r = rng, l = 0;
    for (int i = 0; i < 3; i++) {
      r = (r * r) >> 15;
      const uint32_t b = r >> 16;
      l = (l << 1) | b;
      r >>= b;
    }
    return l;
  }
  // tell_frac() = (tell() << OD_BITRES) - frac, modulo 2^32
  __host__ __device__ inline uint32_t tell_frac() const {
    return ((bytes * 8 + (uint32_t)cnt + 10) << 3) - frac();
  }
};
// tokens (format in rv_ec.hip)
__host__ __device__ inline uint32_t ec_sym(int off, int len, int s) {
  return (uint32_t)off | ((uint32_t)len << 13) | ((uint32_t)s << 18);
}
__host__ __device__ inline uint32_t ec_raw(int b) { return 0x80000000u | (uint32_t)(b & 1); }
__host__ __device__ inline uint32_t ec_edge(int off, int len, int s, int gather, int bsl) {
  return ec_sym(off, len, s) | ((uint32_t)gather << 23) | ((uint32_t)bsl << 25);
}
// a token's fields and the test both counters and the encoder apply to it
__host__ __device__ inline bool ec_token_ok(uint32_t t, int total, int &off, int &len, int &s) {
  off = (int)(t & 0x1FFF);
  len = (int)((t >> 13) & 31);
  s = (int)((t >> 18) & 31);
  return !(off + len > total || len < 2 || s >= len - 1);
}

// ---- the edge token: partition_gather_vert_alike / _horz_alike
// (src/context.rs:1995-2057), shared by the host coders (rv_ec.hip) and the
// device counter of mixed streams (rv_ec_rate.hip).
// The test of an edge token's fields (after ec_token_ok): gather 1 or 2, a
// whole 10-type partition CDF of the table whose partition CDFs start at
// `part`, the symbol is_split.
__host__ __device__ inline bool ec_edge_ok(int gather, int off, int len, int s, int part) {
  return !(gather < 1 || gather > 2 || len != 11 || s > 1 || off < part ||
           off + len > part + 20 * 11 || (off - part) % 11);
}
// Entry e (0 .. 9) of the partition CDF c[] enters gather g with its
// probability (e > 0 ? c[e - 1] : 32768) - c[e] when the reference's gather
// lists it (1 vert-alike: entries 2 3 4 6 7 9, 2 horz-alike: 1 3 4 5 6 8),
// with 0 otherwise.
__host__ __device__ inline uint32_t ec_gather_term(int gather, int e, uint32_t prev, uint32_t cur) {
  const uint32_t mask = gather == 1 ? 0x2DCu : 0x17Au;
  return (mask >> e) & 1 ? prev - cur : 0u;
}
// The 2-entry CDF is [x, 0], x = 32768 - (32768 - the terms), in u16 arithmetic
__host__ __device__ inline uint32_t ec_gather_x(uint32_t sum_of_terms) { return sum_of_terms & 0xFFFF; }
// Writer::symbol(s, [x, 0]) as store()'s arguments
__host__ __device__ inline void ec_edge_store_args(uint32_t x, int s, uint32_t &fl, uint32_t &fh,
                                                   uint32_t &nms) {
  fl = s ? x : 32768u;
  fh = s ? 0u : x;
  nms = s ? 1u : 2u;
}
// the serial form (host)
inline uint32_t ec_gather_cdf(const uint16_t *c, int gather) {
  uint32_t sum = 0;
  for (int e = 0; e < 10; e++) sum += ec_gather_term(gather, e, e > 0 ? c[e - 1] : 32768u, c[e]);
  return ec_gather_x(sum);
}

// exclusive scan of v[0..n) in place (rv_ec.hip); v[n] and status[0] = the total
void ec_scan(uint32_t *v, int n, const uint32_t *dn, uint32_t *bsum, uint32_t *status,
             hipStream_t st);
// the mixed-stream counter's launch (rv_ec_rate.hip), behind rv_ec_cand.hip's tokenizer
int ec_rate_stream_launch(const uint32_t *d_tokens, const uint32_t *d_offsets,
                          const int32_t *d_group_first, int n_groups, const uint16_t *d_cdfs,
                          int n_cdfs, const int32_t *d_group_cdf, const uint32_t *d_init,
                          uint32_t *d_rate, uint32_t *d_status, int waves, hipStream_t st);
int ec_frame_tokens(const EcFrameArgs &a, const EcFrameBufs &b, hipStream_t st);
// worst-case jobs of a group of nsb superblocks (8x8 leaves at 4:2:0 or
// 64x64 leaves with four chroma transforms at 4:4:4)
inline int ec_max_jobs(int nsb, int ntiles) { return nsb * 194 + 2 * ntiles + 16; }

}  // namespace rv

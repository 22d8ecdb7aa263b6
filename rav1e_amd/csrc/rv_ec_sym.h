// rv_ec_sym.h -- the symbol-forming device functions of write_coeffs_lv_map
// (src/context.rs:3965-4220), shared by the tokenizer of committed blocks
// (rv_ec.hip) and the tokenizer of RDO candidates (rv_ec_cand.hip).  What
// differs between the two is where a transform block's neighbour contexts
// come from and where its token offset and eob are kept, so both are
// parameters here: ec_job_stats forms a block's eob, stored context value and
// token count, ec_job_tokens its symbols from neighbour values the caller
// reads.
#pragma once

#include "rv_device.h"
#include "rv_ec.h"
#include "rv_ec_tables.h"
#include "rv_quant_tables.h"

namespace rv {

constexpr int kEcPadHor = 4;  // TX_PAD_HOR (src/context.rs:253)
constexpr int kEcLds = 36 * 36 + 16;  // levels of a coded 32x32 block + its pad

__device__ inline int coded_w(int tx) { return tx == 4 ? 32 : 4 << tx; }
__device__ inline int golomb_bits(uint32_t level) {  // write_golomb(level - 15): 2 len - 1 bits
  const uint32_t x = level - 14;
  const int len = 32 - __clz(x);
  return 2 * len - 1;
}
__device__ inline int br_count(uint32_t level) {  // coeff_br symbols (src/context.rs:4145-4170)
  if (level <= 2) return 0;
  const int n = (int)(level - 3) / 3 + 1;
  return n < 4 ? n : 4;
}
__device__ inline int eob_pos_token(int eob, int *extra) {  // src/context.rs:3778-3789
  int t;
  if (eob < 33) {
    t = RV_eob_to_pos_small[eob];
  } else {
    int e = (eob - 1) >> 5;
    t = RV_eob_to_pos_large[e < 16 ? e : 16];
  }
  *extra = eob - RV_k_eob_group_start[t];
  return t;
}
__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline int wave_or(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
__device__ inline int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

struct TokW {
  uint32_t *t;
  uint32_t cap;
  uint32_t *status;
  __device__ void put(uint32_t idx, uint32_t v) const {
    if (idx < cap)
      t[idx] = v;
    else
      status[1] = 1;
  }
};

// One wavefront: a transform block's eob, the context value set_coeff_context
// stores for it (cul_level with the dc sign, src/context.rs:4209-4217; 0 for
// eob == 0) and its token count.
__device__ inline void ec_job_stats(const rv_ec_job &jb, int lane, int &eob_out, uint8_t &val_out,
                                    uint32_t &count_out) {
  const int tx = jb.tx_size, cw = coded_w(tx), area = cw * cw;
  const uint16_t *scan = RV_SCANS + RV_SCAN_OFF[tx * 16 + jb.tx_type];
  const int32_t *co = jb.coeffs;
  uint32_t sum = 0;
  int last = 0;
  for (int i = lane; i < area; i += 64) {
    const int32_t v = co[scan[i]];
    sum += (uint32_t)(v < 0 ? -v : v);
    if (v != 0) last = i + 1;
  }
  sum = (uint32_t)wave_sum((int)sum);
  const int eob = sum ? wave_max(last) : 0;
  int cnt = 0;
  for (int i = lane; i < eob; i += 64) {
    const int32_t v = co[scan[i]];
    const uint32_t level = (uint32_t)(v < 0 ? -v : v);
    cnt += 1 + br_count(level) + (level > 0) + (level > 14 ? golomb_bits(level) : 0);
  }
  cnt = wave_sum(cnt);
  int hdr = 1;
  uint8_t val = 0;
  if (eob) {
    int extra;
    const int pt = eob_pos_token(eob, &extra);
    hdr += (jb.plane == 0 && tx < 4 && jb.is_inter) + 1 + RV_k_eob_offset_bits[pt];
    uint32_t cul = sum < 63 ? sum : 63;
    const int32_t dc = co[0];
    if (dc < 0)
      cul |= 1u << 6;
    else if (dc > 0)
      cul += 2u << 6;
    val = (uint8_t)cul;
  }
  eob_out = eob;
  val_out = val;
  count_out = (uint32_t)(hdr + cnt);
}

// get_nz_map_ctx, TX_CLASS_2D (src/context.rs:3791-3878), over the LDS levels
__device__ inline int nz_ctx(const uint8_t *lv, int pos, int bwl, int height, int c, int eob,
                             int tx) {
  if (c == eob - 1) {
    if (c == 0) return 0;
    if (c <= (height << bwl) / 8) return 1;
    if (c <= (height << bwl) / 4) return 2;
    return 3;
  }
  if (pos == 0) return 0;
  const uint8_t *l = lv + pos + ((pos >> bwl) << 2);
  const int st = (1 << bwl) + kEcPadHor;
  int mag = min((int)l[1], 3) + min((int)l[st], 3) + min((int)l[st + 1], 3) + min((int)l[2], 3) +
            min((int)l[2 * st], 3);
  const int row = pos >> bwl, col = pos - (row << bwl);
  const int ctx = min((mag + 1) >> 1, 4);
  return ctx + RV_av1_nz_map_ctx_offset[tx * 25 + min(row, 4) * 5 + min(col, 4)];
}
// get_br_ctx, TX_CLASS_2D (src/context.rs:3901-3948)
__device__ inline int br_ctx(const uint8_t *lv, int c, int bwl) {
  const int row = c >> bwl, col = c - (row << bwl);
  const int st = (1 << bwl) + kEcPadHor;
  const int pos = row * st + col;
  int mag = lv[pos + 1] + lv[pos + st] + lv[pos + st + 1];
  mag = min((mag + 1) >> 1, 6);
  if (c == 0) return mag;
  if (row < 2 && col < 2) return mag + 7;
  return mag + 14;
}

// One wavefront: a transform block's symbols, in write_coeffs_lv_map's order,
// from token offset o.  ab / lf: in lane i < (1 << tx_size) the stored context
// value of the 4x4 cell above column i / left of row i of the block (zero
// outside the tile), zero in the other lanes (get_txb_ctx, :1776-1868).
__device__ inline void ec_job_tokens(const rv_ec_job &jb, int eob, uint32_t o, int ab, int lf,
                                     const TokW &w, int lane, uint8_t *lv) {
  const int tx = jb.tx_size, cw = coded_w(tx), area = cw * cw, bwl = tx == 4 ? 5 : tx + 2;
  const int p = jb.plane, ptype = p ? 1 : 0;
  const int n4 = 1 << tx;
  const int sgn = (lane < n4 ? ((ab >> 6) == 1 ? -1 : (ab >> 6) == 2 ? 1 : 0) +
                                   ((lf >> 6) == 1 ? -1 : (lf >> 6) == 2 ? 1 : 0)
                             : 0);
  const int dc_sign = wave_sum(sgn);
  const int top = wave_or(ab), left = wave_or(lf);
  const int dc_ctx = dc_sign < 0 ? 1 : dc_sign > 0 ? 2 : 0;
  const int tx_lg = 2 * (tx + 2), plane_lg = jb.bw_lg + jb.bh_lg;
  int skip_ctx;
  if (p == 0) {
    if (plane_lg == tx_lg) {
      skip_ctx = 0;
    } else {
      const int t = top & 63, l = left & 63;
      const int mx = min(t | l, 4), mn = min(min(t, l), 4);
      // skip_contexts[min][max] (src/context.rs:1832-1838)
      skip_ctx = mx == 0 ? 1 : mn == 0 ? 2 + (mx > 3) : mx <= 3 ? 4 : mn <= 3 ? 5 : 6;
    }
  } else {
    skip_ctx = (top != 0) + (left != 0) + (plane_lg > tx_lg ? 10 : 7);
  }
  const int txs = tx;
  if (lane == 0) w.put(o, ec_sym(RV_EC_TXB_SKIP + (txs * 13 + skip_ctx) * 3, 3, eob == 0));
  o++;
  if (eob == 0) return;
  // txb_init_levels into LDS (pad columns / rows zero)
  const int st = cw + kEcPadHor;
  for (int i = lane; i < st * (cw + 4); i += 64) lv[i] = 0;
  wave_sync();
  const int32_t *co = jb.coeffs;
  for (int i = lane; i < area; i += 64) {
    const int32_t v = co[i];
    const int32_t av = v < 0 ? -v : v;
    lv[(i >> bwl) * st + (i & (cw - 1))] = (uint8_t)min(av, 127);
  }
  wave_sync();
  if (p == 0 && tx < 4 && jb.is_inter) {
    // write_tx_type: TX_SET_DCT_IDTX (set 1) -> inter_tx_cdf[3][sqr][..=2]
    if (lane == 0)
      w.put(o, ec_sym(RV_EC_INTER_TX + (RV_tx_set_index_inter[1] * 4 + tx) * 17,
                      RV_num_tx_set[1] + 1, RV_av1_tx_ind[16 + jb.tx_type]));
    o++;
  }
  int extra;
  const int pt = eob_pos_token(eob, &extra);
  const int em = min(2 * (tx + 2) - 4, 6), elen = 6 + em;
  int eoff;
  switch (em) {
    case 0: eoff = RV_EC_EOB16; break;
    case 1: eoff = RV_EC_EOB32; break;
    case 2: eoff = RV_EC_EOB64; break;
    case 3: eoff = RV_EC_EOB128; break;
    case 4: eoff = RV_EC_EOB256; break;
    case 5: eoff = RV_EC_EOB512; break;
    default: eoff = RV_EC_EOB1024; break;
  }
  if (lane == 0) w.put(o, ec_sym(eoff + ptype * 2 * elen, elen, pt - 1));
  o++;
  const int ebits = RV_k_eob_offset_bits[pt];
  if (ebits > 0) {
    if (lane == 0)
      w.put(o, ec_sym(RV_EC_EOB_EXTRA + ((txs * 2 + ptype) * 9 + (pt - 3)) * 3, 3,
                      (extra >> (ebits - 1)) & 1));
    if (lane >= 1 && lane < ebits) w.put(o + lane, ec_raw(extra >> (ebits - 1 - lane)));
    o += ebits;
  }
  // the coefficients: lane chunks of the scan, K positions each
  const uint16_t *scan = RV_SCANS + RV_SCAN_OFF[tx * 16 + jb.tx_type];
  const int K = (eob + 63) >> 6;
  const int c0 = min(lane * K, eob), c1 = min(c0 + K, eob);
  int sa = 0, sb = 0;
  for (int c = c0; c < c1; c++) {
    const int32_t v = co[scan[c]];
    const uint32_t level = (uint32_t)(v < 0 ? -v : v);
    sa += 1 + br_count(level);
    sb += (level > 0) + (level > 14 ? golomb_bits(level) : 0);
  }
  const int pa = wave_incl_scan(sa, lane), pb = wave_incl_scan(sb, lane);
  const int ta = __shfl(pa, 63, 64);
  // base / base-range symbols, reverse scan order (src/context.rs:4120-4172)
  uint32_t oa = o + (uint32_t)(ta - pa);
  const int btx = min(txs, 3);
  for (int c = c1 - 1; c >= c0; c--) {
    const int pos = scan[c];
    const int32_t v = co[pos];
    const uint32_t level = (uint32_t)(v < 0 ? -v : v);
    const int ctx = nz_ctx(lv, pos, bwl, cw, c, eob, tx);
    if (c == eob - 1)
      w.put(oa++, ec_sym(RV_EC_BASE_EOB + ((txs * 2 + ptype) * 4 + ctx) * 4, 4,
                         (int)min(level, 3u) - 1));
    else
      w.put(oa++, ec_sym(RV_EC_BASE + ((txs * 2 + ptype) * 42 + ctx) * 5, 5, (int)min(level, 3u)));
    if (level > 2) {
      const int bctx = br_ctx(lv, pos, bwl);
      const int off = RV_EC_BR + ((btx * 2 + ptype) * 21 + bctx) * 5;
      const int br = (int)level - 3;
      for (int idx = 0; idx < 12; idx += 3) {
        const int k = min(br - idx, 3);
        w.put(oa++, ec_sym(off, 5, k));
        if (k < 3) break;
      }
    }
  }
  // signs (dc through dc_sign_cdf) and golomb remainders, scan order
  uint32_t ob = o + (uint32_t)ta + (uint32_t)(pb - sb);
  for (int c = c0; c < c1; c++) {
    const int32_t v = co[scan[c]];
    const uint32_t level = (uint32_t)(v < 0 ? -v : v);
    if (level == 0) continue;
    if (c == 0)
      w.put(ob++, ec_sym(RV_EC_DC_SIGN + (ptype * 3 + dc_ctx) * 3, 3, v < 0));
    else
      w.put(ob++, ec_raw(v < 0));
    if (level > 14) {
      const uint32_t x = level - 14;
      const int len = 32 - __clz(x);
      for (int k = 0; k < len - 1; k++) w.put(ob++, ec_raw(0));
      for (int k = len - 1; k >= 0; k--) w.put(ob++, ec_raw((int)(x >> k)));
    }
  }
}

}  // namespace rv

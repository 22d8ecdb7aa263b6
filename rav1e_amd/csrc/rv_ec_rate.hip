// rv_ec_rate.hip -- the real rate of coefficient coding: WriterBase<
// WriterCounter> (src/ec.rs:187-205: store; :540-551, 891-905:
// symbol_with_update / update_cdf; :501-503: bit; :366-388, 765-780: tell,
// tell_frac, frac_compute) over the token streams of rv_ec_tokenize, one
// counter per candidate ("group": the consecutive jobs a candidate codes).
// It is what encode_tx_block takes as cost_coeffs under the RealRate RDO
// types (src/encoder.rs:1172-1190): write_coeffs_lv_map into a counting
// writer whose CDFs adapt, the tell_frac() difference, then cw.rollback.
//
// One wavefront per group.  A candidate is a serial chain twice over (the
// range state, and the CDFs every symbol adapts), candidates are independent:
//  * the group's CDF snapshot (RV_EC_TOTAL u16) is copied into the wave's
//    LDS slice with 16-byte loads; the copy adapts, the snapshot is only
//    read, and dropping the copy is the rollback;
//  * tokens come in 64 per load, one per lane, and are walked with lane
//    reads, so a token's fields and the whole range state (rng, cnt, bytes)
//    are wave-uniform: store() runs on the scalar unit;
//  * a symbol's CDF (up to 31 entries with its counter) is read by lanes
//    0 .. len - 1, one entry each; fl / fh / the counter are lane reads, and
//    update_cdf's entries adapt in their lanes in parallel;
//  * the next symbol's lanes may read what other lanes just wrote:
//    wave_sync() orders the wave's LDS accesses between the two.
// Nothing here indexes with an unchecked input word: a token is tested
// before its offset is used, a snapshot index before it is multiplied.
#include "rv_ec.h"
#include "rv_ec_tables.h"

namespace rv {

constexpr int kRateWaves = 4;  // groups per workgroup
// The LDS slice keeps the snapshot's 16-byte phase (entry i at i + shift,
// shift < 8), so that whole aligned 16-byte units copy straight across.
constexpr int kRateLds = (RV_EC_TOTAL + 7 + 7) / 8 * 8;  // u16

struct EcRateArgs {
  const uint32_t *tokens, *offsets;
  const int32_t *first;
  int n_groups;
  const uint16_t *cdfs;
  int n_cdfs;
  const int32_t *group_cdf;
  const uint32_t *init;
  uint32_t *rate, *status;
};

__global__ __launch_bounds__(64 * kRateWaves) void ec_rate_kernel(EcRateArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kRateWaves][kRateLds];
  const int lane = threadIdx.x & 63;
  // the wave's index, known uniform: the group's words then load as scalars
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int g = blockIdx.x * kRateWaves + wv;
  if (g >= a.n_groups) return;  // the waves of a block never meet at a barrier
  uint16_t *cdf = lds[wv];

  const uint32_t t0 = a.offsets[a.first[g]], t1 = a.offsets[a.first[g + 1]];
  const int32_t ci = a.group_cdf ? a.group_cdf[g] : 0;
  bool bad = ci < 0 || ci >= a.n_cdfs;
  int shift = 0;
  if (!bad && t0 < t1) {
    const uint16_t *src = a.cdfs + (size_t)ci * RV_EC_TOTAL;
    shift = (int)(((uintptr_t)src & 15) >> 1);
    // unit c holds entries c * 8 - shift .. + 7: a unit inside the snapshot
    // is one aligned 16-byte load, the first / last ones go entry by entry
    for (int c = lane; c < (RV_EC_TOTAL + shift + 7) / 8; c += 64) {
      const int e0 = c * 8 - shift;
      if (e0 >= 0 && e0 + 8 <= RV_EC_TOTAL) {
        reinterpret_cast<uint4 *>(cdf)[c] = *reinterpret_cast<const uint4 *>(src + e0);
      } else {
        for (int k = 0; k < 8; k++)
          if (e0 + k >= 0 && e0 + k < RV_EC_TOTAL) cdf[c * 8 + k] = src[e0 + k];
      }
    }
    wave_sync();
  }
  cdf += shift;

  EcCounter w;
  if (a.init) {
    const uint32_t s = a.init[g];
    w.rng = s & 0xFFFF;
    w.cnt = (int16_t)(s >> 16);
  }
  const uint32_t before = w.tell_frac();
  for (uint32_t base = t0; base < t1 && !bad; base += 64) {
    const uint32_t left = t1 - base;
    const int nt = left < 64 ? (int)left : 64;
    const uint32_t mine = lane < nt ? a.tokens[base + lane] : 0;
    for (int i = 0; i < nt; i++) {
      const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
      if (t >> 31) {
        w.bit(t & 1);
        continue;
      }
      int off, len, s;
      if (!ec_token_ok(t, RV_EC_TOTAL, off, len, s)) {
        bad = true;
        break;
      }
      // off + len <= RV_EC_TOTAL: lanes below len stay inside the slice
      const int nsymbs = len - 1;
      const uint32_t v = lane < len ? cdf[off + lane] : 0;
      const uint32_t fl = s > 0 ? (uint32_t)__builtin_amdgcn_readlane((int)v, s - 1) : 32768u;
      const uint32_t fh = (uint32_t)__builtin_amdgcn_readlane((int)v, s);
      const uint32_t count = (uint32_t)__builtin_amdgcn_readlane((int)v, nsymbs);
      w.store(fl, fh, (uint32_t)(nsymbs - s));
      const int rate = ec_cdf_rate(nsymbs, count);
      if (lane < nsymbs - 1)
        cdf[off + lane] = ec_cdf_step(v, rate, lane < s);
      else if (lane == nsymbs)
        cdf[off + lane] = ec_cdf_count(count);
      wave_sync();
    }
  }
  if (lane == 0) {
    a.rate[g] = bad ? 0xFFFFFFFFu : w.tell_frac() - before;
    if (bad) atomicAdd(a.status, 1u);
  }
}

}  // namespace rv

using namespace rv;

extern "C" int rv_ec_rate_batch(const uint32_t *d_tokens, const uint32_t *d_offsets,
                                const int32_t *d_group_first, int n_groups,
                                const uint16_t *d_cdfs, int n_cdfs, const int32_t *d_group_cdf,
                                const uint32_t *d_init, uint32_t *d_rate, uint32_t *d_status,
                                void *stream) {
  if (n_groups < 0 || n_cdfs < 1 || !d_cdfs || ((uintptr_t)d_cdfs & 1) || !d_status ||
      (n_groups && (!d_offsets || !d_group_first || !d_rate)))
    return rv_set_error(RV_EINVAL, "rv_ec_rate_batch: bad arguments");
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess)
    return rv_set_error(RV_EHIP, "rv_ec_rate_batch: status");
  if (n_groups == 0) return RV_OK;
  const EcRateArgs a = {d_tokens, d_offsets, d_group_first, n_groups, d_cdfs,
                        n_cdfs,   d_group_cdf, d_init,       d_rate,   d_status};
  ec_rate_kernel<<<(n_groups + kRateWaves - 1) / kRateWaves, 64 * kRateWaves, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

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
//
// rv_ec_rate_stream_batch is the same counter over the combined table
// (RV_EC_TOTAL_ALL u16 per snapshot) and the mixed streams of rv_ec_mode.hip /
// rv_ec_cand.hip: what luma_chroma_mode_rdo takes as the rate of a whole
// candidate (src/rdo.rs:689-768: write_partition, encode_block_pre_cdef,
// encode_block_post_cdef into one WriterCounter, the tell_frac() difference).
// It adds the third token kind, the frame-edge partition symbol: lanes 0 .. 9
// hold the partition CDF's entries, each forms its term of
// partition_gather_vert_alike / _horz_alike (src/context.rs:1995-2057; the
// function the host coders use, rv_ec.h), a 16-lane reduction sums them, and
// the symbol is stored against [x, 0] with nothing adapted.
#include "rv_ec.h"
#include "rv_ec_tables.h"
#include "rv_ec_mode_tables.h"

namespace rv {

constexpr int kRateWaves = 4;  // groups per workgroup
// The LDS slice keeps the snapshot's 16-byte phase (entry i at i + shift,
// shift < 8), so that whole aligned 16-byte units copy straight across.
constexpr int kRateLds = (RV_EC_TOTAL + 7 + 7) / 8 * 8;  // u16
constexpr int kStreamLds = (RV_EC_TOTAL_ALL + 7 + 7) / 8 * 8;  // 5968 u16 = 11 936 B per group
constexpr int kStreamWaves = 4;  // groups per workgroup of rv_ec_rate_stream_batch

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

// One group through one wavefront: the body of both kernels.  Total: the u16
// per snapshot (the table the tokens index); Mixed: the tokens are those of
// the combined table's streams, so the edge-partition token is coded, else
// bits 23-30 are not looked at (as in the host's ec_run_stream).  cdf: the
// wave's LDS slice, (Total + 7 + 7) / 8 * 8 u16, 16-byte aligned.
template <int Total, bool Mixed>
__device__ __forceinline__ void ec_rate_group(const EcRateArgs &a, int g, int lane, uint16_t *cdf) {
  const uint32_t t0 = a.offsets[a.first[g]], t1 = a.offsets[a.first[g + 1]];
  const int32_t ci = a.group_cdf ? a.group_cdf[g] : 0;
  bool bad = ci < 0 || ci >= a.n_cdfs;
  int shift = 0;
  if (!bad && t0 < t1) {
    const uint16_t *src = a.cdfs + (size_t)ci * Total;
    shift = (int)(((uintptr_t)src & 15) >> 1);
    // unit c holds entries c * 8 - shift .. + 7: a unit inside the snapshot
    // is one aligned 16-byte load, the first / last ones go entry by entry
    for (int c = lane; c < (Total + shift + 7) / 8; c += 64) {
      const int e0 = c * 8 - shift;
      if (e0 >= 0 && e0 + 8 <= Total) {
        reinterpret_cast<uint4 *>(cdf)[c] = *reinterpret_cast<const uint4 *>(src + e0);
      } else {
        for (int k = 0; k < 8; k++)
          if (e0 + k >= 0 && e0 + k < Total) cdf[c * 8 + k] = src[e0 + k];
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
      if (!ec_token_ok(t, Total, off, len, s)) {
        bad = true;
        break;
      }
      // off + len <= Total: lanes below len stay inside the slice
      const int nsymbs = len - 1;
      const uint32_t v = lane < len ? cdf[off + lane] : 0;
      if (Mixed) {
        const int gather = (int)((t >> 23) & 3);
        if (gather) {
          // the frame-edge partition symbol: Writer::symbol against the 2-entry
          // CDF gathered from the adapting partition CDF; nothing adapts
          if (!ec_edge_ok(gather, off, len, s, RV_ECM_PARTITION)) {
            bad = true;
            break;
          }
          // lane e < 10 holds entry e: its term, summed over the first 16 lanes
          const uint32_t up = (uint32_t)__shfl_up((int)v, 1, 64);
          uint32_t sum = lane < 10 ? ec_gather_term(gather, lane, lane ? up : 32768u, v) : 0u;
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o, 64);
          uint32_t fl, fh, nms;
          ec_edge_store_args(ec_gather_x((uint32_t)__builtin_amdgcn_readfirstlane((int)sum)), s, fl,
                             fh, nms);
          w.store(fl, fh, nms);
          continue;
        }
      }
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

__global__ __launch_bounds__(64 * kRateWaves) void ec_rate_kernel(EcRateArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kRateWaves][kRateLds];
  const int lane = threadIdx.x & 63;
  // the wave's index, known uniform: the group's words then load as scalars
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int g = blockIdx.x * kRateWaves + wv;
  if (g >= a.n_groups) return;  // the waves of a block never meet at a barrier
  ec_rate_group<RV_EC_TOTAL, false>(a, g, lane, lds[wv]);
}

// The same over the combined table and mixed streams, W groups per workgroup.
template <int W>
__global__ __launch_bounds__(64 * W) void ec_rate_stream_kernel(EcRateArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[W][kStreamLds];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int g = blockIdx.x * W + wv;
  if (g >= a.n_groups) return;
  ec_rate_group<RV_EC_TOTAL_ALL, true>(a, g, lane, lds[wv]);
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

namespace rv {

// rv_ec_rate_stream_batch's launch with `waves` groups per workgroup (1, 2, 4;
// 0: kStreamWaves); no status clear (rv_ec_cand.hip launches it behind its own)
int ec_rate_stream_launch(const uint32_t *d_tokens, const uint32_t *d_offsets,
                          const int32_t *d_group_first, int n_groups, const uint16_t *d_cdfs,
                          int n_cdfs, const int32_t *d_group_cdf, const uint32_t *d_init,
                          uint32_t *d_rate, uint32_t *d_status, int waves, hipStream_t st) {
  const EcRateArgs a = {d_tokens, d_offsets, d_group_first, n_groups, d_cdfs,
                        n_cdfs,   d_group_cdf, d_init,       d_rate,   d_status};
  if (waves != 1 && waves != 2 && waves != 4) waves = kStreamWaves;
  const int grid = (n_groups + waves - 1) / waves;
  if (waves == 1)
    ec_rate_stream_kernel<1><<<grid, 64, 0, st>>>(a);
  else if (waves == 2)
    ec_rate_stream_kernel<2><<<grid, 128, 0, st>>>(a);
  else
    ec_rate_stream_kernel<4><<<grid, 256, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

}  // namespace rv

extern "C" int rv_ec_rate_stream_batch_waves(const uint32_t *d_tokens, const uint32_t *d_offsets,
                                             const int32_t *d_group_first, int n_groups,
                                             const uint16_t *d_cdfs_all, int n_cdfs,
                                             const int32_t *d_group_cdf, const uint32_t *d_init,
                                             uint32_t *d_rate, uint32_t *d_status, int waves,
                                             void *stream) {
  if (n_groups < 0 || n_cdfs < 1 || !d_cdfs_all || ((uintptr_t)d_cdfs_all & 1) || !d_status ||
      (waves != 1 && waves != 2 && waves != 4) ||
      (n_groups && (!d_offsets || !d_group_first || !d_rate)))
    return rv_set_error(RV_EINVAL, "rv_ec_rate_stream_batch: bad arguments");
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 4, st) != hipSuccess)
    return rv_set_error(RV_EHIP, "rv_ec_rate_stream_batch: status");
  if (n_groups == 0) return RV_OK;
  return ec_rate_stream_launch(d_tokens, d_offsets, d_group_first, n_groups, d_cdfs_all, n_cdfs,
                               d_group_cdf, d_init, d_rate, d_status, waves, st);
}

extern "C" int rv_ec_rate_stream_batch(const uint32_t *d_tokens, const uint32_t *d_offsets,
                                       const int32_t *d_group_first, int n_groups,
                                       const uint16_t *d_cdfs_all, int n_cdfs,
                                       const int32_t *d_group_cdf, const uint32_t *d_init,
                                       uint32_t *d_rate, uint32_t *d_status, void *stream) {
  return rv_ec_rate_stream_batch_waves(d_tokens, d_offsets, d_group_first, n_groups, d_cdfs_all,
                                       n_cdfs, d_group_cdf, d_init, d_rate, d_status, kStreamWaves,
                                       stream);
}

// rv_tx2d.h -- what the 2-D transform launches share around the 1-D networks
// of rv_tx.h: the forward shifts, the inverse's intermediate shift and the
// run-time dispatch on the 1-D kind.  Used by rv_tx_fwd.hip, rv_tx_inv.hip and
// the fused transform-block kernel (rv_tx_blocks.hip).
#pragma once

#include "rv_tx.h"

namespace rv {

// FWD_SHIFT_* (forward.rs:22-40) by TxSize, shift_idx = (bd - 8) / 2.
static __constant__ int8_t kFwdShift[19][3][3] = {
    {{3, 0, 0}, {2, 0, 1}, {0, 0, 3}},    {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},
    {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},   {{4, -2, 0}, {2, 0, 0}, {0, 0, 2}},
    {{4, -1, -2}, {2, 0, -1}, {0, 0, 1}}, {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},
    {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},   {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},
    {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},   {{4, -2, 0}, {2, 0, 0}, {0, 0, 2}},
    {{4, -2, 0}, {2, 0, 0}, {0, 0, 2}},   {{4, -1, -2}, {2, 0, -1}, {0, 0, 1}},
    {{4, -1, -2}, {2, 0, -1}, {0, 0, 1}}, {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},
    {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},   {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},
    {{4, -1, 0}, {2, 0, 1}, {0, 0, 3}},   {{4, -2, 0}, {2, 0, 0}, {0, 0, 2}},
    {{4, -2, 0}, {2, 0, 0}, {0, 0, 2}}};

// InvBlock::INTERMEDIATE_SHIFT (inverse.rs:1643-1666) by TxSize.
static __constant__ uint8_t kInvShift[19] = {0, 1, 2, 2, 2, 0, 0, 1, 1, 1,
                                             1, 1, 1, 1, 1, 2, 2, 2, 2};

// round_shift_array (src/transform/mod.rs:499-521): bit > 0 rounds right,
// bit < 0 shifts left.
__device__ __forceinline__ int32_t rsa(int32_t v, int bit) {
  if (bit > 0) return round_shift(v, bit);
  if (bit < 0) return (int32_t)((uint32_t)v << -bit);
  return v;
}

template <int KIND, int N>
__device__ __forceinline__ void fwd_dispatch(int32_t *v) {
  if constexpr (tx::fwd_supported(KIND, N)) tx::fwd1d<KIND, N>(v, v);
}

template <int N>
__device__ __forceinline__ void fwd_kind(int kind, int32_t *v) {
  switch (kind) {
    case 0: fwd_dispatch<0, N>(v); break;
    case 1: fwd_dispatch<1, N>(v); break;
    default: fwd_dispatch<2, N>(v); break;  // Adst and FlipAdst (flip is 2-D)
  }
}

template <int KIND, int N>
__device__ __forceinline__ void inv_dispatch(int32_t *v, int range) {
  if constexpr (tx::inv_supported(KIND, N)) tx::inv1d<KIND, N>(v, range);
}
template <int N>
__device__ __forceinline__ void inv_kind(int kind, int32_t *v, int range) {
  switch (kind) {
    case 0: inv_dispatch<0, N>(v, range); break;
    case 1: inv_dispatch<1, N>(v, range); break;
    default: inv_dispatch<2, N>(v, range); break;
  }
}

}  // namespace rv

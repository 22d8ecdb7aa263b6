// rv_distortion.h -- internal: the distortion primitives (src/rdo.rs) shared
// by the RDO kernels (rv_rdo.hip) and loop restoration's unit decision
// (rv_lrf.hip).  Every float operation is the reference's, in its order.
#pragma once
#include "rv_device.h"

namespace rv {

// compute_mean_importance (src/rdo.rs:477-493) of the importance area of
// mw x mh 4x4 blocks at 4x4-block (mi_x, mi_y) of the frame: the f32
// importances of the in-frame 4x4 blocks summed in y-then-x order, divided by
// the full area.  imp: block_importances, w_imp per row, or null (all zero).
__device__ __forceinline__ float mean_importance(const float *imp, int w_imp, int w_in_b, int h_in_b,
                                                 int mi_x, int mi_y, int mw, int mh) {
  if (!imp) return 0.f;
  const int x2 = mi_x + mw < w_in_b ? mi_x + mw : w_in_b;
  const int y2 = mi_y + mh < h_in_b ? mi_y + mh : h_in_b;
  float tot = 0.f;
  for (int y = mi_y; y < y2; y++)
    for (int x = mi_x; x < x2; x++) tot = __fadd_rn(tot, imp[(y >> 1) * w_imp + (x >> 1)]);
  return __fdiv_rn(tot, (float)(mw * mh));
}
// compute_distortion_bias (src/rdo.rs:495-508) of that area (BLOCK_8X8: mw =
// mh = 2; a chroma plane narrower than 8 pixels biases BLOCK_4X4 areas, 1 x 1;
// mh = 0: a square of mw): (mean / 3) as f64 + 0.65.
__device__ __forceinline__ double distortion_bias(const float *imp, int w_imp, int w_in_b, int h_in_b,
                                                  int mi_x, int mi_y, int mw = 2, int mh = 0) {
  if (!imp) return 0.65;  // (0f32 / 3) as f64 + 0.65
  const float mean = mean_importance(imp, w_imp, w_in_b, h_in_b, mi_x, mi_y, mw, mh ? mh : mw);
  return (double)__fdiv_rn(mean, 3.0f) + 0.65;
}
// RawDistortion * bias (src/rdo.rs:539-544): `(value as f64 * bias) as u64`
__device__ __forceinline__ uint64_t distortion_biased(uint64_t v, double bias) {
  return (uint64_t)((double)v * bias);
}

// cdef_dist_wxh_8x8's f64 tail (src/rdo.rs:219-261) from the 8x8 block's
// moments (sums of the source, the distorted block, their squares and
// their products): the ssim boost, `(sse * ssim_boost + 0.5) as u64`.
__device__ __forceinline__ uint64_t cdef_dist_finish(int32_t ss, int32_t sd, uint32_t ss2, uint32_t sd2,
                                                     uint32_t ssd, int bd) {
  const int cs = bd - 8;
  const int64_t s2 = (int64_t)ss2, d2 = (int64_t)sd2, sdv = (int64_t)ssd;
  const double svar = (double)(s2 - (((int64_t)ss * ss + 32) >> 6));
  const double dvar = (double)(d2 - (((int64_t)sd * sd + 32) >> 6));
  const double sse = (double)(d2 + s2 - 2 * sdv);
  const double boost = (4033.0 / 16384.0) * (svar + dvar + (double)(16384ll << (2 * cs))) /
                       sqrt((double)(16265089ull << (4 * cs)) + svar * dvar);
  const double v = sse * boost + 0.5;
  return v > 0.0 ? (uint64_t)v : 0;
}

}  // namespace rv

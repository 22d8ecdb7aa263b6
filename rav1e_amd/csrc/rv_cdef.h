// rv_cdef.h -- internal: rv_cdef.hip's device-resident frame filter (all three
// planes in one launch; the replay's F7), and the CDEF primitives it shares
// with loop restoration's unit input (rv_lrf.hip).
#pragma once
#include "rv_device.h"

namespace rv {

constexpr int kCdefVeryLarge = 0x8000;  // CDEF_VERY_LARGE: outside the visible plane / the tile

// constrain (src/cdef.rs:134-148)
__device__ __forceinline__ int cdef_constrain(int diff, int threshold, int damping) {
  if (!threshold) return 0;
  const int shift = max(0, damping - msb(threshold));
  const int ad = diff < 0 ? -diff : diff;
  const int mag = min(ad, max(0, threshold - (ad >> shift)));
  return diff < 0 ? -mag : mag;
}

// adjust_strength (src/cdef.rs:232-239)
__device__ __forceinline__ int cdef_adjust(int strength, int32_t var) {
  const int i = (var >> 6) ? min(msb(var >> 6), 12) : 0;
  return var ? (strength * (4 + i) + 8) >> 4 : 0;
}

// tap offsets (dy, dx) of cdef_directions (src/cdef.rs:164-173): [dir][k]
static __constant__ int8_t kCdefDirs[8][2][2] = {
    {{-1, 1}, {-2, 2}}, {{0, 1}, {-1, 2}}, {{0, 1}, {0, 2}},  {{0, 1}, {1, 2}},
    {{1, 1}, {2, 2}},   {{1, 0}, {2, 1}},  {{1, 0}, {2, 0}},  {{1, 0}, {2, -1}}};

}  // namespace rv

int rv_cdef_filter_frame_dev(const rv_plane src[3], const rv_plane dst[3], int width, int height,
                             const uint8_t *d_skip, int mi_stride, const uint8_t *d_dir,
                             const int32_t *d_var, const uint8_t *d_cdef_index,
                             const uint8_t *y_strengths, const uint8_t *uv_strengths, int damping,
                             int bit_depth, hipStream_t s);

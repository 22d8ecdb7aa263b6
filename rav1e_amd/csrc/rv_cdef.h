// rv_cdef.h -- internal: rv_cdef.hip's device-resident frame filter (all three
// planes in one launch; the replay's F7).
#pragma once
#include "rv_device.h"

int rv_cdef_filter_frame_dev(const rv_plane src[3], const rv_plane dst[3], int width, int height,
                             const uint8_t *d_skip, int mi_stride, const uint8_t *d_dir,
                             const int32_t *d_var, const uint8_t *d_cdef_index,
                             const uint8_t *y_strengths, const uint8_t *uv_strengths, int damping,
                             int bit_depth, hipStream_t s);

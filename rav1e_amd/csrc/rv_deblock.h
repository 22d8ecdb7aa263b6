// rv_deblock.h -- internal: rv_deblock.hip's device-resident entry points
// (the block map and the levels stay in device memory; the replay's F7).
#pragma once
#include "rv_device.h"

int rv_deblock_plane_dev(const rv_plane *p, int pli, int width, int height, const uint8_t *d_lg,
                         const uint8_t *d_skip, int mi_stride, const uint8_t levels[4],
                         int bit_depth, hipStream_t s);
int rv_deblock_sse_dev(const rv_plane rec[3], const rv_plane src[3], int width, int height,
                       const uint8_t *d_lg, const uint8_t *d_skip, int mi_stride,
                       int64_t *d_tally, uint8_t *d_levels, int bit_depth, hipStream_t s);
int rv_deblock_frame_dev(const rv_plane planes[3], int width, int height, const uint8_t *d_lg,
                         const uint8_t *d_skip, int mi_stride, const uint8_t *d_levels,
                         int bit_depth, hipStream_t s, const uint8_t *levels);

// rv_frame.h -- internal: rv_frame.hip's frame-level helpers the replay calls
// (padding of a whole frame, the input pyramid, synthetic inputs).
#pragma once
#include "rv_device.h"

int rv_frame_pad_dev(const rv_plane dst[3], const rv_plane *src, hipStream_t s);
int rv_plane_pyramid(const rv_plane *y, const rv_plane *h, const rv_plane *q, void *stream);
int rv_synth_frame(const rv_plane *y, const rv_plane *u, const rv_plane *v, int t, int bit_depth,
                   void *stream);

// rv_scenecut.hip -- the whole-frame |a - b| sums of the scene-change
// detector: what has_scenecut (src/scenechange/mod.rs:167-207) folds over
// Frame::iter() (PixelIter, src/frame/mod.rs:126-172), before its division,
// for every pair of a window of frames in one pass over the pixels.
//
// PixelIter walks the luma positions (x, y) of [0, w) x [0, h), reads plane k
// at (x >> xdec, y >> ydec) and stops before the last position (w - 1,
// h - 1).  Per plane that is a weighted sum over the plane's own pixels: a
// pixel (cx, cy) counts min(1 << xdec, w - (cx << xdec)) * min(1 << ydec,
// h - (cy << ydec)) times, the last pixel of the plane one time less.  Every
// column but the last has the weight WX = 1 << xdec and every row but the
// last WY = 1 << ydec, so the kernel needs four integers (wx, wx_last, wy,
// wy_last) and the luma plane is the case 1, 1, 1, 1.
//
// A row is cut into runs of 16 bytes (16 pixels at 8 bit, 8 above).  The
// runs of a plane, in row-major order, are dealt to the workgroups in equal
// contiguous spans (bands of rows, cut at run granularity so that no
// workgroup gets a short band).  A lane loads the run at its position from
// every frame of the window -- each frame's pixels are read once per call --
// and then accumulates every requested pair out of those registers with
// v_sad_u8 / v_sad_u16.  The accumulators are one per unordered pair of the
// window (28 for 8 frames) and statically indexed; a uniform bit mask says
// which of them the call asked for, and (b, a), repeats and a == b cost
// nothing extra.  The last run of a row goes through a masked path where it
// is short, where its last pixel has another weight, or where that pixel is
// the one PixelIter drops: pixels are then loaded one by one and nothing
// outside the visible area is touched.
//
// Lane accumulators are u32 (a lane sees at most kDeltaMaxIters runs: 1024 * 8 *
// 65535 * 4 < 2^32 for any u16 content, less at 8 bit); the sum over the
// wavefront, over the workgroup's wavefronts (LDS) and over the workgroups is
// u64.  A workgroup stores its partial sums into a slab [plane][workgroup]
// [slot]; a second, one-workgroup kernel adds them up per (pair, plane) and
// writes d_sums.  The first version added them with one atomicAdd per
// workgroup, pair and plane into a zeroed d_sums: 1024 workgroups queueing
// on the same few cache lines cost 5 us of a 26 us luma call and 45 of 96 us
// with three planes and nine pairs.  The slab belongs
// to the calling thread and the stream, so calls on one stream reuse it in
// order.
#include <stdio.h>

#include <vector>

#include "rv_device.h"

namespace rv {

constexpr int kDeltaThreads = 256;
constexpr int kDeltaSlots = RV_DELTA_MAX_FRAMES * (RV_DELTA_MAX_FRAMES - 1) / 2;
constexpr int kDeltaMaxWgs = 512;  // two workgroups per CU
constexpr int kDeltaMaxIters = 1024;

// Plane k of every frame of the window.
struct DeltaPlane {
  const void *base[RV_DELTA_MAX_FRAMES];  // pixel (0, 0) of the visible area
  int32_t stride[RV_DELTA_MAX_FRAMES];    // in pixels
  int32_t w, h;                           // the plane's visible size
  int32_t wx, wxl, wy, wyl;               // weights: columns / last column, rows / last row
  uint32_t rpr;                           // runs per row
  uint32_t n_runs;                        // rpr * h
  uint32_t n_wgs, iters;                  // workgroups of this plane, runs per lane
};

struct DeltaCall {
  int32_t n_frames, n_pairs, n_planes;  // n_planes: row pitch of d_sums
  int32_t plane0;                       // plane index of blockIdx.y == 0
  uint32_t slab_wgs;                    // workgroup pitch of the slab
  uint32_t mask;                        // requested slots
  uint8_t slot[RV_DELTA_MAX_PAIRS];     // slot of pair p, 255 for a == b
};

template <int N>
struct DeltaPlanes {
  DeltaPlane p[N];
};

// Slot of the unordered pair a < b: the order of the kernel's unrolled loops.
static int delta_slot(int a, int b) {
  int s = 0;
  for (int i = 0; i < RV_DELTA_MAX_FRAMES; i++)
    for (int j = i + 1; j < RV_DELTA_MAX_FRAMES; j++, s++)
      if (i == a && j == b) return s;
  return -1;
}

template <typename Px>
__device__ __forceinline__ uint32_t delta_sad(uint32_t a, uint32_t b, uint32_t acc) {
  if constexpr (sizeof(Px) == 1)
    return __builtin_amdgcn_sad_u8(a, b, acc);
  else
    return __builtin_amdgcn_sad_u16(a, b, acc);
}

// acc[slot] += wgt * sum |v[a] - v[b]| over the 16 bytes, for the requested
// slots.  W == false: wgt is 1.
template <typename Px, bool W>
__device__ __forceinline__ void delta_accumulate(const uint4 (&v)[RV_DELTA_MAX_FRAMES],
                                                 uint32_t mask, uint32_t wgt,
                                                 uint32_t (&acc)[kDeltaSlots]) {
  int s = 0;
#pragma unroll
  for (int a = 0; a < RV_DELTA_MAX_FRAMES; a++) {
#pragma unroll
    for (int b = a + 1; b < RV_DELTA_MAX_FRAMES; b++, s++) {
      if ((mask >> s) & 1) {  // uniform
        uint32_t r = W ? 0u : acc[s];
        r = delta_sad<Px>(v[a].x, v[b].x, r);
        r = delta_sad<Px>(v[a].y, v[b].y, r);
        r = delta_sad<Px>(v[a].z, v[b].z, r);
        r = delta_sad<Px>(v[a].w, v[b].w, r);
        acc[s] = W ? acc[s] + r * wgt : r;
      }
    }
  }
}

// The first n (< 16 / sizeof(Px), possibly 0) pixels at p, the rest 0: one
// load per pixel, none past p[n - 1].
template <typename Px>
__device__ __forceinline__ uint4 delta_load_masked(const Px *p, int n) {
  constexpr int PPR = 16 / (int)sizeof(Px), PPD = 4 / (int)sizeof(Px);
  uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < PPR; i++) {
    const uint32_t px = i < n ? (uint32_t)p[i] : 0u;
    d[i / PPD] |= px << (8 * (int)sizeof(Px) * (i % PPD));
  }
  return make_uint4(d[0], d[1], d[2], d[3]);
}

template <typename Px, bool W, int NP>
__global__ __launch_bounds__(kDeltaThreads) void frame_delta_kernel(DeltaPlanes<NP> planes,
                                                                    DeltaCall c,
                                                                    unsigned long long *slab) {
  constexpr int PPR = 16 / (int)sizeof(Px);
  const DeltaPlane &P = planes.p[NP == 1 ? 0 : blockIdx.y];
  if (blockIdx.x >= P.n_wgs) return;
  __shared__ unsigned long long part[kDeltaThreads / RV_WAVE][kDeltaSlots];
  const int tid = threadIdx.x;

  uint32_t acc[kDeltaSlots];
#pragma unroll
  for (int s = 0; s < kDeltaSlots; s++) acc[s] = 0;

  const uint32_t span = P.iters * kDeltaThreads;
  const uint32_t first = blockIdx.x * span;
#pragma unroll 1
  for (uint32_t it = 0; it < P.iters; it++) {
    const uint32_t idx = first + it * kDeltaThreads + tid;
    if (idx >= P.n_runs) break;  // the runs of a lane ascend: nothing after this one
    const uint32_t row = idx / P.rpr, run = idx - row * P.rpr;
    const int x0 = (int)run * PPR;
    const int nv = min(PPR, P.w - x0);  // pixels of the run inside the row: >= 1
    const bool last_run = run == P.rpr - 1, last_row = (int)row == P.h - 1;
    const uint32_t wy = last_row ? P.wyl : P.wy;
    // W: the last pixel of a row apart where the run is short, where its
    // weight differs or where PixelIter drops one visit of it; else: only
    // the short run and the dropped pixel matter
    const bool apart = W && last_run && (nv < PPR || last_row || P.wxl != P.wx);
    const int nreg = W ? nv - (apart ? 1 : 0) : nv - (last_run && last_row ? 1 : 0);

    uint4 v[RV_DELTA_MAX_FRAMES];
#pragma unroll
    for (int f = 0; f < RV_DELTA_MAX_FRAMES; f++) v[f] = make_uint4(0, 0, 0, 0);
    if (nreg == PPR) {
#pragma unroll
      for (int f = 0; f < RV_DELTA_MAX_FRAMES; f++)
        if (f < c.n_frames) {  // uniform
          const Px *p = (const Px *)P.base[f] + (int64_t)row * P.stride[f] + x0;
          __builtin_memcpy(&v[f], p, 16);  // rows of foreign planes need not be 16-byte aligned
        }
    } else {
#pragma unroll
      for (int f = 0; f < RV_DELTA_MAX_FRAMES; f++)
        if (f < c.n_frames)
          v[f] = delta_load_masked<Px>((const Px *)P.base[f] + (int64_t)row * P.stride[f] + x0,
                                       nreg);
    }
    delta_accumulate<Px, W>(v, c.mask, P.wx * wy, acc);
    if constexpr (W) {
      if (apart) {
        const uint32_t wl = P.wxl * wy - (last_row ? 1u : 0u);
#pragma unroll
        for (int f = 0; f < RV_DELTA_MAX_FRAMES; f++)
          if (f < c.n_frames)
            v[f] = make_uint4(
                ((const Px *)P.base[f])[(int64_t)row * P.stride[f] + x0 + nv - 1], 0, 0, 0);
        delta_accumulate<Px, true>(v, c.mask, wl, acc);
      }
    }
  }

  // wavefront, then workgroup, then this workgroup's row of the slab
  const int wave = tid / RV_WAVE, lane = tid % RV_WAVE;
#pragma unroll
  for (int s = 0; s < kDeltaSlots; s++) {
    if ((c.mask >> s) & 1) {
      const unsigned long long t = group_sum<RV_WAVE, unsigned long long>(acc[s]);
      if (lane == 0) part[wave][s] = t;
    }
  }
  __syncthreads();
  if (tid < kDeltaSlots && ((c.mask >> tid) & 1)) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < kDeltaThreads / RV_WAVE; w++) t += part[w][tid];
    const uint32_t plane = c.plane0 + (NP == 1 ? 0 : blockIdx.y);
    slab[((size_t)plane * c.slab_wgs + blockIdx.x) * kDeltaSlots + tid] = t;
  }
}

struct DeltaFinish {
  uint32_t n_wgs[3];
};

// d_sums[p][k] = the sum over plane k's workgroups of the slab entries of
// pair p's slot (0 for a == b): one wavefront per output, no atomics.
__global__ __launch_bounds__(kDeltaThreads) void frame_delta_finish_kernel(
    DeltaCall c, DeltaFinish f, const unsigned long long *slab, unsigned long long *sums) {
  const int wave = threadIdx.x / RV_WAVE, lane = threadIdx.x % RV_WAVE;
  for (int o = wave; o < c.n_pairs * c.n_planes; o += kDeltaThreads / RV_WAVE) {
    const int p = o / c.n_planes, k = o - p * c.n_planes;
    const uint32_t slot = c.slot[p];
    unsigned long long t = 0;
    if (slot != 255)
      for (uint32_t g = lane; g < f.n_wgs[k]; g += RV_WAVE)
        t += slab[((size_t)k * c.slab_wgs + g) * kDeltaSlots + slot];
    t = group_sum<RV_WAVE, unsigned long long>(t);
    if (lane == 0) sums[o] = t;
  }
}

// The slab of the calling thread for (device, stream): grown on demand, kept.
static unsigned long long *delta_slab(hipStream_t s, size_t bytes) {
  struct Slab {
    int device;
    hipStream_t stream;
    void *ptr;
    size_t bytes;
  };
  static thread_local std::vector<Slab> slabs;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return nullptr;
  Slab *e = nullptr;
  for (Slab &x : slabs)
    if (x.device == device && x.stream == s) e = &x;
  if (!e) {
    slabs.push_back({device, s, nullptr, 0});
    e = &slabs.back();
  }
  if (e->bytes < bytes) {
    if (e->ptr) (void)hipFree(e->ptr);  // waits for the work that still reads it
    e->ptr = nullptr;
    e->bytes = 0;
    if (hipMalloc(&e->ptr, bytes) != hipSuccess) return nullptr;
    e->bytes = bytes;
  }
  return (unsigned long long *)e->ptr;
}

// Fills the plane-k entry of the window, or says why not.
static const char *delta_plane_setup(const rv_plane *frames, int n_frames, int n_planes, int k,
                                     DeltaPlane *P) {
  const rv_plane &f0 = frames[k];
  const int B = f0.hbd ? 2 : 1, ppr = 16 / B;
  const int lw = frames[0].width, lh = frames[0].height;
  for (int f = 0; f < n_frames; f++) {
    const rv_plane &p = frames[f * n_planes + k];
    if (p.hbd != frames[0].hbd || p.width != f0.width || p.height != f0.height ||
        p.xdec != f0.xdec || p.ydec != f0.ydec)
      return "the frames differ in hbd, size or decimation";
    if (!p.data) return "a plane has no data";
    if (p.xorigin < 0 || p.yorigin < 0 || p.stride < p.xorigin + p.width ||
        p.alloc_height < p.yorigin + p.height)
      return "a plane's visible area leaves its allocation";
    P->base[f] = (const uint8_t *)p.data + plane_origin_index(p) * B;
    P->stride[f] = p.stride;
  }
  for (int f = n_frames; f < RV_DELTA_MAX_FRAMES; f++) {
    P->base[f] = nullptr;
    P->stride[f] = 0;
  }
  P->w = f0.width;
  P->h = f0.height;
  P->wx = 1 << f0.xdec;
  P->wy = 1 << f0.ydec;
  P->wxl = lw - ((f0.width - 1) << f0.xdec);
  P->wyl = lh - ((f0.height - 1) << f0.ydec);
  const int64_t rpr = (f0.width + ppr - 1) / ppr, n_runs = rpr * f0.height;
  if (n_runs >= ((int64_t)1 << 31)) return "a plane is too large";
  int64_t wgs = (n_runs + kDeltaThreads - 1) / kDeltaThreads;
  if (wgs > kDeltaMaxWgs) wgs = kDeltaMaxWgs;
  int64_t iters = (n_runs + wgs * kDeltaThreads - 1) / (wgs * kDeltaThreads);
  if (iters > kDeltaMaxIters) {  // the u32 lane accumulators
    iters = kDeltaMaxIters;
    wgs = (n_runs + iters * kDeltaThreads - 1) / (iters * kDeltaThreads);
  }
  P->rpr = (uint32_t)rpr;
  P->n_runs = (uint32_t)n_runs;
  P->n_wgs = (uint32_t)wgs;
  P->iters = (uint32_t)iters;
  return nullptr;
}

template <typename Px, bool W, int NP>
static void delta_launch(const DeltaPlane *P, const DeltaCall &c, unsigned long long *slab,
                         hipStream_t s) {
  DeltaPlanes<NP> planes;
  uint32_t wgs = 0;
  for (int i = 0; i < NP; i++) {
    planes.p[i] = P[i];
    wgs = P[i].n_wgs > wgs ? P[i].n_wgs : wgs;
  }
  frame_delta_kernel<Px, W, NP><<<dim3(wgs, NP), kDeltaThreads, 0, s>>>(planes, c, slab);
}

template <typename Px>
static void delta_launch_all(const DeltaPlane *P, DeltaCall c, bool weighted,
                             unsigned long long *slab, uint64_t *d_sums, hipStream_t s) {
  c.plane0 = 0;
  if (c.n_planes == 1) {
    delta_launch<Px, false, 1>(P, c, slab, s);
  } else if (!weighted) {  // 4:4:4: three planes of the luma kind
    delta_launch<Px, false, 3>(P, c, slab, s);
  } else {
    delta_launch<Px, false, 1>(P, c, slab, s);
    c.plane0 = 1;
    delta_launch<Px, true, 2>(P + 1, c, slab, s);
  }
  DeltaFinish f = {};
  for (int k = 0; k < c.n_planes; k++) f.n_wgs[k] = P[k].n_wgs;
  frame_delta_finish_kernel<<<1, kDeltaThreads, 0, s>>>(c, f, slab,
                                                        (unsigned long long *)d_sums);
}

}  // namespace rv

using namespace rv;

extern "C" int rv_frame_delta_batch(const rv_plane *frames, int n_frames, int n_planes,
                                    const rv_delta_pair *pairs, int n_pairs, uint64_t *d_sums,
                                    void *stream) {
  if (n_frames < 2 || n_frames > RV_DELTA_MAX_FRAMES)
    return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: n_frames outside 2 .. 8");
  if (n_pairs < 1 || n_pairs > RV_DELTA_MAX_PAIRS)
    return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: n_pairs outside 1 .. 16");
  if (n_planes != 1 && n_planes != 3)
    return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: n_planes is 1 or 3");
  if (!frames || !pairs)
    return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: null frames or pairs");
  DeltaCall c = {};
  c.n_frames = n_frames;
  c.n_pairs = n_pairs;
  c.n_planes = n_planes;
  for (int p = 0; p < n_pairs; p++) {
    const int a = pairs[p].a, b = pairs[p].b;
    if (a < 0 || a >= n_frames || b < 0 || b >= n_frames)
      return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: a pair index is out of range");
    c.slot[p] = a == b ? 255 : (uint8_t)delta_slot(a < b ? a : b, a < b ? b : a);
    if (a != b) c.mask |= 1u << c.slot[p];
  }
  const rv_plane &luma = frames[0];
  if (luma.width < 1 || luma.height < 1 || luma.xdec != 0 || luma.ydec != 0)
    return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: plane 0 is no luma plane");
  bool weighted = false;
  for (int k = 1; k < n_planes; k++) {
    const rv_plane &ch = frames[k];
    if (!((ch.xdec == 0 && ch.ydec == 0) || (ch.xdec == 1 && (ch.ydec == 0 || ch.ydec == 1))) ||
        ch.xdec != frames[1].xdec || ch.ydec != frames[1].ydec)
      return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: chroma must be 4:4:4, 4:2:2 or 4:2:0");
    if (ch.width != (luma.width + ch.xdec) >> ch.xdec ||
        ch.height != (luma.height + ch.ydec) >> ch.ydec)
      return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: a chroma plane's size is not the "
                                     "luma size rounded up by its decimation");
    weighted = ch.xdec != 0;
  }
  DeltaPlane P[3];
  for (int k = 0; k < n_planes; k++) {
    const char *why = delta_plane_setup(frames, n_frames, n_planes, k, &P[k]);
    if (why) {
      char msg[160];  // rv_set_error copies it
      snprintf(msg, sizeof(msg), "rv_frame_delta_batch: %s", why);
      return rv_set_error(RV_EINVAL, msg);
    }
  }
  if (!d_sums) return rv_set_error(RV_EINVAL, "rv_frame_delta_batch: null d_sums");
  hipStream_t s = rv_resolve_stream(stream);
  if (c.mask == 0) {  // only a == b pairs: zeros are the answer
    hipError_t e = hipMemsetAsync(d_sums, 0, sizeof(uint64_t) * n_pairs * n_planes, s);
    if (e != hipSuccess) return rv_set_hip_error(e, __func__);
    return RV_OK;
  }
  for (int k = 0; k < n_planes; k++) c.slab_wgs = P[k].n_wgs > c.slab_wgs ? P[k].n_wgs : c.slab_wgs;
  unsigned long long *slab =
      delta_slab(s, sizeof(uint64_t) * kDeltaSlots * c.slab_wgs * (size_t)n_planes);
  if (!slab) return rv_set_error(RV_EHIP, "rv_frame_delta_batch: no memory for the partial sums");
  if (luma.hbd)
    delta_launch_all<uint16_t>(P, c, weighted, slab, d_sums, s);
  else
    delta_launch_all<uint8_t>(P, c, weighted, slab, d_sums, s);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

// rv_me.h -- internal: the multi-reference motion searches of rv_me.hip and
// rv_me_diamond.hip as the replay launches them: every reference in one
// launch, per-job evaluation counts, winners chained into the next stage's
// jobs.
#pragma once
#include "rv_chain.h"
#include "rv_device.h"

namespace rv {
// get_mv_rate's diff_to_rate (src/me.rs:1006-1021), shared by the diamond
// searches of rv_me_diamond.hip and rv_motion_est.hip
__device__ __forceinline__ uint32_t ds_diff_to_rate(int16_t diff, int hp) {
  int16_t d = hp ? diff : (int16_t)(diff >> 1);
  if (d == 0) return 0;
  uint32_t a = (uint16_t)(d < 0 ? -d : d);
  return 2u * (16u - (uint32_t)(__builtin_clz(a) - 16));
}
}  // namespace rv

// rv_me.hip
int rv_full_search_multi(const rv_plane *org, const rv_plane *refs, int n_refs,
                         const rv_fs_job *d_jobs, int n_per_ref, int blk_w, int blk_h,
                         int step, int allow_hp, rv_fs_result *d_out, const rv::ChainNext *next,
                         const uint32_t *const *box, void *stream);
// rv_me_diamond.hip
int rv_diamond_search_multi(const rv_plane *org, const rv_plane *refs, int n_refs,
                            const rv_ds_job *d_jobs, int n_per_ref, int blk_w, int blk_h,
                            int subpixel, int use_satd, int allow_hp, int bit_depth,
                            rv_fs_result *d_out, uint32_t *d_evals, const rv::ChainNext *next,
                            void *stream, const uint8_t *active = nullptr,
                            const int32_t *alist = nullptr, const int32_t *acount = nullptr,
                            int lper = 1, const uint8_t *dirty = nullptr, int list_grid = 0,
                            uint32_t *eval_acc = nullptr, unsigned long long *t01 = nullptr);
int rv_diamond_f2_f3(const rv_plane *org_h, const rv_plane *refs_h, const rv_ds_job *jobs_h,
                     rv_fs_result *out_h, const uint8_t *dirty_h, const rv_plane *org,
                     const rv_plane *refs, const rv_ds_job *jobs, rv_fs_result *out,
                     const uint8_t *dirty, const rv::ChainNext *next, int n_refs, int n_per_ref,
                     int bit_depth, const int32_t *alist, const int32_t *acount, int list_grid,
                     void *stream, const rv_ds_job *jobs_sub = nullptr,
                     rv_fs_result *out_sub = nullptr, uint32_t *eval_acc = nullptr,
                     unsigned long long *t01 = nullptr);

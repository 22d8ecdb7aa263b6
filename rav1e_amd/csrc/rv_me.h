// rv_me.h -- internal: the multi-reference motion searches of rv_me.hip and
// rv_me_diamond.hip as the replay launches them: every reference in one
// launch, per-job evaluation counts, winners chained into the next stage's
// jobs.
#pragma once
#include "rv_chain.h"
#include "rv_device.h"

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

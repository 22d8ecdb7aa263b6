// rv_ec_mode.hip -- the block mode-info symbols: a device tokenizer for what a
// block codes ahead of its coefficients (encode_block_pre_cdef and the symbol
// part of encode_block_post_cdef, src/encoder.rs:1446-1662) and for
// write_partition (src/context.rs:2059-2109).
//
// The split is rv_ec.hip's.  Every context these symbols use comes from the
// block's own fields and from the blocks directly above and left of it in
// the same tile (skip_context, intra_inter_context, get_cdf_intra_mode_kf,
// fill_neighbours_ref_counts, get_comp_mode_ctx, get_comp_ref_type_ctx,
// get_segment_pred also from the above-left one; partition_plane_context from
// the partition-context bytes the above / left leaves stored).  Those
// neighbours are final before the block is coded (z-order never revisits
// them), so one launch scatters every leaf's neighbour record into a per-tile
// map and a second forms every job's symbols.  The range coder and the CDF
// adaptation stay on the host (rv_ec_code_stream / rv_ec_count_stream).
//
// Map: one u32 per 8x8 luma cell (the smallest block in scope):
//   bit 0 skip, bits 1-5 luma mode, 6-9 ref_frames[0], 10-13 ref_frames[1],
//   14-16 segmentation_idx, 17-21 the partition-context byte
//   (partition_context_lookup of a square size: above == left ==
//   (31 << (log2 size - 2)) & 31).  A cleared cell is Block::default with zero
// partition context.  Only a leaf's bottom row and right column are ever read,
// so only they are stored.  A tile's top row and left column read zero:
// BlockContext::new, and reset_left_contexts at every superblock row.
//
// Tokens are rv_ec.hip's over the combined table (rv_ec_mode_tables.h), the
// token's length being the length of the slice the reference passes
// (write_partition at 8x8: 5, write_intra_uv_mode without CfL: 14), plus the
// frame-edge partition symbol (format in rv_ec.h).
//
// Restrictions (a job outside them emits no tokens, stores no record and adds
// 1 to d_status[2]; nothing out of range is used as an index; the blocks next
// to a rejected leaf read a cleared cell in its place):
//  * square blocks BLOCK_8X8 .. BLOCK_64X64 aligned to their size, top-left
//    inside the tile; tile cols / rows even and within the map;
//  * partition nodes PARTITION_NONE or PARTITION_SPLIT (the edge forms SPLIT
//    only, above 8x8: the reference's assert!s);
//  * no tx_mode_select (write_tx_size_intra), no filter-intra, no block
//    deblock deltas, no write_cdef / write_lrf;
//  * modes, refs, segment ids, CfL numbers, mode_context and MV differences in
//    the ranges the reference can code (its array bounds and assert!s): inter
//    blocks on INTER frames only, compound blocks bidirectional (LAST..GOLDEN
//    with BWDREF..ALTREF) and only when reference_mode is not SINGLE,
//    NEW_NEWMV with >= 2 stack entries, a NEAR mode with its stack entry.
//  * write_segmentation stores its *prediction* into a skip block
//    (src/context.rs:3541-3543) and later neighbours read it: a raster-order
//    chain the kernel does not resolve.  seg_idx is read as given; the job list
//    must hold what the reference would have stored (the Python mirror's
//    resolve_skip_segments; the identity when every block is in segment 0).
#include "rv_device.h"
#include "rv_ec.h"
#include "rv_ec_mode_sym.h"

namespace rv {

// Launch 1, one lane per job: the leaf's record into the bottom row and the
// right column of its cells (inside the map), and the job's token count.
__global__ __launch_bounds__(256) void mode_prep_kernel(ModeArgs a, uint32_t *map) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const rv_ec_mode_job j = a.jobs[i];
  int cols, rows;
  if (!mode_job_ok(j, a, cols, rows)) {
    a.count[i] = 0;
    atomicAdd(a.status + 2, 1u);
    return;
  }
  if (j.kind == 0) {
    const int lg = bsize_lg(j.bsize), n8 = 1 << (lg - 3);
    const uint32_t rec = (uint32_t)j.skip | (uint32_t)j.luma_mode << 1 | (uint32_t)j.ref[0] << 6 |
                         (uint32_t)j.ref[1] << 10 | (uint32_t)j.seg_idx << 14 |
                         ((31u << (lg - 2)) & 31u) << 17;
    uint32_t *m = map + (size_t)j.tile * a.map_w8 * a.map_h8;
    const int x8 = j.bx >> 1, y8 = j.by >> 1;
    const int xe = min(x8 + n8, a.map_w8), ye = min(y8 + n8, a.map_h8);
    if (y8 + n8 - 1 < a.map_h8)
      for (int x = x8; x < xe; x++) m[(size_t)(y8 + n8 - 1) * a.map_w8 + x] = rec;
    if (x8 + n8 - 1 < a.map_w8)
      for (int y = y8; y < ye; y++) m[(size_t)y * a.map_w8 + x8 + n8 - 1] = rec;
  }
  CountSink c;
  mode_symbols(j, a, cols, rows, c);
  a.count[i] = c.n;
}

// Launch 2, one lane per job: its symbols from its token offset.
__global__ __launch_bounds__(256) void mode_token_kernel(ModeArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.count[i + 1] == a.count[i]) return;  // a rejected job or a silent partition node
  const rv_ec_mode_job j = a.jobs[i];
  int cols, rows;
  if (!mode_job_ok(j, a, cols, rows)) return;
  WriteSink w{a.tokens, a.count[i], a.cap, a.status};
  mode_symbols(j, a, cols, rows, w);
}

}  // namespace rv

using namespace rv;

extern "C" {

size_t rv_ec_mode_scratch_bytes(int n_jobs) {
  return (((size_t)(n_jobs < 0 ? 0 : n_jobs) + 1023) / 1024 + 1) * 4 + 16;
}

int rv_ec_mode_tokenize(const rv_ec_mode_job *d_jobs, int n, rv_ec_mode_params params, int n_tiles,
                        const int32_t *d_tile_dims, int map_w8, int map_h8, uint32_t *d_map,
                        void *d_scratch, uint32_t *d_offsets, uint32_t *d_tokens,
                        uint32_t token_cap, uint32_t *d_status, void *stream) {
  if (n < 0 || n > 1024 * 1024 || n_tiles < 1 || n_tiles > 1024 || map_w8 < 1 || map_h8 < 1 ||
      map_w8 > 8192 || map_h8 > 8192 || !d_tile_dims || !d_map || !d_scratch || !d_offsets ||
      !d_status || (token_cap && !d_tokens) || (n && !d_jobs))
    return rv_set_error(RV_EINVAL, "rv_ec_mode_tokenize: bad arguments");
  hipStream_t st = rv_resolve_stream(stream);
  if (hipMemsetAsync(d_status, 0, 12, st) != hipSuccess ||
      hipMemsetAsync(d_map, 0, (size_t)n_tiles * map_w8 * map_h8 * 4, st) != hipSuccess)
    return rv_set_error(RV_EHIP, "rv_ec_mode_tokenize: clear");
  if (n == 0) {
    if (hipMemsetAsync(d_offsets, 0, 4, st) != hipSuccess)
      return rv_set_error(RV_EHIP, "rv_ec_mode_tokenize: offsets");
    return RV_OK;
  }
  ModeArgs a;
  a.jobs = d_jobs;
  a.n = n;
  a.prm = params;
  a.n_tiles = n_tiles;
  a.tile_dims = d_tile_dims;
  a.map = d_map;
  a.map_w8 = map_w8;
  a.map_h8 = map_h8;
  a.count = d_offsets;
  a.tokens = d_tokens;
  a.cap = token_cap;
  a.status = d_status;
  const int grid = (n + 255) / 256;
  mode_prep_kernel<<<grid, 256, 0, st>>>(a, d_map);
  ec_scan(d_offsets, n, nullptr, (uint32_t *)d_scratch, d_status, st);
  mode_token_kernel<<<grid, 256, 0, st>>>(a);
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

}  // extern "C"

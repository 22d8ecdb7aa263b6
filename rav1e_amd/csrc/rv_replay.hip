// rv_replay.hip -- hot-path replay driver: the per-frame call structure of a
// speed-10 encode of a stream, for the stages this library accelerates, with
// every frame resident in HBM.  Per coded frame:
//
//   F0  hres / qres of the input (encode_frame, src/encoder.rs:3382-3385)
//   F1  coarse ME: full_search at 1/4 res, 16x16 per 64x64 superblock and
//       reference (estimate_motion_ss4, src/me.rs:1023-1075)
//   F2  half-res diamond, 32x32 (me_ss2, src/me.rs:287-519)
//   F3  full-res full-pel diamond then sub-pel diamond, 64x64
//       (motion_estimation, src/me.rs:193-285)
//   F4  RDO: every inter candidate of rdo_mode_decision (src/rdo.rs:825-1006:
//       NEARESTMV / NEAR0MV / GLOBALMV / NEWMV per reference), skip and
//       non-skip (luma_chroma_mode_rdo, :649-700): put_8tap, diff + fht,
//       quantize + dequantize, estimate_rate, inverse + add,
//       compute_distortion (rv_rdo.hip); then compute_rd_cost and the
//       per-superblock argmin in rav1e's candidate order
//   F6  commit: the winner of every superblock re-runs its chain and writes
//       its levels and its reconstruction into the frame
//   F5  8x8 importance SATD against reference 0 (compute_block_importances,
//       src/api/internal.rs:823-1010) + lookahead intra cost (:680-765)
//   F7  the reconstruction becomes a reference: pad (single tile group), or
//       pack the group's region, all-gather it over RCCL, unpack every other
//       group's region and pad (tile-parallel multi-GPU, src/encoder.rs:
//       2772-2781, 3411-3429)
//
// Frames run in the coding order of rav1e's reorder pyramid (src/api/
// internal.rs:40-95; group_input_len 4): display 4g+4, 4g+2, 4g+1, 4g+3 at
// me_range_scale 4, 2, 1, 1 (src/encoder.rs:838), each referencing the
// reconstructions its pyramid level sees.  Display frame 0 is the key frame:
// intra coding is out of scope, its input is taken as its reconstruction.
// The CPU replay (oracle/orc_replay.c) runs the same schedule and must
// produce the same result words.
//
// This file: the instance (create / destroy / twin), the static job tables,
// setters and getters, the tile-group copy and the loop filters of a slot,
// the results and the timing / probe / counter read-outs, the RCCL
// communicator.  rv_replay_frame.hip: one coded frame.  rv_replay_la.hip: the
// lookahead and its engine.  rv_replay.h: what the three share.
#include "rv_replay.h"

namespace rv {

// Verification checksum of the committed levels (results time, not per
// frame): sum of q * (position in block + 1), wrapping u64.
__global__ void coeff_checksum(const int32_t *packed, int64_t total, int per_block,
                               unsigned long long *out) {
  uint64_t s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x)
    s += (uint64_t)(int64_t)packed[i] * (uint64_t)(i % per_block + 1);
  block_atomic_add(s, out);
}

// Sum of the visible pixels of a rectangle of a plane (results time).
template <typename Px>
__global__ void sum_rect(rv_plane p, int x0, int y0, int w, int h, unsigned long long *out) {
  uint64_t s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)w * h;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    s += *plane_ptr<Px>(p, x0 + x, y0 + y);
  }
  block_atomic_add(s, out);
}

// F7 exchange: the kernel behind xcopy (XRect: rv_replay.h).  blockIdx.y = rectangle.
struct XArgs {
  rv_plane pl[3];
  XRect rect[3 * kMaxGroups];  // pixel rectangles (or block-map ones, bytewise)
  int n;
  int to_plane;  // 1: buffer -> planes (unpack), 0: planes -> buffer (pack)
  uint8_t *buf;
};
template <typename Px>
__global__ __launch_bounds__(256) void xcopy_kernel(XArgs a) {
  const XRect &r = a.rect[blockIdx.y];
  const int64_t n = (int64_t)r.w * r.h;
  Px *b = reinterpret_cast<Px *>(a.buf + r.off);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int y = (int)(i / r.w), x = (int)(i - (int64_t)y * r.w);
    Px *p = plane_ptr_mut<Px>(a.pl[r.plane], r.x0 + x, r.y0 + y);
    if (a.to_plane)
      *p = b[i];
    else
      b[i] = *p;
  }
}

// Levels checksum over the committed blocks of a list: sum of q *
// (position in its transform block + 1), wrapping u64.
__global__ void coeff_checksum_list(const int32_t *packed, const int32_t *list,
                                    const int32_t *count, int per, int wmod,
                                    unsigned long long *out) {
  const int64_t total = (int64_t)*count * per;
  uint64_t s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = i / per;
    const int e = (int)(i - j * per);
    s += (uint64_t)(int64_t)packed[(int64_t)list[j] * per + e] * (uint64_t)(e % wmod + 1);
  }
  block_atomic_add(s, out);
}

}  // namespace rv

// ---- EcHost (stage F8's host side) ---------------------------------------------
void EcHost::code(const Item &it) {
  const uint32_t *st = stat_h[it.slot];
  if (st[1]) {  // tokens past the buffer were dropped
    err = RV_EINVAL;
    return;
  }
  const int total = rv_ec_cdf_total();
  std::vector<uint16_t> init(total), cdf(total), best_cdf(total);
  if (chain[it.level].empty())
    rv_ec_default_cdf(it.qctx, init.data());
  else
    init = chain[it.level];
  uint64_t h = 1469598103934665603ull, bytes = 0;
  long best = -1;
  std::vector<uint8_t> out;
  for (int t = 0; t < ntiles; t++) {
    const uint32_t a = st[3 + t], b = st[3 + t + 1];
    cdf = init;
    out.resize(2 * (size_t)(b - a) + 64);
    const long nb = rv_ec_code_tokens(tok_h[it.slot] + a, b - a, cdf.data(), out.data(), out.size());
    if (nb < 0 || (size_t)nb > out.size()) {
      err = RV_EINVAL;
      return;
    }
    for (long i = 0; i < nb; i++) h = (h ^ out[i]) * 1099511628211ull;
    bytes += (uint64_t)nb;
    if (nb >= best) {  // Iterator::max_by_key keeps the last maximum
      best = nb;
      best_cdf = cdf;
    }
  }
  rv_ec_reset_counts(best_cdf.data());
  chain[it.level] = best_cdf;
  stat[0] = bytes;
  stat[1] = (uint64_t)ntiles;
  stat[2] = h;
  stat[3]++;
  stat[4] += bytes;
}
void EcHost::run() {
  for (;;) {
    Item it;
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return stop || !q.empty(); });
      if (q.empty()) return;
      it = q.front();
      q.pop_front();
    }
    (void)hipEventSynchronize(ev[it.slot]);
    code(it);
    std::lock_guard<std::mutex> lk(mu);
    busy[it.slot] = false;
    done++;
    cv.notify_all();
  }
}
void EcHost::drain() {
  std::unique_lock<std::mutex> lk(mu);
  cv.wait(lk, [&] { return done == queued; });
}

namespace rv {

// kernel probe p's pairs [kp_done, upto): their elapsed times and device
// spans summed (the spans in at most two copies)
hipError_t kp_harvest(rv_replay *r, int p, long upto) {
  const long d0 = r->kp_done[p], n = upto - d0;
  if (n <= 0) return hipSuccess;
  constexpr long K = rv_replay::kKp;
  for (long k = d0; k < upto; k++) {
    const size_t i = 2 * (size_t)(k % K);
    hipError_t e = hipEventSynchronize(r->kp_ev[p][i + 1]);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, r->kp_ev[p][i], r->kp_ev[p][i + 1]);
    if (e != hipSuccess) return e;
    r->kp_ms[p] += ms;
  }
  std::vector<unsigned long long> t(2 * (size_t)n);
  const long s0 = d0 % K, first = std::min(n, K - s0);
  hipError_t e = hipMemcpy(t.data(), r->kp_ts[p] + 2 * s0, 2 * sizeof(unsigned long long) * first,
                           hipMemcpyDeviceToHost);
  if (e == hipSuccess && n > first)
    e = hipMemcpy(t.data() + 2 * first, r->kp_ts[p], 2 * sizeof(unsigned long long) * (n - first),
                  hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  for (long k = 0; k < n; k++)
    if (t[2 * k + 1] > t[2 * k]) r->kp_dev_ms[p] += (double)(t[2 * k + 1] - t[2 * k]) * r->kp_tick_ms;
  r->kp_done[p] = upto;
  return hipSuccess;
}

// Frame::new (src/frame/mod.rs:55-90): luma pad 64 + 24, chroma >> dec
size_t frame_planes(const Geo &g, rv_plane &y, rv_plane &u, rv_plane &v) {
  const int pad = 88;
  const int cw = (g.W + g.xdec) >> g.xdec, ch = (g.H + g.ydec) >> g.ydec;
  size_t b = rv_plane_geometry(&y, g.W, g.H, 0, 0, pad, pad, g.hbd);
  b += rv_plane_geometry(&u, cw, ch, g.xdec, g.ydec, pad >> g.xdec, pad >> g.ydec, g.hbd);
  rv_plane_geometry(&v, cw, ch, g.xdec, g.ydec, pad >> g.xdec, pad >> g.ydec, g.hbd);
  y.bit_depth = u.bit_depth = v.bit_depth = g.bd;
  return b;
}
size_t plane_bytes(const rv_plane &p) { return (size_t)p.stride * p.alloc_height * (p.hbd ? 2 : 1); }

// One zeroed block per input / DPB slot, carved at 256-byte steps (a failed
// allocation latches in r->own)
static size_t up256(size_t v) { return (v + 255) / 256 * 256; }
static uint8_t *carve(uint8_t *&m, size_t bytes) {
  uint8_t *p = m;
  m += up256(bytes);
  return p;
}

void alloc_input(rv_replay *r, RvInput &in, bool pyramid) {
  const Geo &g = r->g;
  frame_planes(g, in.y, in.u, in.v);
  const int pad = 88;
  rv_plane_geometry(&in.hres, g.W / 2, g.H / 2, 1, 1, pad / 2, pad / 2, g.hbd);
  rv_plane_geometry(&in.qres, g.W / 4, g.H / 4, 2, 2, pad / 4, pad / 4, g.hbd);
  in.hres.bit_depth = in.qres.bit_depth = g.bd;
  const size_t by = plane_bytes(in.y), bu = plane_bytes(in.u);
  const size_t bh = pyramid ? plane_bytes(in.hres) : 0, bq = pyramid ? plane_bytes(in.qres) : 0;
  const size_t bs8 = pyramid ? (size_t)in.qres.stride * in.qres.alloc_height * 8 : 0;
  uint8_t *m = r->dev<uint8_t>(up256(by) + 2 * up256(bu) + up256(bh) + up256(bq) + up256(bs8),
                               Fill::Zero);
  if (!m) return;
  in.y.data = carve(m, by);
  in.u.data = carve(m, bu);
  in.v.data = carve(m, bu);
  if (!pyramid) return;
  in.hres.data = carve(m, bh);
  in.qres.data = carve(m, bq);
  in.qres_box = (uint32_t *)m;
}

void alloc_slot(rv_replay *r, RvSlot &s) {
  const Geo &g = r->g;
  frame_planes(g, s.y, s.u, s.v);
  const size_t by = plane_bytes(s.y), bu = plane_bytes(s.u);
  const size_t bf = (size_t)(g.w_in_b / 2) * (g.h_in_b / 2) * g.R * sizeof(rv_mv);
  uint8_t *m = r->dev<uint8_t>(up256(by) + 2 * up256(bu) + up256(bf), Fill::Zero);
  if (!m) return;
  s.y.data = carve(m, by);
  s.u.data = carve(m, bu);
  s.v.data = carve(m, bu);
  s.fmv = (rv_mv *)m;
}

// A round ring: the device counts (zeroed on st) from `dev`, the host-mapped
// publication ring from `host` (the engine's ring: the replay's, its own)
void round_ring_alloc(Owned &dev, Owned &host, RoundRing &q, hipStream_t st) {
  q.cnt = dev.dev<int32_t>(2 * RoundRing::kCnt + 1, Fill::Zero, st);
  q.h_pub = host.pinned<unsigned long long>(RoundRing::kPub,
                                            hipHostMallocMapped | hipHostMallocCoherent);
  if (!q.cnt || !q.h_pub) return;
  q.ticket = (uint32_t *)(q.cnt + 2 * RoundRing::kCnt);
  if (hipHostGetDevicePointer((void **)&q.d_pub, q.h_pub, 0) != hipSuccess) host.failed = true;
  for (int i = 0; i < RoundRing::kPub; i++) q.h_pub[i] = ~0ull;
}

int build_static_jobs(rv_replay *r) {
  const Geo &g = r->g;
  auto mx = [](int a, int b) { return a > b ? a : b; };
  auto mn = [](int a, int b) { return a < b ? a : b; };
  auto upload = [&](auto &vec, auto *&dst) -> int {
    if (!dst) dst = r->dev<std::decay_t<decltype(vec[0])>>(vec.size());
    if (!dst) return RV_EHIP;
    return hipMemcpy(dst, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice) ==
                   hipSuccess
               ? RV_OK
               : RV_EHIP;
  };
  for (int lv = 0; lv < 3; lv++) {
    const double me_lambda = r->lv[lv].me_lambda;
    // F1 coarse jobs (estimate_motion_ss4) at this level's me_range_scale
    const int s = 4 >> lv;
    const uint32_t lambda4 = (uint32_t)(me_lambda * 256.0 / 16.0 * 0.125);
    // every job array holds the lookahead's references (RA >= R: the
    // encode's first, then LAST3, la_refs_of); the encode launches R
    std::vector<rv_fs_job> jobs(g.nsb * r->RA);
    for (int sb = 0; sb < g.nsb; sb++) {
      const int sx = sb % g.tw, sy = sb / g.tw;
      int t0x, t0y, mi_w, mi_h;
      sb_tile(g, sx, sy, t0x, t0y, mi_w, mi_h);
      int bx = (g.tx0 + sx - t0x) * 16, by = (g.ty0 + sy - t0y) * 16;
      adjust_bo(mi_w, mi_h, bx, by, 64, 64);
      const int fbx = bx + t0x * 16, fby = by + t0y * 16;
      const int range_x = 192 * s, range_y = 64 * s;
      int mr[4];
      mv_range(g, fbx, fby, 64, 64, mr);
      rv_fs_job j;
      memset(&j, 0, sizeof(j));
      j.po_x = fbx;  // (bo << 2) >> 2
      j.po_y = fby;
      j.x_lo = fbx + (mx(-range_x, div_trunc8(mr[0])) >> 2);
      j.x_hi = fbx + (mn(range_x, div_trunc8(mr[1])) >> 2);
      j.y_lo = fby + (mx(-range_y, div_trunc8(mr[2])) >> 2);
      j.y_hi = fby + (mn(range_y, div_trunc8(mr[3])) >> 2);
      j.lambda = lambda4;
      for (int k = 0; k < r->RA; k++) jobs[k * g.nsb + sb] = j;  // ref-major
    }
    int e;
    if ((e = upload(jobs, r->fs_jobs[lv]))) return e;
    // F2 / F3 / lookahead diamond jobs: static fields (positions, MV ranges,
    // lambdas, predictor counts); fill_preds_kernel writes the predictors
    // from the coarse / half-res results every frame
    const uint32_t lambda2 = (uint32_t)(me_lambda * 256.0 / 4.0 * 0.125);
    const uint32_t lambda1 = (uint32_t)(me_lambda * 256.0 * 0.5);
    const int nsb = g.nsb;
    std::vector<rv_ds_job> jh((size_t)nsb * r->RA * 4), jf(nsb * r->RA), js(nsb * r->RA),
        jl((size_t)nsb * r->RA * 16);
    std::vector<int32_t> sh(jh.size() * 8, -1), sf(jf.size() * 8, -1), sl(jl.size() * 8, -1);
    for (int k = 0; k < r->RA; k++)
      for (int sb = 0; sb < nsb; sb++) {
        const int i = k * nsb + sb;
        const int sx = sb % g.tw, sy = sb / g.tw;
        int t0x, t0y, mi_w, mi_h;
        sb_tile(g, sx, sy, t0x, t0y, mi_w, mi_h);
        // the superblock in its tile, and the tile's size in superblocks
        const int tsx = g.tx0 + sx - t0x, tsy = g.ty0 + sy - t0y;
        const int tsw = (mi_w + 15) / 16, tsh = (mi_h + 15) / 16;
        const bool hw = tsx > 0, he = tsx < tsw - 1, hn = tsy > 0, hs = tsy < tsh - 1;
        auto coarse_src = [&](int sb2) { return 2 * (k * nsb + sb2); };
        auto half_src = [&](int sb2, int q) { return 2 * ((k * nsb + sb2) * 4 + q) + 1; };
        // diamond job at tile-relative 4x4 offset (bx, by), size bw, adjust_bo'd
        auto make = [&](int bx, int by, int bw, bool adj, int shift, uint32_t lambda) {
          if (adj) adjust_bo(mi_w, mi_h, bx, by, bw, bw);
          const int fbx = bx + t0x * 16, fby = by + t0y * 16;
          int mr[4];
          mv_range(g, fbx, fby, bw, bw, mr);
          rv_ds_job j;
          memset(&j, 0, sizeof(j));
          j.po_x = (fbx * 4) >> shift;
          j.po_y = (fby * 4) >> shift;
          j.mvx_min = mr[0] >> shift;
          j.mvx_max = mr[1] >> shift;
          j.mvy_min = mr[2] >> shift;
          j.mvy_max = mr[3] >> shift;
          j.lambda = lambda;
          return j;
        };
        // F2: build_half_res_pmvs (src/encoder.rs:2864-3019): the four 32x32
        // quadrants at half resolution (estimate_motion_ss2 / me_ss2,
        // src/me.rs:280-327, 465-519) from [the superblock's coarse MV, the
        // horizontal, the vertical neighbour's] (inside the tile)
        for (int q = 0; q < 4; q++) {
          rv_ds_job j = make(tsx * 16 + (q & 1) * 8, tsy * 16 + (q >> 1) * 8, 32, true, 1, lambda2);
          int32_t *ps = &sh[((size_t)i * 4 + q) * 8];
          int n = 1;
          ps[n++] = coarse_src(sb);
          if ((q & 1) ? he : hw) ps[n++] = coarse_src((q & 1) ? sb + 1 : sb - 1);
          if ((q >> 1) ? hs : hn) ps[n++] = coarse_src((q >> 1) ? sb + g.tw : sb - g.tw);
          j.n_pred = n;
          jh[(size_t)i * 4 + q] = j;
        }
        // F3: motion_estimation of the 64x64 (src/me.rs:193-278) from zero and
        // pmvs[0], the coarse MV; sub-pel from the full-pel winner
        {
          rv_ds_job j = make(tsx * 16, tsy * 16, 64, false, 0, lambda1);
          sf[(size_t)i * 8 + 1] = coarse_src(sb);
          j.n_pred = 2;
          jf[i] = j;
          j.n_pred = 1;
          js[i] = j;
        }
        // lookahead: build_full_res_pmvs (src/encoder.rs:3021-3166), the 16
        // 16x16 blocks from [the coarse MV, the covering quadrant, two
        // vertical and two horizontal candidates of this and the adjacent
        // superblocks] (estimate_motion, src/me.rs:337-390, full-pel)
        for (int y = 0; y < 4; y++)
          for (int x = 0; x < 4; x++) {
            rv_ds_job j = make(tsx * 16 + x * 4, tsy * 16 + y * 4, 16, true, 0, lambda1);
            // pmvs_X[0] = coarse, [1..4] = quadrants of superblock X; -1 absent
            auto pm = [&](int dx, int dy, int e) -> int {
              const bool ok = dx < 0 ? hw : dx > 0 ? he : dy < 0 ? hn : dy > 0 ? hs : true;
              if (!ok) return -1;
              const int sb2 = sb + dx + dy * g.tw;
              return e == 0 ? coarse_src(sb2) : half_src(sb2, e - 1);
            };
            const int L = x <= 1, T = y <= 1;
            const int cover = pm(0, 0, T ? (L ? 1 : 2) : (L ? 3 : 4));
            int v1, v2, h1, h2;
            switch (y) {
              case 0: v1 = pm(0, -1, 0); v2 = pm(0, -1, L ? 3 : 4); break;
              case 1: v1 = pm(0, -1, L ? 3 : 4); v2 = pm(0, 0, L ? 3 : 4); break;
              case 2: v1 = pm(0, 1, L ? 1 : 2); v2 = pm(0, 0, L ? 1 : 2); break;
              default: v1 = pm(0, 1, 0); v2 = pm(0, 1, L ? 1 : 2); break;
            }
            switch (x) {
              case 0: h1 = pm(-1, 0, 0); h2 = pm(-1, 0, T ? 2 : 4); break;
              case 1: h1 = pm(-1, 0, T ? 2 : 4); h2 = pm(0, 0, T ? 2 : 4); break;
              case 2: h1 = pm(1, 0, T ? 1 : 3); h2 = pm(0, 0, T ? 1 : 3); break;
              default: h1 = pm(1, 0, 0); h2 = pm(1, 0, T ? 2 : 4); break;
            }
            const int cand[6] = {coarse_src(sb), cover, v1, v2, h1, h2};
            int32_t *ps = &sl[((size_t)i * 16 + y * 4 + x) * 8];
            int n = 1;
            for (int c = 0; c < 6; c++)
              if (cand[c] >= 0) ps[n++] = cand[c];
            j.n_pred = n;
            jl[(size_t)i * 16 + y * 4 + x] = j;
          }
      }
    if ((e = upload(jh, r->jobs_half[lv])) || (e = upload(jh, r->jobs_half_l[lv])) ||
        (e = upload(jf, r->jobs_full[lv])) || (e = upload(js, r->jobs_sub[lv])) ||
        (e = upload(jl, r->jobs_look[lv])))
      return e;
    if (lv == 0 && ((e = upload(sh, r->src_half)) || (e = upload(sf, r->src_full)) ||
                    (e = upload(sl, r->src_look))))
      return e;
    // speed 6: motion_estimation of every 32x32 / 16x16 / 8x8 block at its
    // own position (no adjust_bo, src/me.rs:193-278): zero + the seeded
    // coarse predictor, then the sub-pel search from the full-pel winner
    for (int l = 1; r->lvl && l < kLevels; l++) {
      rv_replay::PLevel &P = r->pl[l];
      std::vector<rv_ds_job> f6((size_t)P.n * g.R), s6((size_t)P.n * g.R);
      for (int k = 0; k < g.R; k++)
        for (int b = 0; b < P.n; b++) {
          const int X = (P.cg.tx0 + b % P.gw) * P.B, Y = (P.cg.ty0 + b / P.gw) * P.B;
          int mr[4];
          mv_range(g, X >> 2, Y >> 2, P.B, P.B, mr);
          rv_ds_job j;
          memset(&j, 0, sizeof(j));
          j.po_x = X;
          j.po_y = Y;
          j.mvx_min = mr[0];
          j.mvx_max = mr[1];
          j.mvy_min = mr[2];
          j.mvy_max = mr[3];
          j.lambda = lambda1;
          j.n_pred = 2;
          f6[(size_t)k * P.n + b] = j;
          j.n_pred = 1;
          s6[(size_t)k * P.n + b] = j;
        }
      if ((e = upload(f6, P.jobs_full[lv])) || (e = upload(s6, P.jobs_sub[lv]))) return e;
    }
  }
  r->jobs_built = true;
  return RV_OK;
}

// The static job records, built once: the first coded frame, or the
// lookahead engine when it starts before any frame (inputs declared ready).
int ensure_jobs(rv_replay *r) {
  std::lock_guard<std::mutex> lk(r->jobs_mu);
  if (r->jobs_built) return RV_OK;
  if (!r->lv[0].set || !r->lv[1].set || !r->lv[2].set)
    return rv_set_error(RV_EINVAL, "rv_replay: level params not set");
  return build_static_jobs(r);
}

// Packed rectangles of group k (its visible Y, U, V region; with
// deblocking also its rows of the block map, planes 3 = log2 size, 4 =
// skip), bytes into the group's slice of the exchange buffer.  Returns the
// bytes; *n = the rectangles.
int group_rects(const rv_replay *r, int k, XRect out[9], int *n) {
  const Geo &g = r->g;
  const int32_t *gr = r->grects + 4 * k;
  const int px = g.hbd ? 2 : 1;
  const int cw = (g.W + g.xdec) >> g.xdec, ch = (g.H + g.ydec) >> g.ydec;
  int64_t off = 0;
  for (int p = 0; p < 3; p++) {
    const int xd = p ? g.xdec : 0, yd = p ? g.ydec : 0;
    const int pw = p ? cw : g.W, ph = p ? ch : g.H;
    const int x0 = (gr[0] * kSb) >> xd, y0 = (gr[1] * kSb) >> yd;
    int x1 = ((gr[0] + gr[2]) * kSb) >> xd, y1 = ((gr[1] + gr[3]) * kSb) >> yd;
    x1 = x1 < pw ? x1 : pw;
    y1 = y1 < ph ? y1 : ph;
    out[p] = XRect{off, p, x0, y0, x1 - x0, y1 - y0};
    off += (int64_t)(x1 - x0) * (y1 - y0) * px;
  }
  *n = 3;
  if (r->deblock) {
    const int x0 = gr[0] * 16, y0 = gr[1] * 16;
    int x1 = (gr[0] + gr[2]) * 16, y1 = (gr[1] + gr[3]) * 16;
    x1 = x1 < r->mi_cols ? x1 : r->mi_cols;
    y1 = y1 < r->mi_rows ? y1 : r->mi_rows;
    for (int m = 0; m < 2; m++) {
      out[3 + m] = XRect{off, 3 + m, x0, y0, x1 - x0, y1 - y0};
      off += (int64_t)(x1 - x0) * (y1 - y0);
    }
    *n = 5;
  }
  if (r->exact) {  // the group's 8x8 cells of the frame's motion field (bytes)
    const int w8 = g.w_in_b / 2, h8 = g.h_in_b / 2, cb = g.R * (int)sizeof(rv_mv);
    const int x0 = gr[0] * 8, y0 = gr[1] * 8;
    int x1 = (gr[0] + gr[2]) * 8, y1 = (gr[1] + gr[3]) * 8;
    x1 = x1 < w8 ? x1 : w8;
    y1 = y1 < h8 ? y1 : h8;
    out[*n] = XRect{off, 5, x0 * cb, y0, (x1 - x0) * cb, y1 - y0};
    off += (int64_t)(x1 - x0) * cb * (y1 - y0);
    (*n)++;
  }
  if (r->lrf) {  // the group's loop-restoration units ((set, xqd0, xqd1) per superblock)
    const int sbc = (g.W + kSb - 1) / kSb, sbr = (g.H + kSb - 1) / kSb;
    const int x0 = gr[0], y0 = gr[1];
    int x1 = gr[0] + gr[2], y1 = gr[1] + gr[3];
    x1 = x1 < sbc ? x1 : sbc;
    y1 = y1 < sbr ? y1 : sbr;
    for (int p = 0; p < 3; p++) {
      out[*n] = XRect{off, 6 + p, 3 * x0, y0, 3 * (x1 - x0), y1 - y0};
      off += (int64_t)3 * (x1 - x0) * (y1 - y0);
      (*n)++;
    }
  }
  return (int)off;
}

template <typename Px>
static void xcopy_launch(hipStream_t st, const rv_plane *pl, const XRect *rects, int n,
                         int to_plane, uint8_t *buf) {
  if (n == 0) return;
  XArgs a;
  memset(&a, 0, sizeof(a));
  for (int p = 0; p < 3; p++) a.pl[p] = pl[p];
  int64_t most = 0;
  for (int i = 0; i < n; i++) {
    a.rect[i] = rects[i];
    const int64_t px = (int64_t)rects[i].w * rects[i].h;
    most = px > most ? px : most;
  }
  a.n = n;
  a.to_plane = to_plane;
  a.buf = buf;
  int64_t gx = (most + 255) / 256;
  gx = gx > 4096 ? 4096 : gx < 1 ? 1 : gx;
  xcopy_kernel<Px><<<dim3((unsigned)gx, (unsigned)n), 256, 0, st>>>(a);
}

// Copy rectangles between the slot's planes / the block map and a packed
// buffer (pixel rectangles at the pixel width, map rectangles bytewise).
int xcopy(rv_replay *r, const RvSlot &s, const XRect *rects, int n, int to_plane, uint8_t *buf) {
  XRect px[3 * kMaxGroups], mp[3 * kMaxGroups], un[3 * kMaxGroups];
  int npx = 0, nmp = 0, nun = 0;
  for (int i = 0; i < n; i++) {
    if (rects[i].plane < 3) {
      px[npx++] = rects[i];
    } else if (rects[i].plane < 6) {
      mp[nmp] = rects[i];
      mp[nmp++].plane -= 3;
    } else {
      un[nun] = rects[i];
      un[nun++].plane -= 6;
    }
  }
  const rv_plane pl[3] = {s.y, s.u, s.v};
  if (r->g.hbd)
    xcopy_launch<uint16_t>(r->stream, pl, px, npx, to_plane, buf);
  else
    xcopy_launch<uint8_t>(r->stream, pl, px, npx, to_plane, buf);
  if (nmp) {
    rv_plane m[3];
    memset(m, 0, sizeof(m));
    m[0].data = r->mi_lg;
    m[1].data = r->mi_skip;
    for (int i = 0; i < 2; i++) {
      m[i].stride = r->mi_stride;
      m[i].width = r->mi_cols;
      m[i].height = r->mi_rows;
    }
    // plane 5: the slot's motion field as bytes ([h8][w8][R] rv_mv)
    const int fb = r->g.w_in_b / 2 * r->g.R * (int)sizeof(rv_mv);
    m[2].data = s.fmv;
    m[2].stride = fb;
    m[2].width = fb;
    m[2].height = r->g.h_in_b / 2;
    xcopy_launch<uint8_t>(r->stream, m, mp, nmp, to_plane, buf);
  }
  if (nun) {  // planes 6-8: the loop-restoration units of Y, U, V ([sbr][sbc][3] bytes each)
    const int sbc = (r->g.W + kSb - 1) / kSb, sbr = (r->g.H + kSb - 1) / kSb;
    rv_plane u[3];
    memset(u, 0, sizeof(u));
    for (int p = 0; p < 3; p++) {
      u[p].data = r->lrf_units + (size_t)p * sbr * sbc * 3;
      u[p].stride = 3 * sbc;
      u[p].width = 3 * sbc;
      u[p].height = sbr;
    }
    xcopy_launch<uint8_t>(r->stream, u, un, nun, to_plane, buf);
  }
  RV_HIP_CHECK_LAUNCH();
  return RV_OK;
}

int pad_slot(rv_replay *r, const RvSlot &s) {
  const rv_plane pl3[3] = {s.y, s.u, s.v};
  return rv_frame_pad_dev(pl3, nullptr, r->stream);
}

// deblock_filter_optimize + deblock_filter_frame of a slot coded from input
// `in` (src/encoder.rs:2789-2793): speed 6 searches the levels on the
// device (sse_optimize) and the filter reads them there; speed 10 takes
// pyramid level lv's fast levels.  Nothing is filtered unless a luma level
// is non-zero.
int deblock_slot(rv_replay *r, const RvSlot &s, const RvInput &in, int lv) {
  const rv_plane pl3[3] = {s.y, s.u, s.v};
  if (r->s6) {
    const rv_plane src[3] = {in.y, in.u, in.v};
    const int e = rv_deblock_sse_dev(pl3, src, r->g.W, r->g.H, r->mi_lg, r->mi_skip,
                                     r->mi_stride, r->db_tally, r->db_dlev, r->g.bd, r->stream);
    if (e != RV_OK) return e;
    return rv_deblock_frame_dev(pl3, r->g.W, r->g.H, r->mi_lg, r->mi_skip, r->mi_stride,
                                r->db_dlev, r->g.bd, r->stream, nullptr);
  }
  const uint8_t l = r->db_level[lv];
  if (!l) return RV_OK;
  const uint8_t lv4[4] = {l, l, l, l};
  return rv_deblock_frame_dev(pl3, r->g.W, r->g.H, r->mi_lg, r->mi_skip, r->mi_stride, nullptr,
                              r->g.bd, r->stream, lv4);
}

// cdef_filter_frame of a deblocked slot (src/encoder.rs:2795-2802), then
// the slot's padding: the directions come from the slot's luma, every plane
// is filtered out of the slot into the scratch frame (one launch), and the
// scratch frame is copied back and padded in one pass (rv_frame_pad_dev) --
// three launches.  cdef_bits 0: every superblock uses entry 0 of the
// tables, the level's strengths.
int cdef_pad_slot(rv_replay *r, const RvSlot &s, int lv, const LrfGeo *lg) {
  const rv_plane rec[3] = {s.y, s.u, s.v};
  const rv_plane out[3] = {r->cdef_pre.y, r->cdef_pre.u, r->cdef_pre.v};
  uint8_t ys[8] = {}, us[8] = {};
  ys[0] = r->cdef_str[lv][0];
  us[0] = r->cdef_str[lv][1];
  RV_R(rv_cdef_find_dirs(&rec[0], r->g.W, r->g.H, r->mi_skip, r->mi_stride, r->cdef_dir,
                         r->cdef_var, r->g.bd, r->stream));
  // cdef_damping = 3 (src/encoder.rs:665)
  RV_R(rv_cdef_filter_frame_dev(rec, out, r->g.W, r->g.H, r->mi_skip, r->mi_stride, r->cdef_dir,
                                r->cdef_var, r->cdef_idx, ys, us, 3, r->g.bd, r->stream));
  if (!lg) return rv_frame_pad_dev(rec, out, r->stream);
  // lrf_filter_frame: the CDEF output restored, the deblocked slot for the
  // stripes' edges (pre_cdef_frame, src/encoder.rs:2795-2806)
  const rv_plane lo[3] = {r->lrf_out.y, r->lrf_out.u, r->lrf_out.v};
  RV_R(lrf_filter_launch(out, rec, lo, *lg, r->lrf_units, 1, r->stream));
  return rv_frame_pad_dev(rec, lo, r->stream);
}

// rdo_loop_decision's restoration choices for the superblocks of group
// rect (in superblocks; null: the frame), from the reconstruction as the
// tile's coding leaves it (before the deblocking), into r->lrf_units.
int lrf_decide_slot(rv_replay *r, const RvSlot &s, const RvInput &in, int lv, const LrfGeo &lg,
                           const int32_t *rect) {
  const Geo &g = r->g;
  const rv_plane rec[3] = {s.y, s.u, s.v}, src[3] = {in.y, in.u, in.v};
  // its CDEF's directions (cdef_pad_slot finds the deblocked frame's
  // afterwards, in the same buffers)
  if (r->cdef)
    RV_R(rv_cdef_find_dirs(&rec[0], g.W, g.H, r->mi_skip, r->mi_stride, r->cdef_dir, r->cdef_var, g.bd,
                           r->stream));
  RV_R(lrf_rdo_launch(rec, src, r->mi_skip, r->mi_stride, r->imp_last, g.w_imp, g.w_in_b, g.h_in_b, lg,
                      r->cdef, r->cdef_dir, r->cdef_var, r->cdef_str[lv], r->lv[lv].ds, r->lrf_err,
                      r->lrf_xqd, rect, r->stream));
  return lrf_decide_launch(lg, r->lrf_err, r->lrf_xqd, r->lv[lv].lambda, r->lrf_units, rect, r->lrf_fix_passes, r->stream);
}


// The loop filters of a coded slot and its padding: the frame is then a
// reference (src/encoder.rs:2789-2802, 3411-3429).
int filter_slot(rv_replay *r, const RvSlot &s, const RvInput &in, int lv) {
  LrfGeo lg;
  if (r->lrf) {
    const Geo &g = r->g;
    RV_R(lrf_geometry(g.W, g.H, g.xdec, g.ydec, g.bd, r->lv[lv].qidx, g.tws, g.ths, &lg));
    if (!groups_active(r)) RV_R(lrf_decide_slot(r, s, in, lv, lg, nullptr));
  }
  if (r->deblock) RV_R(deblock_slot(r, s, in, lv));
  return r->cdef ? cdef_pad_slot(r, s, lv, r->lrf ? &lg : nullptr) : pad_slot(r, s);
}

// Coding order of the reorder pyramid: coded frame n >= 1 (n = 0 is the
// key frame, display 0).
void frame_info(long n, int R, rv_replay_frame_info *f) {
  memset(f, 0, sizeof(*f));
  if (n == 0) {
    f->is_key = 1;
    return;
  }
  const long g = (n - 1) / 4, j = (n - 1) % 4;
  static const int kOff[4] = {4, 2, 1, 3}, kScale[4] = {4, 2, 1, 1};
  static const int kRef[4][2] = {{0, -4}, {0, 4}, {0, 2}, {2, 4}};
  f->display = (int)(4 * g + kOff[j]);
  f->me_range_scale = kScale[j];
  f->level = j == 0 ? 0 : j == 1 ? 1 : 2;
  for (int k = 0; k < R; k++) {
    long d = 4 * g + kRef[j][k];
    f->ref_display[k] = (int)(d < 0 ? 0 : d);
  }
  // reference_mode SELECT unless the frame is the first output of its group
  // (src/encoder.rs:832-836); compound needs a forward and a backward
  // reference (src/rdo.rs:914-941): display 4g+2 and 4g+3
  f->compound = R == 2 && (j == 1 || j == 3);
}

// The lookahead's references of coded frame m >= 1: rav1e's distinct DPB
// slots of fi.ref_frames (compute_block_importances' unique_indices,
// src/api/internal.rs:875-882); compute_lookahead_motion_vectors searches
// each slot once (build_coarse_pmvs / build_full_res_pmvs loop over
// ALL_INTER_REFS, src/encoder.rs:2732-2738, 3037-3040).  k < R are the
// encode's references (k = 0: LAST, the backward reference; k = 1: LAST2 at
// level 0, ALTREF -- the forward reference -- above); with R = 2 a frame
// above level 0 adds k = 2, LAST3: its own slot, which holds the previous
// frame of its level, or the key frame, which fills every slot
// (src/encoder.rs:658, 772-828).  order: the propagation's reference order
// (mv index order: LAST, LAST2 / LAST3, ALTREF).  oracle/orc_replay.c
// la_refs_of is the same table; tests/test_importance_window.py derives it
// from rav1e's slot logic.
LaRefs la_refs_of(long m, int R) {
  LaRefs l;
  memset(&l, 0, sizeof(l));
  rv_replay_frame_info f;
  frame_info(m, R, &f);
  for (int k = 0; k < R; k++) {
    l.disp[k] = f.ref_display[k];
    l.order[k] = k;
  }
  l.n = R;
  const long g = (m - 1) / 4, j = (m - 1) % 4;
  if (R == 2 && j > 0) {
    const long d3 = j == 1 ? 4 * g - 2 : j == 2 ? 4 * g - 1 : 4 * g + 1;
    l.disp[2] = (int)(d3 < 0 ? 0 : d3);
    l.n = 3;
    l.order[1] = 2;
    l.order[2] = 1;
  }
  return l;
}

// Where the 32x32 .. 8x8 levels run (s6, lvl, the rectangle ex0, ey0 + ew x
// eh), which of them hold leaves / search motion, their grids over that
// rectangle and the layout of the result words.
static int configure_levels(rv_replay *r) {
  const Geo &g = r->g;
  r->nwords = (size_t)g.nsb * (kWordsPerRef * g.R + 4);
  if (r->cfg.flags & RV_REPLAY_SPEED6) {
    if (g.xdec != g.ydec)
      return rv_set_error(RV_EINVAL, "rv_replay_create: speed 6 needs 4:2:0 or 4:4:4");
    r->s6 = true;
    r->lvl = true;
    r->ew = g.tw;
    r->eh = g.th;
    for (int l = 1; l < kLevels; l++) r->lv_used[l] = true;  // every level holds leaves
  } else if (g.xdec == g.ydec) {
    // speed 10: encode_partition_topdown's must_split (src/encoder.rs:2407-
    // 2445) at the frame edges, over the bounding rectangle of the group's
    // superblocks past the right / bottom edge; the levels holding leaves are
    // those of the must_split walk of these superblocks (largest blocks inside)
    int x0 = g.tw, y0 = g.th, x1 = -1, y1 = -1;
    for (int sb = 0; sb < g.nsb; sb++) {
      const int sx = sb % g.tw, sy = sb / g.tw, X = (g.tx0 + sx) * kSb, Y = (g.ty0 + sy) * kSb;
      if (X + kSb <= g.W && Y + kSb <= g.H) continue;
      x0 = std::min(x0, sx);
      y0 = std::min(y0, sy);
      x1 = std::max(x1, sx);
      y1 = std::max(y1, sy);
      for (int l = 1; l < kLevels; l++) {
        const int B = kSb >> l;
        for (int y = Y; y < Y + kSb; y += B)
          for (int x = X; x < X + kSb; x += B) {
            const int inside = x + B <= g.W && y + B <= g.H;
            const int pin = (x & ~(2 * B - 1)) + 2 * B <= g.W && (y & ~(2 * B - 1)) + 2 * B <= g.H;
            if (inside && !pin) r->lv_used[l] = true;  // a leaf: inside, its parent is not
          }
      }
    }
    if (x1 >= 0) {
      r->lvl = true;
      r->ex0 = x0;
      r->ey0 = y0;
      r->ew = x1 - x0 + 1;
      r->eh = y1 - y0 + 1;
    }
  }
  if (!r->lvl) return RV_OK;
  r->lv_me[1] = r->lv_used[1] || r->lv_used[2] || r->lv_used[3];
  r->lv_me[2] = r->lv_used[2];
  r->lv_me[3] = r->lv_used[3];
  rv_replay::PLevel &P0 = r->pl[0];
  P0.B = kSb;
  P0.n = g.nsb;
  P0.gw = g.tw;
  P0.gh = g.th;
  for (int l = 1; l < kLevels; l++) {
    rv_replay::PLevel &P = r->pl[l];
    const int k = 1 << l;
    P.B = kSb >> l;
    P.gw = r->ew * k;
    P.gh = r->eh * k;
    P.n = P.gw * P.gh;
    P.bc = P.B >> g.xdec;
    P.bch = P.B >> g.ydec;
    P.txl = 4 - l;                                              // TX_32X32 .. TX_8X8
    P.txc = P.bc == 32 ? 3 : P.bc == 16 ? 2 : P.bc == 8 ? 1 : 0;  // .. TX_4X4
    P.cg = CandGeo{P.n, P.gw, P.gh, (g.tx0 + r->ex0) * k, (g.ty0 + r->ey0) * k, g.tws * k,
                   g.ths * k, g.R, g.M, 0};
    P.woff = r->nwords;
    r->nwords += (size_t)P.n * (4 * g.R + 4);
  }
  r->wpart = r->nwords;
  r->nwords += (size_t)g.nsb;
  return RV_OK;
}

// The stages the flags switch on, their host-side sizes, and the two
// environment switches.
static int configure_stages(rv_replay *r) {
  const Geo &g = r->g;
  const uint32_t flags = r->cfg.flags;
  // intra-mode screening: speed 10 4:2:0 unless RV_REPLAY_NO_INTRA
  r->intra = !r->s6 && !(flags & RV_REPLAY_NO_INTRA) && g.xdec == 1 && g.ydec == 1;
  // speed 10: rav1e's MV stacks in coding-order rounds
  r->exact = !r->s6 && !(flags & RV_REPLAY_MVREF_STANDIN);
  // does a superblock's top-right neighbour (same tile) lie past the right
  // frame edge, i.e. is it a must_split leaf?
  for (int sb = 0; sb < g.nsb && r->exact && r->lvl; sb++) {
    const int fsx = g.tx0 + sb % g.tw, fsy = g.ty0 + sb / g.tw;
    const int t0x = fsx - fsx % g.tws;
    const int cols = std::min(g.tws * 16, g.w_in_b - t0x * 16);
    if ((fsx + 1) * 64 <= g.W && (fsy + 1) * 64 <= g.H && fsy % g.ths != 0 &&
        (fsx - t0x) * 16 + 16 < cols && (fsx + 2) * 64 > g.W)
      r->edge_tr = true;
  }
  if (flags & RV_REPLAY_CDEF) {
    if (!(flags & RV_REPLAY_DEBLOCK) || (g.W & 7) || (g.H & 7))
      return rv_set_error(RV_EINVAL, "rv_replay_create: RV_REPLAY_CDEF needs RV_REPLAY_DEBLOCK and a "
                                     "frame size that is a multiple of 8");
    r->cdef = true;
  }
  if (flags & RV_REPLAY_LRF) {
    LrfGeo lg;
    // (the unit size depends on the quantizer: rv_replay_set_level_params
    // checks every level's; 100 here is the replay's default level 0)
    if (!r->cdef || g.xdec != g.ydec ||
        lrf_geometry(g.W, g.H, g.xdec, g.ydec, g.bd, 100, g.tws, g.ths, &lg) != RV_OK)
      return rv_set_error(RV_EINVAL, "rv_replay_create: RV_REPLAY_LRF needs RV_REPLAY_CDEF, 4:2:0 or 4:4:4 "
                                     "(rav1e's enable_restoration is off in 4:2:2) and units of one superblock");
    r->lrf = true;
    // RAV1E_LRF_FIX=0 (A/B): the one-wave serial decision; RAV1E_LRF_FIX_PASSES
    // = 1 .. caps the fixed point's parallel passes (tests: the serial rest
    // after the cap).  Read here, once: the worker threads of a pipelined
    // replay must not call getenv per frame while the caller may setenv.
    const char *fe = getenv("RAV1E_LRF_FIX"), *fp = getenv("RAV1E_LRF_FIX_PASSES");
    r->lrf_fix_passes = (fe && fe[0] == '0') ? 0 : fp ? std::max(atoi(fp), 1) : 1 << 30;
  }
  r->entropy = (flags & RV_REPLAY_ENTROPY) != 0;
  if (r->entropy && g.xdec != g.ydec)
    return rv_set_error(RV_EINVAL, "rv_replay_create: RV_REPLAY_ENTROPY needs xdec == ydec");
  r->deblock = (flags & RV_REPLAY_DEBLOCK) != 0;
  if (r->deblock || r->entropy) {  // the block map
    r->mi_cols = (g.W + 3) / 4;
    r->mi_rows = (g.H + 3) / 4;
    r->mi_stride = (r->mi_cols + 15) / 16 * 16;
  }
  if (r->entropy) {
    EcFrameBufs &b = r->ecb;
    b.ntiles = ((g.tw + g.tws - 1) / g.tws) * ((g.th + g.ths - 1) / g.ths);
    b.max_jobs = ec_max_jobs(g.nsb, b.ntiles);
    b.map_w4 = g.tws * 16;
    b.map_h4 = g.ths * 16;
    // one token per coded coefficient plus 4 per job covers every block
    // whose levels stay below 3; more sets the overflow flag (an error)
    b.cap = (uint32_t)((size_t)g.nsb * (1024 + 2 * r->ntx_c * 1024) + (size_t)b.max_jobs * 4);
  }
  const char *e = getenv("RAV1E_HIP_REPLAY_SERIAL");
  r->overlap = !(e && e[0] == '1');
  return RV_OK;
}

// Every check, in the order its message is reported, and every derived value
// that needs no device (the frame and the tile group, a rectangle of whole tiles,
// here).  No HIP call: a rejected configuration has touched no device.
static int replay_configure(const rv_replay_cfg *cfg, rv_replay *r) {
  if (!cfg || cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 7) || (cfg->height & 7) ||
      (cfg->bit_depth != 8 && cfg->bit_depth != 10 && cfg->bit_depth != 12) || cfg->xdec < 0 ||
      cfg->xdec > 1 || cfg->ydec < 0 || cfg->ydec > 1 || cfg->n_refs < 1 || cfg->n_refs > 2 ||
      cfg->n_inputs < 1 || cfg->tile_w_sb < 0 || cfg->tile_h_sb < 0)
    return rv_set_error(RV_EINVAL, "rv_replay_create: bad config");
  r->cfg = *cfg;
  Geo &g = r->g;
  g.W = cfg->width;
  g.H = cfg->height;
  g.xdec = cfg->xdec;
  g.ydec = cfg->ydec;
  g.bd = cfg->bit_depth;
  g.hbd = cfg->bit_depth > 8;
  g.w_in_b = 2 * ((g.W + 7) >> 3);
  g.h_in_b = 2 * ((g.H + 7) >> 3);
  const int sbc = (g.W + kSb - 1) / kSb, sbr = (g.H + kSb - 1) / kSb;
  g.tx0 = cfg->tile_x0;
  g.ty0 = cfg->tile_y0;
  g.tw = cfg->tile_w > 0 ? cfg->tile_w : sbc - g.tx0;
  g.th = cfg->tile_h > 0 ? cfg->tile_h : sbr - g.ty0;
  g.tws = cfg->tile_w_sb > 0 ? cfg->tile_w_sb : sbc;
  g.ths = cfg->tile_h_sb > 0 ? cfg->tile_h_sb : sbr;
  if (g.tx0 < 0 || g.ty0 < 0 || g.tw <= 0 || g.th <= 0 || g.tx0 + g.tw > sbc ||
      g.ty0 + g.th > sbr || g.tx0 % g.tws || g.ty0 % g.ths ||
      ((g.tx0 + g.tw) % g.tws && g.tx0 + g.tw != sbc) ||
      ((g.ty0 + g.th) % g.ths && g.ty0 + g.th != sbr))
    return rv_set_error(RV_EINVAL,
                        "rv_replay_create: the tile group is not a rectangle of whole tiles");
  g.vis_w = (g.W - g.tx0 * kSb) < g.tw * kSb ? g.W - g.tx0 * kSb : g.tw * kSb;
  g.vis_h = (g.H - g.ty0 * kSb) < g.th * kSb ? g.H - g.ty0 * kSb : g.th * kSb;
  g.nsb = g.tw * g.th;
  g.R = cfg->n_refs;
  r->RA = g.R == 2 ? kImpMaxRefs : g.R;
  g.M = kCandModes;
  g.C = g.R * g.M + (g.R == 2 ? kCompModes : 0);  // the most a frame evaluates
  g.cw = kSb >> g.xdec;
  g.ch = kSb >> g.ydec;
  g.w_imp = g.w_in_b / 2;
  g.h_imp = g.h_in_b / 2;
  r->cg = CandGeo{g.nsb, g.tw, g.th, g.tx0, g.ty0, g.tws, g.ths, g.R, g.M, 0};
  // 8x8 sums of 10-bit pixels fit the u16 box-sum table; 12-bit searches
  // exhaustively
  r->sea = g.bd <= 10 && (cfg->flags & RV_REPLAY_EXHAUSTIVE_FS) == 0;
  r->ntx_c = (g.cw / 32) * (g.ch / 32);
  r->imp_bx = g.vis_w / 8;
  r->imp_by = g.vis_h / 8;
  r->n_imp = r->imp_bx * r->imp_by;
  const int32_t me[4] = {g.tx0, g.ty0, g.tw, g.th};
  memcpy(r->grects, me, sizeof(me));
  RV_R(configure_levels(r));
  return configure_stages(r);
}

// the DPB and the inputs (a twin borrows the primary's)
static void alloc_dpb(rv_replay *r, const rv_replay *share) {
  r->slots = share ? share->slots : std::vector<RvSlot>(kSlots);
  r->inputs = share ? share->inputs : std::vector<RvInput>(r->cfg.n_inputs);
  if (share) return;
  for (auto &s : r->slots) alloc_slot(r, s);
  for (auto &in : r->inputs) alloc_input(r, in, true);
}

// the 64x64 stages: F1 .. F3 and the lookahead (results per superblock and
// reference), F4 / F6, the result words and their tail
static void alloc_superblocks(rv_replay *r) {
  const Geo &g = r->g;
  const size_t nsb = (size_t)g.nsb, nr = nsb * g.R, nc = nsb * g.C;
  r->coarse = r->dev<rv_fs_result>(nr);
  r->half = r->dev<rv_fs_result>(nr * 4);
  r->look = r->dev<rv_fs_result>(nr * 16, Fill::Zero);
  r->half_l = r->dev<rv_fs_result>(nr * 4, Fill::Zero);
  r->la_list = r->dev<int32_t>(nr * 20);
  r->full = r->dev<rv_fs_result>(nr);
  r->sub = r->dev<rv_fs_result>(nr);
  r->ds_evals = r->dev<uint32_t>((size_t)rv_replay::kRing * 2 * nr, Fill::Zero);
  r->l_out = r->dev<uint64_t>(nc * 3);
  r->c_out = r->dev<uint64_t>(nc * r->ntx_c * 3 * 2);
  r->win = r->dev<RdoWinner>(nsb);
  r->cand_list = r->dev<int32_t>(nc);
  // zeroed: tag 0 matches no frame
  r->cand_key = r->dev<CandKey>(nsb * (g.R * g.M + kCompModes), Fill::Zero);
  r->f3dirty = r->dev<uint8_t>(nsb * g.R);
  r->f2dirty = r->dev<uint8_t>(nsb * g.R * 4);
  r->cand_count = r->dev<int32_t>(2, Fill::Zero);  // [single, compound]
  r->f4_args = r->dev<RdoArgs>(4);
  r->cand_evals = r->dev<uint32_t>((size_t)rv_replay::kRing * 2 * kLevels, Fill::Zero);
  r->l_lev = r->dev<int32_t>(nsb * 1024, Fill::Zero);
  r->c_lev = r->dev<int32_t>(nsb * r->ntx_c * 1024 * 2, Fill::Zero);
  r->words = r->dev<uint64_t>(r->nwords, Fill::Zero);
  r->tail = r->dev<unsigned long long>(5, Fill::Zero);
}

// the 32x32 .. 8x8 levels' arrays and every level's leaf list
static void alloc_levels(rv_replay *r) {
  if (!r->lvl) return;
  size_t nleaf = (size_t)r->g.nsb;
  for (int l = 1; l < kLevels; l++) {
    rv_replay::PLevel &P = r->pl[l];
    const size_t n = (size_t)P.n, nr = n * r->g.R, nc = n * r->g.C;
    P.full = r->dev<rv_fs_result>(nr);
    P.sub = r->dev<rv_fs_result>(nr);
    P.l_out = r->dev<uint64_t>(nc * 3);
    P.c_out = r->dev<uint64_t>(nc * 3 * 2);
    P.win = r->dev<RdoWinner>(n);
    P.cand_list = r->dev<int32_t>(nc);
    P.cand_count = r->dev<int32_t>(2, Fill::Zero);
    P.l_lev = r->dev<int32_t>(n * P.B * P.B, Fill::Zero);
    P.c_lev = r->dev<int32_t>(n * P.bc * P.bch * 2, Fill::Zero);
    nleaf += n;
  }
  int32_t *lf = r->dev<int32_t>(nleaf);
  r->leaf_count = r->dev<int32_t>(kLevels, Fill::Zero);
  for (int l = 0; l < kLevels && lf; l++) {
    r->pl[l].leaf = lf;
    lf += r->pl[l].n;
  }
}

static void alloc_intra(rv_replay *r) {
  r->i_stats = r->dev<uint32_t>((size_t)rv_replay::kRing * 3, Fill::Zero);
  if (!r->intra) return;
  const size_t n = (size_t)r->g.nsb;
  r->i_elig = r->dev<uint8_t>(n);
  r->i_was = r->dev<uint8_t>(n, Fill::Zero);
  r->i_win = r->dev<uint8_t>(2 * n, Fill::Zero);
  r->i_modes = r->dev<uint8_t>(4 * n);
  for (int32_t **list : {&r->i_mark, &r->i_list[0], &r->i_list[1], &r->i_commit, &r->i_revert})
    *list = r->dev<int32_t>(n);
  r->i_cnt = r->dev<int32_t>(4);
  r->i_edges = r->dev<uint8_t>(n * 3 * kIntraEdge * (r->g.hbd ? 2 : 1));
  r->i_lout = r->dev<uint64_t>(n * 3 * 3);
  r->i_cout = r->dev<uint64_t>(n * 6 * 3 * 2);
  r->h_cnt = r->own.pinned<int32_t>(4, hipHostMallocDefault);
  r->ev_ielig = r->own.event(hipEventDisableTiming);
}

// the rounds' counts (the lookahead's EPZS rounds at every speed, the MV-
// stack rounds at speed 10) and the stacks' state
static void alloc_mvref(rv_replay *r) {
  round_ring_alloc(r->own, r->own, r->rr, r->stream);
  if (!r->exact) return;
  const size_t n = (size_t)r->g.nsb;
  r->stk = r->dev<MvStack>(n);
  for (int l = 0; l < 3; l++) r->dec_lv[l] = r->dev<BlkDec>(n, Fill::Zero);
  r->mv_active = r->dev<uint8_t>(n);
  r->mv_list = r->dev<int32_t>(2 * n);
}

// the loop filters: CDEF, loop restoration, the block map, speed 6's tallies
static void alloc_filters(rv_replay *r) {
  const Geo &g = r->g;
  const size_t n8 = (size_t)(g.W / 8) * (g.H / 8), n64 = (size_t)((g.W + 63) / 64) * ((g.H + 63) / 64);
  if (r->cdef) {
    r->cdef_dir = r->dev<uint8_t>(n8);
    r->cdef_var = r->dev<int32_t>(n8);
    r->cdef_idx = r->dev<uint8_t>(n64, Fill::Zero);
    alloc_input(r, r->cdef_pre, false);
  }
  if (r->lrf) {  // per plane and superblock of the frame (LrfGeo::nsb)
    r->lrf_err = r->dev<uint64_t>(3 * n64 * 17);
    r->lrf_xqd = r->dev<int8_t>(3 * n64 * 32);
    r->lrf_units = r->dev<int8_t>(3 * n64 * 3);
    alloc_input(r, r->lrf_out, false);
  }
  if (!r->deblock && !r->entropy) return;
  const size_t mb = (size_t)r->mi_stride * (r->mi_rows + 16);
  r->mi_lg = r->dev<uint8_t>(mb, Byte(4));
  r->mi_skip = r->dev<uint8_t>(mb, Fill::Zero);
  if (r->s6 && r->deblock) {
    r->db_tally = r->dev<int64_t>(3 * 130);
    r->db_dlev = r->dev<uint8_t>(4);
  }
}

// the timing event ring; speed 10: the edge levels' stream and its events
static void alloc_sync(rv_replay *r) {
  for (int f = 0; f < rv_replay::kRing; f++)
    for (int i = 0; i < kEvCount; i++) r->evs[f][i] = r->own.event(hipEventDisableSystemFence);
  if (!r->overlap || !r->lvl || r->s6) return;
  for (hipEvent_t *ev : {&r->ev_efork, &r->ev_l1me, &r->ev_epart})
    *ev = r->own.event(hipEventDisableTiming);
  // one stream for all levels (in order): every stream beyond the hardware
  // queues (GPU_MAX_HW_QUEUES) is multiplexed onto them
  const hipStream_t es = r->own.stream();
  for (int l = 1; l < kLevels; l++) {
    r->edge[l] = es;
    r->ev_ejoin[l] = r->own.event(hipEventDisableTiming);
    r->ev_ecommit[l] = r->own.event(hipEventDisableTiming);
  }
}

// F8: its buffers, the host-mapped token rings, then the coder thread (the
// last thing created, and only if nothing has failed)
static void alloc_entropy(rv_replay *r) {
  if (!r->entropy) return;
  EcFrameBufs &b = r->ecb;
  b.jobs = r->dev<rv_ec_job>((size_t)b.max_jobs);
  b.sb_off = r->dev<uint32_t>((size_t)r->g.nsb + 1);
  b.map = r->dev<uint8_t>((size_t)b.ntiles * 3 * b.map_w4 * b.map_h4);
  b.scratch = r->dev<uint8_t>(rv_ec_scratch_bytes(b.max_jobs));
  b.offsets = r->dev<uint32_t>((size_t)b.max_jobs + 1);
  b.dstat = r->dev<uint32_t>(4);
  EcHost *eh = r->ech = new EcHost();
  eh->ntiles = b.ntiles;
  for (int k = 0; k < 2; k++) {
    eh->tok_h[k] = r->own.pinned<uint32_t>(b.cap, hipHostMallocMapped | hipHostMallocCoherent);
    eh->stat_h[k] = r->own.pinned<uint32_t>((size_t)b.ntiles + 8, hipHostMallocMapped | hipHostMallocCoherent);
    // blocking sync: the coder thread sleeps instead of spinning on the GPU
    eh->ev[k] = r->own.event(hipEventBlockingSync | hipEventDisableTiming);
  }
  if (!r->own.failed) eh->th = std::thread([eh] { eh->run(); });
}

}  // namespace rv

extern "C" {

void rv_replay_destroy(rv_replay *r) {
  if (!r) return;
  la_engine_destroy(r);  // its thread first: it launches on the replay's arrays
  // the streams drain before anything they may still read is freed
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  if (r->ech) {  // the host coder finishes the frames it holds, then stops
    {
      std::lock_guard<std::mutex> lk(r->ech->mu);
      r->ech->stop = true;
    }
    r->ech->cv.notify_all();
    if (r->ech->th.joinable()) r->ech->th.join();
    delete r->ech;
  }
  if (r->edge[1]) (void)hipStreamSynchronize(r->edge[1]);
  r->own.release();
  delete r;
}

// share: a primary instance whose DPB and inputs this one borrows
// (rv_replay_create_twin)
static rv_replay *create_impl(const rv_replay_cfg *cfg, void *stream, const rv_replay *share) {
  rv_replay *r = new rv_replay();
  if (replay_configure(cfg, r) != RV_OK) {
    delete r;
    return nullptr;
  }
  r->own_stream = !stream;
  r->stream = stream ? (hipStream_t)stream : r->own.stream();
  if (!r->stream) {
    rv_set_error(RV_EHIP, "rv_replay_create: stream");
    delete r;
    return nullptr;
  }
  alloc_dpb(r, share);
  alloc_superblocks(r);
  alloc_levels(r);
  alloc_intra(r);
  alloc_mvref(r);
  alloc_filters(r);
  alloc_sync(r);
  alloc_entropy(r);
  if (r->own.failed) rv_set_error(RV_EHIP, "rv_replay_create: device allocation failed");
  if (r->own.failed || hipStreamSynchronize(r->stream) != hipSuccess) {
    rv_replay_destroy(r);
    return nullptr;
  }
  return r;
}

rv_replay *rv_replay_create(const rv_replay_cfg *cfg, void *stream) {
  return create_impl(cfg, stream, nullptr);
}

rv_replay *rv_replay_create_twin(rv_replay *primary, void *stream) {
  if (!primary || primary->n_groups > 1) {
    rv_set_error(RV_EINVAL, "rv_replay_create_twin: needs a one-group primary");
    return nullptr;
  }
  rv_replay *r = create_impl(&primary->cfg, stream, primary);
  if (!r) return nullptr;
  for (int l = 0; l < 3; l++) {
    r->lv[l] = primary->lv[l];
    r->db_level[l] = primary->db_level[l];
    r->cdef_str[l][0] = primary->cdef_str[l][0];
    r->cdef_str[l][1] = primary->cdef_str[l][1];
  }
  r->imp = primary->imp;  // owned by the primary
  r->eng = primary->eng;  // so is the importance window's engine
  r->coded = primary->coded;
  return r;
}

int rv_replay_seek(rv_replay *r, long n) {
  if (!r || n < 1) return rv_set_error(RV_EINVAL, "rv_replay_seek: n >= 1");
  r->coded = n;
  return RV_OK;
}

void *rv_replay_stream(rv_replay *r) { return r ? (void *)r->stream : nullptr; }

// The quantizers and lambdas of the frames of pyramid level `level`
// (FrameInvariants::set_quantizers, src/encoder.rs:865-880, from
// QuantizerParameters; the host computes them, rav1e_amd/rate.py).  Every
// level must be set before the first inter frame.
int rv_replay_set_level_params(rv_replay *r, int level, const rv_replay_level_params *p) {
  if (!r || !p || level < 0 || level > 2 || p->base_q_idx < 1 || p->base_q_idx > 255)
    return rv_set_error(RV_EINVAL, "rv_replay_set_level_params: bad arguments");
  rv_replay::Level &L = r->lv[level];
  const int bd = r->g.bd;
  // QuantizationContext::update of write_tx_tree's inter blocks
  // (src/encoder.rs:1925-1931, 1987-1994): per plane dc / ac deltas
  RV_R(rv_quant_ctx(p->base_q_idx, 64 * 64, 0, bd, p->dc_delta_q[0], p->ac_delta_q[0], &L.ql));
  RV_R(rv_quant_ctx(p->base_q_idx, 32 * 32, 0, bd, p->dc_delta_q[1], p->ac_delta_q[1], &L.qu));
  RV_R(rv_quant_ctx(p->base_q_idx, 32 * 32, 0, bd, p->dc_delta_q[2], p->ac_delta_q[2], &L.qv));
  RV_R(rv_quant_ctx(p->base_q_idx, 64 * 64, 1, bd, p->dc_delta_q[0], p->ac_delta_q[0], &L.qil));
  RV_R(rv_quant_ctx(p->base_q_idx, 32 * 32, 1, bd, p->dc_delta_q[1], p->ac_delta_q[1], &L.qiu));
  RV_R(rv_quant_ctx(p->base_q_idx, 32 * 32, 1, bd, p->dc_delta_q[2], p->ac_delta_q[2], &L.qiv));
  for (int l = 1; r->lvl && l < kLevels; l++) {  // the levels' smaller transforms
    const rv_replay::PLevel &P = r->pl[l];
    RV_R(rv_quant_ctx(p->base_q_idx, P.B * P.B, 0, bd, p->dc_delta_q[0], p->ac_delta_q[0], &L.qs[l][0]));
    for (int c = 1; c < 3; c++)
      RV_R(rv_quant_ctx(p->base_q_idx, P.bc * P.bch, 0, bd, p->dc_delta_q[c], p->ac_delta_q[c],
                        &L.qs[l][c]));
  }
  if (r->lrf) {  // the level's restoration units must be one superblock (checked before any frame)
    LrfGeo lg;
    RV_R(lrf_geometry(r->g.W, r->g.H, r->g.xdec, r->g.ydec, bd, p->base_q_idx, r->g.tws, r->g.ths, &lg));
  }
  L.qidx = p->base_q_idx;
  // deblock_filter_optimize's fast levels (inter frames at speed 10; speed 6
  // searches them on the device, deblock_slot)
  r->db_level[level] = (uint8_t)rv_deblock_fast_level(rv_q_lookup(1, p->base_q_idx, bd), bd, 0);
  r->cdef_str[level][0] = (uint8_t)(p->cdef_strengths & 0xff);
  r->cdef_str[level][1] = (uint8_t)((p->cdef_strengths >> 8) & 0xff);
  if (r->cdef_str[level][0] > 63 || r->cdef_str[level][1] > 63)
    return rv_set_error(RV_EINVAL, "rv_replay_set_level_params: cdef strength above 63");
  L.lambda = p->lambda;
  L.me_lambda = p->me_lambda;
  for (int i = 0; i < 3; i++) L.ds[i] = p->dist_scale[i];
  L.set = true;
  r->jobs_built = false;
  return RV_OK;
}

int rv_replay_synth_inputs(rv_replay *r, int t0) {
  if (!r) return rv_set_error(RV_EINVAL, "rv_replay_synth_inputs: null");
  for (size_t i = 0; i < r->inputs.size(); i++) {
    const RvInput &in = r->inputs[i];
    RV_R(rv_synth_frame(&in.y, &in.u, &in.v, t0 + (int)i, r->g.bd, r->stream));
  }
  RV_H(hipStreamSynchronize(r->stream));
  return RV_OK;
}

static int copy_plane(rv_replay *r, const rv_plane &p, uint8_t *host, bool to_device) {
  const int px = p.hbd ? 2 : 1;
  uint8_t *dev = (uint8_t *)p.data + ((size_t)p.yorigin * p.stride + p.xorigin) * px;
  if (to_device) {
    RV_H(hipMemcpy2DAsync(dev, (size_t)p.stride * px, host, (size_t)p.width * px,
                          (size_t)p.width * px, p.height, hipMemcpyHostToDevice, r->stream));
    return rv_plane_pad(&p, r->stream);
  }
  RV_H(hipMemcpy2DAsync(host, (size_t)p.width * px, dev, (size_t)p.stride * px,
                        (size_t)p.width * px, p.height, hipMemcpyDeviceToHost, r->stream));
  return RV_OK;
}

static int copy_frame(rv_replay *r, const rv_plane *pl, void *host, bool to_device) {
  const int px = r->g.hbd ? 2 : 1;
  uint8_t *p = (uint8_t *)host;
  for (int k = 0; k < 3; k++) {
    RV_R(copy_plane(r, pl[k], p, to_device));
    p += (size_t)pl[k].width * pl[k].height * px;
  }
  RV_H(hipStreamSynchronize(r->stream));
  return RV_OK;
}

int rv_replay_set_input(rv_replay *r, int idx, const void *host_yuv) {
  if (!r || !host_yuv || idx < 0 || idx >= (int)r->inputs.size())
    return rv_set_error(RV_EINVAL, "rv_replay_set_input: bad index");
  const RvInput &in = r->inputs[idx];
  const rv_plane pl[3] = {in.y, in.u, in.v};
  return copy_frame(r, pl, const_cast<void *>(host_yuv), true);
}

int rv_replay_get_input(rv_replay *r, int idx, void *host_yuv) {
  if (!r || !host_yuv || idx < 0 || idx >= (int)r->inputs.size())
    return rv_set_error(RV_EINVAL, "rv_replay_get_input: bad index");
  const RvInput &in = r->inputs[idx];
  const rv_plane pl[3] = {in.y, in.u, in.v};
  return copy_frame(r, pl, host_yuv, false);
}

// The reconstruction of display frame `display` (it must still be in the
// DPB: the last 12 displays).
int rv_replay_get_recon(rv_replay *r, int display, void *host_yuv) {
  if (!r || !host_yuv || display < 0) return rv_set_error(RV_EINVAL, "rv_replay_get_recon");
  const RvSlot &s = r->slots[display % kSlots];
  const rv_plane pl[3] = {s.y, s.u, s.v};
  return copy_frame(r, pl, host_yuv, false);
}

int rv_replay_set_importances(rv_replay *r, const float *host, int n) {
  if (!r) return rv_set_error(RV_EINVAL, "rv_replay_set_importances: null");
  const int need = r->g.w_imp * r->g.h_imp;
  if (!host) {
    r->imp = nullptr;
    return RV_OK;
  }
  if (n != need) return rv_set_error(RV_EINVAL, "rv_replay_set_importances: size != w_imp * h_imp");
  // A fresh buffer per call, all kept until destroy (on purpose): frames in
  // flight on the non-blocking stream may still read the previous one.
  float *d = r->dev<float>((size_t)need);
  if (!d) return rv_set_error(RV_EHIP, "rv_replay_set_importances: alloc");
  RV_H(hipMemcpy(d, host, (size_t)need * 4, hipMemcpyHostToDevice));
  r->imp = d;
  return RV_OK;
}

// Tile groups of all ranks (rects in superblocks, 4 per group), this
// instance's index among them, and the RCCL communicator (rv_comm_create)
// that all-gathers the reconstructions; comm may be null: then the caller
// moves the packed regions itself (rv_replay_exchange_buffers,
// rv_replay_import).
int rv_replay_set_groups(rv_replay *r, int n_groups, const int32_t *rects, int my_group,
                         void *comm) {
  if (!r || n_groups < 1 || n_groups > kMaxGroups || !rects || my_group < 0 ||
      my_group >= n_groups)
    return rv_set_error(RV_EINVAL, "rv_replay_set_groups: bad groups");
  const Geo &g = r->g;
  if (rects[4 * my_group] != g.tx0 || rects[4 * my_group + 1] != g.ty0 ||
      rects[4 * my_group + 2] != g.tw || rects[4 * my_group + 3] != g.th)
    return rv_set_error(RV_EINVAL, "rv_replay_set_groups: my group != the configured tile group");
  memcpy(r->grects, rects, (size_t)n_groups * 4 * sizeof(int32_t));
  r->n_groups = n_groups;
  r->my_group = my_group;
  size_t most = 0;
  for (int k = 0; k < n_groups; k++) {
    XRect xr[9];
    int nx;
    const size_t b = (size_t)group_rects(r, k, xr, &nx);
    most = b > most ? b : most;
  }
  r->xbytes = (most + 255) / 256 * 256;
  if (n_groups > 1 || comm) {  // one group + a communicator: a 1-rank all-gather
    r->xsend = r->dev<uint8_t>(r->xbytes);
    r->xrecv = r->dev<uint8_t>(r->xbytes * n_groups);
    if (!r->xsend || !r->xrecv) return rv_set_error(RV_EHIP, "rv_replay_set_groups: alloc");
  }
  r->comm = comm;
  return RV_OK;
}

int rv_replay_exchange_buffers(rv_replay *r, void **send, void **recv, size_t *bytes_per_group) {
  if (!r || !send || !recv || !bytes_per_group)
    return rv_set_error(RV_EINVAL, "rv_replay_exchange_buffers: null");
  *send = r->xsend;
  *recv = r->xrecv;
  *bytes_per_group = r->xbytes;
  return RV_OK;
}

// Unpack every other group's region of the last coded frame from the
// gathered buffer (group k at k * bytes_per_group) and pad: the frame is
// then a complete reference on this rank (src/encoder.rs:3411-3429).
int rv_replay_import(rv_replay *r) {
  if (!r) return rv_set_error(RV_EINVAL, "rv_replay_import: null");
  // one group without a communicator, or the key frame (every rank copied
  // its own input): nothing to move
  if ((r->n_groups < 2 && !r->comm) || r->last.is_key) return RV_OK;
  const RvSlot &s = r->slots[r->last.display % kSlots];
  XRect rects[9 * kMaxGroups];
  int n = 0;
  for (int k = 0; k < r->n_groups; k++) {
    if (k == r->my_group) continue;
    XRect xr[9];
    int nx;
    group_rects(r, k, xr, &nx);
    for (int p = 0; p < nx; p++) {
      xr[p].off += (int64_t)k * (int64_t)r->xbytes;
      rects[n++] = xr[p];
    }
  }
  RV_R(xcopy(r, s, rects, n, 1, r->xrecv));
  // the whole frame and its block map are in: deblock it (every rank the
  // same way), then pad
  return filter_slot(r, s, r->inputs[r->last.display % r->inputs.size()], r->last.level);
}

int rv_replay_results(rv_replay *r, uint64_t *host_out, int cap) {
  if (!r || !host_out) return rv_set_error(RV_EINVAL, "rv_replay_results: null");
  const Geo &g = r->g;
  const int nw = (int)r->nwords;
  const int total = nw + 5;
  if (cap < total) return rv_set_error(RV_EINVAL, "rv_replay_results: cap too small");
  // verification checksums of the last coded frame (outside the per-frame work)
  hipStream_t st = r->stream;
  const int64_t nl = (int64_t)g.nsb * 1024, nc = (int64_t)g.nsb * r->ntx_c * 1024;
  RV_H(hipMemsetAsync(r->tail, 0, 2 * 8, st));
  RV_H(hipMemsetAsync(r->tail + 3, 0, 2 * 8, st));
  if (!r->lvl) {
    coeff_checksum<<<1024, 256, 0, st>>>(r->l_lev, nl, 1024, r->tail);
    coeff_checksum<<<1024, 256, 0, st>>>(r->c_lev, 2 * nc, 1024, r->tail);
  } else {  // the committed blocks (leaves) of every level
    coeff_checksum_list<<<1024, 256, 0, st>>>(r->l_lev, r->pl[0].leaf, r->leaf_count, 1024, 1024,
                                              r->tail);
    for (int q = 0; q < 2; q++)
      coeff_checksum_list<<<1024, 256, 0, st>>>(r->c_lev + q * nc, r->pl[0].leaf, r->leaf_count,
                                                r->ntx_c * 1024, 1024, r->tail);
    for (int l = 1; l < kLevels; l++) {
      const rv_replay::PLevel &P = r->pl[l];
      const int pl_ = P.B * P.B, pc = P.bc * P.bch;
      coeff_checksum_list<<<1024, 256, 0, st>>>(P.l_lev, P.leaf, r->leaf_count + l, pl_, pl_,
                                                r->tail);
      for (int q = 0; q < 2; q++)
        coeff_checksum_list<<<1024, 256, 0, st>>>(P.c_lev + (size_t)q * P.n * pc, P.leaf,
                                                  r->leaf_count + l, pc, pc, r->tail);
    }
  }
  const RvSlot &s = r->slots[r->last.display % kSlots];
  const rv_plane *pl[3] = {&s.y, &s.u, &s.v};
  for (int i = 0; i < 3; i++) {
    const rv_plane &p = *pl[i];
    const int xd = i ? g.xdec : 0, yd = i ? g.ydec : 0;
    const int x0 = (g.tx0 * kSb) >> xd, y0 = (g.ty0 * kSb) >> yd;
    int x1 = ((g.tx0 + g.tw) * kSb) >> xd, y1 = ((g.ty0 + g.th) * kSb) >> yd;
    x1 = x1 < p.width ? x1 : p.width;
    y1 = y1 < p.height ? y1 : p.height;
    // the group's region, and (after the exchange) the whole frame
    if (g.hbd) {
      sum_rect<uint16_t><<<1024, 256, 0, st>>>(p, x0, y0, x1 - x0, y1 - y0, r->tail + 1);
      sum_rect<uint16_t><<<1024, 256, 0, st>>>(p, 0, 0, p.width, p.height, r->tail + 4);
    } else {
      sum_rect<uint8_t><<<1024, 256, 0, st>>>(p, x0, y0, x1 - x0, y1 - y0, r->tail + 1);
      sum_rect<uint8_t><<<1024, 256, 0, st>>>(p, 0, 0, p.width, p.height, r->tail + 4);
    }
  }
  RV_H(hipGetLastError());
  RV_H(hipMemcpyAsync(host_out, r->words, (size_t)nw * 8, hipMemcpyDeviceToHost, st));
  RV_H(hipMemcpyAsync(host_out + nw, r->tail, 5 * 8, hipMemcpyDeviceToHost, st));
  RV_H(hipStreamSynchronize(st));
  host_out[nw + 3] = (uint64_t)r->n_imp;
  return total;
}

static int stage_times(rv_replay *r, float *ms_out, int cap, int last) {
  if (!r || !ms_out) return rv_set_error(RV_EINVAL, "rv_replay_stage_times: null");
  if (r->timed == 0) return rv_set_error(RV_EINVAL, "rv_replay_stage_times: no timed frame");
  if (last < 1) last = 1;
  if (last > rv_replay::kRing) last = rv_replay::kRing;
  if (last > r->timed) last = (int)r->timed;
  for (int i = 0; i < cap && i < kEvLaBegin; i++) ms_out[i] = 0.f;
  // after the main stream's stages: the lookahead's own span, the edge
  // levels' (speed 10, beside F3 .. F4), F8's coefficient tokens
  const StageEv spans[3][2] = {
      {kEvLaBegin, kEvLaEnd}, {kEvEdgeBegin, kEvEdgeEnd}, {kEvF8Begin, kEvF8End}};
  const int nspans = r->entropy ? 3 : 2;
  int n = 0;
  for (int f = 0; f < last; f++) {
    hipEvent_t *e = r->evs[(r->timed - 1 - f) % rv_replay::kRing];
    RV_H(hipEventSynchronize(e[kEvF7]));
    n = 0;
    for (int i = kEvStart; i < kEvF7 && n < cap; i++) {
      float ms = 0.f;
      RV_H(hipEventElapsedTime(&ms, e[i], e[i + 1]));
      ms_out[n++] += ms;
    }
    for (int k = 0; k < nspans && n < cap; k++) {
      float ms = 0.f;
      RV_H(hipEventSynchronize(e[spans[k][1]]));
      RV_H(hipEventElapsedTime(&ms, e[spans[k][0]], e[spans[k][1]]));
      ms_out[n++] += ms;
    }
  }
  return n;
}

int rv_replay_entropy_stats(rv_replay *r, uint64_t *out, int cap) {
  if (!r || !out || cap < 4) return rv_set_error(RV_EINVAL, "rv_replay_entropy_stats: null / cap");
  if (!r->ech) return rv_set_error(RV_EINVAL, "rv_replay_entropy_stats: RV_REPLAY_ENTROPY off");
  r->ech->drain();
  if (r->ech->err) return rv_set_error(r->ech->err, "rv_replay_entropy_stats: token buffer overflow");
  const int n = cap < 5 ? cap : 5;
  for (int i = 0; i < n; i++) out[i] = r->ech->stat[i];
  return n;
}

int rv_replay_set_timing(rv_replay *r, int stride, int block) {
  if (!r || stride < 0 || block < 1)
    return rv_set_error(RV_EINVAL, "rv_replay_set_timing: bad stride / block");
  r->timing_stride = stride;
  r->timing_block = block;
  return RV_OK;
}

int rv_replay_stage_times(rv_replay *r, float *ms_out, int cap) {
  return stage_times(r, ms_out, cap, 1);
}
int rv_replay_stage_times_sum(rv_replay *r, int last_frames, float *ms_out, int cap) {
  return stage_times(r, ms_out, cap, last_frames);
}

// The kernel probe: on (re)start, the sums so far are dropped (the pairs in
// flight are waited for); off stops recording.
int rv_replay_set_kernel_probe(rv_replay *r, int on) {
  if (!r) return rv_set_error(RV_EINVAL, "rv_replay_set_kernel_probe: null");
  constexpr int P = rv_replay::kProbes, C = rv_replay::kKpCnt;
  if (on && r->kp_ev[0].empty()) {
    for (int p = 0; p < P; p++) {
      r->kp_ev[p].assign(2 * rv_replay::kKp, nullptr);
      for (auto &ev : r->kp_ev[p]) ev = r->own.event(hipEventDefault);
      r->kp_cnt[p] = r->dev<uint32_t>(C);
      r->kp_ts[p] = r->dev<unsigned long long>(2 * rv_replay::kKp);
      if (r->own.failed)
        return rv_set_error(RV_EHIP, "rv_replay_set_kernel_probe: allocation failed");
    }
    int dev = 0, khz = 0;
    RV_H(hipGetDevice(&dev));
    RV_H(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
    r->kp_tick_ms = khz > 0 ? 1.0 / (double)khz : 0.0;
  }
  if (!r->kp_ev[0].empty()) {
    for (int p = 0; p < P; p++) RV_H(kp_harvest(r, p, r->kp_n[p]));
    RV_H(hipDeviceSynchronize());
    for (int p = 0; p < P; p++) RV_H(hipMemset(r->kp_cnt[p], 0, C * sizeof(uint32_t)));
    RV_H(hipDeviceSynchronize());
  }
  for (int p = 0; p < P; p++) {
    r->kp_ms[p] = 0.0;
    r->kp_dev_ms[p] = 0.0;
    r->kp_base[p] = r->kp_n[p];
  }
  r->kprobe = on != 0;
  return RV_OK;
}

// probe 0: out[0] launches, [1] their summed milliseconds (event pairs on
// their streams), [2] candidate evaluations, [3] jobs, [4] device-clock ms;
// probe 1 (cap >= 11): out[5] launches, [6] event ms, [7] device-clock ms,
// [8] single / [9] compound luma candidates, [10] single chroma transform
// blocks, [11] compound ones (cap >= 12)
int rv_replay_kernel_probe(rv_replay *r, double *out, int cap) {
  if (!r || !out || cap < 4) return rv_set_error(RV_EINVAL, "rv_replay_kernel_probe: null / cap");
  const int nout = cap >= 12 ? 12 : cap < 5 ? 4 : 5;
  for (int i = 0; i < nout; i++) out[i] = 0.0;
  if (r->kp_ev[0].empty()) return nout;
  for (int p = 0; p < rv_replay::kProbes; p++) RV_H(kp_harvest(r, p, r->kp_n[p]));
  uint32_t c[2][rv_replay::kKpCnt] = {{0}};
  RV_H(hipDeviceSynchronize());
  for (int p = 0; p < rv_replay::kProbes; p++)
    RV_H(hipMemcpy(c[p], r->kp_cnt[p], sizeof(c[p]), hipMemcpyDeviceToHost));
  out[0] = (double)(r->kp_n[0] - r->kp_base[0]);
  out[1] = r->kp_ms[0];
  out[2] = (double)c[0][0];
  out[3] = (double)c[0][1];
  if (nout > 4) out[4] = r->kp_dev_ms[0];
  if (nout >= 12) {
    out[5] = (double)(r->kp_n[1] - r->kp_base[1]);
    out[6] = r->kp_ms[1];
    out[7] = r->kp_dev_ms[1];
    for (int i = 0; i < 4; i++) out[8 + i] = (double)c[1][i];
  }
  return nout;
}
// Candidate evaluations summed over the last min(frames, 64) coded frames:
// out[0] F3 full-pel diamond, out[1] F3 sub-pel diamond (64x64 jobs), out[2]
// frames summed, (cap >= 5) out[3] / out[4] the F4 single-reference /
// compound RDO candidates of the 64x64 blocks, (cap >= 11, speed 6) out[5 +
// 2 (l - 1)] / out[6 + 2 (l - 1)] those of the 32x32, 16x16, 8x8 blocks.
int rv_replay_dpb_slots(void) { return kSlots; }

int rv_replay_counters(rv_replay *r, uint64_t *out, int cap) {
  if (!r || !out || cap < 3) return rv_set_error(RV_EINVAL, "rv_replay_counters");
  const Geo &g = r->g;
  const int nj = g.nsb * g.R;
  const long nonkey = r->coded > 0 ? r->coded - 1 : 0;
  const int nf = nonkey < rv_replay::kRing ? (int)nonkey : rv_replay::kRing;
  RV_H(hipStreamSynchronize(r->stream));
  std::vector<uint32_t> h((size_t)nf * 2 * nj);
  if (nf) RV_H(hipMemcpy(h.data(), r->ds_evals, h.size() * 4, hipMemcpyDeviceToHost));
  out[0] = out[1] = 0;
  for (int f = 0; f < nf; f++)
    for (int k = 0; k < 2; k++)
      for (int j = 0; j < nj; j++) out[k] += h[((size_t)f * 2 + k) * nj + j];
  out[2] = (uint64_t)nf;
  if (cap < 5) return 3;
  const int nl = cap >= 11 ? kLevels : 1;
  std::vector<uint32_t> ce((size_t)nf * 2 * kLevels);
  if (nf) RV_H(hipMemcpy(ce.data(), r->cand_evals, ce.size() * 4, hipMemcpyDeviceToHost));
  for (int l = 0; l < nl; l++) {
    uint64_t &a = out[l ? 5 + 2 * (l - 1) : 3], &b = out[l ? 6 + 2 * (l - 1) : 4];
    a = b = 0;
    for (int f = 0; f < nf; f++) {
      a += ce[(size_t)(f * kLevels + l) * 2];
      b += ce[(size_t)(f * kLevels + l) * 2 + 1];
    }
  }
  if (cap < 14) return nl == 1 ? 5 : 11;
  std::vector<uint32_t> is((size_t)nf * 3);
  if (nf) RV_H(hipMemcpy(is.data(), r->i_stats, is.size() * 4, hipMemcpyDeviceToHost));
  out[11] = out[12] = out[13] = 0;
  for (int f = 0; f < nf; f++)
    for (int k = 0; k < 3; k++) out[11 + k] += is[(size_t)f * 3 + k];
  if (cap < 17) return 14;
  // speed 10 MV-stack rounds since creation: rounds (F3 + F4 launches),
  // superblock re-evaluations after the first round, frames
  out[14] = (uint64_t)r->mv_round_sum;
  out[15] = (uint64_t)r->mv_reeval;
  out[16] = (uint64_t)r->mv_frames;
  if (cap < 18) return 17;
  // round runs: 1 + the MV / intra passes (the joint fixed point's outer
  // iterations), summed over frames
  out[17] = (uint64_t)r->mv_run_sum;
  if (cap < 20) return 18;
  // the lookahead's EPZS rounds and re-run jobs (the engine's on its owner)
  const bool own_eng = r->eng && r->eng_owned;
  long er = 0, ere = 0, ef = 0;
  if (own_eng) {
    std::lock_guard<std::mutex> lk(r->eng->mu);
    er = r->eng->la_round_sum;
    ere = r->eng->la_reeval;
    ef = r->eng->la_frames;
  }
  out[18] = (uint64_t)(r->la_round_sum + er);
  out[19] = (uint64_t)(r->la_reeval + ere);
  if (cap < 21) return 20;
  // the frames those lookahead rounds belong to (the engine runs ahead of
  // the encode: up to W frames past the last coded one)
  out[20] = (uint64_t)(r->la_frames + ef);
  return 21;
}

// Host-only test hook: the slots RoundRing gives check q -- out[0] the
// device count slot it counts into, out[1] the slot it zeroes for check
// q + 1, out[2] its host publication slot -- and out[3] kRoundsAhead,
// out[4] kCnt, out[5] kPub (cap >= 6).  Returns 6.
int rv_round_ring_slots(uint32_t q, int32_t *out, int cap) {
  if (!out || cap < 6) return rv_set_error(RV_EINVAL, "rv_round_ring_slots: cap");
  static int32_t cnt[2 * RoundRing::kCnt + 1];
  static unsigned long long pub[RoundRing::kPub];
  RoundRing rr;
  rr.cnt = cnt;
  rr.d_pub = pub;
  const RoundPub p = rr.pub(q);
  out[0] = (int32_t)((p.cnt - cnt) / 2);
  out[1] = (int32_t)((p.next - cnt) / 2);
  out[2] = (int32_t)(p.host - pub);
  out[3] = rv_replay::kRoundsAhead;
  out[4] = RoundRing::kCnt;
  out[5] = RoundRing::kPub;
  return 6;
}

// Host-only test hook: the lookahead references of coded frame m >= 1
// (la_refs_of): out[0] = n, out[1..3] their displays in k order, out[4..6]
// the propagation order (-1: unused).  Returns 0.
// RV_REPLAY_LRF: the last coded frame's loop-restoration units of plane p,
// (set, xqd0, xqd1) per unit in raster order (set -1: None); synchronous
int rv_replay_lrf_units(rv_replay *r, int plane, int8_t *out, int cap) {
  if (!r || !out || plane < 0 || plane > 2) return rv_set_error(RV_EINVAL, "rv_replay_lrf_units: bad arguments");
  if (!r->lrf) return rv_set_error(RV_EINVAL, "rv_replay_lrf_units: RV_REPLAY_LRF is off");
  const Geo &g = r->g;
  const int nsb = ((g.W + 63) / 64) * ((g.H + 63) / 64);
  if (cap < 3 * nsb) return rv_set_error(RV_EINVAL, "rv_replay_lrf_units: cap < 3 * superblocks");
  RV_H(hipStreamSynchronize(r->stream));
  RV_H(hipMemcpy(out, r->lrf_units + (size_t)plane * nsb * 3, (size_t)nsb * 3, hipMemcpyDeviceToHost));
  return RV_OK;
}

int rv_replay_la_refs(long m, int R, int32_t *out) {
  if (!out || m < 1 || R < 1 || R > 2) return rv_set_error(RV_EINVAL, "rv_replay_la_refs");
  const LaRefs l = la_refs_of(m, R);
  out[0] = l.n;
  for (int k = 0; k < 3; k++) {
    out[1 + k] = k < l.n ? l.disp[k] : -1;
    out[4 + k] = k < l.n ? l.order[k] : -1;
  }
  return RV_OK;
}

// ---- RCCL communicator for the tile-group exchange ---------------------------
int rv_comm_unique_id(uint8_t *out, int cap) {
#if RV_HAVE_RCCL
  if (!out || cap < (int)sizeof(ncclUniqueId)) return rv_set_error(RV_EINVAL, "rv_comm_unique_id");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return rv_set_error(RV_EHIP, "ncclGetUniqueId");
  memcpy(out, &id, sizeof(id));
  return (int)sizeof(id);
#else
  (void)out;
  (void)cap;
  return rv_set_error(RV_EINVAL, "rv_comm_unique_id: built without RCCL");
#endif
}

void *rv_comm_create(const uint8_t *id, int nranks, int rank) {
#if RV_HAVE_RCCL
  if (!id || nranks < 1 || rank < 0 || rank >= nranks) {
    rv_set_error(RV_EINVAL, "rv_comm_create");
    return nullptr;
  }
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  ncclComm_t c = nullptr;
  if (ncclCommInitRank(&c, nranks, u, rank) != ncclSuccess) {
    rv_set_error(RV_EHIP, "ncclCommInitRank");
    return nullptr;
  }
  return c;
#else
  (void)id;
  (void)nranks;
  (void)rank;
  rv_set_error(RV_EINVAL, "rv_comm_create: built without RCCL");
  return nullptr;
#endif
}

void rv_comm_destroy(void *comm) {
#if RV_HAVE_RCCL
  if (comm) (void)ncclCommDestroy((ncclComm_t)comm);
#else
  (void)comm;
#endif
}

}  // extern "C"

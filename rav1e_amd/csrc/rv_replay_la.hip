// rv_replay_la.hip -- the replay's lookahead: one frame's lookahead with its
// EPZS rounds (lookahead_frame, la_check_kernel), the lookahead engine of an
// importance window (its thread, la_step, what the encode takes from it and
// releases), and the exchanges of the engines' frame parts between tile
// groups (the in-process hub, RCCL).
#include "rv_replay.h"

namespace rv {

// ---- the lookahead's EPZS rounds ---------------------------------------------
// compute_lookahead_motion_vectors (src/api/internal.rs:514-622) searches a
// tile's superblocks in raster order, first every build_half_res_pmvs
// (F2L: four 32x32 quadrants at half resolution), then every
// build_full_res_pmvs (FL: sixteen 16x16 blocks), each from
// get_subset_predictors over the lookahead's own tile field, which starts
// at zero and takes the quadrants' and then the 16x16 blocks' MVs as they
// are found (save_block_motion); its references carry no field (no subset
// C).  A check recomputes every job's set from the current results and
// lists the jobs whose set changed; a round re-runs them.
struct LaArgs {
  Geo g;
  EpzsGeo eg;
  rv_ds_job *jh, *jl;            // F2L jobs [R][nsb][4], FL jobs [R][nsb][16]
  const int32_t *sl;             // FL's cmv sources (8 per job, fill_preds_kernel's code)
  const rv_fs_result *coarse, *half_l, *look;
  int32_t *list_h, *list_l;      // out: the marked F2L / FL jobs
  int init;                      // 1: store the sets, mark nothing
  int what;                      // bit 0: the F2L jobs, bit 1: the FL jobs
  int nref;                      // the lookahead's references (LaRefs::n)
  RoundPub pub;                  // pub.cnt: [F2L marked, FL marked]
};

__device__ inline rv_mv la_coarse4(const LaArgs &a, int k, int sb) {
  const rv_mv c = a.coarse[(size_t)k * a.g.nsb + sb].best_mv;
  return rv_mv{(int16_t)(c.row * 4), (int16_t)(c.col * 4)};
}

__global__ __launch_bounds__(256) void la_check_kernel(LaArgs a) {
  const Geo &g = a.g;
  const int nh = (a.what & 1) ? a.nref * g.nsb * 4 : 0, nl = (a.what & 2) ? a.nref * g.nsb * 16 : 0;
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool mh = false, ml = false;
  int job = 0;
  if (i < nh) {  // F2L: me_ss2 of quadrant q (src/me.rs:465-519)
    job = i;
    const int k = i / (g.nsb * 4), sb = (i / 4) % g.nsb, q = i % 4;
    const int sx = sb % g.tw, sy = sb / g.tw;
    int t0x, t0y, mi_w, mi_h;
    sb_tile(g, sx, sy, t0x, t0y, mi_w, mi_h);
    const int fsx = g.tx0 + sx, fsy = g.ty0 + sy, tsx = fsx - t0x, tsy = fsy - t0y;
    const int tsw = (mi_w + 15) / 16, tsh = (mi_h + 15) / 16;
    const bool hh = (q & 1) ? tsx < tsw - 1 : tsx > 0, hv = (q >> 1) ? tsy < tsh - 1 : tsy > 0;
    const rv_mv ch = hh ? la_coarse4(a, k, (q & 1) ? sb + 1 : sb - 1) : rv_mv{0, 0};
    const rv_mv cv = hv ? la_coarse4(a, k, (q >> 1) ? sb + g.tw : sb - g.tw) : rv_mv{0, 0};
    const rv_mv cm[3] = {la_coarse4(a, k, sb), hh ? ch : cv, cv};  // static slots
    const int nc = 1 + (int)hh + (int)hv;
    int bx = tsx * 16 + (q & 1) * 8, by = tsy * 16 + (q >> 1) * 8;
    adjust_bo(mi_w, mi_h, bx, by, 32, 32);
    // the field: an earlier superblock's quadrant MV (estimate_motion_ss2's *
    // 2), zero inside this one (its quadrants are saved after all four)
    auto rd = [&](int X4, int Y4) {
      const int SX = X4 >> 4, SY = Y4 >> 4;
      if (SX == fsx && SY == fsy) return rv_mv{0, 0};
      const int gsb = (SY - g.ty0) * g.tw + (SX - g.tx0);
      const rv_mv h =
          a.half_l[((size_t)k * g.nsb + gsb) * 4 + ((Y4 >> 3) & 1) * 2 + ((X4 >> 3) & 1)].best_mv;
      return rv_mv{(int16_t)(h.row * 2), (int16_t)(h.col * 2)};
    };
    mh = epzs_update(a.jh + i, 1, a.eg, t0x * 16, t0y * 16, mi_w, bx, by, cm, nc, rd, nullptr, 1) &&
         !a.init;
  } else if (i - nh < nl) {  // FL: estimate_motion of 16x16 block b (src/me.rs:337-390)
    const int j = i - nh;
    job = j;
    const int k = j / (g.nsb * 16), sb = (j / 16) % g.nsb, b = j % 16;
    const int sx = sb % g.tw, sy = sb / g.tw;
    int t0x, t0y, mi_w, mi_h;
    sb_tile(g, sx, sy, t0x, t0y, mi_w, mi_h);
    const int tsx = g.tx0 + sx - t0x, tsy = g.ty0 + sy - t0y;
    rv_mv cm[6];
    int nc = 0;
    bool more = true;
#pragma unroll
    for (int p = 1; p < 7; p++) {  // the coarse MV, the covering quadrant, 4 neighbours' (a prefix)
      const int v = more ? a.sl[8 * j + p] : -1;
      more = more && v >= 0;
      const rv_mv m = !more ? rv_mv{0, 0}
                            : (v & 1) ? a.half_l[v >> 1].best_mv : a.coarse[v >> 1].best_mv;
      const int sc = (v & 1) ? 2 : 4;
      cm[p - 1] = rv_mv{(int16_t)(m.row * sc), (int16_t)(m.col * sc)};
      nc += more ? 1 : 0;
    }
    int bx = tsx * 16 + (b % 4) * 4, by = tsy * 16 + (b / 4) * 4;
    adjust_bo(mi_w, mi_h, bx, by, 16, 16);
    // the field: the 16x16 block holding the unit (every block read comes
    // before this one in raster order, so it holds its FL MV)
    auto rd = [&](int X4, int Y4) {
      const int gsb = ((Y4 >> 4) - g.ty0) * g.tw + ((X4 >> 4) - g.tx0);
      return a.look[((size_t)k * g.nsb + gsb) * 16 + ((Y4 & 15) >> 2) * 4 + ((X4 & 15) >> 2)]
          .best_mv;
    };
    ml = epzs_update(a.jl + j, 0, a.eg, t0x * 16, t0y * 16, mi_w, bx, by, cm, nc, rd, nullptr, 1) &&
         !a.init;
  }
  const int lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1;
  const uint64_t bh = __ballot(mh), bl = __ballot(ml);
  int b0 = 0, b1 = 0;
  if (lane == 0) {
    if (bh) b0 = atomicAdd(a.pub.cnt, (int)__popcll(bh));
    if (bl) b1 = atomicAdd(a.pub.cnt + 1, (int)__popcll(bl));
  }
  b0 = __shfl(b0, 0, 64);
  b1 = __shfl(b1, 0, 64);
  if (mh) a.list_h[b0 + __popcll(bh & below)] = job;
  if (ml) a.list_l[b1 + __popcll(bl & below)] = job;
  round_publish(a.pub);
}

// The lookahead of coded frame fi (compute_lookahead_motion_vectors,
// src/api/internal.rs:514-622) on stream xs: F0 the input's hres / qres
// (pyramid: false when they are already current), F1 build_coarse_pmvs,
// then F2L + FL (build_half_res_pmvs / build_full_res_pmvs) with their EPZS
// sets (la_check_kernel): round 0 stores every F2L set (the field guessed
// from o's previous contents) and runs every F2L search, then the same for
// FL; then the rounds.  Budget: a quadrant search reads the quadrants of
// the superblocks left of and above it, so it settles by round tws + ths - 1;
// a 16x16 search reads its coarse / quadrant predictors (settled by then)
// and the 16x16 blocks left of and above it, so it settles 4 tws + 4 ths - 2
// rounds later.  e: the frame's timing events (null: untimed).
int lookahead_frame(rv_replay *r, RoundRing &rr, hipStream_t xs,
                    const rv_replay_frame_info &fi, const LaRefs &lr, long frame,
                    const LaOut &o, int32_t *la_list, bool pyramid, long *nrounds,
                    long *nre, hipEvent_t *e) {
  const Geo &g = r->g;
  const int lv = fi.level, nr = g.nsb, RL = lr.n;
  const RvInput &cur = r->inputs[fi.display % r->inputs.size()];
  rv_plane refs_h[kImpMaxRefs], refs_q[kImpMaxRefs], refs_o[kImpMaxRefs];
  const uint32_t *box[kImpMaxRefs];
  for (int k = 0; k < RL; k++) {
    const RvInput &ri = r->inputs[lr.disp[k] % r->inputs.size()];
    refs_h[k] = ri.hres;
    refs_q[k] = ri.qres;
    refs_o[k] = ri.y;  // the lookahead searches the references' original frames
    box[k] = ri.qres_box;
  }
  auto ev = [&](StageEv i) -> int {
    if (e) RV_H(hipEventRecord(e[i], xs));
    return RV_OK;
  };
  if (pyramid) {  // F0 (encode_frame, src/encoder.rs:3382-3385)
    RV_R(rv_plane_pyramid(&cur.y, &cur.hres, &cur.qres, xs));
    if (r->sea) RV_R(rv_plane_box_sums(&cur.qres, cur.qres_box, xs));
  }
  RV_R(ev(kEvF0));
  // F1 coarse full search (build_coarse_pmvs), every reference in one launch
  RV_R(rv_full_search_multi(&cur.qres, refs_q, RL, r->fs_jobs[lv], nr, 16, 16, 1, 0, o.coarse,
                            nullptr, r->sea ? box : nullptr, xs));
  RV_R(ev(kEvF1));
  LaArgs la_a;
  memset(&la_a, 0, sizeof(la_a));
  la_a.g = g;
  la_a.eg = EpzsGeo{g.tx0, g.ty0, g.tw, g.th, g.tws, g.ths, g.W, g.H, g.w_in_b, g.h_in_b};
  la_a.jh = r->jobs_half_l[lv];
  la_a.jl = r->jobs_look[lv];
  la_a.sl = r->src_look;
  la_a.coarse = o.coarse;
  la_a.half_l = o.half_l;
  la_a.look = o.look;
  const int nh = nr * RL * 4, nl = nr * RL * 16;
  la_a.nref = RL;
  la_a.list_h = la_list;
  la_a.list_l = la_list + nh;
  auto la_launch = [&](int what, uint32_t q, bool init) -> int {
    la_a.what = what;
    la_a.init = init ? 1 : 0;
    la_a.pub = rr.pub(q, !init);
    const int n = ((what & 1) ? nh : 0) + ((what & 2) ? nl : 0);
    la_check_kernel<<<(n + 255) / 256, 256, 0, xs>>>(la_a);
    RV_H(hipGetLastError());
    return RV_OK;
  };
  auto f2l = [&](const int32_t *list, const int32_t *cnt) {
    return rv_diamond_search_multi(&cur.hres, refs_h, RL, r->jobs_half_l[lv], nr * 4, 16, 16, 0,
                                   0, 0, g.bd, o.half_l, nullptr, nullptr, xs, nullptr, list, cnt,
                                   0);
  };
  auto fl = [&](const int32_t *list, const int32_t *cnt) {
    return rv_diamond_search_multi(&cur.y, refs_o, RL, r->jobs_look[lv], nr * 16, 16, 16, 0, 0, 0,
                                   g.bd, o.look, nullptr, nullptr, xs, nullptr, list, cnt, 0);
  };
  RV_R(la_launch(1, 0, true));
  RV_R(f2l(nullptr, nullptr));
  RV_R(ev(kEvF2));
  RV_R(ev(kEvLaBegin));
  RV_R(la_launch(2, 0, true));
  RV_R(fl(nullptr, nullptr));
  (*nrounds)++;
  RV_R(run_rounds(
      rr, xs, 5 * (g.tws + g.ths), [&](uint32_t q) { return la_launch(3, q, false); },
      [&](uint32_t q) -> int {
        RV_R(f2l(la_list, rr.slot(q)));
        return fl(la_list + nh, rr.slot(q) + 1);
      },
      nrounds, nre, nullptr, "lookahead", frame, lv));
  RV_R(ev(kEvLaEnd));
  return RV_OK;
}

// the coded index of display d (frame_info's inverse)
static long coded_of_display(long d) {
  if (d == 0) return 0;
  static const int jof[4] = {0, 2, 1, 3}, off[4] = {4, 2, 1, 3};
  const int j = jof[d % 4];
  return 4 * ((d - off[j]) / 4) + j + 1;
}

// Several tile groups: every group's part of frame m's importance data into
// every group's entry (the propagation reads the whole frame).  One group
// covering the frame: nothing to do.
static int la_exchange(rv_replay *r, long m, RvLaEngine::Entry &e, int R, hipStream_t xs) {
  RvLaEngine &E = *r->eng;
  const Geo &g = r->g;
  const int ng = r->n_groups;
  if (ng <= 1 && !E.comm) {
    if (g.tx0 || g.ty0 || g.vis_w != g.W || g.vis_h != g.H)
      return rv_set_error(RV_EINVAL, "rv_replay_frame: a tile group's window needs the other groups "
                                     "(rv_replay_set_groups + rv_replay_set_la_exchange)");
    return RV_OK;
  }
  auto rect = [&](int j) { return r->grects + 4 * j; };
  (void)R;
  if (E.comm) {  // the encode thread all-gathers (la_encode_exchange)
    RV_H(hipEventRecord(e.ev_data, xs));
    std::unique_lock<std::mutex> lk(E.mu);
    E.data_ready = m;
    E.cv.notify_all();
    if (!E.cv.wait_for(lk, std::chrono::seconds(kEngineWaitS),
                       [&] { return E.stop || E.xchg_done >= m; }))
      return rv_set_error(RV_EHIP, "la_exchange: the frame's parts were never all-gathered");
    if (E.stop) return rv_set_error(RV_EINVAL, "la_exchange: stopped");
    lk.unlock();
    RV_H(hipStreamWaitEvent(xs, e.ev_xchg, 0));
    return RV_OK;
  }
  rv_la_hub *h = E.hub;
  if (!h || h->n != ng)
    return rv_set_error(RV_EINVAL, "rv_replay_frame: a tile group's window needs an exchange "
                                   "(rv_replay_set_la_exchange)");
  const int k = E.hub_k, slot = (int)(m % rv_la_hub::kRing);
  const int32_t *me = rect(k);
  RV_R(impwin_part(e.f, R, me[0], me[1], me[2], me[3], g.w_imp, g.h_imp, h->buf[slot][k], false, xs));
  RV_H(hipEventRecord(h->ev[slot][k], xs));
  {
    std::unique_lock<std::mutex> lk(h->mu);
    h->posted[k] = m;
    h->cv.notify_all();
    if (!h->cv.wait_for(lk, std::chrono::seconds(kEngineWaitS), [&] {
          for (int j = 0; j < ng; j++)
            if (h->posted[j] < m) return false;
          return true;
        }))
      return rv_set_error(RV_EHIP, "la_exchange: a group's part never arrived");
  }
  for (int j = 0; j < ng; j++) {
    if (j == k) continue;
    RV_H(hipStreamWaitEvent(xs, h->ev[slot][j], 0));
    RV_R(impwin_part(e.f, R, rect(j)[0], rect(j)[1], rect(j)[2], rect(j)[3], g.w_imp, g.h_imp,
                     h->buf[slot][j], true, xs));
  }
  return RV_OK;
}

// One step of the engine: coded frame m's lookahead and importance data
// into its entry, then the window propagation of every frame whose window
// is now complete (n + W = m, or the stream's last frame).
static int la_step(rv_replay *r, long m) {
  RvLaEngine &E = *r->eng;
  const Geo &g = r->g;
  hipStream_t xs = E.las;
  RvLaEngine::Entry &e = E.at(m);
  if (m - E.RW >= 1) RV_H(hipStreamWaitEvent(xs, e.ev_used, 0));  // frame m - RW is done with it
  rv_replay_frame_info fi;
  frame_info(m, g.R, &fi);
  const LaRefs lr = la_refs_of(m, g.R);
  // the pyramids of the frame's and its lookahead references' inputs
  long ds[1 + kImpMaxRefs];
  int nd = 0;
  ds[nd++] = fi.display;
  for (int k = 0; k < lr.n; k++) ds[nd++] = lr.disp[k];
  for (int i = 0; i < nd; i++) {
    const size_t idx = (size_t)(ds[i] % (long)r->inputs.size());
    if (E.pyr_display[idx] == ds[i]) continue;
    const RvInput &in = r->inputs[idx];
    RV_R(rv_plane_pyramid(&in.y, &in.hres, &in.qres, xs));
    if (r->sea) RV_R(rv_plane_box_sums(&in.qres, in.qres_box, xs));
    E.pyr_display[idx] = ds[i];
  }
  const size_t nr = (size_t)g.nsb * lr.n;
  if (m > 1) {  // the field's first guess: the previous frame's lookahead
    const RvLaEngine::Entry &p = E.at(m - 1);
    RV_H(hipMemcpyAsync(e.o.half_l, p.o.half_l, nr * 4 * sizeof(rv_fs_result),
                        hipMemcpyDeviceToDevice, xs));
    RV_H(hipMemcpyAsync(e.o.look, p.o.look, nr * 16 * sizeof(rv_fs_result),
                        hipMemcpyDeviceToDevice, xs));
  }
  long la_rounds = 0, la_reeval = 0;
  RV_R(lookahead_frame(r, E.rr, xs, fi, lr, m - 1, e.o, E.la_list, false, &la_rounds, &la_reeval,
                       nullptr));
  {
    std::lock_guard<std::mutex> lk(E.mu);
    E.la_round_sum += la_rounds;
    E.la_reeval += la_reeval;
    E.la_frames++;
  }
  rv_plane refs_o[kImpMaxRefs];
  for (int k = 0; k < lr.n; k++) refs_o[k] = r->inputs[lr.disp[k] % r->inputs.size()].y;
  // the entry is frame m's from here on (the encode's part exchange reads it)
  e.m = m;
  e.fi = fi;
  e.lr = lr;
  RV_R(impwin_group_data(r->inputs[fi.display % r->inputs.size()].y, refs_o, lr.n, g.bd, e.o.look,
                         g.tx0, g.ty0, g.tw, g.th, g.w_imp, g.h_imp, e.f, xs));
  RV_R(la_exchange(r, m, e, lr.n, xs));
  RV_R(impwin_lists(e.f, lr.n, g.w_imp, g.h_imp, E.scratch, E.scratch_bytes, xs));
  const long last_frame = E.limit > 0 ? E.limit - 1 : -1;
  const size_t ni = (size_t)g.w_imp * g.h_imp;
  while (E.imp_next <= m && (E.imp_next + E.W <= m || m == last_frame)) {
    const long n = E.imp_next, last = n + E.W < m ? n + E.W : m;
    {
      std::vector<float *> zs;
      for (long t = n; t <= last; t++) zs.push_back(E.at(t).f.imp);
      RV_R(impwin_zero(zs.data(), (int)zs.size(), (int)ni, xs));
    }
    for (long s2 = last; s2 > n; s2--) {
      const RvLaEngine::Entry &es = E.at(s2);
      // the frame's passes into its reference slots in the window (mv index
      // order; the split is over every slot, :886-942), one launch: within
      // the window they land on distinct frames (only the key frame, before
      // every window, can fill two slots)
      const int nu = es.lr.n;
      int ks[kImpMaxRefs], np = 0;
      float *dst[kImpMaxRefs];
      for (int j = 0; j < nu; j++) {
        const int k = es.lr.order[j];
        const long t = coded_of_display(es.lr.disp[k]);
        if (t < n) continue;  // before the window: gone (:944-948)
        for (int i = 0; i < np; i++)
          if (dst[i] == E.at(t).f.imp)
            return rv_set_error(RV_EINVAL, "la_step: two passes into one frame");
        ks[np] = k;
        dst[np++] = E.at(t).f.imp;
      }
      if (np) RV_R(impwin_pass(es.f, ks, dst, np, nu, g.w_imp, g.h_imp, xs));
    }
    RV_R(impwin_final(E.at(n).f, g.w_imp, g.h_imp, xs));
    RV_H(hipEventRecord(E.at(n).ev_imp, xs));
    std::lock_guard<std::mutex> lk(E.mu);
    E.imp_ready = n;
    E.imp_next = n + 1;
    E.cv.notify_all();
  }
  return RV_OK;
}

static void la_thread_main(rv_replay *r) {
  RvLaEngine &E = *r->eng;
  (void)hipSetDevice(E.dev);
  for (long m = 1;; m++) {
    {
      std::unique_lock<std::mutex> lk(E.mu);
      E.cv.wait(lk, [&] {
        if (E.stop) return true;
        // frame m reads the inputs of displays <= 4 ((m - 1) / 4) + 4
        // (frame_info): with them in place it may run before frame m - W
        // is asked for, as rav1e computes a frame's lookahead on arrival
        // not before the first frame is asked for -- or the inputs are declared
        // in place (tile groups coded one after another in one process need
        // every group's engine running: their parts meet in the hub)
        if (E.requested < 1 && E.inputs_ready == 0) return false;
        if (m > E.requested + E.W && 4 * ((m - 1) / 4) + 4 >= E.inputs_ready) return false;
        if (E.limit > 0 && m >= E.limit) return false;
        return m - E.RW < 1 || E.at(m).used_by == m - E.RW;
      });
      if (E.stop) return;
    }
    if (!E.las) E.las = E.own.stream();
    int rc = E.las ? RV_OK : rv_set_error(RV_EHIP, "the lookahead engine's stream");
    if (rc == RV_OK) rc = ensure_jobs(r);  // (the engine may start before the first frame)
    if (rc == RV_OK) rc = la_step(r, m);
    if (rc != RV_OK) {
      std::lock_guard<std::mutex> lk(E.mu);
      E.err = rc;
      E.msg = rv_last_error();
      E.cv.notify_all();
      return;
    }
  }
}

void la_engine_destroy(rv_replay *r) {
  RvLaEngine *E = r->eng;
  if (E && r->eng_owned) {
    {
      std::lock_guard<std::mutex> lk(E->mu);
      E->stop = true;
      E->cv.notify_all();
    }
    // (its thread reads r->eng from its first statement on: cleared once it has ended)
    if (E->th.joinable()) E->th.join();
    if (E->las) (void)hipStreamSynchronize(E->las);
    E->own.release();
    delete E;  // its device arrays are the replay's allocations (freed with it)
  }
  r->eng = nullptr;
}

// Tile groups over RCCL: before frame n takes its importances, the encode
// thread all-gathers the lookahead parts of every frame up to n + W (the
// window's end) on its own stream, with the same communicator as the
// reconstruction all-gathers -- each rank issues the same collectives in
// the same order on one stream: [parts 1 .. W + 1], frame 1, recon 1,
// [part W + 2], frame 2, ...
int la_encode_exchange(rv_replay *r, long n, hipStream_t st) {
  RvLaEngine &E = *r->eng;
  if (!E.comm) return RV_OK;
  if (!r->eng_owned)
    return rv_set_error(RV_EINVAL, "rv_replay_frame: RCCL lookahead parts on the primary only");
#if RV_HAVE_RCCL
  const Geo &g = r->g;
  long last = n + E.W;
  if (E.limit > 0 && last > E.limit - 1) last = E.limit - 1;
  {
    std::lock_guard<std::mutex> lk(E.mu);
    if (n > E.requested) E.requested = n;  // the engine runs up to n + W
    E.cv.notify_all();
  }
  for (long m = E.xchg_next; m <= last; m++) {
    {
      std::unique_lock<std::mutex> lk(E.mu);
      if (!E.cv.wait_for(lk, std::chrono::seconds(kEngineWaitS),
                         [&] { return E.err != 0 || E.data_ready >= m; }))
        return rv_set_error(RV_EHIP, "rv_replay_frame: the lookahead engine's part never came");
      if (E.err) return rv_set_error(E.err, E.msg.c_str());
    }
    RvLaEngine::Entry &e = E.at(m);
    if (e.m != m) return rv_set_error(RV_EINVAL, "rv_replay_frame: the lookahead ring lost a frame");
    const int R = e.lr.n;
    const int32_t *me = r->grects + 4 * r->my_group;
    RV_H(hipStreamWaitEvent(st, e.ev_data, 0));
    RV_R(impwin_part(e.f, R, me[0], me[1], me[2], me[3], g.w_imp, g.h_imp, E.psend, false, st));
    if (ncclAllGather(E.psend, E.precv, E.pbytes, ncclUint8, (ncclComm_t)E.comm, st) != ncclSuccess)
      return rv_set_error(RV_EHIP, "rv_replay_frame: ncclAllGather (lookahead parts)");
    for (int j = 0; j < r->n_groups; j++) {
      if (j == r->my_group) continue;
      const int32_t *q = r->grects + 4 * j;
      RV_R(impwin_part(e.f, R, q[0], q[1], q[2], q[3], g.w_imp, g.h_imp,
                       E.precv + (size_t)j * E.pbytes, true, st));
    }
    RV_H(hipEventRecord(e.ev_xchg, st));
    std::lock_guard<std::mutex> lk(E.mu);
    E.xchg_done = m;
    E.xchg_next = m + 1;
    E.cv.notify_all();
  }
  return RV_OK;
#else
  (void)n;
  (void)st;
  return rv_set_error(RV_EINVAL, "rv_replay_frame: built without RCCL");
#endif
}

// The encode side: wait for frame n's importances, take its lookahead.
// (rv_replay_set_inputs_ready below lets the engine run further ahead.)
int la_engine_take(rv_replay *r, long n, hipStream_t st, const float **imp) {
  RvLaEngine &E = *r->eng;
  // the engine never computes a frame at or past the stream's limit
  if (E.limit > 0 && n >= E.limit)
    return rv_set_error(RV_EINVAL, "rv_replay_frame: past the stream's limit "
                                   "(rv_replay_set_imp_window)");
  {
    std::unique_lock<std::mutex> lk(E.mu);
    if (n > E.requested) E.requested = n;
    E.cv.notify_all();
    // Bounded: an engine frame takes milliseconds.  It never arrives when a
    // frame RW or more back was skipped (rv_replay_seek) and never coded:
    // the engine then waits for that frame's entry to be released.
    if (!E.cv.wait_for(lk, std::chrono::seconds(kEngineWaitS),
                       [&] { return E.err != 0 || E.imp_ready >= n; }))
      return rv_set_error(RV_EHIP, "rv_replay_frame: the lookahead engine did not deliver the "
                                   "frame's importances (a frame skipped and never coded?)");
    if (E.err) return rv_set_error(E.err, E.msg.c_str());
  }
  const RvLaEngine::Entry &e = E.at(n);
  if (e.m != n) return rv_set_error(RV_EINVAL, "rv_replay_frame: the lookahead ring lost a frame");
  RV_H(hipStreamWaitEvent(st, e.ev_imp, 0));
  const size_t nr = (size_t)r->g.nsb * r->g.R;
  RV_H(hipMemcpyAsync(r->coarse, e.o.coarse, nr * sizeof(rv_fs_result), hipMemcpyDeviceToDevice, st));
  RV_H(hipMemcpyAsync(r->half_l, e.o.half_l, nr * 4 * sizeof(rv_fs_result),
                      hipMemcpyDeviceToDevice, st));
  RV_H(hipMemcpyAsync(r->look, e.o.look, nr * 16 * sizeof(rv_fs_result), hipMemcpyDeviceToDevice,
                      st));
  *imp = e.f.fin;
  return RV_OK;
}

// ... and when the frame's last reader of the entry is queued
int la_engine_release(rv_replay *r, long n, hipStream_t st) {
  RvLaEngine &E = *r->eng;
  RvLaEngine::Entry &e = E.at(n);
  RV_H(hipEventRecord(e.ev_used, st));
  std::lock_guard<std::mutex> lk(E.mu);
  e.used_by = n;
  E.cv.notify_all();
  return RV_OK;
}

}  // namespace rv

extern "C" {

// The inputs of displays < `displays` are in place and stay until coded:
// the engine may run the lookahead of every frame they cover (up to its
// ring), not only up to W frames past the last frame asked for.
int rv_replay_set_inputs_ready(rv_replay *r, long displays) {
  if (!r || displays < 0) return rv_set_error(RV_EINVAL, "rv_replay_set_inputs_ready: bad arguments");
  if (displays > (long)r->inputs.size())
    return rv_set_error(RV_EINVAL, "rv_replay_set_inputs_ready: more displays than input slots");
  if (r->eng) {
    // the engine may start now, before any frame: its job records first
    RV_R(ensure_jobs(r));
    std::lock_guard<std::mutex> lk(r->eng->mu);
    r->eng->inputs_ready = displays;
    r->eng->cv.notify_all();
  }
  return RV_OK;
}

// The importance window W (rdo_lookahead_frames) and the stream's length in
// coded frames (limit; 0: unbounded).  W = 0: the importances are an input
// (rv_replay_set_importances).  Only before the first frame, on a primary
// instance replaying the whole frame as one group.
int rv_replay_set_imp_window(rv_replay *r, int window, long limit) {
  if (!r || window < 0 || window > 1024 || limit < 0)
    return rv_set_error(RV_EINVAL, "rv_replay_set_imp_window: bad arguments");
  if (r->coded > 0) return rv_set_error(RV_EINVAL, "rv_replay_set_imp_window: after the first frame");
  const Geo &g = r->g;
  if (r->eng && !r->eng_owned)
    return rv_set_error(RV_EINVAL, "rv_replay_set_imp_window: on the primary instance");
  la_engine_destroy(r);
  if (!window) return RV_OK;
  RvLaEngine *E = new RvLaEngine();
  E->W = window;
  E->RW = window + 1 + RvLaEngine::kLaSlack;
  E->limit = limit;
  // The engine's stream is created on its thread when the first frame is
  // asked for, after the twin instance's streams: HIP gives a new stream the
  // least-used hardware queue, so the engine's then shares one with a
  // frame-edge or entropy stream instead of with the twin's round kernels
  // (which the trace showed waiting 6-7 us behind the lookahead's).
  // Its device arrays are the replay's (freed with it, after the encode
  // stream has drained); the rest is its own.
  E->own.failed = hipGetDevice(&E->dev) != hipSuccess;
  round_ring_alloc(r->own, E->own, E->rr, r->stream);
  const int ni = g.w_imp * g.h_imp, nr = g.nsb * r->RA;  // the lookahead's references
  E->la_list = r->dev<int32_t>((size_t)nr * 20);
  E->scratch_bytes = impwin_scratch_bytes(ni);
  E->scratch = r->dev<uint8_t>(E->scratch_bytes);
  E->ring.resize((size_t)E->RW);
  const size_t ob = ((size_t)nr * 21 * sizeof(rv_fs_result) + 255) / 256 * 256;
  for (auto &en : E->ring) {
    // one block per entry: the lookahead's results (zeroed), then the ImpFrame
    uint8_t *m = r->dev<uint8_t>(ob + impwin_frame_bytes(ni, r->RA));
    if (!m || hipMemsetAsync(m, 0, ob, r->stream) != hipSuccess) E->own.failed = true;
    if (r->own.failed || E->own.failed) break;
    for (hipEvent_t *ev : {&en.ev_imp, &en.ev_used, &en.ev_data, &en.ev_xchg})
      *ev = E->own.event(hipEventDisableTiming);
    en.o.coarse = (rv_fs_result *)m;
    en.o.half_l = en.o.coarse + nr;
    en.o.look = en.o.half_l + (size_t)nr * 4;
    impwin_frame_carve(en.f, m + ob, ni, r->RA);
  }
  E->pyr_display.assign(r->inputs.size(), -1);
  r->eng = E;
  r->eng_owned = true;
  if (r->own.failed || E->own.failed || hipStreamSynchronize(r->stream) != hipSuccess) {
    la_engine_destroy(r);
    return rv_set_error(RV_EHIP, "rv_replay_set_imp_window: allocation failed");
  }
  E->th = std::thread(la_thread_main, r);
  return RV_OK;
}

// Tile groups with an importance window: how each frame's importance data
// of the other groups arrives (la_exchange).
rv_la_hub *rv_la_hub_create(int n_groups) {
  if (n_groups < 2 || n_groups > kMaxGroups) {
    rv_set_error(RV_EINVAL, "rv_la_hub_create: 2 .. kMaxGroups groups");
    return nullptr;
  }
  rv_la_hub *h = new rv_la_hub();
  h->n = n_groups;
  h->posted.assign((size_t)n_groups, 0);
  for (int s = 0; s < rv_la_hub::kRing; s++) {
    h->buf[s].assign((size_t)n_groups, nullptr);
    h->ev[s].assign((size_t)n_groups, nullptr);
  }
  return h;
}
void rv_la_hub_destroy(rv_la_hub *h) { delete h; }  // the members own the buffers / events

int rv_replay_set_la_exchange(rv_replay *r, void *comm, rv_la_hub *hub) {
  if (!r || (!comm == !hub)) return rv_set_error(RV_EINVAL, "rv_replay_set_la_exchange: comm xor hub");
  if (!r->eng || !r->eng_owned || r->coded > 0)
    return rv_set_error(RV_EINVAL, "rv_replay_set_la_exchange: a primary instance with a window, "
                                   "before the first frame");
  if (r->n_groups < 2 && !comm)
    return rv_set_error(RV_EINVAL, "rv_replay_set_la_exchange: rv_replay_set_groups first");
  RvLaEngine &E = *r->eng;
  const Geo &g = r->g;
  size_t most = 0;
  for (int j = 0; j < r->n_groups; j++) {
    int bx0, by0, bw, bh;
    impwin_group_blocks(r->grects[4 * j], r->grects[4 * j + 1], r->grects[4 * j + 2],
                        r->grects[4 * j + 3], g.w_imp, g.h_imp, bx0, by0, bw, bh);
    const size_t b = (size_t)bw * bh * kImpPartBytes;
    most = b > most ? b : most;
  }
  E.pbytes = (most + 255) / 256 * 256;
  if (comm) {
    E.psend = r->dev<uint8_t>(E.pbytes);
    E.precv = r->dev<uint8_t>(E.pbytes * (size_t)r->n_groups);
    if (!E.psend || !E.precv) return rv_set_error(RV_EHIP, "rv_replay_set_la_exchange: alloc");
    E.comm = comm;
    return RV_OK;
  }
  if (hub->n != r->n_groups)
    return rv_set_error(RV_EINVAL, "rv_replay_set_la_exchange: the hub's group count");
  const int k = r->my_group;
  std::lock_guard<std::mutex> lk(hub->mu);
  for (int s = 0; s < rv_la_hub::kRing; s++) {
    if (hub->buf[s][k]) return rv_set_error(RV_EINVAL, "rv_replay_set_la_exchange: group joined twice");
    hub->buf[s][k] = r->dev<uint8_t>(E.pbytes);
    hub->ev[s][k] = E.own.event(hipEventDisableTiming);  // (released with the engine)
    if (!hub->buf[s][k] || !hub->ev[s][k])
      return rv_set_error(RV_EHIP, "rv_replay_set_la_exchange: alloc");
  }
  E.hub = hub;
  E.hub_k = k;
  return RV_OK;
}

// The importances ([h_imp][w_imp] f32) the last coded frame's RDO used.
int rv_replay_get_importances(rv_replay *r, float *host, int n) {
  if (!r || !host || n != r->g.w_imp * r->g.h_imp)
    return rv_set_error(RV_EINVAL, "rv_replay_get_importances: bad arguments");
  RV_H(hipStreamSynchronize(r->stream));
  if (!r->imp_last) {
    memset(host, 0, (size_t)n * 4);
    return RV_OK;
  }
  RV_H(hipMemcpy(host, r->imp_last, (size_t)n * 4, hipMemcpyDeviceToHost));
  return RV_OK;
}

}  // extern "C"

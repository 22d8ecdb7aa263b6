// rv_replay.h -- internal: what the replay's three files share.  The constants
// and geometry helpers, the instance (rv_replay) with its DPB slots, round
// ring, lookahead engine and entropy host thread (an Owned, rv_owned.h, holds
// what the runtime hands out to them), the round loop's host side
// (run_rounds), the names of the timing events, and the host functions one
// file defines and another calls.  rv_replay.hip: create / destroy, job
// tables, setters, getters, read-outs; rv_replay_frame.hip: one coded frame;
// rv_replay_la.hip: the lookahead and its engine.
#pragma once
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <algorithm>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "rv_cdef.h"
#include "rv_chain.h"
#include "rv_deblock.h"
#include "rv_device.h"
#include "rv_ec.h"
#include "rv_frame.h"
#include "rv_intra.h"
#include "rv_intra_pass.h"
#include "rv_me.h"
#include "rv_mvref.h"
#include "rv_owned.h"
#include "rv_impwin.h"
#include "rv_lrf.h"
#include "rv_rdo.h"
#include <string>

#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#define RV_HAVE_RCCL 1
#else
#define RV_HAVE_RCCL 0
#endif

#define RV_R(expr)                  \
  do {                              \
    int e_ = (expr);                \
    if (e_ != RV_OK) return e_;     \
  } while (0)
#define RV_H(expr)                                            \
  do {                                                        \
    hipError_t e_ = (expr);                                   \
    if (e_ != hipSuccess) return rv_set_hip_error(e_, #expr); \
  } while (0)

namespace rv {

constexpr int kSb = 64;
// DPB slots, keyed by display index % kSlots.  24 (round 6; 12 before): the
// reuse of a slot orders a level-0 frame after the level-2 frames that read
// the slot's previous occupant, and with 12 slots that closed a cycle of
// two groups (level 0 of g -> level 1 -> level 2 -> level 0 of g + 2) that
// bounded the three pipelined instances; with 24 it spans five groups.
constexpr int kSlots = 24;
// result words per superblock and reference: coarse (mv, cost), the four
// half-res quadrants, full-pel, sub-pel, the 16 lookahead 16x16 blocks
constexpr int kWordsPerRef = 2 + 8 + 2 + 2 + 32 + 8;
// Workgroups of the list-driven launches of the MV-stack rounds after the
// first (a fixed pool that loops over the device counts)
constexpr int kRoundGrid = 256;
constexpr int kMaxGroups = 8;

struct Geo {
  int W, H, xdec, ydec, bd, hbd;
  int w_in_b, h_in_b;       // MiCols / MiRows (src/encoder.rs:580-581)
  int tx0, ty0, tw, th;     // this instance's tile group, in superblocks
  int tws, ths;             // uniform tile size in superblocks (TilingInfo)
  int nsb, R, M, C;         // superblocks, references, modes per ref, candidates
  int cw, ch;               // chroma block of a superblock
  int w_imp, h_imp;         // importance grid (src/encoder.rs:624-625)
  int vis_w, vis_h;         // the group's visible size (pixels)
};

__host__ __device__ inline int div_trunc8(int v) { return v / 8; }

// get_mv_range (src/me.rs:64-80); bo in 4x4 units (frame).  Rust usize
// arithmetic wraps and is cast back to isize, i.e. signed here.
__host__ __device__ inline void mv_range(const Geo &g, int bx, int by, int bw, int bh, int r[4]) {
  const int border_w = 128 + bw * 8, border_h = 128 + bh * 8;
  r[0] = -bx * 32 - border_w;
  r[1] = (g.w_in_b - bx - bw / 4) * 32 + border_w;
  r[2] = -by * 32 - border_h;
  r[3] = (g.h_in_b - by - bh / 4) * 32 + border_h;
}
// The tile of superblock (sx, sy) of the group: its origin (superblocks)
// and visible size in 4x4 units (TileStateMut mi_width / mi_height,
// src/tiling/tile_state.rs:93).
__host__ __device__ inline void sb_tile(const Geo &g, int sx, int sy, int &t0x, int &t0y,
                                        int &mi_w, int &mi_h) {
  const int fx = g.tx0 + sx, fy = g.ty0 + sy;
  t0x = fx - fx % g.tws;
  t0y = fy - fy % g.ths;
  const int vw = g.W - t0x * kSb < g.tws * kSb ? g.W - t0x * kSb : g.tws * kSb;
  const int vh = g.H - t0y * kSb < g.ths * kSb ? g.H - t0y * kSb : g.ths * kSb;
  mi_w = vw >> 2;
  mi_h = vh >> 2;
}
// adjust_bo (src/me.rs:993-1004) on tile-relative 4x4 offsets
__host__ __device__ inline void adjust_bo(int mi_w, int mi_h, int &bx, int &by, int bw, int bh) {
  int x = bx < mi_w - bw / 4 ? bx : mi_w - bw / 4;
  int y = by < mi_h - bh / 4 ? by : mi_h - bh / 4;
  bx = x > 0 ? x : 0;
  by = y > 0 ? y : 0;
}
__host__ __device__ inline uint32_t pack_mv(rv_mv m) {
  return ((uint32_t)(uint16_t)m.row << 16) | (uint16_t)m.col;
}
// Block-level reduction helper: one atomic per workgroup (never one per
// wavefront: same-address atomics serialise, MI355X_MICROARCH.md).
__device__ inline void block_atomic_add(uint64_t s, unsigned long long *out) {
  __shared__ uint64_t red[4];
  s = group_sum<64>(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) t += red[i];
    if (t) atomicAdd(out, (unsigned long long)t);
  }
}

// ---- speed 6 (config D): the partition levels below 64x64 -----------------
constexpr int kLevels = 4;  // 64x64, 32x32, 16x16, 8x8

// What a candidate slot's F4 outputs (l_out / c_out) were computed for: an
// F4 evaluation (rdo_quad: prediction, transform, quantisation, distortion,
// coefficient rate) is a function of the block, its reference(s) and
// MV(s) alone -- the stacks only enter the mode / MV rates, which the argmin
// adds (cand_cost) -- so a later round of the same frame whose candidate has
// the MV the slot was last evaluated with keeps the slot's outputs instead of
// re-running it.  tag: the frame (rv_replay::coded + 1; 0 = never).
struct CandKey {
  uint32_t tag, mv0, mv1;
};

// F7 exchange: copy rectangles between planes and a packed buffer (row-major
// per rectangle, `off` bytes into it).  blockIdx.y = rectangle.
struct XRect {
  int64_t off;
  int plane, x0, y0, w, h;
};

// The timing events of an instrumented frame (rv_replay::evs).  kEvStart ..
// kEvF7 are the stage boundaries on the main stream, in order: stage i of
// rv_replay_stage_times spans events i and i + 1.  The pairs after them are
// spans of their own, read out in this order: the lookahead (on the main
// stream without an importance window), the frame-edge levels (on the edge
// stream at speed 10) and F8's coefficient tokens.
enum StageEv {
  kEvStart = 0,
  kEvF0,        // hres / qres of the input
  kEvF1,        // coarse search
  kEvF2,        // the lookahead's half-res quadrants
  kEvFL,        // the lookahead's 16x16 blocks and its rounds
  kEvF3Full,    // F2 + F3 full-pel
  kEvF3Sub,     // F3 sub-pel + the candidate lists
  kEvF4Single,  // F4, single-reference candidates
  kEvF4Comp,    // F4, compound candidates
  kEvArgmin,    // the argmin, the MV-stack rounds, the partition
  kEvCommit,    // F6
  kEvIntra,     // F6b + the MV / intra fixed point + the frame's MVs
  kEvF5,
  kEvF7,        // block map, F8, loop filters / exchange
  kEvLaBegin,
  kEvLaEnd,
  kEvEdgeBegin,
  kEvEdgeEnd,
  kEvF8Begin,
  kEvF8End,
  kEvCount
};

}  // namespace rv

using namespace rv;

struct RvSlot {  // one frame of the DPB: the reconstruction and its motion field
  rv_plane y, u, v;
  // the frame's motion field (frame_mvs: the encode's tile field when the
  // frame was coded; zero for the key frame), 8x8 cells [h_in_b/2][w_in_b/2][R]
  rv_mv *fmv = nullptr;
};
struct RvInput {
  rv_plane y, u, v;
  // input_hres / input_qres (FrameState, src/encoder.rs:362-377: downsample
  // + pad): the half / quarter resolution planes the searches of this frame
  // and of every frame referencing it read; F0 of the frame (or the
  // lookahead running ahead) writes them
  rv_plane hres, qres;
  uint32_t *qres_box = nullptr;  // rv_plane_box_sums of qres (the SEA coarse search)
};

// The host side of stage F8 (RV_REPLAY_ENTROPY): a thread that range-codes
// each frame's tile token streams once the device has written them into
// host-mapped memory (two ring slots), keeping the CDF chain per pyramid
// level (get_initial_cdfcontext / the biggest tile, src/encoder.rs:
// 2750-2761, 2824-2833).
struct EcHost {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  struct Item {
    int slot, level, qctx;
  };
  std::deque<Item> q;
  bool stop = false;
  long queued = 0, done = 0;
  int ntiles = 1;
  uint32_t *tok_h[2] = {nullptr, nullptr}, *stat_h[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool busy[2] = {false, false};
  std::vector<uint16_t> chain[3];
  uint64_t stat[5] = {0, 0, 0, 0, 0};
  int err = 0;

  void code(const Item &it);
  void run();
  void drain();
};

// The counts of one chain of round checks (the lookahead's EPZS rounds, the
// MV-stack rounds): check q counts into the device slot q % kCnt and
// publishes (q << 32 | count) into the host-mapped ring at q % kPub
// (round_publish), where the host reads it without a stream sync.  One
// ring per host thread that runs round loops.
struct RoundRing {
  static constexpr int kCnt = 64, kPub = 64;
  int32_t *cnt = nullptr;  // [kCnt][2], then the ticket
  uint32_t *ticket = nullptr;
  unsigned long long *h_pub = nullptr, *d_pub = nullptr;
  uint32_t seq = 0;
  int last_count = -1;  // the run's last count the host read (-1: none yet)
  int32_t *slot(uint32_t q) const { return cnt + 2 * (q % kCnt); }
  // check q's publication (publish = false: counted, not published)
  RoundPub pub(uint32_t q, bool publish = true) const {
    return RoundPub{slot(q), slot(q + 1), ticket, publish ? d_pub + q % kPub : nullptr, q};
  }
};

// A frame's lookahead references (la_refs_of below): the displays in k order
// and the propagation order
struct LaRefs {
  int n, disp[kImpMaxRefs], order[kImpMaxRefs];
};

// Where a frame's lookahead writes (compute_lookahead_motion_vectors):
// F1 [R][nsb], F2L [R][nsb][4], FL [R][nsb][16]
struct LaOut {
  rv_fs_result *coarse = nullptr, *half_l = nullptr, *look = nullptr;
};

// The lookahead engine of an importance window W (rdo_lookahead_frames,
// src/api/config.rs:158; rv_replay_set_imp_window).  rav1e computes every
// frame's lookahead as the frame arrives, far ahead of its encode
// (compute_lookahead_data, src/api/internal.rs:767-820), and before coding
// output frame n propagates block importances over the window [n, n + W]
// (compute_block_importances, :823-1081).  Here a host thread of its own
// runs, on its own stream and round ring, the lookahead of coded frame m
// (F0 pyramids, F1, F2L, FL with their EPZS rounds, then the importance
// data of rv_impwin.h) into ring entry m % RW, and as soon as frame n + W is
// in, the window propagation for frame n.  The encode of frame n waits for
// that (a host flag, then a stream event), takes its lookahead results and
// final importances from the entry, and marks the entry used when the frame
// is done; the engine reuses entry m % RW for frame m + RW only after that.
// RW = W + 1 + kLaSlack: the slack covers the frames a twin instance still
// has in flight behind the primary.
constexpr int kEngineWaitS = 60;  // la_engine_take's bound on one frame's wait

// An in-process exchange of the lookahead engines' frame parts between the
// tile groups of one process (rv_la_hub_create: the GPU tests and the
// bench's rank emulation; real ranks all-gather over RCCL).  Group k's
// engine packs coded frame m's part into its buffer m % kRing, records an
// event and posts m; once every group has posted m it waits on the others'
// events and unpacks their parts.  A buffer is rewritten kRing frames later,
// after every group's unpack of it (each group posts frame m + 1 only after
// issuing its unpack of m).
struct rv_la_hub {
  static constexpr int kRing = 4;
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<long> posted;
  std::vector<uint8_t *> buf[kRing];
  std::vector<hipEvent_t> ev[kRing];
};

struct RvLaEngine {
  static constexpr int kLaSlack = 28;
  int W = 0, RW = 0, dev = 0;
  long limit = 0;  // coded frames in the stream (0: unbounded)
  Owned own;  // its stream, events (its hub events too), pinned ring; its device arrays are the replay's
  hipStream_t las = nullptr;  // the engine's stream: the searches and the window passes
  RoundRing rr;
  int32_t *la_list = nullptr;
  void *scratch = nullptr;
  size_t scratch_bytes = 0;
  struct Entry {
    LaOut o;
    ImpFrame f;
    long m = -1;       // the coded frame the entry holds
    long used_by = -1; // host: the frame whose encode recorded ev_used
    rv_replay_frame_info fi{};
    LaRefs lr{};
    hipEvent_t ev_imp = nullptr, ev_used = nullptr;
    hipEvent_t ev_data = nullptr, ev_xchg = nullptr;  // RCCL parts: data in / exchanged
  };
  std::vector<Entry> ring;
  std::vector<long> pyr_display;  // per input: the display whose pyramid it holds
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  long requested = 0;  // the highest frame an encode has asked for (0: none yet)
  long inputs_ready = 0;  // the inputs of displays < this are in place (rv_replay_set_inputs_ready)
  long imp_ready = 0;  // the importances of frames <= imp_ready are recorded
  long imp_next = 1;
  bool stop = false;
  int err = 0;
  std::string msg;
  long la_round_sum = 0, la_reeval = 0, la_frames = 0;  // under mu
  // several tile groups (rv_replay_set_la_exchange): every group's part of
  // each frame's importance data reaches every group, over RCCL (comm, the
  // part buffers psend / precv, pbytes per group) or an in-process hub.
  // RCCL: the all-gathers run on the encode's stream with the reconstruction
  // all-gathers, one communicator and one stream per rank, so every rank
  // issues its collectives in the same order on one queue (la_encode_
  // exchange; two communicators on streams sharing hardware queues can
  // deadlock across ranks).  The engine posts a frame's data (data_ready,
  // ev_data) and waits for its exchange (xchg_done, ev_xchg).
  void *comm = nullptr;
  uint8_t *psend = nullptr, *precv = nullptr;
  size_t pbytes = 0;
  long data_ready = 0, xchg_done = 0, xchg_next = 1;
  rv_la_hub *hub = nullptr;
  int hub_k = -1;
  Entry &at(long m) { return ring[(size_t)(m % RW)]; }
};

struct rv_replay {
  rv_replay_cfg cfg{};
  Geo g{};
  int RA = 1;  // the lookahead's references (LaRefs; R = 2: 3, LAST3 added)
  CandGeo cg{};
  Owned own;  // every device / pinned allocation, event and stream of the instance
  hipStream_t stream = nullptr;
  template <class T>  // a device array, the fill queued on the stream
  T *dev(size_t n, Fill fill = Fill::None) { return own.dev<T>(n, fill, stream); }
  hipEvent_t ev_ielig = nullptr;  // intra_begin's count is on the host
  // the frame-edge levels get a stream of their own (edge, below);
  // RAV1E_HIP_REPLAY_SERIAL=1: one stream (the profiling mode)
  bool overlap = false;
  bool own_stream = false;  // (the caller's stream is not in `own`)
  bool sea = false;  // successive-elimination coarse search (bit depth <= 10)
  // per pyramid level: the frame's quantizers (QuantizationContext of
  // TX_64X64 luma / TX_32X32 chroma, inter) and lambdas
  struct Level {
    bool set = false;
    int qidx = 0;
    QCtx ql{}, qu{}, qv{};
    QCtx qil{}, qiu{}, qiv{};  // the same transforms, intra (is_intra rounding)
    QCtx qs[kLevels][3] = {};  // speed 6: luma / U / V of the 32x32 .. 8x8 blocks
    double lambda = 0.0, me_lambda = 0.0, ds[3] = {0.0, 0.0, 0.0};
  } lv[3] = {};
  // speed 6: the partition levels below 64x64 (index 0 = the superblocks,
  // whose arrays are the ones above)
  struct PLevel {
    int B = 0, n = 0, gw = 0, gh = 0, bc = 0, bch = 0, txl = 0, txc = 0;
    CandGeo cg{};
    rv_ds_job *jobs_full[3] = {nullptr, nullptr, nullptr}, *jobs_sub[3] = {nullptr, nullptr, nullptr};
    rv_fs_result *full = nullptr, *sub = nullptr;
    uint64_t *l_out = nullptr, *c_out = nullptr;
    RdoWinner *win = nullptr;
    int32_t *cand_list = nullptr, *cand_count = nullptr;
    int32_t *l_lev = nullptr, *c_lev = nullptr;
    int32_t *leaf = nullptr;
    size_t woff = 0;  // result words offset
  } pl[kLevels] = {};
  bool s6 = false;
  // the 32x32 .. 8x8 level grids: speed 6 over the group, speed 10 over the
  // bounding rectangle (group superblocks ex0, ey0 + ew x eh) of the
  // superblocks past the frame's right / bottom edge (must_split)
  bool lvl = false;
  int ex0 = 0, ey0 = 0, ew = 0, eh = 0;
  // per level: leaves exist (RDO, score, commit) / the motion search runs
  // (a 16x16 / 8x8 level seeds from the 32x32 searches)
  bool lv_used[kLevels] = {false, false, false, false};
  bool lv_me[kLevels] = {false, false, false, false};
  // speed 10: the edge levels run on their own stream beside the 64x64 stages
  hipStream_t edge[kLevels] = {nullptr, nullptr, nullptr, nullptr};  // [1..3]: one stream, shared
  hipEvent_t ev_efork = nullptr, ev_l1me = nullptr, ev_epart = nullptr;
  hipEvent_t ev_ejoin[kLevels] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_ecommit[kLevels] = {nullptr, nullptr, nullptr, nullptr};
  bool deblock = false;           // RV_REPLAY_DEBLOCK
  uint8_t *mi_lg = nullptr, *mi_skip = nullptr;  // the deblocking block map
  int mi_stride = 0, mi_cols = 0, mi_rows = 0;
  uint8_t db_level[3] = {0, 0, 0};  // fast level per pyramid level
  // speed 6: sse_optimize's level search (rv_deblock_sse): tallies, levels
  int64_t *db_tally = nullptr;
  uint8_t *db_dlev = nullptr;
  bool cdef = false;                // RV_REPLAY_CDEF
  // RV_REPLAY_LRF: the units' distortions / solved xqd per (plane,
  // superblock), the units' filters, the restored frame before its padding
  bool lrf = false;
  uint64_t *lrf_err = nullptr;
  int8_t *lrf_xqd = nullptr, *lrf_units = nullptr;
  int lrf_fix_passes = 1 << 30;  // the decision kernel (create: RAV1E_LRF_FIX[_PASSES])
  RvInput lrf_out{};
  RvInput cdef_pre{};                // the deblocked, pre-CDEF frame (the padded copy's source)
  uint8_t *cdef_dir = nullptr, *cdef_idx = nullptr;  // per 8x8 block; per 64x64 (all 0)
  int32_t *cdef_var = nullptr;
  uint8_t cdef_str[3][2] = {};      // [level] = (y, uv) strengths at cdef_index 0
  int32_t *leaf_count = nullptr;  // [kLevels]
  // RV_REPLAY_ENTROPY: the coefficient-coding stage (F8)
  bool entropy = false;
  EcFrameBufs ecb{};
  EcHost *ech = nullptr;
  long ec_frames = 0;
  // intra-mode screening (rv_intra_pass.hip; speed 10, 4:2:0)
  bool intra = false;
  uint8_t *i_elig = nullptr, *i_was = nullptr, *i_win = nullptr, *i_modes = nullptr;
  int32_t *i_mark = nullptr, *i_list[2] = {nullptr, nullptr}, *i_commit = nullptr,
          *i_revert = nullptr;
  int32_t *i_cnt = nullptr;    // [list 0, list 1, commit, revert]
  int32_t *h_cnt = nullptr;    // pinned host copy of one count
  void *i_edges = nullptr;
  uint64_t *i_lout = nullptr, *i_cout = nullptr;
  uint32_t *i_stats = nullptr; // [kRing][3]: screened, intra winners, rounds
  // speed 10: rav1e's MV stacks (rv_mvref.hip) in coding-order rounds
  bool exact = false;
  MvStack *stk = nullptr;              // the stacks each superblock was evaluated with
  BlkDec *dec_lv[3] = {nullptr, nullptr, nullptr};  // decisions, per pyramid level
  uint8_t *mv_active = nullptr;        // re-evaluate this round
  // the round checks' counts (this instance's host thread)
  static constexpr int kRoundsAhead = 2;  // rounds queued beyond the last count read
  RoundRing rr;
  int32_t *mv_list = nullptr;          // [2][nsb]: check q lists into half q & 1
  bool edge_tr = false;                // a stack reads a frame-edge leaf (top-right)
  // evaluation rounds (round 0 included), re-evaluated superblocks and
  // round runs (1 + the MV / intra passes) per frame, summed
  long mv_round_sum = 0, mv_reeval = 0, mv_run_sum = 0;
  long mv_frames = 0;  // the frames this instance coded with the rounds (a twin codes some)
  size_t nwords = 0, wpart = 0;   // result words; offset of the partition masks
  bool jobs_built = false;
  std::mutex jobs_mu;  // ensure_jobs: the encode and the lookahead engine may both need them
  std::vector<RvSlot> slots;
  std::vector<RvInput> inputs;
  rv_fs_job *fs_jobs[3] = {nullptr, nullptr, nullptr};  // per level (scale 4, 2, 1)
  // half: 4 quadrants per superblock; look(ahead): 16 16x16 blocks per superblock
  rv_fs_result *coarse = nullptr, *half = nullptr, *full = nullptr, *sub = nullptr, *look = nullptr;
  rv_fs_result *half_l = nullptr;             // the lookahead's 4 quadrants per superblock
  rv_ds_job *jobs_half[3] = {}, *jobs_full[3] = {}, *jobs_sub[3] = {}, *jobs_look[3] = {};  // per level
  rv_ds_job *jobs_half_l[3] = {nullptr, nullptr, nullptr};  // the lookahead's F2 (per level)
  int32_t *la_list = nullptr;  // the lookahead rounds' marked jobs: F2 [R nsb 4], then FL [R nsb 16]
  long la_round_sum = 0, la_reeval = 0;  // the lookahead rounds (round 0 included), re-evaluated jobs
  long la_frames = 0;                    // ... and their frames
  RvLaEngine *eng = nullptr;  // the importance window's lookahead engine (null: W = 0)
  bool eng_owned = false;     // the primary owns it; a twin borrows it
  const float *imp_last = nullptr;  // the importances the last coded frame used
  int32_t *src_half = nullptr, *src_full = nullptr, *src_look = nullptr;  // predictor sources
  uint64_t *l_out = nullptr, *c_out = nullptr;  // F4: [skip dist, non-skip dist, rate] per tx block
  RdoWinner *win = nullptr;
  int32_t *cand_list = nullptr, *cand_count = nullptr;  // F4: the valid candidates
  RdoArgs *f4_args = nullptr;        // F4: the frame's list-launch arguments [la, ca, lc, cc]
  CandKey *cand_key = nullptr;       // F4: what each candidate slot was last evaluated with
  uint8_t *f3dirty = nullptr;        // rounds: the F3 jobs whose set / pmv changed [R][nsb]
  uint8_t *f2dirty = nullptr;        // rounds: the F2 jobs whose set changed [R][nsb][4]
  uint32_t *cand_evals = nullptr;  // [kRing][2 * kLevels]: F4 candidates per frame and level (single, compound)
  int32_t *l_lev = nullptr, *c_lev = nullptr;  // F6: committed levels
  uint64_t *words = nullptr;
  unsigned long long *tail = nullptr;  // [levels csum, group recon sum, imp satd sum, -, frame recon sum]
  float *imp = nullptr;      // block_importances (null: all zero)
  int n_imp = 0, imp_bx = 0, imp_by = 0, ntx_c = 0;
  long coded = 0;            // frames coded so far (0 = the key frame next)
  rv_replay_frame_info last{};
  // tile-group exchange (F7)
  int n_groups = 1, my_group = 0;
  int32_t grects[4 * kMaxGroups] = {};
  size_t xbytes = 0;         // packed bytes per group (the largest group)
  uint8_t *xsend = nullptr, *xrecv = nullptr;
  void *comm = nullptr;      // ncclComm_t (rv_comm)
  // Event ring: instrumented frame k records into set k % kRing, so per-
  // kernel times can be summed over a timed run without a host sync per
  // frame.  Every `timing_stride`-th block of frames is instrumented (each
  // record costs ~4.4 us of idle GPU between kernels on MI355X).
  static constexpr int kRing = 64;
  hipEvent_t evs[kRing][kEvCount] = {};  // StageEv
  int timing_stride = 1, timing_block = 1;
  long timed = 0;
  // diamond candidate evaluations per job, per ring slot: [kRing][2][nsb*R]
  uint32_t *ds_evals = nullptr;
  // Kernel probes (rv_replay_set_kernel_probe): on instrumented frames
  // every launch of a probed kernel -- probe 0: F3 sub-pel
  // (ds_fast_kernel<W = H = 64, sub-pel>), probe 1: the F4 candidate lists
  // (rdo_quad_list_kernel); round 0 and the MV-stack rounds -- is bracketed
  // by an event pair on its stream, and the launches add their units into
  // kp_cnt[p] (probe 0: candidate evaluations, jobs; probe 1: single /
  // compound luma candidates, single / compound chroma transform blocks).
  // Pair i of probe p uses kp_ev[p][2 (i % kKp)], harvested (elapsed time
  // summed) before reuse.
  static constexpr int kProbes = 2, kKpCnt = 4;
  bool kprobe = false;
  static constexpr int kKp = 512;
  std::vector<hipEvent_t> kp_ev[kProbes];
  long kp_n[kProbes] = {0, 0}, kp_done[kProbes] = {0, 0}, kp_base[kProbes] = {0, 0};
  // span slots [kp_n, kp_init) are initialised (start = max, end = 0): one
  // copy per kKpInit launches instead of one per launch (each a dependent
  // blit on the round's stream: the probe cost 2.5 % of the line, r06np)
  long kp_init[kProbes] = {0, 0};
  static constexpr int kKpInit = 256;
  double kp_ms[kProbes] = {0.0, 0.0}, kp_dev_ms[kProbes] = {0.0, 0.0};
  uint32_t *kp_cnt[kProbes] = {nullptr, nullptr};  // device [kKpCnt] each
  // ... and each launch's span on the device clock: [kKp][2] (first
  // workgroup's start, last one's end), harvested with the events
  unsigned long long *kp_ts[kProbes] = {nullptr, nullptr};
  double kp_tick_ms = 0.0;  // ms per wall_clock64 tick
};

// The host side of a round loop: check(q) queues check q, which lists the
// jobs to re-run and publishes their count into the ring; eval(q) queues the
// round that re-runs check q's list.  The host keeps kRoundsAhead rounds
// queued beyond the last count it has read (it spins on the published
// counts, no stream synchronisation), so the GPU never waits on the host;
// the loop ends at the first check that lists nothing (the rounds queued
// after it find empty lists).  budget: the chain's depth bound (see the
// callers); a check still listing jobs after it is an internal error.
template <typename Check, typename Eval>
int run_rounds(RoundRing &rr, hipStream_t xs, int budget, Check &&check, Eval &&eval,
               long *nrounds, long *nre, bool *changed, const char *what, long frame, int level) {
  static const bool mv_trace = getenv("RAV1E_HIP_MV_TRACE") != nullptr;
  if (changed) *changed = false;
  rr.last_count = -1;
  const uint32_t first = rr.seq++;
  RV_R(check(first));
  int queued = 0;  // evaluation rounds queued (round j evaluates check j - 1's list)
  for (int seen = 0;; seen++) {
    while (queued < budget && queued < seen + rv_replay::kRoundsAhead) {
      RV_R(eval(first + (uint32_t)queued));
      RV_R(check(rr.seq++));
      queued++;
    }
    const uint32_t q = first + (uint32_t)seen;
    volatile unsigned long long *pub = rr.h_pub + q % RoundRing::kPub;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long v;
    for (long spin = 0;; spin++) {
      v = *pub;
      if ((uint32_t)(v >> 32) == q) break;
      if ((spin & 1023) == 1023) {
        const hipError_t he = hipStreamQuery(xs);
        if (he != hipSuccess && he != hipErrorNotReady)
          return rv_set_error(RV_EHIP, "rv_replay_frame: a round failed");
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30))
          return rv_set_error(RV_EHIP, "rv_replay_frame: a round's count never arrived");
        std::this_thread::yield();
      }
    }
    const int c = (int)(uint32_t)v;
    rr.last_count = c;
    if (mv_trace) fprintf(stderr, "%s frame %ld level %d check %d: %d\n", what, frame, level, seen, c);
    if (c == 0) return RV_OK;
    if (seen >= budget)
      return rv_set_error(RV_EHIP, "rv_replay_frame: rounds beyond the chain's dependency "
                                   "depth (internal error)");
    *nre += c;
    (*nrounds)++;
    if (changed) *changed = true;
  }
}

namespace rv {

// several tile groups (or a one-rank all-gather): each rank decides its own
// units before the exchange and imports the others'
inline bool groups_active(const rv_replay *r) { return r->n_groups >= 2 || r->comm; }

// rv_replay.hip
hipError_t kp_harvest(rv_replay *r, int p, long upto);
size_t plane_bytes(const rv_plane &p);
void round_ring_alloc(Owned &dev, Owned &host, RoundRing &q, hipStream_t st);
int ensure_jobs(rv_replay *r);
int group_rects(const rv_replay *r, int k, XRect out[9], int *n);
int xcopy(rv_replay *r, const RvSlot &s, const XRect *rects, int n, int to_plane, uint8_t *buf);
int lrf_decide_slot(rv_replay *r, const RvSlot &s, const RvInput &in, int lv, const LrfGeo &lg,
                    const int32_t *rect);
int filter_slot(rv_replay *r, const RvSlot &s, const RvInput &in, int lv);
void frame_info(long n, int R, rv_replay_frame_info *f);
LaRefs la_refs_of(long m, int R);

// rv_replay_la.hip
int lookahead_frame(rv_replay *r, RoundRing &rr, hipStream_t xs, const rv_replay_frame_info &fi,
                    const LaRefs &lr, long frame, const LaOut &o, int32_t *la_list, bool pyramid,
                    long *nrounds, long *nre, hipEvent_t *e);
void la_engine_destroy(rv_replay *r);
int la_encode_exchange(rv_replay *r, long n, hipStream_t st);
int la_engine_take(rv_replay *r, long n, hipStream_t st, const float **imp);
int la_engine_release(rv_replay *r, long n, hipStream_t st);

}  // namespace rv

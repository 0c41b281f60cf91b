// ia_host.h — what every host unit of libia.so shares: error plumbing (fail, HIP_TRY, NCCL_TRY),
// the owning device buffer, the context and index structs behind include/ia.h's opaque
// pointers, and the few functions one unit needs from another.  Everything here is internal:
// namespace ia_host and the two structs are hidden from the dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ia.h"
#include "ia_internal.h"
#include "ia_launch.h"

typedef struct ncclComm *ncclComm_t;  // as rccl.h has it; only ia_comm.cpp and the step loop include that

namespace ia_host __attribute__((visibility("hidden"))) {

// records msg as the calling thread's last error (ia_last_error) and returns code; ia_ctx.cpp
int fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(IA_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
  } while (0)
#define NCCL_TRY(expr)                                                                         \
  do {                                                                                         \
    ncclResult_t r_ = (expr);                                                                  \
    if (r_ != ncclSuccess) return fail(IA_ECOMM, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
  } while (0)

// grow-only device buffer; owns its memory (freed with its holder: the device of that memory
// must be current then, which ia_destroy / ia_index_destroy see to)
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return IA_OK;
    release();
    size_t want = std::max<size_t>(bytes, 256);
    if (hipMalloc(&p, want) != hipSuccess) {
      p = nullptr;  // (the destructor frees p)
      return fail(IA_ENOMEM, "hipMalloc of " + std::to_string(want) + " bytes failed");
    }
    cap = want;
    return IA_OK;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const {
    return reinterpret_cast<T *>(p);
  }
};

struct JobBufs {  // moved, never copied, when ia_ctx::jb grows (earlier jobs' buffers stay live)
  DevBuf B, Bc, Bpc, Bp, S, IM, W, DSRC, DDIST, pstat, NN;
};

inline int kh_for(int d_plus_norm) {  // smallest instantiated K3 width that holds d + norm column
  if (d_plus_norm <= 56) return 28;
  if (d_plus_norm <= 112) return 56;
  if (d_plus_norm <= 168) return 84;
  return -1;
}

// device-side waits (handoffs, exchange flags) give up after 20 s of the 100 MHz s_memrealtime clock
static constexpr long long IA_WAIT_TICKS = 2000000000LL;

static inline int64_t tile_pad(int64_t n) { return (n + IA_TILE - 1) / IA_TILE * IA_TILE; }

// a level's share of the process-wide budget of handoff-chained waves (ia_ctx.cpp g_chain_waves),
// returned when the level call ends
struct ChainReservation {
  int n = 0;
  ~ChainReservation();
  bool take(int w, int budget);
};
int chain_waves_in_flight();

// ia_comm.cpp
int xchg_alloc(ia_ctx *c, int world, bool fresh = false);
void comm_close(ia_ctx *c);  // the communicator and the peers' IPC mappings (ia_destroy)
bool shard_level(int64_t n_tiles, int world);

}  // namespace ia_host

using ia_host::DevBuf;
using ia_host::JobBufs;

struct __attribute__((visibility("hidden"))) ia_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  // uploads (IA_MEM_HOST) and per-level scratch
  DevBuf A, Ac, Ap, Apc;
  std::vector<JobBufs> jb;  // per job of a batch: B-side uploads / outputs, stats words
  DevBuf jobs;              // device JobPtrs[n_jobs]
  DevBuf db, db64, mu, Rbits, q64, qn2, qf, rec, recT, win, allwin, counters, absmax;
  // certified pruned scan (option "prune"): per-level basis, sorted DB table, tile boxes
  DevBuf pr_part, pr_cov, pr_basis, pr_proj, pr_keys, pr_rows, pr_tmp, pos2row, boxes, qinfo, pairs;
  DevBuf qs_order, qs_info, qs_frag, qs_tbox;  // presorted queries of a step (K2s, or the fused gathers' sort)
  DevBuf tnorm;  // per DB tile of a pruned level: R_t >= max |a'| over its rows
  DevBuf sim;    // k-coherence levels (ia_synthesize_levels_kcoh): the similarity sets of a host-memory call,
  DevBuf kc_part, kc_cnt;  // ... and their scan waves' minima and counts (ia_kcoh.hip KcohScan)
  DevBuf mk_mask, mk_off, mk_list;  // masked resynthesis (ia_synthesize_levels_masked): the jobs' masks, the step offsets and lists
  int64_t mk_levels = 0;            // ... and its totals (ia_masked_stats): levels run, device ms of their lists
  double mk_list_ms = 0.;
  DevBuf py_in, py_tmp, py_sm, py_mm, py_out;  // GPU preprocessing (ia_gaussian_pyramid, ia_color_matrix)
  std::vector<double> basis_h;   // staging of the basis upload (lives until the copy ran)
  int64_t prune_min_rows = IA_PRUNE_MIN_ROWS;  // option "prune_min_rows": smallest DB that prunes
  int prune = 1;
  int row_source = 0;            // option "row_source": exact rows from 0 = the fp64 row DB (1 = the A images,
                                 // measured slower, is in git history only)
  int shard_emulate = 1;         // option "shard_emulate": W > 1 runs a W-way DB shard on this device
  int shard_unpruned = 0;        // option "shard_unpruned": 1 = shard levels that scan unpruned too
  int prune_group = 1;           // option "prune_group": Morton tiles interleaved in groups of G (ia_prune.hip k_make_table)
  int matcher = IA_MATCH_F16X3;  // option "matcher"
  int k3p_variant = 24;          // option "k3p_variant": pruned-scan kernel version (ia_k3h.hip k3h_prune*),
                                 // 24 / 25 two passes (a hi stream three tiles deep, then
                                 // the passing tiles' chains); 22 hi-only stream with the chains one tile later;
                                 // 20 / 21 whole tiles, corrections fused on query-tile pairs.  In-kernel sort up
                                 // to 512 queries (20, 22, 24), presorted above (21, 25); the other versions are
                                 // in git history
  int k3_variant = 1;            // option "k3_variant": K3h epilogue (1 = packed index, the only one built)
  int k3p_blocks = 1;            // option "k3p_blocks": 1 = a wide step's presorted pruned scan is one launch over
                                 // all its query blocks (2-D grid); 0 = one launch per block
  int fuse_gather = 1;           // option "fuse_gather": 1 = K4 of step t and K2p of step t + 1 in one launch
  int fuse_unpruned = 0;         // option "fuse_unpruned": 1 = also on unpruned levels (K4 + K2h)
  HandSlot *hand = nullptr;      // its per-row handoff slots (uncached)
  int hand_rows = 0;
  int prefetch_next = 1;         // option "prefetch_next" (NextStep::prefetch)
  int early_gather = 1;          // option "early_gather" (NextStep::early)
  int gather_wave = 1;           // option "gather_wave" (NextStep::gwave): the early path on two-wave workgroups
  int nn_bound = 1;              // option "nn_bound" (JobPtrs::nn): the pruned one-rank levels' gathers also
                                 // bound U' by the causal neighbours' exact NN rows, shifted
  int fuse_sort = 0;             // option "fuse_sort": the fused gathers of step t + 1 also sort it (NextStep::kslot);
                                 // 2 = on levels whose widest step has >= IA_FUSE_SORT_MINQ queries; off by
                                 // default: no gain left with nn_bound
  int chain_budget = 0;          // waves of handoff-chained launches this context's CUs hold deadlock-free
  int scan_wgs = IA_NWG_H;       // option "scan_wgs": workgroups of a pruned scan launch (<= one per CU)
                                 // (ia_init: 2 x the resident merge-gather waves - a margin; see g_chain_waves)
  unsigned long long *kslot = nullptr;  // their per-query key slots (uncached)
  int kslot_n = 0;
  unsigned hseq = 0;
  // per-step K3 timing (optional)
  int time_dist = 0;
  int stamps = 0;                 // option "stamps": per-launch device time from kernel stamps
  int rec_wt = 1;                 // option "rec_wt": K3p records stored write-through
  DevBuf stamp_k3, stamp_mg, stamp_dur;
  std::vector<hipEvent_t> evs, evg, evm;  // sampled steps: K3, K2 and K4 brackets
  hipEvent_t lv0 = nullptr, lv1 = nullptr, lv2 = nullptr;
  hipEvent_t kb[4] = {nullptr, nullptr, nullptr, nullptr};  // per level: K1b start / end, K1 start / end
  // multi-GPU
  int rank = 0, world = 1;
  ncclComm_t comm = nullptr;
  int exchange = 0;               // option "exchange": 0 = RCCL all-gather + finish, 1 = peer-write merge,
                                  // 2 = owner-computes (rank o owns job o; every rank scans its shard for all)
  DevBuf xo_inv;                  // exchange = 2: the owners' query -> slot tables of the current step
  int xo_presort = 0;             // option "xo_presort": 1 = owners always sort with K2s (tests)
  int xo_wait = 0;                // option "xo_wait": 1 = the fused merge waits for every owner's next
                                  // queries (one wave), so the next scan does not spin on all CUs
  void *xbuf = nullptr;           // this process's exchange buffer (uncached, IPC-exportable)
  int xbuf_w = 0;                 // ranks the buffer was sized for
  XSlot *xpeer[IA_XCHG_MAXW] = {};  // every rank's buffer in this address space (ia_xchg_open)
  bool xmapped[IA_XCHG_MAXW] = {};  // opened through hipIpcOpenMemHandle (closed on destroy)
  unsigned xseq = 0;              // exchange sequence number (one per sharded step, same on every rank)
  bool xfresh = false;            // the buffer was zeroed by ia_xchg_alloc and not opened since
  DevBuf xerr;
  // level pipelining: a recording context publishes, per level call (a
  // generation), the wavefront steps it has enqueued, each followed by an event; a context told
  // to depend on it (ia_pipeline_depend) makes each of its steps wait for the steps of that
  // generation it reads from (level l + 1 step t reads B' of level l steps <= t / 2 + 4)
  int p_record = 0;                          // option "pipeline_record"
  int p_last = 0;                            // option "pipeline_last": the next level call has no
                                             // dependents (no per-step events; one call only)
  std::vector<hipEvent_t> p_ev[3];           // per generation mod 3: one event per step
  std::atomic<long long> p_enq{-1};          // last step of the current generation enqueued
  std::atomic<long long> p_T{0};             // steps of the current generation
  std::atomic<int> p_gen{0}, p_done{0};      // current / last finished generation
  ia_ctx *dep = nullptr;                     // the next level call waits on dep's generation dep_gen
  int dep_gen = 0;
};

struct __attribute__((visibility("hidden"))) ia_index {
  ia_ctx *ctx = nullptr;
  int64_t n = 0;
  int d = 0, KH = 0, n_tiles = 0, tpw = 0, nwg = 0;
  double sc = 1.;             // power-of-two prescale of the centred fp32 copy (ia_dense.hip)
  std::vector<double> mu_h;   // column means (the queries' range check)
  DevBuf pts, db, mu, Rbits, q, q64, qn2, qf, rec, recT, idx, dist, counters;  // idx / dist: batch x k results
  DevBuf cpx, cs, cim, cout;  // ia_coherence_batch staging
  unsigned long long knn_stats[2] = {0, 0};  // the last ia_index_query_knn call: exact rows, chunks rescanned
  // fixed-radius search (ia_index_radius.cpp): per batch the radii, thresholds, per-(query, workgroup)
  // counts and segments, per-query totals and offsets, result counts; per fill sub-batch the
  // candidates (row, distance) and the staged results
  DevBuf r_rad, r_thr, r_cnt, r_seg, r_ts, r_qoff, r_soff, r_cntq, r_wr, r_wd, r_sidx, r_sdist;
  int64_t workspace = 0;                  // ia_index_set_workspace: candidate entries per fill pass (0: default)
  int64_t radius_stats[4] = {0, 0, 0, 0};  // the last radius call (ia_index_radius_stats)
};

// the index's query driver (ia_index.cpp), shared by ia_index_query, ia_index_query_knn and the
// radius search (ia_index_radius.cpp)
namespace ia_host __attribute__((visibility("hidden"))) {

static constexpr int64_t IA_INDEX_BATCH = 4096;  // queries scanned against the DB at a time

// the prescaled fp32 copy of a query must stay far inside fp32: refuses (as entry point who) queries
// farther than 2^100 times the rows' spread from their mean (the rows themselves are <= 1 there),
// and NaN / inf
int index_check_queries(const ia_index *x, const std::string &who, const double *q, int64_t nq);
// allocates x->q, x->qn2 and x->qf for the batches of nq queries; every entry point's first
// allocation, before it takes a device pointer of the index
int index_reserve_batch(ia_index *x, int64_t nq);
// The dense rules of the index, which the window level (ia_level_nbhd.cpp) runs on its own rows.
// Scan decomposition of n_tiles DB tiles: tiles per workgroup, workgroups.
inline void dense_geometry(int n_tiles, int *tpw, int *nwg) {
  *tpw = std::max(4, (n_tiles + IA_WG_TARGET - 1) / IA_WG_TARGET);
  *nwg = (n_tiles + *tpw - 1) / *tpw;
}
// prescale of the centred fp32 copy: 2^-e with the largest centred |value| amax in [2^(e-1), 2^e), so
// the fp32 scan sees values in [0.5, 1) (|e| <= 500 keeps sc^2 a normal fp64; an all-equal DB keeps 1)
inline double dense_prescale(double amax) {
  return amax > 0. ? std::ldexp(1.0, -std::max(-500, std::min(500, std::ilogb(amax) + 1))) : 1.;
}
// the arguments of a dense merge (k_merge_dense, _knn) over the whole unpruned, unsharded DB
inline MergeArgs dense_merge_args(const float4 *rec, const float *recT, const double *qn2, const unsigned *Rbits, int nwg,
                                  int tpw, int n_tiles, int64_t n, int KH) {
  MergeArgs ma;
  ma.db64 = nullptr;
  ma.rec = rec;
  ma.recT = recT;
  ma.q64 = nullptr;
  ma.qn2 = qn2;
  ma.Rbits = Rbits;
  ma.nwg = nwg;
  ma.tpw = tpw;
  ma.pos0 = 0;
  ma.pos_end = n_tiles * IA_TILE;
  ma.NT = n_tiles;
  ma.NA = (int)n;
  ma.pos2row = nullptr;
  ma.rr = 0;
  ma.qinfo = nullptr;
  ma.boxes = nullptr;
  ma.ufac = 0.;
  ma.img_rows = 0;
  ma.eps_c = ia_eps_c(2 * KH);
  ma.eps_a = 0.;
  return ma;
}
// the merge arguments of an index: its records (x->rec, x->recT, x->qn2 as allocated now) over the whole DB
inline MergeArgs index_merge_args(const ia_index *x) {
  return dense_merge_args(x->rec.as<float4>(), x->recT.as<float>(), x->qn2.as<double>(), x->Rbits.as<unsigned>(), x->nwg,
                          x->tpw, x->n_tiles, x->n, x->KH);
}
// per batch of IA_INDEX_BATCH queries: uploads the queries b0 .. b0 + nb to x->q (q = nullptr: copies
// the index's own rows b0 .. b0 + nb there, on the device), builds x->qn2 and
// x->qf (Mpad = nb padded to qtt query tiles), then body(b0, nb, Mpad, qtt), which enqueues its scans
// and merge, copies its results and waits for the stream; stops at the first status that is not IA_OK
int index_for_batches(ia_index *x, const double *q, int64_t nq, const std::function<int(int64_t, int, int, int)> &body);
// the query tiles [qta, qtb) in launches of at most ia_k3_qtmax(KH): launch(first tile, tiles)
template <class F>
void index_scan_tiles(int KH, int qta, int qtb, F &&launch) {
  const int qtmax = ia_k3_qtmax(KH);
  for (int qt0 = qta; qt0 < qtb; qt0 += qtmax) launch(qt0, std::min(qtmax, qtb - qt0));
}

}  // namespace ia_host

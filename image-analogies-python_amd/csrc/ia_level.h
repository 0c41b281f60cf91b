// ia_level.h — what the phases of a level call (ia_synthesize_levels) hand to each other: the
// plan, the staged inputs, a step's descriptor, the stamp slots, the scan tally and the link
// between pipelined levels, and the phase functions that ia_level_plan.cpp, ia_level_stats.cpp
// and ia_level_kcoh.cpp define for the level call in ia_level_run.cpp (its steps: ia_level_run.h), and
// what ia_level_nbhd.cpp's call (other window sizes) and ia_level_mask.cpp's (masked resynthesis) take from them.
#pragma once
#include <chrono>
#include <thread>

#include "ia_host.h"

namespace ia_host __attribute__((visibility("hidden"))) {

// ---- phase 1: the plan ----------------------------------------------------------------------
struct Shard {
  int t0, t1, nwg, tpw;  // storage tiles [t0, t1) of the level's DB, scan decomposition
};

// What a level call decides before it builds the DB.  plan_shards fills the geometry and how the
// level is sharded and exchanged; plan_scan, once the matcher is known (one device read-back),
// the scan's decomposition and buffer sizes.
struct LevelPlan {
  LevelGeo g;
  int J = 1, DP = 0;                  // jobs of the batch; fp32 columns of a DB row
  size_t nA = 0, nAc = 0, nB = 0, nBc = 0;  // doubles of an A / coarse A / B / coarse B image
  int64_t NB = 0;                     // pixels of the B level
  bool sharded = false, emulated = false, multi = false;
  bool xchg = false;                  // peer-write winner exchange (k_merge_xchg)
  bool xo = false;                    // owner-computes sharded steps (exchange = 2, ia_internal.h XOLayout)
  int Wsh = 1;                        // shards of this level
  // plan_scan
  bool use_h = false, prune = false;  // split-f16 matcher; certified pruned scan
  int64_t T = 0, Mmax = 0;            // wavefront steps, queries of the widest step of one job ...
  int64_t Mtmax = 0, Mpad_max = 0;    // ... and over all jobs (padded to query tiles)
  int xo_bpj = 1, xo_QTx = 1, xo_QTs = 1;  // owner geometry: per owner bpj blocks of QTx tiles, QTs = bpj QTx
  int ns = 0;                         // DB tiles this process holds
  std::vector<Shard> shards;          // the shards this process scans
  size_t rec_stride = 0;              // records of one shard's scan
  size_t db_row_bytes = 0, tile_bytes = 0;  // one stored DB row (hi+lo f16 / fp32 per column) / tile
  int qtmax = 0;                      // query tiles of one scan launch's block
  int stride = 0;                     // option "time_dist": every stride-th step is sampled (0: none)
};

// ---- phase 2: staging -----------------------------------------------------------------------
struct LevelInputs {
  std::vector<JobPtrs> jp;  // per job: its B side on the device
  Imgs Aim, Bim;            // the A side; the B shape (images per job: JobPtrs)
  APairs Apairs;            // the A side's per-image strides (the DB builders; 0: one shared A)
  JobSet jobs() const { return JobSet{jp[0], dev_jobs, (int)jp.size()}; }
  JobSet job(int j) const { return JobSet{jp[j], dev_jobs + j, 1}; }
  const JobPtrs *dev_jobs = nullptr;
};

// ---- what the steps share -------------------------------------------------------------------
// Step t of the level for J jobs stepped together (J = 1: one owner's view of a batched step).
// M <= 0: the step holds no query (levels narrower than 3 columns); the callers skip it.
inline StepDesc step_desc(const LevelGeo &g, int64_t t, int J) {
  StepDesc sd{(int)t, 0, 0, 0, J};
  ia_wavefront_step(g.bh, g.bw, t, &sd.r0, &sd.M);
  sd.Mpad = (int)tile_pad(J * sd.M);
  return sd;
}

// Level pipelining: this level's per-step events (a recording context) and its
// waits on the level before it (ia_pipeline_depend).  Every return after open() - errors too -
// releases the dependents' waits (p_done).
struct PipelineLink {
  ia_ctx *c = nullptr;
  int gen = 0;                      // this call's generation (0: not recording)
  std::vector<hipEvent_t> *pev = nullptr;
  bool no_events = false;           // option "pipeline_last": nothing waits on this call's steps
  ia_ctx *dp = nullptr;             // the context of the level before, its generation
  int dgen = 0;
  int64_t waited = -1;
  // the previous level's host thread stopped enqueueing (it failed): 120 s without progress of
  // its generation or its enqueued steps (a long but healthy predecessor keeps resetting this)
  std::chrono::steady_clock::time_point t_prog;
  long long seen_enq = -2;
  int seen_gen = -1;

  int open(ia_ctx *ctx, int64_t T) {
    c = ctx;
    const int g = c->p_record ? c->p_gen.load() + 1 : 0;
    if (g) {
      pev = &c->p_ev[g % 3];
      while ((int64_t)pev->size() < T) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        pev->push_back(e);
      }
      c->p_enq.store(-1);
      c->p_T.store(T);
      c->p_gen.store(g);  // published last: a dependent reads p_T / p_enq of this generation after it
    }
    gen = g;
    dp = c->dep;
    dgen = c->dep_gen;
    c->dep = nullptr;  // one level call per ia_pipeline_depend
    c->dep_gen = 0;
    t_prog = std::chrono::steady_clock::now();
    no_events = c->p_last != 0;
    c->p_last = 0;
    return IA_OK;
  }
  ~PipelineLink() {
    if (gen) c->p_done.store(gen);
  }
  bool stalled() {
    const auto now = std::chrono::steady_clock::now();
    const long long e = dp->p_enq.load();
    const int gn = dp->p_gen.load();
    if (e != seen_enq || gn != seen_gen) {
      seen_enq = e;
      seen_gen = gn;
      t_prog = now;
      return false;
    }
    return now - t_prog > std::chrono::seconds(120);
  }
  // step t reads B' of the previous level's steps <= t / 2 + 4
  int wait_dep(int64_t t) {
    if (!dp) return IA_OK;
    while (dp->p_gen.load() < dgen && dp->p_done.load() < dgen)  // it has started that level
      if (stalled()) return fail(IA_ECOMM, "pipeline: the previous level did not start");
      else std::this_thread::yield();
    const int64_t need = std::min<int64_t>(t / 2 + 4, dp->p_T.load() - 1);
    if (need <= waited) return IA_OK;
    while (dp->p_done.load() < dgen && dp->p_enq.load() < need)
      if (stalled()) return fail(IA_ECOMM, "pipeline: the previous level stopped enqueueing");
      else std::this_thread::yield();
    if (dp->p_done.load() < dgen) {
      hipEvent_t ev = dp->p_ev[dgen % 3][need];
      // the previous level usually runs far ahead: an event that already completed needs no
      // barrier packet on this stream
      if (hipEventQuery(ev) != hipSuccess) HIP_TRY(hipStreamWaitEvent(c->st, ev, 0));
    }
    waited = need;
    return IA_OK;
  }
  void mark_step(int64_t t) {
    if (!gen) return;
    if (!no_events) hipEventRecord((*pev)[t], c->st);
    c->p_enq.store(t);
  }
};

// Option "stamps" (pruned levels): per-launch workgroup stamps of every K3p launch (<= IA_NWG_H
// workgroups each) and every fused merge launch (<= Mpad_max + J + 1 workgroups).  The slots
// start zeroed (fresh buffers here), and the slots a level wrote are cleared on EVERY exit
// (an early error return after some stamped launches left non-zero slots that a
// later, smaller launch would have read).
struct StampSlots {
  ia_ctx *c = nullptr;
  bool on = false;
  int64_t k3_cap = 0, mg_cap = 0, k3_n = 0, mg_n = 0;
  int mg_stride = 0;
  int open(ia_ctx *ctx, const LevelPlan &P) {
    c = ctx;
    on = c->stamps && P.prune;
    k3_cap = P.T * (int64_t)P.shards.size() * (c->k3p_blocks ? 1 : 8);
    mg_stride = (int)P.Mpad_max + P.J + 64;
    mg_cap = P.T * (P.xo ? P.J : 1);  // merge launches per step: one, or one per owned job (exchange 2)
    if (!on) return IA_OK;
    int rc;
    const size_t k3b = (size_t)k3_cap * IA_NWG_H * 16, mgb = (size_t)mg_cap * mg_stride * 16;
    const bool fresh_k3 = c->stamp_k3.cap < k3b, fresh_mg = c->stamp_mg.cap < mgb;
    if ((rc = c->stamp_k3.ensure(k3b)) || (rc = c->stamp_mg.ensure(mgb)) ||
        (rc = c->stamp_dur.ensure((size_t)(2 * k3_cap + mg_cap) * 16)))
      return rc;
    if (fresh_k3) HIP_TRY(hipMemsetAsync(c->stamp_k3.p, 0, c->stamp_k3.cap, c->st));
    if (fresh_mg) HIP_TRY(hipMemsetAsync(c->stamp_mg.p, 0, c->stamp_mg.cap, c->st));
    return IA_OK;
  }
  unsigned long long *k3() {  // the next scan launch's slots (nullptr: not stamped)
    return on && k3_n < k3_cap ? c->stamp_k3.as<unsigned long long>() + (size_t)2 * IA_NWG_H * k3_n++ : nullptr;
  }
  unsigned long long *mg() {  // the next merge launch's
    return on && mg_n < mg_cap ? c->stamp_mg.as<unsigned long long>() + (size_t)2 * mg_stride * mg_n++ : nullptr;
  }
  void durations() {  // per-launch device ticks: K3p launches first, then the merges
    if (!on) return;
    unsigned long long *dur = c->stamp_dur.as<unsigned long long>();
    ia_launch_stamp_durations(c->stamp_k3.as<unsigned long long>(), (int)k3_n, IA_NWG_H, dur, c->st, dur + 2 * (k3_n + mg_n));
    ia_launch_stamp_durations(c->stamp_mg.as<unsigned long long>(), (int)mg_n, mg_stride, dur + 2 * k3_n, c->st);
  }
  ~StampSlots() {
    if (k3_n) (void)hipMemsetAsync(c->stamp_k3.p, 0, (size_t)k3_n * IA_NWG_H * 16, c->st);
    if (mg_n) (void)hipMemsetAsync(c->stamp_mg.p, 0, (size_t)mg_n * mg_stride * 16, c->st);
  }
};

// What the scan launches of a level add up to (ia_stats), and the event bracket of a sampled
// step's scans.  Each launch states its own quantities: the (DB tile, query tile) pairs and tile
// visits an unpruned scan would make, its MFMA flops (unpruned; the pruned kernels count their
// pairs), and for a pruned launch the algorithmic bytes besides its DB stream - tile boxes, query
// fragments and pruning records, K3 records written - and the whole tiles of its DB range.
struct ScanTally {
  ia_ctx *c;
  int stride;
  bool timed = false;           // the current step is sampled
  int64_t n_rec = 0;            // sampled steps
  int64_t dist_launches = 0, launches_timed = 0;
  double dist_flops = 0., flops_timed = 0., pairs_full = 0., tiles_full = 0.;
  double bytes_all_fixed = 0., bytes_timed_fixed = 0.;
  double db_cap_all = 0.;       // each launch's tiles counted once (a launch of nqb query blocks streams a tile once per block)
  void begin_step(int64_t t) {
    timed = stride && t % stride == 0;
    if (timed) hipEventRecord(c->evs[2 * n_rec], c->st);
  }
  void end_step() {
    if (timed) hipEventRecord(c->evs[2 * n_rec++ + 1], c->st);
  }
  // per-workgroup counter slots of the pruned scan: [pairs | pairs (timed steps) | tiles | tiles
  // (timed) | extra half-tiles | extra half-tiles (timed)][wg]
  unsigned long long *pairs() const { return c->pairs.as<unsigned long long>() + (timed ? IA_NWG_H : 0); }
  unsigned long long *tiles() const { return c->pairs.as<unsigned long long>() + (timed ? 3 : 2) * IA_NWG_H; }
  void add(double pairs, double tile_visits, double flops, bool pruned, double fixed_bytes, double db_bytes) {
    dist_flops += flops;
    pairs_full += pairs;
    tiles_full += tile_visits;
    dist_launches++;
    if (pruned) {
      bytes_all_fixed += fixed_bytes;
      db_cap_all += db_bytes;
    }
    if (timed) {
      flops_timed += flops;
      launches_timed++;
      bytes_timed_fixed += fixed_bytes;
    }
  }
};

// phases 1-3 (ia_level_plan.cpp), in the order ia_synthesize_levels calls them
int check_level_args(const ia_level_args *a);
int check_level_batch(const ia_level_args *args, int n_jobs);
int plan_shards(ia_ctx *c, const ia_level_args *args, int J, LevelPlan &P);
int stage_level(ia_ctx *c, const ia_level_args *args, const LevelPlan &P, LevelInputs &in);
int probe_matcher(ia_ctx *c, const LevelPlan &P, const LevelInputs &in, bool *use_h);
int plan_scan(ia_ctx *c, bool use_h, LevelPlan &P);
int stage_jobs(ia_ctx *c, const LevelPlan &P, LevelInputs &in);
int ensure_scratch(ia_ctx *c, const LevelPlan &P);
int build_level_db(ia_ctx *c, LevelPlan &P, const LevelInputs &in, double *ufac);

// the level's ia_stats (ia_level_stats.cpp): n_gm sampled steps' gather / merge brackets
int accumulate_stats(ia_ctx *c, const LevelPlan &P, const StampSlots &stamps, const ScanTally &tally, int64_t n_gm,
                     double gather_bytes_timed, ia_stats *stats);
int accumulate_kcoh_stats(ia_ctx *c, const LevelPlan &P, ia_stats *stats);  // a k-coherence level's
// What a level of any side path (k-coherence, window, masked) adds: pixels, steps, scan launches, the
// coherence and kappa counters, and - when the level built a DB - its lv0 / lv1 / lv2 brackets.  tail: the
// stats words and the two brackets as read, for the caller's own fields.
struct SideTail {
  unsigned long long ctr[5] = {0, 0, 0, 0, 0};
  float ms_db = 0.f, ms_syn = 0.f;
};
int accumulate_side_stats(ia_ctx *c, int64_t pixels, int64_t steps, int64_t scans, bool built, ia_stats *stats,
                          SideTail *tail = nullptr);

// phase 5 (ia_level_run.cpp): the stats words' reduction, the D2H copies of host-memory jobs, the
// level's one sync, and the error word of the handoffs (chain) and exchanges
int finish_level(ia_ctx *c, const ia_level_args *args, const LevelPlan &P, const LevelInputs &in, bool chain, bool want_stats);

// k-coherence levels (ia_level_kcoh.cpp): what the sets, the context and the batch must be for
// one, and the level after plan_shards and stage_level
int check_kcoh(ia_ctx *c, const ia_level_args *args, int J, const int32_t *sim, int sim_k);
int run_kcoh_level(ia_ctx *c, const ia_level_args *args, LevelPlan &P, LevelInputs &in, const int32_t *sim_in, int K,
                   ia_stats *stats);

// the side paths' refusal rule (ia_level_nbhd.cpp): sharded, pipelined (a pending ia_pipeline_depend is
// consumed here) and debug-recording calls; who: the entry point the message names, what: its subject
int refuse_side_path(ia_ctx *c, const ia_level_args *args, int J, const std::string &who, const std::string &what);

// The two window calls (ia_level_nbhd.cpp; ia_level_mask.cpp, §13).  What the sizes, the
// context and the batch must be (who: the entry point the refusals name); the prologue after the checks
// (plan_shards with P.g.D = w.D, stage_level); the window call's level after it.
int check_nbhd(ia_ctx *c, const ia_level_args *args, int J, int n_sm, int n_lg, const std::string &who = "ia_synthesize_levels_nbhd");
int plan_nbhd_level(ia_ctx *c, const ia_level_args *args, int J, const NbhdGeo &w, LevelPlan &P, LevelInputs &in);
int run_nbhd_level(ia_ctx *c, const ia_level_args *args, LevelPlan &P, LevelInputs &in, const NbhdGeo &w, ia_stats *stats);
// What a window level's steps share, in the order a level fills it: ensure_nbhd_steps sizes the step
// buffers (q64, qn2, qf, rec, recT, win, allwin) for a largest step of Mt_max queries and sets the scan's
// decomposition; build_nbhd_db builds the DB between lv0 and lv1 (fp64 rows, finite check, fp32 tiles)
// and sets their prescale and the merges' arguments; run_nbhd_step runs one step (ia_launch.h NbhdStep:
// a wavefront step or a slice of a masked level's list) and returns its scan launches.
struct NbhdScan {
  int tpw = 0, nwg = 0;
  double sc = 1.;
  MergeArgs ma;
};
int ensure_nbhd_steps(ia_ctx *c, const LevelGeo &g, const NbhdGeo &w, int64_t Mt_max, NbhdScan *scan);
int build_nbhd_db(ia_ctx *c, const LevelPlan &P, const LevelInputs &in, const NbhdGeo &w, const std::string &who, NbhdScan *scan);
int64_t run_nbhd_step(ia_ctx *c, const LevelGeo &g, const LevelInputs &in, const NbhdGeo &w, const NbhdScan &scan,
                      const NbhdStep &step);

}  // namespace ia_host

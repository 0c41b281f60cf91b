// ia_level_run.h — LevelRun, phase 4 of a level call: what the steps of one level share, and the
// rules a step's producers and consumers must agree on, each written once (the chunk count of a
// one-launch scan, the path-independent half of a scan launch, the owner's layout of a step).
// The one-rank, all-gather and peer-write steps are defined in ia_level_run.cpp, the
// owner-computes steps (exchange = 2) in ia_level_owner.cpp.
#pragma once
#include "ia_level.h"

namespace ia_host __attribute__((visibility("hidden"))) {

struct QBufs {  // the query buffers of one step
  double *q64, *qn2;
  float4 *qinfo;
};

// DB chunks of a scan that runs its nqb query blocks as one launch over `tiles` DB tiles: a
// multiple of 8 (the blocks of a chunk on one XCD) when that loses little.  Records per query =
// chunks, so the merge of the step indexes with the same number.
inline int scan_chunks(int tiles, int nqb) {
  int nch = std::max(1, std::min(tiles, IA_NWG_H / nqb));
  if (nch >= 64) nch &= ~7;
  return nch;
}

// How the owners lay out a step of M queries each (ia_internal.h XOLayout).  Both the step's own
// launches and the fused merge of the step before (which runs its gather, and publishes its
// queries only when ink) read it from LevelRun::owner_layout.
struct OwnerLayout {
  int Mpj;   // one owner's padded queries
  bool ink;  // owners whose step fits one launch's query tiles skip K2s: K2p publishes the unsorted
             // queries and each K3p block sorts its owner's queries itself (XOPub)
  int QTs;   // tiles per owner in this step's layout
  int Mrec, nqb, nch;
};

// One owner-computes sharded step (exchange = 2): every local owner (a rank: its own job;
// emulated: job j = owner j, each at its own tile-aligned offset) gathers its queries (K2p) and
// sorts them into every rank's area (K2s); this process's shard scans (K3p) run for all owners'
// queries and push their records to the owners; each local owner's fused merge (K4) runs over
// W nch records per query.  The emulated launches are exactly the ranks' launches, one after the
// other.
struct OwnerStep : OwnerLayout {
  unsigned seq;
  char *loc;    // this process's area of the step's parity
  StepDesc s1;  // one owner's step
};

struct LevelRun {
  ia_ctx *c;
  const LevelPlan &P;
  const LevelGeo &g;
  const LevelInputs &in;
  StampSlots &stamps;
  PipelineLink &link;
  ScanTally tally;
  double ufac;
  MergeArgs ma;                     // the level's merge arguments; per shard: its records,
  std::vector<MergeArgs> mas;       // decomposition, DB positions (and table / boxes when pruned);
  MergeArgs mxo;                    // an owner's (exchange = 2), but for its step's fields
  std::vector<int64_t> shard_rows;  // real DB rows in each shard (unpruned flops)
  bool chain = false;               // fused K4(t) + K2(t + 1) launches, handoff-chained (option "fuse_gather")
  ChainReservation &chain_res;
  bool gwave = false;               // ... as two-wave workgroups, reserved as such (option "gather_wave")
  bool fsort = false;               // their gathers may also sort the next step (option "fuse_sort")
  int64_t gathered = -1;            // the step whose gather the previous fused launch ran
  bool gsort = false;               // ... and that launch also sorted it (no K2s, no in-scan sort)
  int64_t n_gm = 0;                 // sampled steps (gather / merge brackets)
  double gq_bytes = 0., gather_bytes_timed = 0.;

  LevelRun(ia_ctx *ctx, const LevelPlan &plan, const LevelInputs &inputs, StampSlots &s, PipelineLink &l, ChainReservation &r,
           double uf)
      : c(ctx), P(plan), g(plan.g), in(inputs), stamps(s), link(l), tally{ctx, plan.stride}, ufac(uf), chain_res(r) {}

  void init_merge_args();
  int init_chain();
  int step(int64_t t);

  // query buffers of step t (chain: parity half t & 1)
  QBufs qhalf(int64_t t) const {
    const size_t h = chain && (t & 1) ? 1 : 0;
    return QBufs{c->q64.as<double>() + h * P.Mpad_max * g.D, c->qn2.as<double>() + h * P.Mpad_max,
                 P.prune ? c->qinfo.as<float4>() + h * 3 * P.Mpad_max : nullptr};
  }
  // a step's merge also runs the next step's gather; not on sampled steps (their K2 / K4 brackets)
  bool fuses_next(int64_t t) const {
    return chain && t + 1 < P.T && !(P.stride && (t % P.stride == 0 || (t + 1) % P.stride == 0));
  }
  // algorithmic bytes of a pruned launch besides its DB tiles
  double scan_fixed_bytes(double tile_visits, double query_slots, double rec_bytes) const {
    return tile_visits * 32 + query_slots * (16.0 * 16 * g.KS + 48) + rec_bytes;
  }
  const char *shard_db(const Shard &x) const { return (const char *)c->db.p + (size_t)(x.t0 - g.tile0) * P.tile_bytes; }
  NextStep next_step(const StepDesc &sn, int jl, size_t q0n);

  // The scan launch of shard i in step sd, but for what its path sets: the query sources, qt, qt0,
  // nwg, nqb, qt_end, M, Mpad, rec, recT, xo.  launch_scan takes the launch's stamp slots and
  // launches it.
  K3pLaunch scan_base(size_t i, const StepDesc &sd) const {
    const Shard &x = P.shards[i];
    K3pLaunch k{};
    k.db = shard_db(x);
    k.NT = x.t1 - x.t0;
    k.boxes = mas[i].boxes;
    k.pos2row = mas[i].pos2row;
    k.tnorm = P.prune ? c->tnorm.as<float>() + x.t0 : nullptr;
    k.pairs = tally.pairs();
    k.tiles = tally.tiles();
    k.step = sd.t;
    k.r0 = sd.r0;
    k.rec_wt = c->rec_wt;
    return k;
  }
  int launch_scan(K3pLaunch &k, bool presorted) {
    k.stamp = stamps.k3();
    if (ia_launch_k3p(k, c->k3p_variant, presorted, c->st)) return fail(IA_EINVAL, "pruned scan: no kernel instance for k3p_variant");
    return IA_OK;
  }

  // ---- one-rank, all-gather and peer-write steps (ia_level_run.cpp)
  void gather(const StepDesc &sd, const QBufs &q);
  int scan(const StepDesc &sd, const QBufs &q);
  int merge(const StepDesc &sd);  // one of:
  int merge_fused_next(const StepDesc &sd);
  void merge_fused(const StepDesc &sd);
  void merge_peer_write(const StepDesc &sd);
  int merge_all_gather(const StepDesc &sd);

  // ---- owner-computes steps (ia_level_owner.cpp)
  void init_owner_merge_args();
  int owner_of(int jl) const { return P.sharded ? c->rank : jl; }
  char *xo_area(int p, unsigned seq) const;
  void xo_areas(char *(&area)[IA_XCHG_MAXW], int n, unsigned seq) const;
  XOPub owner_pub(int jl, int Mpj, unsigned seq) const;
  OwnerLayout owner_layout(int M) const;
  OwnerStep owner_step(const StepDesc &sd);
  void owner_sort(const StepDesc &sd, const OwnerStep &os, const QBufs &q, int jl);
  void owner_gather(const StepDesc &sd, const OwnerStep &os, const QBufs &q);
  int owner_scan(const StepDesc &sd, const OwnerStep &os);
  int owner_merge(const StepDesc &sd, const OwnerStep &os, const QBufs &q);
};

}  // namespace ia_host

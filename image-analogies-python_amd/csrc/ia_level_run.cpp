// ia_level_run.cpp — phases 4 and 5 of a level call and the call itself: the skewed wavefront's
// steps (gather, scan, merge of every form: one-rank, all-gather, peer-write, owner-computes),
// the links between pipelined levels, the results' copies and error words, and the entry points
// ia_synthesize_level(s) with the wavefront's pure shape helpers.
#include <rccl/rccl.h>  // the all-gather of a sharded step's winners (LevelRun::merge)

#include <chrono>
#include <thread>

#include "ia_level.h"

#if IA_PROBE & 16
void ia_k3p_probe_dump();
#endif

namespace ia_host {
namespace {

#define IA_FUSE_SORT_MAXW 768  // waves of a k_merge_gather launch whose gathers sort the next step
#define IA_FUSE_SORT_MINQ 512  // fuse_sort 2: the widest step's queries (all jobs) from which the gathers sort

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

// (re)allocates an uncached, zeroed device array once a level needs more elements than it holds
static int grow_uncached(ia_ctx *c, void **p, int *have, int64_t want, size_t elem_bytes) {
  if (*have >= want) return IA_OK;
  HIP_TRY(hipStreamSynchronize(c->st));
  if (*p) hipFree(*p);
  *p = nullptr;
  *have = 0;
  HIP_TRY(hipExtMallocWithFlags(p, (size_t)want * elem_bytes, hipDeviceMallocUncached));
  HIP_TRY(hipMemset(*p, 0, (size_t)want * elem_bytes));
  HIP_TRY(hipDeviceSynchronize());
  *have = (int)want;
  return IA_OK;
}

struct QBufs {  // the query buffers of one step
  double *q64, *qn2;
  float4 *qinfo;
};

// One owner-computes sharded step (exchange = 2, ia_internal.h XOLayout): every local owner (a
// rank: its own job; emulated: job j = owner j, each at its own tile-aligned offset) gathers its
// queries (K2p) and sorts them into every rank's area (K2s); this process's shard scans (K3p) run
// for all owners' queries and push their records to the owners; each local owner's fused merge
// (K4) runs over W nch records per query.  The emulated launches are exactly the ranks'
// launches, one after the other.
struct OwnerStep {
  unsigned seq;
  char *loc;    // this process's area of the step's parity
  StepDesc s1;  // one owner's step
  int Mpj;      // one owner's padded queries
  bool ink;     // owners whose step fits one launch's query tiles skip K2s: K2p publishes the unsorted
                // queries and each K3p block sorts its owner's queries itself (XOPub)
  int QTs;      // tiles per owner in this step's layout
  int Mrec, nqb, nch;
};

// ---- phase 4: the steps of one level --------------------------------------------------------
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
  std::vector<MergeArgs> mas;       // decomposition, DB positions (and table / boxes when pruned)
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

  void init_merge_args() {
    const bool prune = P.prune, use_h = P.use_h;
    ma.db64 = c->db64.as<double>();
    ma.rec = c->rec.as<float4>();
    ma.recT = c->recT.as<float>();
    ma.q64 = c->q64.as<double>();
    ma.qn2 = c->qn2.as<double>();
    ma.Rbits = c->Rbits.as<unsigned>();
    ma.nwg = g.nwg;
    ma.tpw = g.tiles_per_wg;
    ma.pos0 = g.tile0 * IA_TILE;
    ma.pos_end = g.tile1 * IA_TILE;
    ma.NT = g.n_tiles;
    ma.NA = (int)g.NA;
    ma.pos2row = g.pos2row;
    ma.rr = prune ? 1 : 0;
    ma.qinfo = prune ? c->qinfo.as<float4>() : nullptr;
    ma.boxes = prune ? c->boxes.as<float4>() : nullptr;
    ma.ufac = ufac;
    ma.img_rows = 0;  // (exact rows from the A images: git history only, option "row_source")
    ma.eps_c = use_h ? ia_eps_c_h(g.KS, prune || c->k3_variant == 1) : ia_eps_c(P.DP);
    ma.eps_a = use_h ? ia_eps_a_h() : 0.;
    mas.assign(P.shards.size(), ma);
    shard_rows.assign(P.shards.size(), 0);
    for (size_t i = 0; i < P.shards.size(); i++) {
      const Shard &x = P.shards[i];
      MergeArgs &m = mas[i];
      m.rec = c->rec.as<float4>() + i * P.rec_stride;
      m.recT = c->recT.as<float>() + i * P.rec_stride;
      m.nwg = x.nwg;
      m.tpw = x.tpw;
      m.pos0 = x.t0 * IA_TILE;
      m.pos_end = x.t1 * IA_TILE;
      if (prune) {
        m.pos2row = g.pos2row + (size_t)x.t0 * IA_TILE;
        m.boxes = c->boxes.as<float4>() + 2 * (size_t)x.t0;
        m.NT = x.t1 - x.t0;
      }
      for (int t = x.t0; t < x.t1 && !prune; t++) {
        const int64_t tr = ia_tile_perm(t, g.n_tiles);
        shard_rows[i] += std::min<int64_t>(IA_TILE, (g.NA - tr + g.n_tiles - 1) / g.n_tiles);
      }
    }
    // algorithmic bytes of one query's gather (K2h / K2p): its 55*ch features read, (K2p) the 12
    // causal coherence candidates' fp64 rows for U, the fp64 row + MFMA fragments + |q'|^2 (+ K2p's
    // pruning record) written
    gq_bytes = 55.0 * g.ch * 8 + (prune ? 12.0 * ia_db64_stride(g.ch) * 8 : 0.) + g.D * 8.0 +
               (use_h ? 16.0 * g.KS * 4 : P.DP * 4.0) + 8.0 + (prune ? 48.0 : 0.);
  }

  // Fused K4(t) + K2p(t + 1) (option "fuse_gather", ia_kernels.hip k_merge_gather): unsharded
  // pruned levels (<= 256 records per query: one launch's chunks, or nch <= 256 of a wide step's
  // 2-D launch), batched jobs with one handoff row set per job, and owner-computes steps (each
  // local owner's merge + its next gather, which publishes); the query buffers alternate by step
  // parity.  (Unpruned levels - K2h fused, option "fuse_unpruned" - measured slower: their longer
  // fused launches delay the pipelined finest level's scans, and cfg5's batched 512^2 steps lose
  // 1-2 %.)  A level chains only while the process-wide chained-wave budget (g_chain_waves) has
  // room for its widest launch: at most Mpad + J waves (merges, entering rows, pads).  Owner-
  // computes levels take the same reservation: their fused launches chain rows like any other
  // (and wait for peers' records besides, which never depend on a chained wave of this process).
  int init_chain() {
    static_assert(IA_NWG_H <= 4 * IA_WAVE, "k_merge_gather reads 4 records per lane");
    const int J = P.J;
    chain = c->fuse_gather && P.use_h && g.ch == 1 && g.bw >= 3 && (P.prune || c->fuse_unpruned) &&
            ((!P.multi && !P.xo && mas[0].nwg <= 4 * IA_WAVE) || (P.xo && P.prune));
    // (option "gather_wave": the early path of a one-job, one-rank pruned level whose gathers do
    // not sort runs two waves per query and reserves them; ia_chain_choice)
    const bool want_sort = P.prune && !P.xo && (c->fuse_sort == 1 || (c->fuse_sort == 2 && P.Mtmax >= IA_FUSE_SORT_MINQ));
    const bool two = c->gather_wave && c->early_gather && c->prefetch_next && P.prune && !P.multi && !P.xo && J == 1 && !want_sort;
    if (chain) {
      const int lw = (int)(P.Mpad_max + J) + (P.xo ? 1 : 0);
      // (another thread's level may take budget between the choice and the reservation: then the next smaller form)
      int form = ia_chain_choice(lw, chain_waves_in_flight(), c->chain_budget, two);
      while (form && !chain_res.take(form * lw, c->chain_budget)) form--;
      chain = form > 0;
      gwave = form == 2;
    }
    if (chain) {
      int rc;  // handoff slots per row of every job (local owner); key slots of the gathers' sort
      if ((rc = grow_uncached(c, (void **)&c->hand, &c->hand_rows, g.bh * J, sizeof(HandSlot))) ||
          (rc = grow_uncached(c, (void **)&c->kslot, &c->kslot_n, P.Mpad_max, 8)) || (rc = c->xerr.ensure(4)))
        return rc;
      HIP_TRY(hipMemsetAsync(c->xerr.p, 0, 4, c->st));
    }
    // (the gathers' sort waits for every wave of its launch: only while all chained waves in flight
    // fit the resident slots, half the budget)
    fsort = chain && want_sort && chain_waves_in_flight() <= c->chain_budget / 2;
    const int64_t n_timed = P.stride ? (P.T + P.stride - 1) / P.stride : 0;
    for (auto *v : {&c->evs, &c->evg, &c->evm})
      if ((int64_t)v->size() < 2 * n_timed) {
        size_t old = v->size();
        v->resize(2 * n_timed);
        for (size_t i = old; i < v->size(); i++) hipEventCreate(&(*v)[i]);
      }
    return IA_OK;
  }

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

  // the gather of step sn fused into a merge: outputs at query q0n of the step's buffers, the
  // handoff rows of local job jl
  NextStep next_step(const StepDesc &sn, int jl, size_t q0n) {
    NextStep nx{};
    nx.sn = sn;
    const QBufs q = qhalf(sn.t);
    nx.q64 = q.q64 + q0n * g.D;
    nx.qn2 = q.qn2 + q0n;
    nx.qinfo = q.qinfo ? q.qinfo + 3 * q0n : nullptr;
    nx.qf = (char *)c->qf.p + q0n * P.db_row_bytes;
    nx.mu = c->mu.as<double>();
    nx.basis = c->pr_basis.as<double>();
    nx.ufac = ufac;
    nx.hand = c->hand + (size_t)jl * g.bh;
    nx.seq = ++c->hseq;
    nx.err = c->xerr.as<unsigned>();
    nx.timeout_ticks = IA_WAIT_TICKS;
    nx.prefetch = c->prefetch_next;
    nx.early = c->early_gather;
    nx.gwave = gwave;
    return nx;
  }

  int step(int64_t t) {
    StepDesc sd;
    sd.t = (int)t;
    sd.J = P.J;
    ia_wavefront_step(g.bh, g.bw, t, &sd.r0, &sd.M);
    if (sd.M <= 0) return IA_OK;  // levels narrower than 3 columns have empty steps
    const int Mt = P.J * sd.M;    // queries of this step over all jobs
    sd.Mpad = (int)tile_pad(Mt);
    const bool timed_gm = P.stride && t % P.stride == 0;
    if (timed_gm) {
      hipEventRecord(c->evg[2 * n_gm], c->st);
      gather_bytes_timed += gq_bytes * Mt;
    }
    const QBufs q = qhalf(t);
    int rc;
    if (P.xo) {
      const OwnerStep os = owner_step(sd);
      owner_gather(sd, os, q);
      if (timed_gm) hipEventRecord(c->evg[2 * n_gm + 1], c->st);
      if ((rc = owner_scan(sd, os))) return rc;
      if (timed_gm) hipEventRecord(c->evm[2 * n_gm], c->st);
      if ((rc = owner_merge(sd, os, q))) return rc;
    } else {
      gather(sd, q);
      if (timed_gm) hipEventRecord(c->evg[2 * n_gm + 1], c->st);
      if ((rc = scan(sd, q))) return rc;
      if (timed_gm) hipEventRecord(c->evm[2 * n_gm], c->st);
      if ((rc = merge(sd))) return rc;
    }
    if (timed_gm) hipEventRecord(c->evm[2 * n_gm++ + 1], c->st);
    return IA_OK;
  }

  // ---- one-rank, all-gather and peer-write steps
  void gather(const StepDesc &sd, const QBufs &q) {
    if (chain) {
      mas[0].q64 = q.q64;
      mas[0].qn2 = q.qn2;
      mas[0].qinfo = q.qinfo;
    }
    if (chain && gathered == sd.t) return;  // this step's gather ran in the previous step's fused merge
    if (P.prune)
      ia_launch_gather_p(g, sd, in.Bim, in.jobs(), c->mu.as<double>(), q.q64, q.qn2, c->qf.p, c->db64.as<double>(),
                         c->pr_basis.as<double>(), ufac, q.qinfo, in.Aim, c->st);
    else if (P.use_h)
      ia_launch_gather_h(g, sd, in.Bim, in.jobs(), c->mu.as<double>(), q.q64, q.qn2, c->qf.p, c->st);
    else
      ia_launch_gather(g, sd, in.Bim, in.jobs(), c->mu.as<double>(), c->q64.as<double>(), c->qn2.as<double>(),
                       c->qf.as<float>(), c->st);
  }

  int scan(const StepDesc &sd, const QBufs &q) {
    const bool prune = P.prune;
    const int Mt = P.J * sd.M;
    // The pruned scan takes its queries presorted (one K2s launch per step) when the option names
    // a presorted form, when the step is wider than the in-kernel sort (512 queries), when it is
    // wider than one launch's query tiles and its blocks run as one launch (k3p_blocks: one K2s
    // launch instead of a second scan launch), or when the previous launch's gathers sorted it
    // (then without K2s, the tile boxes taken from the slice)
    const bool wide = sd.Mpad > 512 || (c->k3p_blocks && sd.Mpad > P.qtmax * IA_TILE);
    const bool gsorted = fsort && gathered == sd.t && gsort;
    const bool presorted = prune && (c->k3p_variant == 21 || c->k3p_variant == 25 || wide || gsorted);
    if (presorted && !gsorted)
      ia_launch_query_sort(q.qinfo, c->qf.p, sd.Mpad, g.KS, c->qs_order.as<int>(), c->qs_info.as<float4>(), c->qs_frag.p,
                           c->qs_tbox.as<float4>(), c->st);
    if (P.ns <= 0) return IA_OK;
    const int qtt = sd.Mpad / IA_TILE, nqb = (qtt + P.qtmax - 1) / P.qtmax;
    tally.begin_step(sd.t);
    for (size_t i = 0; i < P.shards.size(); i++) {
      const Shard &x = P.shards[i];
      MergeArgs &m = mas[i];
      const int n = x.t1 - x.t0;
      const char *dbp = shard_db(x);
      m.nwg = x.nwg;
      K3pLaunch k{};
      k.db = dbp;
      k.NT = n;
      k.qf = presorted ? c->qs_frag.p : c->qf.p;
      k.qinfo = presorted ? c->qs_info.as<float4>() : q.qinfo;
      k.order = presorted ? c->qs_order.as<int>() : nullptr;
      k.tbox = presorted && !gsorted ? c->qs_tbox.as<float4>() : nullptr;
      k.boxes = m.boxes;
      k.pos2row = m.pos2row;
      k.tnorm = prune ? c->tnorm.as<float>() + x.t0 : nullptr;
      k.M = Mt;
      k.Mpad = sd.Mpad;
      k.rec = (float4 *)m.rec;
      k.recT = (float *)m.recT;
      k.pairs = tally.pairs();
      k.tiles = tally.tiles();
      k.step = sd.t;
      k.r0 = sd.r0;
      k.rec_wt = c->rec_wt;
      if (presorted && nqb > 1 && c->k3p_blocks) {
        // one launch for all query blocks (option "k3p_blocks"): nqb blocks x nch DB chunks of
        // the shard, nch a multiple of 8 (the blocks of a chunk on one XCD) when that loses
        // little; records per query = nch, the merge's chunk count for this step
        int nch = std::max(1, std::min(n, IA_NWG_H / nqb));
        if (nch >= 64) nch &= ~7;
        if ((n + nch - 1) / nch <= IA_K3P_MAXK_LDS) {
          k.qt = (qtt + nqb - 1) / nqb;
          k.nwg = nch;
          k.nqb = nqb;
          k.qt_end = qtt;
          k.stamp = stamps.k3();
          if (ia_launch_k3p(k, c->k3p_variant, true, c->st)) return fail(IA_EINVAL, "pruned scan: no kernel instance for k3p_variant");
          m.nwg = nch;
          tally.add((double)n * qtt, (double)n * nqb, 0., true, scan_fixed_bytes((double)n * nqb, sd.Mpad, (double)Mt * nch * 20),
                    (double)n * P.tile_bytes);
          continue;
        }
      }
      int qt0 = 0;
      for (int b = 0; b < nqb; b++) {  // one launch per query block
        const int qt = qtt / nqb + (b < qtt % nqb ? 1 : 0);
        if (prune) {
          k.qt = qt;
          k.qt0 = qt0;
          k.nwg = x.nwg;
          k.stamp = stamps.k3();
          if (ia_launch_k3p(k, c->k3p_variant, presorted, c->st)) return fail(IA_EINVAL, "pruned scan: no kernel instance for k3p_variant");
        } else if (P.use_h) {
          ia_launch_k3h(g.KS, qt, dbp, c->qf.p, n, x.tpw, qt0, Mt, x.nwg, m.pos0, g.n_tiles, (float4 *)m.rec, (float *)m.recT, c->st);
        } else {
          ia_launch_k3(g.KH, qt, (const float4 *)dbp, c->qf.as<float4>(), n, x.tpw, qt0, Mt, x.nwg, m.pos0, g.n_tiles,
                       (float4 *)m.rec, (float *)m.recT, c->st);
        }
        const int mq = std::min(Mt, (qt0 + qt) * IA_TILE) - qt0 * IA_TILE;
        const double fl = prune ? 0. : 2.0 * g.D * (double)shard_rows[i] * std::max(mq, 0);  // pruned: pair counters
        tally.add((double)n * qt, (double)n, fl, prune, scan_fixed_bytes((double)n, sd.Mpad, (double)mq * x.nwg * 20),
                  (double)n * P.tile_bytes);
        qt0 += qt;
      }
    }
    tally.end_step();
    return IA_OK;
  }

  int merge(const StepDesc &sd) {
    const int64_t t = sd.t;
    const int Mt = P.J * sd.M;
    if (!P.multi && fuses_next(t)) {
      // this step's merge + the next step's gather, which reads the previous level
      int rc;
      if ((rc = link.wait_dep(t + 1))) return rc;
      StepDesc sn;
      sn.t = (int)(t + 1);
      sn.J = P.J;
      ia_wavefront_step(g.bh, g.bw, t + 1, &sn.r0, &sn.M);
      sn.Mpad = (int)tile_pad(P.J * sn.M);
      NextStep nx = next_step(sn, 0, 0);
      // the gathers also sort step t + 1 into k_query_sort's outputs when every wave of the launch
      // can be resident at once (each gather waits for all of the step's keys): k_merge_gather
      // holds one wave per SIMD (264 VGPRs), 1,024 on the chip; 768 leaves room for the kernels of
      // concurrent (pipelined) levels, which never wait on this one
      const int nw = P.J * sd.M + P.J + (sn.Mpad - P.J * sn.M);
      const bool srt = fsort && nw <= IA_FUSE_SORT_MAXW;
      if (srt) {
        nx.kslot = c->kslot;
        nx.sorder = c->qs_order.as<int>();
        nx.sinfo = c->qs_info.as<float4>();
        nx.sfrag = c->qs_frag.p;
      }
      mas[0].stamp = stamps.mg();
      ia_launch_merge_gather(g, sd, in.Aim, mas[0], in.jobs(), in.Bim, nx, P.prune, c->st);
      gathered = t + 1;
      gsort = srt;
    } else if (!P.multi) {
      mas[0].stamp = stamps.mg();
      ia_launch_merge(g, sd, in.Aim, mas[0], c->win.as<Winner>(), in.jobs(), true, c->st);
    } else if (P.xchg) {
      // one-shot peer-write exchange fused into the merge: each shard's winner goes into every
      // rank's buffer; the last launch of this process waits for all W and finishes the pixels
      XchgArgs xa;
      for (int p = 0; p < IA_XCHG_MAXW; p++) xa.peer[p] = P.sharded ? c->xpeer[p] : (XSlot *)c->xbuf;
      xa.local = P.sharded ? c->xpeer[c->rank] : (XSlot *)c->xbuf;
      xa.W = P.Wsh;
      xa.seq = ++c->xseq;
      xa.err = c->xerr.as<unsigned>();
      xa.timeout_ticks = IA_WAIT_TICKS;
      for (size_t i = 0; i < P.shards.size(); i++) {
        xa.rank = P.sharded ? c->rank : (int)i;
        ia_launch_merge_xchg(g, sd, in.Aim, mas[i], xa, in.jobs(), i + 1 == P.shards.size(), c->st);
      }
    } else {
      // certified per-shard winners, then the global winner (smallest exact distance, lowest row)
      // and coherence / kappa / writeback, identical on every rank
      for (size_t i = 0; i < P.shards.size(); i++)
        ia_launch_merge(g, sd, in.Aim, mas[i], (P.sharded ? c->win.as<Winner>() : c->allwin.as<Winner>() + i * Mt), in.jobs(),
                        false, c->st);
      if (P.sharded)
        NCCL_TRY(ncclAllGather(c->win.p, c->allwin.p, (size_t)Mt * sizeof(Winner), ncclUint8, c->comm, c->st));
      ia_launch_finish(g, sd, in.Aim, c->db64.as<double>(), c->q64.as<double>(), c->allwin.as<Winner>(), P.Wsh, Mt, in.jobs(),
                       c->st);
    }
    return IA_OK;
  }

  // ---- owner-computes steps
  int owner_of(int jl) const { return P.sharded ? c->rank : jl; }
  char *xo_area(int p, unsigned seq) const {  // parity base of rank p's area for the step of sequence seq
    return (char *)(P.sharded ? (void *)c->xpeer[p] : c->xbuf) + ia_xslots_bytes(P.Wsh) + (size_t)(seq & 1u) * XOLayout::PARITY;
  }
  OwnerStep owner_step(const StepDesc &sd) {
    OwnerStep os;
    os.seq = ++c->xseq;
    os.loc = xo_area(P.sharded ? c->rank : 0, os.seq);
    os.Mpj = (int)tile_pad(sd.M);
    os.ink = os.Mpj <= ia_k3h_qtmax(g.KS) * IA_TILE && !c->xo_presort;
    os.QTs = os.ink ? os.Mpj / IA_TILE : P.xo_QTs;
    os.Mrec = P.Wsh * os.QTs * IA_TILE;
    os.s1 = sd;
    os.s1.J = 1;
    os.s1.Mpad = os.Mpj;
    os.nqb = os.ink ? P.Wsh : P.Wsh * P.xo_bpj;
    // one chunk count for every shard (the owners' merges index records as shard * nch + chunk
    // and map a chunk back to its tiles with it): from the smallest shard, which every rank
    // computes alike (shards differ by at most one tile, ia_shard_off)
    os.nch = std::max(1, std::min((int)(g.n_tiles / P.Wsh), IA_NWG_H / os.nqb));
    if (os.nch >= 64) os.nch &= ~7;
    return os;
  }
  // owner jl's K2s: its queries sorted into every rank's area
  void owner_sort(const StepDesc &sd, const OwnerStep &os, const QBufs &q, int jl) {
    const size_t q0 = (size_t)jl * os.Mpj;
    XOSort xs{};
    xs.inv = c->xo_inv.as<int>();
    xs.W = P.sharded ? P.Wsh : 1;
    for (int p = 0; p < xs.W; p++) xs.area[p] = xo_area(p, os.seq);
    xs.q0 = 0;
    xs.Mj = sd.M;
    xs.tile0 = owner_of(jl) * os.QTs;
    xs.QTs = os.QTs;
    xs.seq = os.seq;
    ia_launch_query_sort_xo(q.qinfo + 3 * q0, (char *)c->qf.p + q0 * P.db_row_bytes, xs, c->st);
  }
  void owner_gather(const StepDesc &sd, const OwnerStep &os, const QBufs &q) {
    for (int jl = 0; jl < P.J; jl++) {
      const size_t q0 = (size_t)jl * os.Mpj;
      if (chain && gathered == sd.t) {  // K2p (+ publish) ran in the previous step's fused merge
        if (!os.ink) owner_sort(sd, os, q, jl);
        continue;
      }
      XOPub xp{};
      if (os.ink) {
        xp.W = P.sharded ? P.Wsh : 1;
        for (int p = 0; p < xp.W; p++) xp.area[p] = xo_area(p, os.seq);
        xp.slot0 = owner_of(jl) * os.Mpj;
        xp.seq = os.seq;
      }
      ia_launch_gather_p(g, os.s1, in.Bim, in.job(jl), c->mu.as<double>(), q.q64 + q0 * g.D, q.qn2 + q0,
                         (char *)c->qf.p + q0 * P.db_row_bytes, c->db64.as<double>(), c->pr_basis.as<double>(), ufac,
                         q.qinfo + 3 * q0, in.Aim, c->st, &xp);
      if (!os.ink) owner_sort(sd, os, q, jl);
    }
  }
  int owner_scan(const StepDesc &sd, const OwnerStep &os) {
    const int Wsh = P.Wsh;
    tally.begin_step(sd.t);
    for (size_t i = 0; i < P.shards.size(); i++) {
      const Shard &x = P.shards[i];
      const int n = x.t1 - x.t0;
      if ((n + os.nch - 1) / os.nch > IA_K3P_MAXK_LDS || (int64_t)Wsh * os.nch * os.Mrec > IA_XO_MAXREC)
        return fail(IA_EINVAL, "ia_synthesize_level: exchange = 2: shard too large for the pruned scan's chunks");
      XOScan xs{};
      for (int p = 0; p < Wsh; p++) xs.area[p] = P.sharded ? xo_area(p, os.seq) : os.loc;
      xs.flag = reinterpret_cast<const unsigned *>(os.loc + (os.ink ? XOLayout::QSEQ : XOLayout::FLAG));
      xs.inv = c->xo_inv.as<int>();
      xs.on = 1;
      xs.s = P.sharded ? c->rank : (int)i;
      xs.bpj = os.ink ? 1 : P.xo_bpj;
      xs.Mrec = os.Mrec;
      xs.seq = os.seq;
      xs.err = c->xerr.as<unsigned>();
      xs.timeout_ticks = IA_WAIT_TICKS;
      K3pLaunch k{};  // the queries come from this process's area, the records go to the owners'
      k.db = shard_db(x);
      k.NT = n;
      k.qf = os.loc + XOLayout::FRAG;
      k.qinfo = reinterpret_cast<const float4 *>(os.loc + XOLayout::INFO);
      k.order = reinterpret_cast<const int *>(os.loc + XOLayout::ORD);
      k.tbox = reinterpret_cast<const float4 *>(os.loc + XOLayout::TBOX);
      k.boxes = mas[i].boxes;
      k.pos2row = mas[i].pos2row;
      k.tnorm = c->tnorm.as<float>() + x.t0;
      k.qt = os.ink ? os.QTs : P.xo_QTx;
      k.M = sd.M;
      k.Mpad = os.ink ? os.Mpj : os.Mrec;
      k.nwg = os.nch;
      k.nqb = os.nqb;
      k.qt_end = Wsh * os.QTs;
      k.pairs = tally.pairs();
      k.tiles = tally.tiles();
      k.step = sd.t;
      k.r0 = sd.r0;
      k.xo = &xs;
      k.stamp = stamps.k3();
      k.rec_wt = c->rec_wt;
      if (ia_launch_k3p(k, c->k3p_variant, !os.ink, c->st)) return fail(IA_EINVAL, "pruned scan: no kernel instance for k3p_variant");
      tally.add((double)n * Wsh * os.QTs, (double)n * os.nqb, 0., true,
                scan_fixed_bytes((double)n * os.nqb, os.Mrec, (double)os.Mrec * os.nch * 24), (double)n * P.tile_bytes);
    }
    tally.end_step();
    return IA_OK;
  }
  int owner_merge(const StepDesc &sd, const OwnerStep &os, const QBufs &q) {
    const int64_t t = sd.t;
    const int Wsh = P.Wsh;
    // the next step's layout (fused merge + gather: each owner publishes its next queries)
    const bool fuse_next = fuses_next(t);
    StepDesc sn{};
    int Mpj_n = 0;
    bool ink_n = false;
    if (fuse_next) {
      int rc;
      if ((rc = link.wait_dep(t + 1))) return rc;
      sn.t = (int)(t + 1);
      sn.J = 1;
      ia_wavefront_step(g.bh, g.bw, t + 1, &sn.r0, &sn.M);
      Mpj_n = (int)tile_pad(sn.M);
      sn.Mpad = Mpj_n;
      ink_n = Mpj_n <= ia_k3h_qtmax(g.KS) * IA_TILE && !c->xo_presort;
    }
    for (int jl = 0; jl < P.J; jl++) {
      const size_t q0 = (size_t)jl * os.Mpj;
      MergeArgs mx = ma;
      mx.q64 = q.q64 + q0 * g.D;
      mx.qn2 = q.qn2 + q0;
      mx.qinfo = q.qinfo + 3 * q0;
      mx.rec = reinterpret_cast<const float4 *>(os.loc + XOLayout::REC);
      mx.xo_rts = reinterpret_cast<const unsigned long long *>(os.loc + XOLayout::RTS);
      mx.nwg = Wsh * os.nch;
      mx.rr = 1;
      mx.NT = g.n_tiles;
      mx.boxes = c->boxes.as<float4>();
      mx.pos2row = g.pos2row;
      mx.xo_inv = c->xo_inv.as<int>();
      mx.xo_W = Wsh;
      mx.xo_nch = os.nch;
      mx.xo_Mrec = os.Mrec;
      mx.xo_o0 = owner_of(jl);
      mx.xo_M = sd.M;
      mx.xo_QTs = os.QTs;
      mx.xo_seq = os.seq;
      mx.xo_err = c->xerr.as<unsigned>();
      mx.xo_timeout = IA_WAIT_TICKS;
      mx.stamp = stamps.mg();
      if (!fuse_next) {
        ia_launch_merge(g, os.s1, in.Aim, mx, c->win.as<Winner>(), in.job(jl), true, c->st);
        continue;
      }
      NextStep nx = next_step(sn, jl, (size_t)jl * Mpj_n);
      if (ink_n) {  // the next step's queries go straight to every rank's area (else its K2s sorts them)
        nx.xp.W = P.sharded ? Wsh : 1;
        for (int p = 0; p < nx.xp.W; p++) nx.xp.area[p] = xo_area(p, os.seq + 1);
        nx.xp.slot0 = owner_of(jl) * Mpj_n;
        nx.xp.seq = os.seq + 1;
        if (P.sharded && c->xo_wait && jl == P.J - 1) {  // ranks: wait here for every owner's next queries
          nx.wait_seq = reinterpret_cast<const unsigned *>(xo_area(c->rank, os.seq + 1) + XOLayout::QSEQ);
          nx.wait_n = Wsh * Mpj_n;
        }
      }
      ia_launch_merge_gather(g, os.s1, in.Aim, mx, in.job(jl), in.Bim, nx, true, c->st);
    }
    if (fuse_next) gathered = t + 1;
    return IA_OK;
  }
};

// ---- phase 5: results -----------------------------------------------------------------------
// the stats words' reduction, the D2H copies of host-memory jobs, the level's one sync, and the
// error words of the handoffs and exchanges
static int finish_level(ia_ctx *c, const ia_level_args *args, const LevelPlan &P, const LevelInputs &in, bool chain,
                        bool want_stats) {
  const int64_t NB = P.NB;
  if (want_stats)
    for (int j = 0; j < P.J; j++) ia_launch_reduce_stats(in.jp[j].pstat, NB, c->counters.as<unsigned long long>(), c->st);
  for (int j = 0; j < P.J; j++) {
    const ia_level_args *x = &args[j];
    const JobPtrs &p = in.jp[j];
    if (x->mem != IA_MEM_HOST) continue;
    HIP_TRY(hipMemcpyAsync(x->Bp, p.Bp, P.nB * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(x->s_out, p.s, (size_t)NB * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(x->im_out, p.im, (size_t)NB * 4, hipMemcpyDeviceToHost, c->st));
    if (x->dbg_src) {
      HIP_TRY(hipMemcpyAsync(x->dbg_src, p.dbg_src, (size_t)NB * 24, hipMemcpyDeviceToHost, c->st));
      HIP_TRY(hipMemcpyAsync(x->dbg_dist, p.dbg_dist, (size_t)NB * 16, hipMemcpyDeviceToHost, c->st));
    }
  }
  HIP_TRY(hipStreamSynchronize(c->st));
#if IA_PROBE & 16
  if (P.prune) ia_k3p_probe_dump();
#endif
  if (chain) {
    unsigned xe = 0;
    HIP_TRY(hipMemcpy(&xe, c->xerr.p, 4, hipMemcpyDeviceToHost));
    if (xe & 16) return fail(IA_EHIP, "ia_synthesize_level: a fused gather's handoff did not arrive within 20 s");
  }
  if (P.xchg || P.xo) {
    unsigned xe = 0;
    HIP_TRY(hipMemcpy(&xe, c->xerr.p, 4, hipMemcpyDeviceToHost));
    if (xe)
      return fail(IA_ECOMM, std::string("ia_synthesize_level: a peer's ") +
                                (xe & 4 ? "sorted queries" : xe & 8 ? "scan records" : "shard winner") +
                                " did not arrive within 20 s (peer-write exchange)");
  }
  return IA_OK;
}

// ---- k-coherence levels (ia_synthesize_levels_kcoh) - ---------------------------
// what the sets, the context and the batch must be for one (the jobs' own checks are check_level_args')
static int check_kcoh(ia_ctx *c, const ia_level_args *args, int J, const int32_t *sim, int sim_k) {
  const ia_level_args *a = &args[0];
  if (sim_k < 0 || sim_k > IA_KCOH_MAX || (int64_t)sim_k > (int64_t)a->n_ap * a->a_h * a->a_w - 1)
    return fail(IA_EINVAL, "ia_synthesize_levels_kcoh: sim_k must be 0 (the exact path) or 1..min(IA_KCOH_MAX, N_A - 1)");
  if (!sim_k) return IA_OK;
  if (!sim) return fail(IA_EINVAL, "ia_synthesize_levels_kcoh: sim_k > 0 needs sim");
  const bool dep = c->dep != nullptr;
  c->dep = nullptr;  // one level call per ia_pipeline_depend, refused or not
  c->dep_gen = 0;
  if (c->world > 1 || c->shard_emulate > 1)
    return fail(IA_EINVAL, "ia_synthesize_level: k-coherence levels (sim_k > 0) do not run on a sharded or shard-emulating context");
  if (c->p_record || dep) return fail(IA_EINVAL, "ia_synthesize_level: k-coherence levels (sim_k > 0) are not pipelined");
  for (int j = 0; j < J; j++)
    if (args[j].dbg_src) return fail(IA_EINVAL, "ia_synthesize_level: k-coherence levels (sim_k > 0) produce no debug records");
  return IA_OK;
}

// The level after its staging: the similarity sets checked on the device (one pre-pass, one
// read-back), the fp64 row DB (K1b) alone, then one launch per wavefront step over all jobs, on
// the exact path's t = col + 3 row schedule.  No tiles, no scan, no records, no merge.  (If a call
// fails between two steps, the scan waves' counts may be left non-zero: they are cleared here.)
static int run_kcoh_level(ia_ctx *c, const ia_level_args *args, LevelPlan &P, LevelInputs &in, const int32_t *sim_in, int K,
                          ia_stats *stats) {
  const ia_level_args *a = &args[0];
  const LevelGeo &g = P.g;
  int rc;
  ia_wavefront_shape(g.bh, g.bw, &P.T, &P.Mmax);
  P.Mtmax = P.Mmax * P.J;
  const size_t sim_bytes = (size_t)g.NA * K * 4;
  const int32_t *sim = sim_in;
  if (a->mem == IA_MEM_HOST) {
    if ((rc = c->sim.ensure(sim_bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(c->sim.p, sim_in, sim_bytes, hipMemcpyHostToDevice, c->st));
    sim = c->sim.as<int32_t>();
  }
  if ((rc = stage_jobs(c, P, in)) || (rc = c->db64.ensure((size_t)g.NA * ia_db64_stride(g.ch) * 8)) ||
      (rc = c->counters.ensure(5 * 8)) || (rc = c->xerr.ensure(4)))
    return rc;
  const int H = ia_kcoh_scan_waves(g.NA);
  if ((rc = c->kc_part.ensure((size_t)P.Mtmax * H * sizeof(Winner))) || (rc = c->kc_cnt.ensure((size_t)P.Mtmax * 4))) return rc;
  HIP_TRY(hipMemsetAsync(c->kc_cnt.p, 0, (size_t)P.Mtmax * 4, c->st));
  unsigned bad = 0;
  HIP_TRY(hipMemsetAsync(c->xerr.p, 0, 4, c->st));
  ia_launch_kcoh_check(sim, (int64_t)g.NA * K, (int)g.NA, c->xerr.as<unsigned>(), c->st);
  HIP_TRY(hipMemcpyAsync(&bad, c->xerr.p, 4, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  if (bad) return fail(IA_EINVAL, "ia_synthesize_level: a sim entry lies outside the level's DB rows [0, n_ap a_h a_w)");
  HIP_TRY(hipMemsetAsync(c->counters.p, 0, 5 * 8, c->st));
  HIP_TRY(hipEventRecord(c->lv0, c->st));
  ia_launch_db64_build(g, in.Aim, in.Apairs, c->db64.as<double>(), c->st);
  HIP_TRY(hipEventRecord(c->lv1, c->st));
  for (int64_t t = 0; t < P.T; t++) {
    StepDesc sd;
    sd.t = (int)t;
    sd.J = P.J;
    ia_wavefront_step(g.bh, g.bw, t, &sd.r0, &sd.M);
    if (sd.M <= 0) continue;  // levels narrower than 3 columns have empty steps
    sd.Mpad = (int)tile_pad(P.J * sd.M);
    ia_launch_kcoh_step(g, sd, in.Aim, in.Bim, in.jobs(), c->db64.as<double>(), sim, K, H, c->kc_part.p, c->kc_cnt.as<unsigned>(),
                        c->st);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->lv2, c->st));
  if ((rc = finish_level(c, args, P, in, false, stats != nullptr))) return rc;
  return stats ? accumulate_kcoh_stats(c, P, stats) : IA_OK;
}

}  // namespace
}  // namespace ia_host

using namespace ia_host;

extern "C" {

int ia_wavefront_shape(int h, int w, int64_t *steps, int64_t *max_queries) {
  if (h < 1 || w < 1) return fail(IA_EINVAL, "ia_wavefront_shape: empty level");
  if (steps) *steps = (int64_t)w + 3 * (int64_t)(h - 1);
  if (max_queries) *max_queries = std::min<int64_t>(h, (w + 2) / 3);
  return IA_OK;
}

int ia_wavefront_step(int h, int w, int64_t t, int *r0, int *M) {
  if (h < 1 || w < 1 || t < 0 || t >= (int64_t)w + 3 * (int64_t)(h - 1)) return fail(IA_EINVAL, "ia_wavefront_step: bad step");
  const int64_t r_lo = std::max<int64_t>(0, (t - w + 1 + 2) / 3);  // ceil((t - w + 1) / 3), t - w + 3 > 0
  const int64_t r_hi = std::min<int64_t>(h - 1, t / 3);
  *r0 = (int)r_lo;
  *M = (int)(r_hi - r_lo + 1);
  return IA_OK;
}

// ------------------------------------------------------------------------------------------
// fast path: one pyramid level (image_analogies.py:130-239)
// ------------------------------------------------------------------------------------------
int ia_synthesize_level(ia_ctx *c, const ia_level_args *a, ia_stats *stats) { return ia_synthesize_levels_kcoh(c, a, 1, nullptr, 0, stats); }

int ia_synthesize_levels(ia_ctx *c, const ia_level_args *args, int n_jobs, ia_stats *stats) {
  return ia_synthesize_levels_kcoh(c, args, n_jobs, nullptr, 0, stats);
}

// the level call: the exact path (sim_k = 0) or k-coherence search on the similarity sets sim
int ia_synthesize_levels_kcoh(ia_ctx *c, const ia_level_args *args, int n_jobs, const int32_t *sim, int sim_k, ia_stats *stats) {
  if (!c || !args) return fail(IA_EINVAL, "ia_synthesize_level: NULL argument");
  if (n_jobs < 1 || n_jobs > IA_MAX_JOBS)
    return fail(IA_EINVAL, "ia_synthesize_levels: n_jobs must be 1.." + std::to_string(IA_MAX_JOBS));
  const ia_level_args *a = &args[0];
  int rc;
  for (int j = 0; j < n_jobs; j++) {
    const ia_level_args *x = &args[j];
    if ((rc = check_level_args(x))) return rc;
    if (x->ch != a->ch || x->n_ap != a->n_ap || x->n_a != a->n_a || x->a_h != a->a_h || x->a_w != a->a_w || x->b_h != a->b_h ||
        x->b_w != a->b_w || x->mem != a->mem)
      return fail(IA_EINVAL, "ia_synthesize_levels: every job of a batch has the same shapes, channels, n_a and mem kind");
    if (x->A != a->A || x->Ac != a->Ac || x->Ap != a->Ap || x->Apc != a->Apc)
      return fail(IA_EINVAL, "ia_synthesize_levels: every job of a batch shares the A side (same A / A' buffers)");
  }
  if ((rc = check_kcoh(c, args, n_jobs, sim, sim_k))) return rc;
  HIP_TRY(hipSetDevice(c->dev));

  // plan and stage (the plan's second half needs the matcher: one device read-back)
  LevelPlan P;
  LevelInputs in;
  bool use_h = false;
  if (sim_k) {  // a k-coherence level: no matcher, no scan plan, no tiles
    if ((rc = plan_shards(c, args, n_jobs, P)) || (rc = stage_level(c, args, P, in))) return rc;
    return run_kcoh_level(c, args, P, in, sim, sim_k, stats);
  }
  if ((rc = plan_shards(c, args, n_jobs, P)) || (rc = stage_level(c, args, P, in)) || (rc = probe_matcher(c, P, in, &use_h)) ||
      (rc = plan_scan(c, use_h, P)) || (rc = stage_jobs(c, P, in)) || (rc = ensure_scratch(c, P)))
    return rc;
  // the guards fire on every return from here on and outlive the step loop: the dependents'
  // waits released (PipelineLink), the chain reservation returned, the used stamp slots cleared
  StampSlots stamps;
  if ((rc = stamps.open(c, P))) return rc;
  HIP_TRY(hipMemsetAsync(c->pairs.p, 0, 6 * IA_NWG_H * 8, c->st));  // the scans' per-workgroup counters (ScanTally)
  HIP_TRY(hipMemsetAsync(c->Rbits.p, 0, 4, c->st));
  HIP_TRY(hipMemsetAsync(c->counters.p, 0, 5 * 8, c->st));
  double ufac = 0.;
  if ((rc = build_level_db(c, P, in, &ufac))) return rc;

  ChainReservation chain_res;
  PipelineLink link;
  LevelRun run(c, P, in, stamps, link, chain_res, ufac);
  run.init_merge_args();
  if ((rc = run.init_chain()) || (rc = link.open(c, P.T))) return rc;
  for (int64_t t = 0; t < P.T; link.mark_step(t), t++)
    if ((rc = link.wait_dep(t)) || (rc = run.step(t))) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->lv2, c->st));
  stamps.durations();  // (the slots this level wrote are cleared when the call returns)

  if ((rc = finish_level(c, args, P, in, run.chain, stats != nullptr))) return rc;
  return stats ? accumulate_stats(c, P, stamps, run.tally, run.n_gm, run.gather_bytes_timed, stats) : IA_OK;
}

}  // extern "C"

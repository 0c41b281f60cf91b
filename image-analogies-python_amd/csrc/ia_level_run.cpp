// ia_level_run.cpp — phases 4 and 5 of a level call and the call itself: the skewed wavefront's
// step and its one-rank, all-gather and peer-write forms (LevelRun, ia_level_run.h; the
// owner-computes form is ia_level_owner.cpp's), the results' copies and error word, and the entry
// points ia_synthesize_level(s) with the wavefront's pure shape helpers.
#include <rccl/rccl.h>  // the all-gather of a sharded step's winners (LevelRun::merge_all_gather)

#include "ia_level_run.h"

#if IA_PROBE & 16
void ia_k3p_probe_dump();
#endif

namespace ia_host {

#define IA_FUSE_SORT_MAXW 768  // waves of a k_merge_gather launch whose gathers sort the next step
#define IA_FUSE_SORT_MINQ 512  // fuse_sort 2: the widest step's queries (all jobs) from which the gathers sort

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

// ---- phase 4: the steps of one level --------------------------------------------------------
void LevelRun::init_merge_args() {
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
  if (P.xo) init_owner_merge_args();
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
int LevelRun::init_chain() {
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

// the gather of step sn fused into a merge: outputs at query q0n of the step's buffers, the
// handoff rows of local job jl
NextStep LevelRun::next_step(const StepDesc &sn, int jl, size_t q0n) {
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

int LevelRun::step(int64_t t) {
  const StepDesc sd = step_desc(g, t, P.J);
  if (sd.M <= 0) return IA_OK;  // levels narrower than 3 columns have empty steps
  const int Mt = P.J * sd.M;    // queries of this step over all jobs
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
void LevelRun::gather(const StepDesc &sd, const QBufs &q) {
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

int LevelRun::scan(const StepDesc &sd, const QBufs &q) {
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
  int rc;
  tally.begin_step(sd.t);
  for (size_t i = 0; i < P.shards.size(); i++) {
    const Shard &x = P.shards[i];
    MergeArgs &m = mas[i];
    const int n = x.t1 - x.t0;
    m.nwg = x.nwg;
    K3pLaunch k = scan_base(i, sd);
    k.qf = presorted ? c->qs_frag.p : c->qf.p;
    k.qinfo = presorted ? c->qs_info.as<float4>() : q.qinfo;
    k.order = presorted ? c->qs_order.as<int>() : nullptr;
    k.tbox = presorted && !gsorted ? c->qs_tbox.as<float4>() : nullptr;
    k.M = Mt;
    k.Mpad = sd.Mpad;
    k.rec = (float4 *)m.rec;
    k.recT = (float *)m.recT;
    // one launch for all query blocks (option "k3p_blocks"): nqb blocks x nch DB chunks of the
    // shard; records per query = nch, the merge's chunk count for this step
    const int nch = scan_chunks(n, nqb);
    if (presorted && nqb > 1 && c->k3p_blocks && (n + nch - 1) / nch <= IA_K3P_MAXK_LDS) {
      k.qt = (qtt + nqb - 1) / nqb;
      k.nwg = nch;
      k.nqb = nqb;
      k.qt_end = qtt;
      if ((rc = launch_scan(k, true))) return rc;
      m.nwg = nch;
      tally.add((double)n * qtt, (double)n * nqb, 0., true, scan_fixed_bytes((double)n * nqb, sd.Mpad, (double)Mt * nch * 20),
                (double)n * P.tile_bytes);
      continue;
    }
    int qt0 = 0;
    for (int b = 0; b < nqb; b++) {  // one launch per query block
      const int qt = qtt / nqb + (b < qtt % nqb ? 1 : 0);
      if (prune) {
        k.qt = qt;
        k.qt0 = qt0;
        k.nwg = x.nwg;
        if ((rc = launch_scan(k, presorted))) return rc;
      } else if (P.use_h) {
        ia_launch_k3h(g.KS, qt, k.db, c->qf.p, n, x.tpw, qt0, Mt, x.nwg, m.pos0, g.n_tiles, (float4 *)m.rec, (float *)m.recT, c->st);
      } else {
        ia_launch_k3(g.KH, qt, (const float4 *)k.db, c->qf.as<float4>(), n, x.tpw, qt0, Mt, x.nwg, m.pos0, g.n_tiles,
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

int LevelRun::merge(const StepDesc &sd) {
  if (!P.multi && fuses_next(sd.t)) return merge_fused_next(sd);
  if (!P.multi) merge_fused(sd);
  else if (P.xchg) merge_peer_write(sd);
  else return merge_all_gather(sd);
  return IA_OK;
}

// this step's merge + the next step's gather, which reads the previous level
int LevelRun::merge_fused_next(const StepDesc &sd) {
  const int64_t t = sd.t;
  int rc;
  if ((rc = link.wait_dep(t + 1))) return rc;
  const StepDesc sn = step_desc(g, t + 1, P.J);
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
  return IA_OK;
}

void LevelRun::merge_fused(const StepDesc &sd) {
  mas[0].stamp = stamps.mg();
  ia_launch_merge(g, sd, in.Aim, mas[0], c->win.as<Winner>(), in.jobs(), true, c->st);
}

// one-shot peer-write exchange fused into the merge: each shard's winner goes into every
// rank's buffer; the last launch of this process waits for all W and finishes the pixels
void LevelRun::merge_peer_write(const StepDesc &sd) {
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
}

// certified per-shard winners, then the global winner (smallest exact distance, lowest row)
// and coherence / kappa / writeback, identical on every rank
int LevelRun::merge_all_gather(const StepDesc &sd) {
  const int Mt = P.J * sd.M;
  for (size_t i = 0; i < P.shards.size(); i++)
    ia_launch_merge(g, sd, in.Aim, mas[i], (P.sharded ? c->win.as<Winner>() : c->allwin.as<Winner>() + i * Mt), in.jobs(),
                    false, c->st);
  if (P.sharded) NCCL_TRY(ncclAllGather(c->win.p, c->allwin.p, (size_t)Mt * sizeof(Winner), ncclUint8, c->comm, c->st));
  ia_launch_finish(g, sd, in.Aim, c->db64.as<double>(), c->q64.as<double>(), c->allwin.as<Winner>(), P.Wsh, Mt, in.jobs(), c->st);
  return IA_OK;
}

// ---- phase 5: results -----------------------------------------------------------------------
int finish_level(ia_ctx *c, const ia_level_args *args, const LevelPlan &P, const LevelInputs &in, bool chain, bool want_stats) {
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
  if (!chain && !P.xchg && !P.xo) return IA_OK;
  unsigned xe = 0;  // the device error word: a handoff first, then any bit of an exchange
  HIP_TRY(hipMemcpy(&xe, c->xerr.p, 4, hipMemcpyDeviceToHost));
  if (chain && (xe & 16)) return fail(IA_EHIP, "ia_synthesize_level: a fused gather's handoff did not arrive within 20 s");
  if ((P.xchg || P.xo) && xe)
    return fail(IA_ECOMM, std::string("ia_synthesize_level: a peer's ") +
                              (xe & 4 ? "sorted queries" : xe & 8 ? "scan records" : "shard winner") +
                              " did not arrive within 20 s (peer-write exchange)");
  return IA_OK;
}

}  // namespace ia_host

using namespace ia_host;

extern "C" {

// the default windows' wavefront: the window call's (ia_level_nbhd.cpp) at pad 2, i.e. skew 3
int ia_wavefront_shape(int h, int w, int64_t *steps, int64_t *max_queries) {
  if (h < 1 || w < 1) return fail(IA_EINVAL, "ia_wavefront_shape: empty level");
  return ia_wavefront_shape_pad(h, w, 2, steps, max_queries);
}

int ia_wavefront_step(int h, int w, int64_t t, int *r0, int *M) {
  if (h < 1 || w < 1 || t < 0 || t >= (int64_t)w + 3 * (int64_t)(h - 1)) return fail(IA_EINVAL, "ia_wavefront_step: bad step");
  return ia_wavefront_step_pad(h, w, 2, t, r0, M);
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
  int rc;
  if ((rc = check_level_batch(args, n_jobs))) return rc;
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

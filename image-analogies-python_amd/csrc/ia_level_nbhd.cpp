// ia_level_nbhd.cpp — exact levels for window sizes other than 3x3 / 5x5 (ia_synthesize_levels_nbhd,
// DESIGN.md §11): the call, its checks, its step loop and the wavefront's shape for any skew, and what
// the masked call (ia_level_mask.cpp) runs too: the prologue, the DB, the step buffers and the step
// itself (run_nbhd_step: the window kernels of ia_nbhd.hip around the index's query prep, fp32 scan
// and certified merge, ia_dense.hip, ia_k3.hip).  Here is also the side paths' one refusal rule.
// These calls share the plan's first half, the staging and finish_level with the default path
// (ia_level_run.cpp) and none of its steps.
#include <cmath>
#include <cstring>

#include "ia_level.h"

namespace ia_host {

// The side paths' refusal rule (this file's two window calls and the k-coherence level,
// ia_level_kcoh.cpp): their levels run alone on one device, outside the level pipeline, without debug
// records.  It consumes the pending ia_pipeline_depend, whether it then refuses the call or not.
// who: the entry point the message names; what: its levels, the sentence's subject.
int refuse_side_path(ia_ctx *c, const ia_level_args *args, int J, const std::string &who, const std::string &what) {
  const bool dep = c->dep != nullptr;
  c->dep = nullptr;  // one level call per ia_pipeline_depend, refused or not
  c->dep_gen = 0;
  const std::string subject = who + ": " + what;
  if (c->world > 1 || c->shard_emulate > 1) return fail(IA_EINVAL, subject + " do not run on a sharded or shard-emulating context");
  if (c->p_record || dep) return fail(IA_EINVAL, subject + " are not pipelined");
  for (int j = 0; j < J; j++)
    if (args[j].dbg_src) return fail(IA_EINVAL, subject + " produce no debug records");
  return IA_OK;
}

int check_nbhd(ia_ctx *c, const ia_level_args *args, int J, int n_sm, int n_lg, const std::string &who) {
  // first, so that a call refused for its sizes consumes the dependency too; the sizes' message wins
  const int rc = refuse_side_path(c, args, J, who, "levels of this call");
  const int ch = args[0].ch;
  const NbhdGeo w = ia_nbhd_geo(ch, n_sm, n_lg);
  const bool sizes = (n_sm == 1 || n_sm == 3 || n_sm == 5) && (n_lg == 3 || n_lg == 5 || n_lg == 7 || n_lg == 9);
  if (!sizes || w.D > IA_MAX_D - 1)
    return fail(IA_EINVAL, who + ": n_sm = " + std::to_string(n_sm) + ", n_lg = " + std::to_string(n_lg) +
                               " at " + std::to_string(ch) + " channel(s)" +
                               (sizes ? " gives D = " + std::to_string(w.D) + " features" : std::string()) +
                               ": n_sm must be 1, 3 or 5, n_lg 3, 5, 7 or 9, and D = ch (2 n_sm^2 + n_lg^2 + n_lg^2 / 2) <= " +
                               std::to_string(IA_MAX_D - 1));
  return rc;
}

// what both window calls do between their checks and their level: the default plan's first half with
// this call's weight length and row width in place of the 3 / 5 ones, then the staging
int plan_nbhd_level(ia_ctx *c, const ia_level_args *args, int J, const NbhdGeo &w, LevelPlan &P, LevelInputs &in) {
  int rc;
  if ((rc = plan_shards(c, args, J, P))) return rc;
  P.g.D = w.D;
  P.g.KH = kh_for(w.D + 1);
  P.DP = 2 * P.g.KH;
  return stage_level(c, args, P, in);
}

// The window calls' DB (this call's and the masked one's, ia_level_mask.cpp), bracketed by lv0 / lv1:
// the fp64 rows with their column statistics (one read-back: it also finds a non-finite A side before
// any step runs; who: the entry point the refusal names), then the index's centred, prescaled fp32
// tiles.  Completes scan (after ensure_nbhd_steps): the tiles' prescale and the merges' arguments.
int build_nbhd_db(ia_ctx *c, const LevelPlan &P, const LevelInputs &in, const NbhdGeo &w, const std::string &who, NbhdScan *scan) {
  const LevelGeo &g = P.g;
  const int D = w.D, KH = g.KH;
  int rc;
  if ((rc = c->db64.ensure((size_t)g.NA * D * 8)) || (rc = c->mu.ensure((size_t)D * 8)) || (rc = c->absmax.ensure(4)) ||
      (rc = c->Rbits.ensure(4)) || (rc = c->db.ensure((size_t)g.n_tiles * IA_TILE * 2 * KH * 4)))
    return rc;
  double *rows = c->db64.as<double>(), *mu = c->mu.as<double>();
  HIP_TRY(hipMemsetAsync(c->absmax.p, 0, 4, c->st));
  HIP_TRY(hipMemsetAsync(c->Rbits.p, 0, 4, c->st));
  HIP_TRY(hipEventRecord(c->lv0, c->st));
  ia_launch_nbhd_rows(w, in.Aim, in.Apairs, g.NA, rows, mu, c->absmax.as<unsigned>(), c->st);
  HIP_TRY(hipGetLastError());
  std::vector<double> mu_h(D);
  unsigned abits = 0;
  HIP_TRY(hipMemcpyAsync(mu_h.data(), mu, (size_t)D * 8, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipMemcpyAsync(&abits, c->absmax.p, 4, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  float amaxf;
  std::memcpy(&amaxf, &abits, 4);
  bool finite = std::isfinite(amaxf);
  for (int f = 0; f < D; f++) finite = finite && std::isfinite(mu_h[f]);
  if (!finite) return fail(IA_EINVAL, who + ": the A side must be finite (and its column sums too)");
  scan->sc = dense_prescale(amaxf);
  ia_launch_dense_db(KH, rows, g.NA, D, g.n_tiles, mu, scan->sc, c->db.as<float4>(), c->Rbits.as<unsigned>(), c->st);
  HIP_TRY(hipEventRecord(c->lv1, c->st));
  scan->ma = dense_merge_args(c->rec.as<float4>(), c->recT.as<float>(), c->qn2.as<double>(), c->Rbits.as<unsigned>(), scan->nwg,
                              scan->tpw, g.n_tiles, g.NA, KH);
  return IA_OK;
}

// The step buffers of a level whose largest step holds Mt_max queries, and the scan's decomposition.
int ensure_nbhd_steps(ia_ctx *c, const LevelGeo &g, const NbhdGeo &w, int64_t Mt_max, NbhdScan *scan) {
  const int64_t Mpad_max = tile_pad(Mt_max);
  dense_geometry(g.n_tiles, &scan->tpw, &scan->nwg);
  const int nwg = scan->nwg;
  int rc;
  if ((rc = c->q64.ensure((size_t)Mt_max * w.D * 8)) || (rc = c->qn2.ensure((size_t)Mpad_max * 8)) ||
      (rc = c->qf.ensure((size_t)Mpad_max * 2 * g.KH * 4)) || (rc = c->rec.ensure((size_t)Mt_max * nwg * 16)) ||
      (rc = c->recT.ensure((size_t)Mt_max * nwg * 4)) || (rc = c->win.ensure((size_t)Mt_max * 8)) ||
      (rc = c->allwin.ensure((size_t)Mt_max * 8)))
    return rc;
  return IA_OK;
}

// One step of a window level, its queries from the wavefront's geometry or from a masked step's list:
// gather the query rows, the index's query prep, its scan in blocks of ia_k3_qtmax(KH) query tiles, its
// certified merge, then coherence / kappa / writeback: five launches (more scans when the step is
// wider than one block), nothing fused, nothing pruned.  Returns the scan launches.
int64_t run_nbhd_step(ia_ctx *c, const LevelGeo &g, const LevelInputs &in, const NbhdGeo &w, const NbhdScan &scan,
                      const NbhdStep &step) {
  const int D = w.D, KH = g.KH, Mt = step.n, Mpad = (int)tile_pad(Mt);
  double *rows = c->db64.as<double>(), *mu = c->mu.as<double>(), *q64 = c->q64.as<double>();
  int64_t *idx = c->win.as<int64_t>();
  int64_t scans = 0;
  ia_launch_nbhd_gather(w, step, in.Bim, in.jobs(), q64, c->st);
  ia_launch_dense_query(KH, q64, Mt, D, Mpad, mu, scan.sc, c->qn2.as<double>(), c->qf.as<float>(), c->st);
  index_scan_tiles(KH, 0, Mpad / IA_TILE, [&](int qt0, int qt) {
    ia_launch_k3(KH, qt, c->db.as<float4>(), c->qf.as<float4>(), g.n_tiles, scan.tpw, qt0, Mt, scan.nwg, 0, g.n_tiles,
                 c->rec.as<float4>(), c->recT.as<float>(), c->st);
    scans++;
  });
  ia_launch_merge_dense(scan.ma, rows, D, q64, Mt, scan.sc * scan.sc, idx, c->allwin.as<double>(), c->st);
  ia_launch_nbhd_finish(w, g, step, in.Aim, in.jobs(), rows, q64, idx, c->st);
  return scans;
}

// The level after its staging: the DB above, then the steps of the schedule t = col + (p_l + 1) row,
// all jobs in each.
int run_nbhd_level(ia_ctx *c, const ia_level_args *args, LevelPlan &P, LevelInputs &in, const NbhdGeo &w, ia_stats *stats) {
  const LevelGeo &g = P.g;
  int rc;
  ia_wavefront_shape_pad(g.bh, g.bw, w.p_l, &P.T, &P.Mmax);
  P.Mtmax = P.Mmax * P.J;
  P.Mpad_max = tile_pad(P.Mtmax);
  NbhdScan scan;
  if ((rc = stage_jobs(c, P, in)) || (rc = c->counters.ensure(5 * 8)) || (rc = ensure_nbhd_steps(c, g, w, P.Mtmax, &scan))) return rc;
  HIP_TRY(hipMemsetAsync(c->counters.p, 0, 5 * 8, c->st));
  if ((rc = build_nbhd_db(c, P, in, w, "ia_synthesize_levels_nbhd", &scan))) return rc;
  int64_t scans = 0;
  for (int64_t t = 0; t < P.T; t++) {
    StepDesc sd{(int)t, 0, 0, 0, P.J};
    ia_wavefront_step_pad(g.bh, g.bw, w.p_l, t, &sd.r0, &sd.M);
    if (sd.M <= 0) continue;  // levels narrower than p_l + 1 columns have empty steps
    sd.Mpad = (int)tile_pad(P.J * sd.M);
    scans += run_nbhd_step(c, g, in, w, scan, NbhdStep{sd, nullptr, P.J * sd.M});
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->lv2, c->st));
  if ((rc = finish_level(c, args, P, in, false, stats != nullptr))) return rc;
  if (!stats) return IA_OK;
  stats->nbhd_levels += P.J;
  return accumulate_side_stats(c, P.NB * P.J, P.T, scans, true, stats);
}

}  // namespace ia_host

using namespace ia_host;

extern "C" {

int ia_wavefront_shape_pad(int h, int w, int pad, int64_t *steps, int64_t *max_queries) {
  if (h < 1 || w < 1 || pad < 0 || pad > 4) return fail(IA_EINVAL, "ia_wavefront_shape_pad: empty level or pad outside 0..4");
  const int64_t k = pad + 1;
  if (steps) *steps = (int64_t)w + k * (int64_t)(h - 1);
  if (max_queries) *max_queries = std::min<int64_t>(h, (w + k - 1) / k);
  return IA_OK;
}

int ia_wavefront_step_pad(int h, int w, int pad, int64_t t, int *r0, int *M) {
  const int64_t k = pad + 1;
  if (h < 1 || w < 1 || pad < 0 || pad > 4 || !r0 || !M || t < 0 || t >= (int64_t)w + k * (int64_t)(h - 1))
    return fail(IA_EINVAL, "ia_wavefront_step_pad: bad step");
  const int64_t over = t - w + 1;  // rows r with t - k r >= w lie before the step
  const int64_t r_lo = over <= 0 ? 0 : (over + k - 1) / k;
  const int64_t r_hi = std::min<int64_t>(h - 1, t / k);
  *r0 = (int)r_lo;
  *M = (int)(r_hi - r_lo + 1);
  return IA_OK;
}

int ia_synthesize_levels_nbhd(ia_ctx *c, const ia_level_args *args, int n_jobs, int n_sm, int n_lg, ia_stats *stats) {
  if (!c || !args) return fail(IA_EINVAL, "ia_synthesize_levels_nbhd: NULL argument");
  int rc;
  if ((rc = check_level_batch(args, n_jobs)) || (rc = check_nbhd(c, args, n_jobs, n_sm, n_lg))) return rc;
  HIP_TRY(hipSetDevice(c->dev));
  const NbhdGeo w = ia_nbhd_geo(args[0].ch, n_sm, n_lg);
  LevelPlan P;
  LevelInputs in;
  if ((rc = plan_nbhd_level(c, args, n_jobs, w, P, in))) return rc;
  return run_nbhd_level(c, args, P, in, w, stats);
}

}  // extern "C"

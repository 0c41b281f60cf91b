// ia_level_kcoh.cpp — the k-coherence level (ia_synthesize_levels_kcoh with sim_k > 0, DESIGN.md
// §10): its checks and its step loop.  It shares the plan's first half, the staging and
// finish_level with the exact path (ia_level_run.cpp), and none of its steps; the context refusals are
// the side paths' one rule (ia_level_nbhd.cpp refuse_side_path).
#include "ia_level.h"

namespace ia_host {

// what the sets, the context and the batch must be for one (the jobs' own checks are check_level_args')
int check_kcoh(ia_ctx *c, const ia_level_args *args, int J, const int32_t *sim, int sim_k) {
  const ia_level_args *a = &args[0];
  if (sim_k < 0 || sim_k > IA_KCOH_MAX || (int64_t)sim_k > (int64_t)a->n_ap * a->a_h * a->a_w - 1)
    return fail(IA_EINVAL, "ia_synthesize_levels_kcoh: sim_k must be 0 (the exact path) or 1..min(IA_KCOH_MAX, N_A - 1)");
  if (!sim_k) return IA_OK;
  if (!sim) return fail(IA_EINVAL, "ia_synthesize_levels_kcoh: sim_k > 0 needs sim");
  return refuse_side_path(c, args, J, "ia_synthesize_level", "k-coherence levels (sim_k > 0)");
}

// The level after its staging: the similarity sets checked on the device (one pre-pass, one
// read-back), the fp64 row DB (K1b) alone, then one launch per wavefront step over all jobs, on
// the exact path's t = col + 3 row schedule.  No tiles, no scan, no records, no merge.  (If a call
// fails between two steps, the scan waves' counts may be left non-zero: they are cleared here.)
int run_kcoh_level(ia_ctx *c, const ia_level_args *args, LevelPlan &P, LevelInputs &in, const int32_t *sim_in, int K,
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
    const StepDesc sd = step_desc(g, t, P.J);
    if (sd.M <= 0) continue;  // levels narrower than 3 columns have empty steps
    ia_launch_kcoh_step(g, sd, in.Aim, in.Bim, in.jobs(), c->db64.as<double>(), sim, K, H, c->kc_part.p, c->kc_cnt.as<unsigned>(),
                        c->st);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->lv2, c->st));
  if ((rc = finish_level(c, args, P, in, false, stats != nullptr))) return rc;
  return stats ? accumulate_kcoh_stats(c, P, stats) : IA_OK;
}

}  // namespace ia_host

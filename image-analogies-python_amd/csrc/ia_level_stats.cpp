// ia_level_stats.cpp — what a finished level adds to the caller's ia_stats: the counters read
// back from the device, the event brackets of the sampled steps, and (option "stamps") the
// per-launch device times of the pruned scan and its merges; and the one tail of the side paths'
// levels (k-coherence, window, masked).
#include <cstdio>
#include <cstdlib>

#include "ia_level.h"

namespace ia_host {

// option "stamps": the level's per-launch device times (K3p launches, then merges) and the
// pruned scan's algorithmic bytes; db_stream = the DB bytes its kernels counted
static int accumulate_stamp_stats(ia_ctx *c, const StampSlots &s, const ScanTally &tally, double db_stream, ia_stats *stats) {
  const int64_t k3_n = s.k3_n, mg_n = s.mg_n;
  if (const char *dp = std::getenv("IA_STAMP_DUMP")) {
    // diagnostic: the raw per-workgroup stamps of this level's launches (K3p: IA_NWG_H slots
    // per launch, merges: mg_stride slots; (start | 1, end) ticks of 100 MHz) appended to a file
    std::vector<unsigned long long> r3((size_t)k3_n * IA_NWG_H * 2), rm((size_t)mg_n * s.mg_stride * 2);
    HIP_TRY(hipMemcpy(r3.data(), c->stamp_k3.p, r3.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rm.data(), c->stamp_mg.p, rm.size() * 8, hipMemcpyDeviceToHost));
    if (FILE *f = std::fopen(dp, "ab")) {
      const int64_t hdr[4] = {k3_n, IA_NWG_H, mg_n, s.mg_stride};
      std::fwrite(hdr, 8, 4, f);
      std::fwrite(r3.data(), 8, r3.size(), f);
      std::fwrite(rm.data(), 8, rm.size(), f);
      std::fclose(f);
    }
  }
  std::vector<unsigned long long> sp((size_t)2 * (k3_n + mg_n));  // (start, end) per launch: K3p, then merges
  HIP_TRY(hipMemcpy(sp.data(), c->stamp_dur.p, sp.size() * 8, hipMemcpyDeviceToHost));
  double tk = 0., tm = 0.;
  for (int64_t i = 0; i < k3_n; i++) tk += (double)(sp[2 * i + 1] - sp[2 * i]);
  for (int64_t i = k3_n; i < k3_n + mg_n; i++) tm += (double)(sp[2 * i + 1] - sp[2 * i]);
  stats->k3p_stamp_ms += tk * 1e-5;  // 100 MHz ticks
  {  // the launches' start spread and mean workgroup duration (k_stamp_durations span2)
    std::vector<unsigned long long> s2((size_t)2 * k3_n);
    HIP_TRY(hipMemcpy(s2.data(), c->stamp_dur.as<unsigned long long>() + 2 * (k3_n + mg_n), s2.size() * 8,
                      hipMemcpyDeviceToHost));
    double ss = 0., sw = 0.;
    for (int64_t i = 0; i < k3_n; i++) {
      ss += (double)s2[2 * i];
      sw += (double)s2[2 * i + 1];
    }
    stats->k3p_stamp_start_ms += ss * 1e-5;
    stats->k3p_stamp_wg_ms += sw * 1e-5;
  }
  stats->k3p_stamp_launches += k3_n;
  stats->merge_stamp_ms += tm * 1e-5;
  stats->merge_stamp_launches += mg_n;
  // one scan and one merge per step (a one-job unsharded level): the idle time of the level's
  // chain between its kernels, scan(t) -> merge(t) and merge(t) -> scan(t + 1)
  if (k3_n == mg_n + 1 || k3_n == mg_n) {
    const unsigned long long *m = sp.data() + 2 * k3_n;
    double gap = 0., gsm = 0.;
    int64_t ng = 0, nsm = 0;
    for (int64_t i = 0; i < mg_n; i++) {
      if (m[2 * i] && sp[2 * i + 1] && m[2 * i] >= sp[2 * i + 1]) {
        gsm += (double)(m[2 * i] - sp[2 * i + 1]);
        nsm++;
      }
      if (i + 1 < k3_n && sp[2 * (i + 1)] && m[2 * i + 1] && sp[2 * (i + 1)] >= m[2 * i + 1]) {
        gap += (double)(sp[2 * (i + 1)] - m[2 * i + 1]);
        ng++;
      }
    }
    stats->stamp_gap_ms += (gap + gsm) * 1e-5;
    stats->stamp_gaps += ng + nsm;
    stats->stamp_gap_sm_ms += gsm * 1e-5;
    stats->stamp_gaps_sm += nsm;
    stats->stamp_window_ms += (double)(std::max(sp[2 * k3_n - 1], m[2 * mg_n - 1]) - sp[0]) * 1e-5;
  }
  stats->k3p_bytes_all += db_stream + tally.bytes_all_fixed;
  // unique DB bytes: a launch reads each tile of its range at most once as
  // far as the roofline is concerned, however many query blocks stream it
  stats->k3p_bytes_unique_all += std::min(db_stream, tally.db_cap_all) + tally.bytes_all_fixed;
  return IA_OK;
}

int accumulate_stats(ia_ctx *c, const LevelPlan &P, const StampSlots &stamps, const ScanTally &tally, int64_t n_gm,
                     double gather_bytes_timed, ia_stats *stats) {
  const LevelGeo &g = P.g;
  const bool prune = P.prune;
  const int J = P.J;
  unsigned long long ctr[5], prs[4], pfull = 0, ptp = 0, ext[2] = {0, 0};
  HIP_TRY(hipMemcpy(ctr, c->counters.p, sizeof(ctr), hipMemcpyDeviceToHost));
  {  // per-workgroup counter slots (no same-address atomics in the distance kernel)
    std::vector<unsigned long long> slots(6 * IA_NWG_H);
    HIP_TRY(hipMemcpy(slots.data(), c->pairs.p, slots.size() * 8, hipMemcpyDeviceToHost));
    for (int j = 0; j < 4; j++) {
      prs[j] = 0;
      for (int w = 0; w < IA_NWG_H; w++) {
        const unsigned long long v = slots[j * IA_NWG_H + w];
        // pair slots: (pairs with corrections << 32) + pairs; tile slots: (tiles with a
        // filter-passing block << 32) + tiles loaded
        prs[j] += v & 0xffffffffull;
        (j < 2 ? pfull : ptp) += v >> 32;
      }
    }
    for (int w = 0; w < IA_NWG_H; w++) {  // DB half-tiles loaded besides one per loaded tile
      ext[0] += slots[4 * IA_NWG_H + w];
      ext[1] += slots[5 * IA_NWG_H + w];
    }
  }
  const double pair_flops = 2.0 * g.D * IA_TILE * IA_TILE;  // one (DB tile, query tile) pair
  // algorithmic DB bytes of the pruned scan, as each launch's kernel counted them (a
  // step may run another kernel than the option names, ia_k3p_launch.hip k3p_kernel): one half tile
  // (hi or lo) per loaded tile + the extra halves (whole tiles: the lo halves; hi-only stream:
  // the lo halves of the filter-passing tiles; two passes: the passing tiles again, whole)
  auto tile_stream_bytes = [&](double tiles, double extra) { return 0.5 * ia_k3h_tile_bytes(g.KS) * (tiles + extra); };
  const double dist_flops = prune ? pair_flops * (double)(prs[0] + prs[1]) : tally.dist_flops;
  const double flops_timed = prune ? pair_flops * (double)prs[1] : tally.flops_timed;
  stats->pruned_levels += prune ? J : 0;
  stats->dist_pairs += prune ? (double)(prs[0] + prs[1]) : tally.pairs_full;
  stats->dist_pairs_full += tally.pairs_full;
  stats->dist_tiles += prune ? (double)(prs[2] + prs[3]) : tally.tiles_full;
  stats->dist_tiles_full += tally.tiles_full;
  stats->dist_pairs_corrected += (double)pfull;
  stats->dist_tiles_rows += (double)ptp;
  float ms_db = 0.f, ms_syn = 0.f, ms_k1b = 0.f, ms_k1 = 0.f;
  hipEventElapsedTime(&ms_db, c->lv0, c->lv1);
  hipEventElapsedTime(&ms_syn, c->lv1, c->lv2);
  hipEventElapsedTime(&ms_k1b, c->kb[0], c->kb[1]);
  hipEventElapsedTime(&ms_k1, c->kb[2], c->kb[3]);
  if (g.NA >= stats->build_rows) {  // K1b: A-side images read once, every fp64 row written; K1: this
                                    // process's rows read, tiles written (the largest level seen)
    if (g.NA > stats->build_rows) {
      stats->k1b_ms = stats->k1b_bytes = stats->k1_ms = stats->k1_bytes = 0.;
      stats->build_levels = 0;
      stats->build_rows = g.NA;
    }
    const int DSb = ia_db64_stride(g.ch);
    stats->k1b_ms += ms_k1b;
    stats->k1b_bytes += (double)(P.nA + P.nAc) * (g.n_a + g.n_ap) * 8 + (double)g.NA * DSb * 8;
    if (P.ns > 0 && P.use_h) {
      stats->k1_ms += ms_k1;
      stats->k1_bytes += (double)std::min<int64_t>((int64_t)P.ns * IA_TILE, g.NA) * DSb * 8 + (double)P.ns * P.tile_bytes;
    }
    stats->build_levels += 1;
  }
  for (int64_t i = 0; i < n_gm; i++) {
    float mg = 0.f, mm = 0.f;
    hipEventElapsedTime(&mg, c->evg[2 * i], c->evg[2 * i + 1]);
    hipEventElapsedTime(&mm, c->evm[2 * i], c->evm[2 * i + 1]);
    stats->gather_ms_timed += mg;
    stats->merge_ms_timed += mm;
  }
  stats->gather_launches_timed += n_gm;
  stats->merge_launches_timed += n_gm;
  stats->gather_bytes_timed += gather_bytes_timed;
  stats->pixels += P.NB * J;
  stats->steps += P.T;
  stats->reranked += (int64_t)ctr[0];
  stats->fallbacks += (int64_t)ctr[1];
  stats->coherence_wins += (int64_t)ctr[2];
  stats->bound_violations += (int64_t)ctr[3];
  stats->kappa_ambiguous += (int64_t)ctr[4];
  stats->f16_levels += P.use_h ? J : 0;
  stats->db_ms += ms_db;
  stats->synth_ms += ms_syn;
  stats->dist_launches += tally.dist_launches;
  stats->dist_flops += dist_flops;
  // the pruned scan's timing fields (prune_*, k3p_*, merge_stamp_*, stamp_*) describe the
  // pruned levels with the largest DB seen (prune_rows: the bench's finest level), like k1*_ms
  bool prune_acc = false;
  if (prune && g.NA >= stats->prune_rows) {
    if (g.NA > stats->prune_rows) {
      stats->prune_ms_timed = stats->prune_flops_timed = stats->prune_bytes_timed = 0.;
      stats->prune_launches_timed = 0;
      stats->k3p_stamp_ms = stats->k3p_bytes_all = stats->merge_stamp_ms = stats->stamp_gap_ms = stats->stamp_window_ms = 0.;
      stats->k3p_stamp_start_ms = stats->k3p_stamp_wg_ms = stats->stamp_gap_sm_ms = 0.;
      stats->stamp_gaps_sm = 0;
      stats->k3p_stamp_launches = stats->merge_stamp_launches = stats->stamp_gaps = 0;
      stats->k3p_bytes_unique_all = 0.;
      stats->prune_rows = g.NA;
    }
    prune_acc = true;
  }
  int rc;
  if (stamps.on && prune_acc && stamps.k3_n + stamps.mg_n > 0 &&
      (rc = accumulate_stamp_stats(c, stamps, tally, tile_stream_bytes((double)(prs[2] + prs[3]), (double)(ext[0] + ext[1])),
                                   stats)))
    return rc;
  if (P.stride && P.ns > 0) {
    double tot = 0.;
    for (int64_t i = 0; i < tally.n_rec; i++) {
      float ms = 0.f;
      hipEventElapsedTime(&ms, c->evs[2 * i], c->evs[2 * i + 1]);
      tot += ms;
    }
    stats->dist_ms += tot;
    stats->dist_launches_timed += tally.launches_timed;
    stats->dist_flops_timed += flops_timed;
    if (prune_acc) {  // the pruned scan alone (bench roofline): time, MFMA flops, algorithmic bytes
      stats->prune_ms_timed += tot;
      stats->prune_launches_timed += tally.launches_timed;
      stats->prune_flops_timed += flops_timed;
      stats->prune_bytes_timed += tile_stream_bytes((double)prs[3], (double)ext[1]) + tally.bytes_timed_fixed;
    }
  }
  return IA_OK;
}

int accumulate_side_stats(ia_ctx *c, int64_t pixels, int64_t steps, int64_t scans, bool built, ia_stats *stats, SideTail *tail) {
  SideTail t;
  HIP_TRY(hipMemcpy(t.ctr, c->counters.p, sizeof(t.ctr), hipMemcpyDeviceToHost));
  stats->pixels += pixels;
  stats->steps += steps;
  stats->coherence_wins += (int64_t)t.ctr[2];
  stats->kappa_ambiguous += (int64_t)t.ctr[4];
  stats->dist_launches += scans;
  if (built) {
    hipEventElapsedTime(&t.ms_db, c->lv0, c->lv1);
    hipEventElapsedTime(&t.ms_syn, c->lv1, c->lv2);
    stats->db_ms += t.ms_db;
    stats->synth_ms += t.ms_syn;
  }
  if (tail) *tail = t;
  return IA_OK;
}

// a k-coherence level (no scan, no tiles): the side paths' tail, and of its own the stats words that
// carry the candidates where K4 counts reranks and the fallback pixels where it counts rescanned
// chunks, and the K1b fields (K1b is the whole DB build)
int accumulate_kcoh_stats(ia_ctx *c, const LevelPlan &P, ia_stats *stats) {
  const LevelGeo &g = P.g;
  SideTail t;
  int rc;
  if ((rc = accumulate_side_stats(c, P.NB * P.J, P.T, 0, true, stats, &t))) return rc;
  if (g.NA >= stats->build_rows) {
    if (g.NA > stats->build_rows) {
      stats->k1b_ms = stats->k1b_bytes = stats->k1_ms = stats->k1_bytes = 0.;
      stats->build_levels = 0;
      stats->build_rows = g.NA;
    }
    stats->k1b_ms += t.ms_db;
    stats->k1b_bytes += (double)(P.nA + P.nAc) * (g.n_a + g.n_ap) * 8 + (double)g.NA * ia_db64_stride(g.ch) * 8;
    stats->build_levels += 1;
  }
  stats->kcoh_levels += P.J;
  stats->kcoh_candidates += (int64_t)t.ctr[0];
  stats->kcoh_fallbacks += (int64_t)t.ctr[1];
  return IA_OK;
}

}  // namespace ia_host

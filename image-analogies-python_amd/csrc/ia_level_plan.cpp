// ia_level_plan.cpp — phases 1-3 of a level call, everything before its first step: the
// argument checks, the plan (geometry, shards, scan decomposition, scratch), the staging of the
// A side and of every job's B side, and the level's DB with the pruned scan's table.
#include <cmath>
#include <cstring>

#include "ia_level.h"

namespace ia_host {

// cyclic Jacobi eigen-decomposition of a symmetric n x n matrix (row-major, overwritten);
// V's column k is the eigenvector of eigenvalue w[k]
static void jacobi_eig(int n, std::vector<double> &A, std::vector<double> &V, std::vector<double> &w) {
  V.assign((size_t)n * n, 0.);
  for (int i = 0; i < n; i++) V[(size_t)i * n + i] = 1.;
  auto a = [&](int i, int j) -> double & { return A[(size_t)i * n + j]; };
  for (int sweep = 0; sweep < 100; sweep++) {
    double off = 0., dia = 0.;
    for (int p = 0; p < n; p++) {
      dia += a(p, p) * a(p, p);
      for (int q = p + 1; q < n; q++) off += a(p, q) * a(p, q);
    }
    if (off <= 1e-32 * dia || off == 0.) break;
    for (int p = 0; p < n - 1; p++) {
      for (int q = p + 1; q < n; q++) {
        const double apq = a(p, q);
        if (apq == 0.) continue;
        const double theta = (a(q, q) - a(p, p)) / (2. * apq);
        const double t = (theta >= 0. ? 1. : -1.) / (std::fabs(theta) + std::sqrt(theta * theta + 1.));
        const double cs = 1. / std::sqrt(t * t + 1.), sn = t * cs;
        for (int k = 0; k < n; k++) {  // columns p, q
          const double akp = a(k, p), akq = a(k, q);
          a(k, p) = cs * akp - sn * akq;
          a(k, q) = sn * akp + cs * akq;
        }
        for (int k = 0; k < n; k++) {  // rows p, q
          const double apk = a(p, k), aqk = a(q, k);
          a(p, k) = cs * apk - sn * aqk;
          a(q, k) = sn * apk + cs * aqk;
        }
        for (int k = 0; k < n; k++) {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = cs * vkp - sn * vkq;
          V[(size_t)k * n + q] = sn * vkp + cs * vkq;
        }
      }
    }
  }
  w.resize(n);
  for (int i = 0; i < n; i++) w[i] = a(i, i);
}

// Per-level setup of the certified pruned scan (ia_prune.hip): covariance of
// the centred fp64 DB (sampled) -> top IA_NPC eigenvectors (host Jacobi) -> projections and
// Morton keys of every row -> radix sort -> position -> row table + per-tile projection boxes.
// Sets g.pos2row; *ufac = the U' factor of ia_prune.h.  One host sync (the covariance).
static int prepare_prune(ia_ctx *c, LevelGeo &g, const double *mu, int W, double *ufac) {
  constexpr int D = 55, NPAIR = D * (D + 1) / 2, NWG_COV = 256;
  const int64_t NA = g.NA, NT = g.n_tiles;
  const int64_t stride = std::max<int64_t>(1, NA / 65536), nsamp = (NA + stride - 1) / stride;
  int rc;
  if ((rc = c->pr_part.ensure((size_t)NWG_COV * NPAIR * 8)) || (rc = c->pr_cov.ensure((size_t)NPAIR * 8)) ||
      (rc = c->pr_basis.ensure((size_t)(IA_NPC * D + IA_NPC) * 8)) || (rc = c->pr_proj.ensure((size_t)NA * (IA_NPC * 8 + 4))) ||
      (rc = c->pr_keys.ensure((size_t)NA * 8)) || (rc = c->pr_rows.ensure((size_t)NA * 8)) ||
      (rc = c->pos2row.ensure((size_t)NT * IA_TILE * 4)) || (rc = c->boxes.ensure((size_t)NT * 2 * IA_NPC * 4)) ||
      (rc = c->tnorm.ensure((size_t)NT * 4)))
    return rc;
  const size_t sort_bytes = ia_sort_temp_bytes(NA);
  if ((rc = c->pr_tmp.ensure(sort_bytes))) return rc;
  ia_launch_cov(c->db64.as<double>(), NA, stride, NWG_COV, mu, c->pr_part.as<double>(), c->pr_cov.as<double>(), c->st);
  std::vector<double> cov(NPAIR);
  HIP_TRY(hipMemcpyAsync(cov.data(), c->pr_cov.p, NPAIR * 8, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  std::vector<double> A((size_t)D * D), V, w;
  for (int f = 0, p = 0; f < D; f++)
    for (int h = f; h < D; h++, p++) A[(size_t)f * D + h] = A[(size_t)h * D + f] = cov[p] / (double)nsamp;
  jacobi_eig(D, A, V, w);
  std::vector<int> idx(D);
  for (int i = 0; i < D; i++) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return w[x] > w[y]; });
  c->basis_h.assign((size_t)IA_NPC * D + IA_NPC, 0.);
  for (int i = 0; i < IA_NPC; i++) {
    double nrm = 0.;
    for (int f = 0; f < D; f++) nrm += V[(size_t)f * D + idx[i]] * V[(size_t)f * D + idx[i]];
    nrm = std::sqrt(nrm);
    for (int f = 0; f < D; f++) c->basis_h[(size_t)i * D + f] = V[(size_t)f * D + idx[i]] / nrm;
    const double lam = w[idx[i]];
    c->basis_h[(size_t)IA_NPC * D + i] = lam > 0. ? 1. / (4. * std::sqrt(lam)) : 0.;
  }
  // deviation of the basis from orthonormality: lambda_max(U^T U) <= 1 + sum |G - I|
  long double delta = 0.L;
  for (int i = 0; i < IA_NPC; i++)
    for (int j = 0; j < IA_NPC; j++) {
      long double gij = 0.L;
      for (int f = 0; f < D; f++) gij += (long double)c->basis_h[(size_t)i * D + f] * c->basis_h[(size_t)j * D + f];
      delta += std::fabs((double)(gij - (i == j ? 1.L : 0.L)));
    }
  *ufac = (1.0 + 2.0 * (double)delta + 1e-15) * (1.0 + std::ldexp(1.0, -17)) * (1.0 + std::ldexp(1.0, -19));
  HIP_TRY(hipMemcpyAsync(c->pr_basis.p, c->basis_h.data(), c->basis_h.size() * 8, hipMemcpyHostToDevice, c->st));
  unsigned *keys = c->pr_keys.as<unsigned>();
  int *rows = c->pr_rows.as<int>();
  float *rnorm = reinterpret_cast<float *>(c->pr_proj.as<double>() + NA * IA_NPC);  // |a'| per row, rounded up
  ia_launch_proj_keys(c->db64.as<double>(), NA, mu, c->pr_basis.as<double>(), c->pr_proj.as<double>(), keys, rows, rnorm,
                      c->st);
  if (ia_sort_pairs(c->pr_tmp.p, sort_bytes, keys, keys + NA, rows, rows + NA, NA, c->st) != 0)
    return fail(IA_EHIP, "prepare_prune: radix sort failed");
  ia_launch_table_boxes(rows + NA, c->pr_proj.as<double>(), NA, (int)NT, W, c->prune_group, c->pos2row.as<int>(),
                        c->boxes.as<float>(), rnorm,
                        c->tnorm.as<float>(), c->st);
  HIP_TRY(hipGetLastError());
  g.pos2row = c->pos2row.as<int>();
  return IA_OK;
}

static int stage(ia_ctx *c, DevBuf &buf, const void *src, size_t bytes, int mem, const void **dev) {
  if (mem == IA_MEM_DEVICE) {
    *dev = src;
    return IA_OK;
  }
  int rc = buf.ensure(bytes);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, c->st));
  *dev = buf.p;
  return IA_OK;
}

int check_level_args(const ia_level_args *a) {
  if (a->ch < 1 || a->ch > 3) return fail(IA_EINVAL, "ia_synthesize_level: ch must be 1, 2 or 3");
  if (a->n_ap < 1 || a->a_h < 1 || a->a_w < 1 || a->b_h < 1 || a->b_w < 1)
    return fail(IA_EINVAL, "ia_synthesize_level: empty image or no A' image");
  if (!a->A || !a->Ac || !a->Ap || !a->Apc || !a->B || !a->Bc || !a->Bpc || !a->Bp || !a->weights || !a->s_out ||
      !a->im_out)
    return fail(IA_EINVAL, "ia_synthesize_level: NULL image pointer");
  if (a->mem != IA_MEM_HOST && a->mem != IA_MEM_DEVICE) return fail(IA_EINVAL, "ia_synthesize_level: bad mem kind");
  if ((a->dbg_src == nullptr) != (a->dbg_dist == nullptr))
    return fail(IA_EINVAL, "ia_synthesize_level: dbg_src and dbg_dist are given together or not at all");
  if (a->n_a != 0 && a->n_a != 1 && a->n_a != a->n_ap)
    return fail(IA_EINVAL, "ia_synthesize_level: n_a must be 0 or 1 (one A shared by every A') or n_ap (one A per A')");
  if ((int64_t)a->n_ap * a->a_h * a->a_w >= (int64_t)INT32_MAX)
    return fail(IA_EINVAL, "ia_synthesize_level: DB rows exceed int32 row ids");
  return IA_OK;
}

// the jobs of one level call: each valid, all on one A side with one set of shapes
int check_level_batch(const ia_level_args *args, int n_jobs) {
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
  return IA_OK;
}

int plan_shards(ia_ctx *c, const ia_level_args *args, int J, LevelPlan &P) {
  const ia_level_args *a = &args[0];
  int rc;
  LevelGeo &g = P.g;
  g.pos2row = nullptr;
  g.ch = a->ch;
  g.D = 55 * a->ch;
  g.KH = kh_for(g.D + 1);
  P.J = J;
  P.DP = 2 * g.KH;
  g.n_ap = a->n_ap;
  g.n_a = a->n_a > 1 ? a->n_a : 1;
  g.ah = a->a_h;
  g.aw = a->a_w;
  g.ahc = (a->a_h + 1) / 2;
  g.awc = (a->a_w + 1) / 2;
  g.bh = a->b_h;
  g.bw = a->b_w;
  g.bhc = (a->b_h + 1) / 2;
  g.bwc = (a->b_w + 1) / 2;
  g.NA = (int64_t)g.n_ap * g.ah * g.aw;
  g.n_tiles = (int)((g.NA + IA_TILE - 1) / IA_TILE);
  // DB shards: over the ranks of ia_comm_init (world > 1), or emulated on this device (option
  // "shard_emulate" = W: the W shards' scans and per-shard certified winners run here one after
  // the other, then the multi-rank finish; no RCCL).  Levels under 64 tiles per shard replicate.
  // Only levels that run the pruned scan are sharded by default: the unpruned scan of a 512^2 or
  // smaller DB gains nothing from 1/W of the tiles once the exchange is paid (DESIGN.md §7,
  // profiles/r03/shard); option "shard_unpruned" = 1 shards those too (tests, very large DBs).
  const bool shard_here = c->shard_unpruned ||
                          (c->prune && c->matcher == IA_MATCH_F16X3 && g.ch == 1 && g.NA >= c->prune_min_rows);
  P.sharded = shard_here && shard_level(g.n_tiles, c->world);
  P.emulated = shard_here && !P.sharded && c->world == 1 && c->shard_emulate > 1 && shard_level(g.n_tiles, c->shard_emulate);
  P.Wsh = P.sharded ? c->world : P.emulated ? c->shard_emulate : 1;
  P.multi = P.Wsh > 1;
  P.xchg = P.multi && c->exchange == 1;
  // owner-computes: a rank brings its own job (emulated: one job per shard); checked against the
  // pruned scan in plan_scan
  P.xo = P.multi && c->exchange == 2;
  if (P.xo) {
    if (P.sharded && !c->xpeer[0]) return fail(IA_EINVAL, "ia_synthesize_level: exchange = 2 needs ia_xchg_open");
    if (P.Wsh > IA_XCHG_MAXW) return fail(IA_EINVAL, "ia_synthesize_level: the owner exchange takes <= 16 shards");
    if (P.sharded && J != 1) return fail(IA_EINVAL, "ia_synthesize_level: exchange = 2 takes the rank's own job (n_jobs = 1)");
    if (P.emulated && J != P.Wsh)
      return fail(IA_EINVAL, "ia_synthesize_levels: emulated exchange = 2 takes one job per shard (n_jobs = shard_emulate)");
    if (P.emulated && (rc = xchg_alloc(c, P.Wsh))) return rc;
    if ((rc = c->xo_inv.ensure((size_t)IA_XO_MAXT * IA_TILE * 4))) return rc;
    HIP_TRY(hipMemsetAsync(c->xerr.p, 0, 4, c->st));
  }
  if (P.xchg) {
    if (P.sharded && !c->xpeer[0]) return fail(IA_EINVAL, "ia_synthesize_level: exchange = 1 needs ia_xchg_open");
    if (P.Wsh > IA_XCHG_MAXW) return fail(IA_EINVAL, "ia_synthesize_level: the peer-write exchange takes <= 16 shards");
    if (P.emulated && (rc = xchg_alloc(c, P.Wsh))) return rc;
    if ((int64_t)std::min(g.bh, (g.bw + 2) / 3) * J > IA_XCHG_MAXQ)
      return fail(IA_EINVAL, "ia_synthesize_level: wavefront steps (all jobs) wider than the exchange slots");
    HIP_TRY(hipMemsetAsync(c->xerr.p, 0, 4, c->st));
  }
  for (int j = 0; j < J; j++)
    if (P.multi && args[j].dbg_src)
      return fail(IA_EINVAL, "ia_synthesize_level: debug outputs are produced by single-rank levels only");
  int64_t t0 = 0, t1 = g.n_tiles;  // this rank's contiguous DB tiles (unpruned sharded levels hold only those)
  if (P.sharded) ia_shard_tiles(g.NA, c->world, c->rank, &t0, &t1);
  g.tile0 = (int)t0;
  g.tile1 = (int)t1;
  P.nA = (size_t)g.ah * g.aw * g.ch;
  P.nAc = (size_t)g.ahc * g.awc * g.ch;
  P.nB = (size_t)g.bh * g.bw * g.ch;
  P.nBc = (size_t)g.bhc * g.bwc * g.ch;
  P.NB = (int64_t)g.bh * g.bw;
  return IA_OK;
}

int plan_scan(ia_ctx *c, bool use_h, LevelPlan &P) {
  LevelGeo &g = P.g;
  const int J = P.J;
  P.use_h = use_h;
  g.KS = use_h ? ia_ks_for(g.ch) : 0;
  // certified pruned scan (1 channel, large DBs; every query of a step sorted in one
  // workgroup's LDS)
  ia_wavefront_shape(g.bh, g.bw, &P.T, &P.Mmax);
  P.Mtmax = P.Mmax * J;
  // (exchange = 2 emulated: each owner's queries at its own tile-aligned offset j Mpad_j)
  P.Mpad_max = std::max(tile_pad(P.Mtmax), P.xo ? J * tile_pad(P.Mmax) : 0);
  P.prune = c->prune && use_h && g.ch == 1 && g.NA >= c->prune_min_rows && P.Mpad_max <= 4096 &&
            (g.n_tiles + c->scan_wgs - 1) / c->scan_wgs <= IA_K3P_MAXK_LDS;
  const bool prune = P.prune;
  if (P.xo && !prune)
    return fail(IA_EINVAL, "ia_synthesize_level: exchange = 2 shards pruned levels only (1 channel, split-f16, <= 4096 "
                           "queries per step)");
  // owner-computes geometry (pads past an owner's QTj query tiles are never contracted)
  if (P.xo) {
    const int QTj = (int)(tile_pad(P.Mmax) / IA_TILE);
    P.xo_bpj = (QTj + ia_k3h_qtmax(g.KS) - 1) / ia_k3h_qtmax(g.KS);
    P.xo_QTx = (QTj + P.xo_bpj - 1) / P.xo_bpj;
    P.xo_QTs = P.xo_bpj * P.xo_QTx;
    if (P.Wsh * P.xo_QTs > IA_XO_MAXT || P.Wsh * P.xo_bpj > IA_NWG_H)
      return fail(IA_EINVAL, "ia_synthesize_level: exchange = 2: wavefront steps too wide for the exchange area");
  }
  // Pruned levels: every rank holds the whole Morton-sorted DB, its tiles stored shard by shard
  // (ia_internal.h ia_shard_morton_tile: shard r = Morton tiles r, r + W, ...), and scans its own
  // contiguous storage range.  Unpruned levels: contiguous tile ranges (ia_shard_tiles).
  if (prune) {
    g.tile0 = 0;
    g.tile1 = g.n_tiles;
  }
  P.ns = g.tile1 - g.tile0;
  auto decomp = [&](int t0, int t1) {
    Shard d{t0, t1, 0, 0};
    const int n = t1 - t0;
    if (prune) d.nwg = std::min(c->scan_wgs, n);  // round-robin chunks: WG w owns tiles w + nwg*k
    else {
      d.tpw = use_h ? std::max(IA_WGH / IA_WAVE, (n + c->scan_wgs - 1) / c->scan_wgs) : std::max(4, (n + IA_WG_TARGET - 1) / IA_WG_TARGET);
      d.nwg = (n + d.tpw - 1) / d.tpw;
    }
    return d;
  };
  if (!P.multi) {
    P.shards.push_back(decomp(g.tile0, g.tile1));
  } else {
    for (int r = P.sharded ? c->rank : 0; r < (P.sharded ? c->rank + 1 : P.Wsh); r++) {
      int64_t t0 = ia_shard_off(g.n_tiles, P.Wsh, r), t1 = ia_shard_off(g.n_tiles, P.Wsh, r + 1);
      if (!prune) ia_shard_tiles(g.NA, P.Wsh, r, &t0, &t1);
      P.shards.push_back(decomp((int)t0, (int)t1));
    }
  }
  int nwg_max = 1;
  for (const Shard &x : P.shards) nwg_max = std::max(nwg_max, x.nwg);
  g.nwg = P.shards[0].nwg;
  g.tiles_per_wg = P.shards[0].tpw;
  P.rec_stride = (size_t)P.Mtmax * nwg_max;
  P.db_row_bytes = use_h ? (size_t)16 * g.KS * 4 : (size_t)P.DP * 4;
  P.tile_bytes = use_h ? (size_t)ia_k3h_tile_bytes(g.KS) : (size_t)IA_TILE * P.DP * 4;
  P.qtmax = use_h ? ia_k3h_qtmax(g.KS) : ia_k3_qtmax(g.KH);
  P.stride = c->time_dist > 0 ? c->time_dist : 0;
  return IA_OK;
}

// per-level scratch
int ensure_scratch(ia_ctx *c, const LevelPlan &P) {
  const LevelGeo &g = P.g;
  const size_t Mp = (size_t)P.Mpad_max, nsh = P.shards.size();
  int rc;
  if ((rc = c->db.ensure((size_t)std::max(P.ns, 1) * IA_TILE * P.db_row_bytes)) || (rc = c->mu.ensure((16 + 4 * 3 * 128) * 8)) ||
      (rc = c->db64.ensure((size_t)g.NA * ia_db64_stride(g.ch) * 8)) ||
      (rc = c->Rbits.ensure(4)) || (rc = c->q64.ensure(Mp * g.D * 8 * 2)) ||
      (rc = c->qn2.ensure(Mp * 8 * 2)) || (rc = c->qf.ensure(Mp * P.db_row_bytes)) ||
      (rc = c->rec.ensure(P.rec_stride * nsh * 16)) || (rc = c->recT.ensure(P.rec_stride * nsh * 4)) ||
      (rc = c->win.ensure((size_t)P.Mtmax * 16)) || (rc = c->allwin.ensure((size_t)P.Mtmax * 16 * P.Wsh)) ||
      (rc = c->counters.ensure(5 * 8)) || (rc = c->pairs.ensure(6 * IA_NWG_H * 8)) ||
      (rc = c->qinfo.ensure(P.prune ? Mp * 3 * 16 * 2 : 16)))
    return rc;
  if (P.prune && ((rc = c->qs_order.ensure(Mp * 4)) || (rc = c->qs_info.ensure(Mp * 3 * 16)) ||
                  (rc = c->qs_frag.ensure(Mp * P.db_row_bytes)) || (rc = c->qs_tbox.ensure(Mp / IA_TILE * 3 * 16))))
    return rc;
  return IA_OK;
}

// the A side and the B side of every job (host buffers: one staging set per job)
int stage_level(ia_ctx *c, const ia_level_args *args, const LevelPlan &P, LevelInputs &in) {
  const ia_level_args *a = &args[0];
  const LevelGeo &g = P.g;
  const int J = P.J;
  const size_t nA = P.nA, nAc = P.nAc, nB = P.nB, nBc = P.nBc;
  const int64_t NB = P.NB;
  int rc;
  const void *dA, *dAc, *dAp, *dApc;
  if ((rc = stage(c, c->A, a->A, nA * g.n_a * 8, a->mem, &dA)) || (rc = stage(c, c->Ac, a->Ac, nAc * g.n_a * 8, a->mem, &dAc)) ||
      (rc = stage(c, c->Ap, a->Ap, nA * g.n_ap * 8, a->mem, &dAp)) ||
      (rc = stage(c, c->Apc, a->Apc, nAc * g.n_ap * 8, a->mem, &dApc)))
    return rc;
  in.Aim = Imgs{(const double *)dAc, (const double *)dA, (const double *)dApc, (const double *)dAp,
                g.ah, g.aw, g.ahc, g.awc, (int64_t)nA, (int64_t)nAc};
  in.Apairs = g.n_a > 1 ? APairs{(int64_t)nA, (int64_t)nAc, g.n_a} : APairs{0, 0, 1};
  in.Bim = Imgs{nullptr, nullptr, nullptr, nullptr, g.bh, g.bw, g.bhc, g.bwc, 0, 0};
  if ((int)c->jb.size() < J) c->jb.resize(J);
  in.jp.resize(J);
  for (int j = 0; j < J; j++) {
    const ia_level_args *x = &args[j];
    JobBufs &b = c->jb[j];
    const void *dB, *dBc, *dBpc, *dW;
    if ((rc = stage(c, b.B, x->B, nB * 8, x->mem, &dB)) || (rc = stage(c, b.Bc, x->Bc, nBc * 8, x->mem, &dBc)) ||
        (rc = stage(c, b.Bpc, x->Bpc, nBc * 8, x->mem, &dBpc)) || (rc = stage(c, b.W, x->weights, (size_t)g.D * 8, x->mem, &dW)) ||
        (rc = b.pstat.ensure((size_t)NB * 4)))
      return rc;
    JobPtrs &p = in.jp[j];
    p.Bc = (const double *)dBc;
    p.B = (const double *)dB;
    p.Bpc = (const double *)dBpc;
    p.weights = (const double *)dW;
    p.kf = x->kappa_factor;
    p.pstat = b.pstat.as<unsigned>();
    p.nn = nullptr;
    if (x->mem == IA_MEM_DEVICE) {
      p.Bp = x->Bp;
      p.s = x->s_out;
      p.im = x->im_out;
      p.dbg_src = x->dbg_src;
      p.dbg_dist = x->dbg_dist;
    } else {
      if ((rc = b.Bp.ensure(nB * 8)) || (rc = b.S.ensure((size_t)NB * 8)) || (rc = b.IM.ensure((size_t)NB * 4))) return rc;
      p.Bp = b.Bp.as<double>();
      p.s = b.S.as<int32_t>();
      p.im = b.IM.as<int32_t>();
      HIP_TRY(hipMemcpyAsync(p.Bp, x->Bp, nB * 8, hipMemcpyHostToDevice, c->st));
      p.dbg_src = nullptr;
      p.dbg_dist = nullptr;
      if (x->dbg_src) {
        if ((rc = b.DSRC.ensure((size_t)NB * 24)) || (rc = b.DDIST.ensure((size_t)NB * 16))) return rc;
        p.dbg_src = b.DSRC.as<int32_t>();
        p.dbg_dist = b.DDIST.as<double>();
      }
    }
    HIP_TRY(hipMemsetAsync(p.pstat, 0, (size_t)NB * 4, c->st));
  }
  return IA_OK;
}

// matcher: split-f16 when the channel count has a K3h instance and every image value fits
// (IA_F16_MAXABS, one 4-byte read-back per level); otherwise the fp32 MFMA scan
int probe_matcher(ia_ctx *c, const LevelPlan &P, const LevelInputs &in, bool *use_h) {
  const LevelGeo &g = P.g;
  *use_h = false;
  if (c->matcher != IA_MATCH_F16X3 || ia_ks_for(g.ch) <= 0) return IA_OK;
  int rc;
  if ((rc = c->absmax.ensure(4))) return rc;
  HIP_TRY(hipMemsetAsync(c->absmax.p, 0, 4, c->st));
  const Imgs &A = in.Aim;
  for (int j = 0; j < P.J; j++) {
    const JobPtrs &p = in.jp[j];
    const double *arrs[8] = {j ? nullptr : A.p1, j ? nullptr : A.p0, j ? nullptr : A.p3, j ? nullptr : A.p2, p.B, p.Bc, p.Bpc, p.Bp};
    const int64_t ns8[8] = {(int64_t)(P.nA * g.n_a), (int64_t)(P.nAc * g.n_a), (int64_t)(P.nA * g.n_ap), (int64_t)(P.nAc * g.n_ap),
                            (int64_t)P.nB, (int64_t)P.nBc, (int64_t)P.nBc, (int64_t)P.nB};
    ia_launch_absmax(arrs, ns8, c->absmax.as<unsigned>(), c->st);
  }
  unsigned mbits = 0;
  HIP_TRY(hipMemcpyAsync(&mbits, c->absmax.p, 4, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  float mx;
  std::memcpy(&mx, &mbits, 4);
  *use_h = mx <= IA_F16_MAXABS;
  return IA_OK;
}

// option "nn_bound": per-pixel exact NN rows of a pruned one-rank level (-1 until merged; every
// merge form writes it: fused, owner-computes, exchange finishes); then the device JobPtrs table
int stage_jobs(ia_ctx *c, const LevelPlan &P, LevelInputs &in) {
  int rc;
  for (int j = 0; j < P.J && P.prune && c->nn_bound; j++) {
    JobBufs &b = c->jb[j];
    if ((rc = b.NN.ensure((size_t)P.NB * 4))) return rc;
    in.jp[j].nn = b.NN.as<int32_t>();
    HIP_TRY(hipMemsetAsync(in.jp[j].nn, 0xFF, (size_t)P.NB * 4, c->st));
  }
  if ((rc = c->jobs.ensure(sizeof(JobPtrs) * P.J))) return rc;
  HIP_TRY(hipMemcpyAsync(c->jobs.p, in.jp.data(), sizeof(JobPtrs) * P.J, hipMemcpyHostToDevice, c->st));
  in.dev_jobs = c->jobs.as<JobPtrs>();
  return IA_OK;
}

// ---- phase 3: the DB ------------------------------------------------------------------------
// means, the fp64 row DB (K1b: every row, coherence reads any row), the pruned scan's table
// (sets g.pos2row, *ufac) and this process's tiles (K1), bracketed by lv0 / kb[0..3] / lv1
int build_level_db(ia_ctx *c, LevelPlan &P, const LevelInputs &in, double *ufac) {
  LevelGeo &g = P.g;
  int rc;
  HIP_TRY(hipEventRecord(c->lv0, c->st));
  ia_launch_means(g.ch, in.Aim, in.Apairs, g.n_ap, c->mu.as<double>(), c->st);
  HIP_TRY(hipEventRecord(c->kb[0], c->st));
  ia_launch_db64_build(g, in.Aim, in.Apairs, c->db64.as<double>(), c->st);
  HIP_TRY(hipEventRecord(c->kb[1], c->st));
  *ufac = 0.;
  if (P.prune && (rc = prepare_prune(c, g, c->mu.as<double>(), P.Wsh, ufac))) return rc;
  HIP_TRY(hipEventRecord(c->kb[2], c->st));
  if (P.ns > 0) {
    if (P.use_h) ia_launch_db_build_h(g, in.Aim, c->db64.as<double>(), c->mu.as<double>(), c->db.p, c->Rbits.as<unsigned>(), c->st);
    else ia_launch_db_build(g, in.Aim, in.Apairs, c->mu.as<double>(), c->db.as<float4>(), c->Rbits.as<unsigned>(), c->st);
  }
  HIP_TRY(hipEventRecord(c->kb[3], c->st));
  HIP_TRY(hipEventRecord(c->lv1, c->st));
  return IA_OK;
}

}  // namespace ia_host

// ia_index_radius.cpp — the exact fixed-radius search of the FLANN-compatible index (nn_radius):
// ia_index_count_radius, ia_index_query_radius, ia_index_set_workspace, ia_index_radius_stats.
// Kernels in ia_k3r.hip; the argument in DESIGN.md §5 "Radius queries".
//
// Per batch of queries (ia_index.cpp's driver, as for ia_index_query): thresholds, the counting
// scan, per-query offsets; the host reads the per-query candidate totals and cuts the batch into
// sub-batches of consecutive queries whose candidates fit the workspace; per sub-batch the filling
// scan, the exact fp64 verification, the per-query sort and count, and one copy of the staged results.
#include <cmath>
#include <cstring>
#include <limits>

#include "ia_host.h"

using namespace ia_host;

namespace {

constexpr int64_t R_WORKSPACE_DEFAULT = (int64_t)1 << 23;  // candidate entries (12 B each on the device)
constexpr int64_t R_WORKSPACE_MAX = 0xffffff00LL;          // offsets inside a sub-batch are 32-bit

int64_t effective_workspace(const ia_index *x) {
  const int64_t want = x->workspace > 0 ? x->workspace : R_WORKSPACE_DEFAULT;
  return std::min(R_WORKSPACE_MAX, std::max(want, (int64_t)x->n_tiles * IA_TILE));  // one query always fits
}

// count_only: offsets / idx_out / dist_out unused
int radius_run(ia_index *x, const std::string &who, const double *q, int64_t nq, const double *radius, const int64_t *offsets,
               int64_t *idx_out, double *dist_out, int64_t *count_out, bool count_only) {
  if (!x || !q || !radius || !count_out || nq < 0) return fail(IA_EINVAL, who + ": bad arguments");
  if (!count_only) {
    if (!offsets) return fail(IA_EINVAL, who + ": offsets is NULL");
    if (offsets[0] < 0) return fail(IA_EINVAL, who + ": offsets[0] is negative");
    for (int64_t i = 0; i < nq; i++)
      if (offsets[i + 1] < offsets[i]) return fail(IA_EINVAL, who + ": offsets decrease at query " + std::to_string(i));
    if (!idx_out && offsets[nq] > offsets[0]) return fail(IA_EINVAL, who + ": idx_out is NULL for a non-empty layout");
  }
  for (int64_t i = 0; i < nq; i++)
    if (!(radius[i] >= 0.)) return fail(IA_EINVAL, who + ": radius " + std::to_string(i) + " is negative or NaN");
  int rc;
  if ((rc = index_check_queries(x, who, q, nq))) return rc;
  int64_t *stats = x->radius_stats;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (nq == 0) return IA_OK;
  ia_ctx *c = x->ctx;
  HIP_TRY(hipSetDevice(c->dev));
  const int64_t bmax = std::min(nq, IA_INDEX_BATCH), bpad = tile_pad(bmax);
  const int NT = x->n_tiles, nwg = x->nwg;
  if ((rc = index_reserve_batch(x, nq)) || (rc = x->r_rad.ensure((size_t)bmax * 8)) || (rc = x->r_thr.ensure((size_t)bpad * 8)) ||
      (rc = x->r_cnt.ensure((size_t)bpad * nwg * 8)) || (rc = x->r_seg.ensure((size_t)bpad * nwg * 8)) ||
      (rc = x->r_ts.ensure((size_t)bmax * 8)) || (rc = x->r_qoff.ensure((size_t)bmax * 4)) ||
      (rc = x->r_soff.ensure((size_t)(bmax + 1) * 4)) || (rc = x->r_cntq.ensure((size_t)bmax * 8)))
    return rc;
  const int64_t W = effective_workspace(x);
  const int sort_lds = ia_k3r_sort_lds();
  const float4 *db = x->db.as<float4>(), *qf = x->qf.as<float4>();
  const float2 *thr = x->r_thr.as<float2>();
  const uint2 *ts_d = x->r_ts.as<uint2>();
  std::vector<uint2> ts(bmax);
  std::vector<unsigned> qoff(bmax), soff(bmax + 1);
  std::vector<int64_t> cntq(bmax), st_idx;
  std::vector<double> st_dist;
  return index_for_batches(x, q, nq, [&](int64_t b0, int nb, int Mpad, int qtt) -> int {
    HIP_TRY(hipMemcpyAsync(x->r_rad.p, radius + b0, (size_t)nb * 8, hipMemcpyHostToDevice, c->st));
    ia_launch_k3r_thresholds(x->r_rad.as<double>(), x->qn2.as<double>(), x->Rbits.as<unsigned>(), nb, Mpad, x->sc * x->sc,
                             ia_eps_c(2 * x->KH), x->r_thr.as<float2>(), c->st);
    index_scan_tiles(x->KH, 0, qtt, [&](int qt0, int qt) {
      ia_launch_k3r_count(x->KH, qt, db, qf, thr, NT, x->tpw, qt0, nb, nwg, x->r_cnt.as<uint2>(), c->st);
    });
    ia_launch_k3r_offsets(x->r_cnt.as<uint2>(), nb, nwg, count_only, x->r_seg.as<uint2>(), x->r_ts.as<uint2>(), c->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ts.data(), x->r_ts.p, (size_t)nb * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    for (int j0 = 0, j1; j0 < nb; j0 = j1) {
      // the sub-batch [j0, j1): consecutive queries while their candidates fit the workspace
      int64_t sum = 0, stage = 0;
      unsigned max_len = 0;
      bool direct = true;  // every capacity <= its candidates: the staged layout is the caller's (exact CSR)
      for (j1 = j0; j1 < nb && (j1 == j0 || sum + ts[j1].x <= W); j1++) {
        qoff[j1] = (unsigned)sum;
        soff[j1] = (unsigned)stage;
        sum += ts[j1].x;
        max_len = std::max(max_len, ts[j1].x);
        if (!count_only) {
          const int64_t cap = offsets[b0 + j1 + 1] - offsets[b0 + j1];
          stage += std::min<int64_t>(cap, ts[j1].x);
          direct = direct && cap <= (int64_t)ts[j1].x;
          stats[3] += ts[j1].x > (unsigned)sort_lds;
        }
      }
      soff[j1] = (unsigned)stage;
      stats[0] += sum;
      if ((rc = x->r_wr.ensure((size_t)std::max<int64_t>(sum, 1) * 4)) ||
          (rc = x->r_wd.ensure((size_t)std::max<int64_t>(sum, 1) * 8)) ||
          (rc = x->r_sidx.ensure((size_t)std::max<int64_t>(stage, 1) * 8)) ||
          (rc = x->r_sdist.ensure((size_t)std::max<int64_t>(stage, 1) * 8)))
        return rc;
      const unsigned *qoff_d = x->r_qoff.as<unsigned>(), *soff_d = x->r_soff.as<unsigned>();
      HIP_TRY(hipMemcpyAsync(x->r_qoff.as<unsigned>() + j0, &qoff[j0], (size_t)(j1 - j0) * 4, hipMemcpyHostToDevice, c->st));
      HIP_TRY(hipMemcpyAsync(x->r_soff.as<unsigned>() + j0, &soff[j0], (size_t)(j1 - j0 + 1) * 4, hipMemcpyHostToDevice, c->st));
      if (sum > 0) {
        // the query tiles that hold [j0, j1)
        index_scan_tiles(x->KH, j0 / IA_TILE, (j1 - 1) / IA_TILE + 1, [&](int qt0, int qt) {
          ia_launch_k3r_fill(x->KH, qt, count_only, db, qf, thr, NT, x->tpw, qt0, j0, j1, nwg, x->r_seg.as<uint2>(), qoff_d,
                             x->r_wr.as<int>(), c->st);
        });
        ia_launch_k3r_verify(x->pts.as<double>(), x->n, x->d, NT, x->q.as<double>(), x->r_rad.as<double>(), ts_d, qoff_d, j0, j1,
                             max_len, x->r_wr.as<int>(), x->r_wd.as<double>(), c->st);
        stats[2]++;
      }
      ia_launch_k3r_finish(count_only, ts_d, qoff_d, soff_d, j0, j1, x->r_wr.as<int>(), x->r_wd.as<double>(),
                           x->r_sidx.as<int64_t>(), x->r_sdist.as<double>(), x->r_cntq.as<int64_t>(), c->st);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&cntq[j0], x->r_cntq.as<int64_t>() + j0, (size_t)(j1 - j0) * 8, hipMemcpyDeviceToHost, c->st));
      if (stage > 0 && direct) {  // straight into the caller's slots [offsets[j0], offsets[j1])
        HIP_TRY(hipMemcpyAsync(idx_out + offsets[b0 + j0], x->r_sidx.p, (size_t)stage * 8, hipMemcpyDeviceToHost, c->st));
        if (dist_out)
          HIP_TRY(hipMemcpyAsync(dist_out + offsets[b0 + j0], x->r_sdist.p, (size_t)stage * 8, hipMemcpyDeviceToHost, c->st));
      } else if (stage > 0) {
        st_idx.resize(std::max<size_t>(st_idx.size(), stage));
        HIP_TRY(hipMemcpyAsync(st_idx.data(), x->r_sidx.p, (size_t)stage * 8, hipMemcpyDeviceToHost, c->st));
        if (dist_out) {
          st_dist.resize(std::max<size_t>(st_dist.size(), stage));
          HIP_TRY(hipMemcpyAsync(st_dist.data(), x->r_sdist.p, (size_t)stage * 8, hipMemcpyDeviceToHost, c->st));
        }
      }
      HIP_TRY(hipStreamSynchronize(c->st));
      for (int j = j0; j < j1; j++) {
        const int64_t cnt = cntq[j];
        count_out[b0 + j] = cnt;
        stats[1] += cnt;
        if (count_only) continue;
        // the device staged the nearest min(capacity, count); the rest of the capacity is padding
        const int64_t o0 = offsets[b0 + j], cap = offsets[b0 + j + 1] - o0, take = std::min(cap, cnt);
        if (take > 0 && !direct) std::memcpy(idx_out + o0, &st_idx[soff[j]], (size_t)take * 8);
        std::fill(idx_out + o0 + take, idx_out + o0 + cap, (int64_t)-1);
        if (dist_out) {
          if (take > 0 && !direct) std::memcpy(dist_out + o0, &st_dist[soff[j]], (size_t)take * 8);
          std::fill(dist_out + o0 + take, dist_out + o0 + cap, std::numeric_limits<double>::infinity());
        }
      }
    }
    return IA_OK;
  });
}

}  // namespace

extern "C" {

int ia_index_count_radius(ia_index *x, const double *q, int64_t nq, const double *radius, int64_t *count_out) {
  return radius_run(x, "ia_index_count_radius", q, nq, radius, nullptr, nullptr, nullptr, count_out, true);
}

int ia_index_query_radius(ia_index *x, const double *q, int64_t nq, const double *radius, const int64_t *offsets,
                          int64_t *idx_out, double *dist_out, int64_t *count_out) {
  return radius_run(x, "ia_index_query_radius", q, nq, radius, offsets, idx_out, dist_out, count_out, false);
}

int ia_index_set_workspace(ia_index *x, int64_t entries) {
  if (!x || entries < 0) return fail(IA_EINVAL, "ia_index_set_workspace: bad arguments");
  x->workspace = entries;
  return IA_OK;
}

int ia_index_radius_stats(const ia_index *x, int64_t out[4]) {
  if (!x || !out) return fail(IA_EINVAL, "ia_index_radius_stats: bad arguments");
  for (int k = 0; k < 4; k++) out[k] = x->radius_stats[k];
  return IA_OK;
}

}  // extern "C"

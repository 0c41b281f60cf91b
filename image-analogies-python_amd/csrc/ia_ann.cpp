// ia_ann.cpp — the approximate index (include/ia.h ia_kmeans, ia_ann_*): the k-means
// loop (assign on the device, grouping by a host counting sort of the read-back assignment, update
// on the device), the list-major layout and the batched query.  Kernels: ia_ann.hip.
#include <chrono>
#include <cmath>

#include "ia_host.h"

using namespace ia_host;

struct __attribute__((visibility("hidden"))) ia_ann {
  ia_ctx *ctx = nullptr;
  int64_t n = 0;
  int d = 0, L = 0, iters_run = 0;
  DevBuf rows, ids, off, centT;        // list-major rows (n x d), their row indices, L + 1 offsets, centres d x L
  DevBuf q, idx, dist, counters;       // a batch's queries and results; the statistics
  std::vector<double> cent_h;          // L x d
  std::vector<int32_t> off_h, rows_h;  // L + 1 offsets; the row indices, list after list
  unsigned long long qstats[2] = {0, 0};
  double build_ms[4] = {0, 0, 0, 0};
};

namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// what ia_kmeans and ia_ann_build refuse alike, before any GPU call; scalars first
int check_build_args(const std::string &who, const char *lists_name, const ia_ctx *c, const double *pts, int64_t n, int d,
                     int L, int iters) {
  if (n < 1 || d < 1) return fail(IA_EINVAL, who + ": n and d must be >= 1");
  if (d > 167) return fail(IA_EINVAL, who + ": d must be 1..167 (got " + std::to_string(d) + ")");
  if (n > (int64_t)INT32_MAX) return fail(IA_EINVAL, who + ": n must be below 2^31 (int32 row ids)");
  const int64_t lmax = std::min<int64_t>(n, IA_ANN_MAX_LISTS);
  if (L < 1 || L > lmax)
    return fail(IA_EINVAL, who + ": " + lists_name + " must be 1.." + std::to_string(lmax) +
                               " (min(n, IA_ANN_MAX_LISTS); got " + std::to_string(L) + ")");
  if (iters < 0) return fail(IA_EINVAL, who + ": iters must be >= 0 (got " + std::to_string(iters) + ")");
  if (!c || !pts) return fail(IA_EINVAL, who + ": NULL context or rows");
  return IA_OK;
}
// finite, and small enough that no squared distance overflows: 167 terms of (2 * 2^500)^2 stay below 2^1010.  A
// distance of +inf would never enter topk_offer's list (ia_topk.h: its sentinel is (DBL_MAX, INT64_MAX))
int check_finite(const std::string &who, const char *what, const double *v, int64_t rows, int d) {
  for (int64_t i = 0; i < rows; i++)
    for (int f = 0; f < d; f++)
      if (!(std::fabs(v[i * d + f]) <= IA_ANN_MAX_ABS))
        return fail(IA_EINVAL, who + ": " + what + " " + std::to_string(i) +
                                   " holds a value that is not finite or exceeds 2^500 in magnitude (IA_ANN_MAX_ABS)");
  return IA_OK;
}

struct KMeans {  // the device state and the host lists of one k-means run
  DevBuf pts, cent, assign, rows, off;
  std::vector<int32_t> a_h, rows_h, off_h;
  int run = 0;
  double ms[3] = {0, 0, 0};  // assign, grouping, update
};

// lists in ascending row order from the assignment: a counting sort, stable by construction
void group_rows(const std::vector<int32_t> &a, int L, std::vector<int32_t> &off, std::vector<int32_t> &rows) {
  off.assign((size_t)L + 1, 0);
  for (int32_t c : a) off[(size_t)c + 1]++;
  for (int c = 0; c < L; c++) off[(size_t)c + 1] += off[c];
  rows.resize(a.size());
  std::vector<int32_t> at(off.begin(), off.end() - 1);
  for (size_t i = 0; i < a.size(); i++) rows[(size_t)at[a[i]]++] = (int32_t)i;
}

int kmeans_run(ia_ctx *c, const double *pts, int64_t n, int d, int L, int iters, KMeans &km) {
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  if ((rc = km.pts.ensure((size_t)n * d * 8)) || (rc = km.cent.ensure((size_t)L * d * 8)) ||
      (rc = km.assign.ensure((size_t)n * 4)) || (rc = km.rows.ensure((size_t)n * 4)) ||
      (rc = km.off.ensure((size_t)(L + 1) * 4)))
    return rc;
  std::vector<double> c0((size_t)L * d);
  for (int64_t j = 0; j < L; j++) std::copy(pts + (j * n / L) * d, pts + (j * n / L + 1) * d, c0.begin() + j * d);
  HIP_TRY(hipMemcpyAsync(km.pts.p, pts, (size_t)n * d * 8, hipMemcpyHostToDevice, c->st));
  HIP_TRY(hipMemcpyAsync(km.cent.p, c0.data(), (size_t)L * d * 8, hipMemcpyHostToDevice, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));  // c0 leaves scope; the phase clocks start on an idle stream
  km.a_h.resize((size_t)n);
  std::vector<int32_t> prev;
  auto assign = [&]() -> int {
    const double t0 = now_ms();
    ia_launch_ann_assign(km.pts.as<double>(), n, d, km.cent.as<double>(), L, km.assign.as<int32_t>(), c->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(km.a_h.data(), km.assign.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    km.ms[0] += now_ms() - t0;
    return IA_OK;
  };
  auto group = [&]() -> int {
    const double t0 = now_ms();
    group_rows(km.a_h, L, km.off_h, km.rows_h);
    HIP_TRY(hipMemcpyAsync(km.rows.p, km.rows_h.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(km.off.p, km.off_h.data(), (size_t)(L + 1) * 4, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    km.ms[1] += now_ms() - t0;
    return IA_OK;
  };
  bool settled = false;  // the last assignment belongs to the current centres
  for (int it = 0; it < iters; it++) {
    if ((rc = assign())) return rc;
    if (it > 0 && km.a_h == prev) {  // the centres did not move the rows: assign(C) is this assignment
      settled = true;
      break;
    }
    if ((rc = group())) return rc;
    const double t0 = now_ms();
    ia_launch_ann_update(km.pts.as<double>(), d, km.rows.as<int32_t>(), km.off.as<int32_t>(), L, km.cent.as<double>(), c->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->st));
    km.ms[2] += now_ms() - t0;
    prev = km.a_h;
    km.run++;
  }
  if (!settled && (rc = assign())) return rc;
  return group();
}

}  // namespace

extern "C" {

int ia_kmeans(ia_ctx *c, const double *pts, int64_t n, int d, int k, int iters, double *centers_out, int32_t *assign_out,
              int *iters_run) {
  int rc;
  if ((rc = check_build_args("ia_kmeans", "k", c, pts, n, d, k, iters))) return rc;
  if (!centers_out) return fail(IA_EINVAL, "ia_kmeans: NULL centers_out");
  if ((rc = check_finite("ia_kmeans", "row", pts, n, d))) return rc;
  KMeans km;
  rc = kmeans_run(c, pts, n, d, k, iters, km);
  if (rc == IA_OK) {
    hipError_t e = hipMemcpyAsync(centers_out, km.cent.p, (size_t)k * d * 8, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) rc = fail(IA_EHIP, std::string("ia_kmeans: ") + hipGetErrorString(e));
  } else {
    hipStreamSynchronize(c->st);  // nothing in flight when the buffers go
  }
  if (rc) return rc;
  if (assign_out) std::copy(km.a_h.begin(), km.a_h.end(), assign_out);
  if (iters_run) *iters_run = km.run;
  return IA_OK;
}

int ia_ann_build(ia_ctx *c, const double *pts, int64_t n, int d, int n_lists, int iters, ia_ann **out) {
  int rc;
  if ((rc = check_build_args("ia_ann_build", "n_lists", c, pts, n, d, n_lists, iters))) return rc;
  if (!out) return fail(IA_EINVAL, "ia_ann_build: NULL out");
  if ((rc = check_finite("ia_ann_build", "row", pts, n, d))) return rc;
  const int L = n_lists;
  KMeans km;
  ia_ann *a = new ia_ann();
  a->ctx = c;
  a->n = n;
  a->d = d;
  a->L = L;
  a->cent_h.resize((size_t)L * d);
  auto finish = [&]() -> int {
    int r;
    if ((r = kmeans_run(c, pts, n, d, L, iters, km))) return r;
    if ((r = a->rows.ensure((size_t)n * d * 8)) || (r = a->centT.ensure((size_t)L * d * 8)) || (r = a->counters.ensure(32)))
      return r;
    const double t0 = now_ms();
    ia_launch_ann_permute(km.pts.as<double>(), d, km.rows.as<int32_t>(), n, a->rows.as<double>(), c->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->st));
    a->build_ms[3] = now_ms() - t0;
    HIP_TRY(hipMemcpyAsync(a->cent_h.data(), km.cent.p, (size_t)L * d * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    std::vector<double> t((size_t)L * d);
    for (int j = 0; j < L; j++)
      for (int f = 0; f < d; f++) t[(size_t)f * L + j] = a->cent_h[(size_t)j * d + f];
    HIP_TRY(hipMemcpyAsync(a->centT.p, t.data(), (size_t)L * d * 8, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return IA_OK;
  };
  if ((rc = finish())) {
    hipStreamSynchronize(c->st);
    delete a;
    return rc;
  }
  a->ids = std::move(km.rows);  // the original-order copy of the rows (km.pts) goes with km
  a->off = std::move(km.off);
  a->off_h = std::move(km.off_h);
  a->rows_h = std::move(km.rows_h);
  a->iters_run = km.run;
  for (int i = 0; i < 3; i++) a->build_ms[i] = km.ms[i];
  *out = a;
  return IA_OK;
}

int ia_ann_lists(const ia_ann *a, double *centers_out, int64_t *sizes_out, int32_t *rows_out) {
  if (!a) return fail(IA_EINVAL, "ia_ann_lists: NULL index");
  if (centers_out) std::copy(a->cent_h.begin(), a->cent_h.end(), centers_out);
  if (sizes_out)
    for (int c = 0; c < a->L; c++) sizes_out[c] = (int64_t)a->off_h[(size_t)c + 1] - a->off_h[c];
  if (rows_out) std::copy(a->rows_h.begin(), a->rows_h.end(), rows_out);
  return IA_OK;
}

int ia_ann_query(ia_ann *a, const double *q, int64_t nq, int k, int checks, int64_t *idx_out, double *dist_out) {
  if (k < 1 || k > IA_KNN_MAX)
    return fail(IA_EINVAL, "ia_ann_query: k must be 1..min(n, IA_KNN_MAX = " + std::to_string(IA_KNN_MAX) + ") (got " +
                               std::to_string(k) + ")");
  if (checks != -1 && checks < 1)
    return fail(IA_EINVAL, "ia_ann_query: checks must be -1 (every row) or >= 1 (got " + std::to_string(checks) + ")");
  if (!a || !q || !idx_out || nq < 0) return fail(IA_EINVAL, "ia_ann_query: NULL index, queries or idx_out, or nq < 0");
  if (k > a->n)
    return fail(IA_EINVAL, "ia_ann_query: k must be 1.." + std::to_string(std::min<int64_t>(IA_KNN_MAX, a->n)) +
                               " (IA_KNN_MAX and the index's rows; got " + std::to_string(k) + ")");
  int rc;
  if ((rc = check_finite("ia_ann_query", "query", q, nq, a->d))) return rc;
  a->qstats[0] = a->qstats[1] = 0;
  if (nq == 0) return IA_OK;
  ia_ctx *c = a->ctx;
  HIP_TRY(hipSetDevice(c->dev));
  const int need = checks == -1 ? (int)a->n : (int)std::min<int64_t>(a->n, std::max(checks, k));
  const int64_t bmax = std::min(nq, IA_INDEX_BATCH);
  if ((rc = a->q.ensure((size_t)bmax * a->d * 8)) || (rc = a->idx.ensure((size_t)bmax * k * 8)) ||
      (rc = a->dist.ensure((size_t)bmax * k * 8)))
    return rc;
  HIP_TRY(hipMemsetAsync(a->counters.p, 0, 32, c->st));
  for (int64_t b0 = 0; b0 < nq; b0 += IA_INDEX_BATCH) {
    const int nb = (int)std::min(IA_INDEX_BATCH, nq - b0);
    HIP_TRY(hipMemcpyAsync(a->q.p, q + b0 * a->d, (size_t)nb * a->d * 8, hipMemcpyHostToDevice, c->st));
    ia_launch_ann_query(a->rows.as<double>(), a->ids.as<int32_t>(), a->off.as<int32_t>(), a->centT.as<double>(), a->L, a->d,
                        a->q.as<double>(), nb, k, need, a->idx.as<int64_t>(), a->dist.as<double>(),
                        a->counters.as<unsigned long long>(), c->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(idx_out + b0 * k, a->idx.p, (size_t)nb * k * 8, hipMemcpyDeviceToHost, c->st));
    if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out + b0 * k, a->dist.p, (size_t)nb * k * 8, hipMemcpyDeviceToHost, c->st));
    if (b0 + nb == nq) HIP_TRY(hipMemcpyAsync(a->qstats, a->counters.p, 16, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
  }
  return IA_OK;
}

int ia_ann_stats(const ia_ann *a, int64_t out[3]) {
  if (!a || !out) return fail(IA_EINVAL, "ia_ann_stats: NULL argument");
  out[0] = (int64_t)a->qstats[0];
  out[1] = (int64_t)a->qstats[1];
  out[2] = a->iters_run;
  return IA_OK;
}

int ia_ann_build_ms(const ia_ann *a, double out[4]) {
  if (!a || !out) return fail(IA_EINVAL, "ia_ann_build_ms: NULL argument");
  for (int i = 0; i < 4; i++) out[i] = a->build_ms[i];
  return IA_OK;
}

void ia_ann_destroy(ia_ann *a) {
  if (!a) return;
  hipSetDevice(a->ctx->dev);
  hipStreamSynchronize(a->ctx->st);
  delete a;
}

}  // extern "C"

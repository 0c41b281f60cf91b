// ia_index.cpp — the entry points beside the level path: GPU preprocessing (Gaussian pyramid,
// colour matrices), the K3h microbenchmark, and the FLANN-compatible exact index with its
// batched coherence search.
#include <cmath>

#include "ia_host.h"

using namespace ia_host;

// ------------------------------------------------------------------------------------------
// the index's query driver (declared in ia_host.h): what ia_index_query, ia_index_query_knn and
// the radius search (ia_index_radius.cpp) do alike
// ------------------------------------------------------------------------------------------
namespace ia_host {

int index_check_queries(const ia_index *x, const std::string &who, const double *q, int64_t nq) {
  for (int64_t i = 0; i < nq; i++)
    for (int f = 0; f < x->d; f++)
      if (!(std::fabs((q[i * x->d + f] - x->mu_h[f]) * x->sc) <= 0x1p100))
        return fail(IA_EINVAL, who + ": query " + std::to_string(i) +
                                   " is not finite or farther than 2^100 x the rows' spread from their mean");
  return IA_OK;
}

int index_reserve_batch(ia_index *x, int64_t nq) {
  const int64_t bmax = std::min(nq, IA_INDEX_BATCH), bpad = tile_pad(bmax);
  int rc;
  if ((rc = x->q.ensure((size_t)bmax * x->d * 8)) || (rc = x->qn2.ensure((size_t)bpad * 8)) ||
      (rc = x->qf.ensure((size_t)bpad * 2 * x->KH * 4)))
    return rc;
  return IA_OK;
}

int index_for_batches(ia_index *x, const double *q, int64_t nq, const std::function<int(int64_t, int, int, int)> &body) {
  ia_ctx *c = x->ctx;
  for (int64_t b0 = 0; b0 < nq; b0 += IA_INDEX_BATCH) {
    const int nb = (int)std::min(IA_INDEX_BATCH, nq - b0), Mpad = (int)tile_pad(nb);
    if (q) HIP_TRY(hipMemcpyAsync(x->q.p, q + b0 * x->d, (size_t)nb * x->d * 8, hipMemcpyHostToDevice, c->st));
    else  // the index's own rows b0 .. b0 + nb (ia_index_similarity)
      HIP_TRY(hipMemcpyAsync(x->q.p, x->pts.as<double>() + b0 * x->d, (size_t)nb * x->d * 8, hipMemcpyDeviceToDevice, c->st));
    ia_launch_dense_query(x->KH, x->q.as<double>(), nb, x->d, Mpad, x->mu.as<double>(), x->sc, x->qn2.as<double>(),
                          x->qf.as<float>(), c->st);
    if (int rc = body(b0, nb, Mpad, Mpad / IA_TILE)) return rc;
  }
  return IA_OK;
}

}  // namespace ia_host

// the top-2 scan of a batch's nb queries (qtt query tiles) into x->rec / x->recT
static void index_scan_top2(ia_index *x, int nb, int qtt) {
  index_scan_tiles(x->KH, 0, qtt, [&](int qt0, int qt) {
    ia_launch_k3(x->KH, qt, x->db.as<float4>(), x->qf.as<float4>(), x->n_tiles, x->tpw, qt0, nb, x->nwg, 0, x->n_tiles,
                 x->rec.as<float4>(), x->recT.as<float>(), x->ctx->st);
  });
}

extern "C" {

// ------------------------------------------------------------------------------------------
// GPU preprocessing: Gaussian pyramid reductions and 3x3 colour matrices
// ------------------------------------------------------------------------------------------
int ia_gaussian_pyramid(ia_ctx *c, const double *img, int h, int w, int ch, int n_reduce, const double *weights7,
                        double *out, int mem) {
  if (!c || !img || !weights7 || (n_reduce > 0 && !out) || h < 1 || w < 1 || ch < 1 || ch > 4 || n_reduce < 0)
    return fail(IA_EINVAL, "ia_gaussian_pyramid: bad arguments");
  if (mem != IA_MEM_HOST && mem != IA_MEM_DEVICE) return fail(IA_EINVAL, "ia_gaussian_pyramid: bad mem kind");
  if (n_reduce == 0) return IA_OK;
  HIP_TRY(hipSetDevice(c->dev));
  const size_t n0 = (size_t)h * w * ch;
  size_t tot = 0;  // doubles of all reduced levels
  {
    int hh = h, ww = w;
    for (int k = 0; k < n_reduce; k++) {
      hh = (hh + 1) / 2;
      ww = (ww + 1) / 2;
      tot += (size_t)hh * ww * ch;
    }
  }
  int rc;
  if ((rc = c->py_in.ensure(n0 * 8)) || (rc = c->py_tmp.ensure(n0 * 8)) || (rc = c->py_sm.ensure(n0 * 8)) ||
      (rc = c->py_mm.ensure(2 * 256 * 8)) || (rc = c->py_out.ensure(std::max<size_t>(tot, 1) * 8)))
    return rc;
  const double *din = img;
  if (mem == IA_MEM_HOST) {
    HIP_TRY(hipMemcpyAsync(c->py_in.p, img, n0 * 8, hipMemcpyHostToDevice, c->st));
    din = c->py_in.as<double>();
  }
  double *dout = mem == IA_MEM_DEVICE ? out : c->py_out.as<double>();
  int hh = h, ww = w;
  const double *src = din;
  double *dst = dout;
  for (int k = 0; k < n_reduce; k++) {
    ia_launch_pyramid_reduce(src, dst, c->py_tmp.as<double>(), c->py_sm.as<double>(), c->py_mm.as<double>(), hh, ww, ch,
                             weights7, c->st);
    src = dst;
    hh = (hh + 1) / 2;
    ww = (ww + 1) / 2;
    dst += (size_t)hh * ww * ch;
  }
  HIP_TRY(hipGetLastError());
  if (mem == IA_MEM_HOST) HIP_TRY(hipMemcpyAsync(out, dout, tot * 8, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  return IA_OK;
}

int ia_color_matrix(ia_ctx *c, const double *in, int64_t npx, const double *M9, double *out, int mem) {
  if (!c || !in || !M9 || !out || npx < 0) return fail(IA_EINVAL, "ia_color_matrix: bad arguments");
  if (mem != IA_MEM_HOST && mem != IA_MEM_DEVICE) return fail(IA_EINVAL, "ia_color_matrix: bad mem kind");
  if (npx == 0) return IA_OK;
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  if ((rc = c->py_mm.ensure(2 * 256 * 8))) return rc;
  HIP_TRY(hipMemcpyAsync(c->py_mm.p, M9, 9 * 8, hipMemcpyHostToDevice, c->st));
  const double *din = in;
  double *dout = out;
  if (mem == IA_MEM_HOST) {
    if ((rc = c->py_in.ensure((size_t)npx * 24)) || (rc = c->py_out.ensure((size_t)npx * 24))) return rc;
    HIP_TRY(hipMemcpyAsync(c->py_in.p, in, (size_t)npx * 24, hipMemcpyHostToDevice, c->st));
    din = c->py_in.as<double>();
    dout = c->py_out.as<double>();
  }
  ia_launch_color3(din, dout, npx, c->py_mm.as<double>(), c->st);
  HIP_TRY(hipGetLastError());
  if (mem == IA_MEM_HOST) HIP_TRY(hipMemcpyAsync(out, dout, (size_t)npx * 24, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  return IA_OK;
}

// ------------------------------------------------------------------------------------------
// K3h microbenchmark (kernel tuning): the split-f16 distance scan alone on random operands
// ------------------------------------------------------------------------------------------
int ia_k3_microbench(ia_ctx *c, int64_t n_rows, int M, int reps, double *us_per_launch) {
  if (!c || n_rows < 1 || M < 1 || reps < 1 || !us_per_launch) return fail(IA_EINVAL, "ia_k3_microbench: bad arguments");
  const int KS = ia_ks_for(1), qtmax = ia_k3h_qtmax(KS);
  const int qt = (M + IA_TILE - 1) / IA_TILE;
  if (qt > qtmax) return fail(IA_EINVAL, "ia_k3_microbench: M exceeds one launch");
  if (n_rows >= (int64_t)INT32_MAX) return fail(IA_EINVAL, "ia_k3_microbench: n_rows exceeds int32 row ids");
  HIP_TRY(hipSetDevice(c->dev));
  const int n_tiles = (int)((n_rows + IA_TILE - 1) / IA_TILE);
  const int tpw = std::max(IA_WGH / IA_WAVE, (n_tiles + IA_NWG_H - 1) / IA_NWG_H);
  const int nwg = (n_tiles + tpw - 1) / tpw;
  const size_t row_bytes = (size_t)16 * KS * 4;
  int rc;
  if ((rc = c->db.ensure((size_t)n_tiles * IA_TILE * row_bytes)) || (rc = c->qf.ensure((size_t)qt * IA_TILE * row_bytes)) ||
      (rc = c->rec.ensure((size_t)M * nwg * 16)) || (rc = c->recT.ensure((size_t)M * nwg * 4)))
    return rc;
  ia_launch_fill_random_f16(c->db.p, (int64_t)n_tiles * IA_TILE * row_bytes / 2, 12345u, c->st);
  ia_launch_fill_random_f16(c->qf.p, (int64_t)qt * IA_TILE * row_bytes / 2, 777u, c->st);
  auto launch = [&]() {
    ia_launch_k3h(KS, qt, c->db.p, c->qf.p, n_tiles, tpw, 0, M, nwg, 0, n_tiles, c->rec.as<float4>(), c->recT.as<float>(),
                  c->st);
  };
  for (int i = 0; i < 3; i++) launch();
  HIP_TRY(hipEventRecord(c->lv0, c->st));
  for (int i = 0; i < reps; i++) launch();
  HIP_TRY(hipEventRecord(c->lv1, c->st));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->lv0, c->lv1));
  *us_per_launch = 1e3 * ms / reps;
  return IA_OK;
}

// ------------------------------------------------------------------------------------------
// FLANN-compatible exact index (algorithms.py:56,69,74)
// ------------------------------------------------------------------------------------------
int ia_index_build(ia_ctx *c, const double *pts, int64_t n, int d, ia_index **out) {
  if (!c || !pts || !out || n < 1 || d < 1) return fail(IA_EINVAL, "ia_index_build: bad arguments");
  const int KH = kh_for(d + 1);
  if (KH < 0) return fail(IA_EINVAL, "ia_index_build: d must be <= 167");
  if (n >= (int64_t)INT32_MAX) return fail(IA_EINVAL, "ia_index_build: n exceeds int32 row ids");
  HIP_TRY(hipSetDevice(c->dev));
  ia_index *x = new ia_index();
  x->ctx = c;
  x->n = n;
  x->d = d;
  x->KH = KH;
  x->n_tiles = (int)((n + IA_TILE - 1) / IA_TILE);
  dense_geometry(x->n_tiles, &x->tpw, &x->nwg);
  // column means (host, fixed order): centre the fp32 copy, shrinking the MFMA error bound
  std::vector<double> mu(d, 0.);
  for (int64_t i = 0; i < n; i++)
    for (int f = 0; f < d; f++) mu[f] += pts[i * d + f];
  for (int f = 0; f < d; f++) mu[f] /= (double)n;
  double amax = 0.;  // the largest centred |value|: the prescale
  for (int64_t i = 0; i < n; i++)
    for (int f = 0; f < d; f++) amax = std::fmax(amax, std::fabs(pts[i * d + f] - mu[f]));
  if (!std::isfinite(amax)) {  // (fmax drops a NaN: the means carry it)
    delete x;
    return fail(IA_EINVAL, "ia_index_build: rows must be finite (and their column sums too)");
  }
  for (int f = 0; f < d; f++)
    if (!std::isfinite(mu[f])) {
      delete x;
      return fail(IA_EINVAL, "ia_index_build: rows must be finite (and their column sums too)");
    }
  x->sc = dense_prescale(amax);
  x->mu_h = mu;
  int rc;
  if ((rc = x->pts.ensure((size_t)n * d * 8)) || (rc = x->db.ensure((size_t)x->n_tiles * IA_TILE * 2 * KH * 4)) ||
      (rc = x->mu.ensure((size_t)d * 8)) || (rc = x->Rbits.ensure(4)) || (rc = x->counters.ensure(32))) {
    delete x;
    return rc;
  }
  hipMemcpyAsync(x->pts.p, pts, (size_t)n * d * 8, hipMemcpyHostToDevice, c->st);
  hipMemcpyAsync(x->mu.p, mu.data(), (size_t)d * 8, hipMemcpyHostToDevice, c->st);
  hipMemsetAsync(x->Rbits.p, 0, 4, c->st);
  ia_launch_dense_db(KH, x->pts.as<double>(), n, d, x->n_tiles, x->mu.as<double>(), x->sc, x->db.as<float4>(),
                     x->Rbits.as<unsigned>(), c->st);
  hipError_t e = hipStreamSynchronize(c->st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    ia_index_destroy(x);
    return fail(IA_EHIP, std::string("ia_index_build: ") + hipGetErrorString(e));
  }
  *out = x;
  return IA_OK;
}

int ia_index_query(ia_index *x, const double *q, int64_t nq, int64_t *idx_out, double *dist_out) {
  if (!x || !q || !idx_out || nq < 0) return fail(IA_EINVAL, "ia_index_query: bad arguments");
  if (nq == 0) return IA_OK;
  ia_ctx *c = x->ctx;
  int rc;
  if ((rc = index_check_queries(x, "ia_index_query", q, nq))) return rc;
  HIP_TRY(hipSetDevice(c->dev));
  const int64_t bmax = std::min(nq, IA_INDEX_BATCH);
  if ((rc = index_reserve_batch(x, nq)) || (rc = x->rec.ensure((size_t)bmax * x->nwg * 16)) ||
      (rc = x->recT.ensure((size_t)bmax * x->nwg * 4)) ||
      (rc = x->idx.ensure((size_t)bmax * 8)) || (rc = x->dist.ensure((size_t)bmax * 8)))
    return rc;
  HIP_TRY(hipMemsetAsync(x->counters.p, 0, 32, c->st));
  const MergeArgs ma = index_merge_args(x);
  return index_for_batches(x, q, nq, [&](int64_t b0, int nb, int, int qtt) -> int {
    index_scan_top2(x, nb, qtt);
    ia_launch_merge_dense(ma, x->pts.as<double>(), x->d, x->q.as<double>(), nb, x->sc * x->sc, x->idx.as<int64_t>(),
                          x->dist.as<double>(), c->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(idx_out + b0, x->idx.p, (size_t)nb * 8, hipMemcpyDeviceToHost, c->st));
    if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out + b0, x->dist.p, (size_t)nb * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return IA_OK;
  });
}

// nn_index(q, k): ia_index_query's batches and scans, merged by k_merge_dense_knn (ia_topk.h)
int ia_index_query_knn(ia_index *x, const double *q, int64_t nq, int k, int64_t *idx_out, double *dist_out) {
  if (!x || !q || !idx_out || nq < 0) return fail(IA_EINVAL, "ia_index_query_knn: bad arguments");
  if (k < 1 || k > IA_KNN_MAX || k > x->n)
    return fail(IA_EINVAL, "ia_index_query_knn: k must be 1.." + std::to_string(std::min<int64_t>(IA_KNN_MAX, x->n)) +
                               " (IA_KNN_MAX and the index's rows)");
  int rc;
  if ((rc = index_check_queries(x, "ia_index_query_knn", q, nq))) return rc;
  x->knn_stats[0] = x->knn_stats[1] = 0;
  if (nq == 0) return IA_OK;
  ia_ctx *c = x->ctx;
  HIP_TRY(hipSetDevice(c->dev));
  const int64_t bmax = std::min(nq, IA_INDEX_BATCH);
  if ((rc = index_reserve_batch(x, nq)) || (rc = x->rec.ensure((size_t)bmax * x->nwg * 16)) ||
      (rc = x->recT.ensure((size_t)bmax * x->nwg * 4)) ||
      (rc = x->idx.ensure((size_t)bmax * k * 8)) || (rc = x->dist.ensure((size_t)bmax * k * 8)))
    return rc;
  HIP_TRY(hipMemsetAsync(x->counters.p, 0, 32, c->st));
  const MergeArgs ma = index_merge_args(x);
  return index_for_batches(x, q, nq, [&](int64_t b0, int nb, int, int qtt) -> int {
    index_scan_top2(x, nb, qtt);
    ia_launch_merge_dense_knn(ma, x->pts.as<double>(), x->d, x->q.as<double>(), nb, k, x->sc * x->sc, x->idx.as<int64_t>(),
                              x->dist.as<double>(), x->counters.as<unsigned long long>(), c->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(idx_out + b0 * k, x->idx.p, (size_t)nb * k * 8, hipMemcpyDeviceToHost, c->st));
    if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out + b0 * k, x->dist.p, (size_t)nb * k * 8, hipMemcpyDeviceToHost, c->st));
    if (b0 + nb == nq)  // the sums over every batch, with the last results
      HIP_TRY(hipMemcpyAsync(x->knn_stats, x->counters.p, 16, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return IA_OK;
  });
}

int ia_index_knn_stats(const ia_index *x, int64_t out[2]) {
  if (!x || !out) return fail(IA_EINVAL, "ia_index_knn_stats: bad arguments");
  out[0] = (int64_t)x->knn_stats[0];
  out[1] = (int64_t)x->knn_stats[1];
  return IA_OK;
}

// the similarity sets of k-coherence search: the (K + 1)-NN of the index's own rows (the k-NN call's
// batches, scans, merge and buffers), each row's own entry deleted on the host
int ia_index_similarity(ia_index *x, int K, int32_t *sim_out) {
  if (!x || !sim_out) return fail(IA_EINVAL, "ia_index_similarity: NULL argument");
  if (K < 1 || K > IA_KCOH_MAX || K > x->n - 1)
    return fail(IA_EINVAL, "ia_index_similarity: K must be 1.." + std::to_string(std::min<int64_t>(IA_KCOH_MAX, x->n - 1)) +
                               " (IA_KCOH_MAX and the index's rows - 1)");
  ia_ctx *c = x->ctx;
  HIP_TRY(hipSetDevice(c->dev));
  const int k = K + 1;
  const int64_t nq = x->n, bmax = std::min(nq, IA_INDEX_BATCH);
  int rc;
  if ((rc = index_reserve_batch(x, nq)) || (rc = x->rec.ensure((size_t)bmax * x->nwg * 16)) ||
      (rc = x->recT.ensure((size_t)bmax * x->nwg * 4)) ||
      (rc = x->idx.ensure((size_t)bmax * k * 8)) || (rc = x->dist.ensure((size_t)bmax * k * 8)))
    return rc;
  HIP_TRY(hipMemsetAsync(x->counters.p, 0, 32, c->st));
  const MergeArgs ma = index_merge_args(x);
  std::vector<int64_t> nn((size_t)bmax * k);
  return index_for_batches(x, nullptr, nq, [&](int64_t b0, int nb, int, int qtt) -> int {
    index_scan_top2(x, nb, qtt);
    ia_launch_merge_dense_knn(ma, x->pts.as<double>(), x->d, x->q.as<double>(), nb, k, x->sc * x->sc, x->idx.as<int64_t>(),
                              x->dist.as<double>(), x->counters.as<unsigned long long>(), c->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(nn.data(), x->idx.p, (size_t)nb * k * 8, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    for (int i = 0; i < nb; i++) {
      int32_t *o = sim_out + (b0 + i) * K;
      int n_out = 0;
      for (int j = 0; j < k && n_out < K; j++)
        if (nn[(size_t)i * k + j] != b0 + i) o[n_out++] = (int32_t)nn[(size_t)i * k + j];
    }
    return IA_OK;
  });
}

int ia_coherence_batch(ia_index *x, const double *q, int64_t nq, const int32_t *px, const int32_t *s, const int32_t *im,
                       int64_t n_s, int a_h, int a_w, int bp_w, int pad, int32_t *p_out, int32_t *img_out, int32_t *rstar_out) {
  if (!x || nq < 0 || n_s < 0 || a_h < 1 || a_w < 1 || bp_w < 1 || pad < 0 || (pad + 1) * (2 * pad + 1) > 64)
    return fail(IA_EINVAL, "ia_coherence_batch: bad arguments (pad must be 0..4)");
  if (nq == 0) return IA_OK;
  if (!q || !px || !p_out || !img_out || !rstar_out || (n_s > 0 && (!s || !im)))
    return fail(IA_EINVAL, "ia_coherence_batch: NULL buffer");
  ia_ctx *c = x->ctx;
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  if ((rc = x->q.ensure((size_t)nq * x->d * 8)) || (rc = x->cpx.ensure((size_t)nq * 8)) ||
      (rc = x->cs.ensure((size_t)std::max<int64_t>(n_s, 1) * 8)) || (rc = x->cim.ensure((size_t)std::max<int64_t>(n_s, 1) * 4)) ||
      (rc = x->cout.ensure((size_t)nq * 20 + 16)))
    return rc;
  int32_t *dp = x->cout.as<int32_t>(), *di = dp + 2 * nq, *dr = di + nq;
  unsigned *derr = reinterpret_cast<unsigned *>(dr + 2 * nq);
  HIP_TRY(hipMemcpyAsync(x->q.p, q, (size_t)nq * x->d * 8, hipMemcpyHostToDevice, c->st));
  HIP_TRY(hipMemcpyAsync(x->cpx.p, px, (size_t)nq * 8, hipMemcpyHostToDevice, c->st));
  if (n_s > 0) {
    HIP_TRY(hipMemcpyAsync(x->cs.p, s, (size_t)n_s * 8, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(x->cim.p, im, (size_t)n_s * 4, hipMemcpyHostToDevice, c->st));
  }
  HIP_TRY(hipMemsetAsync(derr, 0, 4, c->st));
  ia_launch_coherence_batch(x->pts.as<double>(), x->n, x->d, x->q.as<double>(), nq, x->cpx.as<int32_t>(), x->cs.as<int32_t>(),
                            x->cim.as<int32_t>(), n_s, a_h, a_w, bp_w, pad, dp, di, dr, derr, c->st);
  HIP_TRY(hipGetLastError());
  unsigned err = 0;
  HIP_TRY(hipMemcpyAsync(p_out, dp, (size_t)nq * 8, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipMemcpyAsync(img_out, di, (size_t)nq * 4, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipMemcpyAsync(rstar_out, dr, (size_t)nq * 8, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipMemcpyAsync(&err, derr, 4, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  if (err & 1u) return fail(IA_EINVAL, "ia_coherence_batch: a causal neighbour lies beyond the n_s entries of s / im");
  if (err & 2u) return fail(IA_EINVAL, "ia_coherence_batch: a coherence candidate's DB row lies beyond the index");
  return IA_OK;
}

void ia_index_destroy(ia_index *x) {
  if (!x) return;
  hipSetDevice(x->ctx->dev);
  hipStreamSynchronize(x->ctx->st);
  delete x;  // frees its buffers
}

}  // extern "C"

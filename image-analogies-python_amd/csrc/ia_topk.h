// ia_topk.h — the certified exact k nearest rows of one query from the scan's records (the
// index's k-NN merge, ia_dense.hip k_merge_dense_knn): certified_winner's argument (ia_certify.h)
// with "the best" replaced by "the k-th best" (DESIGN.md §5).  One wave per query, k <= 64: lane
// j holds the j-th smallest (distance, row) pair seen so far.
#pragma once
#include "ia_dev.h"

__device__ __forceinline__ bool di_lt(double da, int64_t ia, double db, int64_t ib) {
  return da < db || (da == db && ia < ib);
}

// the wave's sorted list: (md, mi) of lane j is its j-th entry, (DBL_MAX, INT64_MAX) when empty
// and on every lane >= k.  Inserts the wave-uniform pair (nd, ni), nd finite; a pair the list
// already holds is a no-op (a chunk rescan meets the rows that were reranked before it).
__device__ __forceinline__ void topk_insert(double &md, int64_t &mi, double nd, int64_t ni, int k) {
  const int lane = threadIdx.x & 63;
  if (__ballot(md == nd && mi == ni)) return;
  const int pos = __popcll(__ballot(di_lt(md, mi, nd, ni)));  // sorted: the smaller entries are lanes 0..pos-1
  const double ud = __shfl_up(md, 1, 64);
  const int64_t ui = __shfl_up(mi, 1, 64);
  if (lane > pos) {
    md = ud;
    mi = ui;
  } else if (lane == pos) {
    md = nd;
    mi = ni;
  }
  if (lane >= k) {
    md = DBL_MAX;
    mi = INT64_MAX;
  }
}
// one candidate per lane (has: this lane brings one): those below the list's k-th entry are
// inserted one by one off a ballot; every insert lowers the k-th entry and thins the rest
__device__ __forceinline__ void topk_offer(double &md, int64_t &mi, double cd, int64_t ci, bool has, int k) {
  const int lane = threadIdx.x & 63;
  for (;;) {
    const double kd = __shfl(md, k - 1, 64);
    const int64_t ki = __shfl(mi, k - 1, 64);
    has = has && di_lt(cd, ci, kd, ki);
    const unsigned long long mask = __ballot(has);
    if (!mask) break;
    const int j = __ffsll((long long)mask) - 1;
    topk_insert(md, mi, __shfl(cd, j, 64), __shfl(ci, j, 64), k);
    has = has && lane != j;
  }
}

// fp32 -> unsigned with the same order (negative values below positive ones)
__device__ __forceinline__ unsigned f32_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u >> 31) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float f32_unkey(unsigned key) {
  return __uint_as_float((key >> 31) ? key & 0x7fffffffu : ~key);
}

// The k rows of smallest (exact distance, row) of query m, ascending, on lanes 0..k-1 of (md, mi).
// RPL records per lane (nwg <= 64 RPL); dist(row) is the exact distance in the caller's units and
// dist() * dsc is in the units of the scan's values, as for certified_winner.  The dense scan's
// records only (contiguous chunks, no pruning).  n_exact: rows whose exact distance this lane
// computed; n_rescan (wave-uniform): chunks rescanned.
template <int RPL = IA_WG_TARGET / IA_WAVE, class DistFn>
__device__ void certified_topk(const MergeArgs &a, int m, int k, DistFn &&dist, double dsc, double &md, int64_t &mi,
                               unsigned long long &n_exact, unsigned long long &n_rescan) {
  const int lane = threadIdx.x & 63;
  const float4 *rr = a.rec + (int64_t)m * a.nwg;
  const float *rT = a.recT + (int64_t)m * a.nwg;
  // every record load at once (clamped index), masked afterwards; a listed entry counts when it
  // names a real row (padding rows and never-set entries do not)
  float v1[RPL], v2[RPL], tt[RPL];
  unsigned key1[RPL], key2[RPL];
  unsigned listed = 0;  // bit 2j: record j's best is a real row, bit 2j+1: its runner-up
#pragma unroll
  for (int j = 0; j < RPL; j++) {
    const int w = min(lane + IA_WAVE * j, a.nwg - 1);
    const float4 x = rr[w];
    const float t = rT[w];
    const bool ok = lane + IA_WAVE * j < a.nwg;
    const int r1 = __float_as_int(x.y), r2 = __float_as_int(x.w);
    const bool ok1 = ok && r1 >= 0 && r1 < a.NA, ok2 = ok && r2 >= 0 && r2 < a.NA;
    v1[j] = x.x;
    v2[j] = x.z;
    tt[j] = t;
    key1[j] = ok1 ? f32_key(x.x) : 0xffffffffu;
    key2[j] = ok2 ? f32_key(x.z) : 0xffffffffu;
    listed |= (ok1 ? 1u : 0u) << (2 * j) | (ok2 ? 1u : 0u) << (2 * j + 1);
  }
  const double R = (double)__uint_as_float(*a.Rbits);
  const double qn2 = a.qn2[m];
  const double qn = sqrt(qn2);
  const double eps = merge_eps(a, R, qn);

  // a_k: the k-th smallest listed MFMA value, by bisection on the ordered keys (the largest key
  // with fewer than k listed keys below it); +inf when fewer than k rows are listed
  unsigned long long n_listed = 0;
#pragma unroll
  for (int b = 0; b < 2 * RPL; b++) n_listed += __popcll(__ballot((listed >> b) & 1));
  double thr = INFINITY;
  if (n_listed >= (unsigned long long)k) {
    unsigned ak = 0;
    for (int bit = 31; bit >= 0; bit--) {
      const unsigned t = ak | (1u << bit);
      int below = 0;
#pragma unroll
      for (int j = 0; j < RPL; j++) below += __popcll(__ballot(key1[j] < t)) + __popcll(__ballot(key2[j] < t));
      if (below < k) ak = t;
    }
    thr = (double)f32_unkey(ak) + 2.0 * eps;
  }
  // rerank radius: the k listed rows with value <= a_k have exact scaled distance <= a_k + |q'|^2 +
  // eps, so a listed row beyond a_k + 2 eps is strictly farther than all k of them
  unsigned cmask = 0;
#pragma unroll
  for (int j = 0; j < RPL; j++) {
    if ((double)v1[j] <= thr) cmask |= 1u << (2 * j);
    if ((double)v2[j] <= thr) cmask |= 1u << (2 * j + 1);
  }
  cmask &= listed;

  md = DBL_MAX;
  mi = INT64_MAX;
  n_exact = 0;
  n_rescan = 0;
  // exact rerank, one candidate per lane and round
  while (__ballot(cmask != 0)) {
    bool has = cmask != 0;
    double cd = DBL_MAX;
    int64_t ci = INT64_MAX;
    if (has) {
      const int b = __ffs(cmask) - 1;
      cmask &= cmask - 1;
      const float4 x = rr[min(lane + IA_WAVE * (b >> 1), a.nwg - 1)];  // L2-hot re-read of the record
      ci = __float_as_int((b & 1) ? x.w : x.y);
      has = ci >= 0 && ci < a.NA;
      if (has) {
        cd = dist(ci);
        n_exact++;
      }
    }
    topk_offer(md, mi, cd, ci, has, k);
  }

  // certification against the k-th entry: an unlisted row of chunk w has MFMA value >= T_w, hence
  // exact distance >= T_w + |q'|^2 - eps, so only chunks with T_w <= theta may hide a row that
  // beats or ties it.  Later inserts only lower the k-th entry: theta, computed once, is
  // conservative.  A list still short of k entries certifies nothing: every chunk is rescanned.
  const double bdk = __shfl(md, k - 1, 64);
  const bool short_list = bdk == DBL_MAX;
  const float thetaf = short_list ? FLT_MAX : round_down_f(cert_theta(a, R, qn, qn2, bdk * dsc));
#pragma unroll
  for (int jb = 0; jb < RPL; jb++) {
    const int base = jb * IA_WAVE;
    unsigned long long mask = __ballot(base + lane < a.nwg && (short_list || tt[jb] <= thetaf));
    while (mask) {
      const int wgid = base + __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int64_t p0 = (int64_t)a.pos0 + (int64_t)wgid * a.tpw * IA_TILE;
      const int64_t p1 = min((int64_t)a.pos_end, p0 + (int64_t)a.tpw * IA_TILE);
      for (int64_t pb = p0; pb < p1; pb += IA_WAVE) {
        const int64_t p = pb + lane;
        const int64_t ci = p < p1 ? ia_pos_row(p, a.NT) : INT64_MAX;
        const bool has = ci < a.NA;
        double cd = DBL_MAX;
        if (has) {
          cd = dist(ci);
          n_exact++;
        }
        topk_offer(md, mi, cd, ci, has, k);
      }
      n_rescan++;
    }
  }
}

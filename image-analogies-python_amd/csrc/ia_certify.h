// ia_certify.h — K4's building blocks shared by the merges (ia_kernels.hip, ia_merge_shard.hip,
// ia_dense.hip): the certified exact winner of one query from the scan's records, and
// best_coherence_match + the kappa rule + the writeback that finish its pixel.  One wave per query.
#pragma once
#include "ia_dev.h"

// the certified single-rank winner of query m (exact NN over this rank's shard); RPL records per
// lane (nwg <= 64 RPL).  dsc: dist() * dsc is in the units of the scan's values (the prescaled
// index, ia_index.cpp ia_index_build; 1 on the level path)
template <int RPL = IA_WG_TARGET / IA_WAVE, class DistFn>
__device__ Winner certified_winner(const MergeArgs &a, int m, DistFn &&dist, unsigned *stat_out, double dsc = 1.0) {
  const int lane = threadIdx.x & 63;
  const float4 *rr = a.rec + (int64_t)m * a.nwg;
  const float *rT = a.recT + (int64_t)m * a.nwg;
  // issue every record load at once (clamped index, no per-load branch), mask afterwards
  float v1[RPL], v2[RPL], tt[RPL];
#pragma unroll
  for (int j = 0; j < RPL; j++) {
    const int w = min(lane + IA_WAVE * j, a.nwg - 1);
    const float4 x = rr[w];
    const float t = rT[w];
    const bool ok = lane + IA_WAVE * j < a.nwg;
    v1[j] = ok ? x.x : FLT_MAX;
    v2[j] = ok ? x.z : FLT_MAX;
    tt[j] = ok ? t : FLT_MAX;
  }
  const double R = (double)__uint_as_float(*a.Rbits);
  const double qn2 = a.qn2[m];
  float a1 = FLT_MAX;
#pragma unroll
  for (int j = 0; j < RPL; j++) a1 = fminf(a1, v1[j]);
  a1 = wave_min_f(a1);
  const double qn = sqrt(qn2);
  const double eps = merge_eps(a, R, qn);
  const double thr = (double)a1 + 2.0 * eps;

  // rerank every listed candidate that could be the exact winner
  unsigned cmask = 0;
#pragma unroll
  for (int j = 0; j < RPL; j++) {
    if ((double)v1[j] <= thr) cmask |= 1u << (2 * j);
    if ((double)v2[j] <= thr) cmask |= 1u << (2 * j + 1);
  }
  double bd = DBL_MAX;
  int64_t bi = INT64_MAX;
  unsigned long long nre = 0;
  while (cmask) {
    const int b = __ffs(cmask) - 1;
    cmask &= cmask - 1;
    const float4 x = rr[min(lane + IA_WAVE * (b >> 1), a.nwg - 1)];  // L2-hot re-read of the record
    const int64_t i = __float_as_int((b & 1) ? x.w : x.y);
    if (i >= 0 && i < a.NA) {
      const double d = dist(i);
      nre++;
      if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
    }
  }
  wave_min_di(bd, bi);
  if (a.rr && bd == DBL_MAX) {
    // a shard of the pruned scan that contracted no pair for this query: none of its tiles
    // passed the bound U' (K3p computes every pair a query needs), so none of its rows can be
    // the exact NN or tie it.  No winner from this shard.
    *stat_out = 0u;
    return Winner{DBL_MAX, INT64_MAX};
  }

  // certification: every unlisted row of chunk w has MFMA value >= T_w, hence true distance
  // >= T_w + |q'|^2 - eps.  Chunks with T_w <= theta may hide a row that beats or ties bd.
  const double theta = cert_theta(a, R, qn, qn2, bd * dsc);
  const float thetaf = round_down_f(theta);  // (t <= theta  <=>  t <= theta rounded down, t a float)
  unsigned long long nfb = 0;
#pragma unroll
  for (int jb = 0; jb < RPL; jb++) {
    const int base = jb * IA_WAVE;
    unsigned long long mask = __ballot(tt[jb] <= thetaf);
    while (mask) {
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int wgid = base + j;
      double cd = DBL_MAX;
      int64_t ci = INT64_MAX;
      if (a.rr) {
        // pruned scan (a shard of it): chunk = tiles wgid, wgid + nwg, ...  Rows that can
        // displace or tie the winner have exact distance <= bd, and the global NN is <= U (the
        // query's coherence candidate), so only tiles whose projection bound passes
        // min(bd * ufac, U') are rescanned.  A shard none of whose tiles passed U' in K3p holds
        // no such row: nothing is rescanned and it reports no winner (d = DBL_MAX).
        const float4 ql = a.qinfo[3 * m], qh = a.qinfo[3 * m + 1];
        const float ub = fminf(round_up_f(bd * a.ufac), a.qinfo[3 * m + 2].x);
        for (int64_t tb = 0; wgid + (int64_t)a.nwg * tb < a.NT; tb += IA_WAVE) {
          const int64_t t = wgid + (int64_t)a.nwg * (tb + lane);
          const bool nd = t < a.NT && prune_lb(a.boxes[2 * t], a.boxes[2 * t + 1], ql, qh) <= ub;
          unsigned long long nm = __ballot(nd);
          while (nm) {
            const int jt = __ffsll((long long)nm) - 1;
            nm &= nm - 1;
            if (lane < IA_TILE) {
              const int64_t i = a.pos2row[(wgid + (int64_t)a.nwg * (tb + jt)) * IA_TILE + lane];
              if (i < a.NA) {
                const double d = dist(i);
                if (d < cd || (d == cd && i < ci)) { cd = d; ci = i; }
              }
            }
          }
        }
      } else {
        const int64_t p0 = (int64_t)a.pos0 + (int64_t)wgid * a.tpw * IA_TILE;
        const int64_t p1 = min((int64_t)a.pos_end, p0 + (int64_t)a.tpw * IA_TILE);
        for (int64_t p = p0 + lane; p < p1; p += IA_WAVE) {
          const int64_t i = ia_pos_row(p, a.NT);
          if (i >= a.NA) continue;
          const double d = dist(i);
          if (d < cd || (d == cd && i < ci)) { cd = d; ci = i; }
        }
      }
      wave_min_di(cd, ci);
      if (cd < bd || (cd == bd && ci < bi)) { bd = cd; bi = ci; }
      nfb++;
    }
  }
  unsigned long long tot = nre;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
  *stat_out = (unsigned)min((unsigned long long)0xffff, tot) | ((unsigned)min((unsigned long long)0x1fff, nfb) << 16);
  return Winner{bd, bi};
}

// The rows a finish reads, as a policy R: row(i) where row i starts, dist(i, q) its exact unweighted
// distance, len() the kappa dot's length (a constant or an int), pad() the window's p_l (Pad2 or an
// int), ch() the channels; kept: the level holds pixels without a source (im < 0: the masked call's
// kept pixels of unknown origin), which are no coherence candidates.  LevelRows: a
// level's fp64 DB (K1b) under the default windows; the window calls bring their own (ia_nbhd.h
// NbhdRows).
template <int CH>
struct LevelRows {
  static constexpr bool kept = false;
  const double *__restrict__ db64;
  __device__ __forceinline__ const double *row(int64_t i) const { return db64 + i * Geo<CH>::DS; }
  __device__ __forceinline__ double dist(int64_t i, const double *q) const { return exact_dist_level<CH>(db64, i, q); }
  __device__ __forceinline__ std::integral_constant<int, Geo<CH>::D> len() const { return {}; }
  __device__ __forceinline__ Pad2 pad() const { return {}; }
  __device__ __forceinline__ std::integral_constant<int, CH> ch() const { return {}; }
};

// best_coherence_match's pick for query pixel (r, c) (algorithms.py:92-130): candidates in
// product(rows, cols) order (lane = window cell), first argmin of the correctly rounded sqrt of the
// pairwise sum.  Independent of the NN winner, so the exchange merge runs it while the peers'
// winners are in flight.  Every cell read is raster-earlier, hence of an earlier step.  Under a
// policy with `kept` a cell whose im is negative has no source: it is skipped and its s never read.
struct CohPick {
  int pr, pc, img;
  bool has;
};
template <class Rows>
__device__ __forceinline__ CohPick coherence_pick(const Rows &R, const LevelGeo &g, int r, int c, const double *q,
                                                  const int32_t *__restrict__ s, const int32_t *__restrict__ im) {
  const int lane = threadIdx.x & 63;
  const unsigned hw = (unsigned)g.ah * (unsigned)g.aw;
  const int qi = r * g.bw + c;
  CohPick k{-1, -1, 0, false};
  if (qi == 0) return k;
  double dk = DBL_MAX;
  int64_t kk = INT64_MAX;
  int cpr = -1, cpc = -1, cim = 0;
  if (lane < causal_cells(R.pad())) {
    const auto n = causal_cell(R.pad(), g.bw, r, c, qi, lane);
    bool live = n.ok;
    if constexpr (Rows::kept) live = n.ok && im[n.nb] >= 0;
    if (live) {
      const ShiftedSrc t = shifted_src(g.ah, g.aw, s[2 * n.nb], s[2 * n.nb + 1], r, c, n.nr, n.nc);
      if (t.ok) {
        cim = im[n.nb];
        cpr = t.tr;
        cpc = t.tc;
        dk = cr_sqrt(R.dist((int64_t)cim * hw + (int64_t)t.tr * g.aw + t.tc, q));
        kk = lane;
      }
    }
  }
  wave_min_di(dk, kk);
  if (kk != INT64_MAX) {
    const int src = (int)kk;
    k.pr = __shfl(cpr, src, 64);
    k.pc = __shfl(cpc, src, 64);
    k.img = __shfl(cim, src, 64);
    k.has = true;
  }
  return k;
}
// kappa rule + writeback for query pixel (r, c) whose NN row is app_ix and coherence pick ck
// (image_analogies.py:182-220, algorithms.py:133-135)
template <class Rows>
__device__ void finish_pick(const Rows &R, const LevelGeo &g, const Imgs &A, int r, int c, int64_t app_ix, const CohPick &ck,
                            const double *q, int32_t *__restrict__ s, int32_t *__restrict__ im, double *__restrict__ Bp,
                            const double *__restrict__ weights, double kf, unsigned *pstat, unsigned stat,
                            int32_t *__restrict__ nn = nullptr) {
  const int lane = threadIdx.x & 63, CH = R.ch();
  const unsigned hw = (unsigned)g.ah * (unsigned)g.aw;
  const int qi = r * g.bw + c;
  int img = (int)((unsigned)app_ix / hw);
  const unsigned rem = (unsigned)app_ix - (unsigned)img * hw;
  int pr = (int)(rem / (unsigned)g.aw), pc = (int)(rem - (unsigned)pr * (unsigned)g.aw);
  bool coh_won = false, kamb = false;
  if (ck.has) {
    // compute_distance's norm((a - q) * w) for app (lane 0) and coh (lane 1)
    double y = 0.;
    if (lane < 2) {
      const int ii = lane == 0 ? img : ck.img, rr_ = lane == 0 ? pr : ck.pr, cc_ = lane == 0 ? pc : ck.pc;
      const double *arow = R.row((int64_t)ii * hw + (int64_t)rr_ * g.aw + cc_);
      y = cr_sqrt(blas_dot_sq(R.len(), [&](int f) { return (arow[f] - q[f]) * weights[f]; }));
    }
    if (kappa_rule(__shfl(y, 0, 64), __shfl(y, 1, 64), kf, &kamb)) {
      img = ck.img;
      pr = ck.pr;
      pc = ck.pc;
      coh_won = true;
    }
  }
  if (lane < CH) Bp[(int64_t)qi * CH + lane] = A.p3[img * A.img_stride_f + ((int64_t)pr * g.aw + pc) * CH + lane];
  if (lane == 0) {
    s[2 * qi] = pr;
    s[2 * qi + 1] = pc;
    im[qi] = img;
    if (pstat) pstat[qi] = stat | (kamb ? 1u << 29 : 0u) | (coh_won ? 1u << 30 : 0u);
    if (nn) nn[qi] = app_ix >= 0 && app_ix < (int64_t)g.NA ? (int)app_ix : -1;  // option "nn_bound"
  }
}
// coherence + kappa + writeback for query pixel (r, c) whose NN row is app_ix
template <class Rows>
__device__ void finish_pixel(const Rows &R, const LevelGeo &g, const Imgs &A, int r, int c, int64_t app_ix, const double *q,
                             int32_t *__restrict__ s, int32_t *__restrict__ im, double *__restrict__ Bp,
                             const double *__restrict__ weights, double kf, unsigned *pstat, unsigned stat,
                             int32_t *__restrict__ nn = nullptr) {
  const CohPick ck = coherence_pick(R, g, r, c, q, s, im);
  finish_pick(R, g, A, r, c, app_ix, ck, q, s, im, Bp, weights, kf, pstat, stat, nn);
}

// row of the lowest set candidate bit (bit 2j: record j's best, bit 2j+1: its runner-up)
template <int RPL>
__device__ __forceinline__ int lowest_cand(unsigned cmask, const int (&i1)[RPL], const int (&i2)[RPL],
                                           const float (&v1)[RPL], const float (&v2)[RPL], float &v) {
  int row = -1;
  v = FLT_MAX;
#pragma unroll
  for (int j = RPL - 1; j >= 0; j--) {
    const bool b2 = (cmask >> (2 * j + 1)) & 1, b1 = (cmask >> (2 * j)) & 1;
    row = b2 ? i2[j] : row;
    v = b2 ? v2[j] : v;
    row = b1 ? i1[j] : row;
    v = b1 ? v1[j] : v;
  }
  return row;
}

// ia_nbhd.h — the window calls' per-query bodies, one wave per query, and the two places a step's
// queries come from: the wavefront's geometry (ia_synthesize_levels_nbhd) or the step's list
// (ia_synthesize_levels_masked).  ia_nbhd.hip compiles its gather and finish kernels once per source.
#pragma once
#include "ia_certify.h"
#include "ia_launch.h"

// A step's queries: count() of them, query m at pixel qpix(w, m, width of the B level).  kept: the level
// holds kept pixels, some without a source (NbhdRows below).
struct WaveSource {  // step sd of the schedule t = col + (p_l + 1) row, all jobs (ia_qpix)
  static constexpr bool kept = false;
  StepDesc sd;
  __device__ __forceinline__ int count() const { return sd.J * sd.M; }
  __device__ __forceinline__ QPix qpix(const NbhdGeo &w, int m, int bw) const { return ia_qpix(sd, bw, m, w.p_l + 1); }
};
struct ListSource {  // entry m of the step's list: its job and raster index (ia_mask.hip k_mask_steps)
  static constexpr bool kept = true;
  const int2 *__restrict__ list;
  int n;
  __device__ __forceinline__ int count() const { return n; }
  __device__ __forceinline__ QPix qpix(const NbhdGeo &, int m, int bw) const {
    const int2 e = list[m];
    QPix p;
    p.job = e.x;
    p.qi = e.y;
    p.r = e.y / bw;
    p.c = e.y - p.r * bw;
    return p;
  }
};

// the fp64 query row of pixel px (query m of its step) into q[m, 0..D)
template <class JS>
__device__ __forceinline__ void nbhd_gather_query(const NbhdGeo &w, Imgs B, const JS &jobs, const QPix &px, int m,
                                                  double *__restrict__ q) {
  const int lane = threadIdx.x & 63;
  if constexpr (!JS::single) B = job_imgs(B, jobs.get(px.job));  // single job: B already holds its images
  for (int f = lane; f < w.D; f += IA_WAVE) q[(int64_t)m * w.D + f] = win_feat(w, B, f, px.r, px.c, 0);
}

// these calls' rows as finish_pixel reads them (ia_certify.h LevelRows): N_A x D contiguous.  KEPT:
// the coherence pick skips cells without a source
template <bool KEPT = false>
struct NbhdRows {
  static constexpr bool kept = KEPT;
  const double *__restrict__ rows;
  int D, p_l, nch;
  __device__ __forceinline__ const double *row(int64_t i) const { return rows + i * D; }
  __device__ __forceinline__ double dist(int64_t i, const double *q) const { return row_dist2_rt(row(i), q, D); }
  __device__ __forceinline__ int len() const { return D; }
  __device__ __forceinline__ int pad() const { return p_l; }
  __device__ __forceinline__ int ch() const { return nch; }
};

// K4's finish_pixel (ia_certify.h) for pixel px, query m of its step, from the certified winner idx[m]
template <bool KEPT, class JS>
__device__ __forceinline__ void nbhd_finish_query(const NbhdGeo &w, const LevelGeo &g, const Imgs &A, const JS &jobs,
                                                  const QPix &px, int m, const double *__restrict__ rows,
                                                  const double *__restrict__ q64, const int64_t *__restrict__ idx) {
  const JobPtrs jp = jobs.get(px.job);
  int64_t app_ix = idx[m];
  if ((uint64_t)app_ix >= (uint64_t)g.NA) app_ix = 0;  // (no winner: a NaN query; never an index past the DB)
  finish_pixel(NbhdRows<KEPT>{rows, w.D, w.p_l, w.ch}, g, A, px.r, px.c, app_ix, q64 + (int64_t)m * w.D, jp.s, jp.im, jp.Bp,
               jp.weights, jp.kf, jp.pstat, 0u);
}

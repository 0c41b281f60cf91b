// ia_gather.hip — the stand-alone gathers of a wavefront step: K2 (fp32 matcher), K2h
// (split-f16) and K2p (split-f16, pruned scan), and their launchers.  The fused merge + gather
// launch (ia_kernels.hip) runs the same bodies from ia_gather.h.
#include "ia_gather.h"
#include "ia_launch.h"

// ------------------------------------------------------------------------------------------
// K2: queries of one wavefront step (one wave per query pixel)
// ------------------------------------------------------------------------------------------
template <int CH>
__device__ __forceinline__ void put_qfrag(float *qf, int m, int f, float v) {
  using G = Geo<CH>;
  const int qt = m / IA_TILE, j = m % IA_TILE, h = f / G::KH, s = f % G::KH;
  qf[(((int64_t)qt * G::KP + s / 4) * IA_WAVE + h * IA_TILE + j) * 4 + (s % 4)] = v;
}

template <int CH, class JS>
__global__ void __launch_bounds__(IA_WG) k_gather_query(LevelGeo g, StepDesc sd, Imgs B, JS jobs,
                                                         const double *__restrict__ mu_part,
                                                         double *__restrict__ q64, double *__restrict__ qn2,
                                                         float *__restrict__ qf) {
  using G = Geo<CH>;
  const int lane = threadIdx.x & 63;
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= sd.Mpad) return;
  if (m >= sd.J * sd.M) {
    for (int f = lane; f < G::DP; f += IA_WAVE) put_qfrag<CH>(qf, m, f, 0.f);
    return;
  }
  const QPix px = ia_qpix(sd, g.bw, m);
  if constexpr (!JS::single) B = job_imgs(B, jobs.get(px.job));  // single job: B already holds its images
  const int r = px.r, c = px.c;
  double ss = 0.;
  for (int f = lane; f < G::DP; f += IA_WAVE) {
    if (f < G::D) {
      const double v = win_feat(Geo<CH>{}, B, f, r, c, 0);
      q64[(int64_t)m * G::D + f] = v;
      const double qc = v - mu_part[feat_part<CH>(f) * CH + feat_ch<CH>(f)];
      ss += qc * qc;
      put_qfrag<CH>(qf, m, f, -2.f * (float)qc);
    } else {
      put_qfrag<CH>(qf, m, f, f == G::D ? 1.f : 0.f);
    }
  }
  ss = wave_sum_d(ss);
  if (lane == 0) qn2[m] = ss;
}

template <int CH, int KS, class JS>
__global__ void __launch_bounds__(IA_PQ_WG) k_gather_query_h(LevelGeo g, StepDesc sd, Imgs B, JS jobs,
                                                           const double *__restrict__ mu_part,
                                                           double *__restrict__ q64, double *__restrict__ qn2,
                                                           _Float16 *__restrict__ qf) {
  constexpr int D = 55 * CH, KD = 16 * KS;
  const int lane = threadIdx.x & 63;
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * IA_PQ_WPB + (threadIdx.x >> 6));  // wave-uniform
  if (m >= sd.Mpad) return;
  if (m >= sd.J * sd.M) {
    for (int f = lane; f < KD; f += IA_WAVE) put_qh<KS>(qf, m, f, 0.);
    return;
  }
  const QPix px = ia_qpix(sd, g.bw, m);
  if constexpr (!JS::single) B = job_imgs(B, jobs.get(px.job));  // single job: B already holds its images
  const int r = px.r, c = px.c;
  double ss = 0.;
  for (int f = lane; f < KD; f += IA_WAVE) {
    if (f < D) {
      const double v = win_feat(Geo<CH>{}, B, f, r, c, 0);
      q64[(int64_t)m * D + f] = v;
      const double qc = v - mu_part[feat_part<CH>(f) * CH + feat_ch<CH>(f)];
      ss += qc * qc;
      put_qh<KS>(qf, m, f, -2.0 * qc);
    } else {
      put_qh<KS>(qf, m, f, f == D ? IA_NORM_SCALE : 0.);
    }
  }
  ss = wave_sum_d(ss);
  if (lane == 0) qn2[m] = ss;
}

// ------------------------------------------------------------------------------------------
// K2p: K2h for the pruned scan (1 channel) — one wave per query.  Besides the split-f16 query
// fragments it writes the query's pruning record (ia_prune.h), qinfo[3m .. 3m+2]:
//   (qlo_0..3), (qhi_0..3): f32 interval around the fp64 projection onto the level's basis
//   (U', key bits, 0, 0):   U' from the exact fp64 distance of the best coherence candidate
//                           (best_coherence_match's candidate set: the causal 5x5 neighbours'
//                           shifted source pixels, all final at this wavefront step), the
//                           Morton key of the projection (sort order of the query tiles)
// (the A-side images stay in the argument list, unread: the kernel's argument layout is fixed)
// ------------------------------------------------------------------------------------------
template <int KS, class JS>
__global__ void __launch_bounds__(IA_PQ_WG) k_gather_query_p(LevelGeo g, StepDesc sd, Imgs B, JS jobs,
                                                          const double *__restrict__ mu_part,
                                                          double *__restrict__ q64, double *__restrict__ qn2,
                                                          _Float16 *__restrict__ qf, const double *__restrict__ db64,
                                                          const double *__restrict__ basis, double ufac,
                                                          float4 *__restrict__ qinfo, Imgs A, XOPub xp) {
  constexpr int KD = 16 * KS;
  __shared__ double qsh[IA_PQ_WPB][Geo<1>::DS];
  __shared__ __attribute__((aligned(16))) _Float16 xh[IA_PQ_WPB][2][KD];  // owner publish: the query's hi / lo columns
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = blockIdx.x * IA_PQ_WPB + wv;
  if (m >= sd.Mpad) return;
  float4 i0, i1, i2;
  if (m >= sd.J * sd.M) {
    gather_p_pad<KS>(m, lane, qf, qinfo, i0, i1, i2);
    if (xp.W && lane < KD) xh[wv][0][lane] = xh[wv][1][lane] = (_Float16)0.f;
  } else {
    const QPix px = ia_qpix(sd, g.bw, m);
    const JobPtrs jp = jobs.get(px.job);
    if constexpr (!JS::single) B = job_imgs(B, jp);  // single job: B already holds its images
    gather_p_query<KS, false>(g, sd, B, jp, m, lane, mu_part, q64, qn2, qf, db64, basis, ufac, qinfo, qsh[wv],
                              xp.W ? xh[wv][0] : nullptr, xh[wv][1], QHand{}, i0, i1, i2);
  }
  if (xp.W) xo_publish<KS>(xp, m, lane, xh[wv][0], xh[wv][1], i0, i1, i2);
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_level_run.cpp, ia_level_owner.cpp)
// ------------------------------------------------------------------------------------------
void ia_launch_gather(const LevelGeo &g, const StepDesc &sd, const Imgs &B, const JobSet &jobs, const double *mu, double *q64,
                      double *qn2, float *qf, hipStream_t st) {
  const dim3 grid(cdiv(sd.Mpad, IA_WG / IA_WAVE));
  with_ch(g.ch, [&](auto c) {
    with_jobs(jobs, B, [&](auto js, const Imgs &Bj) {
      hipLaunchKernelGGL((k_gather_query<decltype(c)::CH, decltype(js)>), grid, dim3(IA_WG), 0, st, g, sd, Bj, js, mu, q64, qn2,
                         qf);
    });
  });
}

void ia_launch_gather_h(const LevelGeo &g, const StepDesc &sd, const Imgs &B, const JobSet &jobs, const double *mu,
                        double *q64, double *qn2, void *qf, hipStream_t st) {
  const dim3 grid(cdiv(sd.Mpad, IA_PQ_WPB));
  with_ch_ks(g.ch, [&](auto c) {
    with_jobs(jobs, B, [&](auto js, const Imgs &Bj) {
      hipLaunchKernelGGL((k_gather_query_h<decltype(c)::CH, decltype(c)::KS, decltype(js)>), grid, dim3(IA_PQ_WG), 0, st, g, sd,
                         Bj, js, mu, q64, qn2, (_Float16 *)qf);
    });
  });
}

void ia_launch_gather_p(const LevelGeo &g, const StepDesc &sd, const Imgs &B, const JobSet &jobs, const double *mu,
                        double *q64, double *qn2, void *qf, const double *db64, const double *basis, double ufac,
                        float4 *qinfo, const Imgs &A, hipStream_t st, const XOPub *xp) {
  const XOPub x = xp ? *xp : XOPub{};
  const dim3 grid(cdiv(sd.Mpad, IA_PQ_WPB));
  with_jobs(jobs, B, [&](auto js, const Imgs &Bj) {
    hipLaunchKernelGGL((k_gather_query_p<4, decltype(js)>), grid, dim3(IA_PQ_WG), 0, st, g, sd, Bj, js, mu, q64, qn2,
                       (_Float16 *)qf, db64, basis, ufac, qinfo, A, x);
  });
}

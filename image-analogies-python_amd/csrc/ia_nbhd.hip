// ia_nbhd.hip — exact levels for runtime window sizes (include/ia.h ia_synthesize_levels_nbhd,
// DESIGN.md §11): the kernels that know the windows.  n_sm, n_lg and ch arrive at run time; there
// is no instance per size.
//
//   k_nbhd_rows      the level's fp64 row DB, N_A x D contiguous: [A n_sm^2 | A n_lg^2 | A' n_sm^2 |
//                    A' first n_half cells] per pixel (algorithms.py:11-47,50-70)
//   k_nbhd_colstats  beside it: the D column means and the largest centred |value|, which centre
//                    and prescale the fp32 copy (ia_dense.hip k_dense_db_build)
//   k_nbhd_gather    the fp64 query rows of one step, one wave per query, all jobs
//   k_nbhd_finish    K4's finish_pixel (ia_certify.h) over this call's rows: best_coherence_match
//                    over the (p_l + 1) x (2 p_l + 1) window, the kappa rule, the B' / s / im writeback
//                    Both are compiled once per source of the step's queries (ia_nbhd.h): the wavefront's
//                    geometry for this call, the step's list for the masked one (ia_level_mask.cpp,
//                    whose list kernels are ia_mask.hip's); the finish's coherence pick skips cells
//                    without a source only in the list form.
//
// Between gather and finish a step runs the index's kernels unchanged: k_dense_query, k3_dist and
// k_merge_dense (certified_winner over row_dist2_rt), so the NN is the exact fp64 one.
// The per-pixel rules are the default path's own text, compiled here with run-time geometry:
// win_feat, ia_qpix, causal_cell / shifted_src, blas_dot_sq and kappa_rule (ia_dev.h, ia_internal.h).
#include "ia_nbhd.h"

__global__ void __launch_bounds__(IA_WG) k_nbhd_rows(NbhdGeo w, Imgs A, APairs ap, int64_t NA, double *__restrict__ rows) {
  const int64_t n = NA * w.D, hw = (int64_t)A.h * A.w;
  for (int64_t i = (int64_t)blockIdx.x * IA_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IA_WG) {
    const int64_t row = i / w.D;
    const int f = (int)(i - row * w.D), img = (int)(row / hw);
    const int px = (int)(row - img * hw), r = px / A.w, c = px - r * A.w;
    rows[i] = win_feat(w, ia_pair_imgs(A, ap, img), f, r, c, img);
  }
}

// Column f's mean (thread t sums rows t, t + 256, ... in order, then a fixed LDS tree) and the
// largest |value - mean| over all columns (atomicMax on the bits of a float rounded up, as Rbits).
// Neither decides a result: the mean only centres the fp32 copy and the maximum only picks its
// power-of-two prescale.  The certification takes R and |q'| from the centred copy itself, so any
// finite pair gives the same exact winners; they size the error bound, i.e. the rescans.
__global__ void __launch_bounds__(IA_WG) k_nbhd_colstats(const double *__restrict__ rows, int64_t NA, int D,
                                                         double *__restrict__ mu, unsigned *__restrict__ amax_bits) {
  __shared__ double red[IA_WG];
  const int f = blockIdx.x, t = threadIdx.x;
  double s = 0.;
  for (int64_t i = t; i < NA; i += IA_WG) s += rows[i * D + f];
  red[t] = s;
  __syncthreads();
  for (int o = IA_WG / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double mean = red[0] / (double)NA;
  __syncthreads();
  double mx = 0.;
  for (int64_t i = t; i < NA; i += IA_WG) mx = fmax(mx, fabs(rows[i * D + f] - mean));
  red[t] = mx;
  __syncthreads();
  for (int o = IA_WG / 2; o > 0; o >>= 1) {
    if (t < o) red[t] = fmax(red[t], red[t + o]);
    __syncthreads();
  }
  if (t == 0) {
    mu[f] = mean;
    atomicMax(amax_bits, __float_as_uint(round_up_f(red[0])));
  }
}

template <class SRC, class JS>
__global__ void __launch_bounds__(IA_WG) k_nbhd_gather(NbhdGeo w, SRC src, Imgs B, JS jobs, double *__restrict__ q) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= src.count()) return;
  nbhd_gather_query(w, B, jobs, src.qpix(w, m, B.w), m, q);
}

template <class SRC, class JS>
__global__ void __launch_bounds__(IA_WG) k_nbhd_finish(NbhdGeo w, LevelGeo g, SRC src, Imgs A, JS jobs,
                                                       const double *__restrict__ rows, const double *__restrict__ q64,
                                                       const int64_t *__restrict__ idx) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= src.count()) return;
  nbhd_finish_query<SRC::kept>(w, g, A, jobs, src.qpix(w, m, g.bw), m, rows, q64, idx);
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_level_nbhd.cpp: the DB, and the one step of both window calls)
// ------------------------------------------------------------------------------------------
void ia_launch_nbhd_rows(const NbhdGeo &w, const Imgs &A, const APairs &ap, int64_t NA, double *rows, double *mu,
                         unsigned *amax_bits, hipStream_t st) {
  const unsigned nwg = (unsigned)std::min<int64_t>(4096, (NA * w.D + IA_WG - 1) / IA_WG);
  hipLaunchKernelGGL(k_nbhd_rows, dim3(nwg), dim3(IA_WG), 0, st, w, A, ap, NA, rows);
  hipLaunchKernelGGL(k_nbhd_colstats, dim3(w.D), dim3(IA_WG), 0, st, rows, NA, w.D, mu, amax_bits);
}

// the step's source as the kernels' SRC argument: f(src)
template <class F>
static inline void with_source(const NbhdStep &step, F &&f) {
  if (step.list) f(ListSource{step.list, step.n});
  else f(WaveSource{step.sd});
}

void ia_launch_nbhd_gather(const NbhdGeo &w, const NbhdStep &step, const Imgs &B, const JobSet &jobs, double *q, hipStream_t st) {
  const dim3 grid(cdiv(step.n, IA_WG / IA_WAVE));
  with_source(step, [&](auto src) {
    with_jobs(jobs, B, [&](auto js, const Imgs &Bj) {
      hipLaunchKernelGGL((k_nbhd_gather<decltype(src), decltype(js)>), grid, dim3(IA_WG), 0, st, w, src, Bj, js, q);
    });
  });
}

void ia_launch_nbhd_finish(const NbhdGeo &w, const LevelGeo &g, const NbhdStep &step, const Imgs &A, const JobSet &jobs,
                           const double *rows, const double *q, const int64_t *idx, hipStream_t st) {
  const dim3 grid(cdiv(step.n, IA_WG / IA_WAVE));
  with_source(step, [&](auto src) {
    with_jobs(jobs, [&](auto js) {
      hipLaunchKernelGGL((k_nbhd_finish<decltype(src), decltype(js)>), grid, dim3(IA_WG), 0, st, w, g, src, A, js, rows, q, idx);
    });
  });
}

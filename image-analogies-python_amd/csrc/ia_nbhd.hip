// ia_nbhd.hip — exact levels for runtime window sizes (include/ia.h ia_synthesize_levels_nbhd,
// DESIGN.md §11): the kernels that know the windows.  n_sm, n_lg and ch arrive at run time; there
// is no instance per size.
//
//   k_nbhd_rows      the level's fp64 row DB, N_A x D contiguous: [A n_sm^2 | A n_lg^2 | A' n_sm^2 |
//                    A' first n_half cells] per pixel (algorithms.py:11-47,50-70)
//   k_nbhd_colstats  beside it: the D column means and the largest centred |value|, which centre
//                    and prescale the fp32 copy (ia_dense.hip k_dense_db_build)
//   k_nbhd_gather    the fp64 query rows of one wavefront step, one wave per query, all jobs
//   k_nbhd_finish    best_coherence_match over the (p_l + 1) x (2 p_l + 1) window, the kappa rule
//                    with the BLAS-order dot for runtime n, and the B' / s / im writeback
//
// Between gather and finish a step runs the index's kernels unchanged: k_dense_query, k3_dist and
// k_merge_dense (certified_winner over row_dist2_rt), so the NN is the exact fp64 one.
// Order of operations in k_nbhd_finish is ia_certify.h coherence_pick + finish_pick's, so that
// (3, 5) gives K4's bits.
#include "ia_dev.h"
#include "ia_launch.h"

// query m of the step: job m / M, row r0 + m % M, column t - skew * row (skew = p_l + 1)
__device__ __forceinline__ QPix nbhd_qpix(const StepDesc &sd, int bw, int skew, int m) {
  QPix p;
  p.job = m / sd.M;
  p.r = sd.r0 + (m - p.job * sd.M);
  p.c = sd.t - skew * p.r;
  p.qi = p.r * bw + p.c;
  return p;
}

// feature f of pixel (r, c): parts in the reference's order, each row-major and channel-minor,
// symmetric padding (ia_reflect takes any reach: periodic for images smaller than the pad)
__device__ __forceinline__ double nbhd_feat(const NbhdGeo &w, const Imgs &I, int f, int r, int c, int img) {
  const int part = f < w.o1 ? 0 : f < w.o2 ? 1 : f < w.o3 ? 2 : 3;
  const int e = f - (part == 0 ? 0 : part == 1 ? w.o1 : part == 2 ? w.o2 : w.o3);
  const int k = e / w.ch, chn = e - k * w.ch;
  if (part == 0 || part == 2) {
    const int y = ia_reflect((r >> 1) + k / w.n_sm - w.p_s, I.hc), x = ia_reflect((c >> 1) + k % w.n_sm - w.p_s, I.wc);
    const double *b = part == 0 ? I.p0 : I.p2 + img * I.img_stride_c;
    return b[((int64_t)y * I.wc + x) * w.ch + chn];
  }
  const int y = ia_reflect(r + k / w.n_lg - w.p_l, I.h), x = ia_reflect(c + k % w.n_lg - w.p_l, I.w);
  const double *b = part == 1 ? I.p1 : I.p3 + img * I.img_stride_f;
  return b[((int64_t)y * I.w + x) * w.ch + chn];
}

__global__ void __launch_bounds__(IA_WG) k_nbhd_rows(NbhdGeo w, Imgs A, APairs ap, int64_t NA, double *__restrict__ rows) {
  const int64_t n = NA * w.D, hw = (int64_t)A.h * A.w;
  for (int64_t i = (int64_t)blockIdx.x * IA_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IA_WG) {
    const int64_t row = i / w.D;
    const int f = (int)(i - row * w.D), img = (int)(row / hw);
    const int px = (int)(row - img * hw), r = px / A.w, c = px - r * A.w;
    rows[i] = nbhd_feat(w, ia_pair_imgs(A, ap, img), f, r, c, img);
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

template <class JS>
__global__ void __launch_bounds__(IA_WG) k_nbhd_gather(NbhdGeo w, StepDesc sd, Imgs B, JS jobs, double *__restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= sd.J * sd.M) return;
  const QPix px = nbhd_qpix(sd, B.w, w.p_l + 1, m);
  if constexpr (!JS::single) B = job_imgs(B, jobs.get(px.job));  // single job: B already holds its images
  for (int f = lane; f < w.D; f += IA_WAVE) q[(int64_t)m * w.D + f] = nbhd_feat(w, B, f, px.r, px.c, 0);
}

// x.x in blas_dot_sq's order (ia_dev.h; oracle/ia_oracle.py blas_ddot_sq) for n known at run time
template <class X>
__device__ double nbhd_blas_dot_sq(X &&x, int n) {
  const int n1 = n & ~15, n32 = n1 & ~31;
  double acc[4][4];
  if (n32 > 0) {
    double z[4][8];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int l = 0; l < 8; l++) {
        const double v = x(8 * k + l);
        z[k][l] = v * v;  // fma(v, v, 0)
      }
    for (int i = 32; i < n32; i += 32)
#pragma unroll
      for (int k = 0; k < 4; k++)
#pragma unroll
        for (int l = 0; l < 8; l++) {
          const double v = x(i + 8 * k + l);
          z[k][l] = __builtin_fma(v, v, z[k][l]);
        }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int l = 0; l < 4; l++) acc[k][l] = z[k][l] + z[k][l + 4];
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int l = 0; l < 4; l++) acc[k][l] = 0.;
  }
  for (int i = n32; i < n1; i += 16)
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const double v = x(i + 4 * k + l);
        acc[k][l] = __builtin_fma(v, v, acc[k][l]);
      }
  double dot = 0.;
  if (n1 > 0) {
    double sl[4];
#pragma unroll
    for (int l = 0; l < 4; l++) sl[l] = ((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l];
    dot = (sl[0] + sl[2]) + (sl[1] + sl[3]);
  }
  for (int f = n1; f < n; f++) {
    const double v = x(f);
    dot = __builtin_fma(v, v, dot);
  }
  return dot;
}

template <class JS>
__global__ void __launch_bounds__(IA_WG) k_nbhd_finish(NbhdGeo w, LevelGeo g, StepDesc sd, Imgs A, JS jobs,
                                                       const double *__restrict__ rows, const double *__restrict__ q64,
                                                       const int64_t *__restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= sd.J * sd.M) return;
  const QPix px = nbhd_qpix(sd, g.bw, w.p_l + 1, m);
  const JobPtrs jp = jobs.get(px.job);
  const int r = px.r, c = px.c, qi = px.qi, D = w.D;
  const double *q = q64 + (int64_t)m * D;
  const unsigned hw = (unsigned)g.ah * (unsigned)g.aw;
  int64_t app_ix = idx[m];
  if ((uint64_t)app_ix >= (uint64_t)g.NA) app_ix = 0;  // (no winner: a NaN query; never an index past the DB)

  // best_coherence_match: lane = window cell in product(rows, cols) order, first argmin of the
  // correctly rounded sqrt of the pairwise sum.  Every cell read here is raster-earlier, hence of
  // an earlier step: s / im hold it before this launch writes anything.
  const int wd = 2 * w.p_l + 1;
  double dk = DBL_MAX;
  int64_t kk = INT64_MAX;
  int cpr = -1, cpc = -1, cim = 0;
  if (qi > 0 && lane < (w.p_l + 1) * wd) {
    const int nr = r - w.p_l + lane / wd, nc = c - w.p_l + lane % wd;
    if (nr >= 0 && nc >= 0 && nc < g.bw && nr * g.bw + nc < qi) {
      const int nb = nr * g.bw + nc;
      const int tr = jp.s[2 * nb] + r - nr, tc = jp.s[2 * nb + 1] + c - nc;
      if (tr >= 0 && tr < g.ah && tc >= 0 && tc < g.aw) {
        cim = jp.im[nb];
        cpr = tr;
        cpc = tc;
        const int64_t row = (int64_t)cim * hw + (int64_t)tr * g.aw + tc;
        dk = cr_sqrt(row_dist2_rt(rows + row * D, q, D));
        kk = lane;
      }
    }
  }
  wave_min_di(dk, kk);
  const bool has = kk != INT64_MAX;
  int kpr = -1, kpc = -1, kim = 0;
  if (has) {
    kpr = __shfl(cpr, (int)kk, 64);
    kpc = __shfl(cpc, (int)kk, 64);
    kim = __shfl(cim, (int)kk, 64);
  }

  int img = (int)((unsigned)app_ix / hw);
  const unsigned rem = (unsigned)app_ix - (unsigned)img * hw;
  int pr = (int)(rem / (unsigned)g.aw), pc = (int)(rem - (unsigned)pr * (unsigned)g.aw);
  bool coh_won = false, kamb = false;
  if (has) {
    // compute_distance(AAp_feat, BBp_feat, weights) = norm((a - q) * w)**2 for app (lane 0) and coh (lane 1)
    double part = 0.;
    if (lane < 2) {
      const int ii = lane == 0 ? img : kim, rr_ = lane == 0 ? pr : kpr, cc_ = lane == 0 ? pc : kpc;
      const double *arow = rows + ((int64_t)ii * hw + (int64_t)rr_ * g.aw + cc_) * D;
      const double *wt = jp.weights;
      part = cr_sqrt(nbhd_blas_dot_sq([&](int f) { return (arow[f] - q[f]) * wt[f]; }, D));
    }
    const double y_app = __shfl(part, 0, 64), y_coh = __shfl(part, 1, 64);
    const double d_app = y_app * y_app, d_coh = y_coh * y_coh;
    kamb = kappa_ambiguous(y_app, d_app, y_coh, d_coh, jp.kf);
    if (d_coh <= d_app * jp.kf) {
      img = kim;
      pr = kpr;
      pc = kpc;
      coh_won = true;
    }
  }
  if (lane < w.ch) jp.Bp[(int64_t)qi * w.ch + lane] = A.p3[img * A.img_stride_f + ((int64_t)pr * g.aw + pc) * w.ch + lane];
  if (lane == 0) {
    jp.s[2 * qi] = pr;
    jp.s[2 * qi + 1] = pc;
    jp.im[qi] = img;
    jp.pstat[qi] = (kamb ? 1u << 29 : 0u) | (coh_won ? 1u << 30 : 0u);
  }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_level_nbhd.cpp)
// ------------------------------------------------------------------------------------------
void ia_launch_nbhd_rows(const NbhdGeo &w, const Imgs &A, const APairs &ap, int64_t NA, double *rows, double *mu,
                         unsigned *amax_bits, hipStream_t st) {
  const unsigned nwg = (unsigned)std::min<int64_t>(4096, (NA * w.D + IA_WG - 1) / IA_WG);
  hipLaunchKernelGGL(k_nbhd_rows, dim3(nwg), dim3(IA_WG), 0, st, w, A, ap, NA, rows);
  hipLaunchKernelGGL(k_nbhd_colstats, dim3(w.D), dim3(IA_WG), 0, st, rows, NA, w.D, mu, amax_bits);
}

void ia_launch_nbhd_gather(const NbhdGeo &w, const StepDesc &sd, const Imgs &B, const JobSet &jobs, double *q, hipStream_t st) {
  const dim3 grid(cdiv((int64_t)sd.J * sd.M, IA_WG / IA_WAVE));
  with_jobs(jobs, B, [&](auto js, const Imgs &Bj) {
    hipLaunchKernelGGL((k_nbhd_gather<decltype(js)>), grid, dim3(IA_WG), 0, st, w, sd, Bj, js, q);
  });
}

void ia_launch_nbhd_finish(const NbhdGeo &w, const LevelGeo &g, const StepDesc &sd, const Imgs &A, const JobSet &jobs,
                           const double *rows, const double *q, const int64_t *idx, hipStream_t st) {
  const dim3 grid(cdiv((int64_t)sd.J * sd.M, IA_WG / IA_WAVE));
  with_jobs(jobs, [&](auto js) {
    hipLaunchKernelGGL((k_nbhd_finish<decltype(js)>), grid, dim3(IA_WG), 0, st, w, g, sd, A, js, rows, q, idx);
  });
}

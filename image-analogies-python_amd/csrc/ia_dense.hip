// ia_dense.hip — kernels off the level path: the dense variants for the FLANN-compatible index
// (ia_index_*), the per-level statistics, option "stamps", the microbenchmark operands; and
// their launchers.
#include "ia_certify.h"
#include "ia_launch.h"
#include "ia_topk.h"

// option "stamps": launch i's first workgroup start and last workgroup end over its `stride`
// workgroup slots (unwritten slots are zero), in s_memrealtime ticks; one wave per launch
// span2 (optional): per launch the last workgroup start - the first, and the mean workgroup
// duration (ticks)
__global__ void __launch_bounds__(IA_WAVE) k_stamp_durations(const unsigned long long *__restrict__ stamps, int stride,
                                                            unsigned long long *__restrict__ span,
                                                            unsigned long long *__restrict__ span2) {
  const int i = blockIdx.x, lane = threadIdx.x;
  unsigned long long lo = ~0ull, hi = 0ull, smax = 0ull, dsum = 0ull, n = 0ull;
  for (int j = lane; j < stride; j += IA_WAVE) {
    const unsigned long long a = stamps[2 * ((int64_t)i * stride + j)], b = stamps[2 * ((int64_t)i * stride + j) + 1];
    if (a) {
      lo = a < lo ? a : lo;
      hi = b > hi ? b : hi;
      smax = a > smax ? a : smax;
      dsum += b > a ? b - a : 0ull;
      n++;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64), m2 = __shfl_xor(smax, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
    smax = m2 > smax ? m2 : smax;
    dsum += __shfl_xor(dsum, o, 64);
    n += __shfl_xor(n, o, 64);
  }
  if (lane == 0) {
    const bool ok = hi >= lo && hi;
    span[2 * i] = ok ? lo : 0ull;
    span[2 * i + 1] = ok ? hi : 0ull;
    if (span2) {
      span2[2 * i] = ok ? smax - lo : 0ull;
      span2[2 * i + 1] = ok && n ? dsum / n : 0ull;
    }
  }
}
void ia_launch_stamp_durations(const unsigned long long *stamps, int n, int stride, unsigned long long *span, hipStream_t st,
                               unsigned long long *span2) {
  if (n > 0) hipLaunchKernelGGL(k_stamp_durations, dim3(n), dim3(IA_WAVE), 0, st, stamps, stride, span, span2);
}

// per-level statistics: sum the per-pixel stats words.  Grid-stride loop over up to 256
// workgroups; each workgroup reduces in LDS and adds its five integer sums with one u64
// atomicAdd per counter (integer sums are order-free; counters are zeroed per level)
__global__ void __launch_bounds__(IA_WG) k_reduce_stats(const unsigned *__restrict__ pstat, int64_t n,
                                                         unsigned long long *__restrict__ counters) {
  unsigned long long rr = 0, fb = 0, cw = 0, bv = 0, ka = 0;
  for (int64_t i = (int64_t)blockIdx.x * IA_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IA_WG) {
    const unsigned v = pstat[i];
    rr += v & 0xffff;
    fb += (v >> 16) & 0x1fff;
    ka += (v >> 29) & 1;
    cw += (v >> 30) & 1;
    bv += v >> 31;
  }
  __shared__ unsigned long long red[5][IA_WG];
  red[0][threadIdx.x] = rr;
  red[1][threadIdx.x] = fb;
  red[2][threadIdx.x] = cw;
  red[3][threadIdx.x] = bv;
  red[4][threadIdx.x] = ka;
  __syncthreads();
  for (int o = IA_WG / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < 5; k++) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  // integer sums: order-free, so one global atomic per counter and workgroup (counters are
  // zeroed at the start of the level)
  if (threadIdx.x < 5) atomicAdd(&counters[threadIdx.x], red[threadIdx.x][0]);
}

// ------------------------------------------------------------------------------------------
// dense (FLANN-compatible index) variants: rows given as n x d fp64
//
// The fp32 copy of the rows and of the queries is centred (mu) and multiplied by sc, a power of two
// chosen at ia_index_build so that the largest centred |value| lies in [0.5, 1): the scan's squares
// and products then neither overflow nor underflow fp32 whatever the caller's units, which is
// what the error bound ia_eps_c assumes (there is no range gate as on the level path).  The scan's
// values, qn2 and R are in the scaled units; the exact distances are computed from the caller's
// rows and enter the certification threshold multiplied by dsc = sc^2 (exact).
// ------------------------------------------------------------------------------------------
template <int KH>
__global__ void __launch_bounds__(IA_WG) k_dense_db_build(const double *__restrict__ pts, int64_t n, int d, int n_tiles,
                                                           const double *__restrict__ mu, double sc,
                                                           float4 *__restrict__ db, unsigned *__restrict__ Rbits) {
  constexpr int KP = KH / 4;
  const int64_t pos = (int64_t)blockIdx.x * IA_WG + threadIdx.x;
  if (pos >= (int64_t)n_tiles * IA_TILE) return;
  const int64_t row = ia_pos_row(pos, n_tiles);
  const bool real = row < n;
  const int64_t tile = pos / IA_TILE;
  const int j = (int)(pos % IA_TILE);
  double norm = 0.;
  for (int h = 0; h < 2; h++) {
    for (int p = 0; p < KP; p++) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int f = h * KH + 4 * p + e;
        if (f < d) {
          double a = real ? (pts[row * d + f] - mu[f]) * sc : 0.;
          norm += a * a;
          v[e] = (float)a;
        } else if (f == d) {
          v[e] = real ? (float)norm : IA_PAD_NORM;
        } else {
          v[e] = 0.f;
        }
      }
      db[(tile * KP + p) * IA_WAVE + h * IA_TILE + j] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  if (real) atomicMax(Rbits, __float_as_uint((float)(sqrt(norm) * (1.0 + 1e-6))));
}

template <int KH>
__global__ void __launch_bounds__(IA_WG) k_dense_query(const double *__restrict__ q, int64_t nq, int d, int Mpad,
                                                        const double *__restrict__ mu, double sc,
                                                        double *__restrict__ qn2, float *__restrict__ qf) {
  constexpr int KP = KH / 4;
  const int lane = threadIdx.x & 63;
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= Mpad) return;
  double ss = 0.;
  for (int f = lane; f < 2 * KH; f += IA_WAVE) {
    float v = 0.f;
    if (m < nq && f < d) {
      const double qc = (q[(int64_t)m * d + f] - mu[f]) * sc;
      ss += qc * qc;
      v = -2.f * (float)qc;
    } else if (m < nq && f == d) {
      v = 1.f;
    }
    const int qt = m / IA_TILE, j = m % IA_TILE, h = f / KH, s = f % KH;
    qf[(((int64_t)qt * KP + s / 4) * IA_WAVE + h * IA_TILE + j) * 4 + (s % 4)] = v;
  }
  ss = wave_sum_d(ss);
  if (lane == 0 && m < nq) qn2[m] = ss;
}

__global__ void __launch_bounds__(IA_WG) k_merge_dense(MergeArgs ma, const double *__restrict__ pts, int d, const double *__restrict__ q,
                                                        int64_t nq, double dsc, int64_t *__restrict__ idx_out,
                                                        double *__restrict__ dist_out) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= nq) return;
  const double *qm = q + (int64_t)m * d;
  unsigned stat;
  const Winner wn = certified_winner(ma, m, [&](int64_t row) { return row_dist2_rt(pts + row * d, qm, d); }, &stat, dsc);
  if ((threadIdx.x & 63) == 0) {
    idx_out[m] = wn.idx;
    dist_out[m] = wn.d;
  }
}

// exact k-NN of the index (ia_index_query_knn): the certified k nearest rows of each query,
// ascending (distance, row), from the same scan records as k_merge_dense.  counters[0] += rows
// whose exact distance was computed, counters[1] += chunks rescanned (ia_index_knn_stats).
__global__ void __launch_bounds__(IA_WG) k_merge_dense_knn(MergeArgs ma, const double *__restrict__ pts, int d,
                                                            const double *__restrict__ q, int64_t nq, int k, double dsc,
                                                            int64_t *__restrict__ idx_out, double *__restrict__ dist_out,
                                                            unsigned long long *__restrict__ counters) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= nq) return;
  const int lane = threadIdx.x & 63;
  const double *qm = q + (int64_t)m * d;
  double md;
  int64_t mi;
  unsigned long long n_exact, n_rescan;
  certified_topk(ma, m, k, [&](int64_t row) { return row_dist2_rt(pts + row * d, qm, d); }, dsc, md, mi, n_exact, n_rescan);
  if (lane < k) {
    idx_out[(int64_t)m * k + lane] = mi;
    dist_out[(int64_t)m * k + lane] = md;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_exact += __shfl_xor(n_exact, o, 64);
  if (lane == 0) {  // integer sums: order-free
    atomicAdd(&counters[0], n_exact);
    if (n_rescan) atomicAdd(&counters[1], n_rescan);
  }
}

// best_coherence_match (algorithms.py:92-130) for a batch of B' pixels against an index's rows,
// one wave per pixel.  Lane j < (pad+1)(2 pad+1) is the window cell (row - pad + j / (2 pad+1),
// col - pad + j % (2 pad+1)), i.e. product(rows, cols) order (:101-104); a cell is a candidate
// when it is inside the level, raster-earlier (:107) and its shifted source s[r] + (q - r) lies
// inside A (:116).  Distance = sqrt of numpy's pairwise sum of squares (norm(..., axis=1),
// :126), first argmin.  err bit 0: an s index beyond n_s; bit 1: a DB row beyond the index.
__global__ void __launch_bounds__(IA_WG) k_coherence_batch(const double *__restrict__ pts, int64_t n, int d,
                                                            const double *__restrict__ q, int64_t nq,
                                                            const int32_t *__restrict__ px, const int32_t *__restrict__ s,
                                                            const int32_t *__restrict__ im, int64_t n_s, int a_h, int a_w,
                                                            int bp_w, int pad, int32_t *__restrict__ p_out,
                                                            int32_t *__restrict__ img_out, int32_t *__restrict__ r_out,
                                                            unsigned *__restrict__ err) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  const int lane = threadIdx.x & 63;
  if (m >= nq) return;
  const int row = px[2 * m], col = px[2 * m + 1];
  const auto cl = causal_cell(pad, bp_w, row, col, (int64_t)row * bp_w + col, lane);
  const int rr = cl.nr, rc = cl.nc;
  const int64_t ri = cl.nb;
  bool ok = lane < causal_cells(pad) && cl.ok;
  int pr0 = 0, pr1 = 0, img = 0;
  int64_t dbrow = 0;
  unsigned e = 0;
  if (ok && ri >= n_s) {
    e |= 1u;
    ok = false;
  }
  if (ok) {
    const ShiftedSrc t = shifted_src(a_h, a_w, s[2 * ri], s[2 * ri + 1], row, col, rr, rc);
    pr0 = t.tr;
    pr1 = t.tc;
    img = im[ri];
    ok = t.ok;
    dbrow = src_row<int64_t>(a_h, a_w, img, pr0, pr1);
    if (ok && (dbrow < 0 || dbrow >= n)) {
      e |= 2u;
      ok = false;
    }
  }
  double dist = INFINITY;
  int64_t key = ok ? lane : 64;
  if (ok) dist = cr_sqrt(row_dist2_rt(pts + dbrow * d, q + (int64_t)m * d, d));
  if (e) atomicOr(err, e);
  wave_min_di(dist, key);  // first argmin (lowest window cell) among the candidates
  if (key >= 64) {
    if (lane == 0) {
      p_out[2 * m] = -1;
      p_out[2 * m + 1] = -1;
      img_out[m] = 0;
      r_out[2 * m] = 0;
      r_out[2 * m + 1] = 0;
    }
    return;
  }
  if (lane == (int)key) {  // s[r*] + q - r*, im[r*], r*
    p_out[2 * m] = pr0;
    p_out[2 * m + 1] = pr1;
    img_out[m] = img;
    r_out[2 * m] = rr;
    r_out[2 * m + 1] = rc;
  }
}

// microbenchmark operands: pseudo-random f16 values in [-0.5, 0.5) (hash of the index)
__global__ void __launch_bounds__(IA_WG) k_fill_random_f16(_Float16 *__restrict__ p, int64_t n, unsigned seed) {
  for (int64_t i = (int64_t)blockIdx.x * IA_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IA_WG) {
    unsigned h = (unsigned)i * 2654435761u ^ seed;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    p[i] = (_Float16)((float)(h & 0xffff) * (1.f / 65536.f) - 0.5f);
  }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_index.cpp)
// ------------------------------------------------------------------------------------------
void ia_launch_reduce_stats(const unsigned *pstat, int64_t n, unsigned long long *counters, hipStream_t st) {
  const int64_t nwg = std::min<int64_t>(256, std::max<int64_t>(1, cdiv(n, (int64_t)IA_WG * 16)));
  hipLaunchKernelGGL(k_reduce_stats, dim3((unsigned)nwg), dim3(IA_WG), 0, st, pstat, n, counters);
}

void ia_launch_dense_db(int KH, const double *pts, int64_t n, int d, int n_tiles, const double *mu, double sc, float4 *db,
                        unsigned *Rbits, hipStream_t st) {
  dim3 grid(cdiv((int64_t)n_tiles * IA_TILE, IA_WG));
  if (KH == 28) hipLaunchKernelGGL(k_dense_db_build<28>, grid, dim3(IA_WG), 0, st, pts, n, d, n_tiles, mu, sc, db, Rbits);
  else if (KH == 56) hipLaunchKernelGGL(k_dense_db_build<56>, grid, dim3(IA_WG), 0, st, pts, n, d, n_tiles, mu, sc, db, Rbits);
  else hipLaunchKernelGGL(k_dense_db_build<84>, grid, dim3(IA_WG), 0, st, pts, n, d, n_tiles, mu, sc, db, Rbits);
}
void ia_launch_dense_query(int KH, const double *q, int64_t nq, int d, int Mpad, const double *mu, double sc, double *qn2,
                           float *qf, hipStream_t st) {
  dim3 grid(cdiv(Mpad, IA_WG / IA_WAVE));
  if (KH == 28) hipLaunchKernelGGL(k_dense_query<28>, grid, dim3(IA_WG), 0, st, q, nq, d, Mpad, mu, sc, qn2, qf);
  else if (KH == 56) hipLaunchKernelGGL(k_dense_query<56>, grid, dim3(IA_WG), 0, st, q, nq, d, Mpad, mu, sc, qn2, qf);
  else hipLaunchKernelGGL(k_dense_query<84>, grid, dim3(IA_WG), 0, st, q, nq, d, Mpad, mu, sc, qn2, qf);
}
void ia_launch_merge_dense(const MergeArgs &ma, const double *pts, int d, const double *q, int64_t nq, double dsc,
                           int64_t *idx, double *dist, hipStream_t st) {
  hipLaunchKernelGGL(k_merge_dense, dim3(cdiv(nq, IA_WG / IA_WAVE)), dim3(IA_WG), 0, st, ma, pts, d, q, nq, dsc, idx, dist);
}
void ia_launch_merge_dense_knn(const MergeArgs &ma, const double *pts, int d, const double *q, int64_t nq, int k, double dsc,
                               int64_t *idx, double *dist, unsigned long long *counters, hipStream_t st) {
  hipLaunchKernelGGL(k_merge_dense_knn, dim3(cdiv(nq, IA_WG / IA_WAVE)), dim3(IA_WG), 0, st, ma, pts, d, q, nq, k, dsc, idx,
                     dist, counters);
}
void ia_launch_coherence_batch(const double *pts, int64_t n, int d, const double *q, int64_t nq, const int32_t *px,
                               const int32_t *s, const int32_t *im, int64_t n_s, int a_h, int a_w, int bp_w, int pad,
                               int32_t *p_out, int32_t *img_out, int32_t *r_out, unsigned *err, hipStream_t st) {
  hipLaunchKernelGGL(k_coherence_batch, dim3(cdiv(nq, IA_WG / IA_WAVE)), dim3(IA_WG), 0, st, pts, n, d, q, nq, px, s, im, n_s,
                     a_h, a_w, bp_w, pad, p_out, img_out, r_out, err);
}
void ia_launch_fill_random_f16(void *p, int64_t n, unsigned seed, hipStream_t st) {
  hipLaunchKernelGGL(k_fill_random_f16, dim3(1024), dim3(IA_WG), 0, st, (_Float16 *)p, n, seed);
}

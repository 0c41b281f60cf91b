// ia_ann.hip — the approximate index (ia_ann_*, ia_kmeans): a deterministic k-means
// inverted file.  Every distance is row_dist2_rt (ia_dev.h): fp64, numpy's pairwise order, so the
// numpy restatement (tests/ann_inputs.py) pins every kernel bit for bit.
//
//   k_ann_assign   per row the centre of smallest (distance, centre index), a row per lane; the row
//                  tile (transposed) and blocks of centres in LDS
//   k_ann_update   one thread per (list, column): the list's rows added in ascending row order,
//                  one divide (np.add.accumulate(pts[rows])[-1] / len(rows)); an empty list keeps its centre
//   k_ann_permute  the list-major copy of the rows
//   k_ann_query    one workgroup per query: centre distances, a bitonic sort of (distance, centre)
//                  in LDS, a prefix over the list sizes in that order, the probed lists' rows through
//                  topk_offer (ia_topk.h) per wave, the waves' lists merged through LDS
//
// Plain launches, no waits inside a kernel; the only atomics are the integer statistics.
#include "ia_dev.h"
#include "ia_launch.h"
#include "ia_topk.h"

#define IA_ANN_CB 16    // centres staged per block of k_ann_assign
#define IA_ANN_QWG 256  // k_ann_query: four waves per query

__global__ void k_ann_assign(const double *__restrict__ pts, int64_t n, int d, const double *__restrict__ cent, int L,
                             int32_t *__restrict__ assign) {
  extern __shared__ double ann_lds[];
  const int BS = blockDim.x, tid = threadIdx.x;
  double *rowsT = ann_lds;               // [d][BS]: lane tid reads its row at stride BS, conflict-free
  double *cs = ann_lds + (size_t)d * BS;  // [IA_ANN_CB][d]
  const int64_t r0 = (int64_t)blockIdx.x * BS;
  const int64_t tile = min((int64_t)BS, n - r0) * d;  // the block's rows are contiguous in pts
  for (int e = tid; e < BS * d; e += BS) {
    const int row = e / d, f = e - row * d;
    rowsT[(size_t)f * BS + row] = e < tile ? pts[r0 * d + e] : 0.;
  }
  double best = INFINITY;
  int bc = 0;
  for (int c0 = 0; c0 < L; c0 += IA_ANN_CB) {
    const int cn = min(IA_ANN_CB, L - c0);
    __syncthreads();
    for (int e = tid; e < cn * d; e += BS) cs[e] = cent[(int64_t)c0 * d + e];
    __syncthreads();
    for (int c = 0; c < cn; c++) {
      const double *cc = cs + c * d;
      const double v = pw_sum_rt([&](int f) {
        const double x = cc[f] - rowsT[(size_t)f * BS + tid];
        return x * x;
      }, d);
      if (v < best) {  // ascending centres: an exact tie stays with the lower one
        best = v;
        bc = c0 + c;
      }
    }
  }
  if (r0 + tid < n) assign[r0 + tid] = bc;
}

__global__ void __launch_bounds__(256) k_ann_update(const double *__restrict__ pts, int d, const int32_t *__restrict__ rows,
                                                    const int32_t *__restrict__ off, int L, double *__restrict__ cent) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // adjacent threads, adjacent columns
  if (t >= (int64_t)L * d) return;
  const int c = (int)(t / d), f = (int)(t - (int64_t)c * d);
  const int64_t i0 = off[c], i1 = off[c + 1];  // 64-bit walks: i + 4 and b + lane stay exact at n = 2^31 - 1
  if (i0 == i1) return;
  double s = pts[(int64_t)rows[i0] * d + f];
  int64_t i = i0 + 1;
  for (; i + 4 <= i1; i += 4) {  // four loads in flight, added in row order
    const double v0 = pts[(int64_t)rows[i] * d + f], v1 = pts[(int64_t)rows[i + 1] * d + f];
    const double v2 = pts[(int64_t)rows[i + 2] * d + f], v3 = pts[(int64_t)rows[i + 3] * d + f];
    s += v0;
    s += v1;
    s += v2;
    s += v3;
  }
  for (; i < i1; i++) s += pts[(int64_t)rows[i] * d + f];
  cent[t] = s / (double)(i1 - i0);
}

__global__ void __launch_bounds__(256) k_ann_permute(const double *__restrict__ pts, int d, const int32_t *__restrict__ rows,
                                                     int64_t n, double *__restrict__ out) {
  const int64_t total = n * d;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / d;
    out[e] = pts[(int64_t)rows[i] * d + (e - i * d)];
  }
}

// rows: list-major n x d; ids: their row indices; off: L + 1 list offsets; centT: d x L (lane c reads
// centre c coalesced); P: L rounded up to a power of two; need: rows to take (host: n, or
// min(n, max(checks, k))).  counters[0] += rows taken, counters[1] += lists probed.
__global__ void __launch_bounds__(IA_ANN_QWG) k_ann_query(const double *__restrict__ rows, const int32_t *__restrict__ ids,
                                                          const int32_t *__restrict__ off, const double *__restrict__ centT,
                                                          int L, int P, int d, const double *__restrict__ q, int k, int need,
                                                          int64_t *__restrict__ idx_out, double *__restrict__ dist_out,
                                                          unsigned long long *__restrict__ counters) {
  extern __shared__ double ann_lds[];
  constexpr int NW = IA_ANN_QWG / IA_WAVE;
  double *sd = ann_lds;                                         // [P] centre distances
  double *qs = sd + P;                                          // [d] the query
  double *wd = qs + d;                                          // [(NW - 1) * 64] the other waves' lists
  int64_t *wi = reinterpret_cast<int64_t *>(wd + (NW - 1) * 64);  // [(NW - 1) * 64]
  int *si = reinterpret_cast<int *>(wi + (NW - 1) * 64);          // [P] centre indices
  __shared__ int s_np;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int f = tid; f < d; f += IA_ANN_QWG) qs[f] = q[(int64_t)m * d + f];
  __syncthreads();
  for (int c = tid; c < P; c += IA_ANN_QWG) {
    double v = INFINITY;  // padding sorts behind every centre
    if (c < L)
      v = pw_sum_rt([&](int f) {
        const double x = centT[(int64_t)f * L + c] - qs[f];
        return x * x;
      }, d);
    sd[c] = v;
    si[c] = c;
  }
  __syncthreads();
  // bitonic sort, ascending (distance, centre): the keys are distinct
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += IA_ANN_QWG) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const double di = sd[i], dl = sd[l];
        const int ii = si[i], il = si[l];
        const bool up = (i & k2) == 0;
        if ((dl < di || (dl == di && il < ii)) == up) {
          sd[i] = dl;
          sd[l] = di;
          si[i] = il;
          si[l] = ii;
        }
      }
      __syncthreads();
    }
  // lists are taken whole, in that order, while fewer than need rows are taken (need <= n: it ends)
  if (wave == 0) {
    int cum = 0, np = L, taken = 0;
    for (int base = 0; base < L; base += IA_WAVE) {
      const int i = base + lane;
      int inc = 0;
      if (i < L) {
        const int c = si[i];
        inc = off[c + 1] - off[c];
      }
      for (int o = 1; o < IA_WAVE; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      const unsigned long long mask = __ballot(cum + inc >= need);
      if (mask) {
        const int j = __ffsll((long long)mask) - 1;
        np = base + j + 1;
        taken = cum + __shfl(inc, j, 64);
        break;
      }
      cum += __shfl(inc, 63, 64);
    }
    if (lane == 0) {
      s_np = np;
      atomicAdd(&counters[0], (unsigned long long)taken);
      atomicAdd(&counters[1], (unsigned long long)np);
    }
  }
  __syncthreads();
  const int np = s_np;
  double md = DBL_MAX;
  int64_t mi = INT64_MAX;
  for (int i = 0; i < np; i++) {  // the waves stride over each probed list, a row per lane
    const int c = si[i];
    const int64_t i0 = off[c], i1 = off[c + 1];
    for (int64_t b = i0 + wave * IA_WAVE; b < i1; b += NW * IA_WAVE) {
      const int64_t p = b + lane;
      const bool has = p < i1;
      double cd = DBL_MAX;
      int64_t ci = INT64_MAX;
      if (has) {
        cd = row_dist2_rt(rows + p * d, qs, d);
        ci = ids[p];
      }
      topk_offer(md, mi, cd, ci, has, k);
    }
  }
  if (wave > 0) {
    wd[(wave - 1) * 64 + lane] = md;
    wi[(wave - 1) * 64 + lane] = mi;
  }
  __syncthreads();
  if (wave == 0) {
    for (int w = 0; w < NW - 1; w++) {
      const double cd = wd[w * 64 + lane];
      const int64_t ci = wi[w * 64 + lane];
      topk_offer(md, mi, cd, ci, ci != INT64_MAX, k);
    }
    if (lane < k) {
      idx_out[(int64_t)m * k + lane] = mi;
      dist_out[(int64_t)m * k + lane] = md;
    }
  }
}

// rows of a k_ann_assign workgroup: as many waves (<= 4) as keep the row tile under 96 KiB
static int ann_assign_bs(int d) { return IA_WAVE * std::max(1, std::min(4, (96 * 1024) / (IA_WAVE * d * 8))); }

void ia_launch_ann_assign(const double *pts, int64_t n, int d, const double *cent, int L, int32_t *assign, hipStream_t st) {
  const int BS = ann_assign_bs(d);
  const size_t lds = ((size_t)d * BS + (size_t)IA_ANN_CB * d) * 8;
  ia_allow_full_lds((const void *)k_ann_assign);
  hipLaunchKernelGGL(k_ann_assign, dim3(cdiv(n, BS)), dim3(BS), lds, st, pts, n, d, cent, L, assign);
}
void ia_launch_ann_update(const double *pts, int d, const int32_t *rows, const int32_t *off, int L, double *cent,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_ann_update, dim3(cdiv((int64_t)L * d, 256)), dim3(256), 0, st, pts, d, rows, off, L, cent);
}
void ia_launch_ann_permute(const double *pts, int d, const int32_t *rows, int64_t n, double *out, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n * d, 256), 1 << 16);
  hipLaunchKernelGGL(k_ann_permute, dim3(grid), dim3(256), 0, st, pts, d, rows, n, out);
}
void ia_launch_ann_query(const double *rows, const int32_t *ids, const int32_t *off, const double *centT, int L, int d,
                         const double *q, int nq, int k, int need, int64_t *idx, double *dist, unsigned long long *counters,
                         hipStream_t st) {
  int P = 1;
  while (P < L) P <<= 1;
  constexpr int NW = IA_ANN_QWG / IA_WAVE;
  const size_t lds = ((size_t)P + d + (NW - 1) * 64) * 8 + (size_t)(NW - 1) * 64 * 8 + (size_t)P * 4;  // <= 54 KiB at L = 4096
  hipLaunchKernelGGL(k_ann_query, dim3(nq), dim3(IA_ANN_QWG), lds, st, rows, ids, off, centT, L, P, d, q, k, need, idx, dist,
                     counters);
}

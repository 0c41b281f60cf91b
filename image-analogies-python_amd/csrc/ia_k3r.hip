// ia_k3r.hip — the exact fixed-radius search of the FLANN-compatible index (ia_index_count_radius,
// ia_index_query_radius; host side ia_index_radius.cpp; DESIGN.md §5 "Radius queries"):
//
//   k3r_thresholds  per query two fp32 thresholds on the scan's MFMA value: every row inside the
//                   radius has value <= hi, every row with value <= lo is inside
//   k3r_count       K3's scan (ia_k3_scan.h k3_scan, the body k3_dist runs: one text, so the same
//                   geometry and MFMA chain) with a threshold test for epilogue: per (query,
//                   workgroup) the number of values <= lo and <= hi
//   k3r_offsets     per query the prefix sums of its workgroups' counts: private output segments
//   k3r_fill        the same scan again; a hit takes the next slot of its workgroup's segment
//   k3r_verify      the exact fp64 distance (numpy's pairwise order) of every appended (query, row)
//   k3r_finish      per query: bitonic sort by (distance, row), count, write-out
//
// Two scan passes and private segments instead of one pass that appends through global counters:
// no global atomic anywhere (the only atomics are LDS slot counters), so the counts are
// deterministic and the candidates of one query are contiguous for the sort.
#include "ia_dev.h"
#include "ia_k3_scan.h"
#include "ia_launch.h"

#define IA_R_LO_MAX 1.0e29  // lo never reaches IA_PAD_NORM: a padding row is never "certainly inside"
#define IA_R_SORT_LDS 4096  // entries of the longest segment sorted in LDS (48 KiB)

// ------------------------------------------------------------------------------------------
// thresholds.  Scaled units (ia_dense.hip): r' = radius sc^2, a row's MFMA value v = |a'|^2 -
// 2 q'.a' = D' - |q'|^2 within merge_eps(|a'| bound, |q'|), D' its exact scaled distance.
//   inside (D' < r')  =>  |a'| <= |q'| + sqrt(r')  =>  v <= r' - |q'|^2 + merge_eps(Rl, |q'|)  = hi
//   v <= r' - |q'|^2 - merge_eps(R, |q'|) = lo     =>  D' < r'
// Every rounding goes outward: r' up for hi and down for lo where the product with sc^2 is inexact
// (underflow) or overflows, 1e-13 (r' + |q'|^2 + 1) for the fp64 roundings of |q'|^2, of the
// threshold itself and of numpy's distance sum, hi up to fp32 and lo down.  hi is clamped to
// FLT_MAX (radius +inf: every finite value), lo to IA_R_LO_MAX.  Padding queries: nothing hits.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(IA_WG) k3r_thresholds(const double *__restrict__ radius, const double *__restrict__ qn2,
                                                         const unsigned *__restrict__ Rbits, int nq, int Mpad, double dsc,
                                                         double eps_c, float2 *__restrict__ thr) {
  const int m = blockIdx.x * IA_WG + threadIdx.x;
  if (m >= Mpad) return;
  float hi = -FLT_MAX, lo = -FLT_MAX;
  if (m < nq) {
    MergeArgs a;
    a.eps_c = eps_c;
    a.eps_a = 0.;
    const double R = (double)__uint_as_float(*Rbits);
    const double r = radius[m], q2 = qn2[m], qn = sqrt(q2);
    double ru = r * dsc, rd = r * dsc;
    if (ru / dsc < r) ru = nextafter(ru, (double)INFINITY);
    if (rd / dsc > r) rd = nextafter(rd, -(double)INFINITY);
    rd = fmin(rd, 1e300);  // (keeps lo's arithmetic finite; lo is clamped far below anyway)
    const double Rl = fmin(R, (qn + sqrt(ru)) * (1.0 + 1e-12) + 1e-12);
    const double h = ru - q2 + merge_eps(a, Rl, qn) + 1e-13 * (ru + q2 + 1.0);
    const double l = fmin(rd - q2 - merge_eps(a, R, qn) - 1e-13 * (rd + q2 + 1.0), IA_R_LO_MAX);
    hi = h >= (double)FLT_MAX ? FLT_MAX : fmaxf(round_up_f(h), -FLT_MAX);
    lo = l <= -(double)FLT_MAX ? -FLT_MAX : round_down_f(l);
  }
  thr[m] = make_float2(hi, lo);
}

// ------------------------------------------------------------------------------------------
// the scan: ia_k3_scan.h's k3_scan (k3_dist's own body: geometry and C layout there) with a
// threshold epilogue.  Per accumulator: the minimum of its 16 values against the lane's hi;
// hit(acc, q, m, pbase) runs, wave-uniformly, only where some lane has a value <= hi (m: this
// lane's minimum, pbase: the position of acc[0]).
// ------------------------------------------------------------------------------------------
template <int KH, int QT, class Hit>
__device__ __forceinline__ void k3r_scan(const float4 *__restrict__ db, const float4 *lds, int n_tiles, int tpw,
                                         const float (&hi)[QT], Hit &&hit) {
  k3_scan<KH, QT>(db, lds, n_tiles, tpw, [&](const f32x16 &acc, int q, int pbase) {
    float m = fminf(fminf(acc[0], acc[1]), acc[2]);  // v_min3_f32 chain
#pragma unroll
    for (int r = 3; r < 15; r += 2) m = fminf(fminf(m, acc[r]), acc[r + 1]);
    m = fminf(m, acc[15]);
    if (__any(m <= hi[q])) hit(acc, q, m, pbase);
  });
}

// pass 1: cnt[q nwg + wg] = (values <= lo, values <= hi) of query q in workgroup wg's tiles
template <int KH, int QT>
__global__ void __launch_bounds__(IA_WG, 2)
k3r_count(const float4 *__restrict__ db, const float4 *__restrict__ qf, const float2 *__restrict__ thr, int n_tiles, int tpw,
          int qt0, int M, int nwg, uint2 *__restrict__ cnt) {
  extern __shared__ float4 lds[];  // QT * KP * 64 float4 (queries), reused for the reduction
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  k3_stage<KH, QT>(qf, qt0, lds);
  float hi[QT];
  unsigned nlo[QT], nhi[QT];
#pragma unroll
  for (int q = 0; q < QT; q++) {
    hi[q] = thr[(qt0 + q) * IA_TILE + (lane & 31)].x;
    nlo[q] = 0;
    nhi[q] = 0;
  }
  k3r_scan<KH, QT>(db, lds, n_tiles, tpw, hi, [&](const f32x16 &acc, int q, float, int) {
    const float lo = thr[(qt0 + q) * IA_TILE + (lane & 31)].y;  // only here: not worth a register per tile
#pragma unroll
    for (int r = 0; r < 16; r++) {
      nhi[q] += acc[r] <= hi[q] ? 1u : 0u;
      nlo[q] += acc[r] <= lo ? 1u : 0u;
    }
  });
  // ---- lane halves by shuffle, the 4 waves through LDS
  __syncthreads();  // queries no longer needed: reuse LDS
  uint2 *red = reinterpret_cast<uint2 *>(lds);  // [4 waves][QT][32]
#pragma unroll
  for (int q = 0; q < QT; q++) {
    const unsigned l = nlo[q] + __shfl_xor(nlo[q], 32, 64), h = nhi[q] + __shfl_xor(nhi[q], 32, 64);
    if (half == 0) red[(wave * QT + q) * IA_TILE + lane] = make_uint2(l, h);
  }
  __syncthreads();
  for (int x = threadIdx.x; x < QT * IA_TILE; x += IA_WG) {
    uint2 s = red[x];
#pragma unroll
    for (int w = 1; w < 4; w++) {
      const uint2 o = red[(w * QT) * IA_TILE + x];
      s.x += o.x;
      s.y += o.y;
    }
    const int qg = qt0 * IA_TILE + x;
    if (qg < M) cnt[(int64_t)qg * nwg + blockIdx.x] = s;
  }
}

// per query (one wave): seg[q nwg + wg] = (start, length) of workgroup wg's segment inside the
// query's candidates, ts[q] = (candidates, rows certainly inside that are not appended).
// count_only: the candidates are the boundary rows lo < v <= hi, else every row v <= hi.
__global__ void __launch_bounds__(IA_WG) k3r_offsets(const uint2 *__restrict__ cnt, int nq, int nwg, int count_only,
                                                      uint2 *__restrict__ seg, uint2 *__restrict__ ts) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= nq) return;
  const int lane = threadIdx.x & 63;
  unsigned run = 0, sure = 0;
  for (int w0 = 0; w0 < nwg; w0 += IA_WAVE) {
    const int w = w0 + lane;
    const uint2 c = w < nwg ? cnt[(int64_t)m * nwg + w] : make_uint2(0u, 0u);
    const unsigned len = count_only ? c.y - c.x : c.y;
    unsigned x = len;  // inclusive prefix sum over the wave
#pragma unroll
    for (int o = 1; o < IA_WAVE; o <<= 1) {
      const unsigned u = __shfl_up(x, o, 64);
      if (lane >= o) x += u;
    }
    if (w < nwg) seg[(int64_t)m * nwg + w] = make_uint2(run + x - len, len);
    run += __shfl(x, 63, 64);
    sure += count_only ? c.x : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sure += __shfl_xor(sure, o, 64);
  if (lane == 0) ts[m] = make_uint2(run, sure);
}

// pass 2 over the queries [j0, j1) of the batch (every other query of a loaded tile: hi =
// -FLT_MAX): a hit takes slot seg[(q, wg)].start + (LDS counter of q)++ of the query's candidates,
// which start at qoff[q] in cand, and stores its tile position.  The same MFMA chain (k3_scan, one
// text for both passes) on the same operands as pass 1 gives the same values, so the counter ends
// at the segment's length; a slot beyond it is dropped all the same (never written).
template <int KH, int QT, bool COUNT_ONLY>
__global__ void __launch_bounds__(IA_WG, 2)
k3r_fill(const float4 *__restrict__ db, const float4 *__restrict__ qf, const float2 *__restrict__ thr, int n_tiles, int tpw,
         int qt0, int j0, int j1, int nwg, const uint2 *__restrict__ seg, const unsigned *__restrict__ qoff,
         int *__restrict__ cand) {
  constexpr int KP = KH / 4;
  extern __shared__ float4 lds[];  // QT * KP * 64 float4 (queries), then QT * 32 slot counters
  unsigned *slot = reinterpret_cast<unsigned *>(lds + QT * KP * IA_WAVE);
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < QT * IA_TILE; i += IA_WG) slot[i] = 0u;
  k3_stage<KH, QT>(qf, qt0, lds);
  float hi[QT];
#pragma unroll
  for (int q = 0; q < QT; q++) {
    const int qg = (qt0 + q) * IA_TILE + (lane & 31);
    hi[q] = qg >= j0 && qg < j1 ? thr[qg].x : -FLT_MAX;
  }
  k3r_scan<KH, QT>(db, lds, n_tiles, tpw, hi, [&](const f32x16 &acc, int q, float m, int pbase) {
    if (m <= hi[q]) {  // (a lane with hi = -FLT_MAX never gets here: its qoff is not set)
      const int qg = (qt0 + q) * IA_TILE + (lane & 31);
      const float lo = COUNT_ONLY ? thr[qg].y : -FLT_MAX;
      const uint2 sg = seg[(int64_t)qg * nwg + blockIdx.x];
      int *dst = cand + ((size_t)qoff[qg] + sg.x);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        if (acc[r] <= hi[q] && (!COUNT_ONLY || acc[r] > lo)) {
          const unsigned s = atomicAdd(&slot[q * IA_TILE + (lane & 31)], 1u);  // LDS, ds_add_rtn_u32
          if (s < sg.y) dst[s] = pbase + (r & 3) + 8 * (r >> 2);
        }
      }
    }
  });
}

// exact fp64 distance of every candidate of the queries [j0, j0 + gridDim.x): (position) ->
// (distance, row), or (+inf, INT32_MAX) for a row outside the radius and for a padding position
__global__ void __launch_bounds__(IA_WG) k3r_verify(const double *__restrict__ pts, int64_t n, int d, int NT,
                                                     const double *__restrict__ q, const double *__restrict__ radius,
                                                     const uint2 *__restrict__ ts, const unsigned *__restrict__ qoff, int j0,
                                                     int *__restrict__ wr, double *__restrict__ wd) {
  const int m = j0 + blockIdx.x;
  const unsigned len = ts[m].x;
  const size_t base = qoff[m];
  const double *qm = q + (int64_t)m * d;
  const double rad = radius[m];
  for (unsigned i = blockIdx.y * IA_WG + threadIdx.x; i < len; i += gridDim.y * IA_WG) {
    const int pos = wr[base + i];
    double dd = INFINITY;
    int rr = INT32_MAX;
    if ((unsigned)pos < (unsigned)NT * IA_TILE) {
      const int64_t row = ia_pos_row(pos, NT);
      if (row < n) {
        const double x2 = row_dist2_rt(pts + row * d, qm, d);
        if (x2 < rad) {
          dd = x2;
          rr = (int)row;
        }
      }
    }
    wd[base + i] = dd;
    wr[base + i] = rr;
  }
}

// ascending bitonic sort of len (distance, row) pairs by one workgroup, as a network of N = 2^k >=
// len inputs whose comparators all point the same way (the first step of each stage mirrors its
// block): the inputs beyond len are +inf, stay where they are and are never touched
__device__ void k3r_sort(double *kd, int *kr, unsigned len, int logN) {
  const unsigned half_n = 1u << (logN - 1);
  for (int lk = 1; lk <= logN; lk++) {
    for (int lj = lk - 1; lj >= 0; lj--) {
      const unsigned j = 1u << lj;
      for (unsigned t = threadIdx.x; t < half_n; t += IA_WG) {
        const unsigned off = t & (j - 1), i = ((t >> lj) << (lj + 1)) + off;
        const unsigned l = lj == lk - 1 ? i - off + 2 * j - 1 - off : i + j;
        if (l < len) {
          const double di = kd[i], dl = kd[l];
          const int ri = kr[i], rl = kr[l];
          if (dl < di || (dl == di && rl < ri)) {
            kd[i] = dl; kr[i] = rl;
            kd[l] = di; kr[l] = ri;
          }
        }
      }
      __syncthreads();
    }
  }
}

// per query of [j0, j0 + gridDim.x), one workgroup.  COUNT_ONLY: count = certainly-inside rows +
// verified boundary rows.  Else: sort the candidates (in LDS up to IA_R_SORT_LDS, in place in global
// memory beyond: cold), count = the finite ones, and the nearest min(capacity, count) go to the
// staging arrays at soff[q] (capacity = soff[q + 1] - soff[q], already <= the candidates).
template <bool COUNT_ONLY>
__global__ void __launch_bounds__(IA_WG) k3r_finish(const uint2 *__restrict__ ts, const unsigned *__restrict__ qoff,
                                                     const unsigned *__restrict__ soff, int j0, int *__restrict__ wr,
                                                     double *__restrict__ wd, int64_t *__restrict__ sidx,
                                                     double *__restrict__ sdist, int64_t *__restrict__ cntq) {
  __shared__ double kd[COUNT_ONLY ? 1 : IA_R_SORT_LDS];
  __shared__ int kr[COUNT_ONLY ? 1 : IA_R_SORT_LDS];
  __shared__ unsigned total;
  const int m = j0 + blockIdx.x;
  const unsigned len = ts[m].x;
  const size_t base = len ? qoff[m] : 0;
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  double *sd = wd + base;
  int *sr = wr + base;
  if constexpr (!COUNT_ONLY) {
    if (len > 1) {
      int logN = 1;
      while ((1ull << logN) < len) logN++;
      if (len <= IA_R_SORT_LDS) {
        for (unsigned i = threadIdx.x; i < len; i += IA_WG) {
          kd[i] = sd[i];
          kr[i] = sr[i];
        }
        __syncthreads();
        k3r_sort(kd, kr, len, logN);
        sd = kd;
        sr = kr;
      } else {
        k3r_sort(sd, sr, len, logN);
      }
    }
  }
  unsigned mine = 0;
  for (unsigned i = threadIdx.x; i < len; i += IA_WG) mine += sr[i] != INT32_MAX ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&total, mine);  // LDS
  __syncthreads();
  const unsigned count = total;
  if (threadIdx.x == 0) cntq[m] = (int64_t)count + (COUNT_ONLY ? (int64_t)ts[m].y : 0);
  if constexpr (!COUNT_ONLY) {
    const unsigned so = soff[m], take = min(soff[m + 1] - so, count);
    for (unsigned i = threadIdx.x; i < take; i += IA_WG) {  // sorted: the finite entries come first
      sidx[(size_t)so + i] = sr[i];
      sdist[(size_t)so + i] = sd[i];
    }
  }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_index_radius.cpp)
// ------------------------------------------------------------------------------------------
typedef void (*k3r_count_fn)(const float4 *, const float4 *, const float2 *, int, int, int, int, int, uint2 *);
typedef void (*k3r_fill_fn)(const float4 *, const float4 *, const float2 *, int, int, int, int, int, int, const uint2 *,
                            const unsigned *, int *);
template <int KH, int... QTs>
struct K3rTable {
  static k3r_count_fn count(int qt) {
    static const k3r_count_fn tab[] = {k3r_count<KH, QTs>...};
    return tab[qt - 1];
  }
  template <bool CO>
  static k3r_fill_fn fill(int qt) {
    static const k3r_fill_fn tab[] = {k3r_fill<KH, QTs, CO>...};
    return tab[qt - 1];
  }
};
typedef K3rTable<28, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11> K3rT28;  // ia_k3_qtmax's tables
typedef K3rTable<56, 1, 2, 3, 4, 5> K3rT56;
typedef K3rTable<84, 1, 2, 3> K3rT84;

void ia_launch_k3r_thresholds(const double *radius, const double *qn2, const unsigned *Rbits, int nq, int Mpad, double dsc,
                              double eps_c, float2 *thr, hipStream_t st) {
  hipLaunchKernelGGL(k3r_thresholds, dim3(cdiv(Mpad, IA_WG)), dim3(IA_WG), 0, st, radius, qn2, Rbits, nq, Mpad, dsc, eps_c,
                     thr);
}

void ia_launch_k3r_count(int KH, int qt, const float4 *db, const float4 *qf, const float2 *thr, int n_tiles, int tpw, int qt0,
                         int M, int nwg, uint2 *cnt, hipStream_t st) {
  const k3r_count_fn fn = KH == 28 ? K3rT28::count(qt) : KH == 56 ? K3rT56::count(qt) : K3rT84::count(qt);
  const size_t lds = (size_t)qt * (KH / 4) * IA_WAVE * sizeof(float4);
  ia_allow_full_lds((const void *)fn);
  hipLaunchKernelGGL(fn, dim3(nwg), dim3(IA_WG), lds, st, db, qf, thr, n_tiles, tpw, qt0, M, nwg, cnt);
}

void ia_launch_k3r_offsets(const uint2 *cnt, int nq, int nwg, bool count_only, uint2 *seg, uint2 *ts, hipStream_t st) {
  hipLaunchKernelGGL(k3r_offsets, dim3(cdiv(nq, IA_WG / IA_WAVE)), dim3(IA_WG), 0, st, cnt, nq, nwg, count_only ? 1 : 0, seg,
                     ts);
}

void ia_launch_k3r_fill(int KH, int qt, bool count_only, const float4 *db, const float4 *qf, const float2 *thr, int n_tiles,
                        int tpw, int qt0, int j0, int j1, int nwg, const uint2 *seg, const unsigned *qoff, int *cand,
                        hipStream_t st) {
  k3r_fill_fn fn;
  if (count_only) fn = KH == 28 ? K3rT28::fill<true>(qt) : KH == 56 ? K3rT56::fill<true>(qt) : K3rT84::fill<true>(qt);
  else fn = KH == 28 ? K3rT28::fill<false>(qt) : KH == 56 ? K3rT56::fill<false>(qt) : K3rT84::fill<false>(qt);
  const size_t lds = (size_t)qt * (KH / 4) * IA_WAVE * sizeof(float4) + (size_t)qt * IA_TILE * sizeof(unsigned);
  ia_allow_full_lds((const void *)fn);
  hipLaunchKernelGGL(fn, dim3(nwg), dim3(IA_WG), lds, st, db, qf, thr, n_tiles, tpw, qt0, j0, j1, nwg, seg, qoff, cand);
}

void ia_launch_k3r_verify(const double *pts, int64_t n, int d, int NT, const double *q, const double *radius, const uint2 *ts,
                          const unsigned *qoff, int j0, int j1, unsigned max_len, int *wr, double *wd, hipStream_t st) {
  const unsigned gy = std::min(64u, std::max(1u, cdiv(max_len, IA_WG)));
  hipLaunchKernelGGL(k3r_verify, dim3(j1 - j0, gy), dim3(IA_WG), 0, st, pts, n, d, NT, q, radius, ts, qoff, j0, wr, wd);
}

void ia_launch_k3r_finish(bool count_only, const uint2 *ts, const unsigned *qoff, const unsigned *soff, int j0, int j1,
                          int *wr, double *wd, int64_t *sidx, double *sdist, int64_t *cntq, hipStream_t st) {
  if (count_only)
    hipLaunchKernelGGL(k3r_finish<true>, dim3(j1 - j0), dim3(IA_WG), 0, st, ts, qoff, soff, j0, wr, wd, sidx, sdist, cntq);
  else
    hipLaunchKernelGGL(k3r_finish<false>, dim3(j1 - j0), dim3(IA_WG), 0, st, ts, qoff, soff, j0, wr, wd, sidx, sdist, cntq);
}
int ia_k3r_sort_lds() { return IA_R_SORT_LDS; }

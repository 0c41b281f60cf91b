// ia_kcoh.hip — k-coherence search (include/ia.h ia_synthesize_levels_kcoh): one
// wavefront step of a level that runs without a DB scan, and the pre-pass that checks the
// similarity sets.  One wave per query pixel, like K4: the wave gathers its query (BBp_feat) into
// LDS, lists the base rows (the shifted sources of the causal neighbours, best_coherence_match's
// cells) and their K similar rows, computes each candidate's exact fp64 distance in numpy's
// pairwise order, takes the smallest (distance, row) as the approximate match and finishes the
// pixel with K4's coherence pick, kappa rule and writeback (ia_certify.h finish_pixel).
//
// A pixel without a base row needs the exact NN over the whole fp64 row DB.  One wave takes about
// 40 ms for that at 2^20 rows (measured: a handful of such pixels cost more than the level's 4,093
// steps), so the launch carries H scan waves behind its pixel waves.  Every scan wave works out,
// from the same s / im the pixel waves read, which pixels of the step have no base row (almost
// always none: it then ends); for each it scans its 1/H of the rows, stores its (distance, row)
// minimum and counts itself in.  The wave that counts in last - nothing waits, nothing spins -
// reduces the H minima (the lexicographic minimum: independent of the order) and finishes the
// pixel; the pixel's own wave ended when it found no base row.
#include "ia_certify.h"
#include "ia_launch.h"

// exact_dist_level with the row known to be 16-byte aligned (Geo::DS is a multiple of 8 doubles),
// so the loads pair up as double2; the summation order is pw_sum's
template <int CH>
__device__ __forceinline__ double kcoh_dist(const double *__restrict__ db64, int64_t row, const double *q) {
  const double *a = static_cast<const double *>(__builtin_assume_aligned(db64 + row * Geo<CH>::DS, 16));
  return pw_sum<Geo<CH>::D>([&](int f) {
    const double d = a[f] - q[f];
    return d * d;
  });
}

// the base row of causal cell k < 15 (coherence_pick's) of pixel (r, c), raster index qi: the
// neighbour's source shifted by the offset, or -1 (no such neighbour before qi, or the shifted
// source outside A)
__device__ __forceinline__ int kcoh_base_row(const LevelGeo &g, const int32_t *__restrict__ s, const int32_t *__restrict__ im,
                                             int r, int c, int qi, int k) {
  const auto n = causal_cell(Pad2{}, g.bw, r, c, qi, k);
  if (!n.ok) return -1;
  const ShiftedSrc t = shifted_src(g.ah, g.aw, s[2 * n.nb], s[2 * n.nb + 1], r, c, n.nr, n.nc);
  return t.ok ? src_row(g.ah, g.aw, im[n.nb], t.tr, t.tc) : -1;
}
// the pixel has a base row; cell 11, the left neighbour, first: it settles nearly every pixel
__device__ __forceinline__ bool kcoh_has_base(const LevelGeo &g, const int32_t *__restrict__ s, const int32_t *__restrict__ im,
                                              int r, int c, int qi) {
  if (kcoh_base_row(g, s, im, r, c, qi, 11) >= 0) return true;
  for (int k = 0; k < causal_cells(Pad2{}); k++)
    if (kcoh_base_row(g, s, im, r, c, qi, k) >= 0) return true;
  return false;
}

// the scan waves' state: H of them, part[m H + h] the minimum of wave h for query m of the step,
// cnt[m] the waves that stored theirs (zero between steps: the last one clears it)
struct KcohScan {
  int H;
  Winner *part;
  unsigned *cnt;
};

template <int CH, class JS>
__device__ __forceinline__ void kcoh_gather(const LevelGeo &g, Imgs B, const JS &jobs, const QPix &px, const JobPtrs &jp,
                                            int lane, double *q) {
  if constexpr (!JS::single) B = job_imgs(B, jp);  // single job: B already holds its images
  for (int f = lane; f < Geo<CH>::D; f += IA_WAVE) q[f] = win_feat(Geo<CH>{}, B, f, px.r, px.c, 0);
  __builtin_amdgcn_wave_barrier();  // written by this wave's lanes, read by all of them
}

// scan wave h's share of query m, a pixel without a base row
template <int CH, class JS>
__device__ void kcoh_scan_pixel(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const Imgs &B, const JS &jobs,
                                const double *__restrict__ db64, const KcohScan &ks, int m, int h, int lane, double *q) {
  const QPix px = ia_qpix(sd, g.bw, m);
  const JobPtrs jp = jobs.get(px.job);
  __builtin_amdgcn_wave_barrier();  // the previous pixel's reads of q are done
  kcoh_gather<CH>(g, B, jobs, px, jp, lane, q);
  const int64_t chunk = (g.NA + ks.H - 1) / ks.H, r0 = (int64_t)h * chunk, r1 = min(g.NA, r0 + chunk);
  double bd = DBL_MAX;
  int64_t bi = INT64_MAX;
  for (int64_t row = r0 + lane; row < r1; row += IA_WAVE) {
    const double d = kcoh_dist<CH>(db64, row, q);
    if (d < bd || (d == bd && row < bi)) { bd = d; bi = row; }
  }
  wave_min_di(bd, bi);
  unsigned before = 0;
  if (lane == 0) {
    ks.part[(int64_t)m * ks.H + h] = Winner{bd, bi};
    __threadfence();  // the minimum is visible on the device before this wave counts in
    before = atomicAdd(&ks.cnt[m], 1u);
  }
  if (__builtin_amdgcn_readfirstlane(before) != (unsigned)ks.H - 1u) return;
  // the last wave in: every other wave's minimum was stored before its count
  __threadfence();
  bd = DBL_MAX;
  bi = INT64_MAX;
  for (int i = lane; i < ks.H; i += IA_WAVE) {
    const Winner w = ks.part[(int64_t)m * ks.H + i];
    if (w.d < bd || (w.d == bd && w.idx < bi)) { bd = w.d; bi = w.idx; }
  }
  wave_min_di(bd, bi);
  if (lane == 0) ks.cnt[m] = 0u;
  // (stats word as below: no candidates, one fallback)
  finish_pixel(LevelRows<CH>{db64}, g, A, px.r, px.c, bi, q, jp.s, jp.im, jp.Bp, jp.weights, jp.kf, jp.pstat, 1u << 16);
}

template <int CH, class JS>
__global__ void __launch_bounds__(IA_PQ_WG) k_kcoh_step(LevelGeo g, StepDesc sd, Imgs A, Imgs B, JS jobs,
                                                      const double *__restrict__ db64, const int32_t *__restrict__ sim,
                                                      int K, KcohScan ks) {
  __shared__ __attribute__((aligned(16))) double qsh[IA_PQ_WPB][Geo<CH>::DS];
  __shared__ int bsh[IA_PQ_WPB][16];  // the pixel's base rows, compacted
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = blockIdx.x * IA_PQ_WPB + wv;  // wave-uniform
  const int nq = sd.J * sd.M;
  double *q = qsh[wv];
  if (m >= nq) {
    // scan wave h: the step's pixels without a base row, 64 at a time
    const int h = m - nq;
    if (h >= ks.H) return;
    for (int m0 = 0; m0 < nq; m0 += IA_WAVE) {
      bool fb = false;
      if (m0 + lane < nq) {
        const QPix px = ia_qpix(sd, g.bw, m0 + lane);
        const JobPtrs jp = jobs.get(px.job);
        fb = !kcoh_has_base(g, jp.s, jp.im, px.r, px.c, px.qi);
      }
      unsigned long long todo = __ballot(fb);
      while (todo) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        kcoh_scan_pixel<CH>(g, sd, A, B, jobs, db64, ks, m0 + j, h, lane, q);
      }
    }
    return;
  }
  const QPix px = ia_qpix(sd, g.bw, m);
  const JobPtrs jp = jobs.get(px.job);
  const int r = px.r, c = px.c, qi = px.qi;
  const int b = lane < causal_cells(Pad2{}) ? kcoh_base_row(g, jp.s, jp.im, r, c, qi, lane) : -1;
  const unsigned long long bal = __ballot(b >= 0);
  const int nbase = __popcll(bal);  // <= 12: the causal cells
  if (nbase == 0) return;           // the scan waves find its exact NN and finish it
  kcoh_gather<CH>(g, B, jobs, px, jp, lane, q);
  if (b >= 0) bsh[wv][lane_prefix(bal)] = b;
  __builtin_amdgcn_wave_barrier();  // bsh written by this wave's lanes, read below

  // candidate j: base row j / (K + 1), itself (j % (K + 1) = 0) or its similar row j % (K + 1) - 1
  double bd = DBL_MAX;
  int64_t bi = INT64_MAX;
  const int ncand = nbase * (K + 1);
  for (int j = lane; j < ncand; j += IA_WAVE) {
    const int base = bsh[wv][j / (K + 1)], k = j % (K + 1);
    const int64_t row = k == 0 ? base : sim[(int64_t)base * K + (k - 1)];
    const double d = kcoh_dist<CH>(db64, row, q);
    if (d < bd || (d == bd && row < bi)) { bd = d; bi = row; }
  }
  wave_min_di(bd, bi);
  // stats word as K4's (JobPtrs::pstat): bits 0-15 the candidates computed, bit 16 a fallback
  finish_pixel(LevelRows<CH>{db64}, g, A, r, c, bi, q, jp.s, jp.im, jp.Bp, jp.weights, jp.kf, jp.pstat, (unsigned)ncand);
}

// pre-pass: every entry of sim (n of them) is a DB row
__global__ void __launch_bounds__(IA_WG) k_kcoh_check(const int32_t *__restrict__ sim, int64_t n, int NA,
                                                     unsigned *__restrict__ err) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * IA_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IA_WG)
    bad |= (unsigned)sim[i] >= (unsigned)NA;
  if (bad) *err = 1u;  // every writer stores the same word
}

void ia_launch_kcoh_check(const int32_t *sim, int64_t n, int NA, unsigned *err, hipStream_t st) {
  const unsigned nwg = (unsigned)std::min<int64_t>(1024, (n + IA_WG - 1) / IA_WG);
  hipLaunchKernelGGL(k_kcoh_check, dim3(nwg), dim3(IA_WG), 0, st, sim, n, NA, err);
}

int ia_kcoh_scan_waves(int64_t NA) { return (int)std::min<int64_t>(256, (NA + IA_WAVE - 1) / IA_WAVE); }

void ia_launch_kcoh_step(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const Imgs &B, const JobSet &jobs,
                         const double *db64, const int32_t *sim, int K, int H, void *part, unsigned *cnt, hipStream_t st) {
  const KcohScan ks{H, static_cast<Winner *>(part), cnt};
  const dim3 grid(cdiv((int64_t)sd.J * sd.M + H, IA_PQ_WPB));
  with_ch(g.ch, [&](auto c) {
    with_jobs(jobs, B, [&](auto js, const Imgs &Bj) {
      hipLaunchKernelGGL((k_kcoh_step<decltype(c)::CH, decltype(js)>), grid, dim3(IA_PQ_WG), 0, st, g, sd, A, Bj, js, db64, sim,
                         K, ks);
    });
  });
}

// ia_merge_shard.hip — the merges of a sharded level, where the per-rank certified winners
// (ia_kernels.hip k_merge_level<FUSED = false>, or k_merge_xchg here) meet: k_finish_level after
// an all-gather, k_merge_xchg through peer writes; and their launchers.
#include "ia_certify.h"
#include "ia_launch.h"

// multi-rank finish: global winner over the all-gathered per-rank winners, then coherence
template <int CH, class JS>
__global__ void __launch_bounds__(IA_WG) k_finish_level(LevelGeo g, StepDesc sd, Imgs A, const double *__restrict__ db64,
                                                         const double *__restrict__ q64,
                                                         const Winner *__restrict__ allwin, int world, int Mstride,
                                                         JS jobs) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (m >= sd.J * sd.M) return;
  double bd = DBL_MAX;
  int64_t bi = INT64_MAX;
  for (int k = 0; k < world; k++) {  // same order on every rank -> identical replicas
    const Winner w = allwin[(int64_t)k * Mstride + m];
    if (w.d < bd || (w.d == bd && w.idx < bi)) { bd = w.d; bi = w.idx; }
  }
  const QPix px = ia_qpix(sd, g.bw, m);
  const JobPtrs jp = jobs.get(px.job);
  const unsigned prev = jp.pstat ? jp.pstat[px.qi] : 0u;
  finish_pixel(LevelRows<CH>{db64}, g, A, px.r, px.c, bi, q64 + (int64_t)m * Geo<CH>::D, jp.s, jp.im, jp.Bp, jp.weights, jp.kf,
                   jp.pstat, prev, jp.nn);
}

// Sharded level, peer-write exchange (option "exchange" = 1): the certified winner of this
// rank's shard (as k_merge_level<FUSED = false>) is written into every rank's exchange buffer;
// with FIN the wave then polls its own buffer for the W winners of its query, takes the global
// winner (smallest exact distance, then lowest row: the lexicographic minimum, independent of
// arrival order) and finishes the pixel (coherence, kappa, writeback) exactly as
// k_finish_level.  One launch per step replaces merge + all-gather + finish.  Emulated shards on
// one device (shard_emulate) publish with FIN = false for shards 0..W-2 and FIN = true for the
// last.  A wait beyond xa.timeout_ticks sets *err and finishes with the winners that arrived
// (the host reports IA_ECOMM): no wave spins forever.
template <int CH, bool FIN, class JS, int RPL>
__global__ void __launch_bounds__(IA_PQ_WG) k_merge_xchg(LevelGeo g, StepDesc sd, Imgs A, MergeArgs ma, XchgArgs xa, JS jobs) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * IA_PQ_WPB + (threadIdx.x >> 6));  // wave-uniform
  if (m >= sd.J * sd.M) return;
  const int lane = threadIdx.x & 63;
  const QPix px = ia_qpix(sd, g.bw, m);
  const JobPtrs jp = jobs.get(px.job);
  const double *q = ma.q64 + (int64_t)m * Geo<CH>::D;
  unsigned stat = 0;
  const Winner wn = certified_winner<RPL>(ma, m, [&](int64_t row) { return exact_dist_level<CH>(ma.db64, row, q); }, &stat);
  if (lane < xa.W) {  // lane p publishes to rank p
    XSlot *sl = xa.peer[lane] + ia_xslot(xa.seq, xa.W, xa.rank, m);
    const unsigned row = wn.idx == INT64_MAX ? 0xffffffffu : (unsigned)wn.idx;
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(&sl->d), (unsigned long long)__double_as_longlong(wn.d),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    ia_stores_done();  // the distance has reached the (uncached) slot before its (row, seq) word
    __hip_atomic_store(&sl->row_seq, (unsigned long long)row | ((unsigned long long)xa.seq << 32), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if constexpr (!FIN) {
    if (lane == 0 && jp.pstat) jp.pstat[px.qi] = stat;
    return;
  } else {
    // the coherence pick does not depend on the NN winner: it runs while the peers' winners travel
    const CohPick ck = coherence_pick(LevelRows<CH>{ma.db64}, g, px.r, px.c, q, jp.s, jp.im);
    double bd = DBL_MAX;
    int64_t bi = INT64_MAX;
    bool late = false;
    if (lane < xa.W) {  // lane p reads rank p's winner
      XSlot *sl = xa.local + ia_xslot(xa.seq, xa.W, lane, m);
      const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
      // after an earlier timeout of this context: no waiting (one lost peer costs one timeout)
      const long long lim = __hip_atomic_load(xa.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? -1 : xa.timeout_ticks;
      unsigned long long rs = __hip_atomic_load(&sl->row_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      while ((unsigned)(rs >> 32) != xa.seq) {
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > lim) {
          late = true;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
        rs = __hip_atomic_load(&sl->row_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      if (!late) {
        const unsigned long long db =
            __hip_atomic_load(reinterpret_cast<unsigned long long *>(&sl->d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned row = (unsigned)rs;
        if (row < (unsigned)ma.NA) {  // 0xffffffff: the shard holds no row within the bound
          bd = __longlong_as_double((long long)db);
          bi = (int64_t)row;
        }
      }
    }
    if (__ballot(late) != 0ull && lane == 0) atomicOr(xa.err, 1u);
    wave_min_di(bd, bi);  // lexicographic (d, row) minimum: the same on every rank
    if (bi == INT64_MAX) {  // no shard reported a row (only after a timeout): keep every index in range
      bi = 0;
      if (lane == 0) atomicOr(xa.err, 2u);
    }
    finish_pick(LevelRows<CH>{ma.db64}, g, A, px.r, px.c, bi, ck, q, jp.s, jp.im, jp.Bp, jp.weights, jp.kf, jp.pstat, stat, jp.nn);
  }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_level_run.cpp)
// ------------------------------------------------------------------------------------------
void ia_launch_finish(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const double *db64, const double *q64,
                      const Winner *allwin, int world, int Mstride, const JobSet &jobs, hipStream_t st) {
  const dim3 grid(cdiv(sd.J * sd.M, IA_WG / IA_WAVE));
  with_ch(g.ch, [&](auto c) {
    with_jobs(jobs, [&](auto js) {
      hipLaunchKernelGGL((k_finish_level<decltype(c)::CH, decltype(js)>), grid, dim3(IA_WG), 0, st, g, sd, A, db64, q64, allwin,
                         world, Mstride, js);
    });
  });
}

void ia_launch_merge_xchg(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &ma, const XchgArgs &xa,
                          const JobSet &jobs, bool fin, hipStream_t st) {
  const dim3 grid(cdiv(sd.J * sd.M, IA_PQ_WPB));
  // 4 records per lane when the shard's scan ran <= 256 workgroups (every split-f16 scan)
  const bool r4 = ma.nwg <= 4 * IA_WAVE;
  with_ch(g.ch, [&](auto c) {
    with_jobs(jobs, [&](auto js) {  // (several jobs per sharded level: every rank holds every job's replica)
      constexpr int CH = decltype(c)::CH;
      using JS = decltype(js);
      if (fin && r4) hipLaunchKernelGGL((k_merge_xchg<CH, true, JS, 4>), grid, dim3(IA_PQ_WG), 0, st, g, sd, A, ma, xa, js);
      else if (fin) hipLaunchKernelGGL((k_merge_xchg<CH, true, JS, 8>), grid, dim3(IA_PQ_WG), 0, st, g, sd, A, ma, xa, js);
      else if (r4) hipLaunchKernelGGL((k_merge_xchg<CH, false, JS, 4>), grid, dim3(IA_PQ_WG), 0, st, g, sd, A, ma, xa, js);
      else hipLaunchKernelGGL((k_merge_xchg<CH, false, JS, 8>), grid, dim3(IA_PQ_WG), 0, st, g, sd, A, ma, xa, js);
    });
  });
}

// ia_kernels.hip — K4, the per-step merges of a one-rank level (and of a sharded level's ranks
// before their winners meet, ia_merge_shard.hip): k_merge_level and the fused merge + next
// step's gather k_merge_gather, with their launchers.  Shared device code: ia_dev.h (geometry,
// exact distances, bounds), ia_certify.h (certified winner), ia_gather.h (the gathers' bodies).
#include "ia_certify.h"
#include "ia_gather.h"
#include "ia_launch.h"

#if IA_PROBE & 8  // diagnostic build only: s_memtime phase stamps of sampled merge waves
#define IA_STAMP(k) do { __builtin_amdgcn_sched_barrier(0); stamp[k] = __builtin_amdgcn_s_memtime(); \
                         __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define IA_STAMP(k) do { } while (0)
#endif

struct MergeOut {  // one pixel's result: B' value (first channel), source pixel and A' image
  double v;
  int pr, pc, img;
  int nn;  // its certified exact NN row (-1: none)
  // the lanes whose round-2 row (my_row) is the final source pixel's / the NN winner's (-1: none
  // holds it: the winner came from an overflow candidate or a certification rescan)
  int src_lane, app_lane;
};
// the fused merge + gather launch (k_merge_gather): pixel (r, c)'s result as its wave's next
// query's own pixel
__device__ __forceinline__ void qhand_own(QHand &h, int r, int c, const MergeOut &o) {
  h.r0 = r;
  h.c0 = c;
  h.v0 = o.v;
  h.s0r = o.pr;
  h.s0c = o.pc;
  h.i0 = o.img;
  h.n0 = o.nn;
}
// ... and into its row's handoff slot for the row below (ia_gather.h handoff_wait): the fields,
// store completion, then the step's seq
__device__ __forceinline__ void handoff_publish(HandSlot *hs, const MergeOut &o, const NextStep &nx, int lane) {
  if (lane == 0) {
    hs->v = o.v;
    hs->sr = o.pr;
    hs->sc = o.pc;
    hs->im = o.img;
    hs->nn = o.nn;
  }
  ia_stores_done();
  if (lane == 0) __hip_atomic_store(&hs->seq, nx.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Fused single-rank merge of query m: certified exact NN + coherence + kappa + writeback.
// Memory is touched in two dependent rounds: (1) the K3 records, the coherence neighbours'
// s/im and the query/weights (staged in LDS), (2) ONE fp64-DB row per lane, in which lane
// k < 15 evaluates coherence candidate k and lanes 15..63 the MFMA candidates worth an exact
// rerank (placed by mbcnt rounds); every lane gets the exact unweighted distance (ranking),
// the weighted one (kappa rule) and its row's A' value (the B' write) from the same round.
// Candidates beyond the 49 rerank lanes (rare) are evaluated by the lanes that listed them.
// Wave reductions use DPP / permlane exchanges (no LDS round trips).
struct NoPre {
  __device__ __forceinline__ void operator()(int) const {}
};
template <int CH, int RPL, class Pre = NoPre>
__device__ __forceinline__ void merge_fused(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &a,
                                            int m, const JobPtrs &jp, const QPix &px,
                                            double *qs, double *ws, int *cand_row, float *cand_v,
                                            MergeOut *out = nullptr, Pre pre = Pre{}) {
#if IA_PROBE & 8
  unsigned long long stamp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  IA_STAMP(0);
  // RPL: records per lane (nwg <= 64 RPL); 4 for the split-f16 scans (<= 256 workgroups)
  constexpr int NCOH = causal_cells(Pad2{}), NRR = IA_WAVE - NCOH;  // lanes for coherence / rerank candidates
  const int lane = threadIdx.x & 63;
  const int r = px.r, c = px.c, qi = px.qi;
  int32_t *__restrict__ s = jp.s, *__restrict__ im = jp.im;
  double *__restrict__ Bp = jp.Bp;
  const double *__restrict__ weights = jp.weights;
  const double kf = jp.kf;
  const double *q = a.q64 + (int64_t)m * Geo<CH>::D;
  const float4 *rr = a.rec + (int64_t)m * a.nwg;
  const float *rT = a.recT + (int64_t)m * a.nwg;
  const unsigned hw = (unsigned)g.ah * (unsigned)g.aw;

  // ---- round 1: records (clamped, unconditional loads), coherence neighbours, query/weights
  float v1[RPL], v2[RPL], tt[RPL];
  int i1[RPL], i2[RPL];
  int xslot = 0;  // owner-computes sharded step: the query's slot in the step layout
  if (a.xo_W) {
    const int o = m / a.xo_M;
    xslot = a.xo_inv[(a.xo_o0 + o) * a.xo_QTs * IA_TILE + (m - o * a.xo_M)];
  }
#pragma unroll
  for (int j = 0; j < RPL; j++) {
    const int w = min(lane + IA_WAVE * j, a.nwg - 1);
    float4 x;
    float t;
    if (a.xo_W) {  // records pushed by every shard's scan: wait for this step's (T, seq)
      const int64_t ix = (int64_t)w * a.xo_Mrec + xslot;
      const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
      // after an earlier timeout of this context: no waiting (one lost peer costs one timeout)
      const long long lim = __hip_atomic_load(a.xo_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? -1 : a.xo_timeout;
      unsigned long long ts;
      // relaxed: the records are uncached (nothing stale to invalidate; an acquire would
      // invalidate this CU's caches on every poll); the float4 load issues after the seq was seen
      while (((ts = __hip_atomic_load(const_cast<unsigned long long *>(a.xo_rts) + ix, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_SYSTEM)) >> 32) != a.xo_seq) {
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > lim) {
          atomicOr(a.xo_err, 8u);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      x = a.rec[ix];
      t = __uint_as_float((unsigned)ts);
    } else {
      x = rr[w];
      t = rT[w];
    }
    const bool ok = lane + IA_WAVE * j < a.nwg;
    v1[j] = ok ? x.x : FLT_MAX;
    v2[j] = ok ? x.z : FLT_MAX;
    tt[j] = ok ? t : FLT_MAX;
    i1[j] = __float_as_int(x.y);
    i2[j] = __float_as_int(x.w);
  }
  for (int f = lane; f < Geo<CH>::D; f += IA_WAVE) {
    qs[f] = q[f];
    ws[f] = weights[f];
  }
  int crow = -1, cpr = -1, cpc = -1, cim = 0;
  if (qi > 0 && lane < NCOH) {  // best_coherence_match candidates, product(rows, cols) order
    const auto n = causal_cell(Pad2{}, g.bw, r, c, qi, lane);
    if (n.ok) {
      const ShiftedSrc t = shifted_src(g.ah, g.aw, s[2 * n.nb], s[2 * n.nb + 1], r, c, n.nr, n.nc);
      const int ti = im[n.nb];  // (issued with s, before the bounds test)
      if (t.ok) {
        cpr = t.tr;
        cpc = t.tc;
        cim = ti;
        crow = src_row(g.ah, g.aw, ti, t.tr, t.tc);
      }
    }
  }
  const double R = (double)__uint_as_float(*a.Rbits);
  const double qn2 = a.qn2[m];
#if IA_PROBE & 8
  if (v1[0] == 12345.f && crow == 7) stamp[7] = 1;  // force round 1 to land here
#endif
  IA_STAMP(1);

  // ---- MFMA candidates that may be the exact winner -> lanes 15..63 (mbcnt placement rounds)
  float a1 = FLT_MAX;
#pragma unroll
  for (int j = 0; j < RPL; j++) a1 = fminf(a1, v1[j]);
  a1 = wave_min_f_x(a1);
  const double qn = sqrt(qn2);
  const double eps = merge_eps(a, R, qn);
  const double thr = (double)a1 + 2.0 * eps;
  unsigned cmask = 0;
  // a float v satisfies v <= thr exactly when v <= thr rounded down to float: one conversion
  // instead of one per compared value
  const float thf = round_down_f(thr);
#pragma unroll
  for (int j = 0; j < RPL; j++) {
    if (v1[j] <= thf && i1[j] >= 0 && i1[j] < a.NA) cmask |= 1u << (2 * j);
    if (v2[j] <= thf && i2[j] >= 0 && i2[j] < a.NA) cmask |= 1u << (2 * j + 1);
  }
  int placed = 0;  // candidates given a rerank lane so far (wave-uniform)
  unsigned long long bal = __ballot(cmask != 0);
  while (bal && placed < NRR) {
    const int pos = placed + lane_prefix(bal);
    if (cmask != 0 && pos < NRR) {
      float v;
      cand_row[pos] = lowest_cand<RPL>(cmask, i1, i2, v1, v2, v);
      cand_v[pos] = v;
      cmask &= cmask - 1;
    }
    placed += __popcll(bal);
    bal = __ballot(cmask != 0);
  }
  const int n_cand = min(placed, NRR);
  __builtin_amdgcn_wave_barrier();
  int my_row = lane < NCOH ? crow : (lane - NCOH < n_cand ? cand_row[lane - NCOH] : -1);
  const float my_v = lane >= NCOH && my_row >= 0 ? cand_v[lane - NCOH] : FLT_MAX;
  IA_STAMP(2);
  // (k_merge_gather: the next query's step-independent inputs are loaded here, in flight together
  // with round 2's rows instead of after them; the two-wave form posts the lanes' rows here)
  pre(my_row);

  // ---- round 2: one fp64-DB row + its A' value per lane
  double unw = DBL_MAX, wsq = 0.;
  double av[CH];
#pragma unroll
  for (int k = 0; k < CH; k++) av[k] = 0.;
  if (my_row >= 0) {
    const unsigned img = (unsigned)my_row / hw;
    const double *src = A.p3 + img * A.img_stride_f + (int64_t)((unsigned)my_row - img * hw) * CH;
#pragma unroll
    for (int k = 0; k < CH; k++) av[k] = src[k];
    row_dists<CH>(a.db64, my_row, qs, ws, unw, wsq);
  }
  // bound audit: the exact distance of every reranked candidate must lie within eps of its
  // MFMA value + |q'|^2 (a violation would void the certification; counted, never expected).
  // unw and qn2 are fp64 sums in different orders: their own roundings, <= (D + 3) 2^-53 of each
  // and the counterpart of cert_theta's 1e-13 term, matter once eps is 0 (a constant A side under
  // the fp32 matcher: R = 0, every MFMA value 0, unw and qn2 equal up to their last bits)
  const bool viol = lane >= NCOH && my_row >= 0 && fabs(unw - qn2 - (double)my_v) > eps + 1e-13 * (unw + qn2);
  const bool any_viol = __ballot(viol) != 0;
#if IA_PROBE & 8
  if (unw == 12345.) stamp[7] = 2;
#endif
  IA_STAMP(3);

  // exact NN candidates of this lane: its rerank row, then any overflow it listed (rare)
  double nd = (lane >= NCOH && my_row >= 0) ? unw : DBL_MAX;
  int ni = (lane >= NCOH && my_row >= 0) ? my_row : INT_MAX;
  bool recompute_app = false;
  int n_over = 0;
  while (cmask) {
    float v;
    const int row = lowest_cand<RPL>(cmask, i1, i2, v1, v2, v);
    cmask &= cmask - 1;
    double u, wq;
    row_dists<CH>(a.db64, row, qs, ws, u, wq);
    if (u < nd || (u == nd && row < ni)) {
      nd = u;
      ni = row;
    }
    n_over++;
  }
  if (__ballot(n_over > 0)) recompute_app = true;
  // NN winner (lowest index on ties) and coherence winner (first argmin of the norm): the two
  // minima by interleaved DPP butterflies, then the lanes that hold them by ballot (a tie in the
  // NN distance between lanes - exact duplicate rows - takes the lowest row by a third butterfly)
  const double dkl = (lane < NCOH && my_row >= 0) ? cr_sqrt(unw) : DBL_MAX;
  const double bd0 = wave_min_d_x(nd), dk = wave_min_d_x(dkl);
  double bd = bd0;
  int bi = INT_MAX;
  if (bd0 < DBL_MAX) {
    const unsigned long long eqn = __ballot(nd == bd0);
    bi = __builtin_amdgcn_readlane(ni, __ffsll((long long)eqn) - 1);
    if (eqn & (eqn - 1)) {  // (wave-uniform, rare) several lanes at the same distance
      int x = nd == bd0 ? ni : INT_MAX;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
      bi = x;
    }
  }
  const int kk = dk < DBL_MAX ? __ffsll((long long)__ballot(dkl == dk)) - 1 : INT_MAX;
  const unsigned long long own = __ballot(lane >= NCOH && my_row >= 0 && my_row == bi && unw == bd);
  double wsq_app = 0.;
  int app_lane = 0;
  if (own) {
    app_lane = __ffsll((long long)own) - 1;
    wsq_app = readlane_d(wsq, app_lane);
  } else {
    recompute_app = true;
  }
  IA_STAMP(4);

  // certification (see certified_winner): rescan chunks whose threshold does not clear bd
  const double theta = cert_theta(a, R, qn, qn2, bd);
  const float thetaf = round_down_f(theta);  // (t <= theta  <=>  t <= theta rounded down, t a float)
  unsigned long long nfb = 0;
#pragma unroll
  for (int jb = 0; jb < RPL; jb++) {
    unsigned long long mask = __ballot(tt[jb] <= thetaf);
    while (mask) {
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int wgid = jb * IA_WAVE + j;
      double cd = DBL_MAX;
      int ci = INT_MAX;
      if (a.rr) {
        // pruned scan: chunk = tiles wgid, wgid + nwg, ...  Only rows with exact distance <= bd
        // can displace the winner, and such a row's tile has a projection lower bound
        // <= bd * ufac (ia_prune.h), so the rescan visits just the tiles that pass that box
        // test (one tile per lane), two tiles per wave pass
        const float4 ql = a.qinfo[3 * m], qh = a.qinfo[3 * m + 1];
        const float ub = round_up_f(bd * a.ufac);
        // the chunk's tiles t0 + tst k < tend (owner-computes step: chunk wgid mod nch of shard
        // wgid / nch, in that shard's storage range of the whole level's table)
        int64_t t0 = wgid, tst = a.nwg, tend = a.NT;
        if (a.xo_W) {
          const int sh = wgid / a.xo_nch;
          t0 = ia_shard_off(a.NT, a.xo_W, sh) + (wgid - sh * a.xo_nch);
          tst = a.xo_nch;
          tend = ia_shard_off(a.NT, a.xo_W, sh + 1);
        }
        for (int64_t tb = 0; t0 + tst * tb < tend; tb += IA_WAVE) {
          const int64_t t = t0 + tst * (tb + lane);
          bool nd = false;
          if (t < tend) nd = prune_lb(a.boxes[2 * t], a.boxes[2 * t + 1], ql, qh) <= ub;
          unsigned long long nm = __ballot(nd);
          while (nm) {
            const int j0 = __ffsll((long long)nm) - 1;
            nm &= nm - 1;
            int j1 = -1;
            if (nm) {
              j1 = __ffsll((long long)nm) - 1;
              nm &= nm - 1;
            }
            const int j = lane < 32 ? j0 : j1;
            if (j >= 0) {
              const int64_t i = a.pos2row[(t0 + tst * (tb + j)) * IA_TILE + (lane & 31)];
              if (i < a.NA) {
                const double d = exact_dist_level<CH>(a.db64, i, qs);
                if (d < cd || (d == cd && (int)i < ci)) { cd = d; ci = (int)i; }
              }
            }
          }
        }
      } else {
        const int64_t p0 = (int64_t)a.pos0 + (int64_t)wgid * a.tpw * IA_TILE;
        const int64_t p1 = min((int64_t)a.pos_end, p0 + (int64_t)a.tpw * IA_TILE);
        for (int64_t p = p0 + lane; p < p1; p += IA_WAVE) {
          const int64_t i = ia_pos_row_t(p, a.NT, a.pos2row);
          if (i >= a.NA) continue;
          const double d = exact_dist_level<CH>(a.db64, i, qs);
          if (d < cd || (d == cd && (int)i < ci)) { cd = d; ci = (int)i; }
        }
      }
      double du = DBL_MAX;
      int iu = INT_MAX;
      wave_min2_di(cd, ci, du, iu);
      (void)du;
      (void)iu;
      if (cd < bd || (cd == bd && ci < bi)) {
        bd = cd;
        bi = ci;
        recompute_app = true;
      }
      nfb++;
    }
  }
  IA_STAMP(5);

  int img = (int)((unsigned)bi / hw);
  const unsigned rem = (unsigned)bi - (unsigned)img * hw;
  int pr = (int)(rem / (unsigned)g.aw), pc = (int)(rem - (unsigned)pr * (unsigned)g.aw);
  const int app_img = img, app_pr = pr, app_pc = pc;
  double dbg_app = 0., dbg_coh = 0.;
  bool kamb = false;
  bool coh_won = false;
  int src_lane = recompute_app ? -1 : app_lane;  // lane holding the chosen row's A' value
  if (kk != INT_MAX) {  // a coherence candidate exists (never for the level's first pixel)
    // (ds_bpermute here: v_readlane at kk measured 0.25 us slower per launch, profiles/r06/trims)
    const int kpr = __shfl(cpr, kk, 64), kpc = __shfl(cpc, kk, 64), kim = __shfl(cim, kk, 64);
    const double wsq_coh = __shfl(wsq, kk, 64);
    if (recompute_app) {
      double u, wq = 0.;
      if (lane == 0) row_dists<CH>(a.db64, bi, qs, ws, u, wq);
      wsq_app = readlane_d(wq, 0);
    }
    dbg_app = wsq_app;  // the host finishes compute_distance as np.sqrt(v) ** 2 (libm pow)
    dbg_coh = wsq_coh;
    if (kappa_rule(cr_sqrt(wsq_app), cr_sqrt(wsq_coh), kf, &kamb)) {
      img = kim;
      pr = kpr;
      pc = kpc;
      coh_won = true;
      src_lane = kk;
    }
  }
  IA_STAMP(6);
  double val[CH];
#pragma unroll
  for (int k = 0; k < CH; k++) val[k] = src_lane >= 0 ? readlane_d(av[k], src_lane) : 0.;
  if (src_lane < 0) {  // winner from an overflow candidate or a rescan: fetch its A' value
#pragma unroll
    for (int k = 0; k < CH; k++) val[k] = A.p3[img * A.img_stride_f + ((int64_t)pr * g.aw + pc) * CH + k];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < CH; k++) Bp[(int64_t)qi * CH + k] = val[k];
    s[2 * qi] = pr;
    s[2 * qi + 1] = pc;
    im[qi] = img;
    if (jp.nn) jp.nn[qi] = bi >= 0 && bi < a.NA ? bi : -1;  // option "nn_bound"
    // per-pixel stats word (no shared-counter atomics: hundreds of waves adding to one
    // address serialise at L2 and dominated this kernel); reduced once per level
    const int slot = placed + 0;
    jp.pstat[qi] = (unsigned)min(slot, 0xffff) | ((unsigned)min((int)nfb, 0x1fff) << 16) | (kamb ? 1u << 29 : 0u) |
                  (coh_won ? 1u << 30 : 0u) |
                  (any_viol ? 1u << 31 : 0u);
    if (jp.dbg_src) {  // debug=True structures (image_analogies.py:224-240): p_app, r_star, d_app, d_coh
      const bool has_coh = kk != INT_MAX;
      int32_t *o = jp.dbg_src + (int64_t)qi * 6;
      o[0] = app_pr;
      o[1] = app_pc;
      o[2] = app_img;
      const auto n = causal_cell(Pad2{}, g.bw, r, c, qi, has_coh ? kk : 0);  // r_star
      o[3] = has_coh ? n.nr : 0;
      o[4] = has_coh ? n.nc : 0;
      o[5] = has_coh ? 1 : 0;
      jp.dbg_dist[2 * qi] = dbg_app;
      jp.dbg_dist[2 * qi + 1] = dbg_coh;
    }
  }
  if (out) {  // the pixel's result (wave-uniform) for a fused next-step gather (k_merge_gather)
    out->v = val[0];
    out->pr = pr;
    out->pc = pc;
    out->img = img;
    out->nn = bi >= 0 && bi < a.NA ? bi : -1;
    out->src_lane = src_lane;
    out->app_lane = recompute_app ? -1 : app_lane;
  }
#if IA_PROBE & 8
  if (lane == 0 && m == sd.M / 2 && (sd.t % 256) == 128) {
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t7 = __builtin_amdgcn_s_memtime();
    printf("STAMP bw=%d t=%d M=%d slot=%d nfb=%d d1=%llu d2=%llu d3=%llu d4=%llu d5=%llu d6=%llu d7=%llu\n", g.bw, sd.t,
           sd.M, placed, (int)nfb, stamp[1] - stamp[0], stamp[2] - stamp[1], stamp[3] - stamp[2], stamp[4] - stamp[3],
           stamp[5] - stamp[4], stamp[6] - stamp[5], t7 - stamp[6]);
  }
#endif
}

// K4 of one step.  FUSED: the whole merge (merge_fused), the pixel finished; otherwise (a sharded
// level's rank, exchange = 0) only the certified winner of this rank's shard, for k_finish_level.
template <int CH, bool FUSED, class JS, int RPL = IA_WG_TARGET / IA_WAVE>
__global__ void __launch_bounds__(IA_PQ_WG) k_merge_level(LevelGeo g, StepDesc sd, Imgs A, MergeArgs ma, Winner *__restrict__ win,
                                                        JS jobs) {
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * IA_PQ_WPB + (threadIdx.x >> 6));  // wave-uniform
  if (m >= sd.J * sd.M) return;
  const QPix px = ia_qpix(sd, g.bw, m);
  const JobPtrs jp = jobs.get(px.job);
  if constexpr (FUSED) {
    __shared__ double qsh[IA_PQ_WPB][Geo<CH>::DS], wsh[IA_PQ_WPB][Geo<CH>::DS];
    __shared__ int crsh[IA_PQ_WPB][IA_WAVE];
    __shared__ float cvsh[IA_PQ_WPB][IA_WAVE];
    const int wv = threadIdx.x >> 6;
    const unsigned long long t0 = ma.stamp ? ia_clock() : 0ull;  // option "stamps"
    merge_fused<CH, RPL>(g, sd, A, ma, m, jp, px, qsh[wv], wsh[wv], crsh[wv], cvsh[wv]);
    if (ma.stamp && (threadIdx.x & 63) == 0) ia_stamp_wg(ma.stamp, t0);
  } else {
    const double *q = ma.q64 + (int64_t)m * Geo<CH>::D;
    unsigned stat = 0;
    const Winner wn = certified_winner<RPL>(ma, m, [&](int64_t row) { return exact_dist_level<CH>(ma.db64, row, q); }, &stat);
    if ((threadIdx.x & 63) == 0) {
      win[m] = wn;
      if (jp.pstat) jp.pstat[px.qi] = stat;  // finish adds the coherence bit
    }
  }
}

// ------------------------------------------------------------------------------------------
// K4 + K2 fused (option "fuse_gather"): K4 of step t, then the gather (K2p on pruned levels,
// K2h on the others) of step t + 1, one launch.  Pixel (r, c + 1) of step t + 1 reads two
// results of step t: its own row's (r, c) and the row above's (r - 1, c + 3) (skew 3: both lie
// on step t); everything else it reads is older.  So the wave of query (job j, row r) merges
// (r, c), hands its result to row r + 1 through an uncached slot (fields, store completion, then
// the step's seq), and gathers (r, c + 1), waiting for the slot of row r - 1: a wave of the same
// launch with a LOWER index (rows ascend with the query index within a job), dispatched before
// it, so the waits always drain.  Waves J M .. J M + J - 1 gather each job's row entering at
// step t + 1 (column 0; its row above is that job's last merge wave), the waves after them the
// step's pad queries (and, owner-computes ranks with xo_wait, one waiter).  The query buffers
// alternate by step parity (this launch's merges read step t's half while its gathers write
// step t + 1's).
//
// GW (option "gather_wave"; the one-job, one-rank pruned early path only): workgroups of two waves,
// one workgroup per wave of the form above.  In a merge workgroup (w < M) wave 0, the merge wave,
// only merges (r, c) and publishes the row's slot; wave 1, the gather wave, gathers (r, c + 1)
// from wave start and takes (r, c)'s result from wave 0 through LDS (merge_gather_pair).  The
// other workgroups (the entering row, the pads) run the one-wave code in wave 0; their wave 1
// exits at once.
// ------------------------------------------------------------------------------------------
// A merge workgroup of the two-wave form.  The roles meet at two workgroup barriers, which both
// reach exactly once each on every path, nothing returning in front of them: one at the start
// (prow_on cleared), one that hands MergeOut over through LDS: the merge wave reaches it after its
// merge (it waits for nothing before it), the gather wave after gather_wave_pre / _next, also
// when it has no query to gather (the row's last column).  The gather wave's two polls - prow_on,
// set by its own merge wave, which never waits, and the row above's slot after the second barrier
// - are bounded by nx.timeout_ticks like every handoff wait (err bit 16).
template <int RPL>
__device__ __forceinline__ void merge_gather_pair(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &ma,
                                                  const JobPtrs &jp, const Imgs &B, const NextStep &nx, int w, int role,
                                                  int lane, double *qsh, double *wsh, int *crsh, float *cvsh) {
  constexpr int KS = 4;
  __shared__ double gq[Geo<1>::DS];  // the gather wave's query row
  __shared__ MergeOut mo;
  const QPix px = ia_qpix(sd, g.bw, w);
  const int mn = px.c + 1 < g.bw ? px.r - nx.sn.r0 : -1;  // the query of step t + 1 (one job)
  const bool on = mn >= 0 && mn < nx.sn.M;
  // the merge wave's round-2 rows (my_row of merge_fused), posted as soon as they are placed:
  // the gather wave loads the raster successor of each (gather_wave_next); prow_on: posted
  __shared__ int prow[IA_WAVE];
  __shared__ int prow_on;
  if (role == 0 && lane == 0) __hip_atomic_store(&prow_on, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();  // (the first of the two barriers: prow_on cleared before anyone polls it)
  GatherWave gw;
  MergeOut o;
  if (role == 0) {
    auto post = [&](int my_row) {  // no wait: a flag, not a barrier
      prow[lane] = my_row;
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) __hip_atomic_store(&prow_on, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    merge_fused<1, RPL>(g, sd, A, ma, w, jp, px, qsh, wsh, crsh, cvsh, &o, post);
    if (lane == 0) mo = o;
  } else if (on) {
    gw = gather_wave_pre<KS>(g, nx, B, jp, mn, lane, ma.db64, gq);
    gather_wave_next(g, nx, prow, &prow_on, lane, ma.db64, gq, gw);
  }
  __syncthreads();
  if (role == 0) {
    // (after the barrier: the gather wave, long there, does not wait for these stores' completion)
    if (px.r + 1 < g.bh && px.c >= 2) handoff_publish(nx.hand + px.r, o, nx, lane);  // for (r + 1, c - 2) of step t + 1
    return;
  }
  if (!on) return;
  QHand h;
  h.r0 = px.r;
  h.c0 = px.c;
  h.v0 = mo.v;
  h.s0r = __builtin_amdgcn_readfirstlane(mo.pr);
  h.s0c = __builtin_amdgcn_readfirstlane(mo.pc);
  h.i0 = __builtin_amdgcn_readfirstlane(mo.img);
  h.n0 = __builtin_amdgcn_readfirstlane(mo.nn);
  gather_wave_post<KS>(g, nx, jp, 0, mn, lane, ma.db64, gq, h, __builtin_amdgcn_readfirstlane(mo.src_lane),
                       __builtin_amdgcn_readfirstlane(mo.app_lane), gw);
}

template <int RPL, bool PR, bool XO, class JS, bool GW = false>
__device__ __forceinline__ void merge_gather_body(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &ma,
                                                  const JS &jobs, Imgs B, const NextStep &nx) {
  constexpr int KS = 4;
  static_assert(!GW || (PR && !XO && JS::single && IA_PQ_WPB == 1), "two-wave form: the one-job pruned early path");
  const int w = __builtin_amdgcn_readfirstlane(GW ? blockIdx.x : blockIdx.x * IA_PQ_WPB + (threadIdx.x >> 6));
  const int lane = threadIdx.x & 63, wv = GW ? 0 : threadIdx.x >> 6;
  const int J = JS::single ? 1 : sd.J, JM = J * sd.M;
  __shared__ double qsh[IA_PQ_WPB][Geo<1>::DS], wsh[IA_PQ_WPB][Geo<1>::DS];
  __shared__ int crsh[IA_PQ_WPB][IA_WAVE];
  __shared__ float cvsh[IA_PQ_WPB][IA_WAVE];
  __shared__ __attribute__((aligned(16))) _Float16 xh[IA_PQ_WPB][2][16 * KS];  // owner publish: hi / lo columns
  if constexpr (GW) {
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w < JM) {  // (workgroup-uniform)
      merge_gather_pair<RPL>(g, sd, A, ma, jobs.get(0), B, nx, w, role, lane, qsh[0], wsh[0], crsh[0], cvsh[0]);
      return;
    }
    if (role) return;
  }
  if (XO && w >= JM + J + (nx.sn.Mpad - J * nx.sn.M)) {  // the waiter (nx.wait_n > 0 only)
    // after an earlier timeout of this context: no waiting (one lost peer costs one timeout)
    if (__hip_atomic_load(nx.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    for (int i = lane; i < nx.wait_n; i += IA_WAVE)
      while (__hip_atomic_load(nx.wait_seq + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != nx.xp.seq) {
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > nx.timeout_ticks) {
          atomicOr(nx.err, 4u);
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    return;
  }
  QHand h;
  int mn = -1;   // this wave's query of step t + 1
  int job = 0;
  QPre pf;       // its step-independent inputs, prefetched during the merge (pruned levels)
  // the early gather path (gather_p_early): merge waves of one-rank pruned levels, no publish
  const bool early = PR && !XO && !nx.kslot && nx.prefetch && nx.early;
  QConst qk;
  if (early) qk = qconst_load(nx, lane);
#if IA_PROBE & 8  // diagnostic build only: fused merge + gather phase stamps of one sampled wave
  unsigned long long gs[5] = {__builtin_amdgcn_s_memtime(), 0, 0, 0, 0}, gst[5] = {0, 0, 0, 0, 0};
  const bool gprobe = w == sd.M / 2 && (sd.t % 256) == 128 && JM == sd.M;
#endif
  if (!GW && w < JM) {  // (GW: merge_gather_pair above)
    const QPix px = ia_qpix(sd, g.bw, w);
    job = px.job;
    const JobPtrs jp = jobs.get(job);
    MergeOut o;
    if (px.c + 1 < g.bw) mn = job * nx.sn.M + (px.r - nx.sn.r0);
    const Imgs Bj = JS::single ? B : job_imgs(B, jp);
    auto pre = [&](int) {
      if (PR && nx.prefetch && mn >= 0) pf = qpre_load(g, nx.sn, Bj, jp, mn, lane);
    };
    merge_fused<1, RPL>(g, sd, A, ma, w, jp, px, qsh[wv], wsh[wv], crsh[wv], cvsh[wv], &o, pre);
    if (px.r + 1 < g.bh && px.c >= 2)  // row r + 1 gathers (r + 1, c - 2) at step t + 1
      handoff_publish(nx.hand + (int64_t)job * g.bh + px.r, o, nx, lane);
    qhand_own(h, px.r, px.c, o);
#if IA_PROBE & 8
    __builtin_amdgcn_s_waitcnt(0);
    gs[1] = __builtin_amdgcn_s_memtime();
#endif
  } else if (w < JM + J) {
    job = w - JM;
    if (nx.sn.t - 3 * (nx.sn.r0 + nx.sn.M - 1) == 0) mn = job * nx.sn.M + nx.sn.M - 1;  // a row enters at column 0
  } else {
    mn = J * nx.sn.M + (w - JM - J);
  }
  if (mn < 0 || mn >= nx.sn.Mpad) return;
  _Float16 *qf = (_Float16 *)nx.qf;
  float4 o0, o1, o2;
  if (mn >= J * nx.sn.M) {
    if constexpr (PR) {
      gather_p_pad<KS>(mn, lane, qf, nx.qinfo, o0, o1, o2);
      if ((XO && nx.xp.W) || (!XO && nx.kslot)) {
        if (lane < 16 * KS) xh[wv][0][lane] = xh[wv][1][lane] = (_Float16)0.f;
        if (XO) xo_publish<KS>(nx.xp, mn, lane, xh[wv][0], xh[wv][1], o0, o1, o2);
        else sorted_publish<KS>(nx, mn, lane, xh[wv][0], xh[wv][1], o0, o1, o2);
      }
    } else {
      if (lane < 16 * KS) put_qh<KS>(qf, mn, lane, 0.);
    }
    return;
  }
  const JobPtrs jp = jobs.get(job);
  if constexpr (!JS::single) B = job_imgs(B, jp);  // single job: B already holds its images
  if constexpr (PR) {
    if (early && pf.on) {
      __builtin_amdgcn_wave_barrier();  // the merge's LDS rows are done with
      gather_p_early<KS>(g, nx, B, jp, job, mn, lane, ma.db64, qsh[wv], h, pf, qk);
      return;
    }
  }
  const QPix pn = ia_qpix(nx.sn, g.bw, mn);
  if (pn.r >= 1 && pn.c + 2 < g.bw) {  // (r - 1, c + 2) of step t: the row above's handoff
    const HandSlot *hs = nx.hand + (int64_t)job * g.bh + (pn.r - 1);
    handoff_wait(hs, nx);
    h.r1 = pn.r - 1;
    h.c1 = pn.c + 2;
    h.v1 = hs->v;
    h.s1r = hs->sr;
    h.s1c = hs->sc;
    h.i1 = hs->im;
    h.n1 = hs->nn;
  }
#if IA_PROBE & 8
  __builtin_amdgcn_s_waitcnt(0);
  gs[2] = __builtin_amdgcn_s_memtime();
#endif
  __builtin_amdgcn_wave_barrier();  // the merge's LDS rows are done with
  if constexpr (PR) {
    const bool pub = (XO && nx.xp.W) || (!XO && nx.kslot);
    gather_p_query<KS, true>(g, nx.sn, B, jp, mn, lane, nx.mu, nx.q64, nx.qn2, qf, ma.db64, nx.basis, nx.ufac,
                             nx.qinfo, qsh[wv], pub ? xh[wv][0] : nullptr, xh[wv][1], h, o0, o1, o2, pf
#if IA_PROBE & 8
                             , gprobe ? gst : nullptr
#endif
                             );
    if (XO && nx.xp.W) xo_publish<KS>(nx.xp, mn, lane, xh[wv][0], xh[wv][1], o0, o1, o2);
    if (!XO && nx.kslot) sorted_publish<KS>(nx, mn, lane, xh[wv][0], xh[wv][1], o0, o1, o2);
  } else {
    gather_h_query_fused<KS>(g, nx.sn, B, mn, lane, nx.mu, nx.q64, nx.qn2, qf, h);
  }
#if IA_PROBE & 8
  __builtin_amdgcn_s_waitcnt(0);
  gs[3] = __builtin_amdgcn_s_memtime();
  if (gprobe && lane == 0)
    printf("GSTAMP bw=%d t=%d M=%d merge=%llu handoff_wait=%llu gather=%llu [feat+frag=%llu sums=%llu urow=%llu rec=%llu]\n",
           g.bw, sd.t, sd.M, gs[1] - gs[0], gs[2] - gs[1], gs[3] - gs[2], gst[1] - gst[0], gst[2] - gst[1], gst[3] - gst[2],
           gst[4] - gst[3]);
#endif
}
template <int RPL, bool PR, bool XO, class JS, bool GW = false>
__global__ void __launch_bounds__(GW ? 2 * IA_WAVE : IA_PQ_WG)
k_merge_gather(LevelGeo g, StepDesc sd, Imgs A, MergeArgs ma, JS jobs, Imgs B, NextStep nx) {
  const unsigned long long t0 = ma.stamp ? ia_clock() : 0ull;  // option "stamps"
  merge_gather_body<RPL, PR, XO, JS, GW>(g, sd, A, ma, jobs, B, nx);
  // (GW: both waves stamp their workgroup's slot; the one that ends last, thousands of ticks after
  // the other, leaves the end time)
  if (ma.stamp && (threadIdx.x & 63) == 0) ia_stamp_wg(ma.stamp, t0);
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_level_run.cpp, ia_level_owner.cpp)
// ------------------------------------------------------------------------------------------
void ia_launch_merge(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &ma, Winner *win,
                     const JobSet &jobs, bool fused, hipStream_t st) {
  const dim3 grid(cdiv(sd.J * sd.M, IA_PQ_WPB));
  // the fused merge with 4 records per lane when the scan ran <= 256 workgroups (every
  // split-f16 scan): half the record loads and candidate tests of the 8-per-lane form
  const bool r4 = fused && ma.nwg <= 4 * IA_WAVE;
  with_ch(g.ch, [&](auto c) {
    with_jobs(jobs, [&](auto js) {
      constexpr int CH = decltype(c)::CH;
      using JS = decltype(js);
      if (r4) hipLaunchKernelGGL((k_merge_level<CH, true, JS, 4>), grid, dim3(IA_PQ_WG), 0, st, g, sd, A, ma, win, js);
      else if (fused) hipLaunchKernelGGL((k_merge_level<CH, true, JS>), grid, dim3(IA_PQ_WG), 0, st, g, sd, A, ma, win, js);
      else hipLaunchKernelGGL((k_merge_level<CH, false, JS>), grid, dim3(IA_PQ_WG), 0, st, g, sd, A, ma, win, js);
    });
  });
}

// Every k_merge_gather instance the library launches, by what selects it: the one list both the
// launcher and the chained-wave budget (ia_merge_gather_occupancy) read.  Owner-computes steps
// (xo) exist only as one-job pruned steps, the two-wave form (gw, option "gather_wave") only as
// the one-job, one-rank pruned early path.
struct MergeGatherInst {
  bool single, pruned, xo, gw;
  const void *fn;
  int threads() const { return gw ? 2 * IA_WAVE : IA_PQ_WG; }
};
static const MergeGatherInst k_merge_gather_insts[] = {
    {true, true, true, false, (const void *)k_merge_gather<4, true, true, JobArg1>},
    {true, true, false, false, (const void *)k_merge_gather<4, true, false, JobArg1>},
    {true, true, false, true, (const void *)k_merge_gather<4, true, false, JobArg1, true>},
    {true, false, false, false, (const void *)k_merge_gather<4, false, false, JobArg1>},
    {false, true, false, false, (const void *)k_merge_gather<4, true, false, JobArgN>},
    {false, false, false, false, (const void *)k_merge_gather<4, false, false, JobArgN>},
};

void ia_launch_merge_gather(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &ma, const JobSet &jobs,
                            const Imgs &B, const NextStep &nx, bool pruned, hipStream_t st) {
  // waves: the step's merges, each job's entering row, the next step's pad queries (+ the waiter)
  const int nw = sd.J * sd.M + sd.J + (nx.sn.Mpad - sd.J * nx.sn.M) + (nx.wait_n > 0 ? 1 : 0);
  const bool single = jobs.J == 1;
  const bool xo = single && pruned && (nx.xp.W > 0 || nx.wait_n > 0);
  // two waves per workgroup: where the level reserved them (nx.gwave) and the early path runs
  const bool gw = nx.gwave && single && pruned && !xo && !nx.kslot && nx.prefetch && nx.early;
  for (const MergeGatherInst &k : k_merge_gather_insts) {
    if (k.single != single || k.pruned != pruned || k.xo != xo || k.gw != gw) continue;
    const dim3 grid(gw ? nw : cdiv(nw, IA_PQ_WPB));
    // the kernel's arguments in order; the JS argument by the instance's kind (with_jobs' pairs)
    JobArg1 j1{jobs.j0};
    JobArgN jn{jobs.rest};
    Imgs Bj = single ? job0_imgs(B, jobs) : B;
    void *args[] = {(void *)&g,  (void *)&sd, (void *)&A, (void *)&ma, single ? (void *)&j1 : (void *)&jn,
                    (void *)&Bj, (void *)&nx};
    (void)hipLaunchKernel(k.fn, grid, dim3(k.threads()), args, 0, st);
    return;
  }
}
// the chained-wave budget's inputs (ia_ctx.cpp, ia_chain_budget): the most VGPRs per lane over
// every k_merge_gather instance the library launches, and the workgroups per CU the occupancy
// API admits and the workgroup size of the instance with the fewest resident waves per CU, from
// the compiled kernels themselves
void ia_merge_gather_occupancy(int *vgprs, int *blocks_per_cu, int *wg_threads) {
  int vmax = 0, wmin = 1 << 30;
  *blocks_per_cu = 0;
  *wg_threads = IA_PQ_WG;
  for (const MergeGatherInst &k : k_merge_gather_insts) {
    hipFuncAttributes fa;
    int nb = 0;
    if (hipFuncGetAttributes(&fa, k.fn) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, k.threads(), 0) != hipSuccess)
      nb = 0;
    else
      vmax = std::max(vmax, (int)fa.numRegs);
    const int waves = nb * (k.threads() / IA_WAVE);
    if (waves < wmin) {
      wmin = waves;
      *blocks_per_cu = nb;
      *wg_threads = k.threads();
    }
  }
  *vgprs = vmax;
}

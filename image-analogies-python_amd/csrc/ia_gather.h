// ia_gather.h — the split-f16 gathers' device bodies, one wave per query: what K2h / K2p
// (ia_gather.hip) and the fused merge + gather launch (ia_kernels.hip k_merge_gather) both run.
#pragma once
#include "ia_dev.h"

// query m's feature f (value v) into the split-f16 fragments (hi and lo pieces, ia_dev.h split_h)
template <int KS>
__device__ __forceinline__ void put_qh(_Float16 *qf, int m, int f, double v) {
  const int qt = m / IA_TILE, j = m % IA_TILE, s = f >> 4, h = (f >> 3) & 1, e = f & 7;
  _Float16 hi, lo;
  split_h(v, hi, lo);
  const int64_t base = (((int64_t)qt * 2 * KS + 2 * s) * IA_WAVE + h * IA_TILE + j) * 8 + e;
  qf[base] = hi;
  qf[base + IA_WAVE * 8] = lo;
}

// The two pixels of step t whose results a fused K4(t) + K2p(t + 1) wave (k_merge_gather) hands
// to its next query: its own (r0, c0) and the row above's (r1, c1), both written in the same
// launch, so their B', s and im come from registers / the handoff slot, never from memory.
struct QHand {
  int r0 = -1, c0 = -1, r1 = -1, c1 = -1;
  double v0 = 0., v1 = 0.;
  int s0r = 0, s0c = 0, i0 = 0, s1r = 0, s1c = 0, i1 = 0;
  int n0 = -1, n1 = -1;  // their exact NN rows (option "nn_bound")
};
// B' slot k < 12 (feature 43 + k) of the causal 5x5 window at (r, c): its pixel (y, x), reflected
// at the image's borders (so one pixel can fill several slots)
__device__ __forceinline__ void bslot(const Imgs &B, int k, int r, int c, int &y, int &x) {
  y = ia_reflect(r + k / 5 - 2, B.h);
  x = ia_reflect(c + k % 5 - 2, B.w);
}
// This lane's causal neighbour of the query pixel (r, c), raster index qi: lanes 0..14 carry
// neighbour k of the causal 5x5 (product(rows, cols) order as merge_fused) for its source pixel;
// lanes 15..29, where nnl (the level keeps exact NN rows, option "nn_bound"), the same neighbour
// k = lane - 15 for its NN row.  ok: the lane carries one, inside B and before qi in raster order.
struct CausalNb {
  int k, nr, nc, nb;  // neighbour, its pixel and raster index
  bool ok;
};
__device__ __forceinline__ CausalNb causal_nb(const LevelGeo &g, int r, int c, int qi, int lane, bool nnl) {
  constexpr int NC = causal_cells(Pad2{});
  CausalNb n{0, 0, 0, 0, false};
  if (qi > 0 && (lane < NC || nnl)) {
    n.k = lane < NC ? lane : lane - NC;
    const auto cl = causal_cell(Pad2{}, g.bw, r, c, qi, n.k);
    n.nr = cl.nr;
    n.nc = cl.nc;
    if (cl.ok) {
      n.nb = cl.nb;
      n.ok = true;
    }
  }
  return n;
}
template <bool FUSE>
__device__ __forceinline__ double feat_q1(const Imgs &B, int f, int r, int c, const QHand &h) {
  if constexpr (FUSE) {
    if (f >= 43) {  // the B' part (causal 5x5 at (r, c), k < 12)
      int y, x;
      bslot(B, f - 43, r, c, y, x);
      if (y == h.r0 && x == h.c0) return h.v0;
      if (y == h.r1 && x == h.c1) return h.v1;
      return B.p3[(int64_t)y * B.w + x];
    }
  }
  return win_feat(Geo<1>{}, B, f, r, c, 0);
}

// owner-computes sharded step (XOPub): query m's fragments (16 h16x8 pieces from LDS, one store
// instruction per area), its pruning record, then - once those stores completed - its seq, into
// every rank's area
// lane k < 3 picks record k, component by component (a float4 chosen by a lane-dependent
// ternary becomes a dynamically indexed private array: scratch, and a scratch-using kernel)
__device__ __forceinline__ float4 sel3(int k, const float4 &a, const float4 &b, const float4 &c) {
  return make_float4(k == 0 ? a.x : k == 1 ? b.x : c.x, k == 0 ? a.y : k == 1 ? b.y : c.y,
                     k == 0 ? a.z : k == 1 ? b.z : c.z, k == 0 ? a.w : k == 1 ? b.w : c.w);
}
template <int KS>
__device__ __forceinline__ void xo_publish(const XOPub &xp, int m, int lane, const _Float16 *xh0, const _Float16 *xh1,
                                           float4 i0, float4 i1, float4 i2) {
  __builtin_amdgcn_wave_barrier();  // xh written by this wave's lanes
  const int qt = m / IA_TILE, j = m % IA_TILE;
  const int c = lane, sp = c >> 2, part = (c >> 1) & 1, h = c & 1;  // chunk c < 2 KS * 2
  h16x8 v{};
  if (c < 4 * KS) v = *reinterpret_cast<const h16x8 *>(&(part ? xh1 : xh0)[16 * sp + 8 * h]);
  const int64_t t0 = xp.slot0 / IA_TILE;
  for (int o = 0; o < xp.W; o++) {
    if (c < 4 * KS)
      reinterpret_cast<h16x8 *>(xp.area[o] + XOLayout::FRAG)[((t0 + qt) * 2 * KS + 2 * sp + part) * IA_WAVE + h * IA_TILE + j] = v;
    if (lane < 3) reinterpret_cast<float4 *>(xp.area[o] + XOLayout::INFO)[3 * (xp.slot0 + m) + lane] = sel3(lane, i0, i1, i2);
  }
  ia_stores_done();
  if (lane < xp.W)
    __hip_atomic_store(reinterpret_cast<unsigned *>(xp.area[lane] + XOLayout::QSEQ) + xp.slot0 + m, xp.seq, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

// option "fuse_sort" (NextStep::kslot): query m of step nx.sn publishes its sort key (the Morton
// key's top 20 bits above the 12-bit query index, k_query_sort's order), waits for every key of
// the step, takes its rank x among them and writes its pruning record, query index and split-f16
// fragments (hi / lo columns from xh0 / xh1) at sorted slot x.  Every query of the step is
// gathered by exactly one wave of this launch, all of them resident together (one wave per
// workgroup), so the wait drains; a key that never arrives (bounded, 20 s) sets err bit 4.
template <int KS>
__device__ __forceinline__ void sorted_publish(const NextStep &nx, int m, int lane, const _Float16 *xh0, const _Float16 *xh1,
                                               float4 i0, float4 i1, float4 i2) {
  const unsigned key = (__float_as_uint(i2.y) & 0xFFFFF000u) | (unsigned)m;
  if (lane == 0)
    __hip_atomic_store(nx.kslot + m, ((unsigned long long)nx.seq << 32) | key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __builtin_amdgcn_wave_barrier();  // xh written by this wave's lanes
  // the fragments to registers while the other keys arrive
  const int c = lane, sp = c >> 2, part = (c >> 1) & 1, h = c & 1;  // chunk c < 4 KS
  h16x8 v{};
  if (c < 4 * KS) v = *reinterpret_cast<const h16x8 *>(&(part ? xh1 : xh0)[16 * sp + 8 * h]);
  int below = 0;
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  const bool late = __hip_atomic_load(nx.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
  for (int i = lane; i < nx.sn.Mpad; i += IA_WAVE) {
    unsigned long long x;
    // relaxed: the slots are uncached (no stale line to invalidate)
    while (((x = __hip_atomic_load(nx.kslot + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) >> 32) != nx.seq && !late) {
      if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > nx.timeout_ticks) {
        atomicOr(nx.err, 16u);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    below += (unsigned)x < key ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o, 64);
  const int x = __builtin_amdgcn_readfirstlane(below);
  const int qt = x / IA_TILE, j = x % IA_TILE;
  if (c < 4 * KS) reinterpret_cast<h16x8 *>(nx.sfrag)[((int64_t)qt * 2 * KS + 2 * sp + part) * IA_WAVE + h * IA_TILE + j] = v;
  if (lane < 3) nx.sinfo[3 * x + lane] = sel3(lane, i0, i1, i2);
  if (lane == 3) nx.sorder[x] = m;
}

// The bounded wait for a row's handoff slot (k_merge_gather: written by the wave of this launch
// that merged the row's step-t pixel): until its seq is the step's.  relaxed: the slot is uncached
// (nothing stale to invalidate); its fields load after the seq was seen.  A slot that does not
// arrive within nx.timeout_ticks sets err bit 16.
__device__ __forceinline__ void handoff_wait(const HandSlot *hs, const NextStep &nx) {
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  while (__hip_atomic_load(&hs->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != nx.seq) {
    if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > nx.timeout_ticks) {
      atomicOr(nx.err, 16u);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// Phase stamp of the IA_PROBE & 8 diagnostic builds, on the sampled wave only (on): gst[k] = the
// clock once everything issued so far has completed
#if IA_PROBE & 8
#define IA_GST(on, gst, k) do { if (on) { __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_sched_barrier(0); \
                                          (gst)[k] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define IA_GST(on, gst, k) do { } while (0)
#endif

// The pruning record (uniform values) of a query with |q'|^2 = ss, projections p and exact U'
// candidate distance u (DBL_MAX: no candidate); ksc the key scale, ufac the level's U' factor.
// o0 / o1: the projection interval; o2: U' and the Morton key, and K3p's hi x hi block filter
// bound (ia_k3h.hip k3p_bound): value bound
// z >= U' - |q'|^2 with the f32 rounding of z and of the kernel's lim = z + R_t (...)
// (2^-22 (|q'|^2 + U')) and the subnormal / norm-column terms (2^-24 (16 |q'| + 300));
// w = 2^-8 |q'| (twice the relative error term's |q'| part)
__device__ __forceinline__ void prune_record(double ss, const double (&pp)[IA_NPC], double u, const double *ksc, double ufac,
                                             float4 &o0, float4 &o1, float4 &o2) {
  const double p[IA_NPC] = {pp[0], pp[1], pp[2], pp[3]};  // (a copy: the caller's array stays in registers)
  const double qn = sqrt(ss);
  const bool fin = u < DBL_MAX;
  const unsigned key = fin ? prune_key(p, ksc) : IA_PRUNE_KEY_INF;
  const float up = fin ? round_up_f(u * ufac) : INFINITY;
  const float z = fin ? round_up_f((double)up - ss + 0x1p-22 * (ss + (double)up) + 0x1p-24 * (16.0 * qn + 300.0)) : INFINITY;
  const float w = round_up_f(0x1p-8 * qn * (1.0 + 0x1p-40));
  o0 = make_float4(round_down_f(p[0] - IA_PRUNE_MABS), round_down_f(p[1] - IA_PRUNE_MABS), round_down_f(p[2] - IA_PRUNE_MABS),
                   round_down_f(p[3] - IA_PRUNE_MABS));
  o1 = make_float4(round_up_f(p[0] + IA_PRUNE_MABS), round_up_f(p[1] + IA_PRUNE_MABS), round_up_f(p[2] + IA_PRUNE_MABS),
                   round_up_f(p[3] + IA_PRUNE_MABS));
  o2 = make_float4(up, __uint_as_float(key), z, w);
}
// query m's |q'|^2 and pruning record, from lane 0
__device__ __forceinline__ void prune_record_store(int lane, int m, double *qn2, float4 *qinfo, double ss, const float4 &o0,
                                                   const float4 &o1, const float4 &o2) {
  if (lane == 0) {
    qn2[m] = ss;
    qinfo[3 * m] = o0;
    qinfo[3 * m + 1] = o1;
    qinfo[3 * m + 2] = o2;
  }
}

// K2p's pad query m >= J M: zero fragments, an empty pruning record
template <int KS>
__device__ __forceinline__ void gather_p_pad(int m, int lane, _Float16 *qf, float4 *qinfo, float4 &o0, float4 &o1,
                                             float4 &o2) {
  if (lane < 16 * KS) put_qh<KS>(qf, m, lane, 0.);
  o0 = o1 = make_float4(0.f, 0.f, 0.f, 0.f);
  o2 = make_float4(-INFINITY, __uint_as_float(IA_PRUNE_KEY_PAD), -INFINITY, 0.f);
  if (lane == 0) {
    qinfo[3 * m] = o0;
    qinfo[3 * m + 1] = o1;
    qinfo[3 * m + 2] = o2;
  }
}

// A fused gather's inputs that do not depend on the launch's own merges, loaded during the merge
// (k_merge_gather): lane f < 55 the query's feature f as K2p reads it (the B' part stale exactly
// at the two step-t pixels of QHand, which the gather substitutes), lane k < 15 the causal
// neighbour k's source pixel and A' image (stale at the same two pixels)
struct QPre {
  bool on = false;
  double v = 0.;
  int sr = 0, sc = 0, si = 0;
  int nn = -1;  // lane 15 + k: causal neighbour k's exact NN row (option "nn_bound")
};
__device__ __forceinline__ QPre qpre_load(const LevelGeo &g, const StepDesc &sn, const Imgs &B, const JobPtrs &jp, int m, int lane) {
  constexpr int D = 55;
  QPre p;
  p.on = true;
  const QPix px = ia_qpix(sn, g.bw, m);
  const int r = px.r, c = px.c;
  if (lane < D) p.v = win_feat(Geo<1>{}, B, lane, r, c, 0);
  // lane k < 15 and, with exact NN rows kept, lane 15 + k: causal cell k (causal_nb's lane roles)
  const CausalNb n = causal_nb(g, r, c, px.qi, lane, jp.nn && lane >= 15 && lane < 30);
  if (n.ok && lane < 15) {
    p.sr = jp.s[2 * n.nb];
    p.sc = jp.s[2 * n.nb + 1];
    p.si = jp.im[n.nb];
  }
  if (n.ok && lane >= 15) p.nn = jp.nn[n.nb];
  return p;
}

// U' candidate row of lane (0..14: coherence candidate of causal neighbour lane, 15..29: the
// neighbour's NN row shifted; gather_p_query's sets) from the neighbour's s / im / NN row, -1 when
// it falls outside A or the neighbour has none
__device__ __forceinline__ int ucand_row(const LevelGeo &g, int r, int c, int nr, int nc, bool nnl, int sr, int sc, int si,
                                         int nnrow) {
  if (nnl) {
    sr = -1;
    if (nnrow >= 0 && nnrow < g.NA) {
      const unsigned hw = (unsigned)g.ah * (unsigned)g.aw;
      si = (int)((unsigned)nnrow / hw);
      const unsigned rem = (unsigned)nnrow - (unsigned)si * hw;
      sr = (int)(rem / (unsigned)g.aw);
      sc = (int)(rem - (unsigned)sr * (unsigned)g.aw);
    }
  }
  const ShiftedSrc t = shifted_src(g.ah, g.aw, sr, sc, r, c, nr, nc);
  return (sr >= 0 && t.ok) ? src_row(g.ah, g.aw, si, t.tr, t.tc) : -1;
}

// K2p's work for one query m of step sd (one wave): q64, qn2, fragments, pruning record (also
// returned, uniform, for the owner-computes publish); xh0 / xh1 (optional) receive the query's
// hi / lo columns
template <int KS, bool FUSE>
__device__ __forceinline__ void gather_p_query(const LevelGeo &g, const StepDesc &sd, const Imgs &B, const JobPtrs &jp, int m,
                                               int lane, const double *__restrict__ mu_part, double *__restrict__ q64,
                                               double *__restrict__ qn2, _Float16 *__restrict__ qf,
                                               const double *__restrict__ db64, const double *__restrict__ basis, double ufac,
                                               float4 *__restrict__ qinfo, double *qsh, _Float16 *xh0,
                                               _Float16 *xh1, const QHand &h, float4 &o0, float4 &o1, float4 &o2,
                                               const QPre &pf = QPre{}, unsigned long long *gst = nullptr) {
  constexpr int D = 55, KD = 16 * KS;
  IA_GST(gst, gst, 0);
  static_assert(KD <= IA_WAVE, "one feature per lane");
  const QPix px = ia_qpix(sd, g.bw, m);
  const int32_t *__restrict__ s = jp.s, *__restrict__ im = jp.im;
  const int r = px.r, c = px.c, qi = px.qi;
  // U' candidate of this lane: lanes 0..14 the coherence candidates (product(rows, cols) order as
  // merge_fused); with option "nn_bound" lanes 15..29 the same causal neighbours' exact NN rows,
  // shifted by the neighbour's offset like a coherence candidate.  Any DB row's exact distance
  // bounds the NN distance from above, so U' stays a valid bound whatever row a slot holds (an
  // out-of-range or missing one is skipped); only its tightness depends on them.
  int crow = -1;
  const bool nnl = jp.nn && lane >= 15 && lane < 30;
  {
    const CausalNb n = causal_nb(g, r, c, qi, lane, nnl);
    const int nr = n.nr, nc = n.nc, nb = n.nb;
    if (n.ok) {
      int sr = 0, sc = 0, si = 0, nnrow = -1;
      if (!nnl) {
        if (FUSE && nr == h.r0 && nc == h.c0) {
          sr = h.s0r; sc = h.s0c; si = h.i0;
        } else if (FUSE && nr == h.r1 && nc == h.c1) {
          sr = h.s1r; sc = h.s1c; si = h.i1;
        } else if (pf.on) {
          sr = pf.sr; sc = pf.sc; si = pf.si;
        } else {
          sr = s[2 * nb]; sc = s[2 * nb + 1]; si = im[nb];
        }
      } else {
        nnrow = (FUSE && nr == h.r0 && nc == h.c0) ? h.n0
                : (FUSE && nr == h.r1 && nc == h.c1) ? h.n1
                : pf.on ? pf.nn : jp.nn[nb];
      }
      crow = ucand_row(g, r, c, nr, nc, nnl, sr, sc, si, nnrow);
    }
  }
  double ss = 0., p[IA_NPC];
#pragma unroll
  for (int i = 0; i < IA_NPC; i++) p[i] = 0.;
  if (lane < KD) {
    const int f = lane;
    if (f < D) {
      double v;
      if (pf.on) {  // prefetched; the B' part substituted at the two step-t pixels
        v = pf.v;
        if (FUSE && f >= 43) {
          int y, x;
      bslot(B, f - 43, r, c, y, x);
          v = (y == h.r0 && x == h.c0) ? h.v0 : (y == h.r1 && x == h.c1) ? h.v1 : v;
        }
      } else {
        v = feat_q1<FUSE>(B, f, r, c, h);
      }
      q64[(int64_t)m * D + f] = v;
      qsh[f] = v;
      const double qc = v - mu_part[feat_part<1>(f)];
      ss = qc * qc;
      put_qh<KS>(qf, m, f, -2.0 * qc);
      if (xh0) split_h(-2.0 * qc, xh0[f], xh1[f]);
#pragma unroll
      for (int i = 0; i < IA_NPC; i++) p[i] = basis[i * D + f] * qc;
    } else {
      put_qh<KS>(qf, m, f, f == D ? IA_NORM_SCALE : 0.);
      if (xh0) split_h(f == D ? IA_NORM_SCALE : 0., xh0[f], xh1[f]);
    }
  }
  IA_GST(gst, gst, 1);
  ss = wave_sum_d(ss);
#pragma unroll
  for (int i = 0; i < IA_NPC; i++) p[i] = wave_sum_d_x(p[i]);
  IA_GST(gst, gst, 2);
  __builtin_amdgcn_wave_barrier();  // qsh written by this wave's lanes, read below
  double u = DBL_MAX;
  if (crow >= 0) u = exact_dist_level<1>(db64, crow, qsh);
  u = wave_min_d_x(u);
  IA_GST(gst, gst, 3);
  prune_record(ss, p, u, basis + IA_NPC * D, ufac, o0, o1, o2);
  prune_record_store(lane, m, qn2, qinfo, ss, o0, o1, o2);
  IA_GST(gst, gst, 4);
}
// K2h's work for one query m of step sd (unpruned split-f16 levels), with the fused gather's
// two step-t pixels substituted (QHand) in the B' part
template <int KS>
__device__ __forceinline__ void gather_h_query_fused(const LevelGeo &g, const StepDesc &sd, const Imgs &B, int m, int lane,
                                                     const double *__restrict__ mu_part, double *__restrict__ q64,
                                                     double *__restrict__ qn2, _Float16 *__restrict__ qf, const QHand &h) {
  constexpr int D = 55, KD = 16 * KS;
  static_assert(KD <= IA_WAVE, "one feature per lane");
  const QPix px = ia_qpix(sd, g.bw, m);
  const int r = px.r, c = px.c;
  double ss = 0.;
  if (lane < KD) {
    const int f = lane;
    if (f < D) {
      double v;
      if (f >= 43) {  // the B' part (causal 5x5 at (r, c), k < 12)
        int y, x;
      bslot(B, f - 43, r, c, y, x);
        v = (y == h.r0 && x == h.c0) ? h.v0 : (y == h.r1 && x == h.c1) ? h.v1 : B.p3[(int64_t)y * B.w + x];
      } else {
        v = win_feat(Geo<1>{}, B, f, r, c, 0);
      }
      q64[(int64_t)m * D + f] = v;
      const double qc = v - mu_part[feat_part<1>(f)];
      ss = qc * qc;
      put_qh<KS>(qf, m, f, -2.0 * qc);
    } else {
      put_qh<KS>(qf, m, f, f == D ? IA_NORM_SCALE : 0.);
    }
  }
  ss = wave_sum_d(ss);
  if (lane == 0) qn2[m] = ss;
}

// Per-level constants of the fused gather (lane f < 55: its feature's basis column and part mean;
// the key scale), loaded at wave start so no dependent load of them sits behind the handoff.
struct QConst {
  double bas[IA_NPC] = {0., 0., 0., 0.};
  double mu = 0.;
  double sc[IA_NPC] = {0., 0., 0., 0.};
};
__device__ __forceinline__ QConst qconst_load(const NextStep &nx, int lane) {
  constexpr int D = 55;
  QConst k;
  if (lane < D) {
#pragma unroll
    for (int i = 0; i < IA_NPC; i++) k.bas[i] = nx.basis[i * D + lane];
    k.mu = nx.mu[feat_part<1>(lane)];
  }
#pragma unroll
  for (int i = 0; i < IA_NPC; i++) k.sc[i] = nx.basis[IA_NPC * D + i];
  return k;
}

// The pieces the early gathers share (gather_p_early; the two-wave form below).
// A U' candidate row requested (row 0 where the lane has none: the loads are unconditional) ...
using GatherRow = double2[Geo<1>::DS / 2];
__device__ __forceinline__ void gather_row_load(const double *__restrict__ db64, int crow, GatherRow &rowv) {
  constexpr int DS = Geo<1>::DS;
  const double2 *src = reinterpret_cast<const double2 *>(db64 + (int64_t)(crow >= 0 ? crow : 0) * DS);
#pragma unroll
  for (int i = 0; i < DS / 2; i++) rowv[i] = src[i];
}
// ... and its U' partial distance over the non-late features (pairwise order; a late feature, mask
// lm, adds 0) with the row's values at the twelve B' slots (read after a handoff for the late ones)
__device__ __forceinline__ void gather_row_part(const GatherRow &rowv, const double *qsh, unsigned long long lm, double &part,
                                                double *al) {
  constexpr int D = 55;
  const double *rv = reinterpret_cast<const double *>(rowv);
  part = pw_sum<D>([&](int f) {
    const double d = rv[f] - qsh[f];
    return ((lm >> f) & 1ull) ? 0. : d * d;
  });
#pragma unroll
  for (int k = 0; k < 12; k++) al[k] = rv[43 + k];
}
__device__ __forceinline__ void gather_wave_row(const double *__restrict__ db64, int crow, const double *qsh,
                                                unsigned long long lm, double &part, double *al) {
  GatherRow rowv;
  gather_row_load(db64, crow, rowv);
  gather_row_part(rowv, qsh, lm, part, al);
}
// One late pixel's slots (mask lm, value v; qc: its centred value in the slots' lanes), in slot
// order: its terms of |q'|^2, the projections (bas: the lanes' basis columns) and this lane's U'
// distance (al: its row's values at the B' slots)
__device__ __forceinline__ void gather_late_slots(unsigned long long lm, double v, double qc, const double (&bas)[IA_NPC],
                                                  const double *al, double &ss, double *p, double &part) {
#pragma unroll
  for (int k = 0; k < 12; k++) {
    if ((lm >> (43 + k)) & 1ull) {  // wave-uniform
      const double qcl = readlane_d(qc, 43 + k);
      ss += qcl * qcl;
#pragma unroll
      for (int i = 0; i < IA_NPC; i++) p[i] += readlane_d(bas[i], 43 + k) * qcl;
      const double d = al[k] - v;
      part += d * d;
    }
  }
}

// The fused gather of query mn (step t + 1) for a merge wave of a one-rank pruned level (option
// "prefetch_next"; no publish): everything that does not depend on the row above's step-t result
// runs BEFORE the wait for its handoff - the query's other 54 features (q64, split-f16 fragments,
// projections, |q'|^2 as sums over those lanes) and U': the exact distance of each candidate row
// over those features, the rows requested first so their loads are in flight during the feature
// work.  After the handoff only the late feature (the row above's pixel (r - 1, c + 2) of the
// query's window) is added to each sum.  U' skips the row above's own two candidates (its source
// pixel and NN row, shifted): any DB row's exact distance bounds the NN distance from above, so U'
// stays a valid bound (the scan's passing tiles 0.144 -> 0.147); the summation
// orders of U', |q'|^2 and the projections differ from K2p's, which the bounds' margins cover
// (the NN decisions are the merge's fp64 reranks, unchanged).
template <int KS>
__device__ __forceinline__ void gather_p_early(const LevelGeo &g, const NextStep &nx, const Imgs &B, const JobPtrs &jp,
                                               int job, int mn, int lane, const double *__restrict__ db64, double *qsh,
                                               const QHand &h0, const QPre &pf, const QConst &qk) {
  constexpr int D = 55, KD = 16 * KS;
  static_assert(KD <= IA_WAVE, "one feature per lane");
#if IA_PROBE & 8
  unsigned long long gst[7] = {__builtin_amdgcn_s_memtime(), 0, 0, 0, 0, 0, 0};
  const bool gprobe = mn == nx.sn.M / 2 && (nx.sn.t % 256) == 129;
#endif
  const StepDesc &sn = nx.sn;
  const QPix pn = ia_qpix(sn, g.bw, mn);
  const int r = pn.r, c = pn.c, qi = pn.qi;
  // the row above's step-t pixel: its result arrives through the handoff slot of row r - 1
  const bool above = r >= 1 && c + 2 < g.bw;
  const int ar = r - 1, ac = c + 2;
  // ---- features (lane f < 55): the prefetched value, this wave's own result substituted
  double v = 0.;
  bool late = false;
  if (lane < D) {
    v = pf.v;
    if (lane >= 43) {
      int y, x;
      bslot(B, lane - 43, r, c, y, x);
      if (y == h0.r0 && x == h0.c0) v = h0.v0;
      late = above && y == ar && x == ac;
    }
  }
  // (the late pixel can fill several window slots where the window is reflected at the image's
  // top or sides: up to four of the twelve B' slots 43..54)
  const unsigned long long lm = __ballot(late);
  // ---- U' candidate rows: lanes 0..14 the causal neighbours' shifted sources, 15..29 (option
  // "nn_bound") their shifted NN rows; the row above's pixel skipped (its result is late)
  int crow = -1;
  const bool nnl = jp.nn && lane >= 15 && lane < 30;
  {
    const CausalNb n = causal_nb(g, r, c, qi, lane, nnl);
    const int nr = n.nr, nc = n.nc;
    if (n.ok && !(above && nr == ar && nc == ac)) {
      const bool own = nr == h0.r0 && nc == h0.c0;
      const int sr = own ? h0.s0r : pf.sr, sc = own ? h0.s0c : pf.sc, si = own ? h0.i0 : pf.si;
      const int nnrow = own ? h0.n0 : pf.nn;
      crow = ucand_row(g, r, c, nr, nc, nnl, sr, sc, si, nnrow);
    }
  }
  // the candidate row, requested now (in flight during the feature work below)
  GatherRow rowv;
  gather_row_load(db64, crow, rowv);
  if (lane < D) qsh[lane] = late ? 0. : v;
  // ---- the non-late features: q64, fragments, projections, |q'|^2 (late lanes hold 0)
  double ss = 0., p[IA_NPC] = {0., 0., 0., 0.}, qc = 0.;
  if (lane < KD) {
    if (lane < D) {
      if (!late) {
        nx.q64[(int64_t)mn * D + lane] = v;
        qc = v - qk.mu;
        ss = qc * qc;
        put_qh<KS>((_Float16 *)nx.qf, mn, lane, -2.0 * qc);
#pragma unroll
        for (int i = 0; i < IA_NPC; i++) p[i] = qk.bas[i] * qc;
      }
    } else {
      put_qh<KS>((_Float16 *)nx.qf, mn, lane, lane == D ? IA_NORM_SCALE : 0.);
    }
  }
  ss = wave_sum_d_x(ss);
#pragma unroll
  for (int i = 0; i < IA_NPC; i++) p[i] = wave_sum_d_x(p[i]);
  IA_GST(gprobe, gst, 1);
  __builtin_amdgcn_wave_barrier();  // qsh written by this wave's lanes, read below
  // ---- U' partial distances over the non-late features (pairwise order; a late feature adds 0)
  double part, al[12];
  gather_row_part(rowv, qsh, lm, part, al);
  IA_GST(gprobe, gst, 2);
  // ---- the row above's result (handoff)
  QHand h = h0;
  if (above) {
    const HandSlot *hs = nx.hand + (int64_t)job * g.bh + ar;
    handoff_wait(hs, nx);
    h.v1 = hs->v;
  }
  IA_GST(gprobe, gst, 3);
  // ---- the late slots: their value, fragments and terms, in slot order
  if (lm) {
    if (late) {
      nx.q64[(int64_t)mn * D + lane] = h.v1;
      qc = h.v1 - qk.mu;
      put_qh<KS>((_Float16 *)nx.qf, mn, lane, -2.0 * qc);
    }
    gather_late_slots(lm, h.v1, qc, qk.bas, al, ss, p, part);
  }
  double u = crow >= 0 ? part : DBL_MAX;
  u = wave_min_d_x(u);
  IA_GST(gprobe, gst, 4);
  float4 o0, o1, o2;
  prune_record(ss, p, u, qk.sc, nx.ufac, o0, o1, o2);
  prune_record_store(lane, mn, nx.qn2, nx.qinfo, ss, o0, o1, o2);
  IA_GST(gprobe, gst, 5);
#if IA_PROBE & 8
  if (gprobe && lane == 0)
    printf("ESTAMP bw=%d t=%d M=%d pre=%llu part=%llu handoff=%llu late=%llu rec=%llu\n", g.bw, sn.t, sn.M, gst[1] - gst[0],
           gst[2] - gst[1], gst[3] - gst[2], gst[4] - gst[3], gst[5] - gst[4]);
#endif
}

// The gather wave of a two-wave merge + gather workgroup (option "gather_wave", ia_kernels.hip
// merge_gather_pair): gather_p_early's work split at the merge wave's result instead of behind it.
// The query's window holds TWO late pixels here: the workgroup's own (r, c - 1), merged by wave 0
// while this wave runs, and the row above's (r - 1, c + 2); under reflection each can fill several
// of the twelve B' slots.  gather_wave_pre runs from wave start and needs neither: the constants
// and prefetched inputs, the candidate rows of every causal neighbour but those two pixels, and
// all sums (q64, fragments, projections, |q'|^2, the U' partial distances) over the non-late
// features.  gather_wave_next, still beside the merge, loads the raster successors of the rows
// the merge wave holds.  gather_wave_post takes the own result: its two candidate rows (shifted
// source and shifted NN row) from those successors by lane, the own late slots, then the row
// above's handoff and late slots, and the pruning record.  U' runs over the same candidate rows as
// gather_p_early's; only the summation order of the own pixel's terms differs (added in slot order
// after the pairwise / butterfly sums instead of inside them), which the bounds' margins cover.
struct GatherWave {
  QConst qk;
  bool late0 = false, late1 = false;   // this lane's feature is a slot of the own / the row above's pixel
  bool own = false;                    // this lane's U' candidate comes from the own pixel
  unsigned long long lm0 = 0, lm1 = 0; // the two pixels' slots (features 43..54), wave-uniform
  int crow = -1;
  double qc = 0., ss = 0., p[IA_NPC] = {0., 0., 0., 0.};
  double part = 0., al[12] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  // gather_wave_next: the same of row2, the raster successor of the merge wave's row of this lane
  int row2 = -1;
  double part2 = 0., al2[12] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
#if IA_PROBE & 8
  unsigned long long t0 = 0, t1 = 0, t2 = 0;
#endif
};
template <int KS>
__device__ __forceinline__ GatherWave gather_wave_pre(const LevelGeo &g, const NextStep &nx, const Imgs &B, const JobPtrs &jp,
                                                      int mn, int lane, const double *__restrict__ db64, double *qsh) {
  constexpr int D = 55, KD = 16 * KS;
  static_assert(KD <= IA_WAVE, "one feature per lane");
  GatherWave w;
#if IA_PROBE & 8
  w.t0 = __builtin_amdgcn_s_memtime();
#endif
  w.qk = qconst_load(nx, lane);
  const QPre pf = qpre_load(g, nx.sn, B, jp, mn, lane);
  const QPix pn = ia_qpix(nx.sn, g.bw, mn);
  const int r = pn.r, c = pn.c, qi = pn.qi;
  const bool above = r >= 1 && c + 2 < g.bw;
  const int ar = r - 1, ac = c + 2, orr = r, oc = c - 1;  // the two step-t pixels
  if (lane >= 43 && lane < D) {
    int y, x;
    bslot(B, lane - 43, r, c, y, x);
    w.late0 = y == orr && x == oc;
    w.late1 = above && y == ar && x == ac;
  }
  w.lm0 = __ballot(w.late0);
  w.lm1 = __ballot(w.late1);
  const bool late = w.late0 || w.late1;
  // ---- U' candidate rows (gather_p_early's lanes); the two late pixels' skipped here
  const bool nnl = jp.nn && lane >= 15 && lane < 30;
  {
    const CausalNb n = causal_nb(g, r, c, qi, lane, nnl);
    const int nr = n.nr, nc = n.nc;
    if (n.ok && !(above && nr == ar && nc == ac)) {
      if (nr == orr && nc == oc) w.own = true;
      else w.crow = ucand_row(g, r, c, nr, nc, nnl, pf.sr, pf.sc, pf.si, pf.nn);
    }
  }
  if (lane < D) qsh[lane] = late ? 0. : pf.v;
  // ---- the non-late features: q64, fragments, projections, |q'|^2 (late lanes hold 0)
  if (lane < KD) {
    if (lane < D) {
      if (!late) {
        nx.q64[(int64_t)mn * D + lane] = pf.v;
        w.qc = pf.v - w.qk.mu;
        w.ss = w.qc * w.qc;
        put_qh<KS>((_Float16 *)nx.qf, mn, lane, -2.0 * w.qc);
#pragma unroll
        for (int i = 0; i < IA_NPC; i++) w.p[i] = w.qk.bas[i] * w.qc;
      }
    } else {
      put_qh<KS>((_Float16 *)nx.qf, mn, lane, lane == D ? IA_NORM_SCALE : 0.);
    }
  }
  w.ss = wave_sum_d_x(w.ss);
#pragma unroll
  for (int i = 0; i < IA_NPC; i++) w.p[i] = wave_sum_d_x(w.p[i]);
  __builtin_amdgcn_wave_barrier();  // qsh written by this wave's lanes, read below
#if IA_PROBE & 8
  __builtin_amdgcn_s_waitcnt(0);
  w.t1 = __builtin_amdgcn_s_memtime();
#endif
  gather_wave_row(db64, w.crow, qsh, w.lm0 | w.lm1, w.part, w.al);
#if IA_PROBE & 8
  __builtin_amdgcn_s_waitcnt(0);
  w.t2 = __builtin_amdgcn_s_memtime();
#endif
  return w;
}
// No dependent row round after the merge: the own pixel's two U' candidates for query (r, c + 1)
// are `final source + 1` and `NN winner + 1` in A's raster, and both winners are among the rows
// the merge wave's lanes hold after placement (prow, posted without waiting).  Lane l loads row
// prow[l] + 1 where that stays inside the image row, and keeps its partial distance and B'-slot
// values; gather_wave_post picks the two winners' by lane.  The poll is bounded like every wait
// (err bit 16; then no lane has a row and the post part loads its two rows itself).
__device__ __forceinline__ void gather_wave_next(const LevelGeo &g, const NextStep &nx, const int *prow, int *prow_on,
                                                 int lane, const double *__restrict__ db64, const double *qsh,
                                                 GatherWave &w) {
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  bool ok = true;
  while (__hip_atomic_load(prow_on, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != 1) {
    if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > nx.timeout_ticks) {
      atomicOr(nx.err, 16u);
      ok = false;
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  if (ok) {
    const int mr = prow[lane];
    if (mr >= 0 && mr < g.NA && (unsigned)mr % (unsigned)g.aw + 1 < (unsigned)g.aw) w.row2 = mr + 1;
  }
  gather_wave_row(db64, w.row2, qsh, w.lm0 | w.lm1, w.part2, w.al2);
#if IA_PROBE & 8
  __builtin_amdgcn_s_waitcnt(0);
  w.t2 = __builtin_amdgcn_s_memtime();
#endif
}
// h: the own pixel's result (r0, c0, v0, s0r, s0c, i0, n0) from the merge wave
template <int KS>
__device__ __forceinline__ void gather_wave_post(const LevelGeo &g, const NextStep &nx, const JobPtrs &jp, int job, int mn,
                                                 int lane, const double *__restrict__ db64, const double *qsh, const QHand &h,
                                                 int src_lane, int app_lane, GatherWave &w) {
  constexpr int D = 55;
#if IA_PROBE & 8
  unsigned long long gst[5] = {__builtin_amdgcn_s_memtime(), 0, 0, 0, 0};
  const bool gprobe = mn == nx.sn.M / 2 && (nx.sn.t % 256) == 129;
#endif
  const QPix pn = ia_qpix(nx.sn, g.bw, mn);
  const int r = pn.r, c = pn.c;
  const bool above = r >= 1 && c + 2 < g.bw;
  // ---- the own pixel's two candidates: the shifted source (lane 11's) is the successor of the
  // row the merge wave's lane src_lane held, the shifted NN row (lane 26's) of lane app_lane's:
  // their partials by lane read (gather_wave_next).  A winner no lane held (an overflow candidate,
  // a certification rescan; rare) takes the dependent row load.
  const int from = lane < 15 ? src_lane : app_lane;
  const int fl = from >= 0 ? from : lane;
  const int row2 = __shfl(w.row2, fl, 64);
  const double part2 = __shfl(w.part2, fl, 64);
  double al2[12];
#pragma unroll
  for (int k = 0; k < 12; k++) al2[k] = __shfl(w.al2[k], fl, 64);
  if (w.own) {
    w.crow = ucand_row(g, r, c, h.r0, h.c0, lane >= 15, h.s0r, h.s0c, h.i0, h.n0);
    if (from >= 0 && row2 == w.crow) {
      w.part = part2;
#pragma unroll
      for (int k = 0; k < 12; k++) w.al[k] = al2[k];
    } else {
      gather_wave_row(db64, w.crow, qsh, w.lm0 | w.lm1, w.part, w.al);
    }
  }
  // ---- its late slots
  if (w.late0) {
    nx.q64[(int64_t)mn * D + lane] = h.v0;
    w.qc = h.v0 - w.qk.mu;
    put_qh<KS>((_Float16 *)nx.qf, mn, lane, -2.0 * w.qc);
  }
  gather_late_slots(w.lm0, h.v0, w.qc, w.qk.bas, w.al, w.ss, w.p, w.part);
  IA_GST(gprobe, gst, 1);
  // ---- the row above's result (handoff), then its late slots
  if (above) {
    const HandSlot *hs = nx.hand + (int64_t)job * g.bh + (r - 1);
    handoff_wait(hs, nx);
    const double v1 = hs->v;
    IA_GST(gprobe, gst, 2);
    if (w.late1) {
      nx.q64[(int64_t)mn * D + lane] = v1;
      w.qc = v1 - w.qk.mu;
      put_qh<KS>((_Float16 *)nx.qf, mn, lane, -2.0 * w.qc);
    }
    gather_late_slots(w.lm1, v1, w.qc, w.qk.bas, w.al, w.ss, w.p, w.part);
  } else {
    IA_GST(gprobe, gst, 2);
  }
  double u = w.crow >= 0 ? w.part : DBL_MAX;
  u = wave_min_d_x(u);
  IA_GST(gprobe, gst, 3);
  float4 o0, o1, o2;
  prune_record(w.ss, w.p, u, w.qk.sc, nx.ufac, o0, o1, o2);
  prune_record_store(lane, mn, nx.qn2, nx.qinfo, w.ss, o0, o1, o2);
  IA_GST(gprobe, gst, 4);
#if IA_PROBE & 8
  if (gprobe && lane == 0)
    printf("WSTAMP bw=%d t=%d M=%d pre=%llu part=%llu wait_merge=%llu own=%llu handoff=%llu late=%llu rec=%llu\n", g.bw,
           nx.sn.t, nx.sn.M, w.t1 - w.t0, w.t2 - w.t1, gst[0] - w.t2, gst[1] - gst[0], gst[2] - gst[1], gst[3] - gst[2],
           gst[4] - gst[3]);
#endif
}

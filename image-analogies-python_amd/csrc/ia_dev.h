// ia_dev.h — device code shared by the kernel translation units of the Image Analogies
// best-match path (CDNA4, gfx950), one unit per stage:
//
//   ia_level_db.hip     K0 k_part_means, K1 k_db_build / k_db_build_h, K1b k_db64_build: the
//                       level's feature DB (create_index, algorithms.py:11-47,50-70)
//   ia_gather.hip       K2 k_gather_query / _h / _p: BBp_feat of every pixel of one wavefront
//                       step (image_analogies.py:166-168, algorithms.py:78-89)
//   ia_k3.hip           K3 k3_dist: best_approximate_match's distance scan (algorithms.py:73-75)
//                       as a v_mfma_f32_32x32x2_f32 contraction with a fused per-query top-2; the
//                       scan body (staging, tile loop, MFMA chain) is ia_k3_scan.h's
//   ia_kernels.hip      K4 k_merge_level, k_merge_gather: exact fp64 rerank of the MFMA candidates
//                       (numpy pairwise-sum order, lowest-index ties), certification with exact
//                       fallback rescan, best_coherence_match (algorithms.py:92-130),
//                       compute_distance (:133-135), the kappa rule (image_analogies.py:206) and
//                       the B'/s/im writeback (:214-220), one wave per query pixel
//   ia_merge_shard.hip  k_finish_level, k_merge_xchg: the merges of a sharded level
//   ia_dense.hip        dense variants for the FLANN-compatible index (ia_index_*), statistics,
//                       stamps, microbenchmark operands
//   ia_k3r.hip          the index's fixed-radius search: the same scan body (ia_k3_scan.h) with a
//                       threshold epilogue (count and fill passes), exact verification, per-query
//                       sort (ia_index_*_radius)
//   ia_kcoh.hip         k-coherence levels: a step without a DB scan (ia_synthesize_levels_kcoh)
//   ia_nbhd.hip         exact levels for run-time window sizes (ia_synthesize_levels_nbhd)
//   ia_mask.hip         masked resynthesis: step lists and list-driven steps (ia_synthesize_levels_masked)
//   ia_ann.hip          the approximate index: k-means lists whose queries honour checks (ia_ann_*)
//
// The per-pixel window rule lives here, once, for all of them: win_feat (feature f of a pixel),
// causal_cell / shifted_src / src_row (window cell -> neighbour -> shifted source -> DB row),
// blas_dot_sq and kappa_rule; the geometry is a constant (Geo<CH>, Pad2) on the default path and a
// run-time value (NbhdGeo, int) in ia_nbhd.hip and k_coherence_batch.  ia_internal.h has ia_qpix
// (step query -> pixel, any skew), ia_certify.h the coherence pick and the kappa finish over a row
// policy.
//
// Here: feature geometry and access, numpy's and OpenBLAS's summation orders, the wave
// reductions, the exact row distances and the certification bounds; at the end the two host
// helpers every launcher dispatches through.  ia_certify.h, ia_topk.h (the index's certified
// k-NN list) and ia_gather.h build on it.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no FMA contraction: the exact
// fp64 paths must round exactly like numpy's separate multiply and add).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "ia_internal.h"
#include "ia_prune.h"
#include "ia_top2.h"

#ifndef IA_PROBE
#define IA_PROBE 0  // diagnostic phase-stamp builds (8: merge, 16: K3p; never the product build)
#endif
// waves (= queries) per workgroup of the one-wave-per-query kernels K2h, K2p, K4: one, so a
// step's few hundred latency-bound waves spread over as many CUs (their L1, TA and LDS) as
// possible; 3.35 -> 3.44 M px/s against 4 per workgroup on one box (profiles/r02/wpb)
#ifndef IA_PQ_WPB
#define IA_PQ_WPB 1
#endif
#define IA_PQ_WG (IA_WAVE * IA_PQ_WPB)

// ------------------------------------------------------------------------------------------
// feature geometry, compile-time per channel count
// ------------------------------------------------------------------------------------------
template <int CH>
struct Geo {
  static constexpr int D = 55 * CH;
  static constexpr int DP = ((D + 1 + 7) / 8) * 8;  // + norm column, 16-B aligned halves
  static constexpr int KH = DP / 2;                 // k-steps of the 32x32x2 chain
  static constexpr int KP = KH / 4;                 // float4 pieces per lane
  static constexpr int DS = ((D + 7) / 8) * 8;      // fp64 row-major DB row stride (doubles)
  // the windows and where a row's four parts start, under NbhdGeo's names (ia_launch.h): the
  // window rule below takes either, this one folding to constants
  static constexpr int ch = CH, n_sm = 3, n_lg = 5, p_s = 1, p_l = 2, o1 = 9 * CH, o2 = 34 * CH, o3 = 43 * CH;
};

// reflected (symmetric-pad) offsets of the 3x3 coarse and 5x5 fine windows of pixel (r, c)
struct Px {
  int64_t yc[3], yf[5];  // row offsets (already * width * CH)
  int xc[3], xf[5];      // column offsets (already * CH)
};
template <int CH>
__device__ __forceinline__ Px make_px(const Imgs &I, int r, int c) {
  Px P;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    P.yc[k] = (int64_t)ia_reflect((r >> 1) + k - 1, I.hc) * I.wc * CH;
    P.xc[k] = ia_reflect((c >> 1) + k - 1, I.wc) * CH;
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
    P.yf[k] = (int64_t)ia_reflect(r + k - 2, I.h) * I.w * CH;
    P.xf[k] = ia_reflect(c + k - 2, I.w) * CH;
  }
  return P;
}
// value of feature f (reference order) of pixel P of image `img`
// (A' index; 0 on the B side)
template <int CH>
__device__ __forceinline__ double featp(const Imgs &I, const Px &P, int f, int img) {
  if (f < 9 * CH) {
    const int k = f / CH, ch = f % CH;
    return I.p0[P.yc[k / 3] + P.xc[k % 3] + ch];
  } else if (f < 34 * CH) {
    const int k = (f - 9 * CH) / CH, ch = (f - 9 * CH) % CH;
    return I.p1[P.yf[k / 5] + P.xf[k % 5] + ch];
  } else if (f < 43 * CH) {
    const int k = (f - 34 * CH) / CH, ch = (f - 34 * CH) % CH;
    return I.p2[img * I.img_stride_c + P.yc[k / 3] + P.xc[k % 3] + ch];
  } else {
    const int k = (f - 43 * CH) / CH, ch = (f - 43 * CH) % CH;
    return I.p3[img * I.img_stride_f + P.yf[k / 5] + P.xf[k % 5] + ch];
  }
}
// feature f of pixel (r, c) for windows w (Geo<CH>{} or the window call's NbhdGeo): parts in the
// reference's order, each row-major and channel-minor, symmetric padding (ia_reflect takes any
// reach: periodic for images smaller than the pad); part 3 only reaches its first n_lg^2 / 2 cells
template <class W>
__device__ __forceinline__ double win_feat(const W &w, const Imgs &I, int f, int r, int c, int img) {
  int part, k, chn;
  if (f < w.o1) {
    part = 0; k = f / w.ch; chn = f % w.ch;
  } else if (f < w.o2) {
    part = 1; k = (f - w.o1) / w.ch; chn = (f - w.o1) % w.ch;
  } else if (f < w.o3) {
    part = 2; k = (f - w.o2) / w.ch; chn = (f - w.o2) % w.ch;
  } else {
    part = 3; k = (f - w.o3) / w.ch; chn = (f - w.o3) % w.ch;
  }
  if (part == 0 || part == 2) {  // n_sm x n_sm at (floor(r/2), floor(c/2)) of the padded coarse level
    const int y = ia_reflect((r >> 1) + k / w.n_sm - w.p_s, I.hc), x = ia_reflect((c >> 1) + k % w.n_sm - w.p_s, I.wc);
    const double *b = part == 0 ? I.p0 : I.p2 + img * I.img_stride_c;
    return b[((int64_t)y * I.wc + x) * w.ch + chn];
  }
  const int y = ia_reflect(r + k / w.n_lg - w.p_l, I.h), x = ia_reflect(c + k % w.n_lg - w.p_l, I.w);
  const double *b = part == 1 ? I.p1 : I.p3 + img * I.img_stride_f;
  return b[((int64_t)y * I.w + x) * w.ch + chn];
}

// ------------------------------------------------------------------------------------------
// the causal window rule (best_coherence_match, algorithms.py:92-130), written once for every
// level path: pad = p_l as a constant (Pad2: the default 5x5) or a run-time int (the window call,
// the index's coherence batch).  Integer arithmetic on loaded values only: the loads of s / im
// stay with the callers, whose placement of them differs on purpose.
// ------------------------------------------------------------------------------------------
typedef std::integral_constant<int, 2> Pad2;
template <class P>
__host__ __device__ constexpr int causal_cells(P pad) {  // cells of the (pad + 1) x (2 pad + 1) window
  return (pad + 1) * (2 * pad + 1);
}
// cell k (product(rows, cols) order) of pixel (r, c), raster index qi, in a level bw wide: its
// pixel and raster index; ok: inside the level and raster-earlier.  Ix, the type of qi: int on
// the level paths, int64_t where the pixel is the caller's and unchecked (the coherence batch)
template <class Ix>
struct CausalCell {
  int nr, nc;
  Ix nb;
  bool ok;
};
template <class P, class Ix>
__device__ __forceinline__ CausalCell<Ix> causal_cell(P pad, int bw, int r, int c, Ix qi, int k) {
  const int wd = 2 * pad + 1;
  CausalCell<Ix> n;
  n.nr = r - pad + k / wd;
  n.nc = c - pad + k % wd;
  n.ok = n.nr >= 0 && n.nc >= 0 && n.nc < bw && (Ix)n.nr * bw + n.nc < qi;
  n.nb = n.ok ? (Ix)n.nr * bw + n.nc : 0;
  return n;
}
// the source (sr, sc) of neighbour (nr, nc) shifted by its offset to the pixel (r, c): the pixel,
// and ok: inside A.  Its A' image plays no part, so a caller may load im[nb] after the test.
struct ShiftedSrc {
  int tr, tc;
  bool ok;
};
__device__ __forceinline__ ShiftedSrc shifted_src(int ah, int aw, int sr, int sc, int r, int c, int nr, int nc) {
  ShiftedSrc t;
  t.tr = sr + r - nr;
  t.tc = sc + c - nc;
  t.ok = t.tr >= 0 && t.tr < ah && t.tc >= 0 && t.tc < aw;
  return t;
}
// DB row of pixel (tr, tc) of A' image img.  Row: int on the level paths (their rows are int32),
// int64_t where img is the caller's and unchecked (the coherence batch)
template <class Row = int>
__device__ __forceinline__ Row src_row(int ah, int aw, int img, int tr, int tc) {
  return ((Row)img * ah + tr) * aw + tc;
}

// the B side of job jp as the four images its query rows read (B-side FeatDesc parts)
__device__ __forceinline__ Imgs job_imgs(Imgs B, const JobPtrs &jp) {
  B.p0 = jp.Bc;
  B.p1 = jp.B;
  B.p2 = jp.Bpc;
  B.p3 = jp.Bp;
  return B;
}

template <int CH>
__device__ __forceinline__ int feat_part(int f) {
  return f < 9 * CH ? 0 : f < 34 * CH ? 1 : f < 43 * CH ? 2 : 3;
}
template <int CH>
__device__ __forceinline__ int feat_ch(int f) {
  return (f < 9 * CH ? f : f < 34 * CH ? f - 9 * CH : f < 43 * CH ? f - 34 * CH : f - 43 * CH) % CH;
}

// numpy pairwise_sum (loops_utils.h.src) over n <= 128 terms produced in order by term(i)
template <int N, class T>
__device__ __forceinline__ double pw_block(T &&term, int off) {
  static_assert(N <= 128, "block");
  if constexpr (N < 8) {
    double res = 0.;
#pragma unroll
    for (int i = 0; i < N; i++) res += term(off + i);
    return res;
  } else {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = term(off + j);
    constexpr int NB = N - (N % 8);
#pragma unroll
    for (int i = 8; i < NB; i += 8) {
#pragma unroll
      for (int j = 0; j < 8; j++) r[j] += term(off + i + j);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
    for (int i = NB; i < N; i++) res += term(off + i);
    return res;
  }
}
// Correctly rounded fp64 square root, as numpy's np.sqrt / np.linalg.norm give on the host.
// Insurance against a device sqrt expansion that is not correctly rounded (the 1-ulp golden
// differences first blamed on it turned out to be libm pow, see pow2_alt): the result is
// settled among sqrt(x) and its two neighbours by the exact residual |x - y*y| (one fused
// multiply-add each).  Nearest-in-square equals nearest-in-root except in a window of relative
// width ~2^-106 around the rounding midpoint.
__device__ __forceinline__ double cr_sqrt(double x) {
  double y = sqrt(x);
  if (!(x > 0.) || !(x < DBL_MAX)) return y;
  const long long b = __double_as_longlong(y);
  const double yl = __longlong_as_double(b - 1), yh = __longlong_as_double(b + 1);
  double r = fabs(__builtin_fma(-y, y, x));
  const double rl = fabs(__builtin_fma(-yl, yl, x)), rh = fabs(__builtin_fma(-yh, yh, x));
  if (rl < r) {
    y = yl;
    r = rl;
  }
  if (rh < r) y = yh;
  return y;
}

// compute_distance's final `** 2` is libm pow(y, 2.0) on a numpy scalar, K4 uses y * y.  They
// differ only when the exact square lies next to a rounding midpoint (glibc pow is accurate to
// ~0.52 ulp; measured: every difference has |y*y - hi| >= 0.986 half-ulp).  pow2_alt returns the
// other value pow may give there (hi itself elsewhere) so K4 can flag a kappa decision that
// would flip between the two (pstat bit 29, ia_stats.kappa_ambiguous).
__device__ __forceinline__ double pow2_alt(double y, double hi) {
  if (!(hi > 0.) || !(hi < DBL_MAX)) return hi;
  const double lo = __builtin_fma(y, y, -hi);  // y*y = hi + lo exactly
  const long long b = __double_as_longlong(hi);
  const double half = 0.5 * (__longlong_as_double(b + 1) - hi);
  if (fabs(lo) < 0.9 * half) return hi;
  return __longlong_as_double(lo > 0. ? b + 1 : b - 1);
}
__device__ __forceinline__ bool kappa_ambiguous(double ya, double da, double yc, double dc, double kf) {
  const double aa = pow2_alt(ya, da), ac = pow2_alt(yc, dc);
  const bool dec = dc <= da * kf;
  if (ya == yc) return (ac <= aa * kf) != dec;  // one value: pow rounds both the same way
  return ((ac <= da * kf) != dec) || ((dc <= aa * kf) != dec) || ((ac <= aa * kf) != dec);
}
// The kappa rule (image_analogies.py:206) on the two norms y = cr_sqrt(blas_dot_sq(...)) of the
// approximate and the coherence match: compute_distance = norm(x)**2; true: the coherence match
// wins.  kamb: the decision would flip under libm pow (above).  (The roots are the callers': one
// merge takes both on every lane, the finish one per lane before the exchange.)
__device__ __forceinline__ bool kappa_rule(double y_app, double y_coh, double kf, bool *kamb) {
  const double d_app = y_app * y_app, d_coh = y_coh * y_coh;
  *kamb = kappa_ambiguous(y_app, d_app, y_coh, d_coh, kf);
  return d_coh <= d_app * kf;
}

// x.x in the summation order of numpy's dot (x.dot(x) inside np.linalg.norm(ord=2), i.e.
// compute_distance, algorithms.py:133-135) on the host that produced the golden vectors: OpenBLAS
// 0.3.29 ddot, SkylakeX kernel (found by matching np.dot bit-for-bit for n = 1..165,
// oracle/ia_oracle.py blas_ddot).  n1 = N & -16 elements go through fused multiply-adds: 32-wide
// blocks into four 8-lane accumulators, whose halves are added into four 4-lane accumulators
// that take any remaining 16-wide block, then ((a0 + a1) + a2) + a3 per lane and
// (l0 + l2) + (l1 + l3); the tail N - n1 elements are fused into the running sum.
// The length is a constant (std::integral_constant: everything unrolls) or a run-time int (the
// window call's D: the 32-wide, 16-wide and tail loops stay loops, no run-time unrolling).
template <class L, class X>
__device__ __forceinline__ double blas_dot_sq(L len, X &&x) {
  constexpr int U = std::is_same<L, int>::value ? 1 : 16;  // outer-loop unroll: none / all (<= 10 trips)
  const int N = len, N1 = N & ~15, N32 = N1 & ~31;
  double acc[4][4];
  if (N32 > 0) {
    double z[4][8];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int l = 0; l < 8; l++) {
        const double v = x(8 * k + l);
        z[k][l] = v * v;  // fma(v, v, 0)
      }
#pragma unroll U
    for (int i = 32; i < N32; i += 32)
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
#pragma unroll U
  for (int i = N32; i < N1; i += 16)
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const double v = x(i + 4 * k + l);
        acc[k][l] = __builtin_fma(v, v, acc[k][l]);
      }
  double dot = 0.;
  if (N1 > 0) {
    double sl[4];
#pragma unroll
    for (int l = 0; l < 4; l++) sl[l] = ((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l];
    dot = (sl[0] + sl[2]) + (sl[1] + sl[3]);
  }
#pragma unroll U
  for (int f = N1; f < N; f++) {
    const double v = x(f);
    dot = __builtin_fma(v, v, dot);
  }
  return dot;
}
template <int N, class X>
__device__ __forceinline__ double blas_dot_sq(X &&x) {
  return blas_dot_sq(std::integral_constant<int, N>{}, x);
}

template <int N, class T>
__device__ __forceinline__ double pw_sum(T &&term) {
  if constexpr (N <= 128) {
    return pw_block<N>(term, 0);
  } else {
    constexpr int N2 = N / 2 - (N / 2) % 8;
    static_assert(N - N2 <= 128, "single split");
    return pw_block<N2>(term, 0) + pw_block<N - N2>(term, N2);
  }
}
// runtime-length version (dense index path, n <= 167)
template <class T>
__device__ double pw_block_rt(T &&term, int off, int n) {
  if (n < 8) {
    double res = 0.;
    for (int i = 0; i < n; i++) res += term(off + i);
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = term(off + j);
  int nb = n - (n % 8), i = 8;
  for (; i < nb; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] += term(off + i + j);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; i++) res += term(off + i);
  return res;
}
template <class T>
__device__ double pw_sum_rt(T &&term, int n) {
  if (n <= 128) return pw_block_rt(term, 0, n);
  int n2 = n / 2;
  n2 -= n2 % 8;
  return pw_block_rt(term, 0, n2) + pw_block_rt(term, n2, n - n2);
}
// exact squared distance of a row and a query of the index (n doubles each), in numpy's order:
// every exact distance of ia_index_* (the merges, the radius verification, the coherence batch)
__device__ __forceinline__ double row_dist2_rt(const double *a, const double *q, int n) {
  return pw_sum_rt([&](int f) {
    const double x = a[f] - q[f];
    return x * x;
  }, n);
}

// ------------------------------------------------------------------------------------------
// wave helpers (64 lanes)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// lexicographic (d, idx) minimum across the wave; every lane gets the result
__device__ __forceinline__ void wave_min_di(double &d, int64_t &idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    double od = __shfl_xor(d, o, 64);
    int64_t oi = __shfl_xor(idx, o, 64);
    if (od < d || (od == d && oi < idx)) {
      d = od;
      idx = oi;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Split-f16 matcher (IA_MATCH_F16X3): K1h / K2h / K3h
//
// Every operand x (centred DB feature a', |a'|^2/256, query -2q', 256) is split into
// hi = f16(f32(x)) and lo = f16(f32(x) - hi) (22 significant bits together); K3h sums
// lo_a*hi_q + hi_a*lo_q + hi_a*hi_q with v_mfma_f32_32x32x16_f16 (f16 products are exact in
// fp32), i.e. 3 f16 MFMAs replace 8 f32 ones per 16 k.  The value carries a larger, still
// rigorous, error bound (ia_eps_c_h), so K4's certification keeps the NN exact.
// Fragment order (tile of 32 DB rows or 32 queries, k-step s of 16, part 0 = hi / 1 = lo):
//   h16x8 piece p = 2s + part, lane L:  row (L & 31), k = 16s + 8(L >> 5) + e, e = 0..7
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ void split_h(double x, _Float16 &hi, _Float16 &lo) {
  const float xf = (float)x;
  const _Float16 h = (_Float16)xf;
  hi = h;
  lo = (_Float16)(xf - (float)h);  // exact in fp32: xf and h share the leading bits
}

// ------------------------------------------------------------------------------------------
// K4's exact distances and certification bounds
// ------------------------------------------------------------------------------------------
// exact DB-row distance of row `row` (level path): ((a - q)**2).sum() in numpy order, the row
// read from the fp64 DB (K1b)
template <int CH>
__device__ __forceinline__ double exact_dist_level(const double *__restrict__ db64, int64_t row, const double *q) {
  const double *a = db64 + row * Geo<CH>::DS;
  return pw_sum<Geo<CH>::D>([&](int f) {
    const double d = a[f] - q[f];
    return d * d;
  });
}

// MFMA error bound of a row with |a'| <= Rx (ia_internal.h ia_eps_c_h / DESIGN.md §5)
__device__ __forceinline__ double merge_eps(const MergeArgs &a, double Rx, double qn) {
  return a.eps_c * (Rx * Rx + 2.0 * Rx * qn) + a.eps_a * (Rx * Rx + 14.0 * Rx + 28.0 * qn + 260.0);
}
// Certification threshold of the best exact distance bd: a chunk whose unlisted rows all have
// MFMA value >= T can hide a row that beats or ties bd only if T <= theta.  Only rows with exact
// distance <= bd matter, and such a row has |a'| <= |q'| + sqrt(bd) (|a' - q'|^2 = its distance;
// 1e-12 covers the fp64 roundings of qn and bd), so its error bound uses that radius instead of
// the DB-wide R when smaller (at 1024^2 about ten times tighter at the median query: far fewer
// near-duplicate chunks rescanned, the same certified decisions).
__device__ __forceinline__ double cert_theta(const MergeArgs &a, double R, double qn, double qn2, double bd) {
  const double Rl = fmin(R, (qn + sqrt(bd)) * (1.0 + 1e-12) + 1e-12);
  return bd - qn2 + merge_eps(a, Rl, qn) + 1e-13 * (bd + 1.0);
}

// Both distances of DB row `row` against query q from ONE set of feature loads (the row of the
// fp64 DB, K1b; q and w staged in LDS by the caller):
//   unw = ((a - q)**2).sum()  in numpy's pairwise order (NN rerank / coherence ranking)
//   wsq = sum(((a - q) * w)**2) in the OpenBLAS ddot order, blas_dot_sq (compute_distance before
//         its sqrt / square)
template <int CH>
__device__ __forceinline__ void row_dists(const double *__restrict__ db64, int row, const double *q, const double *w,
                                          double &unw, double &wsq) {
  constexpr int D = Geo<CH>::D, DS = Geo<CH>::DS;
  const double *a = db64 + (int64_t)row * DS;
  if constexpr (CH == 1) {
    double t[D + 1];
    const double2 *a2 = reinterpret_cast<const double2 *>(a);
#pragma unroll
    for (int k = 0; k < (D + 1) / 2; k++) {  // all 28 loads issued before any use
      const double2 v = a2[k];
      t[2 * k] = v.x;
      t[2 * k + 1] = v.y;
    }
#pragma unroll
    for (int f = 0; f < D; f++) t[f] -= q[f];
    unw = pw_sum<D>([&](int f) { return t[f] * t[f]; });
    wsq = blas_dot_sq<D>([&](int f) { return t[f] * w[f]; });
  } else {  // 165 doubles do not fit in registers: read the row twice
    unw = pw_sum<D>([&](int f) {
      const double d = a[f] - q[f];
      return d * d;
    });
    wsq = blas_dot_sq<D>([&](int f) { return (a[f] - q[f]) * w[f]; });
  }
}

// ---- cross-lane exchange without LDS: partner of step k of a 64-lane butterfly -----------------
// steps 0-3 stay inside a 16-lane row (DPP quad_perm xor 1, xor 2, row_half_mirror,
// row_mirror), 4 pairs rows 0-1 / 2-3 (v_permlane16_swap), 5 the two wave halves
// (v_permlane32_swap).  Every lane's partner differs from it and the pairing at each step
// joins two groups that are each already reduced, so after step 5 every lane holds the
// reduction of all 64.
template <int STEP>
__device__ __forceinline__ int lane_xchg(int v) {
  if constexpr (STEP == 0) return __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false);
  else if constexpr (STEP == 1) return __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false);
  else if constexpr (STEP == 2) return __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false);
  else if constexpr (STEP == 3) return __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false);
  else if constexpr (STEP == 4) {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    return (int)(((threadIdx.x >> 4) & 1) ? r[0] : r[1]);
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return (int)((threadIdx.x & 32) ? r[0] : r[1]);
  }
}
template <int STEP>
__device__ __forceinline__ double lane_xchg_d(double v) {
  const int lo = lane_xchg<STEP>(__double2loint(v)), hi = lane_xchg<STEP>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
template <int STEP>
__device__ __forceinline__ float lane_xchg_f(float v) {
  return __int_as_float(lane_xchg<STEP>(__float_as_int(v)));
}
// lexicographic (d, i) minimum across the wave for TWO independent keys at once
template <int STEP = 0>
__device__ __forceinline__ void wave_min2_di(double &d0, int &i0, double &d1, int &i1) {
  if constexpr (STEP < 6) {
    const double e0 = lane_xchg_d<STEP>(d0), e1 = lane_xchg_d<STEP>(d1);
    const int j0 = lane_xchg<STEP>(i0), j1 = lane_xchg<STEP>(i1);
    if (e0 < d0 || (e0 == d0 && j0 < i0)) { d0 = e0; i0 = j0; }
    if (e1 < d1 || (e1 == d1 && j1 < i1)) { d1 = e1; i1 = j1; }
    wave_min2_di<STEP + 1>(d0, i0, d1, i1);
  }
}
template <int STEP = 0>
__device__ __forceinline__ float wave_min_f_x(float v) {
  if constexpr (STEP < 6) return wave_min_f_x<STEP + 1>(fminf(v, lane_xchg_f<STEP>(v)));
  else return v;
}
// v of lane l (wave-uniform l): two v_readlane, no LDS crossbar (a __shfl is a ds_bpermute)
__device__ __forceinline__ double readlane_d(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ int lane_prefix(unsigned long long bal) {  // set bits of bal below this lane
  return __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}
template <int STEP = 0>
__device__ __forceinline__ double wave_min_d_x(double v) {
  if constexpr (STEP < 6) return wave_min_d_x<STEP + 1>(fmin(v, lane_xchg_d<STEP>(v)));
  else return v;
}
template <int STEP = 0>
__device__ __forceinline__ double wave_sum_d_x(double v) {  // fixed butterfly order: deterministic
  if constexpr (STEP < 6) return wave_sum_d_x<STEP + 1>(v + lane_xchg_d<STEP>(v));
  else return v;
}

// ------------------------------------------------------------------------------------------
// host side: the two dispatches every launcher makes
// ------------------------------------------------------------------------------------------
static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

// the level's channel count as a compile-time CH: f(c) with decltype(c)::CH (and ::KS, the
// split-f16 k-steps, with_ch_ks: 1 or 2 channels; 3 channels run the fp32 matcher)
template <int CH_, int KS_ = 0>
struct ChTag {
  static constexpr int CH = CH_, KS = KS_;
};
template <class F>
static inline void with_ch(int ch, F &&f) {
  if (ch == 1) f(ChTag<1>{});
  else if (ch == 2) f(ChTag<2>{});
  else f(ChTag<3>{});
}
template <class F>
static inline void with_ch_ks(int ch, F &&f) {
  if (ch == 1) f(ChTag<1, 4>{});
  else f(ChTag<2, 7>{});
}

// the jobs of a launch as the kernel's JS argument: a single job travels by value (JobArg1) with
// its images in the Imgs argument, a batch as the device array (JobArgN); f(js) or, for the
// kernels that read the B side, f(js, B)
static inline Imgs job0_imgs(Imgs B, const JobSet &jobs) {  // a single job's images in the Imgs argument
  B.p0 = jobs.j0.Bc;
  B.p1 = jobs.j0.B;
  B.p2 = jobs.j0.Bpc;
  B.p3 = jobs.j0.Bp;
  return B;
}
template <class F>
static inline void with_jobs(const JobSet &jobs, F &&f) {
  if (jobs.J == 1) f(JobArg1{jobs.j0});
  else f(JobArgN{jobs.rest});
}
template <class F>
static inline void with_jobs(const JobSet &jobs, const Imgs &B, F &&f) {
  if (jobs.J == 1) f(JobArg1{jobs.j0}, job0_imgs(B, jobs));
  else f(JobArgN{jobs.rest}, B);
}

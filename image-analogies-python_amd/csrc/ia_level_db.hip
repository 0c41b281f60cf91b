// ia_level_db.hip — the per-level DB builders: K0 part means, K1 fp32 MFMA tiles, K1b fp64 row
// DB, K1h split-f16 tiles (+ the f16 range check), and their launchers.
#include "ia_dev.h"
#include "ia_launch.h"

// ------------------------------------------------------------------------------------------
// K0: per-(part, channel) means of the A-side images (deterministic tree reduction)
// ------------------------------------------------------------------------------------------
// grid (IA_MEAN_CHUNKS, 4 CH): workgroup (b, part*CH + ch) sums chunk b of that image's pixels
// (fixed-order strided loop + tree), then k_part_means_fold adds the chunks in order: the same
// value on every run (a deterministic centring; any fixed mu keeps the results exact).  Pairs
// (ap.n_a A images, contiguous like the A' images) are averaged over all of them: mu stays the
// mean of what the DB holds, so the centred norms the certified bounds scale with stay small.
#define IA_MEAN_CHUNKS 128
template <int CH>
__global__ void __launch_bounds__(IA_WG) k_part_means(Imgs A, int n_ap, int n_a, double *part_sums) {
  const int pc = blockIdx.y, part = pc / CH, ch = pc % CH, b = blockIdx.x;
  const double *base = part == 0 ? A.p0 : part == 1 ? A.p1 : part == 2 ? A.p2 : A.p3;
  int64_t npx = (part & 1) ? (int64_t)A.h * A.w : (int64_t)A.hc * A.wc;
  npx *= part >= 2 ? n_ap : n_a;  // the images of a part are contiguous
  const int64_t i0 = npx * b / IA_MEAN_CHUNKS, i1 = npx * (b + 1) / IA_MEAN_CHUNKS;
  double s = 0.;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += IA_WG) s += base[i * CH + ch];
  __shared__ double red[IA_WG];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = IA_WG / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part_sums[pc * IA_MEAN_CHUNKS + b] = red[0];
}
template <int CH>
__global__ void __launch_bounds__(IA_WG) k_part_means_fold(Imgs A, int n_ap, int n_a, const double *part_sums,
                                                            double *mu_part) {
  const int pc = threadIdx.x;
  if (pc >= 4 * CH) return;
  const int part = pc / CH;
  int64_t npx = (part & 1) ? (int64_t)A.h * A.w : (int64_t)A.hc * A.wc;
  npx *= part >= 2 ? n_ap : n_a;
  double s = 0.;
  for (int b = 0; b < IA_MEAN_CHUNKS; b++) s += part_sums[pc * IA_MEAN_CHUNKS + b];
  mu_part[pc] = s / (double)npx;
}

// ------------------------------------------------------------------------------------------
// K1: DB tiles of this rank's shard (one thread per DB row)
// ------------------------------------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(IA_WG) k_db_build(LevelGeo g, Imgs A, APairs ap, const double *__restrict__ mu_part,
                                                     float4 *__restrict__ db, unsigned *__restrict__ Rbits) {
  using G = Geo<CH>;
  const int64_t pos = (int64_t)g.tile0 * IA_TILE + (int64_t)blockIdx.x * IA_WG + threadIdx.x;
  if (pos >= (int64_t)g.tile1 * IA_TILE) return;
  const int64_t ltile = pos / IA_TILE - g.tile0;
  const int j = (int)(pos % IA_TILE);
  const int64_t row = ia_pos_row_t(pos, g.n_tiles, g.pos2row);
  const bool real = row < g.NA;
  int img = 0, pr = 0, pc = 0;
  if (real) {
    const unsigned hw = (unsigned)g.ah * (unsigned)g.aw;
    img = (int)((unsigned)row / hw);
    const unsigned rem = (unsigned)row - (unsigned)img * hw;
    pr = (int)(rem / (unsigned)g.aw);
    pc = (int)(rem - (unsigned)pr * (unsigned)g.aw);
  }
  const Px P = make_px<CH>(A, pr, pc);
  const Imgs Ai = ia_pair_imgs(A, ap, img);  // pairs: row img * h * w + ... reads A_img
  double norm = 0.;
#pragma unroll
  for (int h = 0; h < 2; h++) {
#pragma unroll
    for (int p = 0; p < G::KP; p++) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int f = h * G::KH + 4 * p + e;
        if (f < G::D) {
          double a = 0.;
          if (real) {
            a = featp<CH>(Ai, P, f, img) - mu_part[feat_part<CH>(f) * CH + feat_ch<CH>(f)];
            norm += a * a;
          }
          v[e] = (float)a;
        } else if (f == G::D) {
          v[e] = real ? (float)norm : IA_PAD_NORM;
        } else {
          v[e] = 0.f;
        }
      }
      db[(ltile * G::KP + p) * IA_WAVE + h * IA_TILE + j] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  if (real) {
    // upper bound on |a'| (R of the certification bound), atomicMax on non-negative float bits
    float R = (float)(sqrt(norm) * (1.0 + 1e-6)) ;
    atomicMax(Rbits, __float_as_uint(R));
  }
}

// ------------------------------------------------------------------------------------------
// K1b: the fp64 feature DB, row-major (row = img*h*w + r*w + c, stride Geo::DS doubles, the
// tail zero), holding the exact pixel values of create_index's As rows (algorithms.py:63-67):
// [A 3x3 | A 5x5 | A'_img 3x3 | A'_img first 12], with A_img in place of A on a level of pairs.
// The merge reranks candidates from it with contiguous 16-byte loads instead of re-gathering
// four symmetric-padded images per row.
// ------------------------------------------------------------------------------------------
// One wave per 64 consecutive DB rows (= raster pixels of one A' image, so lane-adjacent rows are
// pixel-adjacent): every feature load of the wave reads 64 consecutive image values (coalesced),
// the rows are assembled in LDS (odd row stride: conflict-light) and leave as one contiguous
// 64 * DS * 8 B block of 1 KiB global_store_dwordx4 per instruction.
template <int CH>
__global__ void __launch_bounds__(IA_WAVE) k_db64_build(LevelGeo g, Imgs A, APairs ap, double *__restrict__ db64) {
  using G = Geo<CH>;
  constexpr int DS = G::DS, LS = DS + 1, H2 = DS / 2;
  __shared__ double t[IA_WAVE * LS];
  const int64_t r0 = (int64_t)blockIdx.x * IA_WAVE;
  const int lane = threadIdx.x;
  const int64_t row = r0 + lane;
  if (row < g.NA) {
    const unsigned hw = (unsigned)g.ah * (unsigned)g.aw;
    const int img = (int)((unsigned)row / hw);
    const unsigned rem = (unsigned)row - (unsigned)img * hw;
    const int pr = (int)(rem / (unsigned)g.aw), pc = (int)(rem - (unsigned)pr * (unsigned)g.aw);
    const Px P = make_px<CH>(A, pr, pc);
    const Imgs Ai = ia_pair_imgs(A, ap, img);  // (a wave that straddles two images: per lane)
    double v[G::D];
#pragma unroll
    for (int f = 0; f < G::D; f++) v[f] = featp<CH>(Ai, P, f, img);  // all loads in flight together
#pragma unroll
    for (int f = 0; f < DS; f++) t[lane * LS + f] = f < G::D ? v[f] : 0.;
  }
  __syncthreads();
  const int nrows = (int)min<int64_t>(IA_WAVE, g.NA - r0);
  double2 *dst = reinterpret_cast<double2 *>(db64 + r0 * DS);
  for (int i = lane; i < nrows * H2; i += IA_WAVE) {
    const int rr = i / H2, cc = 2 * (i - rr * H2);
    dst[i] = make_double2(t[rr * LS + cc], t[rr * LS + cc + 1]);
  }
}

// max |x| over the level's images (decides whether every operand fits f16, IA_F16_MAXABS)
struct AbsArrays {
  const double *p[8];
  int64_t n[8];
};
__global__ void __launch_bounds__(IA_WG) k_absmax(AbsArrays arr, unsigned *__restrict__ out) {
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const double *p = arr.p[k];
    const int64_t n = arr.n[k];
    for (int64_t i = (int64_t)blockIdx.x * IA_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IA_WG)
      m = fmaxf(m, (float)fabs(p[i]));  // NaN propagates as "not finite" below
  }
  if (!(m <= 3.0e38f)) m = 3.4e38f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}

// One wave per DB tile (32 rows x 64 columns in v_mfma_f32_32x32x16_f16 operand order): lane L
// (row j = L & 31, column half h = L >> 5) holds columns 16s + 8h .. + 7 of every k-step s, i.e.
// 64 contiguous bytes of its row in the fp64 row DB (K1b, written just before: rows are whole
// 128 B lines, no image gathers).  Centre by mu, |a'|^2 = the two lane halves' partial sums (the
// certified bound does not depend on its rounding order), split into f16 hi + lo, and store
// each piece as one 1 KiB coalesced wave store.  Grid-stride over tiles: one atomicMax of R per
// workgroup.
template <int CH, int KS>
__global__ void __launch_bounds__(IA_WG) k_db_build_h(LevelGeo g, const double *__restrict__ db64,
                                                       const double *__restrict__ mu_part, h16x8 *__restrict__ db,
                                                       unsigned *__restrict__ Rbits) {
  constexpr int D = 55 * CH, DS = Geo<CH>::DS;
  static_assert(16 * KS >= D + 1, "k-steps must hold D features + the norm column");
  static_assert(DS % 8 == 0, "64-byte row pieces");
  __shared__ float wR[IA_WG / IA_WAVE];
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
  const int64_t nloc = (int64_t)g.tile1 - g.tile0;
  double mu[KS][8];  // this lane's feature means (the lane's columns are fixed)
#pragma unroll
  for (int s = 0; s < KS; s++)
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int f = 16 * s + 8 * h + e;
      mu[s][e] = f < D ? mu_part[feat_part<CH>(f) * CH + feat_ch<CH>(f)] : 0.;
    }
  float Rmax = 0.f;
  for (int64_t lt = (int64_t)blockIdx.x * (IA_WG / IA_WAVE) + wave; lt < nloc; lt += (int64_t)gridDim.x * (IA_WG / IA_WAVE)) {
    const int64_t pos = (g.tile0 + lt) * IA_TILE + j;
    const int64_t row = ia_pos_row_t(pos, g.n_tiles, g.pos2row);
    const bool real = row < g.NA;
    double a[KS][8];
#pragma unroll
    for (int s = 0; s < KS; s++) {
      const int f0 = 16 * s + 8 * h;
      double2 v[4];
      if (real && f0 < DS) {
        const double2 *src = reinterpret_cast<const double2 *>(db64 + row * DS + f0);
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = src[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = make_double2(0., 0.);
      }
#pragma unroll
      for (int e = 0; e < 4; e++) {
        a[s][2 * e] = v[e].x;
        a[s][2 * e + 1] = v[e].y;
      }
    }
    double nrm = 0.;
#pragma unroll
    for (int s = 0; s < KS; s++)
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int f = 16 * s + 8 * h + e;
        a[s][e] = f < D ? a[s][e] - mu[s][e] : 0.;
        nrm += a[s][e] * a[s][e];
      }
    nrm += __shfl_xor(nrm, 32, 64);  // both halves: p0 + p1 (addition commutes exactly)
    const int64_t tb = lt * TileFmt<KS>::STRIDE;
#pragma unroll
    for (int s = 0; s < KS; s++) {
      h16x8 vh, vl;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        double x = a[s][e];
        if (16 * s + 8 * h + e == D) x = real ? nrm * (1.0 / IA_NORM_SCALE) : 60000.0;  // padding rows: never a candidate
        _Float16 hi, lo;
        split_h(x, hi, lo);
        vh[e] = hi;
        vl[e] = lo;
      }
      if (!(TileFmt<KS>::CMP && s == KS - 1 && h == 1)) {  // (compact: padding half not stored)
        db[tb + TileFmt<KS>::off(2 * s, lane)] = vh;
        db[tb + TileFmt<KS>::off(2 * s + 1, lane)] = vl;
      }
    }
    if (real) Rmax = fmaxf(Rmax, (float)(sqrt(nrm) * (1.0 + 1e-6)));
  }
  // R = max |a'| (certification bound): wave, then workgroup max, one atomic per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) Rmax = fmaxf(Rmax, __shfl_xor(Rmax, o, 64));
  if (lane == 0) wR[wave] = Rmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = wR[0];
#pragma unroll
    for (int w = 1; w < IA_WG / IA_WAVE; w++) m = fmaxf(m, wR[w]);
    if (m > 0.f) atomicMax(Rbits, __float_as_uint(m));
  }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_level_plan.cpp)
// ------------------------------------------------------------------------------------------
void ia_launch_means(int ch, const Imgs &A, const APairs &ap, int n_ap, double *mu, hipStream_t st) {
  // partial sums live behind the 4 CH means in the same buffer (ia_level_plan.cpp sizes it)
  double *parts = mu + 16;
  with_ch(ch, [&](auto c) {
    constexpr int CH = decltype(c)::CH;
    hipLaunchKernelGGL(k_part_means<CH>, dim3(IA_MEAN_CHUNKS, 4 * CH), dim3(IA_WG), 0, st, A, n_ap, ap.n_a, parts);
    hipLaunchKernelGGL(k_part_means_fold<CH>, dim3(1), dim3(IA_WG), 0, st, A, n_ap, ap.n_a, (const double *)parts, mu);
  });
}

void ia_launch_db_build(const LevelGeo &g, const Imgs &A, const APairs &ap, const double *mu, float4 *db, unsigned *Rbits,
                        hipStream_t st) {
  const int64_t rows = (int64_t)(g.tile1 - g.tile0) * IA_TILE;
  with_ch(g.ch, [&](auto c) {
    hipLaunchKernelGGL(k_db_build<decltype(c)::CH>, dim3(cdiv(rows, IA_WG)), dim3(IA_WG), 0, st, g, A, ap, mu, db, Rbits);
  });
}

void ia_launch_db64_build(const LevelGeo &g, const Imgs &A, const APairs &ap, double *db64, hipStream_t st) {
  with_ch(g.ch, [&](auto c) {
    hipLaunchKernelGGL(k_db64_build<decltype(c)::CH>, dim3(cdiv(g.NA, IA_WAVE)), dim3(IA_WAVE), 0, st, g, A, ap, db64);
  });
}
int ia_db64_stride(int ch) { return ch == 1 ? Geo<1>::DS : ch == 2 ? Geo<2>::DS : Geo<3>::DS; }

// ---- split-f16 matcher -----------------------------------------------------------------------
double ia_k3h_tile_bytes(int KS) { return KS == 4 ? 16.0 * TileFmt<4>::STRIDE : KS == 7 ? 16.0 * TileFmt<7>::STRIDE : 0.; }
int ia_ks_for(int ch) { return ch == 1 ? 4 : ch == 2 ? 7 : 0; }  // 3 channels: fp32 matcher

void ia_launch_absmax(const double *const *p, const int64_t *n, unsigned *out, hipStream_t st) {
  AbsArrays arr;
  for (int k = 0; k < 8; k++) {
    arr.p[k] = p[k];
    arr.n[k] = p[k] ? n[k] : 0;
  }
  hipLaunchKernelGGL(k_absmax, dim3(512), dim3(IA_WG), 0, st, arr, out);
}

void ia_launch_db_build_h(const LevelGeo &g, const Imgs &A, const double *db64, const double *mu, void *db, unsigned *Rbits,
                          hipStream_t st) {
  (void)A;  // the rows come from the fp64 row DB
  const int64_t tiles = (int64_t)g.tile1 - g.tile0;  // one wave per tile, <= 4 tiles per wave
  const int64_t nwg = std::max<int64_t>(1, std::min<int64_t>(cdiv(tiles, IA_WG / IA_WAVE), 2048));
  with_ch_ks(g.ch, [&](auto c) {
    hipLaunchKernelGGL((k_db_build_h<decltype(c)::CH, decltype(c)::KS>), dim3((unsigned)nwg), dim3(IA_WG), 0, st, g, db64, mu,
                       (h16x8 *)db, Rbits);
  });
}

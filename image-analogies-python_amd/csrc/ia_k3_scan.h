// ia_k3_scan.h — the fp32 MFMA distance scan's one body: the query staging and the tile loop of
// K3 (ia_k3.hip k3_dist: top-2 epilogue) and of the index's radius scans (ia_k3r.hip k3r_count,
// k3r_fill: threshold epilogues).  The only place that issues v_mfma_f32_32x32x2_f32: every
// consumer gets the same chain on the same operands, hence the same values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ia_internal.h"
#include "ia_top2.h"  // f32x16

// ------------------------------------------------------------------------------------------
// grid.x = nwg workgroups of 4 waves; WG w owns DB tiles [w*tpw, (w+1)*tpw) of the shard,
// wave v takes tiles w*tpw + v, +4, ... .  QT query tiles (32 queries each) are staged in
// LDS once; each DB tile is loaded once into registers (KH floats per lane) and contracted
// against every query tile:  C[row][query] = sum_k DB[row][k] * Qf[k][query]
//   A operand = DB row (lane & 31), B operand = query (lane & 31), k-half = lane >> 5;
//   C layout: lane holds query (lane & 31), rows (r&3) + 8(r>>2) + 4(lane>>5), r = 0..15.
// ------------------------------------------------------------------------------------------

// stage the launch's QT query tiles in LDS (every thread; ends with a barrier)
template <int KH, int QT>
__device__ __forceinline__ void k3_stage(const float4 *__restrict__ qf, int qt0, float4 *lds) {
  constexpr int KP = KH / 4;
  const float4 *qsrc = qf + (int64_t)qt0 * KP * IA_WAVE;
  for (int i = threadIdx.x; i < QT * KP * IA_WAVE; i += IA_WG) lds[i] = qsrc[i];
  __syncthreads();
}

// the tile loop: epi(acc, q, pbase) once per finished accumulator, q the query tile of the launch,
// pbase = t * IA_TILE + 4 * half the shard position of acc[0] (acc[r]: pbase + (r&3) + 8(r>>2))
template <int KH, int QT, class Epi>
__device__ __forceinline__ void k3_scan(const float4 *__restrict__ db, const float4 *lds, int n_tiles, int tpw, Epi &&epi) {
  constexpr int KP = KH / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  const int wg = blockIdx.x;
  const int t_begin = wg * tpw, t_end = min(n_tiles, t_begin + tpw);
  int t = t_begin + wave;
  float a[KH], an[KH];
  {
    const int tl = min(t, n_tiles - 1);
    const float4 *src = db + (int64_t)tl * KP * IA_WAVE + lane;
#pragma unroll
    for (int p = 0; p < KP; p++) {
      float4 v = src[p * IA_WAVE];
      a[4 * p] = v.x; a[4 * p + 1] = v.y; a[4 * p + 2] = v.z; a[4 * p + 3] = v.w;
    }
  }
  for (; t < t_end; t += 4) {
    {  // prefetch the next tile of this wave (clamped: always issue, never branch per load)
      const int tl = min(t + 4, n_tiles - 1);
      const float4 *src = db + (int64_t)tl * KP * IA_WAVE + lane;
#pragma unroll
      for (int p = 0; p < KP; p++) {
        float4 v = src[p * IA_WAVE];
        an[4 * p] = v.x; an[4 * p + 1] = v.y; an[4 * p + 2] = v.z; an[4 * p + 3] = v.w;
      }
    }
    const int pbase = t * IA_TILE + 4 * half;
    asm volatile("" ::: "memory");  // LDS query fragments are re-read per tile, not hoisted
    // Query tiles go in pairs (two independent accumulation chains share each DB operand);
    // the epilogue of pair j is issued after the MFMAs of pair j+1 so the scheduler can
    // fill the MFMA gaps with it (distinct accumulators, no dependency).
    f32x16 e0, e1;
    auto epilogue = [&](const f32x16 &acc, int q) { epi(acc, q, pbase); };
#pragma unroll
    for (int qp = 0; qp < QT; qp += 2) {
      constexpr f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const bool two = qp + 1 < QT;
      f32x16 c0 = zero, c1 = zero;
      const float4 *qb0 = lds + qp * KP * IA_WAVE + lane;
      const float4 *qb1 = qb0 + KP * IA_WAVE;
#pragma unroll
      for (int p = 0; p < KP; p++) {
        const float4 x0 = qb0[p * IA_WAVE];
        const float4 x1 = two ? qb1[p * IA_WAVE] : x0;
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * p], x0.x, c0, 0, 0, 0);
        if (two) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * p], x1.x, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * p + 1], x0.y, c0, 0, 0, 0);
        if (two) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * p + 1], x1.y, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * p + 2], x0.z, c0, 0, 0, 0);
        if (two) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * p + 2], x1.z, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * p + 3], x0.w, c0, 0, 0, 0);
        if (two) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * p + 3], x1.w, c1, 0, 0, 0);
      }
      if (qp >= 2) {
        epilogue(e0, qp - 2);
        epilogue(e1, qp - 1);
      }
      e0 = c0;
      e1 = c1;
    }
    {
      constexpr int ql = ((QT - 1) / 2) * 2;  // first tile of the last pair
      epilogue(e0, ql);
      if (ql + 1 < QT) epilogue(e1, ql + 1);
    }
#pragma unroll
    for (int k = 0; k < KH; k++) a[k] = an[k];
  }
}

// ia_k3.hip — K3, the fp32 MFMA distance scan, its launcher, and the whole-LDS allowance every
// scan launcher uses.
#include <mutex>
#include <unordered_set>

#include "ia_launch.h"
#include "ia_top2.h"

// ------------------------------------------------------------------------------------------
// K3: MFMA distance scan with fused top-2 / threshold (the hot kernel)
//
// grid.x = nwg workgroups of 4 waves; WG w owns DB tiles [w*tpw, (w+1)*tpw) of the shard,
// wave v takes tiles w*tpw + v, +4, ... .  QT query tiles (32 queries each) are staged in
// LDS once; each DB tile is loaded once into registers (KH floats per lane) and contracted
// against every query tile:  C[row][query] = sum_k DB[row][k] * Qf[k][query]
//   A operand = DB row (lane & 31), B operand = query (lane & 31), k-half = lane >> 5;
//   C layout: lane holds query (lane & 31), rows (r&3) + 8(r>>2) + 4(lane>>5), r = 0..15.
// Each lane keeps, per query tile, the best (value, row) and the second-smallest value of
// the rows it has seen ("subset" = lane half x wave); the workgroup merges its 8 subsets into
// a top-2 list + threshold T (every unlisted row of the chunk has approx value >= T).
// ------------------------------------------------------------------------------------------
template <int KH, int QT>
__global__ void __launch_bounds__(IA_WG, 2)
k3_dist(const float4 *__restrict__ db, const float4 *__restrict__ qf, int n_tiles, int tpw, int qt0, int M,
        int nwg, int row0, int NT, float4 *__restrict__ rec, float *__restrict__ recT) {
  constexpr int KP = KH / 4;
  extern __shared__ float4 lds[];  // QT * KP * 64 float4 (queries), reused for the merge
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  const int wg = blockIdx.x;

  const float4 *qsrc = qf + (int64_t)qt0 * KP * IA_WAVE;
  for (int i = threadIdx.x; i < QT * KP * IA_WAVE; i += IA_WG) lds[i] = qsrc[i];
  __syncthreads();

  float b1[QT], b2[QT];
  int i1[QT];
#pragma unroll
  for (int q = 0; q < QT; q++) {
    b1[q] = FLT_MAX;
    b2[q] = FLT_MAX;
    i1[q] = 0x7fffffff;
  }

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
    const int rbase = row0 + t * IA_TILE + 4 * half;
    asm volatile("" ::: "memory");  // LDS query fragments are re-read per tile, not hoisted
    // Query tiles go in pairs (two independent accumulation chains share each DB operand);
    // the top-2 epilogue of pair j is issued after the MFMAs of pair j+1 so the scheduler can
    // fill the MFMA gaps with it (distinct accumulators, no dependency).
    // Epilogue per value v (4 VALU): c = v < b1;  b2 = med3(b1, b2, v) (b1 <= b2 => the
    // second smallest of the three);  b1 = c ? v : b1;  i1 = c ? row : i1.
    f32x16 e0, e1;
    auto epilogue = [&](const f32x16 &acc, int q) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float v = acc[r];
        const int row = rbase + (r & 3) + 8 * (r >> 2);
        const bool c = v < b1[q];
        b2[q] = __builtin_amdgcn_fmed3f(b1[q], b2[q], v);
        b1[q] = c ? v : b1[q];
        i1[q] = c ? row : i1[q];
      }
    };
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

  // ---- merge the 8 subsets of each query: lane halves by shuffle, waves through LDS
  __syncthreads();  // queries no longer needed: reuse LDS
  Top2 *red = reinterpret_cast<Top2 *>(lds);  // [4 waves][QT][32]
#pragma unroll
  for (int q = 0; q < QT; q++) {
    Top2 mine = {b1[q], FLT_MAX, b2[q], i1[q], 0x7fffffff};
    Top2 other;
    other.v1 = __shfl_xor(b1[q], 32, 64);
    other.i1 = __shfl_xor(i1[q], 32, 64);
    other.T = __shfl_xor(b2[q], 32, 64);
    other.v2 = FLT_MAX;
    other.i2 = 0x7fffffff;
    Top2 mrg = half == 0 ? top2_merge(mine, other) : top2_merge(other, mine);
    if (half == 0) red[(wave * QT + q) * IA_TILE + lane] = mrg;
  }
  __syncthreads();
  for (int x = threadIdx.x; x < QT * IA_TILE; x += IA_WG) {
    Top2 m = red[x];
#pragma unroll
    for (int w = 1; w < 4; w++) m = top2_merge(m, red[(w * QT) * IA_TILE + x]);
    const int qg = qt0 * IA_TILE + x;
    if (qg < M) {  // positions -> DB rows (ia_pos_row); never-set entries stay out of range
      const int r1 = m.i1 == 0x7fffffff ? m.i1 : (int)ia_pos_row(m.i1, NT);
      const int r2 = m.i2 == 0x7fffffff ? m.i2 : (int)ia_pos_row(m.i2, NT);
      rec[(int64_t)qg * nwg + wg] = make_float4(m.v1, __int_as_float(r1), m.v2, __int_as_float(r2));
      recT[(int64_t)qg * nwg + wg] = m.T;
    }
  }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_level_run.cpp, ia_index.cpp)
// ------------------------------------------------------------------------------------------
// K3 dispatch table: QT query tiles per launch (1..QTMAX(KH))
typedef void (*k3_fn)(const float4 *, const float4 *, int, int, int, int, int, int, int, float4 *, float *);
template <int KH, int... QTs>
struct K3Table {
  static k3_fn get(int qt) {
    static const k3_fn tab[] = {k3_dist<KH, QTs>...};
    return tab[qt - 1];
  }
};
int ia_k3_qtmax(int KH) { return KH == 28 ? 11 : KH == 56 ? 5 : 3; }
int ia_k3h_qtmax(int KS) { return KS == 4 ? 11 : 8; }  // the split-f16 scan's (ia_k3h.hip)

// Allow a kernel the architecture's whole LDS as dynamic shared memory (gfx950: 160 KiB per CU;
// the default cap is 64 KiB), once per kernel.  Several host threads launch through one libia
// (one context each: DeviceSweep, bench --streams), so the set is guarded; the attribute is the
// arch maximum rather than the launch's size, so no thread can lower it under another's launch.
void ia_allow_full_lds(const void *fn) {
  static std::mutex mu;
  static std::unordered_set<const void *> done;
  std::lock_guard<std::mutex> lk(mu);
  if (!done.insert(fn).second) return;
  hipFuncAttributes fa;  // dynamic + static shared memory must fit the CU's 160 KiB
  const int stat = hipFuncGetAttributes(&fa, fn) == hipSuccess ? (int)fa.sharedSizeBytes : 1024;
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - stat);
}

void ia_launch_k3(int KH, int qt, const float4 *db, const float4 *qf, int n_tiles, int tpw, int qt0, int M, int nwg,
                  int row0, int NT, float4 *rec, float *recT, hipStream_t st) {
  k3_fn fn;
  if (KH == 28) fn = K3Table<28, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11>::get(qt);
  else if (KH == 56) fn = K3Table<56, 1, 2, 3, 4, 5>::get(qt);
  else fn = K3Table<84, 1, 2, 3>::get(qt);
  const size_t lds = (size_t)qt * (KH / 4) * IA_WAVE * sizeof(float4);
  ia_allow_full_lds((const void *)fn);
  hipLaunchKernelGGL(fn, dim3(nwg), dim3(IA_WG), lds, st, db, qf, n_tiles, tpw, qt0, M, nwg, row0, NT, rec, recT);
}

// ia_k3.hip — K3, the fp32 MFMA distance scan with its top-2 epilogue (the scan body is
// ia_k3_scan.h's, shared with ia_k3r.hip), its launcher, and the whole-LDS allowance every scan
// launcher uses.
#include <mutex>
#include <unordered_set>

#include "ia_k3_scan.h"
#include "ia_launch.h"
#include "ia_top2.h"

// ------------------------------------------------------------------------------------------
// K3: MFMA distance scan with fused top-2 / threshold (the hot kernel)
//
// The scan itself (geometry, staging, tile loop, MFMA chain) is ia_k3_scan.h's, shared with the
// radius scans; here its epilogue and what follows the loop.
// Each lane keeps, per query tile, the best (value, row) and the second-smallest value of
// the rows it has seen ("subset" = lane half x wave); the workgroup merges its 8 subsets into
// a top-2 list + threshold T (every unlisted row of the chunk has approx value >= T).
// ------------------------------------------------------------------------------------------
template <int KH, int QT>
__global__ void __launch_bounds__(IA_WG, 2)
k3_dist(const float4 *__restrict__ db, const float4 *__restrict__ qf, int n_tiles, int tpw, int qt0, int M,
        int nwg, int row0, int NT, float4 *__restrict__ rec, float *__restrict__ recT) {
  extern __shared__ float4 lds[];  // QT * KP * 64 float4 (queries), reused for the merge
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  const int wg = blockIdx.x;
  k3_stage<KH, QT>(qf, qt0, lds);

  float b1[QT], b2[QT];
  int i1[QT];
#pragma unroll
  for (int q = 0; q < QT; q++) {
    b1[q] = FLT_MAX;
    b2[q] = FLT_MAX;
    i1[q] = 0x7fffffff;
  }
  // Epilogue per value v (4 VALU): c = v < b1;  b2 = med3(b1, b2, v) (b1 <= b2 => the
  // second smallest of the three);  b1 = c ? v : b1;  i1 = c ? row : i1.
  k3_scan<KH, QT>(db, lds, n_tiles, tpw, [&](const f32x16 &acc, int q, int pbase) {
    const int rbase = row0 + pbase;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float v = acc[r];
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      const bool c = v < b1[q];
      b2[q] = __builtin_amdgcn_fmed3f(b1[q], b2[q], v);
      b1[q] = c ? v : b1[q];
      i1[q] = c ? row : i1[q];
    }
  });

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

// ia_mask.hip — masked resynthesis of a level (include/ia.h ia_synthesize_levels_masked, DESIGN.md
// §13): the kernels that know the mask.
//
//   k_mask_check     pre-pass: every kept source (s_in, im_in) of a job names a DB row or none
//   k_mask_steps     the level's step lists for all jobs, one wave per step of the schedule
//                    t = col + (p_l + 1) row: a count pass, then (after k_mask_scan) the fill pass
//   k_mask_scan      the exclusive scan of the counts, in place: offsets[0..T]
//
// A step's list drives the window call's own step (ia_level_nbhd.cpp run_nbhd_step): ia_nbhd.hip's
// gather and finish kernels in their list form (ia_nbhd.h ListSource).
#include "ia_dev.h"
#include "ia_launch.h"

__global__ void __launch_bounds__(IA_WG) k_mask_check(const int32_t *__restrict__ s, const int32_t *__restrict__ im,
                                                      int64_t NB, int n_ap, int ah, int aw, unsigned *__restrict__ err) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * IA_WG + threadIdx.x; i < NB; i += (int64_t)gridDim.x * IA_WG) {
    const int m = im[i];
    if (m < 0) continue;  // no source: its s is not read
    bad |= m >= n_ap || (unsigned)s[2 * i] >= (unsigned)ah || (unsigned)s[2 * i + 1] >= (unsigned)aw;
  }
  if (bad) *err = 1u;  // every writer stores the same word
}

// Step t (one wave) holds the pixels (r, t - skew r), r_lo <= r <= r_hi (ia_wavefront_step_pad's
// rows).  Lanes take 64 of those rows of one job at a time, one pixel per row; a ballot of the masked
// ones and the set bits below a lane place them, so the step's entries stand in (job, row) ascending
// order whatever the hardware does: no atomic decides an order.  FILL = false: offsets[t] = the
// step's count.  FILL = true: offsets[t] = where its entries start (k_mask_scan), list[...] = them.
template <bool FILL>
__global__ void __launch_bounds__(IA_WG) k_mask_steps(const uint8_t *__restrict__ mask, int64_t NB, int J, int bh, int bw,
                                                      int skew, int T, int32_t *__restrict__ offsets, int2 *__restrict__ list) {
  const int lane = threadIdx.x & 63;
  const int t = __builtin_amdgcn_readfirstlane(blockIdx.x * (IA_WG / IA_WAVE) + (threadIdx.x >> 6));  // wave-uniform
  if (t >= T) return;
  const int over = t - bw + 1;  // rows r with t - skew r >= bw lie before the step
  const int r_lo = over <= 0 ? 0 : (over + skew - 1) / skew, r_hi = min(bh - 1, t / skew);
  int n = FILL ? offsets[t] : 0;
  for (int j = 0; j < J; j++)
    for (int r0 = r_lo; r0 <= r_hi; r0 += IA_WAVE) {
      const int r = min(r0 + lane, r_hi);      // (lanes past the step's rows re-read its last pixel)
      const int qi = r * bw + (t - skew * r);  // inside the level for r_lo <= r <= r_hi
      const bool on = r0 + lane <= r_hi && mask[(int64_t)j * NB + qi] != 0;
      const unsigned long long bal = __ballot(on);
      if constexpr (FILL)
        if (on) list[n + lane_prefix(bal)] = make_int2(j, qi);
      n += __popcll(bal);
    }
  if (!FILL && lane == 0) offsets[t] = n;
}

// offsets[0..T): counts in, exclusive sums out; offsets[T] = the total.  One workgroup: thread i sums
// its contiguous share, thread 0 scans the 256 sums, thread i writes its share's running sums.
__global__ void __launch_bounds__(IA_WG) k_mask_scan(int32_t *__restrict__ offsets, int T) {
  __shared__ int part[IA_WG];
  const int i = threadIdx.x, per = (T + IA_WG - 1) / IA_WG;
  const int a = min(T, i * per), b = min(T, a + per);
  int s = 0;
  for (int t = a; t < b; t++) s += offsets[t];
  part[i] = s;
  __syncthreads();
  if (i == 0) {
    int run = 0;
    for (int k = 0; k < IA_WG; k++) {
      const int v = part[k];
      part[k] = run;
      run += v;
    }
    offsets[T] = run;
  }
  __syncthreads();
  int run = part[i];
  for (int t = a; t < b; t++) {
    const int v = offsets[t];
    offsets[t] = run;
    run += v;
  }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called from ia_level_mask.cpp)
// ------------------------------------------------------------------------------------------
void ia_launch_mask_check(const int32_t *s, const int32_t *im, int64_t NB, int n_ap, int ah, int aw, unsigned *err,
                          hipStream_t st) {
  const unsigned nwg = (unsigned)std::min<int64_t>(1024, (NB + IA_WG - 1) / IA_WG);
  hipLaunchKernelGGL(k_mask_check, dim3(nwg), dim3(IA_WG), 0, st, s, im, NB, n_ap, ah, aw, err);
}

void ia_launch_mask_count(const uint8_t *mask, int64_t NB, int J, int bh, int bw, int pad, int T, int32_t *offsets,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_mask_steps<false>, dim3(cdiv(T, IA_WG / IA_WAVE)), dim3(IA_WG), 0, st, mask, NB, J, bh, bw, pad + 1, T,
                     offsets, (int2 *)nullptr);
  hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(IA_WG), 0, st, offsets, T);
}

void ia_launch_mask_fill(const uint8_t *mask, int64_t NB, int J, int bh, int bw, int pad, int T, int32_t *offsets, int2 *list,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_mask_steps<true>, dim3(cdiv(T, IA_WG / IA_WAVE)), dim3(IA_WG), 0, st, mask, NB, J, bh, bw, pad + 1, T,
                     offsets, list);
}

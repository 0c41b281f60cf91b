// ia_k3p_launch.hip — host half of the split-f16 scans of ia_k3h.hip: instance tables, kernel
// selection and launch.  The scans' LDS formats are ia_k3p_lds.h's; no size is restated here.
#include <hip/hip_runtime.h>

#include "ia_internal.h"
#include "ia_k3p_lds.h"
#include "ia_launch.h"
#include "ia_top2.h"

// the kernels are compiled once per (KS, QT) instance (ia_k3h.hip, Makefile K3H_INST)
#define IA_K3H_DECL(ks, qt) k3h_fn ia_k3h_get_##ks##_##qt();
IA_K3H_DECL(4, 1) IA_K3H_DECL(4, 2) IA_K3H_DECL(4, 3) IA_K3H_DECL(4, 4) IA_K3H_DECL(4, 5) IA_K3H_DECL(4, 6)
IA_K3H_DECL(4, 7) IA_K3H_DECL(4, 8) IA_K3H_DECL(4, 9) IA_K3H_DECL(4, 10) IA_K3H_DECL(4, 11)
IA_K3H_DECL(7, 1) IA_K3H_DECL(7, 2) IA_K3H_DECL(7, 3) IA_K3H_DECL(7, 4) IA_K3H_DECL(7, 5) IA_K3H_DECL(7, 6)
IA_K3H_DECL(7, 7) IA_K3H_DECL(7, 8)
static k3h_fn k3h_get(int KS, int qt) {
  typedef k3h_fn (*getter)();
  static const getter g4[] = {ia_k3h_get_4_1, ia_k3h_get_4_2, ia_k3h_get_4_3, ia_k3h_get_4_4,  ia_k3h_get_4_5, ia_k3h_get_4_6,
                              ia_k3h_get_4_7, ia_k3h_get_4_8, ia_k3h_get_4_9, ia_k3h_get_4_10, ia_k3h_get_4_11};
  static const getter g7[] = {ia_k3h_get_7_1, ia_k3h_get_7_2, ia_k3h_get_7_3, ia_k3h_get_7_4,
                              ia_k3h_get_7_5, ia_k3h_get_7_6, ia_k3h_get_7_7, ia_k3h_get_7_8};
  return KS == 4 ? g4[qt - 1]() : g7[qt - 1]();
}
void ia_launch_k3h(int KS, int qt, const void *db, const void *qf, int n_tiles, int tpw, int qt0, int M, int nwg, int row0,
                   int NT, float4 *rec, float *recT, hipStream_t st) {
  const k3h_fn fn = k3h_get(KS, qt);
  ia_allow_full_lds((const void *)fn);
  hipLaunchKernelGGL(fn, dim3(nwg), dim3(IA_WGH), k3h_lds_bytes(KS, qt), st, (const h16x8 *)db, (const h16x8 *)qf, n_tiles, tpw,
                     qt0, M, nwg, row0, NT, rec, recT);
}

// pruned split-f16 distance kernels (ia_k3h.hip k3h_prune3, 1 channel)
#define IA_K3P_DECL(qt) k3p_fn ia_k3p_get_4_##qt(int);
IA_K3P_DECL(1) IA_K3P_DECL(2) IA_K3P_DECL(3) IA_K3P_DECL(4) IA_K3P_DECL(5) IA_K3P_DECL(6) IA_K3P_DECL(7) IA_K3P_DECL(8)
IA_K3P_DECL(9) IA_K3P_DECL(10) IA_K3P_DECL(11)
// The one place that decides which pruned-scan kernel a launch runs: from option "k3p_variant",
// whether the queries arrive presorted and whether this is an owner-computes scan; then by what
// fits.  fn = nullptr: the library holds no instance (ia_set_option accepts only built variants).
struct K3pKernel {
  k3p_fn fn;
  size_t lds;  // dynamic LDS bytes
};
static K3pKernel k3p_kernel(int option, bool presorted, bool owner_scan, int qt, int Mpad, int kmax) {
  typedef k3p_fn (*getter)(int);
  static const getter g4[] = {ia_k3p_get_4_1, ia_k3p_get_4_2, ia_k3p_get_4_3, ia_k3p_get_4_4,  ia_k3p_get_4_5, ia_k3p_get_4_6,
                              ia_k3p_get_4_7, ia_k3p_get_4_8, ia_k3p_get_4_9, ia_k3p_get_4_10, ia_k3p_get_4_11};
  // the option's in-kernel-sort form (20 / 22 / 24) or its presorted form: 21, or the two-pass
  // 25 under 24 / 25 (round 6, on the trimmed stream: cfg4 6.66 -> 6.91 M px/s against 21's whole
  // tiles) - owner-computes scans take 25 only where it was asked for by name
  int variant;
  if (presorted) variant = option == 25 || (option == 24 && !owner_scan) ? 25 : 21;
  else variant = option == 21 ? 20 : option == 25 ? 24 : option;
  // the in-kernel sort holds <= IA_K3P3_MAXQ queries (the callers sort wider steps first, K2s);
  // every variant walks any number of tiles (the host keeps kmax <= IA_K3P_MAXK_LDS)
  if (!presorted && Mpad > IA_K3P3_MAXQ) variant = 21;
  if (k3p_variant_form(variant) == K3pStream::TwoPass) {
    hipFuncAttributes fa;
    const k3p_fn f24 = g4[qt - 1](variant);
    const size_t stat = f24 && hipFuncGetAttributes(&fa, (const void *)f24) == hipSuccess ? fa.sharedSizeBytes : 0;
    // (many tiles per workgroup or wide steps): the one-pass forms
    if (!f24 || !k3p_two_pass_fits(qt, k3p_variant_pre(variant), Mpad, kmax, stat)) variant = variant == 25 ? 21 : 22;
  }
  return {g4[qt - 1](variant), k3p_dyn_bytes(qt, k3p_variant_pre(variant), k3p_variant_form(variant), Mpad, kmax)};
}
int ia_launch_k3p(const K3pLaunch &a, int option, bool presorted, hipStream_t st) {
  const bool owner_scan = a.xo && a.xo->on;
  const K3pKernel k = k3p_kernel(option, presorted, owner_scan, a.qt, a.Mpad, (a.NT + a.nwg - 1) / a.nwg);
  // (a missing instance is an error the level reports, never a silently skipped scan whose stale
  // records the merge would consume)
  if (!k.fn) return -1;  // IA_EINVAL (include/ia.h)
  // nqb > 1 (presorted kernels and owner-computes scans only): one launch of nqb query blocks x
  // nwg DB chunks
  const int nqb = presorted || owner_scan ? a.nqb : 1;
  const int qt_end = nqb == 1 ? a.qt0 + a.qt : a.qt_end;
  XOScan x{};  // off unless an owner-computes step passes its exchange
  if (a.xo) x = *a.xo;
  x.stamp = a.stamp;
  x.rec_wt = a.rec_wt;
  ia_allow_full_lds((const void *)k.fn);
  // (alternate steps walk in reverse)
  hipLaunchKernelGGL(k.fn, dim3(nqb * a.nwg), dim3(IA_WGH), k.lds, st, (const h16x8 *)a.db, (const h16x8 *)a.qf, a.qinfo, a.boxes,
                     a.pos2row, a.NT, a.qt0, a.M, a.Mpad, a.nwg, a.rec, a.recT, a.pairs, a.tiles, a.step & 1, a.order, a.r0,
                     a.tbox, a.tnorm, nqb, qt_end, x);
  return 0;
}

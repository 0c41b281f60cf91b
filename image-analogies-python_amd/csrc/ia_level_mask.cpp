// ia_level_mask.cpp — masked resynthesis of a level (ia_synthesize_levels_masked): the
// call, its own checks, the mask pre-pass and step lists (ia_mask.hip), the kept-state copies, the loop
// over the steps that hold a masked pixel, and the host statement of the compaction rule
// (ia_masked_step_list).  Everything else is the window call's (ia_level_nbhd.cpp): its checks, prologue,
// DB, step buffers and its step, run_nbhd_step, given a slice of the list instead of the wavefront's
// geometry; the stats are the side paths' tail (ia_level_stats.cpp).
#include <cmath>
#include <cstring>

#include "ia_level.h"

namespace ia_host {

static const char *const WHO = "ia_synthesize_levels_masked";

struct MaskIn {
  const uint8_t *const *mask;
  const int32_t *const *s, *const *im;
};

// The level after its staging.  The jobs' masks go to one device buffer (job-major) and the kept
// state to the jobs' S / IM buffers (host memory; device memory: checked in place, copied to s_out /
// im_out only once nothing can refuse the call).  One read-back brings the pre-pass's verdict and the
// step offsets; it decides the buffer sizes (the largest step, not the widest wavefront) and whether
// anything runs at all.  Then the window call's DB (with its finite check) and the non-empty steps.
static int run_mask_level(ia_ctx *c, const ia_level_args *args, LevelPlan &P, LevelInputs &in, const NbhdGeo &w,
                          const MaskIn &mk, ia_stats *stats) {
  const LevelGeo &g = P.g;
  const int J = P.J;
  const int64_t NB = P.NB;
  const bool host = args[0].mem == IA_MEM_HOST;
  const hipMemcpyKind in_kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  int rc;
  ia_wavefront_shape_pad(g.bh, g.bw, w.p_l, &P.T, &P.Mmax);
  const int T = (int)P.T;
  if ((rc = stage_jobs(c, P, in)) || (rc = c->mk_mask.ensure((size_t)J * NB)) || (rc = c->mk_off.ensure((size_t)(T + 1) * 4)) ||
      (rc = c->xerr.ensure(4)) || (rc = c->counters.ensure(5 * 8)))
    return rc;
  uint8_t *mask = c->mk_mask.as<uint8_t>();
  int32_t *off = c->mk_off.as<int32_t>();
  HIP_TRY(hipMemsetAsync(c->xerr.p, 0, 4, c->st));
  HIP_TRY(hipMemsetAsync(c->counters.p, 0, 5 * 8, c->st));
  for (int j = 0; j < J; j++) {
    HIP_TRY(hipMemcpyAsync(mask + (size_t)j * NB, mk.mask[j], (size_t)NB, in_kind, c->st));
    const int32_t *s = mk.s[j], *im = mk.im[j];
    if (host) {  // the jobs' S / IM buffers (stage_level): what finish_level copies back
      HIP_TRY(hipMemcpyAsync(in.jp[j].s, s, (size_t)NB * 8, hipMemcpyHostToDevice, c->st));
      HIP_TRY(hipMemcpyAsync(in.jp[j].im, im, (size_t)NB * 4, hipMemcpyHostToDevice, c->st));
      s = in.jp[j].s;
      im = in.jp[j].im;
    }
    ia_launch_mask_check(s, im, NB, g.n_ap, g.ah, g.aw, c->xerr.as<unsigned>(), c->st);
  }
  HIP_TRY(hipEventRecord(c->kb[0], c->st));
  ia_launch_mask_count(mask, NB, J, g.bh, g.bw, w.p_l, T, off, c->st);
  HIP_TRY(hipEventRecord(c->kb[1], c->st));
  HIP_TRY(hipGetLastError());
  unsigned bad = 0;
  std::vector<int32_t> off_h((size_t)T + 1);
  HIP_TRY(hipMemcpyAsync(&bad, c->xerr.p, 4, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipMemcpyAsync(off_h.data(), off, (size_t)(T + 1) * 4, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  if (bad)
    return fail(IA_EINVAL, std::string(WHO) + ": a pixel's im_in is >= n_ap, or its im_in is >= 0 and its s_in lies outside "
                                              "[0, a_h) x [0, a_w)");
  const int64_t total = off_h[T];
  int64_t steps = 0, Mt_max = 0;
  for (int t = 0; t < T; t++) {
    const int n = off_h[t + 1] - off_h[t];
    steps += n > 0;
    Mt_max = std::max<int64_t>(Mt_max, n);
  }

  int64_t scans = 0;
  float ms_list = 0.f, ms_fill = 0.f;
  hipEventElapsedTime(&ms_list, c->kb[0], c->kb[1]);
  NbhdScan scan;
  if (total > 0 &&  // the step buffers, and the window call's DB (with its finite check)
      ((rc = c->mk_list.ensure((size_t)total * sizeof(int2))) || (rc = ensure_nbhd_steps(c, g, w, Mt_max, &scan)) ||
       (rc = build_nbhd_db(c, P, in, w, WHO, &scan))))
    return rc;
  // nothing refuses the call from here on: device-memory jobs take their kept state
  for (int j = 0; j < J && !host; j++) {
    if (mk.s[j] != in.jp[j].s) {
      HIP_TRY(hipMemcpyAsync(in.jp[j].s, mk.s[j], (size_t)NB * 8, hipMemcpyDeviceToDevice, c->st));
    }
    if (mk.im[j] != in.jp[j].im) {
      HIP_TRY(hipMemcpyAsync(in.jp[j].im, mk.im[j], (size_t)NB * 4, hipMemcpyDeviceToDevice, c->st));
    }
  }
  if (total > 0) {
    const int2 *list = c->mk_list.as<int2>();
    HIP_TRY(hipEventRecord(c->kb[2], c->st));
    ia_launch_mask_fill(mask, NB, J, g.bh, g.bw, w.p_l, T, off, c->mk_list.as<int2>(), c->st);
    HIP_TRY(hipEventRecord(c->kb[3], c->st));
    for (int t = 0; t < T; t++) {
      const int Mt = off_h[t + 1] - off_h[t];
      if (Mt <= 0) continue;  // only the steps that hold a masked pixel run
      scans += run_nbhd_step(c, g, in, w, scan, NbhdStep{StepDesc{}, list + off_h[t], Mt});
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->lv2, c->st));
  }
  if ((rc = finish_level(c, args, P, in, false, stats != nullptr))) return rc;
  if (total > 0) hipEventElapsedTime(&ms_fill, c->kb[2], c->kb[3]);
  c->mk_levels += J;
  c->mk_list_ms += ms_list + ms_fill;
  return stats ? accumulate_side_stats(c, total, steps, scans, total > 0, stats) : IA_OK;  // (no nbhd_levels: the window call's)
}

}  // namespace ia_host

using namespace ia_host;

extern "C" {

int ia_masked_step_list(int h, int w, int pad, const uint8_t *mask, int32_t *offsets, int32_t *pixels) {
  if (h < 1 || w < 1 || pad < 0 || pad > 4 || !mask || !offsets || (int64_t)h * w >= (int64_t)INT32_MAX)
    return fail(IA_EINVAL, "ia_masked_step_list: empty or too large level, pad outside 0..4, or NULL mask / offsets");
  const int64_t k = pad + 1, T = (int64_t)w + k * (int64_t)(h - 1);
  int32_t n = 0;
  for (int64_t t = 0; t < T; t++) {
    offsets[t] = n;
    int r0, M;
    ia_wavefront_step_pad(h, w, pad, t, &r0, &M);
    for (int r = r0; r < r0 + M; r++) {
      const int64_t qi = (int64_t)r * w + (t - k * r);
      if (!mask[qi]) continue;
      if (pixels) pixels[n] = (int32_t)qi;
      n++;
    }
  }
  offsets[T] = n;
  return IA_OK;
}

int ia_masked_stats(ia_ctx *c, int64_t *levels, double *list_ms) {
  if (!c) return fail(IA_EINVAL, "ia_masked_stats: NULL context");
  if (levels) *levels = c->mk_levels;
  if (list_ms) *list_ms = c->mk_list_ms;
  return IA_OK;
}

int ia_synthesize_levels_masked(ia_ctx *c, const ia_level_args *args, int n_jobs, int n_sm, int n_lg,
                                const uint8_t *const *mask, const int32_t *const *s_in, const int32_t *const *im_in,
                                ia_stats *stats) {
  if (!c || !args) return fail(IA_EINVAL, std::string(WHO) + ": NULL argument");
  int rc;
  if ((rc = check_level_batch(args, n_jobs)) || (rc = check_nbhd(c, args, n_jobs, n_sm, n_lg, WHO))) return rc;
  if (!mask || !s_in || !im_in) return fail(IA_EINVAL, std::string(WHO) + ": NULL mask, s_in or im_in");
  for (int j = 0; j < n_jobs; j++)
    if (!mask[j] || !s_in[j] || !im_in[j])
      return fail(IA_EINVAL, std::string(WHO) + ": NULL mask, s_in or im_in of job " + std::to_string(j));
  if ((int64_t)n_jobs * args[0].b_h * args[0].b_w >= (int64_t)INT32_MAX)
    return fail(IA_EINVAL, std::string(WHO) + ": n_jobs b_h b_w exceeds the int32 step offsets");
  HIP_TRY(hipSetDevice(c->dev));
  const NbhdGeo w = ia_nbhd_geo(args[0].ch, n_sm, n_lg);
  LevelPlan P;
  LevelInputs in;
  if ((rc = plan_nbhd_level(c, args, n_jobs, w, P, in))) return rc;
  return run_mask_level(c, args, P, in, w, MaskIn{mask, s_in, im_in}, stats);
}

}  // extern "C"

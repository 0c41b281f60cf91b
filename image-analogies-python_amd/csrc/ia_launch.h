// ia_launch.h — host launchers of the kernels in ia_level_db.hip, ia_gather.hip, ia_k3.hip,
// ia_kernels.hip (the per-step merges), ia_merge_shard.hip, ia_dense.hip, ia_k3r.hip, ia_prune.hip,
// ia_kcoh.hip, ia_nbhd.hip, ia_mask.hip, ia_ann.hip, ia_pyramid.hip and ia_k3h.hip (the latter in ia_k3p_launch.hip); used by the host units (ia_host.h).
// ia_k3.hip and ia_k3r.hip scan with one body (ia_k3_scan.h): ia_launch_k3, ia_launch_k3r_count and
// ia_launch_k3r_fill take the same geometry (n_tiles, tpw, nwg; qt <= ia_k3_qtmax(KH) tiles from qt0).
#pragma once
#include <hip/hip_runtime.h>

#include "ia_internal.h"

// allow a kernel the whole LDS of a CU as dynamic shared memory (once per kernel; thread-safe)
void ia_allow_full_lds(const void *fn);
// the DB builders: ap = the A side's per-image strides (pairs) or zeros (one shared A)
void ia_launch_means(int ch, const Imgs &A, const APairs &ap, int n_ap, double *mu, hipStream_t st);
void ia_launch_db_build(const LevelGeo &g, const Imgs &A, const APairs &ap, const double *mu, float4 *db, unsigned *Rbits,
                        hipStream_t st);
void ia_launch_gather(const LevelGeo &g, const StepDesc &sd, const Imgs &B, const JobSet &jobs, const double *mu, double *q64,
                      double *qn2, float *qf, hipStream_t st);
int ia_k3_qtmax(int KH);
void ia_launch_k3(int KH, int qt, const float4 *db, const float4 *qf, int n_tiles, int tpw, int qt0, int M, int nwg,
                  int row0, int NT, float4 *rec, float *recT, hipStream_t st);
void ia_launch_merge(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &ma, Winner *win,
                     const JobSet &jobs, bool fused, hipStream_t st);
// fused K4 of step sd + the gather of step nx.sn (K2p when pruned, else K2h; 1-channel levels,
// <= 256 records per query)
void ia_launch_merge_gather(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &ma, const JobSet &jobs,
                            const Imgs &B, const NextStep &nx, bool pruned, hipStream_t st);
void ia_launch_finish(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const double *db64, const double *q64,
                      const Winner *allwin, int world, int Mstride, const JobSet &jobs, hipStream_t st);
void ia_launch_db64_build(const LevelGeo &g, const Imgs &A, const APairs &ap, double *db64, hipStream_t st);
int ia_db64_stride(int ch);
void ia_launch_reduce_stats(const unsigned *pstat, int64_t n, unsigned long long *counters, hipStream_t st);
// option "stamps": per launch (min start, max end) ticks over its stride workgroup slots
void ia_launch_stamp_durations(const unsigned long long *stamps, int n, int stride, unsigned long long *span, hipStream_t st,
                               unsigned long long *span2 = nullptr);
void ia_launch_dense_db(int KH, const double *pts, int64_t n, int d, int n_tiles, const double *mu, double sc, float4 *db,
                        unsigned *Rbits, hipStream_t st);
void ia_launch_dense_query(int KH, const double *q, int64_t nq, int d, int Mpad, const double *mu, double sc, double *qn2,
                           float *qf, hipStream_t st);
void ia_launch_merge_dense(const MergeArgs &ma, const double *pts, int d, const double *q, int64_t nq, double dsc,
                           int64_t *idx, double *dist, hipStream_t st);
// exact k-NN merge of the index (1 <= k <= 64): idx / dist are nq x k; counters[0..1] accumulate
void ia_launch_merge_dense_knn(const MergeArgs &ma, const double *pts, int d, const double *q, int64_t nq, int k, double dsc,
                               int64_t *idx, double *dist, unsigned long long *counters, hipStream_t st);
// exact fixed-radius search of the index (ia_k3r.hip; sequence in ia_index_radius.cpp).  thr: (hi, lo)
// per padded query; cnt / seg: one record per (query, scan workgroup); ts: (candidates, certain rows)
// per query; qoff / soff: where a query's candidates / staged results start; [j0, j1): the queries of
// a fill sub-batch
void ia_launch_k3r_thresholds(const double *radius, const double *qn2, const unsigned *Rbits, int nq, int Mpad, double dsc,
                              double eps_c, float2 *thr, hipStream_t st);
void ia_launch_k3r_count(int KH, int qt, const float4 *db, const float4 *qf, const float2 *thr, int n_tiles, int tpw, int qt0,
                         int M, int nwg, uint2 *cnt, hipStream_t st);
void ia_launch_k3r_offsets(const uint2 *cnt, int nq, int nwg, bool count_only, uint2 *seg, uint2 *ts, hipStream_t st);
void ia_launch_k3r_fill(int KH, int qt, bool count_only, const float4 *db, const float4 *qf, const float2 *thr, int n_tiles,
                        int tpw, int qt0, int j0, int j1, int nwg, const uint2 *seg, const unsigned *qoff, int *cand,
                        hipStream_t st);
void ia_launch_k3r_verify(const double *pts, int64_t n, int d, int NT, const double *q, const double *radius, const uint2 *ts,
                          const unsigned *qoff, int j0, int j1, unsigned max_len, int *wr, double *wd, hipStream_t st);
void ia_launch_k3r_finish(bool count_only, const uint2 *ts, const unsigned *qoff, const unsigned *soff, int j0, int j1,
                          int *wr, double *wd, int64_t *sidx, double *sdist, int64_t *cntq, hipStream_t st);
int ia_k3r_sort_lds();  // longest segment k3r_finish sorts in LDS
void ia_launch_coherence_batch(const double *pts, int64_t n, int d, const double *q, int64_t nq, const int32_t *px,
                               const int32_t *s, const int32_t *im, int64_t n_s, int a_h, int a_w, int bp_w, int pad,
                               int32_t *p_out, int32_t *img_out, int32_t *r_out, unsigned *err, hipStream_t st);
// the approximate index (ia_ann.hip; sequence in ia_ann.cpp).  rows / off: the lists (row indices list
// after list, L + 1 offsets); centT: the centres transposed, d x L
void ia_launch_ann_assign(const double *pts, int64_t n, int d, const double *cent, int L, int32_t *assign, hipStream_t st);
void ia_launch_ann_update(const double *pts, int d, const int32_t *rows, const int32_t *off, int L, double *cent,
                          hipStream_t st);
void ia_launch_ann_permute(const double *pts, int d, const int32_t *rows, int64_t n, double *out, hipStream_t st);
void ia_launch_ann_query(const double *rows, const int32_t *ids, const int32_t *off, const double *centT, int L, int d,
                         const double *q, int nq, int k, int need, int64_t *idx, double *dist, unsigned long long *counters,
                         hipStream_t st);
// split-f16 matcher (IA_MATCH_F16X3)
int ia_ks_for(int ch);
double ia_k3h_tile_bytes(int KS);  // HBM bytes of one split-f16 DB tile (TileFmt)
int ia_k3h_qtmax(int KS);
void ia_launch_absmax(const double *const *p, const int64_t *n, unsigned *out, hipStream_t st);
void ia_launch_db_build_h(const LevelGeo &g, const Imgs &A, const double *db64, const double *mu, void *db, unsigned *Rbits,
                          hipStream_t st);
void ia_launch_gather_h(const LevelGeo &g, const StepDesc &sd, const Imgs &B, const JobSet &jobs, const double *mu,
                        double *q64, double *qn2, void *qf, hipStream_t st);
void ia_launch_k3h(int KS, int qt, const void *db, const void *qf, int n_tiles, int tpw, int qt0, int M, int nwg, int row0,
                   int NT, float4 *rec, float *recT, hipStream_t st);
void ia_launch_fill_random_f16(void *p, int64_t n, unsigned seed, hipStream_t st);
// certified pruned scan: per-level setup (ia_prune.hip)
void ia_launch_cov(const double *db64, int64_t NA, int64_t stride, int nwg, const double *mu_part, double *part,
                   double *cov, hipStream_t st);
void ia_launch_proj_keys(const double *db64, int64_t NA, const double *mu_part, const double *basis, double *proj,
                         unsigned *keys, int *rows, float *rnorm, hipStream_t st);
size_t ia_sort_temp_bytes(int64_t n);
int ia_sort_pairs(void *temp, size_t temp_bytes, const unsigned *keys_in, unsigned *keys_out, const int *vals_in,
                  int *vals_out, int64_t n, hipStream_t st);
void ia_launch_table_boxes(const int *sorted_rows, const double *proj, int64_t NA, int n_tiles, int W, int G, int *pos2row,
                           float *boxes, const float *rnorm, float *tnorm, hipStream_t st);
void ia_launch_gather_p(const LevelGeo &g, const StepDesc &sd, const Imgs &B, const JobSet &jobs, const double *mu,
                        double *q64, double *qn2, void *qf, const double *db64, const double *basis, double ufac,
                        float4 *qinfo, const Imgs &A, hipStream_t st, const XOPub *xp = nullptr);
void ia_launch_query_sort(const float4 *qinfo, const void *qf, int Mpad, int KS, int *order, float4 *sq, void *qfs,
                          float4 *tbox, hipStream_t st);
// owner-computes sharded step (exchange = 2): the owner's queries sorted into every rank's area
void ia_launch_query_sort_xo(const float4 *qinfo, const void *qf, const XOSort &xs, hipStream_t st);
void ia_merge_gather_occupancy(int *vgprs, int *blocks_per_cu, int *wg_threads);
// One pruned scan launch (ia_k3h.hip k3h_prune3).  The caller names option "k3p_variant" and
// says whether the queries arrive presorted (K2s or the previous fused launch's gathers sorted
// them: qf / qinfo / order / tbox are then k_query_sort's outputs); which kernel instance that
// means for this launch is decided next to the launcher (ia_k3p_launch.hip k3p_kernel).
struct K3pLaunch {
  const void *db;              // the scanned DB slice: its first stored tile ...
  int NT;                      // ... and its tiles
  const void *qf;              // the step's query fragments ...
  const float4 *qinfo;         // ... and pruning records
  const int *order = nullptr;  // presorted: sorted slot -> query ...
  const float4 *tbox = nullptr;  // ... and the sorted query tiles' boxes (nullptr: taken from the slice)
  const float4 *boxes;         // of the slice: tile boxes, position -> row, R_t per tile
  const int *pos2row;
  const float *tnorm;
  int qt, qt0, M, Mpad;        // query tiles per block, first tile, the step's queries (padded)
  int nwg;                     // DB chunks: workgroups per query block
  int nqb = 1, qt_end = 0;     // presorted / owner-computes: query blocks of one launch, their last tile
  float4 *rec = nullptr;       // records (owner-computes: pushed to the owners' areas instead)
  float *recT = nullptr;
  unsigned long long *pairs, *tiles;  // per-workgroup counter slots
  int step, r0;                // step parity picks the walk direction
  const XOScan *xo = nullptr;  // owner-computes step: its exchange
  unsigned long long *stamp = nullptr;  // option "stamps"
  int rec_wt = 0;              // option "rec_wt"
};
// returns IA_EINVAL (nothing launched) when no kernel instance exists for the variant
int ia_launch_k3p(const K3pLaunch &a, int option, bool presorted, hipStream_t st);
// k-coherence search (ia_kcoh.hip): one wavefront step of a level with similarity sets sim
// (NA x K rows), all jobs, with H = ia_kcoh_scan_waves(NA) scan waves for the pixels without a base
// row (part: 16 H bytes per query of the widest step; cnt: one word per query, zero between steps);
// and the pre-pass that sets *err when one of sim's n entries is no DB row
int ia_kcoh_scan_waves(int64_t NA);
void ia_launch_kcoh_step(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const Imgs &B, const JobSet &jobs,
                         const double *db64, const int32_t *sim, int K, int H, void *part, unsigned *cnt, hipStream_t st);
void ia_launch_kcoh_check(const int32_t *sim, int64_t n, int NA, unsigned *err, hipStream_t st);
// exact levels for runtime window sizes (ia_nbhd.hip; include/ia.h ia_synthesize_levels_nbhd): the
// windows of a level and where a row's four parts start (o1, o2, o3; D values in all)
struct NbhdGeo {
  int ch, n_sm, n_lg, p_s, p_l, n_half;
  int o1, o2, o3, D;
};
inline NbhdGeo ia_nbhd_geo(int ch, int n_sm, int n_lg) {
  NbhdGeo w{ch, n_sm, n_lg, n_sm / 2, n_lg / 2, n_lg * n_lg / 2, 0, 0, 0, 0};
  w.o1 = ch * n_sm * n_sm;
  w.o2 = w.o1 + ch * n_lg * n_lg;
  w.o3 = w.o2 + ch * n_sm * n_sm;
  w.D = w.o3 + ch * w.n_half;
  return w;
}
// the fp64 row DB (NA x w.D, contiguous), then mu[0..D) = its column means and *amax_bits (zeroed by
// the caller) = the bits of the largest centred |value| as a float, rounded up
void ia_launch_nbhd_rows(const NbhdGeo &w, const Imgs &A, const APairs &ap, int64_t NA, double *rows, double *mu,
                         unsigned *amax_bits, hipStream_t st);
// One step of a window level, from either window call: n queries, the wavefront step sd's (list =
// nullptr; n = sd.J sd.M, query m at pixel (r, sd.t - (p_l + 1) r)) or the entries list[0..n) of a
// masked step's list (job, raster index; sd unused).
struct NbhdStep {
  StepDesc sd;
  const int2 *list;
  int n;
};
// the step's query rows q[m, 0..D), m < n, and its pixels' coherence pick, kappa rule and writeback
// from the certified winners idx[m] (a listed step's pick skips cells without a source)
void ia_launch_nbhd_gather(const NbhdGeo &w, const NbhdStep &step, const Imgs &B, const JobSet &jobs, double *q, hipStream_t st);
void ia_launch_nbhd_finish(const NbhdGeo &w, const LevelGeo &g, const NbhdStep &step, const Imgs &A, const JobSet &jobs,
                           const double *rows, const double *q, const int64_t *idx, hipStream_t st);
// masked resynthesis (ia_mask.hip; include/ia.h ia_synthesize_levels_masked).  The pre-pass sets *err when a
// pixel's im >= n_ap, or im >= 0 with s outside A.  mask: J x NB bytes, job-major.  count: offsets[t] = where
// step t's entries start among all T steps' (offsets[T] = the total), entries in (job, row) ascending
// order; fill: list[offsets[t] ..] = step t's (job, raster index), which ia_launch_nbhd_gather / _finish take
// as a listed NbhdStep
void ia_launch_mask_check(const int32_t *s, const int32_t *im, int64_t NB, int n_ap, int ah, int aw, unsigned *err,
                          hipStream_t st);
void ia_launch_mask_count(const uint8_t *mask, int64_t NB, int J, int bh, int bw, int pad, int T, int32_t *offsets,
                          hipStream_t st);
void ia_launch_mask_fill(const uint8_t *mask, int64_t NB, int J, int bh, int bw, int pad, int T, int32_t *offsets, int2 *list,
                         hipStream_t st);
// GPU preprocessing (ia_pyramid.hip)
void ia_launch_pyramid_reduce(const double *in, double *out, double *tmp, double *sm, double *mm, int h, int w, int ch,
                              const double *w7, hipStream_t st);
void ia_launch_color3(const double *in, double *out, int64_t npx, const double *M, hipStream_t st);
// sharded level, peer-write winner exchange (option "exchange" = 1): shard winner -> every rank's
// buffer; fin: wait for the W winners of each query and finish the pixel
void ia_launch_merge_xchg(const LevelGeo &g, const StepDesc &sd, const Imgs &A, const MergeArgs &ma, const XchgArgs &xa,
                          const JobSet &jobs, bool fin, hipStream_t st);

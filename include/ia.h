/*
 * ia.h — C ABI of the MI355X-native Image Analogies best-match core (libia.so).
 *
 * The reference (flair2005/image-analogies-python) reaches native code in exactly one place:
 * pyflann, a ctypes shim over libflann's C ABI, called from algorithms.py:56 (pf.FLANN()),
 * algorithms.py:69 (build_index) and algorithms.py:74 (nn_index).  Everything else on the hot
 * path is the Python raster loop image_analogies.py:130-239.  This header replaces both:
 *
 *   ia_index_*            drop-in for the FLANN object API (algorithms.py:56,69,74):
 *                         build an exact-NN index over caller rows, query it in batches.
 *   ia_synthesize_level   drop-in for one iteration of the per-level loop
 *                         (image_analogies.py:130-239 incl. create_index's DB for that level,
 *                         algorithms.py:50-70): DB build, skewed-wavefront schedule, exact NN,
 *                         coherence, kappa selection and B'/s/im writeback, all on the GPU.
 *
 * Conventions (pyflann's, kept): caller-owned C-contiguous buffers, library-owned opaque
 * handles, integer status returns (0 = ok, negative IA_E* on error, never throws across the
 * ABI), thread-local ia_last_error().  Images are row-major (h, w[, ch]) fp64 in [0,1] scale
 * exactly as the reference keeps them; index outputs are int32/int64.
 * A context is not thread-safe; one host thread drives one context (one GPU).
 */
#ifndef IA_H_
#define IA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IA_OK 0
#define IA_EINVAL -1   /* bad argument / shape contract violated */
#define IA_EHIP -2     /* HIP runtime error */
#define IA_ENOMEM -3   /* device allocation failed */
#define IA_ENODEV -4   /* no usable gfx950 device */
#define IA_ECOMM -5    /* RCCL error */

#define IA_MEM_HOST 0   /* pointers in ia_level_args are host (numpy) memory */
#define IA_MEM_DEVICE 1 /* pointers are device memory already resident in HBM */

typedef struct ia_ctx ia_ctx;
typedef struct ia_index ia_index;

/* Per-call statistics (SURVEY §5 'Metrics'). */
typedef struct {
  int64_t pixels;          /* B' pixels synthesised */
  int64_t steps;           /* wavefront steps executed */
  int64_t coherence_wins;  /* pixels whose source came from best_coherence_match */
  int64_t reranked;        /* exact fp64 reranks of MFMA candidates */
  int64_t fallbacks;       /* uncertified DB chunks rescanned exactly */
  double db_ms;            /* DB build time (device) */
  double synth_ms;         /* wavefront time (device) */
  int64_t dist_launches;   /* MFMA distance kernel launches */
  double dist_flops;       /* algorithmic flops 2*D*N_A*(queries) of those launches */
  /* sampled timing of the MFMA distance kernel (option "time_dist" = sampling stride S > 0:
   * every S-th wavefront step's distance launches are bracketed by HIP events) */
  double dist_ms;          /* device time of the sampled launches */
  int64_t dist_launches_timed;
  double dist_flops_timed; /* algorithmic flops of the sampled launches */
  int64_t bound_violations; /* pixels where a reranked candidate's exact distance fell outside
                             * the certified MFMA error bound (audit; expected 0) */
  int64_t f16_levels;       /* levels run on the split-f16 matcher */
  int64_t pruned_levels;    /* levels run on the certified pruned scan (option "prune") */
  double dist_pairs;        /* (DB tile, query tile) pairs the distance kernel contracted */
  double dist_pairs_full;   /* pairs an unpruned scan contracts (dist_pairs / this = work left) */
  double dist_tiles;        /* DB tiles the distance kernel loaded (summed over its launches) */
  double dist_tiles_full;   /* DB tiles an unpruned scan loads (dist_tiles / this = DB bytes left) */
  double prune_ms_timed;    /* pruned-scan launches of the timed steps (option "time_dist"): device ms */
  int64_t prune_launches_timed;
  double prune_flops_timed; /* their MFMA flops (computed pairs x 2 D 32 32) */
  double prune_bytes_timed; /* their algorithmic bytes (DB tiles loaded, boxes, queries, records) */
  int64_t kappa_ambiguous;  /* pixels whose kappa decision (image_analogies.py:206) would flip if
                             * compute_distance's `** 2` (libm pow on a numpy scalar) rounded a
                             * near-midpoint square the other way than y * y does (audit; no
                             * fixture has one) */
  double dist_pairs_corrected; /* the pruned scan's hi x hi block filter (ia_k3h.hip, k3p_bound):
                                * pairs whose hi x hi value passed the bound (correction products +
                                * top-2 epilogue run); 0 without the pruned scan */
  double dist_tiles_rows;   /* the same filter: loaded DB tiles with at least one block passing it
                             * (the only ones whose lo halves the correction products read) */
  /* feature-gather kernels (bench.py roofline.gathers; DESIGN.md §4 algorithmic bytes) */
  double k1b_ms;            /* K1b k_db64_build (fp64 row DB), device ms summed over the levels */
  double k1b_bytes;         /* its algorithmic bytes: A-side images read once + N_A rows written */
  double k1_ms;             /* K1 k_db_build_h (split-f16 tiles), device ms summed over the levels */
  double k1_bytes;          /* its algorithmic bytes: fp64 rows read + tiles written */
  int64_t build_levels;     /* levels summed in k1*_ms / k1*_bytes: those with the largest DB
                             * (build_rows) this ia_stats has seen (the bench's finest level) */
  double gather_ms_timed;   /* K2 (k_gather_query_*) of the sampled steps ("time_dist"): device ms */
  int64_t gather_launches_timed;
  double gather_bytes_timed; /* their algorithmic bytes: 55 features + 12 coherence rows read,
                              * fp64 row + fragments + pruning record written per query */
  double merge_ms_timed;    /* K4 (k_merge_level) of the sampled steps: device ms */
  int64_t merge_launches_timed;
  int64_t build_rows;       /* DB rows of the levels in k1*_ms (the largest seen) */
  /* option "stamps" = 1: device time of EVERY pruned-scan launch and every fused merge launch of
   * the pruned levels, from per-workgroup s_memrealtime stamps written by the kernels themselves
   * (no HIP events, nothing on the stream between kernels: valid in pipelined / concurrent runs) */
  double k3p_stamp_ms;      /* summed over the launches: max(WG end) - min(WG start) each */
  int64_t k3p_stamp_launches;
  double k3p_bytes_all;     /* algorithmic bytes of those launches (tiles loaded, boxes, queries, records) */
  double merge_stamp_ms;    /* the merges (k_merge_gather / fused k_merge_level) of the same levels */
  int64_t merge_stamp_launches;
  double stamp_gap_ms;      /* one-job levels: idle time between the chain's kernels (scan end -> merge
                             * start, merge end -> next scan start), summed */
  int64_t stamp_gaps;
  double stamp_window_ms;   /* those levels' first scan start -> last kernel end */
  int64_t prune_rows;       /* DB rows of the pruned levels in prune_*, k3p_*, merge_stamp_* and
                             * stamp_* (the largest pruned level seen: the bench's finest) */
  double k3p_stamp_start_ms; /* the same K3p launches: last workgroup start - first start, summed */
  double k3p_stamp_wg_ms;    /* ... their mean workgroup duration (end - start), summed */
  double stamp_gap_sm_ms;   /* the scan end -> merge start part of stamp_gap_ms */
  int64_t stamp_gaps_sm;
  double k3p_bytes_unique_all; /* k3p_bytes_all with each launch's DB tiles counted at most once
                                * (<= the launch's whole tiles): launches of several query blocks
                                * stream a tile once per block (cfg4's wide steps) */
  /* k-coherence levels (ia_synthesize_levels_kcoh) */
  int64_t kcoh_levels;      /* levels (jobs) run by k-coherence search */
  int64_t kcoh_fallbacks;   /* their pixels without a base row: exact NN over the whole DB */
  int64_t kcoh_candidates;  /* candidate rows (base rows and their similar rows) whose exact
                             * distance was computed; a fallback pixel's DB scan is not counted */
  /* levels of other window sizes (ia_synthesize_levels_nbhd) */
  int64_t nbhd_levels;      /* levels (jobs) run by that call; it also adds to pixels, steps,
                             * coherence_wins, kappa_ambiguous, dist_launches, db_ms and synth_ms */
} ia_stats;

/* One pyramid level (image_analogies.py:130-239).  Shapes: A/A' level l is (a_h, a_w[, ch]),
 * level l-1 is (ceil(a_h/2), ceil(a_w/2)[, ch]); same for B.  Ap / Apc stack n_ap images.
 * The A side is one image shared by every A' (the reference, algorithms.py:63-67: n_a = 0 or 1)
 * or one image per A' (n_a = n_ap: training pairs (A_i, A'_i) of equal shape, A / Ac stacked the
 * way Ap / Apc are).  DB row img * a_h * a_w + r * a_w + c holds the features of pixel (r, c) of
 * pair img: [A_i 3x3 | A_i 5x5 | A'_i 3x3 | A'_i first 12] with A_i = A for a shared A.
 * Bp: in = initial B' level (initialize_Bp, img_preprocess.py:66-78), out = synthesised.
 * s_out (N x 2, row/col in A) and im_out (N) are the reference's s / im lists for this level. */
typedef struct {
  int ch;          /* channels per pixel: 1 (luminance / grayscale), 2 or 3.  The reference writes
                    * colour back for 3 channels only, so 2 channels have no reference run: they
                    * are pinned to the oracle (oracle/ia_oracle.py, tests/test_gpu_channels.py) */
  int n_ap;        /* number of A' images (Ap_fname_list) */
  int a_h, a_w;    /* A level l */
  int b_h, b_w;    /* B level l */
  const double *A, *Ac;     /* A level l, l-1 (already AB_weight-compressed, image_analogies.py:65) */
  const double *Ap, *Apc;   /* A' level l, l-1, n_ap stacked */
  const double *B, *Bc;     /* B level l, l-1 (compressed) */
  const double *Bpc;        /* B' level l-1, complete */
  double *Bp;               /* B' level l: in init, out synthesised */
  const double *weights;    /* compute_distance weights (config.py:68-79), 55*ch */
  double kappa_factor;      /* 1 + 2^(level - max_levels) * k   (image_analogies.py:206) */
  int32_t *s_out;           /* N x 2 */
  int32_t *im_out;          /* N */
  int mem;                  /* IA_MEM_HOST or IA_MEM_DEVICE for every pointer in this struct */
  /* Optional debug structures of image_analogies_main(debug=True) (image_analogies.py:141-153,
   * 224-240); both NULL (off) or both given, single-rank levels only.  Per raster pixel:
   * dbg_src  N x 6 int32: p_app row, col, image (the NN, Ap_ix2px of best_approximate_match),
   *          r_star row, col (best_coherence_match, algorithms.py:126-130; 0, 0 without one),
   *          has_coh (1 when a coherence candidate existed, i.e. the kappa rule compared);
   * dbg_dist N x 2 fp64: v_app, v_coh = x.dot(x) of compute_distance's x = (a - q) * w
 *          (algorithms.py:133-135) in the golden host's BLAS order; 0 when has_coh = 0.
 *          compute_distance itself is np.sqrt(v) ** 2 with libm's pow (numpy scalar power),
 *          which is not always v's correctly rounded square root squared: the host applies it. */
  int32_t *dbg_src;
  double *dbg_dist;
  int n_a;         /* A images: 0 or 1 = one A shared by all n_ap A' images; n_ap = one A per A'
                    * (A and Ac stack n_a images).  Any other value is IA_EINVAL.  Last field, so
                    * callers built against version 1 (which zero-initialise the struct) keep
                    * their layout and their meaning */
} ia_level_args;

/* ---- context ---------------------------------------------------------------------------- */
int ia_init(int device, ia_ctx **out);
void ia_destroy(ia_ctx *ctx);
const char *ia_last_error(void);
int ia_version(void);  /* 4: ia_synthesize_levels_nbhd, ia_wavefront_*_pad, ia_stats.nbhd_levels;
                        * 3: ia_synthesize_levels_kcoh, ia_index_similarity, ia_stats.kcoh_*; 2: ia_level_args.n_a
                        * (1: the struct ended at dbg_dist) */
/* Options: "time_dist" = S (0 = off): bracket the MFMA distance launches of every S-th
 * wavefront step with HIP events; ia_stats.dist_ms / dist_flops_timed then give the kernel's
 * measured device time and algorithmic flops (bench.py roofline).
 * "matcher" = IA_MATCH_F16X3 (default: split-f16 MFMA scan, 1 and 2 channels, image values
 * within +-64) or IA_MATCH_F32 (fp32 MFMA scan).  Both are certified exact: identical results.
 * "prune" = 1 (default) / 0: certified pruned scan on 1-channel split-f16 levels with at least
 * "prune_min_rows" DB rows (default 2^19): (DB tile, query tile) pairs a
 * projection bound proves farther than the query's best coherence candidate are skipped.
 * "k3p_variant" / "k3_variant": kernel versions of DESIGN.md §4b / §4h / §4i; the product build
 * accepts k3p_variant 24 (default: the pruned scan sorts a step's queries itself up to 512 of
 * them, then runs two passes: every wave streams the hi halves of its DB tiles into LDS by
 * LDS-DMA, two tiles in flight, and runs the hi x hi block filter on the box-needed blocks;
 * then the tiles with a block that can lie within its query's bound get their full products +
 * top-2, handed out over the workgroup's waves; a step wider than 512 queries is sorted once by
 * k_query_sort and runs 21), 25 (24 presorted), 22 (one pass: the hi stream in registers, the
 * passing tiles' lo halves one tile later), 20 (whole tiles; 21 presorted) and k3_variant 1.
 * The other versions of DESIGN.md §4b / §4f are in git history.
 * "k3p_blocks" = 1 (default) / 0: a presorted pruned scan wider than one launch's 11 query tiles
 * runs as ONE launch of (query block x DB chunk) workgroups instead of one launch per block.
 * "fuse_gather" = 1 (default) / 0: on one-job unsharded pruned levels the merge of step t and the
 * gather of step t + 1 run as one launch (the step's results handed row to row through uncached
 * slots); 0 = separate launches.
 * "pipeline_last" = 1: the next level call has no dependents, so it records no per-step events
 * (level pipelining's finest level; applies to one call).
 * "stream_priority" = 0 (default) / 1 (high) / 2 (low): recreate the context's stream with that
 * priority (idle contexts; level pipelining puts the finest level's stream high).
 * "prune_group" = G in {1 (default), 2, 4, 8}: pruned levels store each group of G Morton tiles
 * interleaved (sort neighbours in different tiles and scan chunks: fewer certification rescans,
 * looser tile boxes).
 * "row_source" = 0 (exact rows of the rerank / coherence / pruning bound from the fp64 row DB);
 * 1 (gathered from the A-side pyramid images; measured slower) is in git history only.
 * "shard_emulate" = W (1 = off): on a single-rank context, every level with >= 64 W DB tiles
 * runs as a W-way DB shard on this device (per-shard scans and certified winners, then the
 * multi-rank finish; no RCCL): the sharded code path, testable on one GPU.
 * "shard_unpruned" = 0 (default) / 1: shard only the levels that run the pruned scan / every
 * level with >= 64 W tiles.  "exchange" = 0 (RCCL all-gather + finish) / 1 (peer-write merge)
 * / 2 (owner computes: each rank brings its own job, every rank scans its shard for all of them,
 * queries and scan records exchanged by peer writes; emulated: one job per shard).
 * "nn_bound" = 1 (default) / 0: on all pruned levels (every merge form: one-rank, sharded,
 * peer-write, owner-computes) the merge also keeps each pixel's certified
 * exact NN row, and the gathers bound U' (the pruned scan's radius) by the causal neighbours' NN
 * rows shifted by the neighbour's offset as well as by the coherence candidates (exact either way:
 * any DB row's exact distance bounds the NN distance).
 * "prefetch_next" = 1 (default) / 0: a fused merge + gather wave loads its next query's inputs
 * that do not depend on the launch's own merges (features, causal neighbours' sources) while
 * its merge's DB rows load.
 * "fuse_sort" = 0 (default) / 1 / 2: the fused gathers of step t + 1 also rank its queries' sort
 * keys across the launch and write the presorted scan inputs (no K2s launch, no per-workgroup
 * sort in the scan).  2: only on levels whose widest step has >= 512 queries (all jobs).  Exact
 * either way; no faster since option nn_bound.
 * Fused merge + gather launches (option "fuse_gather") wait row to row; a level uses them only
 * while the chained waves of all levels in flight in the process stay under twice the GPU's
 * resident k_merge_gather waves (else it runs separate launches; ia_ctx.cpp g_chain_waves).
 * "rec_wt" = 1 (default) / 0: the pruned scan stores its per-(query, chunk) records write-through
 * (sc1 buffer stores), so the scan -> merge kernel boundary has no dirty record lines to write
 * back (one-rank steps; the owner-computes exchange has its own uncached stores).  Exact either
 * way: the merge reads the records after the boundary.
 * "early_gather" = 1 (default) / 0: a fused merge + gather wave of a one-rank pruned level (option
 * prefetch_next on, no publish) runs its next query's gather up to the row above's late feature
 * before waiting for that handoff: the other 54 features, fragments, projection and |q'|^2 sums,
 * and U' over the candidate rows requested first; U' then leaves out the row above's own two
 * candidates (a valid bound either way).
 * "gather_wave" = 1 (default) / 0: that early path (one job, one rank, pruned level, options
 * prefetch_next and early_gather on, fuse_sort not engaged) runs workgroups of two waves: wave 0
 * merges the step-t pixel and nothing else, wave 1 gathers the next query beside it from wave
 * start and takes the merged pixel through LDS for its late part (the pixel's two U' candidate
 * rows, its window slots; then the row above's handoff as before).  Those two rows are the raster
 * successors of rows the merge wave's lanes hold, posted through LDS as soon as they are placed:
 * the gather wave loads every lane's successor during the merge and picks the two winners' by
 * lane, so no dependent row load follows the merge (a winner from an overflow candidate or a
 * certification rescan takes that load).  Same U' candidate rows as early_gather; only the
 * summation order of the own pixel's terms differs.  Such a level reserves
 * TWICE its waves of the chained-wave budget; where that is refused it runs the one-wave launches
 * with the single reservation, and where that is refused too, separate launches
 * (ia_chain_choice).  0, or any other merge + gather form (batched jobs, owner-computes,
 * fuse_sort, unpruned levels): the one-wave launches.
 * "scan_wgs" = 8..256 (a multiple of 8; default 256, one per CU): workgroups of the context's
 * split-f16 scans (pruned: one chunk of DB tiles each; unpruned: contiguous tile ranges).  bench.py
 * gives the coarser pipelined levels' contexts 128, so their scans never queue for the whole GPU
 * while the finest level's kernels are dispatched.
 * "stamps" = 1: every pruned-scan and fused-merge launch of a pruned level stamps its
 * workgroups' first / last s_memrealtime tick; ia_stats.k3p_stamp_ms / merge_stamp_ms sum the
 * per-launch device times (bench.py roofline.frac_timed: the timed, pipelined steps' own kernels).
 * "xo_presort" = 1: owner-computes steps always sort in a K2s launch (tests; default 0: steps of
 * <= 352 queries per owner are sorted inside the scan).  Environment IA_CU_SPLIT=k/n (rehearsals
 * of n ranks on ONE GPU only): the context's stream runs on CU slice k of n.
 * Identical results for every setting. */
#define IA_MATCH_F32 0
#define IA_MATCH_F16X3 1
int ia_set_option(ia_ctx *ctx, const char *name, int value);
/* Multi-GPU (one process per GPU): A rows of every level are split into `world` contiguous
 * shards; per wavefront step each rank exchanges its certified per-query winners with one
 * RCCL all-gather and every rank picks the same global winner (lowest index on ties).
 * ia_comm_unique_id fills 128 bytes on rank 0; broadcast them (torch.distributed) and call
 * ia_comm_init on every rank. */
int ia_comm_unique_id(unsigned char id_out[128]);
int ia_comm_init(ia_ctx *ctx, int rank, int world, const unsigned char id[128]);
/* One-shot peer-write exchanges for sharded levels (replace the RCCL all-gather +
 * finish of ia_comm_init).  Every rank calls ia_xchg_alloc (an uncached device buffer, zeroed:
 * 2 x world x 4096 16-byte winner slots for "exchange" = 1, then two parities of the owner
 * areas of "exchange" = 2, about 50 MiB) and publishes the returned 64-byte HIP IPC handle;
 * after gathering all world handles (rank order, world x 64 bytes) it calls ia_xchg_open, which
 * maps the peers' buffers and makes the context a rank of a world-rank DB shard (option
 * "exchange" = 1 unless 2 was set before).  No RCCL communicator is needed.  A peer that stops
 * publishing makes the level fail with IA_ECOMM after 20 s instead of hanging.  With option
 * "shard_emulate" = W and "exchange" = 1 / 2 a single process runs the same kernels over a
 * local buffer.  Every ia_xchg_open needs its own ia_xchg_alloc before the handle swap (a reused
 * buffer is zeroed there and the step sequence restarts on every rank alike; ia_comm_init
 * afterwards drops the peer mappings and returns to "exchange" = 0).  The ranks of one
 * exchange run the same sequence of level calls with identical A levels and identical B shapes
 * (per level): slots and sequence numbers are laid out from the local geometry, so ranks that
 * disagree time out (IA_ECOMM after 20 s) - check the shapes on the host first. */
int ia_xchg_alloc(ia_ctx *ctx, int world, unsigned char handle_out[64]);
int ia_xchg_open(ia_ctx *ctx, int rank, int world, const unsigned char *handles);

/* ---- fast path: one level ----------------------------------------------------------------- */
int ia_synthesize_level(ia_ctx *ctx, const ia_level_args *args, ia_stats *stats);
/* The same level for n_jobs independent jobs at once (multi_script.py's parameter sweeps,
 * multi_script.py:13-32: kappa / pyramid depth change, the A side does not).  args[0..n_jobs)
 * must share the A side (identical A, Ac, Ap, Apc pointers and n_a: one feature DB is built) and
 * every shape, channel count and mem kind; B, Bc, Bpc, Bp, weights, kappa_factor, outputs and debug
 * buffers are per job.  Every wavefront step gathers the queries of all jobs and runs ONE
 * distance scan over the DB for them (the DB is streamed once per step, not once per job), then
 * each job's coherence / kappa / writeback.  Results are those of n_jobs separate
 * ia_synthesize_level calls, bit for bit.  1 <= n_jobs <= 32.  Sharded levels take batches too
 * ("exchange" 0 / 1: every rank holds every job; emulated "exchange" = 2: one job per shard). */
int ia_synthesize_levels(ia_ctx *ctx, const ia_level_args *args, int n_jobs, ia_stats *stats);
/* The same call by k-coherence search: the level runs without a DB scan.  sim_k = K
 * in 1..min(IA_KCOH_MAX, N_A - 1), N_A = n_ap a_h a_w; sim is N_A x K int32 in the memory kind
 * args[0].mem names, like every pointer of the jobs: sim[j] = the K DB rows most similar to row j
 * (ia_index_similarity on the level's rows).  The sets belong to the A side, so one serves every job
 * of the batch.  Per pixel q = (r, c) in raster order the base rows are the shifted sources of its
 * causal neighbours (best_coherence_match's cells: rows r-2..r x cols c-2..c+2, raster-earlier,
 * source + q - r' inside A); the candidates are every base row b and sim[b][0..K); p_app = the
 * candidate with the smallest (exact fp64 distance in numpy's pairwise order, row index).
 * best_coherence_match, the kappa rule and the writeback are unchanged.  A pixel without a base row
 * (always the level's first) takes the exact NN over the whole DB and has no coherence candidate,
 * as on the exact path.  With K = N_A - 1 the level equals ia_synthesize_levels bit for bit;
 * otherwise it is NOT the reference's result.  sim_k = 0 (sim ignored) is ia_synthesize_levels.
 * (ia_level_args keeps its version-2 layout: the sets travel as arguments of their own.)
 * IA_EINVAL, before any step runs and with nothing written: sim_k outside 0..IA_KCOH_MAX or above
 * N_A - 1, sim NULL with sim_k > 0, a sim entry outside [0, N_A) (one pre-pass kernel), debug
 * buffers, a context that is a rank of a shard (ia_comm_init / ia_xchg_open with world > 1) or
 * emulates one ("shard_emulate" > 1), a context with "pipeline_record" = 1 or a pending
 * ia_pipeline_depend (which the refused call consumes). */
#define IA_KCOH_MAX 15
int ia_synthesize_levels_kcoh(ia_ctx *ctx, const ia_level_args *args, int n_jobs, const int32_t *sim, int sim_k,
                              ia_stats *stats);

/* The exact level for other window sizes: n_sm x n_sm coarse and n_lg x n_lg fine
 * neighbourhoods (config.py:15-16) given at run time.  With p_s = n_sm / 2, p_l = n_lg / 2, n_half =
 * n_lg^2 / 2 (integer divisions) and D = ch (2 n_sm^2 + n_lg^2 + n_half):
 *   DB row of pixel (r, c) of pair i = [A_i n_sm x n_sm at (r / 2, c / 2) of level l-1 | A_i n_lg x n_lg
 *     at (r, c) | A'_i n_sm x n_sm | A'_i first n_half cells of its n_lg x n_lg], each window row-major
 *     and channel-minor with symmetric padding (periodic where the image is smaller than the pad):
 *     compute_feature_array's row (algorithms.py:11-47); the query row likewise from B, B';
 *   NN = the smallest fp64 squared L2 in numpy's pairwise order, lowest row on ties;
 *   coherence = rows r - p_l .. r, columns c - p_l .. c + p_l in product order, raster-earlier cells
 *     whose shifted source lies inside A, ranked by the correctly rounded sqrt of the pairwise sum,
 *     first argmin (ia_coherence_batch's rule with pad = p_l);
 *   kappa rule = compute_distance with args[j].weights, which holds D values
 *     (config.compute_weights(n_sm, n_lg, n_half, ch)): x.dot(x) in the BLAS order of dbg_dist, the
 *     correctly rounded sqrt, y * y, and the kappa_ambiguous audit, as the default call does them;
 *   schedule t = col + (p_l + 1) row: every B' pixel a pixel reads in its causal half window or
 *     its coherence cells was written at an earlier step if raster-earlier and is written at a later
 *     step if raster-later (it still holds the initial B'), under reflection at every border.
 * Supported: n_sm in {1, 3, 5}, n_lg in {3, 5, 7, 9} (one coherence cell per lane: p_l <= 4), ch 1..3
 * and D <= 167 (the fp32 scan's widest instance).  (3, 5) is accepted and equals
 * ia_synthesize_levels bit for bit.  Batching (1 <= n_jobs <= 32), n_a and both mem kinds as there.
 * Image values need only be finite: the scan runs on a centred, prescaled fp32 copy, as the
 * index's does, so there is no +-64 gate.  The step is not fused, pruned or split-f16: gather,
 * query prep, fp32 scan over the whole DB, certified merge, finish.
 * IA_EINVAL before any step runs and with nothing written: unsupported sizes (checked before any
 * GPU call; the message names the sizes and D), debug buffers, a context that is a rank of a
 * shard or emulates one, a context with "pipeline_record" = 1 or a pending ia_pipeline_depend
 * (which the refused call consumes), a non-finite value on the A side. */
int ia_synthesize_levels_nbhd(ia_ctx *ctx, const ia_level_args *args, int n_jobs, int n_sm, int n_lg,
                              ia_stats *stats);

/* Masked resynthesis: redo the pixels of a mask and keep the rest of the level, exactly.
 * The jobs, sizes, batching and memory kinds are ia_synthesize_levels_nbhd's.  Per job j, in the memory
 * kind args[0].mem names (the three pointer arrays themselves are host arrays of n_jobs entries):
 *   mask[j]   N = b_h b_w bytes: nonzero = synthesise this pixel, zero = keep it;
 *   s_in[j]   N x 2 int32, im_in[j] N int32: the state of the kept pixels.  im_in < 0: the kept pixel has
 *             no source (a B' known in part, origin unknown): it is never a coherence candidate and its
 *             s_in is not read;
 *   args[j].Bp on entry: the complete B' level: the kept values, and anything at the masked pixels.
 * The masked pixels are visited in raster order, each by ia_synthesize_levels_nbhd's per-pixel rule on the
 * current state, with one change: a coherence cell is a candidate only if it is raster-earlier, its im >= 0
 * and its shifted source lies inside A.  Kept pixels are never written: their Bp values and s / im entries
 * come out bit-identical.  s_out / im_out are the complete maps (kept entries copied, masked entries
 * new); s_in[j] may be args[j].s_out, im_in[j] may be args[j].im_out.  A raster-later pixel a masked pixel
 * reads (through border reflection only: rows and columns below p_l) holds what Bp held on entry.
 * The schedule is t = col + (p_l + 1) row restricted to the masked pixels; only steps that hold one run.
 * An all-ones mask with every im_in = -1 is ia_synthesize_levels_nbhd bit for bit.  From the state a
 * finished ia_synthesize_levels_nbhd run of the same inputs left, any mask inside rows >= p_l and columns
 * >= p_l reproduces that state bit for bit.  A job whose mask is all zero is legal: its outputs are its
 * inputs.  A region's bottom and right borders are not matched against the kept pixels beyond them (the
 * window is causal), so seams there are possible.
 * ia_stats: pixels += masked pixels, steps += steps that held one, dist_launches += scans launched;
 * coherence_wins, kappa_ambiguous, db_ms and synth_ms as ia_synthesize_levels_nbhd; nbhd_levels is not
 * touched (ia_masked_stats counts these levels).
 * IA_EINVAL before any step runs and with nothing written: everything ia_synthesize_levels_nbhd refuses
 * (the message names this call), a NULL mask / s_in / im_in or a NULL entry, a pixel with im_in >= n_ap,
 * a pixel with im_in >= 0 whose s_in lies outside [0, a_h) x [0, a_w) (one pre-pass kernel over every
 * pixel, masked ones included), n_jobs b_h b_w >= 2^31. */
int ia_synthesize_levels_masked(ia_ctx *ctx, const ia_level_args *args, int n_jobs, int n_sm, int n_lg,
                                const uint8_t *const *mask, const int32_t *const *s_in,
                                const int32_t *const *im_in, ia_stats *stats);
/* Totals of the context's ia_synthesize_levels_masked calls since ia_init: *levels = levels (jobs) run,
 * *list_ms = device time of their step lists (count, scan and fill passes).  Either may be NULL.
 * (ia_stats keeps its layout: these counters travel on their own.) */
int ia_masked_stats(ia_ctx *ctx, int64_t *levels, double *list_ms);

/* Level pipelining: level l + 1 of a job only reads B' of level l near
 * (r / 2, c / 2), so its wavefront step t needs level l's steps <= t / 2 + 4, not the whole level.
 * Two contexts driven from two host threads run alternate levels concurrently: the context of
 * level l has option "pipeline_record" = 1 (its level calls are numbered 1, 2, ...: generations,
 * ia_pipeline_generation = the last one started) and before the level l + 1 call the other
 * context calls ia_pipeline_depend(ctx, prev_ctx, generation of level l): each of its steps then
 * waits (a stream event wait, no host sync) for the steps of level l it reads.  Results are those
 * of the sequential order, bit for bit.  A previous level that stops for 120 s makes the
 * dependent call fail with IA_ECOMM. */
int ia_pipeline_depend(ia_ctx *ctx, ia_ctx *prev, int prev_gen);
int ia_pipeline_generation(ia_ctx *ctx);

/* ---- FLANN-compatible exact index (algorithms.py:56,69,74) -------------------------------- */
/* build_index(pts): pts is n x d fp64 (row-major), d <= 167, every value and every column sum
 * finite (IA_EINVAL otherwise).  Any units: the fp32 scan works on a centred copy prescaled by a
 * power of two chosen from the rows, so the answers below are exact at 2^-80 as at 2^+70. */
int ia_index_build(ia_ctx *ctx, const double *pts, int64_t n, int d, ia_index **out);
/* nn_index(q, 1): exact 1-NN, squared L2 in fp64 with numpy's pairwise summation order,
 * lowest index on ties.  q is nq x d fp64; idx_out (nq) int64, dist_out (nq) fp64 (may be NULL).
 * IA_EINVAL (nothing written) when a query value is not finite or lies farther from its column's
 * mean than 2^100 times the largest such distance of any row value. */
int ia_index_query(ia_index *index, const double *q, int64_t nq, int64_t *idx_out, double *dist_out);
/* nn_index(q, k): exact k-NN under the same distance.  Row j of idx_out (nq x k int64) and dist_out
 * (nq x k fp64, may be NULL) holds the k rows with the smallest (distance, row index) pairs in
 * ascending (distance, index) order: ties, also across the k-th place, go to the lower index.
 * k = 1 returns what ia_index_query returns, bit for bit.  1 <= k <= min(n, IA_KNN_MAX); the
 * merge keeps one list entry per lane of a wave, so 64 is the design's limit, not a tunable.
 * IA_EINVAL (nothing written) for k outside that range, a NULL index / q / idx_out, nq < 0 (all
 * checked before any GPU call) and for a query ia_index_query refuses.  The scan is
 * ia_index_query's; only rows its records cannot rule out are computed in fp64. */
#define IA_KNN_MAX 64
int ia_index_query_knn(ia_index *index, const double *q, int64_t nq, int k, int64_t *idx_out,
                       double *dist_out);
/* Work of the last ia_index_query_knn call that ran on this index: out[0] = rows whose exact fp64
 * distance was computed (reranked candidates + rows of rescanned chunks; a brute force computes
 * nq x n), out[1] = scan chunks rescanned exactly. */
int ia_index_knn_stats(const ia_index *index, int64_t out[2]);
/* Similarity sets of the index's own rows (k-coherence search, ia_synthesize_levels_kcoh): for row j the
 * K + 1 nearest rows under ia_index_query_knn's order, the entry equal to j deleted if present,
 * the first K of what remains.  Duplicates of row j with lower indices come before j and stay.
 * The queries are the rows the index holds on the device, in ia_index_query_knn's batches and
 * workspace.  sim_out: n x K int32, host memory.  IA_EINVAL (nothing written) for K outside
 * 1..min(IA_KCOH_MAX, n - 1) or a NULL argument. */
int ia_index_similarity(ia_index *index, int K, int32_t *sim_out);
/* nn_radius(q, radius): exact fixed-radius search under the same distance (pyflann's radius is a
 * squared distance too).  radius holds nq values, one per query, each >= 0 and not NaN; +inf means
 * every row.  A row is inside when dist < radius, strictly: radius 0 returns nothing, even for an
 * exact hit.  count_out[j] (required by both calls) is the exact number of rows inside query j's
 * radius.
 * The counting call returns only that; it verifies in fp64 just the rows whose fp32 scan value
 * lies within the scan's error bound of the radius, every other row is decided by the scan.
 * The query call writes rows as the caller lays them out: offsets holds nq + 1 non-decreasing
 * values, offsets[0] >= 0, and query j owns slots [offsets[j], offsets[j + 1]) of idx_out (int64)
 * and dist_out (fp64, may be NULL).  They receive the min(capacity, count) nearest rows inside the
 * radius in ascending (distance, index) order, ties to the lower index; unused slots get index -1
 * and distance +inf.  offsets[j] = j * max_nn is a fixed width; the running sum of a counting call's
 * result is the exact CSR layout.
 * IA_EINVAL with nothing written, checked before any GPU call, for a NULL index / q / radius /
 * count_out / offsets, nq < 0, a negative or NaN radius, offsets that decrease or start below 0, a
 * NULL idx_out with a non-empty layout, and a query the 1-NN call refuses. */
int ia_index_count_radius(ia_index *index, const double *q, int64_t nq, const double *radius,
                          int64_t *count_out);
int ia_index_query_radius(ia_index *index, const double *q, int64_t nq, const double *radius,
                          const int64_t *offsets, int64_t *idx_out, double *dist_out, int64_t *count_out);
/* Caps the candidate entries (12 bytes each) a radius call keeps on the device per fill pass: a
 * batch whose candidates exceed it is filled in sub-batches of consecutive queries.  0 restores
 * the default, 2^23 entries.  Raised silently to the padded row count (n rounded up to 32), so one
 * query always fits; the buffers grow to what a call needs, not to the cap. */
int ia_index_set_workspace(ia_index *index, int64_t entries);
/* Work of the last radius call (counting or query) that ran on this index: out[0] = (query, row)
 * pairs whose exact fp64 distance was computed, out[1] = rows found inside their radius (the sum
 * of count_out), out[2] = fill sub-batches, out[3] = query segments longer than 4,096 candidates,
 * sorted in global memory instead of LDS. */
int ia_index_radius_stats(const ia_index *index, int64_t out[4]);
void ia_index_destroy(ia_index *index);
/* best_coherence_match (algorithms.py:92-130) for nq B' pixels against the index's rows (the
 * As of create_index, algorithms.py:63-67), one call per batch instead of one per pixel.
 * q: nq x d fp64 query features (BBp_feat); px: nq x 2 int32 (row, col) of each pixel in the
 * B' level of width bp_w; s (n_s x 2 int32) / im (n_s) the raster-order source map of that
 * level, which must hold every causal neighbour of every pixel of the batch (s[r], im[r] for
 * the raster-earlier r in rows row-pad..row, cols col-pad..col+pad); a_h, a_w: A's level
 * shape (DB row = Ap_px2ix(p, im, a_h, a_w), img_preprocess.py:104-106); pad = c.pad_lg (2).
 * Out per pixel: p_out (row, col) = s[r*] + px - r*, img_out = im[r*], rstar_out = r*; or
 * (-1, -1), 0, (0, 0) without a candidate.  Candidates are ranked by sqrt of numpy's pairwise
 * sum of squares, first argmin (np.argmin of norm(..., axis=1)).  IA_EINVAL when a neighbour
 * index reaches beyond n_s or a candidate row beyond the index (an IndexError there). */
int ia_coherence_batch(ia_index *index, const double *q, int64_t nq, const int32_t *px,
                       const int32_t *s, const int32_t *im, int64_t n_s, int a_h, int a_w,
                       int bp_w, int pad, int32_t *p_out, int32_t *img_out, int32_t *rstar_out);

/* ---- approximate index: k-means lists that honour `checks` ------------------ */
/* A deterministic inverted file.  dist(a, b) is ia_index_*'s exact distance (fp64, numpy's pairwise
 * order).  k-means over n rows of width d with L lists: centre c starts as row floor(c n / L);
 * assign gives every row the centre of smallest (dist, centre index); update makes a centre the
 * sum of its rows, added one by one in ascending row order, over their count (a centre without
 * rows keeps its value); at most `iters` rounds of assign + update, stopping early when an
 * assignment repeats; a last assign, so the lists always belong to the returned centres.  List c =
 * the rows assigned to c in ascending row order (it may be empty).
 * A query orders the centres by ascending (dist(centre, q), centre index) and takes lists whole, in
 * that order, while fewer than `need` rows are taken: need = n for checks = -1, else
 * min(n, max(checks, k)).  The answer is the k taken rows of smallest (dist, row index), ascending
 * (ia_index_query_knn's order); checks = -1 or >= n is ia_index_query_knn's result bit for bit.
 * Limits: 1 <= n_lists <= min(n, IA_ANN_MAX_LISTS), d <= 167, 1 <= k <= min(n, IA_KNN_MAX),
 * checks = -1 or >= 1, iters >= 0, n < 2^31, every row and query value finite and at most
 * IA_ANN_MAX_ABS = 2^500 in magnitude (no squared distance overflows).  Anything else is IA_EINVAL before
 * any GPU call with nothing written; nq = 0 is IA_OK.  Not FLANN's randomised trees, and not the
 * reference's result: an opt-in mode. */
#define IA_ANN_MAX_LISTS 4096
#define IA_ANN_MAX_ABS 0x1p500
typedef struct ia_ann ia_ann;
/* Lloyd's k-means by the rule above.  centers_out: k x d fp64; assign_out: n int32 (may be NULL);
 * iters_run: the updates made (may be NULL).  Host memory. */
int ia_kmeans(ia_ctx *ctx, const double *pts, int64_t n, int d, int k, int iters,
              double *centers_out, int32_t *assign_out, int *iters_run);
int ia_ann_build(ia_ctx *ctx, const double *pts, int64_t n, int d, int n_lists, int iters, ia_ann **out);
/* centers_out L x d, sizes_out L int64, rows_out n int32 (list after list, each ascending); any may be NULL */
int ia_ann_lists(const ia_ann *a, double *centers_out, int64_t *sizes_out, int32_t *rows_out);
/* idx_out nq x k int64, dist_out nq x k fp64 (may be NULL) */
int ia_ann_query(ia_ann *a, const double *q, int64_t nq, int k, int checks, int64_t *idx_out, double *dist_out);
/* of the last ia_ann_query on this index, summed over its queries: rows whose distance was computed,
 * lists probed (empty ones included); and the k-means iterations of the build */
int ia_ann_stats(const ia_ann *a, int64_t out[3]);
/* host-clock milliseconds of the build's phases, summed over its iterations: assign (with the
 * read-back), grouping (host counting sort and upload), update, the list-major copy */
int ia_ann_build_ms(const ia_ann *a, double out[4]);
void ia_ann_destroy(ia_ann *a);

/* ---- GPU preprocessing (img_setup, image_analogies.py:17-94) -------------------- */
/* n_reduce steps of skimage 0.18.3 pyramid_reduce (img_preprocess.py:47-63): scipy.ndimage
 * gaussian_filter (sigma 2/3, mode 'reflect', 7 taps: weights7 = scipy's kernel, symmetric;
 * axes 0 and 1, a colour axis unsmoothed) + order-1 resize to ceil(h/2) x ceil(w/2) clipped to
 * the smoothed image's range.  img (h, w, ch) fp64; out = the n_reduce reduced levels, finest
 * first, concatenated.  Bit-identical to ia_amd.img_preprocess.compute_gaussian_pyramid.
 * mem selects host or device memory for img and out; weights7 is ALWAYS a host array (its
 * four distinct taps travel in the kernel arguments). */
int ia_gaussian_pyramid(ia_ctx *ctx, const double *img, int h, int w, int ch, int n_reduce,
                        const double *weights7, double *out, int mem);
/* out[p, i] = sum_j M9[3 i + j] in[p, j] for npx pixels of 3 channels, in numpy's
 * einsum('ij,klj->kli') order (m0 x0 + m2 x2) + m1 x1 (convert_to_YIQ / convert_to_RGB,
 * img_preprocess.py:6-22).  mem selects host or device memory for in and out; M9 is ALWAYS a
 * host array (copied to the device per call). */
int ia_color_matrix(ia_ctx *ctx, const double *in, int64_t npx, const double *M9, double *out,
                    int mem);

/* ---- kernel tuning ------------------------------------------------------------------------- */
/* Time the split-f16 distance scan (K3h, current "k3_variant") alone: n_rows random DB rows
 * (1 channel), M <= 352 random queries, `reps` back-to-back launches on the context's stream;
 * *us_per_launch = mean device time per launch (HIP events). */
int ia_k3_microbench(ia_ctx *ctx, int64_t n_rows, int M, int reps, double *us_per_launch);

/* ---- host-side helpers (no GPU needed) ---------------------------------------------------- */
/* Merge per-rank candidate winners (dist fp64, global row) into the global winner per query:
 * smallest distance, then smallest row.  cand is world x nq (dist, row) pairs, rank-major. */
int ia_merge_winners(const double *dist, const int64_t *row, int world, int64_t nq,
                     double *dist_out, int64_t *row_out);
/* Budget of handoff-chained waves (fused merge + gather launches whose waves wait for the row
 * above) a context may have in flight deadlock-free: 2 x the resident waves of its n_cu CUs, less
 * 1/16, from the compiled kernel's VGPRs per lane, the occupancy API's workgroups per CU and its
 * workgroup size; 0 = never chain.  ia_init computes it from k_merge_gather itself. */
int ia_chain_budget(int n_cu, int vgprs, int api_blocks_per_cu, int wg_threads);
/* What a level takes of that budget.  level_waves: the one-wave workgroups of its widest fused
 * launch; in_flight: waves already reserved in the process; two_wave: the level qualifies for
 * option "gather_wave".  Returns 2 (two-wave workgroups, 2 x level_waves reserved: they fit in
 * budget - in_flight), 1 (one-wave workgroups, level_waves reserved) or 0 (neither fits, or no
 * budget: separate merge and gather launches, nothing reserved). */
int ia_chain_choice(int level_waves, int in_flight, int budget, int two_wave);
/* Wavefront schedule of a level (t = col + 3*row): number of steps and max queries per step. */
int ia_wavefront_shape(int h, int w, int64_t *steps, int64_t *max_queries);
/* Pixels of step t: rows r0 .. r0+M-1, pixel (r, t - 3r).  Used by the level driver. */
int ia_wavefront_step(int h, int w, int64_t t, int *r0, int *M);
/* The same two for the schedule t = col + (pad + 1) row of ia_synthesize_levels_nbhd (pad = n_lg / 2,
 * 0..4): steps = w + (pad + 1)(h - 1), max_queries = min(h, ceil(w / (pad + 1))); step t holds the
 * pixels (r, t - (pad + 1) r), r0 <= r < r0 + M (M = 0: none, on levels narrower than pad + 1).
 * pad = 2 gives what ia_wavefront_shape / ia_wavefront_step give. */
int ia_wavefront_shape_pad(int h, int w, int pad, int64_t *steps, int64_t *max_queries);
int ia_wavefront_step_pad(int h, int w, int pad, int64_t t, int *r0, int *M);
/* The compaction rule of ia_synthesize_levels_masked for one job: the masked pixels (mask: h w bytes,
 * nonzero = masked) of every step of that schedule, T = w + (pad + 1)(h - 1) steps.  offsets has T + 1
 * entries; pixels[offsets[t] .. offsets[t + 1]) are the masked raster indices of step t, rows ascending;
 * offsets[T] = the mask's count, which pixels must hold (pixels = NULL: offsets only). */
int ia_masked_step_list(int h, int w, int pad, const uint8_t *mask, int32_t *offsets, int32_t *pixels);
/* DB tiles [tile0, tile1) owned by `rank` of `world` for a level of n_rows DB rows.  The DB is
 * stored in NT = ceil(n_rows/32) tiles of 32 positions; position j of tile t holds row
 * j*NT + (t * (2654435761 mod NT) mod NT) (tile-strided and tile-scattered, so neighbouring A
 * pixels sit in far-apart tiles).  Tiles are split contiguously over ranks; levels under
 * 64*world tiles are not sharded (every rank owns every tile). */
int ia_shard_tiles(int64_t n_rows, int world, int rank, int64_t *tile0, int64_t *tile1);
/* Pruned levels (certified pruned scan) shard differently: every rank holds the whole
 * Morton-sorted DB, stored shard by shard; shard r = Morton tiles r, r + world, r + 2 world, ...
 * (each covers the whole feature space: balanced pruned work), stored as storage tiles
 * [tile0, tile1).  ia_shard_morton_tile gives the Morton tile of a storage tile. */
int ia_shard_tiles_pruned(int64_t n_rows, int world, int rank, int64_t *tile0, int64_t *tile1);
int64_t ia_shard_morton_tile(int64_t storage_tile, int64_t n_tiles, int world);

#ifdef __cplusplus
}
#endif
#endif /* IA_H_ */

"""Time k-coherence search against the exact path on synth.make_job(size), in
one process on one context, levels run one after the other (no level pipelining: k-coherence levels
take none).  Three things, reported separately:

  * the similarity sets: per level with at least --min-rows DB rows, the host clock around
    ExactIndex.similarity(max K) (a synchronous call; the index build, an upload of the rows, beside
    it).  The sets of a smaller K are the first K columns of a larger K's;
  * the pyramid: the exact path and K = each of --ks, alternated round by round after one warm-up
    round; per level the host clock around the synchronous level call (uploads and read-backs of
    host arrays included) and the device time between the level's events (ia_stats.synth_ms and
    db_ms); the median over the rounds and the spread;
  * how often k-coherence's p_app is the exact NN: teacher forcing on --samples raster pixels of the
    finest level, drawn with a seed, on the K run's own final state (oracle state_at /
    query_feature); p_app from the rule in numpy, the exact NN from the oracle's nn_exact up to 2^16
    DB rows and from the GPU index (pinned to nn_exact by tests/test_gpu_knn.py) above.

Prints one JSON line.
  python3 tools/kcoh_timing.py [--size 1024] [--ks 2,4,8] [--rounds 3] [--samples 400] [--min-rows 1024]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ia_amd  # noqa: F401,E402
from ia_amd import _native, algorithms, config, synth  # noqa: E402
from oracle import ia_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=1024)
ap.add_argument('--ks', default='2,4,8')
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--samples', type=int, default=400)
ap.add_argument('--min-rows', type=int, default=1024)
a = ap.parse_args()
KS = [int(x) for x in a.ks.split(',')]

job = synth.make_job(a.size)
L = job.L
ctx = _native.Context(0)
c = types.SimpleNamespace(n_sm=config.n_sm, n_lg=config.n_lg, n_half=config.n_half, max_levels=L, kcoh_k=max(KS),
                          kcoh_min_rows=a.min_rows)

# ---- the similarity sets, per level -----------------------------------------------------------------------
sim_max, sim_report, rows_of = {}, {}, {}
for level in range(1, L):
    n = len(job.Ap_pyr_list) * int(np.prod(job.Ap_pyr_list[0][level].shape[:2]))
    if n < max(2, a.min_rows):
        continue
    t0 = time.perf_counter()
    rows = algorithms.level_rows(job.A_pyr, job.Ap_pyr_list, c, level)
    t1 = time.perf_counter()
    index = _native.ExactIndex(ctx, rows)
    t2 = time.perf_counter()
    sim_max[level] = index.similarity(min(max(KS), n - 1))
    t3 = time.perf_counter()
    index.close()
    rows_of[level] = rows
    sim_report[level] = dict(rows=n, K=int(sim_max[level].shape[1]), host_rows_ms=round(1e3 * (t1 - t0), 1),
                             index_build_ms=round(1e3 * (t2 - t1), 1), similarity_ms=round(1e3 * (t3 - t2), 1))
    print('level %d: %s' % (level, sim_report[level]), file=sys.stderr, flush=True)
    if level != L - 1:
        del rows_of[level]


def sims_for(K):
    return {level: np.ascontiguousarray(s[:, :min(K, s.shape[1])]) for level, s in sim_max.items()}


# ---- the pyramid ------------------------------------------------------------------------------------------
def run(sims):
    """one pyramid; ({level: (wall ms, device synth ms, device DB ms)}, B' pyramid, S, IM, Stats)"""
    Bp = [x.copy() for x in job.Bp_init]
    st = _native.Stats()
    per, S, IM = {}, {}, {}
    for level in range(1, L):
        Bp[level] = np.ascontiguousarray(Bp[level], dtype=np.float64)
        syn0, db0 = st.synth_ms, st.db_ms
        t0 = time.perf_counter()
        S[level], IM[level] = ctx.synthesize_level(job.A_levels(level), job.A_levels(level - 1), [p[level] for p in job.Ap_pyr_list],
                                                   [p[level - 1] for p in job.Ap_pyr_list], job.B_pyr[level], job.B_pyr[level - 1],
                                                   Bp[level - 1], Bp[level], job.weights, job.kappa_factor(level), st,
                                                   sim=sims.get(level))
        per[level] = (1e3 * (time.perf_counter() - t0), st.synth_ms - syn0, st.db_ms - db0)
    return per, Bp, S, IM, st


variants = [('exact', {})] + [('K%d' % K, sims_for(K)) for K in KS]
final = {}
for name, sims in variants:      # warm every shape
    run(sims)
times = {name: [] for name, _ in variants}
for _ in range(a.rounds):
    for name, sims in variants:
        per, Bp, S, IM, st = run(sims)
        times[name].append(per)
        final[name] = (Bp, S, IM, st)


def summary(rounds):
    med = lambda xs: round(float(np.median(xs)), 3)
    fin = L - 1
    tot = lambda k: [sum(p[level][k] for level in p) for p in rounds]
    return dict(finest_wall_ms=med([p[fin][0] for p in rounds]), finest_synth_ms=med([p[fin][1] for p in rounds]),
                finest_synth_ms_min_max=[round(min(p[fin][1] for p in rounds), 3), round(max(p[fin][1] for p in rounds), 3)],
                finest_db_ms=med([p[fin][2] for p in rounds]),
                pyramid_wall_ms=med(tot(0)), pyramid_synth_ms=med(tot(1)), pyramid_db_ms=med(tot(2)),
                pyramid_synth_ms_min_max=[round(min(tot(1)), 3), round(max(tot(1)), 3)])


report = {name: summary(times[name]) for name, _ in variants}
for name, _ in variants:
    st = final[name][3]
    report[name].update(steps=int(st.steps), kcoh_levels=int(st.kcoh_levels), kcoh_fallbacks=int(st.kcoh_fallbacks),
                        kcoh_candidates=int(st.kcoh_candidates), coherence_wins=int(st.coherence_wins), pixels=int(st.pixels))
    if name != 'exact':
        fin = L - 1
        report[name]['finest_pixels_equal_to_exact'] = round(
            float((final[name][1][fin] == final['exact'][1][fin]).all(axis=1).mean()), 4)

# ---- p_app = exact NN?  teacher forcing on the finest level -----------------------------------------------
fin = L - 1
if fin in sim_max and a.samples > 0:
    As = rows_of[fin]
    A_h, A_w = job.Ap_pyr_list[0][fin].shape[:2]
    B_feat = O.feature_array(job.B_pyr, fin, True)
    h, w = job.B_pyr[fin].shape[:2]
    picks = np.sort(np.random.RandomState(5).choice(np.arange(1, h * w), size=min(a.samples, h * w - 1), replace=False))
    index = _native.ExactIndex(ctx, As) if len(As) > (1 << 16) else None
    for K in KS:
        Bp, S, IM, _ = final['K%d' % K]
        sim = sim_max[fin][:, :K]
        s, im = S[fin].astype(np.int64), IM[fin].astype(np.int64)
        qs, papp, nobase = [], [], 0
        for qi in picks:
            r, col = divmod(int(qi), w)
            q = O.query_feature(B_feat, Bp[fin - 1], O.state_at(Bp[fin], job.Bp_init[fin], qi), r, col, w)
            base = []
            for rr in range(max(0, r - 2), r + 1):
                for rc in range(max(0, col - 2), min(w, col + 3)):
                    ri = rr * w + rc
                    if ri < qi:
                        pr, pc = s[ri, 0] + r - rr, s[ri, 1] + col - rc
                        if 0 <= pr < A_h and 0 <= pc < A_w:
                            base.append(int((A_h * im[ri] + pr) * A_w + pc))
            if not base:
                nobase += 1
                continue
            rows = np.array([x for b in base for x in [b] + [int(v) for v in sim[b]]], dtype=np.int64)
            d = ((As[rows] - q) ** 2).sum(axis=1)
            papp.append(int(rows[np.lexsort((rows, d))[0]]))
            qs.append(q)
        qs = np.array(qs)
        exact = index.query(qs)[0] if index is not None else np.array([O.nn_exact(As, q)[0] for q in qs])
        report['K%d' % K].update(teacher_forced_pixels=len(papp), teacher_forced_without_base=nobase,
                                 p_app_is_exact_nn=round(float((np.array(papp) == exact).mean()), 4))
    if index is not None:
        index.close()
ctx.close()
print(json.dumps({'size': a.size, 'levels': L, 'rounds': a.rounds, 'min_rows': a.min_rows, 'similarity': sim_report,
                  'runs': report}), flush=True)

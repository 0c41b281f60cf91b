"""Time the approximate index on the finest-level DB rows of synth.make_job(size), in one
process on one context, against the exact index on the same rows and queries.  Reported separately, per row
count of --rows (the finest level's rows, thinned by a stride to the smaller counts):

  * the build: the host clock around AnnIndex(...) (a synchronous call: upload, k-means, list-major copy),
    and inside it ia_ann_build_ms's split into assign (with its read-back), grouping (the host counting sort
    and its upload), update and the list-major copy; medians of --rounds builds after one warm-up build,
    with the spread;
  * the queries: --nq queries at each checks of --checks and k of --ks, alternated with
    ExactIndex.query_knn on the same queries round by round after one warm-up round; the host clock around the
    synchronous calls (uploads and read-backs included); medians and spread.  checks = 1 probes one list: what
    it costs is the centre distances and the sort, the rest of a larger checks is the row stream;
  * quality per checks at k = 1: the share of queries whose neighbour is the exact one, the mean ratio of the
    returned distance to the exact one (over queries whose exact distance is not 0), rows taken and lists probed
    per query.
Two query sets: rows of the job's B-side features ([B full | B' half] at the B' initial state), and uniform
random vectors in the rows' bounding box.

Prints one JSON line.
  python3 tools/ann_timing.py [--size 1024] [--rows 65536,1048576] [--lists 0] [--iters 5] [--nq 4096] [--rounds 3]"""
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

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=1024)
ap.add_argument('--rows', default='65536,1048576')
ap.add_argument('--lists', type=int, default=0, help='0: the default, isqrt(n)')
ap.add_argument('--iters', type=int, default=5)
ap.add_argument('--nq', type=int, default=4096)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--checks', default='1,32,1024,4096,-1')
ap.add_argument('--ks', default='1,5')
a = ap.parse_args()
CHECKS = [int(x) for x in a.checks.split(',')]
KS = [int(x) for x in a.ks.split(',')]

job = synth.make_job(a.size)
fin = job.L - 1
c = types.SimpleNamespace(n_sm=config.n_sm, n_lg=config.n_lg, n_half=config.n_half, max_levels=job.L)
rows_all = np.ascontiguousarray(algorithms.level_rows(job.A_pyr, job.Ap_pyr_list, c, fin))
b_rows = algorithms.level_rows(job.B_pyr, [job.Bp_init], c, fin)
rs = np.random.RandomState(31)
q_bside = np.ascontiguousarray(b_rows[rs.choice(len(b_rows), a.nq, replace=False)])
lo, hi = rows_all.min(axis=0), rows_all.max(axis=0)
q_uniform = lo + (hi - lo) * rs.rand(a.nq, rows_all.shape[1])
ctx = _native.Context(0)


def med(xs):
    return dict(median=round(float(np.median(xs)), 3), min=round(float(min(xs)), 3), max=round(float(max(xs)), 3))


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), r


report = {}
for n in [int(x) for x in a.rows.split(',')]:
    stride = max(1, len(rows_all) // n)
    pts = np.ascontiguousarray(rows_all[::stride][:n])
    n_lists = a.lists or None
    _native.AnnIndex(ctx, pts, n_lists, a.iters).close()      # warm-up
    wall, phases, index = [], [], None
    for _ in range(a.rounds):
        if index is not None:
            index.close()
        ms, index = clock(lambda: _native.AnnIndex(ctx, pts, n_lists, a.iters))
        wall.append(ms)
        phases.append(index.build_ms())
    sizes = index.lists()[1]
    run = index.stats()[2]
    ex_ms, exact = clock(lambda: _native.ExactIndex(ctx, pts))
    rep = dict(rows=len(pts), lists=index.n_lists, iterations_run=run, assigns=run + 1, build_wall_ms=med(wall),
               exact_index_build_wall_ms=round(ex_ms, 3),
               list_sizes=dict(min=int(sizes.min()), max=int(sizes.max()), empty=int((sizes == 0).sum())))
    for j, name in enumerate(('assign_ms', 'grouping_ms', 'update_ms', 'list_major_copy_ms')):
        rep[name] = med([p[j] for p in phases])
    print('n=%d build: %s' % (n, rep), file=sys.stderr, flush=True)
    for qname, Q in (('bside', q_bside), ('uniform', q_uniform)):
        qrep = {}
        for k in KS:
            exact.query_knn(Q, k)                              # warm-up round
            for ch in CHECKS:
                index.query(Q, k, ch)
            t_exact, t_ann = [], {ch: [] for ch in CHECKS}
            for _ in range(a.rounds):
                t_exact.append(clock(lambda: exact.query_knn(Q, k))[0])
                for ch in CHECKS:
                    t_ann[ch].append(clock(lambda: index.query(Q, k, ch))[0])
            qrep['k%d' % k] = dict(exact_ms=med(t_exact), **{'checks_%d_ms' % ch: med(t_ann[ch]) for ch in CHECKS})
        i_ex, d_ex = exact.query_knn(Q, 1)
        qual = {}
        for ch in CHECKS:
            idx, dist = index.query(Q, 1, ch)
            taken, probed, _ = index.stats()
            pos = d_ex[:, 0] > 0
            qual['checks_%d' % ch] = dict(first_is_exact=round(float((idx[:, 0] == i_ex[:, 0]).mean()), 4),
                                          mean_dist_ratio=round(float((dist[pos, 0] / d_ex[pos, 0]).mean()), 4),
                                          rows_per_query=round(taken / len(Q), 1), lists_per_query=round(probed / len(Q), 2))
        qrep['quality_k1'] = qual
        rep[qname] = qrep
        print('n=%d %s: %s' % (n, qname, qrep), file=sys.stderr, flush=True)
    index.close()
    exact.close()
    report['n%d' % len(pts)] = rep
ctx.close()
print(json.dumps({'size': a.size, 'nq': a.nq, 'rounds': a.rounds, 'iters': a.iters, 'runs': report}), flush=True)

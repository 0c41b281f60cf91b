"""Time the index's exact k-NN against its 1-NN on one shape: 2^20 seeded rows x 55 columns, one batch
of 4,096 queries (no files needed).  In one process, the calls alternated round by round:
ia_index_query (the baseline) and ia_index_query_knn at k = 1, 8 and 64.  Each variant is warmed, then
timed with a host clock around the synchronous call until every variant has at least a second.
Prints one JSON line: ms per batch (median over the rounds), the spread (min, max), and knn_stats
per query (exact rows computed, chunks rescanned).
  python3 tools/knn_micro.py [--n 1048576] [--nq 4096] [--seconds 1.0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ia_amd  # noqa: F401,E402
from ia_amd import _native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=1 << 20)
ap.add_argument('--nq', type=int, default=4096)
ap.add_argument('--d', type=int, default=55)
ap.add_argument('--seconds', type=float, default=1.0)
a = ap.parse_args()

rs = np.random.RandomState(2024)
pts, q = rs.rand(a.n, a.d), rs.rand(a.nq, a.d)
ctx = _native.Context(0)
index = _native.ExactIndex(ctx, pts)
variants = [('query', lambda: index.query(q))] + [('knn%d' % k, lambda k=k: index.query_knn(q, k)) for k in (1, 8, 64)]
stats = {}
for name, fn in variants:   # warm every shape (buffers, code objects)
    for _ in range(2):
        fn()
    if name != 'query':
        stats[name] = [round(x / float(a.nq), 3) for x in index.knn_stats()]
i1 = index.query(q)[0]
assert np.array_equal(index.query_knn(q, 1)[0][:, 0], i1) and np.array_equal(index.query_knn(q, 8)[0][:, 0], i1)
ms = {name: [] for name, _ in variants}
while min(sum(v) for v in ms.values()) < 1e3 * a.seconds:
    for name, fn in variants:
        t0 = time.perf_counter()
        fn()
        ms[name].append(1e3 * (time.perf_counter() - t0))
index.close()
ctx.close()
print(json.dumps({'n': a.n, 'd': a.d, 'nq': a.nq, 'rounds': len(ms['query']),
                  'ms': {k: round(float(np.median(v)), 3) for k, v in ms.items()},
                  'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                  'knn_stats_per_query': stats}), flush=True)

"""Time the index's exact fixed-radius search against its 1-NN on one shape: 2^20 seeded rows x 55
columns, one batch of 4,096 queries (no files needed).  In one process, the calls alternated round by
round: ia_index_query (the baseline), then for each of two radius sets count_radius, query_radius with
max_nn = 64 and query_radius in the CSR form (a counting call, then the query).  The radius sets:
  r16    per query the midpoint of its 16th and 17th neighbour's distance, from query_knn(q, 17)
  r1000  one global radius holding on the order of 1,000 rows per query: the 1000 / n quantile of the
         distances between the queries and a 4,096-row sample
Each variant is warmed, then timed with a host clock around the synchronous call until every variant
has at least a second.  Prints one JSON line: ms per batch (median over the rounds), the spread (min,
max), and radius_stats per query (pairs verified in fp64, rows inside, fill sub-batches and globally
sorted segments per call).
  python3 tools/radius_micro.py [--n 1048576] [--nq 4096] [--seconds 1.0] [--out FILE]"""
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
ap.add_argument('--out', default=None, help='also write the JSON line to this file')
a = ap.parse_args()

rs = np.random.RandomState(2024)
pts, q = rs.rand(a.n, a.d), rs.rand(a.nq, a.d)
ctx = _native.Context(0)
index = _native.ExactIndex(ctx, pts)
d17 = index.query_knn(q, 17)[1]
sample = pts[rs.choice(a.n, 4096, replace=False)]
dd = (q ** 2).sum(1)[:, None] - 2.0 * q.dot(sample.T) + (sample ** 2).sum(1)[None, :]
radii = {'r16': (d17[:, 15] + d17[:, 16]) / 2, 'r1000': np.full(a.nq, np.quantile(dd, min(1.0, 1000.0 / a.n)))}
variants = [('query', lambda: index.query(q))]
for tag, r in radii.items():
    variants += [('count_' + tag, lambda r=r: index.count_radius(q, r)),
                 ('query64_' + tag, lambda r=r: index.query_radius(q, r, 64)),
                 ('csr_' + tag, lambda r=r: index.query_radius(q, r))]
stats = {}
for name, fn in variants:   # warm every shape (buffers, code objects)
    for _ in range(2):
        fn()
    if name != 'query':
        s = index.radius_stats()
        stats[name] = [round(s[0] / float(a.nq), 3), round(s[1] / float(a.nq), 3), s[2], s[3]]
assert (index.count_radius(q, radii['r16']) == 16).all()
ms = {name: [] for name, _ in variants}
while min(sum(v) for v in ms.values()) < 1e3 * a.seconds:
    for name, fn in variants:
        t0 = time.perf_counter()
        fn()
        ms[name].append(1e3 * (time.perf_counter() - t0))
index.close()
ctx.close()
line = json.dumps({'n': a.n, 'd': a.d, 'nq': a.nq, 'rounds': len(ms['query']), 'r1000': float(radii['r1000'][0]),
                   'ms': {k: round(float(np.median(v)), 3) for k, v in ms.items()},
                   'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                   'radius_stats_per_query': stats})
print(line, flush=True)
if a.out:
    with open(a.out, 'w') as f:
        f.write(line + '\n')

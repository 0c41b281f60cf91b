"""The approximate index's rule (include/ia.h ia_kmeans / ia_ann_*) restated in numpy, and
the cases tests/test_gpu_ann.py compares with it bit for bit.  Pure numpy, no GPU import; every generator is
seeded.  tests/test_ann_cpu.py pins, without a GPU, that each case is what it claims to be.

dist(a, b) = ((a - b) ** 2).sum() in fp64, numpy's pairwise order (knn_inputs.knn_reference's distance).
"""
import functools

import numpy as np

ANN_MAX_LISTS = 4096   # IA_ANN_MAX_LISTS
CHECKS_LADDER = (1, 32, 256, 1024, 20000, -1)
DUPS_K, DUPS_CHECKS = 3, (1, 33, 64, 200)   # checks = 1 stays inside the first list; the others cross empty lists
K_QUERY = (1, 5, 64)


def assign_ref(pts, C):
    """per row the centre of smallest (dist, centre index): argmin returns the first minimum"""
    D = np.empty((len(pts), len(C)))
    for c in range(len(C)):
        D[:, c] = ((pts - C[c]) ** 2).sum(axis=1)
    return D.argmin(axis=1).astype(np.int32)


def assign_per_row(pts, C):
    """the same by the rule's words, one row at a time: lexsort on (dist, centre index)"""
    a = np.empty(len(pts), dtype=np.int32)
    for i in range(len(pts)):
        dd = ((C - pts[i]) ** 2).sum(axis=1)
        a[i] = np.lexsort((np.arange(len(C)), dd))[0]
    return a


def update_ref(pts, C, a):
    C = C.copy()
    for c in range(len(C)):
        rows = np.flatnonzero(a == c)
        if len(rows):
            C[c] = np.add.accumulate(pts[rows], axis=0)[-1] / len(rows)
    return C


def kmeans_ref(pts, L, iters):
    """(centres (L, d), assign (n,) int32, iterations run)"""
    n = len(pts)
    C = pts[[c * n // L for c in range(L)]].copy()
    prev, run = None, 0
    for _ in range(iters):
        a = assign_ref(pts, C)
        if prev is not None and np.array_equal(a, prev):
            break
        C = update_ref(pts, C, a)
        prev = a
        run += 1
    return C, assign_ref(pts, C), run


def lists_ref(a, L):
    """(sizes (L,) int64, rows (n,) int32: list after list, each in ascending row order)"""
    rows = np.argsort(a, kind='stable').astype(np.int32)
    return np.bincount(a, minlength=L).astype(np.int64), rows


def probe_order(C, sizes, q, need):
    """the centres whose lists one query takes, in order: ascending (dist(centre, q), centre index) while fewer
    than need rows are taken; an empty list counts as probed"""
    dc = ((C - q) ** 2).sum(axis=1)
    out, taken = [], 0
    for c in np.lexsort((np.arange(len(C)), dc)):
        if taken >= need:
            break
        out.append(int(c))
        taken += int(sizes[c])
    return out


def query_ref(pts, C, sizes, rows, q, k, checks):
    """(idx (nq, k) int64, dist (nq, k), rows taken (nq,), lists probed (nq,))"""
    q = np.atleast_2d(q)
    n = len(pts)
    off = np.concatenate(([0], np.cumsum(sizes)))
    need = n if checks == -1 else min(n, max(checks, k))
    idx = np.empty((len(q), k), dtype=np.int64)
    dist = np.empty((len(q), k))
    taken = np.zeros(len(q), dtype=np.int64)
    probed = np.zeros(len(q), dtype=np.int64)
    for j in range(len(q)):
        order = probe_order(C, sizes, q[j], need)
        got = [rows[off[c]:off[c + 1]] for c in order]
        taken[j], probed[j] = sum(len(g) for g in got), len(order)
        r = np.concatenate(got).astype(np.int64)
        dd = ((pts[r] - q[j]) ** 2).sum(axis=1)
        o = np.lexsort((r, dd))[:k]
        idx[j], dist[j] = r[o], dd[o]
    return idx, dist, taken, probed


# ---- the cases: name -> (generator of the rows, lists, iterations) ------------------------------------------
def _uniform(seed, n, d):
    return lambda: np.random.RandomState(seed).rand(n, d)


def _dups():
    """600 rows drawn from 40 distinct rows: equal initial centres (exact centre ties, empty lists)"""
    rs = np.random.RandomState(7)
    base = rs.rand(40, 55)
    return base[rs.randint(0, 40, 600)]


def _blobs():
    """20000 rows in 50 Gaussian blobs (sigma 0.05 around uniform centres), in random order"""
    rs = np.random.RandomState(7)
    mid = rs.rand(50, 55)
    return mid[rs.randint(0, 50, 20000)] + 0.05 * rs.randn(20000, 55)


CASES = {
    'u3000': (_uniform(7, 3000, 55), 32, 5),
    'd3': (_uniform(8, 5000, 3), 40, 50),
    'each': (_uniform(9, 100, 8), 100, 2),
    'dups': (_dups, 64, 5),
    'blobs': (_blobs, 128, 5),
    'one': (_uniform(10, 1, 55), 1, 5),
    'w112': (_uniform(11, 700, 112), 16, 4),
    'w150': (_uniform(12, 300, 150), 8, 5),
    'w167': (_uniform(13, 200, 167), 4, 5),
    'u3000_it0': (_uniform(7, 3000, 55), 32, 0),
    'n20000': (_uniform(14, 20000, 55), 64, 3),
}
GPU_CASES = ('u3000', 'd3', 'each', 'dups', 'blobs', 'one', 'w112', 'w150', 'w167', 'u3000_it0', 'n20000')
UNITS_LOG2 = (-80, 70)


@functools.lru_cache(maxsize=None)
def case(name):
    """(pts, L, iters); a name ending in @s is the case with its rows scaled by 2^s"""
    if '@' in name:
        base, s = name.split('@')
        pts, L, iters = case(base)
        pts = pts * 2.0 ** int(s)
    else:
        gen, L, iters = CASES[name]
        pts = np.ascontiguousarray(gen())
    pts.setflags(write=False)
    return pts, L, iters


@functools.lru_cache(maxsize=None)
def reference(name):
    """(centres, assign, iterations run, sizes, rows) of the case, computed once"""
    pts, L, iters = case(name)
    C, a, run = kmeans_ref(pts, L, iters)
    sizes, rows = lists_ref(a, L)
    for x in (C, a, sizes, rows):
        x.setflags(write=False)
    return C, a, run, sizes, rows


@functools.lru_cache(maxsize=None)
def queries(name, nq=64):
    """nq queries of the case: the first half exact rows (distance 0 occurs), the rest rows moved by 1e-2 noise"""
    pts = case(name)[0]
    rs = np.random.RandomState(21)
    pick = rs.randint(0, len(pts), nq)
    q = pts[pick].copy()
    q[nq // 2:] += 1e-2 * rs.randn(nq - nq // 2, pts.shape[1])
    q.setflags(write=False)
    return q


def probed_lists(name, k, checks, nq=64):
    """per query of the case the centres whose lists it takes, in order"""
    pts = case(name)[0]
    C, _, _, sizes, _ = reference(name)
    need = len(pts) if checks == -1 else min(len(pts), max(checks, k))
    return [probe_order(C, sizes, q, need) for q in queries(name, nq)]


@functools.lru_cache(maxsize=None)
def query_reference(name, k, checks, nq=64):
    pts = case(name)[0]
    C, _, _, sizes, rows = reference(name)
    return query_ref(pts, C, sizes, rows, queries(name, nq), k, checks)

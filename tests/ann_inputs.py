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


def _dupwide_base():
    return np.random.RandomState(DUPWIDE_SEED).rand(6, 55)


def _dupwide():
    """2400 rows drawn in random order from 6 distinct rows: three lists of two groups each, every distance of a
    query shared by the about 400 copies of a row, spread over every wave and lane of k_ann_query"""
    rs = np.random.RandomState(DUPWIDE_SEED + 1)
    return _dupwide_base()[rs.randint(0, 6, 2400)]


def _dupwide_queries():
    """the 6 distinct rows, then 26 of the rows moved by 1e-2 noise"""
    rs = np.random.RandomState(DUPWIDE_SEED + 2)
    base = _dupwide_base()
    return np.vstack([base, base[rs.randint(0, 6, DUPWIDE_NQ - 6)] + 1e-2 * rs.randn(DUPWIDE_NQ - 6, 55)])


DUPWIDE_SEED, DUPWIDE_NQ = 45, 32   # (the seed: the first from 31 up whose three lists hold two of the rows each)
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
    'L4096': (_uniform(15, 8192, 8), 4096, 2),
    'L1000': (_uniform(16, 6000, 24), 1000, 3),
    'L300': (_uniform(17, 3000, 55), 300, 3),
    'd1': (_uniform(18, 500, 1), 10, 5),
    'dupwide': (_dupwide, 3, 2),
}
OWN_QUERIES = {'dupwide': (_dupwide_queries, DUPWIDE_NQ)}   # name -> (generator, nq): not rows of the case plus noise
GPU_CASES = ('u3000', 'd3', 'each', 'dups', 'blobs', 'one', 'w112', 'w150', 'w167', 'u3000_it0', 'n20000')
# The sizes at which k_ann_query's loops take their second trip (size trips): more than 256
# and more than 512 lists (the bitonic sort's and the fill's stride), the full 4,096-list sort area, a prefix that
# stops in its second block of 64 lists and in a later one, queries at widths 1, 3, 112, 150 and 167, and ties
# that the merge of the four waves' lists has to cut through.  Built beside GPU_CASES; queried by QUERY_SIZE_RUNS.
QUERY_SIZE_CASES = ('L4096', 'L1000', 'L300', 'd1', 'dupwide')
# (case, k, checks, also compared with ExactIndex.query_knn)
QUERY_SIZE_RUNS = (
    ('L4096', 1, 1, False), ('L4096', 5, 64, False), ('L4096', 64, 2000, False), ('L4096', 3, -1, True),
    ('L1000', 5, 600, False), ('L1000', 64, 1500, False), ('L1000', 5, -1, True),
    ('L300', 5, 1500, False),
    ('w112', 5, 64, False), ('w112', 5, -1, True), ('w150', 5, 64, False), ('w150', 5, -1, True),
    ('w167', 5, 64, False), ('w167', 5, -1, True), ('d3', 5, 64, False), ('d3', 5, -1, True),
    ('d1', 5, 64, False), ('d1', 5, -1, True),
    ('dupwide', 64, 1, False), ('dupwide', 64, 1000, False),
)
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
    if name in OWN_QUERIES:
        gen, own_nq = OWN_QUERIES[name]
        assert nq == own_nq, (name, nq)
        q = np.ascontiguousarray(gen())
        q.setflags(write=False)
        return q
    rs = np.random.RandomState(21)
    pick = rs.randint(0, len(pts), nq)
    q = pts[pick].copy()
    q[nq // 2:] += 1e-2 * rs.randn(nq - nq // 2, pts.shape[1])
    q.setflags(write=False)
    return q


def taken_rows(name, k, checks, nq=64):
    """per query of the case (rows, dist, pos, list): the rows it takes in probe order, their distances, each
    row's position inside its list and the list's place in the probe order"""
    pts = case(name)[0]
    C, _, _, sizes, rows = reference(name)
    off = np.concatenate(([0], np.cumsum(sizes)))
    out = []
    for q, order in zip(queries(name, nq), probed_lists(name, k, checks, nq)):
        r = np.concatenate([rows[off[c]:off[c + 1]] for c in order]).astype(np.int64)
        pos = np.concatenate([np.arange(sizes[c]) for c in order])
        which = np.concatenate([np.full(sizes[c], i) for i, c in enumerate(order)])
        out.append((r, ((pts[r] - q) ** 2).sum(axis=1), pos, which))
    return out


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

"""Cases for the exact k-NN of the GPU index (ia_index_query_knn, certified_topk; pure numpy, no GPU
import) with the plain reference tests/test_gpu_knn.py compares them with bit for bit.  Every
generator is deterministic; tests/test_knn_cpu.py pins, without a GPU, that each case is what it
claims to be.

Reference: numpy fp64 ((pts - q) ** 2).sum(axis=1) per query, the k smallest (distance, index)
pairs in ascending (distance, index) order (np.lexsort).
"""
import functools

import numpy as np

import api_edge_inputs as E

KNN_MAX = 64       # IA_KNN_MAX
TILE_MUL = 2654435761   # IA_TILE_MUL


def knn_reference(pts, q, k):
    """(idx (nq, k) int64, dist (nq, k) float64): per query the k rows of smallest (distance, index)"""
    q = np.atleast_2d(q)
    n = len(pts)
    idx = np.empty((len(q), k), dtype=np.int64)
    dist = np.empty((len(q), k), dtype=np.float64)
    for j in range(len(q)):
        dd = ((pts - q[j]) ** 2).sum(axis=1)
        order = np.lexsort((np.arange(n), dd))[:k]
        idx[j], dist[j] = order, dd[order]
    return idx, dist


def row_tile_slot(row, n):
    """(tile, slot) of DB row `row` of an n-row index: slot j of tile t holds row j * NT + perm(t),
    perm(t) = t * (TILE_MUL mod NT) mod NT (ia_pos_row, restated as _native.shard_rows does)"""
    nt = -(-n // E.TILE)
    perm = np.arange(nt, dtype=np.int64) * (TILE_MUL % nt) % nt
    return int(np.flatnonzero(perm == row % nt)[0]), row // nt


# ---- the cases: name -> () -> (pts, q) -----------------------------------------------------------
CLUSTER_Q0, CLUSTER_ROWS = 40, [7 + 313 * j for j in range(10)]


def _cluster():
    """n10000 (NT = 313) with rows 7 + 313 j, j = 0..9 (slots 0..9 of one tile) within 1e-3 of query 40"""
    pts, q = E.INDEX_CASES['n10000']()
    pts = pts.copy()
    pts[CLUSTER_ROWS] = q[CLUSTER_Q0] + 1e-3 * np.random.RandomState(101).rand(10, 55)
    return pts, q


DUP_ROWS = [7, 7 + 313, 7 + 626]


def _duplicates():
    """n10000 with rows 320 and 633 equal to row 7 (one tile); 64 queries within 1e-3 of that row, the
    first one the row itself"""
    pts, _ = E.INDEX_CASES['n10000']()
    pts = pts.copy()
    pts[DUP_ROWS[1:]] = pts[7]
    q = pts[7] + 1e-3 * np.random.RandomState(102).rand(64, 55)
    q[0] = pts[7]
    return pts, q


def _all_equal():
    """500 equal rows of multiples of 2^-8 (their column sums and means are exact: ia_index_build keeps
    sc = 1 and the centred copy is zero), 64 random queries, the first one the row itself"""
    rs = np.random.RandomState(103)
    pts = np.tile(rs.randint(0, 256, 55) / 256.0, (500, 1))
    q = rs.rand(64, 55)
    q[0] = pts[0]
    return pts, q


def _small(n):
    return lambda: E._rand_index(110 + n, n, 55, 64)


def _head64(case):
    def f():
        pts, q = case()
        return pts, q[:64]
    return f


CASES = {
    'n10000': E.INDEX_CASES['n10000'],
    'n70005': E.INDEX_CASES['n70005'],
    'n70005_neartie': E.INDEX_CASES['n70005_neartie'],
    'n100': _small(100), 'n64': _small(64), 'n33': _small(33), 'n1': _small(1),
    'cluster': _cluster,
    'duplicates': _duplicates,
    'all_equal': _all_equal,
    'nq4097': E.INDEX_CASES['nq4097'],
    'd55_nq353': E.INDEX_CASES['d55_nq353'],
    'd56_nq161': E.INDEX_CASES['d56_nq161'],
    'd112_nq97': E.INDEX_CASES['d112_nq97'],
    'reuse': _head64(lambda: (E.reuse_index()[0], E.reuse_index()[1][2])),
}
K_RANDOM = (2, 3, 5, 16, 63, 64)          # on n10000 and n70005
K_NEARTIE = (16, 64)
SHORT_LIST = (('n100', 3), ('n64', 64), ('n33', 5), ('n1', 1))
K_CLUSTER = (5, 10, 16)
K_DUPLICATES = (2, 4)
K_ALL_EQUAL = 7
K_LOOPS = (('nq4097', 3), ('d55_nq353', 5), ('d56_nq161', 5), ('d112_nq97', 5))
K_REUSE = (64, 2, 16)                      # in this order on one index
UNITS_LOG2, K_UNITS = (-80, 70), 5


@functools.lru_cache(maxsize=None)
def case(name):
    pts, q = CASES[name]()
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


@functools.lru_cache(maxsize=None)
def _case_reference(name):
    pts, q = case(name)
    idx, dist = knn_reference(pts, q, min(KNN_MAX, len(pts)))
    idx.setflags(write=False)
    dist.setflags(write=False)
    return idx, dist


def reference(name, k):
    """knn_reference of the case, computed once per case at k = min(64, n): the k-NN lists of one
    query are prefixes of each other"""
    idx, dist = _case_reference(name)
    return idx[:, :k], dist[:, :k]

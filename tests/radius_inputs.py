"""Cases for the exact fixed-radius search of the GPU index (ia_index_count_radius,
ia_index_query_radius; pure numpy, no GPU import) with the plain reference tests/test_gpu_radius.py
compares them with bit for bit.  The rows and queries are those of tests/knn_inputs.py; the radii are
derived per query from the sorted reference distances.  tests/test_radius_cpu.py pins, without a GPU,
that each case is what it claims to be.

Reference: numpy fp64 dd = ((pts - q) ** 2).sum(axis=1) per query, the rows with dd < radius
(strictly) in ascending (distance, index) order (np.lexsort).
"""
import functools

import numpy as np

import knn_inputs as K

SORT_LDS = 4096    # IA_R_SORT_LDS: the longest query segment sorted in LDS
K_RANDOM = (0, 1, 5, 64, 700)            # rows inside, on n10000 and n70005
BOUNDARY = (('n70005_neartie', 20), ('n10000', 5))
SMALL = ('n1', 'n33', 'n64', 'n100')
LOOPS = ('nq4097', 'd55_nq353', 'd56_nq161', 'd112_nq97')
MAX_NN = (1, 16, 64, 1000)
K_FIXED = (64, 700)
SUB_CASE, SUB_WORKSPACE = 'd55_nq353', 3 * 704   # three padded row counts of its 700-row index
UNITS_LOG2, K_UNITS = (-80, 70), 5
CERT_CASE, CERT_K = 'n70005', 64

case = K.case


def csr(dd_rows, radii):
    """(count (nq,), offsets (nq + 1,), idx, dist): per query the rows with dd < radius, ascending
    (distance, index)"""
    idx, dist, count = [], [], []
    for dd, r in zip(dd_rows, radii):
        order = np.lexsort((np.arange(len(dd)), dd))
        order = order[dd[order] < r]
        idx.append(order)
        dist.append(dd[order])
        count.append(len(order))
    offsets = np.zeros(len(count) + 1, dtype=np.int64)
    np.cumsum(count, out=offsets[1:])
    return (np.array(count, dtype=np.int64), offsets, np.concatenate(idx).astype(np.int64) if idx else np.empty(0, np.int64),
            np.concatenate(dist) if dist else np.empty(0))


def distances(pts, q):
    """dd (nq, n): numpy fp64 ((pts - q) ** 2).sum(axis=1) per query"""
    q = np.atleast_2d(q)
    return np.stack([((pts - q[j]) ** 2).sum(axis=1) for j in range(len(q))])


def radius_reference(pts, q, radii):
    """csr() of arbitrary rows, queries and radii (a scalar or one per query)"""
    dd = distances(pts, q)
    return csr(dd, np.broadcast_to(np.asarray(radii, dtype=np.float64), (len(dd),)))


@functools.lru_cache(maxsize=None)
def dd_of(name):
    """the case's distance matrix (nq, n), computed once and left unchanged"""
    dd = distances(*case(name))
    dd.setflags(write=False)
    return dd


@functools.lru_cache(maxsize=None)
def sorted_dd(name):
    s = np.sort(dd_of(name), axis=1)
    s.setflags(write=False)
    return s


def reference(name, radii, queries=None):
    """csr() of the named case (of its queries `queries`, an index array, when given)"""
    dd = dd_of(name) if queries is None else dd_of(name)[queries]
    return csr(dd, np.broadcast_to(np.asarray(radii, dtype=np.float64), (len(dd),)))


# ---- radii, one per query, from the sorted reference distances s --------------------------------
def midpoint(name, k):
    """a radius that holds exactly k rows: (s[k-1] + s[k]) / 2; k = 0: s[0] / 2, or 0.0 for an exact hit"""
    s = sorted_dd(name)
    if k == 0:
        return s[:, 0] / 2
    return (s[:, k - 1] + s[:, k]) / 2


def at_kth(name, k):
    """(s[k-1], its successor): the radius that just excludes the k-th nearest row and the one that just
    includes it"""
    r = sorted_dd(name)[:, k - 1].copy()
    return r, np.nextafter(r, np.inf)


def median(name):
    return np.median(dd_of(name), axis=1)


def mixed(name):
    """per-query radii in one call: 0, the 5-row midpoint, +inf, in turn"""
    r = midpoint(name, 5).copy()
    r[0::3] = 0.0
    r[2::3] = np.inf
    return r


def ragged_offsets(nq):
    """capacities 0, 3, 70, 0, 1, ... in turn: some empty, some below and some above a count of 64"""
    cap = np.array([0, 3, 70, 0, 1][:5] * (nq // 5 + 1), dtype=np.int64)[:nq]
    off = np.full(nq + 1, 2, dtype=np.int64)    # offsets[0] > 0 is allowed
    off[1:] += np.cumsum(cap)
    return off

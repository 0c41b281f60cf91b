"""pyflann drop-in over libia's exact GPU index ("minimal" depth).

The reference imports pyflann once (`import pyflann as pf`, algorithms.py:5) and uses it at
three call sites: `pf.FLANN()` (algorithms.py:56), `build_index(pts, algorithm='kdtree')`
(:69, returns a params dict with 'checks') and `nn_index(q, 1, checks=...)` (:74, returns
(indices, squared distances)).  A maintainer who keeps the reference's per-pixel loop replaces
that import with `import flann_mi355x as pf`.  Only the C ABI of include/ia.h is used here
(ctypes, no torch): ia_init, ia_index_build, ia_index_query, ia_index_query_knn, ia_index_count_radius,
ia_index_query_radius, ia_index_destroy, ia_kmeans, ia_ann_build, ia_ann_query, ia_ann_destroy, ia_last_error.

Semantics change from FLANN's randomised kd-forest to exact k-NN: squared L2 in fp64 with
numpy's summation order, lowest index on ties (FLANN `linear`, the reference's brute force).
num_neighbors = 1 returns 1-D arrays, 2..min(n, 64) returns (nq, k) arrays, nearest first.
nn_radius(query, radius) returns every row with squared distance < radius of one query, nearest first.

build_index(pts, algorithm='kmeans', iterations=5, n_lists=None, checks=32) is the one setting where
`checks` means something: a deterministic k-means inverted file (ia_ann_*) whose
nn_index(q, k, checks=c) looks at whole lists, nearest centre first, until max(c, k) rows are taken
(checks = -1: every row, the exact answer).  It is neither FLANN's randomised result nor the reference's.
FLANN.kmeans(pts, num_clusters, max_iterations) returns that rule's centres (a flat k-means).
"""
import ctypes
import math
import os

import numpy as np

_LIB = os.environ.get('IA_LIBIA', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libia.so'))
_vp, _i64 = ctypes.c_void_p, ctypes.c_int64
_L = None
_ctx = None
KNN_MAX = 64   # IA_KNN_MAX
ANN_MAX_LISTS = 4096   # IA_ANN_MAX_LISTS


def _lib():
    global _L, _ctx
    if _L is None:
        L = ctypes.CDLL(_LIB)
        L.ia_init.argtypes = [ctypes.c_int, ctypes.POINTER(_vp)]
        L.ia_index_build.argtypes = [_vp, _vp, _i64, ctypes.c_int, ctypes.POINTER(_vp)]
        L.ia_index_query.argtypes = [_vp, _vp, _i64, _vp, _vp]
        L.ia_index_query_knn.argtypes = [_vp, _vp, _i64, ctypes.c_int, _vp, _vp]
        L.ia_index_count_radius.argtypes = [_vp, _vp, _i64, _vp, _vp]
        L.ia_index_query_radius.argtypes = [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]
        L.ia_index_destroy.argtypes = [_vp]
        L.ia_index_destroy.restype = None
        L.ia_kmeans.argtypes = [_vp, _vp, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp,
                                ctypes.POINTER(ctypes.c_int)]
        L.ia_ann_build.argtypes = [_vp, _vp, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]
        L.ia_ann_query.argtypes = [_vp, _vp, _i64, ctypes.c_int, ctypes.c_int, _vp, _vp]
        L.ia_ann_destroy.argtypes = [_vp]
        L.ia_ann_destroy.restype = None
        L.ia_last_error.restype = ctypes.c_char_p
        ctx = _vp()
        if L.ia_init(int(os.environ.get('LOCAL_RANK', 0)), ctypes.byref(ctx)):
            raise RuntimeError(L.ia_last_error().decode())
        _L, _ctx = L, ctx
    return _L


class FLANN(object):
    """pf.FLANN(): one exact index per object (build_index replaces the previous one)."""

    def __init__(self, **kwargs):
        self._h = None
        self._ann = None      # the approximate index of algorithm='kmeans' (then _h is None)
        self._checks = 32     # ... and the checks it was built with
        self._pts = None

    def build_index(self, pts, algorithm='kdtree', **kw):
        L = _lib()
        self.delete_index()
        self._pts = np.ascontiguousarray(pts, dtype=np.float64)
        n, d = self._pts.shape
        h = _vp()
        if algorithm == 'kmeans':
            n_lists = kw.get('n_lists')
            n_lists = max(1, min(ANN_MAX_LISTS, math.isqrt(n))) if n_lists is None else int(n_lists)
            iters, checks = int(kw.get('iterations', 5)), int(kw.get('checks', 32))
            if L.ia_ann_build(_ctx, self._pts.ctypes.data, n, d, n_lists, iters, ctypes.byref(h)):
                raise RuntimeError(L.ia_last_error().decode())
            self._ann, self._checks = h, checks
            return {'algorithm': 'kmeans', 'checks': checks, 'n_lists': n_lists, 'iterations': iters, 'exact': False}
        if L.ia_index_build(_ctx, self._pts.ctypes.data, n, d, ctypes.byref(h)):
            raise RuntimeError(L.ia_last_error().decode())
        self._h = h
        return {'checks': kw.get('checks', 32), 'algorithm': algorithm}

    def nn_index(self, qpts, num_neighbors=1, checks=None, **kw):
        if self._h is None and self._ann is None:
            raise RuntimeError('nn_index called before build_index')
        kmax = min(len(self._pts), KNN_MAX)
        if not 1 <= num_neighbors <= kmax:
            raise ValueError('flann_mi355x: num_neighbors must be 1..%d (got %r)' % (kmax, num_neighbors))
        q = np.ascontiguousarray(np.atleast_2d(qpts), dtype=np.float64)
        if self._ann is not None:   # checks bounds the rows looked at; on every other index it is ignored
            k = int(num_neighbors)
            idx = np.empty((len(q), k), np.int64)
            dist = np.empty((len(q), k), np.float64)
            if _lib().ia_ann_query(self._ann, q.ctypes.data, len(q), k, int(self._checks if checks is None else checks),
                                   idx.ctypes.data, dist.ctypes.data):
                raise RuntimeError(_lib().ia_last_error().decode())
            return (idx[:, 0], dist[:, 0]) if k == 1 else (idx, dist)
        if num_neighbors == 1:
            idx = np.empty(len(q), np.int64)
            dist = np.empty(len(q), np.float64)
            rc = _lib().ia_index_query(self._h, q.ctypes.data, len(q), idx.ctypes.data, dist.ctypes.data)
        else:
            k = int(num_neighbors)
            idx = np.empty((len(q), k), np.int64)
            dist = np.empty((len(q), k), np.float64)
            rc = _lib().ia_index_query_knn(self._h, q.ctypes.data, len(q), k, idx.ctypes.data, dist.ctypes.data)
        if rc:
            raise RuntimeError(_lib().ia_last_error().decode())
        return idx, dist

    def nn_radius(self, query, radius, max_nn=-1, **kw):
        """pyflann's nn_radius: the rows with squared distance < radius of ONE query vector, nearest
        first, as (indices int64, squared distances float64); max_nn < 0: all of them.  sorted= and
        checks= are accepted and ignored."""
        if self._ann is not None:
            raise RuntimeError("flann_mi355x: nn_radius needs an exact index: build_index(pts, algorithm='linear')")
        if self._h is None:
            raise RuntimeError('nn_radius called before build_index')
        q = np.ascontiguousarray(query, dtype=np.float64).reshape(1, -1)
        if q.shape[1] != self._pts.shape[1]:
            raise ValueError('flann_mi355x: one query vector of width %d expected' % self._pts.shape[1])
        L = _lib()
        r = np.array([radius], dtype=np.float64)
        count = np.zeros(1, np.int64)
        if max_nn < 0:   # the exact layout: count first
            if L.ia_index_count_radius(self._h, q.ctypes.data, 1, r.ctypes.data, count.ctypes.data):
                raise RuntimeError(L.ia_last_error().decode())
        cap = int(count[0]) if max_nn < 0 else int(max_nn)
        offsets = np.array([0, cap], dtype=np.int64)
        idx = np.empty(max(cap, 1), np.int64)
        dist = np.empty(max(cap, 1), np.float64)
        if L.ia_index_query_radius(self._h, q.ctypes.data, 1, r.ctypes.data, offsets.ctypes.data, idx.ctypes.data,
                                   dist.ctypes.data, count.ctypes.data):
            raise RuntimeError(L.ia_last_error().decode())
        cnt = min(int(count[0]), cap)
        return idx[:cnt], dist[:cnt]

    def nn(self, pts, qpts, num_neighbors=1, **kw):
        """pyflann's one-shot form: build_index(pts), then nn_index(qpts, num_neighbors)"""
        self.build_index(pts, **kw)
        return self.nn_index(qpts, num_neighbors, **kw)

    def kmeans(self, pts, num_clusters, max_iterations=None, dtype=None, **kw):
        """pyflann's kmeans as a FLAT k-means (include/ia.h ia_kmeans: deterministic initial centres, ties to the
        lower centre): the (num_clusters, d) centres after at most max_iterations rounds (None: 5).  pyflann's
        hierarchical `branching` and its other keywords are accepted and ignored; dtype converts the result."""
        L = _lib()
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        n, d = pts.shape
        k = int(num_clusters)
        centers = np.empty((max(k, 0), d), np.float64)
        if L.ia_kmeans(_ctx, pts.ctypes.data, n, d, k, 5 if max_iterations is None else int(max_iterations),
                       centers.ctypes.data, None, None):
            raise RuntimeError(L.ia_last_error().decode())
        return centers if dtype is None else centers.astype(dtype)

    def delete_index(self):
        if self._h is not None:
            _lib().ia_index_destroy(self._h)
            self._h = None
        if self._ann is not None:
            _lib().ia_ann_destroy(self._ann)
            self._ann = None

    def __del__(self):
        try:
            self.delete_index()
        except Exception:
            pass

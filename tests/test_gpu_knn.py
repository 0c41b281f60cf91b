"""GPU parity of the index's exact k-NN (ia_index_query_knn: k_merge_dense_knn, certified_topk) on the
cases of tests/knn_inputs.py, against numpy fp64: the k rows of smallest (distance, index), ascending.
Each test names the path of certified_topk it executes; tests/test_knn_cpu.py pins that on the CPU.
Every comparison is np.array_equal; there is no tolerance anywhere in this file.
"""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

import api_edge_inputs as E
import knn_inputs as K
from golden_util import GOLDEN

pytestmark = pytest.mark.gpu


def _native():
    import ia_amd  # noqa: F401
    from ia_amd import _native
    return _native


_open = {}


@pytest.fixture(scope='module')
def index_of(ctx):
    """case name -> its ExactIndex, built once per module"""
    def get(name):
        if name not in _open:
            _open[name] = _native().ExactIndex(ctx, K.case(name)[0])
        return _open[name]
    yield get
    for idx in _open.values():
        idx.close()
    _open.clear()


def _check(index, name, k, q=None):
    i_ref, d_ref = K.reference(name, k)
    i_gpu, d_gpu = index.query_knn(K.case(name)[1] if q is None else q, k)
    assert i_gpu.shape == d_gpu.shape == i_ref.shape and i_gpu.dtype == np.int64 and d_gpu.dtype == np.float64
    bad = np.flatnonzero((i_gpu != i_ref).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:3], i_gpu[bad[:3]], i_ref[bad[:3]])
    assert np.array_equal(d_gpu, d_ref)


# ---- 1. k = 1 is ia_index_query ------------------------------------------------------------------
@pytest.mark.parametrize('name', ['n10000', 'n70005_neartie'])
def test_k1_equals_index_query(index_of, name):
    index, q = index_of(name), K.case(name)[1]
    i1, d1 = index.query(q)
    ik, dk = index.query_knn(q, 1)
    assert ik.shape == dk.shape == (len(q), 1)
    assert np.array_equal(ik[:, 0], i1) and np.array_equal(dk[:, 0], d1)


# ---- 2. random rows, every k ---------------------------------------------------------------------
@pytest.mark.parametrize('k', K.K_RANDOM)
@pytest.mark.parametrize('name', ['n10000', 'n70005'])
def test_random_rows(index_of, name, k):
    """a_k by bisection over 158 / 876 listed values (up to 2 / 7 records per lane), the rerank of about k
    candidates, the list at k = 2 .. 64 (63: one lane dropped), exact hits at distance 0 in front"""
    _check(index_of(name), name, k)


# ---- 3. near ties ----------------------------------------------------------------------------------
@pytest.mark.parametrize('k', K.K_NEARTIE)
def test_near_ties_decided_in_fp64(index_of, k):
    """40 rows within 2^-30 of each other: all inside the rerank radius, ordered by their fp64 distances;
    k = 64 continues past the group"""
    _check(index_of('n70005_neartie'), 'n70005_neartie', k)


# ---- 4. fewer listed rows than k -------------------------------------------------------------------
@pytest.mark.parametrize('name,k', K.SHORT_LIST)
def test_short_list_rescans_every_chunk(index_of, name, k):
    """one chunk, two listed rows: the list is short after the reranks, so the chunk is rescanned without
    a threshold (n = 64, k = 64: every row, sorted; n = 1: the single row)"""
    index = index_of(name)
    _check(index, name, k)
    if len(K.case(name)[0]) > 1:
        assert index.knn_stats()[1] == 64   # every query rescanned its one chunk


# ---- 5. many of the k nearest in one tile ----------------------------------------------------------
@pytest.mark.parametrize('k', K.K_CLUSTER)
def test_cluster_in_one_tile(index_of, k):
    """ten of query 40's nearest rows share a tile: two are listed, eight come from the chunk's rescan,
    and the two listed ones meet the idempotent insert there"""
    index = index_of('cluster')
    _check(index, 'cluster', k)
    assert index.knn_stats()[1] >= 1


# ---- 6. exact duplicates ---------------------------------------------------------------------------
@pytest.mark.parametrize('k', K.K_DUPLICATES)
def test_duplicates_go_to_the_lower_index(index_of, k):
    """three equal rows in one tile (T equals the listed value): k = 2 cuts the tie group at the lower
    indices 7 and 320"""
    index = index_of('duplicates')
    _check(index, 'duplicates', k)
    assert (index.query_knn(K.case('duplicates')[1], k)[0][:, :2] == [7, 320]).all()


def test_all_rows_equal(index_of):
    """500 equal rows, sc = 1: every value and every T equal, indices 0..6 at one distance"""
    _check(index_of('all_equal'), 'all_equal', K.K_ALL_EQUAL)


# ---- 7. loops and instances ------------------------------------------------------------------------
@pytest.mark.parametrize('name,k', K.K_LOOPS)
def test_batches_and_scan_launches(index_of, name, k):
    """4,097 queries: a second batch of one (idx_out + b0 * k); d = 55 / 56 / 112: a second scan launch
    of each k3_dist instance"""
    _check(index_of(name), name, k)


def test_reuse_across_k_and_null_dist(index_of):
    """k = 64, then 2, then 16 on one index (result buffers sized by the first call); dist_out = NULL
    returns the same indices"""
    N = _native()
    index, q = index_of('reuse'), np.ascontiguousarray(K.case('reuse')[1])
    for k in K.K_REUSE:
        _check(index, 'reuse', k)
    only_idx = np.full((len(q), 16), -7, dtype=np.int64)
    N.check(N.lib().ia_index_query_knn(index._h, ctypes.c_void_p(q.ctypes.data), len(q), 16,
                                       ctypes.c_void_p(only_idx.ctypes.data), None), 'ia_index_query_knn')
    assert np.array_equal(only_idx, K.reference('reuse', 16)[0])


# ---- 8. units ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('log2_scale', K.UNITS_LOG2)
def test_units(ctx, log2_scale):
    """rows and queries scaled by 2^-80 / 2^70: the indices of scale 1, the distances times 4^s"""
    i_ref, d_ref = K.knn_reference(*E.range_index('signed'), K.K_UNITS)
    pts, q = E.range_index('signed', log2_scale)
    index = _native().ExactIndex(ctx, pts)
    try:
        i_gpu, d_gpu = index.query_knn(q, K.K_UNITS)
    finally:
        index.close()
    assert np.array_equal(i_gpu, i_ref) and np.array_equal(d_gpu, d_ref * 4.0 ** log2_scale)


# ---- 9. refusals ---------------------------------------------------------------------------------------
def test_refusals(ctx, index_of):
    """k = 0, 65, n + 1 and a NaN query: IA_EINVAL with both outputs untouched; the wrappers raise their
    own error types for 0 and 65, and num_neighbors = 1 keeps the 1-D return of query()"""
    N = _native()
    from ia_amd import algorithms, flann_mi355x
    index = index_of('n33')
    pts, q = K.case('n33')
    q = np.ascontiguousarray(q)
    qnan = q.copy()
    qnan[5, 3] = np.nan
    for qq, k in ((q, 0), (q, 65), (q, 34), (qnan, 5)):
        i_out = np.full((len(q), 65), -7, dtype=np.int64)
        d_out = np.full((len(q), 65), -7.0)
        rc = N.lib().ia_index_query_knn(index._h, ctypes.c_void_p(qq.ctypes.data), len(qq), k,
                                        ctypes.c_void_p(i_out.ctypes.data), ctypes.c_void_p(d_out.ctypes.data))
        assert rc == -1 and (i_out == -7).all() and (d_out == -7.0).all(), k
    with pytest.raises(N.IAError, match='IA_EINVAL'):
        index.query_knn(q, 34)
    big, _ = K.case('n100')
    g, f = algorithms.GpuFLANN(ctx), flann_mi355x.FLANN()
    g.build_index(big)
    f.build_index(big)
    try:
        for k in (0, 65):
            with pytest.raises(N.IAError):
                g.nn_index(q, k)
            with pytest.raises(ValueError):
                f.nn_index(q, k)
        i_ref, d_ref = g._index.query(q)
        for w in (g, f):
            i1, d1 = w.nn_index(q, 1)
            assert i1.shape == d1.shape == (len(q),) and np.array_equal(i1, i_ref) and np.array_equal(d1, d_ref)
    finally:
        g.delete_index()
        f.delete_index()


# ---- 10. the wrappers ------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['rand_c1', 'rand_c3'])
def test_wrappers_on_the_golden_features(ctx, tag):
    """GpuFLANN.nn_index(Q, 5) and flann_mi355x.FLANN().nn_index(Q, 5) on features.npz level 2: column 0 is
    the reference's own pick, all five columns numpy's; FLANN().nn is build_index + nn_index"""
    from ia_amd import algorithms, flann_mi355x
    g = np.load(os.path.join(GOLDEN, 'features.npz'))
    As, Q, nn = g[tag + '_As_2'], g[tag + '_Q_2'], g[tag + '_nn_2']
    i_ref, d_ref = K.knn_reference(As, Q, 5)
    a, f = algorithms.GpuFLANN(ctx), flann_mi355x.FLANN()
    try:
        for w in (a, f):
            w.build_index(As, algorithm='kdtree')
            idx, dist = w.nn_index(Q, 5, checks=32)
            assert idx.shape == dist.shape == (len(Q), 5)
            assert np.array_equal(idx[:, 0], nn) and np.array_equal(idx, i_ref) and np.array_equal(dist, d_ref)
        i3, d3 = flann_mi355x.FLANN().nn(As, Q, 3)
        assert np.array_equal(i3, i_ref[:, :3]) and np.array_equal(d3, d_ref[:, :3])
        i1, _ = flann_mi355x.FLANN().nn(As, Q)
        assert np.array_equal(i1, nn)
    finally:
        a.delete_index()
        f.delete_index()


# ---- 11. the certified path is the one that runs ---------------------------------------------------------
def test_certified_path_runs(index_of):
    """64 queries at k = 16 on 70,005 rows compute about 64 x (16 + a few) exact distances plus a rare
    chunk of 160 rows; a brute force computes 64 x 70,005.  A condition, not a measurement."""
    index = index_of('n70005')
    _check(index, 'n70005', 16)
    rows, chunks = index.knn_stats()
    print('knn_stats n70005 k=16: %d exact rows, %d chunks rescanned' % (rows, chunks))
    assert 64 * 16 <= rows <= 64 * 70005 // 8

"""The k-NN entry points exist and refuse a NULL index without a GPU, and each case of
tests/knn_inputs.py is what it claims to be: it reaches the path of certified_topk (ia_topk.h) it is
named for, with the launch geometry restated from ia_index.cpp.  No GPU.

These are conditions on the inputs, not measurements: a generator that misses one is changed (or
reseeded), never the condition.
"""
import ctypes

import numpy as np
import pytest

import api_edge_inputs as E
import knn_inputs as K


def test_knn_symbols_and_null_index():
    """both symbols are bound from EXPORTS; the argument checks answer before any HIP call"""
    import ia_amd  # noqa: F401
    from ia_amd import _native
    assert 'ia_index_query_knn' in _native.EXPORTS and 'ia_index_knn_stats' in _native.EXPORTS
    L = _native.lib()
    assert hasattr(L, 'ia_index_query_knn') and hasattr(L, 'ia_index_knn_stats')
    q = np.zeros((1, 4))
    out = np.full(3, -7, dtype=np.int64)
    rc = L.ia_index_query_knn(None, ctypes.c_void_p(q.ctypes.data), 1, 3, ctypes.c_void_p(out.ctypes.data), None)
    assert rc == -1 and (out == -7).all()   # IA_EINVAL, nothing written
    assert b'ia_index_query_knn' in L.ia_last_error()
    assert L.ia_index_knn_stats(None, (ctypes.c_int64 * 2)()) == -1
    assert _native.KNN_MAX == K.KNN_MAX == 64


def test_reference_is_a_sorted_prefix():
    """knn_reference orders by (distance, index); reference() slices one k = 64 run"""
    pts, q = K.case('duplicates')
    idx, dist = K.knn_reference(pts, q[:3], 5)
    assert np.array_equal(idx, K.reference('duplicates', 5)[0][:3])
    assert np.array_equal(dist, K.reference('duplicates', 5)[1][:3])
    for j in range(3):
        pairs = list(zip(dist[j], idx[j]))
        assert pairs == sorted(pairs) and np.array_equal(dist[j], ((pts[idx[j]] - q[j]) ** 2).sum(axis=1))


def test_random_cases():
    """n10000: 79 chunks (158 listed rows >= every k); n70005: tpw 5, 438 chunks, a last chunk of 3
    tiles and a last tile of 21 rows; 64 queries, half of them exact hits"""
    g = E.index_geometry(10000)
    assert (g['n_tiles'], g['tpw'], g['nwg']) == (313, 4, 79)
    g = E.index_geometry(70005)
    assert (g['n_tiles'], g['tpw'], g['nwg'], g['last_chunk'], g['last_rows']) == (2188, 5, 438, 3, 21)
    assert K.K_RANDOM == (2, 3, 5, 16, 63, 64)
    for name in ('n10000', 'n70005'):
        pts, q = K.case(name)
        assert q.shape == (64, 55) and np.array_equal(q[:32], pts[:32])
        idx, dist = K.reference(name, 64)
        assert (dist[:32, 0] == 0).all() and (idx[:32, 0] == np.arange(32)).all() and (dist[:, 1] > 0).all()


def test_neartie_case():
    """the 40 copies of a query's base are its 40 nearest, within 2^-20 of each other and decided in
    fp64 alone (no exact tie), in an order that is not the index order; the 41st row is far, so k = 64
    reaches past the group"""
    idx, dist = K.reference('n70005_neartie', 64)
    assert K.K_NEARTIE == (16, 64) and E.NEARTIE_COPIES == 40
    unsorted16 = 0
    for j in range(len(idx)):
        assert dist[j, 39] <= dist[j, 0] * (1 + E.REL_TIE) and dist[j, 40] > 100 * dist[j, 39]
        assert len(np.unique(dist[j])) == 64
        unsorted16 += int((np.diff(idx[j, :16]) < 0).any())
    assert unsorted16 == len(idx)


def test_short_list_cases():
    """one chunk lists two rows: fewer than k, so the list is short after the reranks and every chunk
    is rescanned; n = 64 with k = 64 returns every row; n = 1 is the smallest index"""
    assert K.SHORT_LIST == (('n100', 3), ('n64', 64), ('n33', 5), ('n1', 1))
    for name, k in K.SHORT_LIST:
        pts, q = K.case(name)
        n = len(pts)
        assert n == int(name[1:]) and q.shape == (64, 55) and k <= n
        assert E.index_geometry(n)['nwg'] == 1
        if n > 1:
            assert 2 * E.index_geometry(n)['nwg'] < k
    idx, _ = K.reference('n64', 64)
    assert (np.sort(idx, axis=1) == np.arange(64)).all()


def test_cluster_case():
    """the ten planted rows are slots 0..9 of one tile and query 40's ten nearest: the tile's chunk
    lists two of them, the other eight are found by its rescan alone"""
    pts, q = K.case('cluster')
    where = [K.row_tile_slot(r, len(pts)) for r in K.CLUSTER_ROWS]
    assert len({t for t, _ in where}) == 1 and [s for _, s in where] == list(range(10))
    idx, dist = K.reference('cluster', 16)
    assert sorted(idx[K.CLUSTER_Q0, :10]) == K.CLUSTER_ROWS
    assert dist[K.CLUSTER_Q0, 9] < 1e-3 * dist[K.CLUSTER_Q0, 10]
    assert K.K_CLUSTER == (5, 10, 16)


def test_duplicate_cases():
    """three equal rows in one tile, nearest to every query: k = 2 cuts the tie group (7 and 320, never
    633); 500 equal rows with an exact mean: sc = 1, every MFMA value and T equal"""
    pts, q = K.case('duplicates')
    assert np.array_equal(pts[320], pts[7]) and np.array_equal(pts[633], pts[7])
    assert len({K.row_tile_slot(r, len(pts))[0] for r in K.DUP_ROWS}) == 1
    idx, dist = K.reference('duplicates', 4)
    assert (idx[:, :3] == K.DUP_ROWS).all() and (dist[:, 0] == dist[:, 2]).all() and (dist[:, 3] > dist[:, 2]).all()
    assert dist[0, 0] == 0 and K.K_DUPLICATES == (2, 4)
    pts, q = K.case('all_equal')
    mu = np.add.accumulate(pts, axis=0)[-1] / len(pts)   # ia_index_build's column means, in its order
    assert pts.shape == (500, 55) and (pts == mu).all()
    idx, dist = K.reference('all_equal', K.K_ALL_EQUAL)
    assert (idx == np.arange(7)).all() and (dist == dist[:, :1]).all() and dist[0, 0] == 0


def test_loop_cases():
    """a second batch of one query; a second scan launch of every k3_dist instance"""
    assert E.query_blocks(4097, 8) == [[11] * 11 + [7], [1]]
    assert E.query_blocks(353, 55) == [[11, 1]] and E.query_blocks(161, 56) == [[5, 1]]
    assert E.query_blocks(97, 112) == [[3, 1]]
    assert [E.index_geometry(700, d)['KH'] for d in (55, 56, 112)] == [28, 56, 84]
    for (name, k), shape in zip(K.K_LOOPS, ((100, 8, 4097), (700, 55, 353), (700, 56, 161), (700, 112, 97))):
        pts, q = K.case(name)
        assert (len(pts), pts.shape[1], len(q)) == shape and k <= len(pts)
    pts, q = K.case('reuse')
    assert pts.shape == (700, 55) and q.shape == (64, 55) and K.K_REUSE == (64, 2, 16)


def test_units_reference_is_scale_invariant():
    """the numpy k-NN of range_index('signed') at 2^-80 and 2^70: the rows of scale 1, distances x 4^s"""
    pts, q = E.range_index('signed')
    i0, d0 = K.knn_reference(pts, q, K.K_UNITS)
    for s in K.UNITS_LOG2:
        i, d = K.knn_reference(*E.range_index('signed', s), K.K_UNITS)
        assert np.array_equal(i, i0) and np.array_equal(d, d0 * 4.0 ** s) and np.isfinite(d).all()


@pytest.mark.parametrize('tag', ['rand_c1', 'rand_c3'])
def test_golden_picks_are_the_first_column(tag):
    """column 0 of the numpy 5-NN of features.npz's level-2 queries is the reference's own pick"""
    import os
    from golden_util import GOLDEN
    g = np.load(os.path.join(GOLDEN, 'features.npz'))
    idx, _ = K.knn_reference(g[tag + '_As_2'], g[tag + '_Q_2'], 5)
    assert np.array_equal(idx[:, 0], g[tag + '_nn_2'])

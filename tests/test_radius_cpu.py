"""The fixed-radius entry points exist and refuse a NULL index without a GPU, and each case of
tests/radius_inputs.py is what it claims to be: the radius derived from the sorted reference distances
holds the number of rows the GPU test is named for, with the launch geometry restated from
ia_index.cpp.  No GPU.

These are conditions on the inputs, not measurements: a generator that misses one is changed (or
reseeded), never the condition.
"""
import ctypes

import numpy as np
import pytest

import api_edge_inputs as E
import knn_inputs as K
import radius_inputs as R

SYMBOLS = ('ia_index_count_radius', 'ia_index_query_radius', 'ia_index_set_workspace', 'ia_index_radius_stats')


def test_radius_symbols_and_null_index():
    """the four symbols are bound from EXPORTS; the argument checks answer before any HIP call"""
    import ia_amd  # noqa: F401
    from ia_amd import _native
    L = _native.lib()
    for name in SYMBOLS:
        assert name in _native.EXPORTS and hasattr(L, name), name
    q, r = np.zeros((1, 4)), np.ones(1)
    off = np.array([0, 3], dtype=np.int64)
    idx, dist, cnt = np.full(3, -7, dtype=np.int64), np.full(3, -7.0), np.full(1, -7, dtype=np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L.ia_index_count_radius(None, p(q), 1, p(r), p(cnt)) == -1
    assert b'ia_index_count_radius' in L.ia_last_error()
    assert L.ia_index_query_radius(None, p(q), 1, p(r), p(off), p(idx), p(dist), p(cnt)) == -1
    assert b'ia_index_query_radius' in L.ia_last_error()
    assert (idx == -7).all() and (dist == -7.0).all() and (cnt == -7).all()   # IA_EINVAL, nothing written
    assert L.ia_index_set_workspace(None, 0) == -1
    assert L.ia_index_radius_stats(None, (ctypes.c_int64 * 4)()) == -1


def test_reference_is_strict_and_sorted():
    """csr() keeps dd < radius only, ordered by (distance, index); reference() restricts to queries"""
    pts, q = K.case('duplicates')
    dd = R.dd_of('duplicates')
    r = dd[:, 7].copy()                                 # the tie group's distance: rows 7, 320, 633
    cnt, off, idx, dist = R.reference('duplicates', r)
    assert (cnt == 0).all() and len(idx) == 0 and off[-1] == 0
    cnt, off, idx, dist = R.reference('duplicates', np.nextafter(r, np.inf))
    assert (cnt == 3).all() and (idx.reshape(-1, 3) == K.DUP_ROWS).all()
    c2, o2, i2, d2 = R.reference('duplicates', np.nextafter(r, np.inf)[[5, 9]], queries=np.array([5, 9]))
    assert np.array_equal(i2, idx[off[5]:off[6]].tolist() + idx[off[9]:off[10]].tolist())
    c3, o3, i3, d3 = R.radius_reference(pts, q[:3], 1.0)
    for j in range(3):
        pairs = list(zip(d3[o3[j]:o3[j + 1]], i3[o3[j]:o3[j + 1]]))
        assert pairs == sorted(pairs) and len(pairs) == int((dd[j] < 1.0).sum())


def test_random_cases_hold_k_rows():
    """n10000 and n70005: the midpoint radius holds exactly k rows for all 64 queries, k = 0 (half the
    nearest distance, or 0.0 for an exact hit) .. 700; n70005: tpw 5, 438 chunks, a last chunk of 3 tiles
    and a last tile of 21 rows"""
    g = E.index_geometry(10000)
    assert (g['n_tiles'], g['tpw'], g['nwg']) == (313, 4, 79)
    g = E.index_geometry(70005)
    assert (g['n_tiles'], g['tpw'], g['nwg'], g['last_chunk'], g['last_rows']) == (2188, 5, 438, 3, 21)
    assert R.K_RANDOM == (0, 1, 5, 64, 700)
    for name in ('n10000', 'n70005'):
        s = R.sorted_dd(name)
        assert s.shape[0] == 64 and (s[:32, 0] == 0).all() and (s[32:, 0] > 0).all()
        for k in R.K_RANDOM:
            r = R.midpoint(name, k)
            assert ((R.dd_of(name) < r[:, None]).sum(axis=1) == k).all(), (name, k)
        assert (R.midpoint(name, 0)[:32] == 0).all()
    assert 64 <= R.SORT_LDS < 10000     # k = 64 sorts in LDS, every row of n10000 does not


def test_boundary_cases():
    """radius exactly the k-th distance excludes that row, its successor includes it, for all 64 queries
    (the k-th and (k+1)-th distances differ); neartie: decided in fp64 alone, the 40 copies lie within 2^-20"""
    assert R.BOUNDARY == (('n70005_neartie', 20), ('n10000', 5)) and E.NEARTIE_COPIES == 40
    for name, k in R.BOUNDARY:
        r, rn = R.at_kth(name, k)
        dd = R.dd_of(name)
        assert ((dd < r[:, None]).sum(axis=1) == k - 1).all() and ((dd < rn[:, None]).sum(axis=1) == k).all()
    s = R.sorted_dd('n70005_neartie')
    assert (s[:, 39] <= s[:, 0] * (1 + E.REL_TIE)).all()
    # all_equal: 500 rows at one distance per query
    dd = R.dd_of('all_equal')
    assert dd.shape == (64, 500) and (dd == dd[:, :1]).all() and dd[0, 0] == 0
    cnt, _, _, _ = R.reference('all_equal', dd[:, 0])
    assert (cnt == 0).all()
    cnt, off, idx, _ = R.reference('all_equal', np.nextafter(dd[:, 0], np.inf))
    assert (cnt == 500).all() and (idx.reshape(64, 500) == np.arange(500)).all()


def test_exact_hit_radii():
    """radius 0 holds nothing; 2^-1000 holds the hit row alone (32 of n10000's 64 queries are hits)"""
    dd = R.dd_of('n10000')
    assert ((dd < 0.0).sum(axis=1) == 0).all()
    inside = dd < 2.0 ** -1000
    assert (inside.sum(axis=1) == [1] * 32 + [0] * 32).all() and inside[np.arange(32), np.arange(32)].all()


def test_small_loop_and_sub_batch_cases():
    """one-chunk indexes; a second batch of one query and a second scan launch of each KH; the median
    radius of d55_nq353 holds 350 rows per query, so a workspace of 3 x 704 entries takes many sub-batches"""
    for name in R.SMALL:
        n = len(K.case(name)[0])
        assert n == int(name[1:]) and E.index_geometry(n)['nwg'] == 1
        assert ((R.dd_of(name) < R.midpoint(name, n // 2)[:, None]).sum(axis=1) == n // 2).all()
    assert E.query_blocks(4097, 8) == [[11] * 11 + [7], [1]]
    assert E.query_blocks(353, 55) == [[11, 1]] and E.query_blocks(161, 56) == [[5, 1]]
    assert E.query_blocks(97, 112) == [[3, 1]]
    assert R.LOOPS == ('nq4097', 'd55_nq353', 'd56_nq161', 'd112_nq97')
    dd = R.dd_of(R.SUB_CASE)
    assert dd.shape == (353, 700) and ((dd < R.median(R.SUB_CASE)[:, None]).sum(axis=1) == 350).all()
    assert E.index_geometry(700)['n_tiles'] * E.TILE == 704 and R.SUB_WORKSPACE == 3 * 704 < 353 * 350


def test_mixed_radii_and_ragged_layout():
    r = R.mixed('n10000')
    cnt = R.reference('n10000', r)[0]
    assert (cnt[0::3] == 0).all() and (cnt[1::3] == 5).all() and (cnt[2::3] == 10000).all()
    off = R.ragged_offsets(64)
    cap = np.diff(off)
    assert off[0] == 2 and (cap >= 0).all() and (cap == 0).sum() >= 20 and (cap > 64).any() and ((cap > 0) & (cap < 64)).any()


def test_units_reference_is_scale_invariant():
    """the numpy radius search of range_index('signed') at 2^-80 and 2^70 with radii x 4^s: the rows of scale
    1, distances x 4^s"""
    pts, q = E.range_index('signed')
    s = np.sort(R.distances(pts, q), axis=1)
    r = (s[:, R.K_UNITS - 1] + s[:, R.K_UNITS]) / 2
    c0, o0, i0, d0 = R.radius_reference(pts, q, r)
    assert (c0 == R.K_UNITS).all()
    for sh in R.UNITS_LOG2:
        c, o, i, d = R.radius_reference(*E.range_index('signed', sh), r * 4.0 ** sh)
        assert np.array_equal(c, c0) and np.array_equal(i, i0) and np.array_equal(d, d0 * 4.0 ** sh)


@pytest.mark.parametrize('tag', ['rand_c1', 'rand_c3'])
def test_golden_picks_are_the_nearest_inside(tag):
    """with the radius between the 5th and 6th distance, the numpy search of features.npz's level-2 queries
    returns 5 rows, the first the reference's own pick"""
    import os
    from golden_util import GOLDEN
    g = np.load(os.path.join(GOLDEN, 'features.npz'))
    As, Q, nn = g[tag + '_As_2'], g[tag + '_Q_2'], g[tag + '_nn_2']
    s = np.sort(R.distances(As, Q), axis=1)
    cnt, off, idx, _ = R.radius_reference(As, Q, (s[:, 4] + s[:, 5]) / 2)
    assert (cnt == 5).all() and np.array_equal(idx[off[:-1]], nn)

"""GPU parity of the index's exact fixed-radius search (ia_index_count_radius, ia_index_query_radius:
ia_k3r.hip) on the cases of tests/radius_inputs.py, against numpy fp64: the rows with dd < radius,
ascending (distance, index).  tests/test_radius_cpu.py pins on the CPU that each radius holds the rows
the test is named for.  Every comparison is np.array_equal; there is no tolerance anywhere in this file.
"""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

import api_edge_inputs as E
import knn_inputs as K
import radius_inputs as R
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


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _check(index, name, radii, queries=None, count_too=True):
    """the CSR form and the counting call against the reference; returns the reference counts"""
    q = K.case(name)[1] if queries is None else K.case(name)[1][queries]
    c_ref, o_ref, i_ref, d_ref = R.reference(name, radii, queries)
    off, idx, dist = index.query_radius(q, radii)
    stats = index.radius_stats()
    assert off.dtype == idx.dtype == np.int64 and dist.dtype == np.float64
    assert np.array_equal(off, o_ref), np.flatnonzero(np.diff(off) != c_ref)[:5]
    assert np.array_equal(idx, i_ref) and np.array_equal(dist, d_ref)
    assert stats[1] == c_ref.sum()
    if count_too:
        cnt = index.count_radius(q, radii)
        assert cnt.dtype == np.int64 and np.array_equal(cnt, c_ref)
        assert index.radius_stats()[1] == c_ref.sum()
    return c_ref, stats


# ---- 1. random rows ------------------------------------------------------------------------------
@pytest.mark.parametrize('k', R.K_RANDOM)
@pytest.mark.parametrize('name', ['n10000', 'n70005'])
def test_random_rows(index_of, name, k):
    """exactly k rows inside for each of 64 queries, half of them exact hits; k = 64 sorts in LDS"""
    c_ref, stats = _check(index_of(name), name, R.midpoint(name, k))
    assert (c_ref == k).all()
    if k == 64:
        assert stats[3] == 0


# ---- 2. the boundary -----------------------------------------------------------------------------
@pytest.mark.parametrize('name,k', R.BOUNDARY)
def test_radius_at_the_kth_distance_is_strict(index_of, name, k):
    """radius exactly the k-th distance leaves that row out, its successor takes it in; the near ties are
    decided in fp64 alone"""
    r, rn = R.at_kth(name, k)
    assert (_check(index_of(name), name, r)[0] == k - 1).all()
    assert (_check(index_of(name), name, rn)[0] == k).all()


def test_duplicates_at_the_tie_distance(index_of):
    """three equal rows: radius = their distance returns none of them, its successor rows 7, 320, 633 in
    that order (query 0 is the row itself: radius 0, then the smallest subnormal)"""
    index, q = index_of('duplicates'), K.case('duplicates')[1]
    r = R.dd_of('duplicates')[:, 7].copy()
    assert (_check(index, 'duplicates', r)[0] == 0).all()
    assert (_check(index, 'duplicates', np.nextafter(r, np.inf))[0] == 3).all()
    idx, dist, cnt = index.query_radius(q, np.nextafter(r, np.inf), 4)
    assert (idx[:, :3] == K.DUP_ROWS).all() and (idx[:, 3] == -1).all() and (cnt == 3).all() and dist[0, 0] == 0


def test_all_rows_equal(index_of):
    """500 equal rows, sc = 1, every scan value equal: radius = the common distance returns nothing, its
    successor all 500 in index order"""
    index = index_of('all_equal')
    r = R.dd_of('all_equal')[:, 0].copy()
    assert (_check(index, 'all_equal', r)[0] == 0).all()
    assert (_check(index, 'all_equal', np.nextafter(r, np.inf))[0] == 500).all()
    off, idx, _ = index.query_radius(K.case('all_equal')[1], np.nextafter(r, np.inf))
    assert (idx.reshape(64, 500) == np.arange(500)).all()


# ---- 3. exact hits -------------------------------------------------------------------------------
def test_exact_hits(index_of):
    """radius 0 returns nothing even for an exact hit (strict); 2^-1000 returns the hit row alone at
    distance 0"""
    index, q = index_of('n10000'), K.case('n10000')[1]
    assert (_check(index, 'n10000', 0.0)[0] == 0).all()
    c_ref, _ = _check(index, 'n10000', 2.0 ** -1000)
    assert (c_ref == [1] * 32 + [0] * 32).all()
    idx, dist, cnt = index.query_radius(q, 2.0 ** -1000, 1)
    assert (idx[:32, 0] == np.arange(32)).all() and (dist[:32, 0] == 0).all() and (idx[32:] == -1).all()


# ---- 4. everything -------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [np.inf, 1e300])
@pytest.mark.parametrize('name,queries', [('n10000', None), ('n70005', np.array([3, 40]))])
def test_every_row(index_of, name, queries, radius):
    """radius +inf / 1e300: all n rows in the reference's order, no padding row (their norm of 1e30 is
    inside the thresholds: the fp64 verification drops them), segments sorted in global memory"""
    index, n = index_of(name), len(K.case(name)[0])
    c_ref, stats = _check(index, name, radius, queries)
    assert (c_ref == n).all()
    off, idx, dist = index.query_radius(K.case(name)[1] if queries is None else K.case(name)[1][queries], radius)
    assert idx.min() == 0 and idx.max() == n - 1 and np.isfinite(dist).all()
    assert stats[3] >= 1


# ---- 5. small indexes ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.SMALL)
def test_small_indexes(index_of, name):
    """one chunk, fewer rows than a tile or a few: everything, and half of the rows"""
    n = len(K.case(name)[0])
    assert (_check(index_of(name), name, np.inf)[0] == n).all()
    assert (_check(index_of(name), name, R.midpoint(name, n // 2))[0] == n // 2).all()


# ---- 6. loops and instances ----------------------------------------------------------------------
@pytest.mark.parametrize('name', R.LOOPS)
def test_batches_and_scan_launches(index_of, name):
    """4,097 queries: a second batch of one; d = 55 / 56 / 112: a second scan launch of each KH instance of
    both passes; at the median radius (half of the rows)"""
    _check(index_of(name), name, R.median(name))


# ---- 7. fixed width ------------------------------------------------------------------------------
@pytest.mark.parametrize('k', R.K_FIXED)
@pytest.mark.parametrize('max_nn', R.MAX_NN)
def test_fixed_width(index_of, max_nn, k):
    """the max_nn nearest in order, -1 / +inf behind them, count the full count"""
    index, q = index_of('n10000'), K.case('n10000')[1]
    r = R.midpoint('n10000', k)
    c_ref, o_ref, i_ref, d_ref = R.reference('n10000', r)
    idx, dist, cnt = index.query_radius(q, r, max_nn)
    assert idx.shape == dist.shape == (64, max_nn) and np.array_equal(cnt, c_ref) and (cnt == k).all()
    m = min(max_nn, k)
    assert np.array_equal(idx[:, :m], i_ref.reshape(64, k)[:, :m]) and np.array_equal(dist[:, :m], d_ref.reshape(64, k)[:, :m])
    assert (idx[:, m:] == -1).all() and (dist[:, m:] == np.inf).all()


def test_ragged_layout_and_null_dist(index_of):
    """capacities 0, 3, 70, 0, 1, ... starting at offsets[0] = 2: each query's own slots and nothing else
    is written; dist_out = NULL returns the same indices"""
    N = _native()
    index, q = index_of('n10000'), np.ascontiguousarray(K.case('n10000')[1])
    r = np.ascontiguousarray(R.midpoint('n10000', 64))
    c_ref, o_ref, i_ref, d_ref = R.reference('n10000', r)
    off = R.ragged_offsets(64)
    want_i = np.full(off[-1] + 3, -7, dtype=np.int64)
    want_d = np.full(off[-1] + 3, -7.0)
    for j in range(64):
        cap = off[j + 1] - off[j]
        m = min(cap, 64)
        want_i[off[j]:off[j + 1]] = np.concatenate([i_ref[o_ref[j]:o_ref[j] + m], np.full(cap - m, -1)])
        want_d[off[j]:off[j + 1]] = np.concatenate([d_ref[o_ref[j]:o_ref[j] + m], np.full(cap - m, np.inf)])
    for with_dist in (True, False):
        idx, dist, cnt = np.full_like(want_i, -7), np.full_like(want_d, -7.0), np.zeros(64, dtype=np.int64)
        N.check(N.lib().ia_index_query_radius(index._h, _p(q), 64, _p(r), _p(off), _p(idx), _p(dist) if with_dist else None,
                                              _p(cnt)), 'ia_index_query_radius')
        assert np.array_equal(idx, want_i) and np.array_equal(cnt, c_ref)
        assert np.array_equal(dist, want_d) if with_dist else (dist == -7.0).all()


# ---- 8. per-query radii --------------------------------------------------------------------------
def test_per_query_radii(index_of):
    """0, the 5-row midpoint and +inf in one call: counts 0, 5 and n side by side"""
    c_ref, _ = _check(index_of('n10000'), 'n10000', R.mixed('n10000'))
    assert (c_ref[0::3] == 0).all() and (c_ref[1::3] == 5).all() and (c_ref[2::3] == 10000).all()


# ---- 9. sub-batches ------------------------------------------------------------------------------
def test_sub_batches(index_of):
    """a workspace of three padded row counts: the batch of 353 queries x ~350 candidates is filled in many
    sub-batches that do not align to query tiles, with the results of the default workspace"""
    index, q, r = index_of(R.SUB_CASE), K.case(R.SUB_CASE)[1], R.median(R.SUB_CASE)
    whole = index.query_radius(q, r)
    assert index.radius_stats()[2] == 1
    index.set_workspace(R.SUB_WORKSPACE)
    try:
        c_ref, stats = _check(index, R.SUB_CASE, r)
        parts = index.query_radius(q, r)
        print('radius_stats with a workspace of %d entries: %r' % (R.SUB_WORKSPACE, stats))
        assert stats[2] > 1 and stats[0] >= c_ref.sum()
        assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
        index.count_radius(q, r)
    finally:
        index.set_workspace(0)
    _check(index, R.SUB_CASE, r, count_too=False)
    assert index.radius_stats()[2] == 1


# ---- 10. reuse -----------------------------------------------------------------------------------
def test_reuse_with_the_other_queries(index_of):
    """one index answers query, query_knn(16), query_radius and count_radius in turn, then again with
    fewer queries: each resizes the shared query buffers for itself"""
    index, (pts, q) = index_of('reuse'), K.case('reuse')
    r = R.midpoint('reuse', 20)
    for sel in (np.arange(64), np.arange(5)):
        i1, d1 = index.query(q[sel])
        assert np.array_equal(i1, K.reference('reuse', 1)[0][sel, 0])
        ik, dk = index.query_knn(q[sel], 16)
        assert np.array_equal(ik, K.reference('reuse', 16)[0][sel]) and np.array_equal(dk, K.reference('reuse', 16)[1][sel])
        assert (_check(index, 'reuse', r[sel], sel)[0] == 20).all()


# ---- 11. units -----------------------------------------------------------------------------------
@pytest.mark.parametrize('log2_scale', R.UNITS_LOG2)
def test_units(ctx, log2_scale):
    """rows, queries scaled by 2^-80 / 2^70 and radii by 4^s: the indices of scale 1, the distances x 4^s"""
    pts, q = E.range_index('signed')
    s = np.sort(R.distances(pts, q), axis=1)
    r = (s[:, R.K_UNITS - 1] + s[:, R.K_UNITS]) / 2
    c_ref, o_ref, i_ref, d_ref = R.radius_reference(pts, q, r)
    pts, q = E.range_index('signed', log2_scale)
    index = _native().ExactIndex(ctx, pts)
    try:
        off, idx, dist = index.query_radius(q, r * 4.0 ** log2_scale)
        cnt = index.count_radius(q, r * 4.0 ** log2_scale)
    finally:
        index.close()
    assert np.array_equal(off, o_ref) and np.array_equal(idx, i_ref) and np.array_equal(dist, d_ref * 4.0 ** log2_scale)
    assert np.array_equal(cnt, c_ref) and (cnt == R.K_UNITS).all()


# ---- 12. refusals --------------------------------------------------------------------------------
def test_refusals(ctx, index_of):
    """radius -1, NaN, decreasing offsets and a NaN query: IA_EINVAL with all three outputs untouched; the
    wrappers raise before build_index"""
    N = _native()
    from ia_amd import algorithms, flann_mi355x
    index = index_of('n33')
    q = np.ascontiguousarray(K.case('n33')[1])
    nq = len(q)
    ok_r, ok_off = np.full(nq, 1.0), np.arange(nq + 1, dtype=np.int64) * 2
    bad_r1, bad_r2 = ok_r.copy(), ok_r.copy()
    bad_r1[7], bad_r2[9] = -1.0, np.nan
    bad_off = ok_off.copy()
    bad_off[11] = bad_off[10] - 1
    qnan = q.copy()
    qnan[5, 3] = np.nan
    for qq, rr, oo in ((q, bad_r1, ok_off), (q, bad_r2, ok_off), (q, ok_r, bad_off), (qnan, ok_r, ok_off)):
        idx, dist, cnt = np.full(2 * nq, -7, dtype=np.int64), np.full(2 * nq, -7.0), np.full(nq, -7, dtype=np.int64)
        rc = N.lib().ia_index_query_radius(index._h, _p(qq), nq, _p(rr), _p(oo), _p(idx), _p(dist), _p(cnt))
        assert rc == -1 and (idx == -7).all() and (dist == -7.0).all() and (cnt == -7).all()
        if oo is ok_off:
            assert N.lib().ia_index_count_radius(index._h, _p(qq), nq, _p(rr), _p(cnt)) == -1 and (cnt == -7).all()
    with pytest.raises(N.IAError, match='IA_EINVAL'):
        index.count_radius(q, -1.0)
    with pytest.raises(N.IAError):
        algorithms.GpuFLANN(ctx).nn_radius(q[0], 1.0)
    with pytest.raises(RuntimeError):
        flann_mi355x.FLANN().nn_radius(q[0], 1.0)


# ---- 13. the wrappers ----------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['rand_c1', 'rand_c3'])
def test_wrappers_on_the_golden_features(ctx, tag):
    """GpuFLANN.nn_radius and flann_mi355x.FLANN().nn_radius on features.npz level 2 with the radius between
    the query's 5th and 6th distance: 5 rows, the first the reference's own pick, all numpy's; max_nn = 2
    truncates"""
    from ia_amd import algorithms, flann_mi355x
    g = np.load(os.path.join(GOLDEN, 'features.npz'))
    As, Q, nn = g[tag + '_As_2'], g[tag + '_Q_2'], g[tag + '_nn_2']
    sel = np.arange(0, len(Q), max(1, len(Q) // 8))[:8]
    s = np.sort(R.distances(As, Q[sel]), axis=1)
    r = (s[:, 4] + s[:, 5]) / 2
    c_ref, o_ref, i_ref, d_ref = R.radius_reference(As, Q[sel], r)
    a, f = algorithms.GpuFLANN(ctx), flann_mi355x.FLANN()
    try:
        for w in (a, f):
            w.build_index(As, algorithm='kdtree')
            for j, qi in enumerate(sel):
                idx, dist = w.nn_radius(Q[qi], r[j], sorted=True, checks=32)
                assert idx.shape == dist.shape == (5,) and idx.dtype == np.int64 and dist.dtype == np.float64
                assert idx[0] == nn[qi] and np.array_equal(idx, i_ref[o_ref[j]:o_ref[j + 1]])
                assert np.array_equal(dist, d_ref[o_ref[j]:o_ref[j + 1]])
                i2, d2 = w.nn_radius(Q[qi], r[j], max_nn=2)
                assert np.array_equal(i2, idx[:2]) and np.array_equal(d2, dist[:2])
            i9, d9 = w.nn_radius(Q[sel[0]], r[0], max_nn=9)
            assert np.array_equal(i9, i_ref[:5]) and np.array_equal(d9, d_ref[:5])
    finally:
        a.delete_index()
        f.delete_index()


# ---- 14. the certified path is the one that runs -------------------------------------------------
def test_certified_path_runs(index_of):
    """64 queries x 64 rows inside on 70,005 rows: the query verifies the 4,096 rows inside and the few
    within the scan's error bound of the radius (4,099 within r' + 2 eps by a CPU restatement); a brute
    force computes 64 x 70,005.  The counting call verifies the boundary rows only.  Conditions, not
    measurements."""
    index, q = index_of(R.CERT_CASE), K.case(R.CERT_CASE)[1]
    r = R.midpoint(R.CERT_CASE, R.CERT_K)
    index.query_radius(q, r)
    s_query = index.radius_stats()
    index.count_radius(q, r)
    s_count = index.radius_stats()
    print('radius_stats n70005 k=64: query %r, count %r' % (s_query, s_count))
    assert s_query[1] == s_count[1] == 4096
    assert 4096 <= s_query[0] <= 1.25 * 4096
    assert s_count[0] <= 0.25 * 4096

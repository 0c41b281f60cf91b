"""GPU parity of the approximate index (ia_kmeans, ia_ann_*: ia_ann.hip, ia_ann.cpp) with its numpy restatement
(tests/ann_inputs.py) on that file's cases; tests/test_ann_cpu.py pins the cases on the CPU.  Every comparison
is np.array_equal; there is no tolerance anywhere in this file.
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

import ann_inputs as A
import knn_inputs as K

pytestmark = pytest.mark.gpu


def _native():
    import ia_amd  # noqa: F401
    from ia_amd import _native
    return _native


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


_open = {}


@pytest.fixture(scope='module')
def ann_of(ctx):
    """case name -> its AnnIndex, built once per module"""
    def get(name):
        if name not in _open:
            pts, L, iters = A.case(name)
            _open[name] = _native().AnnIndex(ctx, pts, L, iters)
        return _open[name]
    yield get
    for a in _open.values():
        a.close()
    _open.clear()


def _check_build(name, centers, assign, run, sizes, rows):
    C, a, r, s, rw = A.reference(name)
    assert run == r
    if assign is not None:
        assert assign.dtype == np.int32 and np.array_equal(assign, a)
    assert np.array_equal(centers, C)
    if sizes is not None:
        assert sizes.dtype == np.int64 and rows.dtype == np.int32
        assert np.array_equal(sizes, s) and np.array_equal(rows, rw)


# ---- 1. k-means and the lists ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', A.GPU_CASES + A.QUERY_SIZE_CASES)
def test_kmeans_and_lists(ctx, ann_of, name):
    """ia_kmeans and ia_ann_build + ia_ann_lists: the centres, assign, iters_run, sizes and rows of the numpy rule
    (u3000: every iteration; d3: the early exit and sums of fewer than 8 terms; each: one row per list; dups:
    equal centres, empty lists; w150 / w167: the split pairwise sum; u3000_it0: no iteration; n20000: 105
    workgroups of 192 rows; QUERY_SIZE_CASES - L4096: lists of 1 .. 7 rows, every remainder of k_ann_update's
    unroll by 4, and 256 blocks of centres in k_ann_assign; d1: one column; dupwide: 400 equal rows a centre)"""
    pts, L, iters = A.case(name)
    centers, assign, run = _native().kmeans(ctx, pts, L, iters)
    _check_build(name, centers, assign, run, None, None)
    index = ann_of(name)
    centers, sizes, rows = index.lists()
    _check_build(name, centers, None, index.stats()[2], sizes, rows)


@pytest.mark.parametrize('s', A.UNITS_LOG2)
def test_units(ctx, s):
    """u3000 scaled by 2^-80 / 2^70: the lists of scale 1, the centres times 2^s, the distances times 4^s"""
    name = 'u3000@%d' % s
    pts, L, iters = A.case(name)
    centers, assign, run = _native().kmeans(ctx, pts, L, iters)
    _check_build(name, centers, assign, run, None, None)
    assert np.array_equal(assign, A.reference('u3000')[1])
    index = _native().AnnIndex(ctx, pts, L, iters)
    try:
        centers, sizes, rows = index.lists()
        _check_build(name, centers, None, index.stats()[2], sizes, rows)
        assert np.array_equal(rows, A.reference('u3000')[4]) and np.array_equal(centers, A.reference('u3000')[0] * 2.0 ** s)
        idx, dist = index.query(A.queries('u3000') * 2.0 ** s, 5, 256)
    finally:
        index.close()
    i0, d0, _, _ = A.query_reference('u3000', 5, 256)
    assert np.array_equal(idx, i0) and np.array_equal(dist, d0 * 4.0 ** s)


# ---- 2. queries --------------------------------------------------------------------------------------------
def _check_query(index, name, k, checks, nq=64):
    i_ref, d_ref, taken, probed = A.query_reference(name, k, checks, nq)
    idx, dist = index.query(A.queries(name, nq), k, checks)
    assert idx.shape == dist.shape == i_ref.shape and idx.dtype == np.int64 and dist.dtype == np.float64
    bad = np.flatnonzero((idx != i_ref).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:3], idx[bad[:3]], i_ref[bad[:3]])
    assert np.array_equal(dist, d_ref)
    assert index.stats()[:2] == (int(taken.sum()), int(probed.sum()))
    return idx, dist


@pytest.fixture(scope='module')
def exact_blobs(ctx):
    index = _native().ExactIndex(ctx, A.case('blobs')[0])
    yield index
    index.close()


@pytest.mark.parametrize('k', A.K_QUERY)
@pytest.mark.parametrize('checks', A.CHECKS_LADDER)
def test_query_blobs(ann_of, exact_blobs, checks, k):
    """64 queries (half exact rows: distance 0) over the checks ladder and k = 1, 5, 64: idx, dist and the
    statistics of the numpy rule; checks >= n and -1 are the exact index's answer as well"""
    idx, dist = _check_query(ann_of('blobs'), 'blobs', k, checks)
    if checks in (20000, -1):
        i_ex, d_ex = exact_blobs.query_knn(A.queries('blobs'), k)
        assert np.array_equal(idx, i_ex) and np.array_equal(dist, d_ex)
        assert (dist[:32, 0] == 0).all()


def test_empty_and_tiny_lists(ann_of):
    """dups, k = 3: checks = 1 ends inside the first list; at checks = 33, 64 and 200 the probe order crosses
    empty lists (tests/test_ann_cpu.py pins how many queries do), rows taken and lists probed as the numpy
    rule counts them; each, k = 5, checks = 1: need = k, so five one-row lists are probed"""
    for checks in A.DUPS_CHECKS:
        _check_query(ann_of('dups'), 'dups', A.DUPS_K, checks)
    _check_query(ann_of('each'), 'each', 5, 1)
    assert ann_of('each').stats()[:2] == (5 * 64, 5 * 64)


_exact = {}


@pytest.fixture(scope='module')
def exact_of(ctx):
    """case name -> its ExactIndex, built once per module"""
    def get(name):
        if name not in _exact:
            _exact[name] = _native().ExactIndex(ctx, A.case(name)[0])
        return _exact[name]
    yield get
    for a in _exact.values():
        a.close()
    _exact.clear()


@pytest.mark.parametrize('name,k,checks,exact', A.QUERY_SIZE_RUNS, ids=['%s-k%d-c%d' % r[:3] for r in A.QUERY_SIZE_RUNS])
def test_query_sizes(ann_of, exact_of, name, k, checks, exact):
    """the sizes at which k_ann_query's loops take another trip (tests/test_ann_cpu.py pins each): L4096 - the full
    4,096-entry sort area, 8 strided trips of the sort, a prefix over up to 1,003 lists; L1000 - 24 padding slots,
    two trips, a prefix that stops in its second block of 64 lists (checks 600) and in its third or fourth (1500);
    L300 - exactly one full trip of 256 pairs and two of the fill; queries at widths 112, 150, 167, 3 and 1;
    dupwide - k = 64 cuts a group of about 400 rows at one distance that stand on every wave and lane, so the
    merge of the four waves' lists decides by the row index alone.  checks = -1 is the exact index's answer too."""
    nq = A.DUPWIDE_NQ if name == 'dupwide' else 64
    idx, dist = _check_query(ann_of(name), name, k, checks, nq)
    if exact:
        i_ex, d_ex = exact_of(name).query_knn(A.queries(name), k)
        assert np.array_equal(idx, i_ex) and np.array_equal(dist, d_ex)
    if name == 'dupwide':
        assert (dist[:6] == 0).all() and (dist == dist[:, :1]).all() and (np.diff(idx, axis=1) > 0).all()


def test_batches(ann_of):
    """4097 queries: two batches, the second of one query; nq = 0 is IA_OK and writes nothing"""
    N = _native()
    index = ann_of('u3000')
    _check_query(index, 'u3000', 3, 200, nq=4097)
    out = np.full(4, -7, dtype=np.int64)
    q = np.zeros((1, 55))
    assert N.lib().ia_ann_query(index._h, _vp(q), 0, 3, 32, _vp(out), None) == 0 and (out == -7).all()
    assert index.stats()[:2] == (0, 0)


def test_reuse_across_k_and_checks(ann_of):
    """one index, (k, checks) = (64, -1), (2, 32), (16, 256) in that order (result buffers sized by the first
    call): no state carries over; dist_out = NULL returns the same indices"""
    N = _native()
    index = ann_of('u3000')
    for k, checks in ((64, -1), (2, 32), (16, 256)):
        _check_query(index, 'u3000', k, checks)
    q = np.ascontiguousarray(A.queries('u3000'))
    only_idx = np.full((len(q), 16), -7, dtype=np.int64)
    N.check(N.lib().ia_ann_query(index._h, _vp(q), len(q), 16, 256, _vp(only_idx), None), 'ia_ann_query')
    assert np.array_equal(only_idx, A.query_reference('u3000', 16, 256)[0])


# ---- 3. the drop-ins ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['flann_mi355x', 'GpuFLANN'])
def test_drop_ins(ctx, which):
    from ia_amd import algorithms, flann_mi355x
    N = _native()
    w = flann_mi355x.FLANN() if which == 'flann_mi355x' else algorithms.GpuFLANN(ctx)
    err = RuntimeError if which == 'flann_mi355x' else N.IAError
    pts = A.case('u3000')[0]
    Q = A.queries('u3000')
    try:
        params = w.build_index(pts, algorithm='kmeans', n_lists=32, iterations=5)
        assert params == {'algorithm': 'kmeans', 'checks': 32, 'n_lists': 32, 'iterations': 5, 'exact': False}
        idx, dist = w.nn_index(Q, 5, checks=256)
        i_ref, d_ref, _, _ = A.query_reference('u3000', 5, 256)
        assert np.array_equal(idx, i_ref) and np.array_equal(dist, d_ref)
        idx, dist = w.nn_index(Q, 5)     # the checks of the build
        i_ref, d_ref, _, _ = A.query_reference('u3000', 5, 32)
        assert np.array_equal(idx, i_ref) and np.array_equal(dist, d_ref)
        i_ex, d_ex = K.knn_reference(pts, Q, 1)
        i1, d1 = w.nn_index(Q, 1, checks=-1)
        assert i1.shape == d1.shape == (len(Q),) and np.array_equal(i1, i_ex[:, 0]) and np.array_equal(d1, d_ex[:, 0])
        with pytest.raises(err, match="algorithm='linear'"):
            w.nn_radius(Q[0], 1.0)
        assert np.array_equal(w.kmeans(pts, 32, 5), A.reference('u3000')[0])
        assert np.array_equal(w.kmeans(pts, 32, branching=16), A.reference('u3000')[0])   # None: 5 iterations
        assert w.kmeans(pts, 32, 5, dtype=np.float32).dtype == np.float32
        params = w.build_index(pts, algorithm='kdtree')     # exact again, checks ignored
        assert params['algorithm'] == 'kdtree' and params.get('exact', True)
        i5, d5 = w.nn_index(Q, 5, checks=1)
        i_ex, d_ex = K.knn_reference(pts, Q, 5)
        assert np.array_equal(i5, i_ex) and np.array_equal(d5, d_ex)
        assert len(w.nn_radius(Q[0], 1e-9)[0]) == 1          # the exact hit alone
    finally:
        w.delete_index()


# ---- 4. refusals -------------------------------------------------------------------------------------------
def test_refusals(ctx, ann_of):
    """a NaN row at build, an inf query value and each range error: IA_EINVAL, outputs prefilled with -7
    untouched; the same index and the session's context answer afterwards"""
    N = _native()
    L = N.lib()
    index = ann_of('u3000')
    pts = np.array(A.case('u3000')[0])
    n, d = pts.shape
    bad = pts.copy()
    bad[17, 3] = np.nan
    huge = pts.copy()
    huge[17, 3] = -1e154      # finite, beyond IA_ANN_MAX_ABS = 2^500: its squared distances would overflow
    cent = np.full((32, d), -7.0)
    asg = np.full(n, -7, dtype=np.int32)
    run = ctypes.c_int(-7)
    h = ctypes.c_void_p()
    for p, lists, iters in ((bad, 32, 5), (huge, 32, 5), (pts, 0, 5), (pts, n + 1, 5), (pts, 4097, 5), (pts, 32, -1)):
        assert L.ia_kmeans(ctx.handle, _vp(p), n, d, lists, iters, _vp(cent), _vp(asg), ctypes.byref(run)) == -1
        assert b'ia_kmeans' in L.ia_last_error()
        assert L.ia_ann_build(ctx.handle, _vp(p), n, d, lists, iters, ctypes.byref(h)) == -1
        assert b'ia_ann_build' in L.ia_last_error()
        assert (cent == -7).all() and (asg == -7).all() and run.value == -7 and not h
    small = np.zeros((3, 168))
    assert L.ia_ann_build(ctx.handle, _vp(small), 3, 168, 1, 5, ctypes.byref(h)) == -1 and not h
    with pytest.raises(N.IAError, match='IA_EINVAL'):
        N.AnnIndex(ctx, bad, 32)
    q = np.ascontiguousarray(A.queries('u3000'))
    qinf = q.copy()
    qinf[5, 3] = np.inf
    qhuge = q.copy()
    qhuge[5, 3] = 1e154
    tiny = ann_of('each')    # 100 rows: k = 64 fits, 101 rows do not exist
    for a, qq, k, checks in ((index, qinf, 5, 32), (index, qhuge, 5, 32), (index, q, 0, 32), (index, q, 65, 32), (index, q, 5, 0),
                             (index, q, 5, -2), (ann_of('one'), q, 2, 32)):
        i_out = np.full((len(q), 65), -7, dtype=np.int64)
        d_out = np.full((len(q), 65), -7.0)
        assert L.ia_ann_query(a._h, _vp(qq), len(qq), k, checks, _vp(i_out), _vp(d_out)) == -1
        assert b'ia_ann_query' in L.ia_last_error()
        assert (i_out == -7).all() and (d_out == -7.0).all(), (k, checks)
    assert tiny.query(A.queries('each'), 64, 1)[0].shape == (64, 64)
    _check_query(index, 'u3000', 5, 32)
    assert len(index.build_ms()) == 4 and min(index.build_ms()) >= 0
    centers, _, run = N.kmeans(ctx, A.case('each')[0], 100, 2)
    assert run == 1 and np.array_equal(centers, A.reference('each')[0])

"""The approximate index's entry points exist and refuse bad arguments without a GPU, and the numpy
restatement of its rule (tests/ann_inputs.py) and each of its cases is what it claims to be.  No GPU.

These are conditions on the inputs, not measurements: a generator that misses one is changed (or reseeded),
never the condition.
"""
import ctypes

import numpy as np
import pytest

import ann_inputs as A
import knn_inputs as K

SYMBOLS = ('ia_kmeans', 'ia_ann_build', 'ia_ann_lists', 'ia_ann_query', 'ia_ann_stats', 'ia_ann_destroy',
           'ia_ann_build_ms')   # the issue's six and the build's phase clocks (tools/ann_timing.py)


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_ann_symbols_and_refusals():
    """the symbols are bound from EXPORTS; a NULL or out-of-range argument answers IA_EINVAL before any HIP
    call (no GPU here, and a NULL context besides), names the entry point and its range, and writes nothing"""
    import ia_amd  # noqa: F401
    from ia_amd import _native
    L = _native.lib()
    for name in SYMBOLS:
        assert name in _native.EXPORTS and hasattr(L, name), name
    assert L.ia_version() == 4
    assert _native.ANN_MAX_LISTS == A.ANN_MAX_LISTS == 4096 and _native.KNN_MAX == 64
    n, d = 10, 4
    pts = np.random.RandomState(1).rand(n, d)
    wide = np.zeros((n, 168))
    cent = np.full((n + 1, 168), -7.0)
    asg = np.full(n, -7, dtype=np.int32)
    run = ctypes.c_int(-7)
    h = ctypes.c_void_p()
    # (rows, d, lists, iters, words of the message); the context is NULL throughout
    for p, dd, lists, iters, words in ((pts, d, 0, 5, b'1..10'), (pts, d, n + 1, 5, b'1..10'), (pts, d, 2, -1, b'iters'),
                                       (wide, 168, 2, 5, b'1..167'), (pts, d, 2, 5, b'NULL')):
        rc = L.ia_kmeans(None, _vp(p), n, dd, lists, iters, _vp(cent), _vp(asg), ctypes.byref(run))
        assert rc == -1 and b'ia_kmeans' in L.ia_last_error() and words in L.ia_last_error(), (lists, iters, dd)
        rc = L.ia_ann_build(None, _vp(p), n, dd, lists, iters, ctypes.byref(h))
        assert rc == -1 and b'ia_ann_build' in L.ia_last_error() and words in L.ia_last_error(), (lists, iters, dd)
        assert (cent == -7).all() and (asg == -7).all() and run.value == -7 and not h
    q = np.zeros((1, d))
    idx = np.full(65, -7, dtype=np.int64)
    dist = np.full(65, -7.0)
    for k, checks, words in ((0, 32, b'k must be 1..'), (65, 32, b'k must be 1..'), (3, 0, b'checks must be -1'),
                             (3, -2, b'checks must be -1'), (3, 32, b'NULL')):
        rc = L.ia_ann_query(None, _vp(q), 1, k, checks, _vp(idx), _vp(dist))
        assert rc == -1 and b'ia_ann_query' in L.ia_last_error() and words in L.ia_last_error(), (k, checks)
        assert (idx == -7).all() and (dist == -7).all()
    assert L.ia_ann_lists(None, None, None, None) == -1 and b'ia_ann_lists' in L.ia_last_error()
    assert L.ia_ann_stats(None, (ctypes.c_int64 * 3)()) == -1 and b'ia_ann_stats' in L.ia_last_error()
    ms = (ctypes.c_double * 4)(-7, -7, -7, -7)
    assert L.ia_ann_build_ms(None, ms) == -1 and b'ia_ann_build_ms' in L.ia_last_error() and list(ms) == [-7] * 4
    L.ia_ann_destroy(None)
    assert [_native.default_n_lists(v) for v in (1, 3, 4, 3000, 1 << 20, 1 << 30)] == [1, 1, 2, 54, 1024, 4096]


@pytest.mark.parametrize('name', ['u3000', 'dups', 'd3'])
def test_assign_is_the_per_row_rule(name):
    """argmin over the per-centre ((pts - c) ** 2).sum(1) columns is the per-row lexsort on (dist, centre), on
    the initial centres (equal ones among them on dups) and on the final ones"""
    pts, L, _ = A.case(name)
    pts = pts[:400]
    for C in (pts[[c * len(pts) // L for c in range(L)]], A.reference(name)[0]):
        assert np.array_equal(A.assign_ref(pts, C), A.assign_per_row(pts, C))


@pytest.mark.parametrize('name', A.GPU_CASES + A.QUERY_SIZE_CASES)
def test_every_row_sits_with_its_nearest_centre(name):
    """a == assign(C) on the returned centres; the lists partition the rows, each ascending"""
    pts, L, _ = A.case(name)
    C, a, run, sizes, rows = A.reference(name)
    assert np.array_equal(a, A.assign_ref(pts, C))
    assert sizes.sum() == len(pts) and np.array_equal(np.sort(rows), np.arange(len(pts)))
    off = np.concatenate(([0], np.cumsum(sizes)))
    for c in range(L):
        r = rows[off[c]:off[c + 1]]
        assert (a[r] == c).all() and (np.diff(r) > 0).all()


def test_case_claims():
    """what each case is there for (tests/test_gpu_ann.py)"""
    _, _, run, sizes, _ = A.reference('u3000')
    assert run == 5 and sizes.min() > 0                      # every iteration, no empty list
    print('u3000 sizes %d..%d' % (sizes.min(), sizes.max()))
    assert A.case('d3')[0].shape == (5000, 3)                # the n < 8 branch of the pairwise sum
    run = A.reference('d3')[2]
    assert 2 <= run < 50                                     # the a == prev exit
    print('d3 stops after %d iterations' % run)
    _, a, run, sizes, _ = A.reference('each')
    assert run == 1 and (sizes == 1).all() and np.array_equal(a, np.arange(100))
    pts, L, _ = A.case('dups')
    C0 = pts[[c * len(pts) // L for c in range(L)]]
    assert len(np.unique(pts, axis=0)) == 40 and len(np.unique(C0, axis=0)) < L   # exact centre ties
    sizes = A.reference('dups')[3]
    assert (sizes == 0).sum() >= 1
    print('dups: %d empty lists, largest %d' % ((sizes == 0).sum(), sizes.max()))
    assert A.reference('u3000_it0')[2] == 0 and np.array_equal(A.reference('u3000_it0')[0], A.case('u3000')[0][
        [c * 3000 // 32 for c in range(32)]])
    assert A.reference('one')[3].tolist() == [1]
    assert [A.case(n)[0].shape[1] for n in ('w112', 'w150', 'w167')] == [112, 150, 167]   # 150, 167: the split sum
    assert A.case('n20000')[0].shape == (20000, 55) and A.reference('n20000')[2] == 3


def _probed(name, k, checks, nq=64):
    _, _, taken, probed = A.query_reference(name, k, checks, nq)
    print('%s (%d, %d): lists probed %d..%d, rows taken %d..%d' % (name, k, checks, probed.min(), probed.max(), taken.min(),
                                                                   taken.max()))
    return probed


def test_query_size_case_claims():
    """what each case of QUERY_SIZE_CASES is there for: the loops of k_ann_query that GPU_CASES' at most 128 lists
    run once or not at all (P = the lists rounded up to a power of two: the sort area)"""
    P = lambda L: 1 << (L - 1).bit_length()
    assert set(A.QUERY_SIZE_CASES) <= set(A.CASES) and not set(A.QUERY_SIZE_CASES) & set(A.GPU_CASES)
    assert {n for n, _, _, _ in A.QUERY_SIZE_RUNS} == set(A.QUERY_SIZE_CASES) | {'w112', 'w150', 'w167', 'd3'}
    # L4096: the full sort area; lists of 1 .. 8 rows, so k_ann_update's unroll by 4 sees every remainder
    pts, L, iters = A.case('L4096')
    _, _, run, sizes, _ = A.reference('L4096')
    assert pts.shape == (8192, 8) and L == P(L) == A.ANN_MAX_LISTS == 4096 and iters == 2 and run <= 2
    assert 1 <= sizes.min() and sizes.max() <= 8 and all((sizes == s).any() for s in (1, 2, 3, 4, 5)) and (sizes >= 6).any()
    assert {(int(s) - 1) % 4 for s in np.unique(sizes)} == {0, 1, 2, 3}       # the rows after a list's first, mod 4
    assert (_probed('L4096', 1, 1) >= 1).all()
    p = _probed('L4096', 5, 64)
    assert (p > 16).all()
    p = _probed('L4096', 64, 2000)
    assert (p > 512).all() and (p < L).all()
    assert (_probed('L4096', 3, -1) == L).all()
    # L1000: P = 1,024 with 24 padding slots; 512 pairs: two strided trips of the sort
    pts, L, iters = A.case('L1000')
    assert pts.shape == (6000, 24) and (L, P(L), iters) == (1000, 1024, 3) and P(L) // 2 == 2 * 256
    p = _probed('L1000', 5, 600)
    assert (p > 64).all() and (p <= 128).all()                                # the prefix stops inside its second block
    p = _probed('L1000', 64, 1500)
    assert (p > 128).all() and (p < L).all()                                  # third block or later: cum carried twice
    assert (_probed('L1000', 5, -1) == L).all()
    # L300: P = 512: one full trip of 256 pairs, two trips of the fill
    pts, L, iters = A.case('L300')
    assert pts.shape == (3000, 55) and (L, P(L)) == (300, 512) and P(L) // 2 == 256 and P(L) == 2 * 256
    p = _probed('L300', 5, 1500)
    assert (p > 64).all() and (p < L).all()
    # the widths
    assert [A.case(n)[0].shape[1] for n in ('w112', 'w150', 'w167', 'd3', 'd1')] == [112, 150, 167, 3, 1]
    assert A.case('d1')[0].shape == (500, 1) and A.case('d1')[1] == 10
    for name in ('w112', 'w150', 'w167', 'd3', 'd1'):
        assert (name, 5, 64, False) in A.QUERY_SIZE_RUNS and (name, 5, -1, True) in A.QUERY_SIZE_RUNS
        assert (_probed(name, 5, -1) == A.case(name)[1]).all()


@pytest.mark.parametrize('name,k', [('L4096', 3), ('L1000', 5), ('w112', 5), ('w150', 5), ('w167', 5), ('d3', 5), ('d1', 5)])
def test_query_size_unlimited_checks_is_the_exact_knn(name, k):
    i_ref, d_ref = K.knn_reference(A.case(name)[0], A.queries(name), k)
    idx, dist, taken, _ = A.query_reference(name, k, -1)
    assert np.array_equal(idx, i_ref) and np.array_equal(dist, d_ref) and (taken == len(A.case(name)[0])).all()


def test_dupwide_ties_cut_through_the_waves():
    """2,400 rows, 6 distinct, three lists of two of them each: a query's distance is shared by the about 400 copies
    of a row, which stand at every second position of their list or so, i.e. on every wave and lane of
    k_ann_query's stride; k = 64 cuts that group, so the answer is its 64 lowest row indices, which no wave holds
    alone.  (Copies of one row share one list, so at checks = 1000 the second list adds farther rows only.)"""
    pts, L, iters = A.case('dupwide')
    _, a, run, sizes, rows = A.reference('dupwide')
    assert pts.shape == (2400, 55) and (L, iters) == (3, 2) and len(np.unique(pts, axis=0)) == 6
    print('dupwide lists', sizes.tolist(), 'iterations', run)
    assert (sizes >= 700).all() and (sizes <= 900).all()
    assert all(len(np.unique(pts[a == c], axis=0)) == 2 for c in range(3))
    q = A.queries('dupwide', A.DUPWIDE_NQ)
    assert q.shape == (32, 55) and np.array_equal(np.unique(q[:6], axis=0), np.unique(pts, axis=0))
    for checks, lists in ((1, 1), (1000, 2)):
        idx, dist, taken, probed = A.query_reference('dupwide', 64, checks, A.DUPWIDE_NQ)
        assert (probed == lists).all()
        for j, (r, dd, pos, which) in enumerate(A.taken_rows('dupwide', 64, checks, A.DUPWIDE_NQ)):
            o = np.lexsort((r, dd))
            assert dd[o[63]] == dd[o[64]] and (dd == dd[o[0]]).sum() >= 350        # the 64th and 65th candidates tie
            assert np.array_equal(idx[j], r[o[:64]]) and (np.diff(idx[j]) > 0).all() and (dist[j] == dd[o[0]]).all()
            assert len(set(((pos[o[:64]] // 64) % 4).tolist())) > 1                 # not one wave's stride
            assert (which[o[:64]] == 0).all()
            if j < 6:                                                               # a distinct row itself
                assert dd[o[0]] == 0 and np.array_equal(r[o[:64]], np.flatnonzero((pts == q[j]).all(axis=1))[:64])


def test_dups_queries_cross_empty_lists():
    """Equal centres tie on every distance; the lowest index holds their rows and also sorts first, so the empty
    copies follow it at once in every probe order.  checks = 1 (need = k = 3) therefore ends inside the first
    list and crosses none - that follows from the rule, for any rows; a query crosses empty lists as soon as need
    exceeds its first list: many queries at checks = 33 and 64, every query at checks = 200"""
    sizes = A.reference('dups')[3]
    assert A.DUPS_K == 3 and A.DUPS_CHECKS == (1, 33, 64, 200)
    crossing = {}
    for checks in A.DUPS_CHECKS:
        orders = A.probed_lists('dups', A.DUPS_K, checks)
        taken, probed = A.query_reference('dups', A.DUPS_K, checks)[2:]
        assert [len(o) for o in orders] == probed.tolist() and [int(sizes[o].sum()) for o in orders] == taken.tolist()
        # an empty list strictly inside the order: rows are taken before it and after it
        crossing[checks] = sum(1 for o in orders if (sizes[o[1:-1]] == 0).any())
        print('dups checks %d: %d of 64 queries cross an empty list, up to %d lists probed'
              % (checks, crossing[checks], probed.max()))
    assert all(len(o) == 1 and sizes[o[0]] >= 3 for o in A.probed_lists('dups', A.DUPS_K, 1))
    assert crossing[1] == 0 and crossing[33] >= 16 and crossing[64] >= 32 and crossing[200] == 64


def test_blobs_cross_their_empty_list_when_every_row_is_taken():
    """blobs has an empty list, which checks = 20000 and -1 cross on every query"""
    sizes = A.reference('blobs')[3]
    assert (sizes == 0).sum() >= 1
    for checks in (20000, -1):
        assert all((sizes[o[:-1]] == 0).any() for o in A.probed_lists('blobs', 1, checks))


def test_blobs_take_less_than_one_list_too_many():
    """per query the rows taken exceed need = max(checks, k) by less than the last list taken; the means stay
    below the next larger checks plus the largest list"""
    sizes = A.reference('blobs')[3]
    ladder = (1, 256, 1024, 4096)
    means = []
    for checks in ladder:
        _, _, taken, probed = A.query_reference('blobs', 1, checks)
        assert (taken >= checks).all() and (taken < checks + sizes.max()).all() and (probed >= 1).all()
        means.append(taken.mean())
        print('blobs checks %d: mean rows taken %.1f, lists probed %.2f' % (checks, taken.mean(), probed.mean()))
    for m, nxt in zip(means, ladder[1:]):
        assert m < nxt + sizes.max()
    q = A.queries('blobs')
    assert np.array_equal(q[:32], A.case('blobs')[0][np.random.RandomState(21).randint(0, 20000, 64)[:32]])


@pytest.mark.parametrize('k', A.K_QUERY)
def test_unlimited_checks_is_the_exact_knn(k):
    """checks = -1 and checks >= n take every row: knn_inputs.knn_reference bit for bit, distance 0 in front"""
    pts = A.case('blobs')[0]
    i_ref, d_ref = K.knn_reference(pts, A.queries('blobs'), k)
    for checks in (-1, 20000):
        idx, dist, taken, probed = A.query_reference('blobs', k, checks)
        assert np.array_equal(idx, i_ref) and np.array_equal(dist, d_ref)
        assert (taken == 20000).all() and (probed <= 128).all()
    assert (d_ref[:32, 0] == 0).all()


@pytest.mark.parametrize('k', A.K_QUERY)
def test_monotone_in_checks(k):
    """a larger checks takes a superset of the rows: the j-th returned distance never grows"""
    prev = None
    for checks in A.CHECKS_LADDER:
        _, dist, taken, _ = A.query_reference('blobs', k, checks)
        if prev is not None:
            assert (dist <= prev[0]).all() and (taken >= prev[1]).all()
        prev = (dist, taken)


@pytest.mark.parametrize('s', A.UNITS_LOG2)
def test_units(s):
    """u3000 scaled by 2^s: the same assignment and lists, the centres times 2^s, the distances times 4^s"""
    C0, a0, run0, sizes0, rows0 = A.reference('u3000')
    C, a, run, sizes, rows = A.reference('u3000@%d' % s)
    assert np.array_equal(a, a0) and run == run0 and np.array_equal(sizes, sizes0) and np.array_equal(rows, rows0)
    assert np.array_equal(C, C0 * 2.0 ** s)
    i0, d0, t0, p0 = A.query_reference('u3000', 5, 256)
    pts = A.case('u3000@%d' % s)[0]
    i, d, t, p = A.query_ref(pts, C, sizes, rows, A.queries('u3000') * 2.0 ** s, 5, 256)
    assert np.array_equal(i, i0) and np.array_equal(d, d0 * 4.0 ** s) and np.array_equal(t, t0) and np.array_equal(p, p0)

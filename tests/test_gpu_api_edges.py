"""GPU parity of the C ABI off the level path on the cases of tests/api_edge_inputs.py:
ia_index_build / ia_index_query (ia_index.cpp, ia_dense.hip, certified_winner), ia_coherence_batch
(k_coherence_batch), ia_gaussian_pyramid / ia_color_matrix (ia_pyramid.hip).  Each test names the
code path it executes and why its size reaches it; tests/test_api_edge_inputs_cpu.py pins that on
the CPU.  Every comparison is bit for bit with a plain fp64 reference (numpy, the oracle, the
package's host restatement); there is no tolerance anywhere in this file.
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

import api_edge_inputs as E

pytestmark = pytest.mark.gpu


def _native():
    import ia_amd  # noqa: F401
    from ia_amd import _native
    return _native


# ---- 1. the exact index against numpy fp64 -----------------------------------------------------
def _check_index(ctx, pts, q):
    idx = _native().ExactIndex(ctx, pts)
    try:
        i_gpu, d_gpu = idx.query(q)
    finally:
        idx.close()
    i_ref, d_ref = E.index_reference(pts, q)
    bad = np.flatnonzero(i_gpu != i_ref)
    assert len(bad) == 0, (len(bad), bad[:5], i_gpu[bad[:5]], i_ref[bad[:5]])
    assert np.array_equal(d_gpu, d_ref)


@pytest.mark.parametrize('name', ['n10000', 'n65536', 'n70005', 'n70005_neartie'])
def test_index_chunk_shapes(ctx, name):
    """certified_winner's records per lane and k_merge_dense's chunk rescans (RPL = 8 records per
    lane, one record per workgroup): n = 10,000 has 313 tiles on nwg = 79 workgroups, so lanes 0..14
    hold two records; 65,536 fills all 512 (tpw 4, 8 records on every lane); 70,005 has tpw = 5 on
    438 workgroups, a last chunk of 3 tiles and a last tile of 21 rows; the near-tie case makes
    every query rerank and rescan chunks through ia_pos_row at that shape (40 rows within 2^-20
    of the winner, decided in fp64).  No index of the suite had more than 40 workgroups before."""
    _check_index(ctx, *E.INDEX_CASES[name]())


@pytest.mark.parametrize('name', ['nq4096', 'nq4097', 'nq8200'])
def test_index_query_batches(ctx, name):
    """ia_index_query's batch loop (BATCH = 4,096): 4,096 queries are one full batch, 4,097 a second
    batch of one query, 8,200 two full ones and a partial: the q + b0 * d and idx_out + b0 offsets"""
    _check_index(ctx, *E.INDEX_CASES[name]())


@pytest.mark.parametrize('name', ['d55_nq353', 'd56_nq161', 'd111_nq200', 'd112_nq97'])
def test_index_query_blocks(ctx, name):
    """the query-block loop (qt0 > 0) of each K3 instance, at the widths where kh_for(d + 1) switches:
    d = 55 (KH 28, 11 tiles per launch) with 353 queries = 11 + 1 tiles; d = 56 and 111 (KH 56, 5
    per launch) with 161 = 5 + 1 and 200 = 5 + 2 tiles; d = 112 (KH 84, 3 per launch) with 97 = 3 + 1"""
    _check_index(ctx, *E.INDEX_CASES[name]())


def test_index_reuse_and_null_dist(ctx):
    """one index queried with 4,200, 3 and 400 rows (its buffers are sized by the first call; the
    later ones use a part of them) answers as a fresh index does; dist_out = NULL returns the same
    indices"""
    N = _native()
    pts, qs = E.reuse_index()
    idx = N.ExactIndex(ctx, pts)
    try:
        got = [idx.query(q) for q in qs]
        q = np.ascontiguousarray(qs[2])
        only_idx = np.full(len(q), -7, dtype=np.int64)
        N.check(N.lib().ia_index_query(idx._h, ctypes.c_void_p(q.ctypes.data), len(q),
                                       ctypes.c_void_p(only_idx.ctypes.data), None), 'ia_index_query')
    finally:
        idx.close()
    for q, (i_gpu, d_gpu) in zip(qs, got):
        fresh = N.ExactIndex(ctx, pts)
        try:
            i_new, d_new = fresh.query(q)
        finally:
            fresh.close()
        i_ref, d_ref = E.index_reference(pts, q)
        assert np.array_equal(i_gpu, i_new) and np.array_equal(d_gpu, d_new)
        assert np.array_equal(i_gpu, i_ref) and np.array_equal(d_gpu, d_ref)
    assert np.array_equal(only_idx, got[2][0])


@pytest.mark.parametrize('log2_scale', E.RANGE_LOG2)
@pytest.mark.parametrize('family', E.RANGE_FAMILIES)
def test_index_value_range(ctx, family, log2_scale):
    """the fp32 scan of the index under a power-of-two scaling of rows and queries: at 2^-70 / 2^-80
    the squares of the caller's values are fp32 subnormals or zero, at 2^62 (float)norm is just below
    FLT_MAX, at 2^63 past it for most rows of 'signed' but not all, at 2^64 and 2^70 for all.  There is
    no range gate and eps_a = 0; ia_index_build prescales the centred fp32 copy by a power of two taken
    from the rows, so the scan never sees those magnitudes.  The index and the distance must be those
    at scale 1 (the distance times 4^k), bit for bit, which is also numpy's answer on the scaled arrays."""
    N = _native()
    pts1, q1 = E.range_index(family)
    i_ref, d_ref = E.index_reference(pts1, q1)
    pts, q = E.range_index(family, log2_scale)
    idx = N.ExactIndex(ctx, pts)
    try:
        i_gpu, d_gpu = idx.query(q)
    finally:
        idx.close()
    bad = np.flatnonzero(i_gpu != i_ref)
    assert len(bad) == 0, (len(bad), bad[:5], i_gpu[bad[:5]], i_ref[bad[:5]])
    assert np.array_equal(d_gpu, d_ref * 4.0 ** log2_scale)
    i_np, d_np = E.index_reference(pts, q[-3:])
    assert np.array_equal(i_gpu[-3:], i_np) and np.array_equal(d_gpu[-3:], d_np)


def test_index_refuses_what_it_cannot_answer_exactly(ctx):
    """rows that are not finite at ia_index_build; at ia_index_query a NaN and a query 2^101 times
    farther from the rows' mean than any row (its prescaled fp32 copy would leave fp32's range, and
    with it the scan's error bound): IA_EINVAL, never a wrong index.  2^30 and 2^99 times are answered."""
    N = _native()
    pts, q = E.range_index('signed')
    for bad in (np.inf, np.nan, 1e308):
        p = pts.copy()
        p[5, 7] = bad
        if bad == 1e308:
            p[6:200, 7] = bad   # finite values, infinite column sum
        with pytest.raises(N.IAError, match='IA_EINVAL'):
            N.ExactIndex(ctx, p)
    idx = N.ExactIndex(ctx, pts)
    try:
        for bad in (np.nan, np.inf, 2.0 ** 101):
            qq = q.copy()
            qq[33, 2] = bad
            with pytest.raises(N.IAError, match='IA_EINVAL'):
                idx.query(qq)
        got = {k: idx.query(q * 2.0 ** k) for k in (30, 99)}
    finally:
        idx.close()
    for k, (i_gpu, d_gpu) in got.items():   # (at 2^99 every row is at the same fp64 distance: index 0)
        i_ref, d_ref = E.index_reference(pts, q * 2.0 ** k)
        assert np.array_equal(i_gpu, i_ref) and np.array_equal(d_gpu, d_ref), k


# ---- 2. ia_coherence_batch against the oracle --------------------------------------------------
def _coherence(ctx, z, pad=2, s=None, im=None):
    idx = _native().ExactIndex(ctx, z['pts'])
    try:
        return idx.coherence(z['q'], z['px'], z['s'] if s is None else s, z['im'] if im is None else im, z['a_hw'],
                             z['b_hw'][1], pad)
    finally:
        idx.close()


def _same(got, ref):
    for k, (a, b) in enumerate(zip(got, ref)):
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert len(bad) == 0, (k, len(bad), bad[:5], a[bad[:5]], b[bad[:5]])


@pytest.mark.parametrize('name', list(E.COHERENCE_CASES))
def test_coherence_batch_matches_oracle(ctx, name):
    """k_coherence_batch on a whole level in one call against oracle.ia_oracle.coherence per pixel,
    on random source maps: A (9 x 7) smaller than B' (16 x 20) so that shifted sources leave A on all
    four sides (the pr0 / pr1 filter) and a pixel other than pixel 0 has no candidate; two A' images at
    d = 110 and 165 (the wider rows of pw_sum_rt); a wide flat A (5 x 40) under a 12 x 9 B'; exact
    distance ties (first argmin = lowest window cell); and planted pixels where an earlier cell has
    the larger sum of squares but the same square root (ranking is by the root, as numpy's norm)."""
    z = E.COHERENCE_CASES[name]()
    _same(_coherence(ctx, z), E.coherence_reference(z, oracle=True))


@pytest.mark.parametrize('pad', [0, 1, 3, 4])
def test_coherence_batch_other_windows(ctx, pad):
    """the window geometry for pad != 2 (lane -> cell with wd = 2 pad + 1, (pad + 1) wd lanes): 3, 15,
    28 and 45 cells; pad = 0 has no raster-earlier cell, so no pixel has a candidate"""
    z = E.COHERENCE_CASES[E.PAD_CASE]()
    got = _coherence(ctx, z, pad)
    _same(got, E.coherence_reference(z, pad))
    if pad == 0:
        assert (got[0] == -1).all() and (got[1] == 0).all() and (got[2] == 0).all()


def test_coherence_batch_refusals(ctx):
    """pad outside 0 .. 4 and a candidate row beyond the index (an im entry of n_ap) are IA_EINVAL"""
    N = _native()
    z = E.COHERENCE_CASES['A25x19_ap2_d110']()
    for pad in (5, -1):
        with pytest.raises(N.IAError, match='IA_EINVAL'):
            _coherence(ctx, z, pad)
    s, im = z['s'].copy(), z['im'].copy()
    s[0] = (0, 0)           # pixel (0, 1)'s candidate (0, 1) of A lies inside A ...
    im[0] = z['n_ap']       # ... of an A' image the index does not hold
    with pytest.raises(N.IAError, match='IA_EINVAL'):
        _coherence(ctx, z, 2, s, im)
    _same(_coherence(ctx, z), E.coherence_reference(z, oracle=True))   # and the index is still usable


# ---- 3. GPU preprocessing against the host restatement -----------------------------------------
def _check_pyramid(ctx, img, n_reduce):
    import ia_amd  # noqa: F401
    from ia_amd import img_preprocess as ip
    gpu = ctx.gaussian_pyramid(img, n_reduce, ip.gaussian_weights())
    ref = E.pyramid_reference(img, n_reduce)
    assert len(gpu) == len(ref) == n_reduce
    for l, (a, b) in enumerate(zip(gpu, ref)):
        assert a.shape == b.shape, (l, a.shape, b.shape)
        assert np.array_equal(a, b), (l, int((a != b).sum()), float(np.abs(a - b).max()))


@pytest.mark.parametrize('shape', E.SMALL_SHAPES, ids=['x'.join(map(str, s)) for s in E.SMALL_SHAPES])
def test_pyramid_small_sides(ctx, shape):
    """ia_gaussian_pyramid called directly with n_reduce = 1 .. 3, so the reductions really run
    (compute_gaussian_pyramid(img, 3) runs none on sides <= 3): sides of 1 .. 3 take ia_reflect's
    periodic branch in k_gauss1d (the 7-tap window is wider than two folds reach) and give 1-pixel
    output sides in k_bilinear_half; ch = 2, 3 and 4 interleaved"""
    img = E.small_image(shape)
    for n in (1, 2, 3):
        _check_pyramid(ctx, img, n)


@pytest.mark.parametrize('shape', E.LARGE_SHAPES, ids=['x'.join(map(str, s)) for s in E.LARGE_SHAPES])
def test_pyramid_grid_stride_second_trip(ctx, shape):
    """py_grid caps a launch at 4,096 x 256 = 1,048,576 threads: 1025 x 1031 = 1,056,775 and
    600 x 601 x 3 = 1,081,800 values make k_gauss1d (both axes) take a second trip of its
    grid-stride loop and k_minmax a seventeenth; 2049 x 2051 reduced once has an output of 1025 x 1026 =
    1,051,650 values, the second trip of k_bilinear_half; the largest image before was 1024^2 = exactly
    one trip"""
    _check_pyramid(ctx, E.large_image(shape), E.LARGE_REDUCE[shape])


@pytest.mark.parametrize('name', list(E.CLIP_CASES))
def test_pyramid_clip_and_values(ctx, name):
    """the clip to the smoothed level's range (k_minmax -> k_minmax_fold -> fmin(fmax(v, lo), hi)):
    on the plateau cases the unclipped bilinear value rounds past the maximum (negated: the minimum),
    so a kernel without the clip, with a wrong fold or with per-channel bounds differs; also a
    constant image, values in [-1e6, 1e6] and 2^-14 rand, and ch = 2 and 4"""
    _check_pyramid(ctx, E.CLIP_CASES[name](), 2)


def test_pyramid_refuses_5_channels(ctx):
    import ia_amd  # noqa: F401
    from ia_amd import img_preprocess as ip
    N = _native()
    with pytest.raises(N.IAError, match='IA_EINVAL'):
        ctx.gaussian_pyramid(np.zeros((8, 8, 5)), 1, ip.gaussian_weights())


def test_color_matrix_signed_and_sizes(ctx):
    """k_color3 with a random signed matrix on values in [-5, 5] (a wrong summation order shows in
    most values); 700 x 600 x 3 = 1,260,000 values take a second grid-stride trip; npx = 1; npx = 0
    returns IA_OK and leaves the output untouched"""
    N = _native()
    for shape in ((33, 47, 3), E.COLOR_LARGE, (1, 1, 3)):
        M, img = E.color_inputs(shape)
        assert np.array_equal(ctx.color_matrix(img, M), E.color_reference(M, img)), shape
    M, img = E.color_inputs()
    out = np.full(6, 123.5)
    N.check(N.lib().ia_color_matrix(ctx.handle, ctypes.c_void_p(img.ctypes.data), 0, ctypes.c_void_p(M.ctypes.data),
                                    ctypes.c_void_p(out.ctypes.data), N.IA_MEM_HOST), 'ia_color_matrix')
    assert (out == 123.5).all()


def test_preprocessing_on_device_memory(ctx):
    """mem = IA_MEM_DEVICE of both entries (no other caller): torch device tensors, in and out
    distinct, 117 x 180 x 3 with n_reduce = 3.  The output equals the host-memory call's bytes, the
    input is unchanged and the guard elements past the end of the output are untouched."""
    import ia_amd  # noqa: F401
    from ia_amd import img_preprocess as ip
    N = _native()
    GUARD, MARK = 8, -12345.0
    dev = torch.device('cuda', ctx.device)
    img = E.device_image()
    w7 = np.ascontiguousarray(ip.gaussian_weights())
    host = ctx.gaussian_pyramid(img, E.DEVICE_REDUCE, w7)
    flat = np.concatenate([x.ravel() for x in host])
    d_in = torch.from_numpy(img).to(dev)
    d_out = torch.full((len(flat) + GUARD,), MARK, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    h, w, ch = img.shape
    N.check(N.lib().ia_gaussian_pyramid(ctx.handle, ctypes.c_void_p(d_in.data_ptr()), h, w, ch, E.DEVICE_REDUCE,
                                        ctypes.c_void_p(w7.ctypes.data), ctypes.c_void_p(d_out.data_ptr()),
                                        N.IA_MEM_DEVICE), 'ia_gaussian_pyramid')
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:len(flat)], flat) and (out[len(flat):] == MARK).all()
    assert np.array_equal(d_in.cpu().numpy(), img)

    M, cimg = E.color_inputs(E.DEVICE_SHAPE)
    host = ctx.color_matrix(cimg, M)
    d_in = torch.from_numpy(cimg).to(dev)
    d_out = torch.full((cimg.size + GUARD,), MARK, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    N.check(N.lib().ia_color_matrix(ctx.handle, ctypes.c_void_p(d_in.data_ptr()), h * w, ctypes.c_void_p(M.ctypes.data),
                                    ctypes.c_void_p(d_out.data_ptr()), N.IA_MEM_DEVICE), 'ia_color_matrix')
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:cimg.size], host.ravel()) and (out[cimg.size:] == MARK).all()
    assert np.array_equal(d_in.cpu().numpy(), cimg)
    assert np.array_equal(host, E.color_reference(M, cimg))

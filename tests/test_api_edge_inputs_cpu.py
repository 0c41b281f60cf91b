"""Each case of tests/api_edge_inputs.py is what it claims to be: it reaches the code path it is
named for (the launch geometry restated from ia_index.cpp / ia_pyramid.hip) and the reference's own
answer on it has the property the GPU test relies on.  No GPU.

These are conditions on the inputs, not measurements: a generator that misses one is changed (or
reseeded), never the condition.
"""
import numpy as np
import pytest

import api_edge_inputs as E


# ---- the exact index ---------------------------------------------------------------------------
def test_index_chunk_shapes():
    """records per lane of certified_winner (8 per lane, 64 lanes): n = 10,000 has 79 workgroups
    (2 records on 15 lanes), 65,536 all 512 at tpw 4, 70,005 tpw 5 with a ragged last chunk and tile"""
    g = E.index_geometry(10000)
    assert (g['n_tiles'], g['tpw'], g['nwg']) == (313, 4, 79)
    g = E.index_geometry(65536)
    assert (g['n_tiles'], g['tpw'], g['nwg'], g['last_chunk'], g['last_rows']) == (2048, 4, 512, 4, 32)
    g = E.index_geometry(70005)
    assert (g['n_tiles'], g['tpw'], g['nwg'], g['last_chunk'], g['last_rows']) == (2188, 5, 438, 3, 21)
    assert E.index_geometry(5000)['nwg'] == 40   # the largest index of the suite before this file
    for name, n in (('n10000', 10000), ('n65536', 65536), ('n70005', 70005), ('n70005_neartie', 70005)):
        pts, q = E.INDEX_CASES[name]()
        assert pts.shape == (n, 55) and q.shape == (64, 55) and pts.dtype == q.dtype == np.float64


def test_index_query_loops():
    """batches of 4,096 queries and scan launches of qtmax query tiles: which cases take a second
    batch, a partial batch, a second launch"""
    assert E.query_blocks(4096, 8) == [[11] * 11 + [7]]
    assert E.query_blocks(4097, 8) == [[11] * 11 + [7], [1]]
    assert E.query_blocks(8200, 8) == [[11] * 11 + [7]] * 2 + [[1]]
    assert E.query_blocks(353, 55) == [[11, 1]]      # KH 28
    assert E.query_blocks(161, 56) == [[5, 1]]       # KH 56, its first width
    assert E.query_blocks(200, 111) == [[5, 2]]      # KH 56, its last width
    assert E.query_blocks(97, 112) == [[3, 1]]       # KH 84, its first width
    assert [E.index_geometry(700, d)['KH'] for d in (55, 56, 111, 112)] == [28, 56, 56, 84]
    for name, (n, d, nq) in dict(nq4096=(100, 8, 4096), nq4097=(100, 8, 4097), nq8200=(100, 8, 8200),
                                 d55_nq353=(700, 55, 353), d56_nq161=(700, 56, 161), d111_nq200=(700, 111, 200),
                                 d112_nq97=(700, 112, 97)).items():
        pts, q = E.INDEX_CASES[name]()
        assert pts.shape == (n, d) and q.shape == (nq, d)
        h = min(n, nq) // 2
        assert np.array_equal(q[:h], pts[:h]) and not np.array_equal(q[h], pts[h])
    pts, qs = E.reuse_index()
    assert [len(q) for q in qs] == [4200, 3, 400] and len(E.query_blocks(4200, 55)) == 2


def test_index_neartie_case():
    """as test_exact_index_near_duplicates_are_decided_in_fp64: >= 40 rows within REL_TIE of the
    winner, no exact tie, the winner mostly not the lowest index"""
    pts, q = E.INDEX_CASES['n70005_neartie']()
    not_lowest = 0
    for j in range(len(q)):
        dd = ((pts - q[j]) ** 2).sum(axis=1)
        i = int(np.argmin(dd))
        near = np.flatnonzero(dd <= dd[i] * (1 + E.REL_TIE))
        assert len(near) >= 40 and (dd == dd[i]).sum() == 1
        not_lowest += int(near[0] != i)
    assert not_lowest > len(q) // 2


@pytest.mark.parametrize('family', E.RANGE_FAMILIES)
def test_index_range_reference_is_scale_invariant(family):
    """the numpy reference stays finite at 2^-80 ... 2^70 and scales exactly: the same argmin, the
    distance times 4^k bit for bit"""
    pts, q = E.range_index(family)
    i0, d0 = E.index_reference(pts, q)
    assert (d0[:20] == 0).all() and (d0[20:] > 0).all()
    for k in E.RANGE_LOG2:
        p, qq = E.range_index(family, k)
        assert np.array_equal(p, pts * 2.0 ** k) and np.array_equal(p * 2.0 ** -k, pts)
        i, d = E.index_reference(p, qq)
        assert np.isfinite(d).all() and np.isfinite(((p - qq[-1]) ** 2).sum(axis=1)).all()
        assert np.array_equal(i, i0) and np.array_equal(d, d0 * 4.0 ** k)
        assert (d[20:] > 2.0 ** -1000).all()   # far from fp64's own underflow
    if family == 'signed':   # squared norms of the centred rows against FLT_MAX = 2^128 * (1 - 2^-24)
        n2 = ((pts - pts.mean(axis=0)) ** 2).sum(axis=1)
        over = {k: float((n2 * 4.0 ** k >= 2.0 ** 128).mean()) for k in (62, 63, 64, 70)}
        assert over[62] == 0 and 0.5 < over[63] < 1 and over[64] == over[70] == 1, over


# ---- ia_coherence_batch ------------------------------------------------------------------------
def test_coherence_pad_restatement_equals_the_oracle():
    z = E.COHERENCE_CASES['A25x19_ap2_d110']()
    a, b = E.coherence_reference(z, oracle=True), E.coherence_reference(z, pad=2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert (a[0][1:, 0] >= 0).sum() > 200   # most pixels have a candidate


@pytest.mark.parametrize('name', list(E.COHERENCE_CASES))
def test_coherence_case_shapes(name):
    z = E.COHERENCE_CASES[name]()
    n, nq = z['n_ap'] * z['a_hw'][0] * z['a_hw'][1], z['b_hw'][0] * z['b_hw'][1]
    assert z['pts'].shape == (n, z['d']) and z['q'].shape == (nq, z['d'])
    assert z['s'].shape == (nq, 2) and z['im'].shape == (nq,) and z['px'].shape == (nq, 2)
    assert z['s'].dtype == z['im'].dtype == z['px'].dtype == np.int32
    assert (z['s'] >= (-2 if name == E.PAD_CASE else 0, 0)).all() and (z['s'] < z['a_hw']).all() and (z['im'] >= 0).all() and (z['im'] < z['n_ap']).all()
    assert tuple(z['px'][z['b_hw'][1] + 1]) == (1, 1)


def test_coherence_small_a_drops_candidates_on_every_side():
    """A 9 x 7 under B' 16 x 20: some pixel other than pixel 0 has no candidate, and shifted
    sources leave A above, below, left and right of it"""
    z = E.COHERENCE_CASES['A9x7_d55']()
    (a_h, a_w), (b_h, b_w) = z['a_hw'], z['b_hw']
    none, sides = 0, dict(top=0, bottom=0, left=0, right=0)
    for qi in range(1, b_h * b_w):
        r, c = divmod(qi, b_w)
        tr = {}
        got = E.coherence_pad(z['pts'], a_h, a_w, z['q'][qi], z['s'], z['im'], r, c, b_w, 2, tr)
        none += int(got[0] == (-1, -1))
        for _, pr, pc in tr['dropped']:
            sides['top'] += pr < 0
            sides['bottom'] += pr >= a_h
            sides['left'] += pc < 0
            sides['right'] += pc >= a_w
    assert none >= 1 and all(v >= 1 for v in sides.values()), (none, sides)


@pytest.mark.parametrize('name,distinct', [('ties_all_equal', 1), ('ties_4_rows', 4)])
def test_coherence_tie_cases(name, distinct):
    """exact ties: with every row equal the pick is the first candidate cell at every pixel; with 4
    distinct rows most pixels have two or more candidates at the minimum"""
    z = E.COHERENCE_CASES[name]()
    (a_h, a_w), (b_h, b_w) = z['a_hw'], z['b_hw']
    assert len(np.unique(z['pts'], axis=0)) == distinct
    tied = 0
    for qi in range(1, b_h * b_w):
        r, c = divmod(qi, b_w)
        tr = {}
        got = E.coherence_pad(z['pts'], a_h, a_w, z['q'][qi], z['s'], z['im'], r, c, b_w, 2, tr)
        if tr['cells']:
            roots = np.sqrt(tr['sums'])
            tied += int((roots == roots.min()).sum() >= 2)
            assert got[2] == tr['cells'][int(np.flatnonzero(roots == roots.min())[0])]
            if distinct == 1:
                assert got[2] == tr['cells'][0]
    assert tied > (b_h * b_w) // 2


@pytest.mark.parametrize('name', ['root_collapse_d55', 'root_collapse_d165'])
def test_coherence_root_collapse_pixels(name):
    """>= 8 pixels where an earlier cell's row x has the larger sum of squares but the same square
    root as the later cell's row y, every other candidate far: numpy's first argmin of the roots
    picks x's cell, an argmin of the sums would pick y's"""
    z = E.COHERENCE_CASES[name]()
    (a_h, a_w), (b_h, b_w) = z['a_hw'], z['b_hw']
    assert len(z['planted']) >= 8
    for pl in z['planted']:
        r, c = pl['px']
        qi = r * b_w + c
        tr = {}
        got = E.coherence_pad(z['pts'], a_h, a_w, z['q'][qi], z['s'], z['im'], r, c, b_w, 2, tr)
        ix, iy = tr['cells'].index(pl['cell_x']), tr['cells'].index(pl['cell_y'])
        assert tr['rows'][ix] == pl['row_x'] and tr['rows'][iy] == pl['row_y'] and ix < iy
        sx, sy = tr['sums'][ix], tr['sums'][iy]
        assert sx > sy and np.sqrt(sx) == np.sqrt(sy)
        others = np.delete(tr['sums'], [ix, iy])
        assert len(others) >= 1 and (others > 4 * sx).all()
        assert got[2] == pl['cell_x'] and int(np.argmin(tr['sums'])) == iy
        assert got == O_coherence(z, r, c)


def O_coherence(z, r, c):
    from oracle import ia_oracle as O
    return O.coherence(z['pts'], z['a_hw'][0], z['a_hw'][1], z['q'][r * z['b_hw'][1] + c], z['s'], z['im'], r, c,
                       z['b_hw'][1])


def test_coherence_other_pads():
    """pad 0 has no raster-earlier cell; pads 1, 3, 4 differ from pad 2 (the parameter matters)"""
    z = E.COHERENCE_CASES[E.PAD_CASE]()
    ref = {pad: E.coherence_reference(z, pad) for pad in (0, 1, 2, 3, 4)}
    assert (ref[0][0] == -1).all() and (ref[0][1] == 0).all() and (ref[0][2] == 0).all()
    for pad in (1, 3, 4):
        assert not np.array_equal(ref[pad][0], ref[2][0])
        assert (pad + 1) * (2 * pad + 1) <= 64   # one lane per window cell


# ---- GPU preprocessing -------------------------------------------------------------------------
ALL_IMAGES = ([('small', s) for s in E.SMALL_SHAPES] + [('clip', n) for n in E.CLIP_CASES])


def _image(kind, key):
    return E.small_image(key) if kind == 'small' else E.CLIP_CASES[key]()


@pytest.mark.parametrize('kind,key', ALL_IMAGES, ids=[str(k) for _, k in ALL_IMAGES])
def test_reduce_restatement_equals_the_package(kind, key):
    import ia_amd  # noqa: F401
    from ia_amd import img_preprocess as ip
    img = _image(kind, key)
    for _ in range(3):
        nxt = ip._pyramid_reduce(img)
        assert np.array_equal(nxt, E.reduce_variant(img)[0])
        assert nxt.shape[:2] == (-(-img.shape[0] // 2), -(-img.shape[1] // 2))
        img = nxt


def test_small_shapes_were_never_reduced_through_the_pyramid_entry():
    """compute_gaussian_pyramid(img, 3) runs no reduction on sides <= 3, so the direct form is
    needed to reach ia_reflect's periodic branch (side < 4) and 1-pixel outputs"""
    import ia_amd  # noqa: F401
    from ia_amd import img_preprocess as ip
    for shp in [(2, 7), (5, 1), (1, 1)]:
        assert len(ip.compute_gaussian_pyramid(np.zeros(shp), 3)) == 1
    assert sum(min(s[:2]) < 4 for s in E.SMALL_SHAPES) >= 10
    assert all(len(E.pyramid_reference(E.small_image(s), 3)) == 3 for s in E.SMALL_SHAPES)


def test_large_shapes_take_a_second_grid_stride_trip():
    """py_grid caps a launch at 1,048,576 threads: 1024^2 x 1 is exactly one trip; all three shapes are
    more in k_gauss1d (level 0); k_bilinear_half's output is more only for 2049 x 2051 (the others'
    are 264,708 and 270,900 values); k_color3 strides on 700 x 600 x 3"""
    assert 1024 * 1024 == E.PY_THREADS
    assert all(int(np.prod(s)) > E.PY_THREADS for s in E.LARGE_SHAPES)
    assert 513 * 516 < E.PY_THREADS and 300 * 301 * 3 < E.PY_THREADS < 1025 * 1026
    assert E.LARGE_REDUCE[(2049, 2051)] == 1 and E.large_image((2049, 2051)).shape == (2049, 2051)
    assert 700 * 600 * 3 > E.PY_THREADS > 300 * 200 * 3


@pytest.mark.parametrize('name', E.CLIP_ENGAGED)
def test_clip_engages(name):
    """the unclipped bilinear value leaves the smoothed level's range by rounding: >= 1 value above
    the maximum (below the minimum on the negated image), which the clip brings back"""
    img = E.CLIP_CASES[name]()
    raw, sm = E.reduce_variant(img, 'none')
    out, _ = E.reduce_variant(img, 'global')
    n = int((raw > sm.max()).sum()) if not name.startswith('neg_') else int((raw < sm.min()).sum())
    assert n >= 1 and int((raw != out).sum()) >= n
    assert np.abs(raw - out).max() < 1e-15


def test_clip_bounds_are_global_over_channels():
    img = E.CLIP_CASES['disjoint_channels']()
    assert all(img[..., k].max() < img[..., k + 1].min() for k in range(2))
    glob, _ = E.reduce_variant(img, 'global')
    chan, _ = E.reduce_variant(img, 'channel')
    assert int((glob != chan).sum()) >= 1


def test_other_preprocessing_inputs():
    assert len(np.unique(E.CLIP_CASES['constant_0p7']())) == 1
    x = E.CLIP_CASES['range_1e6']()
    assert x.min() < -9e5 and x.max() > 9e5
    assert 0 < E.CLIP_CASES['tiny_2m14']().max() < 2.0 ** -14
    assert E.CLIP_CASES['ch2_33x47']().shape == (33, 47, 2) and E.CLIP_CASES['ch4_33x47']().shape == (33, 47, 4)
    M, img = E.color_inputs()
    assert (M < 0).any() and (M > 0).any() and img.min() < -4.9 and img.max() > 4.9
    # a wrong summation order shows: einsum's (m0 x0 + m2 x2) + m1 x1 against left to right
    ltr = (M[:, 0] * img[..., None, 0] + M[:, 1] * img[..., None, 1]) + M[:, 2] * img[..., None, 2]
    assert (ltr != E.color_reference(M, img)).mean() > 0.1

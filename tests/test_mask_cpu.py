"""Masked resynthesis without a GPU (include/ia.h ia_synthesize_levels_masked): the numpy
restatement of tests/mask_inputs.py is pinned to windows_inputs.run and to the reference's recorded runs, the
idempotence property is shown on it, and the host pieces of the feature - ia_masked_step_list, mask_pyramid,
the bindings' shape checks and the refusals that need no device - are checked against it."""
import ctypes

import numpy as np
import pytest

import ia_amd
import mask_inputs as MI
import windows_inputs as WI
from golden_util import load_e2e
from ia_amd import _native


# ---- 1. an all-ones mask without sources is the full level ------------------------------------------------------
@pytest.mark.parametrize('win', [(3, 3), (3, 7)])
def test_full_mask_equals_the_window_restatement(win):
    z = MI.base(win)
    e = WI.run(z)
    r = MI.resynthesize(z, [x.copy() for x in z['Bp_init']], MI.full_masks(z))
    for level in range(1, z['L']):
        assert np.array_equal(r['s'][level], e['s'][level]) and np.array_equal(r['im'][level], e['im'][level])
        assert np.array_equal(r['Bp'][level], e['Bp'][level])
    full = [x for x in e['log']]
    assert sum(MI.wins(r['log'][l]) for l in r['log']) == sum(1 for x in full if x[4] is not None and x[4][1] <= x[4][0] * x[5])


@pytest.mark.parametrize('case', ['g32', 'multiap'])
def test_full_mask_equals_the_recorded_reference_runs(case):
    z = load_e2e(case)
    z['k'] = float(z['k'])
    r = MI.resynthesize(z, [x.copy() for x in z['Bp_init']], MI.full_masks(z), win=(3, 5))
    for level in range(1, z['L']):
        assert np.array_equal(r['s'][level], z['s'][level]) and np.array_equal(r['im'][level], z['im'][level])
        assert np.array_equal(r['Bp'][level], z['Bp_final'][level])


def test_coherence_equals_the_window_rule_when_every_pixel_has_a_source():
    z, e = WI.make('size_c1_3_7'), WI.expected('size_c1_3_7')
    level = 2
    As = WI.build_db(z, level, 3, 7)
    h, w = z['B_pyr'][level].shape[:2]
    a_h, a_w = z['A_pyr'][level].shape[:2]
    B_feat = WI.feature_array(z['B_pyr'], level, True, 3, 7)
    s, im = e['s'][level], e['im'][level]
    none = im.copy()
    none[:] = -1
    for qi in [0, 1, w + 3, 5 * w + 9, h * w - 1]:
        r, c = divmod(qi, w)
        q = WI.query_feature(B_feat, e['Bp'][level - 1], e['Bp'][level], r, c, w, 3, 7)
        assert MI.coherence(As, a_h, a_w, q, s, im, r, c, w, 3) == WI.coherence(As, a_h, a_w, q, s, im, r, c, w, 3)
        assert MI.coherence(As, a_h, a_w, q, s, none, r, c, w, 3) is None


# ---- 2. idempotence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['rect', 'one', 'rand30'])
def test_a_finished_state_is_a_fixed_point_of_interior_masks(kind):
    win = (3, 7)
    z = MI.base(win)
    e = WI.run(z)
    masks = MI.level_masks(z, win[1] // 2, kind)
    r = MI.resynthesize(z, [x.copy() for x in e['Bp']], masks, e['s'], e['im'])
    for level in range(1, z['L']):
        assert len(r['log'][level]) == masks[level].sum() > 0
        assert np.array_equal(r['s'][level], e['s'][level]) and np.array_equal(r['im'][level], e['im'][level])
        assert np.array_equal(r['Bp'][level], e['Bp'][level])


def test_a_mask_in_the_first_rows_may_change_the_state():
    """what the property excludes: a pixel of rows < p_l reads raster-later pixels through the reflection,
    which hold final values now and held initial ones in the full run"""
    win = (3, 7)
    z = MI.base(win)
    e = WI.run(z)
    masks = {l: np.zeros(shp, dtype=bool) for l, shp in enumerate(MI.shapes(z))}
    for m in masks.values():
        m[:2, :] = True
    r = MI.resynthesize(z, [x.copy() for x in e['Bp']], masks, e['s'], e['im'])
    kept = ~masks[2].ravel()
    assert np.array_equal(r['s'][2][kept], e['s'][2][kept]) and np.array_equal(r['Bp'][2][2:], e['Bp'][2][2:])
    assert not np.array_equal(r['s'][2], e['s'][2])


# ---- 3. the step compaction ----------------------------------------------------------------------------------
def _masks(h, w, seed):
    rs = np.random.RandomState(seed)
    row, col = np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    row[h // 2, :] = True
    col[:, w // 3] = True
    return dict(empty=np.zeros((h, w), dtype=bool), full=np.ones((h, w), dtype=bool), row=row, col=col,
                rand=rs.rand(h, w) < 0.3, rand_u8=(rs.rand(h, w) < 0.5).astype(np.uint8) * 255)


@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (7, 1), (16, 20), (34, 70)])
@pytest.mark.parametrize('pad', [1, 2, 3, 4])
def test_step_list_equals_its_restatement(shape, pad):
    h, w = shape
    for name, m in _masks(h, w, 10 * h + w + pad).items():
        off, px = _native.masked_step_list(m, pad)
        eo, ep = MI.step_list(m, pad)
        assert np.array_equal(off, eo) and np.array_equal(px, ep), name
        assert off[0] == 0 and off[-1] == np.count_nonzero(m) == len(px) and len(off) == w + (pad + 1) * (h - 1) + 1
        assert np.array_equal(np.sort(px), np.flatnonzero(np.asarray(m).ravel()))
        for t in range(len(off) - 1):                      # the step's pixels, rows ascending
            q = px[off[t]:off[t + 1]]
            assert np.array_equal(q % w + (pad + 1) * (q // w), np.full(len(q), t)) and (np.diff(q // w) > 0).all()
            r0, M = _native.wavefront_step_pad(h, w, pad, t)
            assert len(q) <= max(M, 0)


def test_step_list_offsets_only_and_refusals():
    m = np.ones((3, 4), dtype=np.uint8)
    off = np.zeros(4 + 3 * 2 + 1, dtype=np.int32)
    L = _native.lib()
    assert L.ia_masked_step_list(3, 4, 2, _native._ptr(m), _native._ptr(off), None) == 0 and off[-1] == 12
    for args in [(0, 4, 2, _native._ptr(m), _native._ptr(off), None), (3, 0, 2, _native._ptr(m), _native._ptr(off), None),
                 (3, 4, 5, _native._ptr(m), _native._ptr(off), None), (3, 4, -1, _native._ptr(m), _native._ptr(off), None),
                 (3, 4, 2, None, _native._ptr(off), None), (3, 4, 2, _native._ptr(m), None, None)]:
        assert L.ia_masked_step_list(*args) == -1
        assert b'ia_masked_step_list' in L.ia_last_error()


def test_tall_case_has_two_steps_a_scan_thread_and_a_step_of_66_rows():
    """mask_inputs.tall (B 66 x 200 at (3, 5)): 395 steps, so each of k_mask_scan's 256 threads sums a share of two
    counts, and step 197 holds all 66 rows, two of them in k_mask_steps' second 64-row trip"""
    t = MI.tall()
    z, masks = t['z'], t['masks']
    h, w = z['B_pyr'][1].shape
    assert (h, w) == (66, 200) and z['win'] == (3, 5) and z['L'] == 2
    T = w + 3 * (h - 1)
    assert T == MI.TALL_T == 395 and _native.wavefront_shape_pad(h, w, 2) == (395, 66)
    per, shares = MI.scan_shares(T)
    assert per == 2 and shares[0] == (0, 2) and shares[128] == (256, 258) and shares[197] == (394, 395)
    assert all(a == b == T for a, b in shares[198:])                 # the shares from 198 up are empty
    assert _native.wavefront_step_pad(h, w, 2, MI.TALL_LINE_STEP) == (0, 66)
    # the kept state: valid sources, about 5 % without one, B' = A' at the source
    s, im = t['s'], t['im']
    assert ((s >= 0) & (s < [25, 19])).all() and set(np.unique(im)) == {-1, 0} and 0.04 < (im < 0).mean() < 0.06
    has = (im >= 0).reshape(h, w)
    assert np.array_equal(t['Bp'][1][has], z['Ap_pyr'][0][1][s[:, 0], s[:, 1]].reshape(h, w)[has])
    assert np.array_equal(t['Bp'][1][~has], z['Bp_init'][1][~has]) and np.array_equal(t['Bp'][0], z['Bp_init'][0])
    # the masks
    line, sparse, both = masks['line'], masks['sparse'], masks['both']
    assert line.sum() == 66 and [tuple(x) for x in np.argwhere(line)] == [(r, 197 - 3 * r) for r in range(66)]
    off = MI.step_list(line, 2)[0]
    assert np.diff(off).max() == 66 and off[197] == 0 and off[198] == 66
    assert 0.015 < sparse.mean() < 0.025 and np.array_equal(both, line | sparse) and (line & ~sparse).sum() >= 60
    off = MI.step_list(sparse, 2)[0]
    assert (off[256], off[-1] - off[256]) == (202, 72)               # masked pixels in steps on both sides of index 256
    assert int(np.count_nonzero(np.diff(off)[1::2])) > 0             # a share's second count is non-zero: a real sum
    assert np.diff(MI.step_list(both, 2)[0]).max() >= 66
    for name in MI.TALL_MASKS:                                       # the host statement of the compaction
        o, px = _native.masked_step_list(masks[name], 2)
        eo, ep = MI.step_list(masks[name], 2)
        assert np.array_equal(o, eo) and np.array_equal(px, ep), name


def test_tall_restatements_redo_the_masked_pixels_only():
    t = MI.tall()
    for name, n, wins in (('line', 66, 27), ('sparse', 274, 140), ('both', 340, 170)):
        r, m = MI.tall_expected(name), t['masks'][name].ravel()
        assert m.sum() == n == len(r['log'][1]) and MI.wins(r['log'][1]) == wins
        assert np.array_equal(r['s'][1][~m], t['s'][~m]) and np.array_equal(r['im'][1][~m], t['im'][~m])
        assert np.array_equal(r['Bp'][1].ravel()[~m], t['Bp'][1].ravel()[~m]) and (r['im'][1][m] == 0).all()
        assert (r['s'][1][m] != t['s'][m]).any(axis=1).sum() > n // 2     # the redone pixels took other sources
        for _, rec, kf in r['log'][1]:                                   # no kappa comparison near its threshold
            assert rec is None or rec[0] * kf == 0 or abs(rec[1] - rec[0] * kf) > 1e-6 * rec[0] * kf


# ---- 4. mask_pyramid -----------------------------------------------------------------------------------------
def test_mask_pyramid_on_odd_shapes_against_hand_written_arrays():
    a = lambda rows: np.array([[ch == '1' for ch in r] for r in rows])
    m = a(['00000', '00100', '00000', '00000', '00001'])                  # 5 x 5 -> 3 x 3 -> 2 x 2
    shapes = [(2, 2), (3, 3), (5, 5)]
    got = ia_amd.mask_pyramid(m, shapes)
    want = [a(['10', '01']), a(['010', '000', '001']), m]
    for g, w in zip(got, want):
        assert g.dtype == bool and np.array_equal(g, w)
    got = ia_amd.mask_pyramid(m.astype(np.uint8), shapes, grow=1)
    want = [a(['11', '11']), a(['111', '111', '011']), a(['01110', '01110', '01110', '00011', '00011'])]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    m = a(['0000001', '0000000', '1000000'])                              # 3 x 7 -> 2 x 4 -> 1 x 2
    got = ia_amd.mask_pyramid(m, [(1, 2), (2, 4), (3, 7)])
    for g, w in zip(got, [a(['11']), a(['0001', '1000']), m]):
        assert np.array_equal(g, w)
    got = ia_amd.mask_pyramid(m, [(1, 2), (2, 4), (3, 7)], grow=1)
    for g, w in zip(got, [a(['11']), a(['1111', '1111']), a(['0000011', '1100011', '1100000'])]):
        assert np.array_equal(g, w)
    with pytest.raises(ValueError):
        ia_amd.mask_pyramid(m, [(1, 2), (2, 3), (3, 7)])
    with pytest.raises(ValueError):
        ia_amd.mask_pyramid(m, [(2, 4), (3, 6)])


@pytest.mark.parametrize('grow', [0, 1, 2])
def test_mask_pyramid_equals_its_restatement(grow):
    rs = np.random.RandomState(3 + grow)
    for shapes in [[(4, 5), (8, 10), (16, 20)], [(3, 2), (5, 3), (9, 5), (17, 9)], [(1, 1)]]:
        m = rs.rand(*shapes[-1]) < 0.1
        got, want = ia_amd.mask_pyramid(m, shapes, grow), MI.mask_pyramid(m, shapes, grow)
        assert len(got) == len(want) == len(shapes)
        for g, w, shp in zip(got, want, shapes):
            assert g.shape == tuple(shp) and np.array_equal(g, w)


# ---- 5. the bindings and the refusals that need no device ----------------------------------------------------
def test_symbols_and_the_unchanged_stats_layout():
    L = _native.lib()
    for n in ('ia_synthesize_levels_masked', 'ia_masked_step_list', 'ia_masked_stats'):
        assert hasattr(L, n) and n in _native.EXPORTS
    assert ia_amd.mask_pyramid is ia_amd.image_analogies.mask_pyramid
    assert ia_amd.resynthesize_pyramid is ia_amd.image_analogies.resynthesize_pyramid
    assert hasattr(_native.Context, 'resynthesize_levels') and hasattr(_native.Context, 'resynthesize_levels_device')


def test_null_arguments_are_refused_before_any_device_call():
    L = _native.lib()
    st = _native.Stats()
    one = (ctypes.c_void_p * 1)(None)
    arr = (_native.LevelArgs * 1)()
    assert L.ia_synthesize_levels_masked(None, arr, 1, 3, 5, one, one, one, ctypes.byref(st)) == -1
    assert b'ia_synthesize_levels_masked' in L.ia_last_error()
    assert L.ia_masked_stats(None, None, None) == -1
    assert st.pixels == 0 and st.steps == 0


def test_mask_state_contract_raises_before_the_abi():
    B = np.zeros((6, 8))
    n = 48
    mask, s, im = np.zeros((6, 8), dtype=bool), np.zeros((n, 2), dtype=np.int64), np.zeros(n, dtype=np.int32)
    m8, s32, i32 = _native.check_mask_state(B, mask, s, im)
    assert (m8.dtype, s32.dtype, i32.dtype) == (np.uint8, np.int32, np.int32) and s32.flags.c_contiguous
    assert s32 is not s and i32 is not im                       # fresh arrays: the inputs are never written
    m8, s32, i32 = _native.check_mask_state(B, mask.astype(np.uint8), None, None)
    assert (i32 == -1).all() and s32.shape == (n, 2)
    bad = [(np.zeros((6, 7), dtype=bool), s, im), (np.zeros((6, 8)), s, im), (np.zeros(48, dtype=bool), s, im),
           (mask, np.zeros((n, 3), dtype=np.int32), im), (mask, np.zeros((n - 1, 2), dtype=np.int32), im),
           (mask, s, np.zeros(n + 1, dtype=np.int32)), (mask, s.astype(np.float64), im), (mask, s, im.astype(np.float32)),
           (mask, s, None), (mask, None, im)]
    for args in bad:
        with pytest.raises(_native.IAError):
            _native.check_mask_state(B, *args)

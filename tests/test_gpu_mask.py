"""GPU parity for masked resynthesis (include/ia.h ia_synthesize_levels_masked).  Every
comparison is bit for bit (np.array_equal): against the reference's recorded runs and the window call where the
mask is full, against the input state where the property says nothing may change, and against the numpy
restatement of tests/mask_inputs.py (pinned by tests/test_mask_cpu.py) everywhere else.

Shapes are windows_inputs' small ones (A 25 x 19 / B 16 x 20 over three levels) unless a test says otherwise;
the finished states and the restatement runs are computed once per module and never written."""
import ctypes
import types

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

import mask_inputs as MI
import windows_inputs as WI
from golden_util import load_e2e

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    """a context of this module's own: the session's may be left recording or shard-emulating, which this call refuses"""
    import ia_amd  # noqa: F401
    from ia_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _a_side(z, level):
    if 'A_pairs' in z:
        return [p[level] for p in z['A_pairs']], [p[level - 1] for p in z['A_pairs']]
    return z['A_pyr'][level], z['A_pyr'][level - 1]


def _job(z, level, Bp):
    return dict(B=z['B_pyr'][level], Bc=z['B_pyr'][level - 1], Bpc=Bp[level - 1], Bp=Bp[level], weights=z['weights'],
                kappa_factor=1 + (2 ** (level - z['L'])) * z['k'])


def _level_call(ctx, z0, level, jobs, win, st, masked):
    A, Ac = _a_side(z0, level)
    Ap, Apc = [p[level] for p in z0['Ap_pyr']], [p[level - 1] for p in z0['Ap_pyr']]
    if masked:
        return ctx.resynthesize_levels(A, Ac, Ap, Apc, jobs, windows=win, stats=st)
    return ctx.synthesize_levels(A, Ac, Ap, Apc, jobs, st, windows=win)


def _full(ctx, z, win):
    """the finished state of z by the window call: dict(s, im, Bp)"""
    Bp = [x.copy() for x in z['Bp_init']]
    e = dict(s={}, im={}, Bp=Bp)
    for level in range(1, z['L']):
        e['s'][level], e['im'][level] = _level_call(ctx, z, level, [_job(z, level, Bp)], win, None, False)[0]
    return e


def _redo(ctx, Z, win, Bp, masks, S, IM, st=None):
    """every level of the jobs Z (one A side) through the masked call, one call per level.  Bp: a pyramid per job,
    updated in place; masks / S / IM: per job {level: .} (S[j] = None: no sources).  Returns [{level: (s, im)}]"""
    out = [dict() for _ in Z]
    for level in range(1, Z[0]['L']):
        jobs = [dict(_job(z, level, Bp[j]), mask=masks[j][level], s=(S[j] or {}).get(level), im=(IM[j] or {}).get(level))
                for j, z in enumerate(Z)]
        for j, r in enumerate(_level_call(ctx, Z[0], level, jobs, win, st, True)):
            out[j][level] = r
    return out


def _same(out, Bp, e, L, what=''):
    for level in range(1, L):
        assert np.array_equal(out[level][0], e['s'][level]), (what, level, 's')
        assert np.array_equal(out[level][1], e['im'][level]), (what, level, 'im')
        assert np.array_equal(Bp[level], e['Bp'][level]), (what, level, 'Bp')


def _copy(Bp):
    return [np.array(x, dtype=np.float64, order='C') for x in Bp]


_STATE = {}


def state(ctx, win):
    """(z, finished state) of the base case at sizes win, once per module; read-only"""
    if win not in _STATE:
        z = MI.base(win)
        _STATE[win] = (z, _full(ctx, z, win))
    return _STATE[win]


_EDIT = {}


def edit_case(ctx):
    """case 3, once per module: (z1, masks, the state before, the restatement's result); read-only"""
    if not _EDIT:
        z, e0 = state(ctx, (3, 7))
        z1, masks = MI.edited(z)
        _EDIT['x'] = (z1, masks, e0, MI.resynthesize(z1, _copy(e0['Bp']), masks, e0['s'], e0['im']))
    return _EDIT['x']


# ---- 1. an all-ones mask without sources is the full level ----------------------------------------------------
@pytest.mark.parametrize('case', ['g32', 'rect', 'multiap', 'rgb3', 'ties', 'noinit'])
def test_full_mask_at_3_5_equals_the_recorded_reference_runs(ctx, case):
    from ia_amd import _native
    z = load_e2e(case)
    z['k'] = float(z['k'])
    Bp = _copy(z['Bp_init'])
    st = _native.Stats()
    out = _redo(ctx, [z], (3, 5), [Bp], [MI.full_masks(z)], [None], [None], st)
    _same(out[0], Bp, dict(s=z['s'], im=z['im'], Bp=z['Bp_final']), z['L'], case)
    assert st.pixels == sum(z['B_pyr'][l].shape[0] * z['B_pyr'][l].shape[1] for l in range(1, z['L']))
    assert st.nbhd_levels == 0 and st.f16_levels == 0 and st.kappa_ambiguous == 0


@pytest.mark.parametrize('win', [(3, 7), (1, 3)])
def test_full_mask_equals_the_window_call(ctx, win):
    z, e = state(ctx, win)
    Bp = _copy(z['Bp_init'])
    out = _redo(ctx, [z], win, [Bp], [MI.full_masks(z)], [None], [None])
    _same(out[0], Bp, e, z['L'], win)


# ---- 2. idempotence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['rect', 'one', 'checker', 'rand30', 'last'])
@pytest.mark.parametrize('win', [(3, 5), (3, 7)])
def test_a_finished_state_is_a_fixed_point_of_interior_masks(ctx, win, kind):
    from ia_amd import _native
    z, e = state(ctx, win)
    masks = MI.level_masks(z, win[1] // 2, kind)
    Bp = _copy(e['Bp'])
    st = _native.Stats()
    out = _redo(ctx, [z], win, [Bp], [masks], [e['s']], [e['im']], st)
    _same(out[0], Bp, e, z['L'], (win, kind))
    assert st.pixels == sum(int(m.sum()) for m in masks.values()) > 0


@pytest.mark.parametrize('where', ['rows', 'cols'])
@pytest.mark.parametrize('win', [(3, 5), (3, 7)])
def test_masks_in_the_first_rows_or_columns_equal_the_restatement(ctx, win, where):
    """rows / columns below p_l read raster-later pixels through the reflection, which hold the final values now:
    the restatement decides, and the schedule must not matter"""
    z, e = state(ctx, win)
    masks = {}
    for l, shp in enumerate(MI.shapes(z)):
        masks[l] = np.zeros(shp, dtype=bool)
        if where == 'rows':
            masks[l][:2, :] = True
        else:
            masks[l][:, :2] = True
    want = MI.resynthesize(z, _copy(e['Bp']), masks, e['s'], e['im'])
    Bp = _copy(e['Bp'])
    out = _redo(ctx, [z], win, [Bp], [masks], [e['s']], [e['im']])
    _same(out[0], Bp, want, z['L'], (win, where))


# ---- 3. an edit --------------------------------------------------------------------------------------------------
def test_an_edit_equals_the_restatement_and_keeps_the_rest(ctx):
    z1, masks, e0, want = edit_case(ctx)
    assert all(0 < masks[l].sum() < masks[l].size for l in range(1, z1['L']))
    Bp = _copy(e0['Bp'])
    out = _redo(ctx, [z1], (3, 7), [Bp], [masks], [e0['s']], [e0['im']])
    _same(out[0], Bp, want, z1['L'], 'edit')
    changed = 0
    for level in range(1, z1['L']):
        kept = ~masks[level].ravel()
        assert np.array_equal(out[0][level][0][kept], e0['s'][level][kept])
        assert np.array_equal(out[0][level][1][kept], e0['im'][level][kept])
        assert np.array_equal(Bp[level].reshape(kept.size, -1)[kept], e0['Bp'][level].reshape(kept.size, -1)[kept])
        changed += int((out[0][level][0] != e0['s'][level]).any(axis=1).sum())
    assert changed > 0                                         # the edit did re-decide pixels


# ---- 4. hole filling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mix', [False, True])
def test_hole_filling_equals_the_restatement(ctx, mix):
    """B' is known outside the hole and its origin is not: im = -1 everywhere, so no kept pixel is a coherence
    candidate although its s (the finished state's here) would shift to a pixel inside A.  mix: only the kept
    pixels above the hole have sources, and the others' s lies far outside A"""
    win = (3, 7)
    z, e = state(ctx, win)
    masks = MI.level_masks(z, 3, 'rect')
    S, IM = {}, {}
    for level, m in masks.items():
        S[level] = np.full_like(e['s'][level], 10 ** 6) if mix else e['s'][level].copy()
        IM[level] = np.full_like(e['im'][level], -1)
        if mix:
            top = int(np.flatnonzero(m.any(axis=1))[0])
            above = np.arange(m.size) < top * m.shape[1]
            S[level][above], IM[level][above] = e['s'][level][above], e['im'][level][above]
    want = MI.resynthesize(z, _copy(e['Bp']), masks, S, IM)
    Bp = _copy(e['Bp'])
    out = _redo(ctx, [z], win, [Bp], [masks], [S], [IM])
    _same(out[0], Bp, want, z['L'], 'hole')
    for level, m in masks.items():
        kept = ~m.ravel()
        assert (out[0][level][1][kept] == IM[level][kept]).all() and (out[0][level][0][kept] == S[level][kept]).all()
        assert (out[0][level][1][m.ravel()] >= 0).all()
    if mix:
        assert sum(MI.wins(want['log'][l]) for l in want['log']) > 0


# ---- 5. step shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['col', 'row'])
def test_a_full_column_and_a_full_row_have_one_query_a_step(ctx, where):
    win = (3, 7)
    z, e = state(ctx, win)
    masks = {}
    for l, shp in enumerate(MI.shapes(z)):
        masks[l] = np.zeros(shp, dtype=bool)
        if where == 'col':
            masks[l][:, shp[1] // 2] = True
        else:
            masks[l][shp[0] // 2, :] = True
        assert np.diff(MI.step_list(masks[l], 3)[0]).max() == 1
    want = MI.resynthesize(z, _copy(e['Bp']), masks, e['s'], e['im'])
    Bp = _copy(e['Bp'])
    out = _redo(ctx, [z], win, [Bp], [masks], [e['s']], [e['im']])
    _same(out[0], Bp, want, z['L'], where)


def test_steps_of_two_query_tiles(ctx):
    """B 34 x 70 at (3, 3), one level, full mask: steps of up to 34 queries, i.e. two query tiles"""
    z = WI.rand_case(431, 3, 3, geo=dict(a_hw=(25, 19), b_hw=(34, 70), L=2))
    masks = MI.full_masks(z)
    assert np.diff(MI.step_list(masks[1], 1)[0]).max() >= 33
    want = WI.run(z)
    Bp = _copy(z['Bp_init'])
    out = _redo(ctx, [z], (3, 3), [Bp], [masks], [None], [None])
    _same(out[0], Bp, want, 2, '34x70')


def test_borders_narrower_than_the_pad(ctx):
    """B 8 x 8 with A 12 x 10 at (3, 9): p_l = 4, so every pixel's window reflects at a border or two"""
    win = (3, 9)
    z = WI.rand_case(432, 3, 9, geo=dict(a_hw=(12, 10), b_hw=(8, 8), L=2))
    full = WI.run(z)
    Bp = _copy(z['Bp_init'])
    out = _redo(ctx, [z], win, [Bp], [MI.full_masks(z)], [None], [None])
    _same(out[0], Bp, full, 2, 'full')
    rs = np.random.RandomState(5)
    masks = {1: rs.rand(8, 8) < 0.4}
    want = MI.resynthesize(z, _copy(full['Bp']), masks, full['s'], full['im'])
    Bp = _copy(full['Bp'])
    out = _redo(ctx, [z], win, [Bp], [masks], [full['s']], [full['im']])
    _same(out[0], Bp, want, 2, 'random')


def _tall_redo(ctx, kinds, st=None):
    """mask_inputs.tall's state under the masks `kinds` (None: all-zero), one job each in one call.  Returns
    ([(s, im)] per job, [B'] per job)"""
    t = MI.tall()
    z = t['z']
    masks = [np.zeros((66, 200), dtype=bool) if k is None else t['masks'][k] for k in kinds]
    Bp = [_copy(t['Bp']) for _ in kinds]
    out = _redo(ctx, [z] * len(kinds), MI.TALL_WIN, Bp, [{1: m} for m in masks], [{1: t['s']}] * len(kinds),
                [{1: t['im']}] * len(kinds), st)
    return [o[1] for o in out], [b[1] for b in Bp], masks


def _tall_same(got, Bp, kind):
    t = MI.tall()
    if kind is None:                                             # an all-zero mask: the state as it was
        want_s, want_im, want_Bp = t['s'], t['im'], t['Bp'][1]
    else:
        e = MI.tall_expected(kind)
        want_s, want_im, want_Bp = e['s'][1], e['im'][1], e['Bp'][1]
        kept = ~t['masks'][kind].ravel()                         # kept pixels are untouched
        assert np.array_equal(got[0][kept], t['s'][kept]) and np.array_equal(got[1][kept], t['im'][kept]), kind
        assert np.array_equal(Bp.ravel()[kept], t['Bp'][1].ravel()[kept]), kind
    assert np.array_equal(got[0], want_s), (kind, 's')
    assert np.array_equal(got[1], want_im), (kind, 'im')
    assert np.array_equal(Bp, want_Bp), (kind, 'Bp')


@pytest.mark.parametrize('kind', MI.TALL_MASKS)
def test_tall_level_more_than_256_steps_and_a_step_of_66_rows(ctx, kind):
    """B 66 x 200 at (3, 5): 395 steps, so every thread of k_mask_scan sums a share of two counts ('sparse': masked
    pixels on both sides of step 256); 'line' is step 197 with all 66 rows masked: three query tiles, rows 64 and
    65 placed by k_mask_steps' second trip behind the 64 of the first ('both': among sparse steps)"""
    from ia_amd import _native
    st = _native.Stats()
    got, Bp, masks = _tall_redo(ctx, [kind], st)
    _tall_same(got[0], Bp[0], kind)
    e = MI.tall_expected(kind)
    assert st.pixels == int(masks[0].sum()) and st.steps == MI.nonempty_steps(masks, 2)
    assert st.coherence_wins == MI.wins(e['log'][1]) and st.kappa_ambiguous == 0
    if kind == 'line':
        assert st.steps == 1 and st.pixels == 66


def test_tall_batch_of_three_jobs_equals_separate_calls(ctx):
    """jobs 'line', 'sparse' and an all-zero mask in one call: a step's entries stand job after job, so the count
    carried over step 197's 64-row trips goes on into the next job's entries"""
    from ia_amd import _native
    kinds = ['line', 'sparse', None]
    st = _native.Stats()
    got, Bp, masks = _tall_redo(ctx, kinds, st)
    for j, kind in enumerate(kinds):
        _tall_same(got[j], Bp[j], kind)
        one, Bp1, _ = _tall_redo(ctx, [kind])
        assert np.array_equal(one[0][0], got[j][0]) and np.array_equal(one[0][1], got[j][1]) and np.array_equal(Bp1[0], Bp[j])
    assert st.pixels == 66 + int(masks[1].sum()) and st.steps == MI.nonempty_steps(masks, 2)
    assert MI.nonempty_steps(masks, 2) == MI.nonempty_steps([masks[0] | masks[1]], 2)


def test_tall_both_on_device_memory(ctx):
    tl = MI.tall()
    z, e, mask = tl['z'], MI.tall_expected('both'), tl['masks']['both']
    t = lambda x, dt=np.float64: torch.from_numpy(np.array(x, dtype=dt, order='C')).to('cuda:0')   # (copies: the state is read-only)
    n = mask.size
    T = dict(A=t(z['A_pyr'][1]), Ac=t(z['A_pyr'][0]), Ap=t(np.stack([p[1] for p in z['Ap_pyr']])),
             Apc=t(np.stack([p[0] for p in z['Ap_pyr']])), B=t(z['B_pyr'][1]), Bc=t(z['B_pyr'][0]), Bpc=t(tl['Bp'][0]),
             Bp=t(tl['Bp'][1]), weights=t(z['weights']), s_out=torch.full((n, 2), -7, dtype=torch.int32, device='cuda:0'),
             im_out=torch.full((n,), -7, dtype=torch.int32, device='cuda:0'), mask=t(mask, np.uint8),
             s_in=t(tl['s'], np.int32), im_in=t(tl['im'], np.int32))
    torch.cuda.synchronize()
    ctx.resynthesize_levels_device(1, 1, (25, 19), (66, 200), [{k: v.data_ptr() for k, v in T.items()}],
                                   [1 + (2 ** (1 - z['L'])) * z['k']], windows=MI.TALL_WIN)
    torch.cuda.synchronize()
    assert np.array_equal(T['s_out'].cpu().numpy(), e['s'][1]) and np.array_equal(T['im_out'].cpu().numpy(), e['im'][1])
    assert np.array_equal(T['Bp'].cpu().numpy(), e['Bp'][1])
    assert np.array_equal(T['s_in'].cpu().numpy(), tl['s']) and np.array_equal(T['im_in'].cpu().numpy(), tl['im'])


# ---- 6. a batch -------------------------------------------------------------------------------------------------
def test_a_batch_of_three_masks_equals_separate_calls_and_the_restatement(ctx):
    """job 0: an all-zero mask on the finished state; job 1: a full mask from the initial B' without sources;
    job 2: the edited B side with a sparse mask on the finished state"""
    from ia_amd import _native
    win = (3, 7)
    z1, _, e0, _ = edit_case(ctx)
    z, _ = state(ctx, win)
    rs = np.random.RandomState(11)
    shp = MI.shapes(z)
    zero = {l: np.zeros(s, dtype=bool) for l, s in enumerate(shp)}
    sparse = {l: rs.rand(*s) < 0.08 for l, s in enumerate(shp)}
    off_full, off_sparse = MI.step_list(np.ones(shp[2], dtype=bool), 3)[0], MI.step_list(sparse[2], 3)[0]
    assert ((np.diff(off_sparse) == 0) & (np.diff(off_full) > 0)).any()   # steps without a pixel of job 2
    Z, masks = [z, z, z1], [zero, MI.full_masks(z), sparse]
    S, IM = [e0['s'], None, e0['s']], [e0['im'], None, e0['im']]
    start = lambda: [_copy(e0['Bp']), _copy(z['Bp_init']), _copy(e0['Bp'])]
    want = [e0, WI.run(z), MI.resynthesize(z1, _copy(e0['Bp']), sparse, e0['s'], e0['im'])]
    Bp = start()
    st = _native.Stats()
    out = _redo(ctx, Z, win, Bp, masks, S, IM, st)
    for j in range(3):
        _same(out[j], Bp[j], want[j], z['L'], 'batch job %d' % j)
    assert st.pixels == sum(int(m[l].sum()) for m in masks for l in range(1, z['L']))
    assert st.steps == sum(MI.nonempty_steps([m[l] for m in masks], 3) for l in range(1, z['L']))
    Bp1 = start()
    for j in range(3):
        o = _redo(ctx, [Z[j]], win, [Bp1[j]], [masks[j]], [S[j]], [IM[j]])
        _same(o[0], Bp1[j], want[j], z['L'], 'separate job %d' % j)


# ---- 7. device pointers -------------------------------------------------------------------------------------------
def test_device_memory_on_the_edits_finest_level(ctx):
    z1, masks, e0, want = edit_case(ctx)
    level = z1['L'] - 1
    h, w = z1['B_pyr'][level].shape[:2]
    t = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to('cuda:0')
    T = dict(A=t(z1['A_pyr'][level]), Ac=t(z1['A_pyr'][level - 1]), Ap=t(np.stack([p[level] for p in z1['Ap_pyr']])),
             Apc=t(np.stack([p[level - 1] for p in z1['Ap_pyr']])), B=t(z1['B_pyr'][level]), Bc=t(z1['B_pyr'][level - 1]),
             Bpc=t(want['Bp'][level - 1]), Bp=t(e0['Bp'][level]), weights=t(z1['weights']),
             s_out=torch.full((h * w, 2), -7, dtype=torch.int32, device='cuda:0'),
             im_out=torch.full((h * w,), -7, dtype=torch.int32, device='cuda:0'),
             mask=t(masks[level], np.uint8), s_in=t(e0['s'][level], np.int32), im_in=t(e0['im'][level], np.int32))
    torch.cuda.synchronize()
    kf = 1 + (2 ** (level - z1['L'])) * z1['k']
    ptrs = {k: v.data_ptr() for k, v in T.items()}
    ctx.resynthesize_levels_device(1, 1, z1['A_pyr'][level].shape[:2], (h, w), [ptrs], [kf], windows=(3, 7))
    torch.cuda.synchronize()
    assert np.array_equal(T['s_out'].cpu().numpy(), want['s'][level]) and np.array_equal(T['im_out'].cpu().numpy(), want['im'][level])
    assert np.array_equal(T['Bp'].cpu().numpy(), want['Bp'][level])
    assert np.array_equal(T['s_in'].cpu().numpy(), e0['s'][level])            # the inputs are not written
    # the same call with s_in / im_in aliasing the outputs
    T['Bp'].copy_(t(e0['Bp'][level]))
    T['s_out'].copy_(T['s_in'])
    T['im_out'].copy_(T['im_in'])
    torch.cuda.synchronize()
    ptrs.update(s_in=ptrs['s_out'], im_in=ptrs['im_out'])
    ctx.resynthesize_levels_device(1, 1, z1['A_pyr'][level].shape[:2], (h, w), [ptrs], [kf], windows=(3, 7))
    torch.cuda.synchronize()
    assert np.array_equal(T['s_out'].cpu().numpy(), want['s'][level]) and np.array_equal(T['im_out'].cpu().numpy(), want['im'][level])
    assert np.array_equal(T['Bp'].cpu().numpy(), want['Bp'][level])


# ---- 8. several A' images, pairs -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['two_ap', 'pairs2'])
def test_two_a_primes_and_pairs_with_a_sparse_mask(ctx, name):
    win = (3, 7)
    z = WI.rand_case(441, 3, 7, n_ap=2) if name == 'two_ap' else WI.make('pairs2')
    assert len(z['Ap_pyr']) == 2 and (name == 'two_ap') == ('A_pairs' not in z)
    e = _full(ctx, z, win)
    rs = np.random.RandomState(13)
    masks = {l: rs.rand(*s) < 0.2 for l, s in enumerate(MI.shapes(z))}
    last = z['L'] - 1
    assert (e['im'][last][~masks[last].ravel()] == 1).any()               # kept pixels of the second A'
    want = MI.resynthesize(z, _copy(e['Bp']), masks, e['s'], e['im'])
    Bp = _copy(e['Bp'])
    out = _redo(ctx, [z], win, [Bp], [masks], [e['s']], [e['im']])
    _same(out[0], Bp, want, z['L'], name)


# ---- 9. refusals -------------------------------------------------------------------------------------------------
def _raw(ctx, z, win, mask, s_in, im_in, dbg=False, mutate=None, null=None):
    """one raw host-memory call on z's finest level.  Returns (rc, message, untouched, Stats): untouched = s_out,
    im_out and B' are as they were"""
    from ia_amd import _native
    level = z['L'] - 1
    c64 = lambda x: np.array(x, dtype=np.float64, order='C')   # copies: a test may poison them
    Bp = c64(z['Bp_init'][level])
    n = Bp.shape[0] * Bp.shape[1]
    s, im = np.full((n, 2), -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    d = (np.full((n, 6), -7, dtype=np.int32), np.full((n, 2), -7.0)) if dbg else None
    keep = [c64(z['A_pyr'][level]), c64(z['A_pyr'][level - 1]), c64(np.stack([p[level] for p in z['Ap_pyr']])),
            c64(np.stack([p[level - 1] for p in z['Ap_pyr']])), c64(z['B_pyr'][level]), c64(z['B_pyr'][level - 1]),
            c64(z['Bp_init'][level - 1]), Bp, c64(z['weights'])]
    if mutate is not None:
        mutate(keep)
    p = [_native._ptr(x) for x in keep]
    ch = 1 if keep[0].ndim == 2 else keep[0].shape[2]
    a = _native.LevelArgs(ch, len(z['Ap_pyr']), keep[0].shape[0], keep[0].shape[1], Bp.shape[0], Bp.shape[1], p[0], p[1], p[2],
                          p[3], p[4], p[5], p[6], p[7], p[8], 1.25, _native._ptr(s), _native._ptr(im), _native.IA_MEM_HOST,
                          None if d is None else _native._ptr(d[0]), None if d is None else _native._ptr(d[1]), 0)
    arr = (_native.LevelArgs * 1)(a)
    m8 = np.array(mask, dtype=np.uint8, order='C')
    si, ii = np.array(s_in, dtype=np.int32, order='C'), np.array(im_in, dtype=np.int32, order='C')
    one = lambda x, k: (ctypes.c_void_p * 1)(None if null == k else x.ctypes.data)
    pm, ps, pi = one(m8, 'mask'), one(si, 's_in'), one(ii, 'im_in')
    if null == 'masks':
        pm = None
    st = _native.Stats()
    rc = _native.lib().ia_synthesize_levels_masked(ctx.handle, arr, 1, win[0], win[1], pm, ps, pi, ctypes.byref(st))
    msg = _native.lib().ia_last_error().decode() if rc else ''
    untouched = bool((s == -7).all() and (im == -7).all() and np.array_equal(Bp, z['Bp_init'][level]))
    return rc, msg, untouched, st, (s, im, Bp)


def _refused(ctx, z, win, match, mask=None, s_in=None, im_in=None, **kw):
    h, w = z['Bp_init'][z['L'] - 1].shape[:2]
    mask = np.ones((h, w), dtype=np.uint8) if mask is None else mask
    s_in = np.zeros((h * w, 2), dtype=np.int32) if s_in is None else s_in
    im_in = np.full(h * w, -1, dtype=np.int32) if im_in is None else im_in
    before = ctx.masked_stats()
    rc, msg, untouched, st, _ = _raw(ctx, z, win, mask, s_in, im_in, **kw)
    assert rc == -1, rc                                        # IA_EINVAL
    assert 'ia_synthesize_levels_masked' in msg and match in msg, msg
    assert untouched                                           # nothing written
    assert st.pixels == 0 and st.steps == 0 and st.dist_launches == 0 and st.nbhd_levels == 0
    assert ctx.masked_stats() == before
    return msg


def test_refusals_leave_outputs_and_context_intact(ctx):
    from ia_amd import _native
    z1 = WI.rand_case(380, 3, 7, geo=dict(a_hw=(12, 10), b_hw=(6, 7), L=2))
    z3 = WI.rand_case(381, 3, 3, geo=dict(a_hw=(12, 10), b_hw=(6, 7), L=2), ch=3)
    e = WI.run(z1)

    def good(c):                                                # a following good call passes
        rc, _, _, st, (s, im, Bp) = _raw(c, z1, (3, 7), np.ones((6, 7)), np.zeros((42, 2)), np.full(42, -1))
        assert rc == 0 and st.pixels == 42
        assert np.array_equal(s, e['s'][1]) and np.array_equal(im, e['im'][1]) and np.array_equal(Bp, e['Bp'][1])

    # ia_synthesize_levels_nbhd's refusals, under this call's name
    for win in [(0, 5), (2, 5), (7, 5), (3, 1), (3, 4), (3, 11)]:
        _refused(ctx, z1, win, 'n_sm = %d, n_lg = %d' % win)
    assert 'D = 171' in _refused(ctx, z1, (5, 9), 'n_sm = 5, n_lg = 9')
    assert 'D = 273' in _refused(ctx, z3, (3, 7), 'n_sm = 3, n_lg = 7')
    _refused(ctx, z1, (3, 7), 'debug', dbg=True)
    c2, c3 = _native.Context(0), _native.Context(0)
    try:
        c2.set_option('shard_emulate', 2)
        _refused(c2, z1, (3, 7), 'shard')
        c2.set_option('shard_emulate', 1)
        c2.set_option('pipeline_record', 1)
        _refused(c2, z1, (3, 7), 'pipelined')
        c2.set_option('pipeline_record', 0)
        c3.set_option('pipeline_record', 1)
        c2.pipeline_depend(c3, 1)
        _refused(c2, z1, (3, 7), 'pipelined')
        good(c2)                                               # the dependency was consumed: the next call runs
    finally:
        c2.close()
        c3.close()

    def poison(keep):
        keep[2][0, 3, 4] = np.inf                             # one A' value

    _refused(ctx, z1, (3, 7), 'finite', mutate=poison)
    good(ctx)
    # this call's own
    _refused(ctx, z1, (3, 7), 'NULL', null='masks')
    _refused(ctx, z1, (3, 7), 'NULL', null='mask')
    _refused(ctx, z1, (3, 7), 'NULL', null='s_in')
    _refused(ctx, z1, (3, 7), 'NULL', null='im_in')
    im = np.full(42, -1, dtype=np.int32)
    im[17] = 1                                                 # n_ap = 1
    _refused(ctx, z1, (3, 7), 'im_in', im_in=im)
    im[17] = 0
    s = np.zeros((42, 2), dtype=np.int32)
    s[17] = (12, 0)                                            # (a_h, 0)
    _refused(ctx, z1, (3, 7), 's_in', s_in=s, im_in=im)
    s[17] = (0, 10)                                            # (0, a_w)
    _refused(ctx, z1, (3, 7), 's_in', s_in=s, im_in=im)
    s[17] = (-1, 0)
    _refused(ctx, z1, (3, 7), 's_in', s_in=s, im_in=im, mask=np.zeros((6, 7), dtype=np.uint8))   # kept or masked alike
    im[17] = -1                                                # no source: its s is not read
    rc, _, _, _, _ = _raw(ctx, z1, (3, 7), np.ones((6, 7)), s, im)
    assert rc == 0
    good(ctx)


# ---- 10. stats ----------------------------------------------------------------------------------------------------
def test_stats_count_the_masked_pixels_and_the_steps_that_ran(ctx):
    from ia_amd import _native
    z1, masks, e0, want = edit_case(ctx)
    L = z1['L']
    n0, ms0 = ctx.masked_stats()
    st = _native.Stats()
    _redo(ctx, [z1], (3, 7), [_copy(e0['Bp'])], [masks], [e0['s']], [e0['im']], st)
    n1, ms1 = ctx.masked_stats()
    assert n1 - n0 == L - 1 and ms1 > ms0                      # masked_levels, and the lists took device time
    assert st.pixels == sum(int(masks[l].sum()) for l in range(1, L))
    assert st.steps == sum(MI.nonempty_steps([masks[l]], 3) for l in range(1, L))
    assert st.steps < sum(WI.step_shape(*MI.shapes(z1)[l], 3)[0] for l in range(1, L))
    assert st.dist_launches == st.steps                        # at most 16 queries a step here: one scan each
    assert st.kappa_ambiguous == 0 and st.nbhd_levels == 0
    assert st.coherence_wins == sum(MI.wins(want['log'][l]) for l in range(1, L)) > 0
    assert st.synth_ms > 0 and st.db_ms > 0
    # only all-zero masks: nothing runs, the outputs are the inputs
    st = _native.Stats()
    zero = {l: np.zeros(s, dtype=bool) for l, s in enumerate(MI.shapes(z1))}
    Bp = _copy(e0['Bp'])
    out = _redo(ctx, [z1, z1], (3, 7), [Bp, _copy(e0['Bp'])], [zero, zero], [e0['s'], None], [e0['im'], None], st)
    assert st.dist_launches == 0 and st.pixels == 0 and st.steps == 0 and st.coherence_wins == 0
    assert ctx.masked_stats()[0] == n1 + 2 * (L - 1)
    _same(out[0], Bp, e0, L, 'all-zero')
    assert all((out[1][l][1] == -1).all() for l in range(1, L))


# ---- 11. end to end -----------------------------------------------------------------------------------------------
def test_resynthesize_pyramid_equals_the_restatements_pyramid(ctx):
    import ia_amd
    z1, masks, e0, want = edit_case(ctx)
    L = z1['L']
    c = types.SimpleNamespace(n_sm=3, n_lg=7, n_half=24, pad_sm=1, pad_lg=3, num_ch=1, max_levels=L, k=z1['k'],
                              weights=z1['weights'])
    m = np.zeros(MI.shapes(z1)[-1], dtype=bool)
    m[5:11, 6:14] = True                                       # mask_inputs.edited's rectangle
    assert all(np.array_equal(a, b) for a, b in zip(ia_amd.mask_pyramid(m, MI.shapes(z1), 1), masks))
    Bp = _copy(e0['Bp'])
    S, IM = ia_amd.resynthesize_pyramid(z1['A_pyr'], z1['Ap_pyr'], z1['B_pyr'], Bp, e0['s'], e0['im'], m, c, ctx=ctx, grow=1)
    for level in range(1, L):
        assert np.array_equal(S[level], want['s'][level]) and np.array_equal(IM[level], want['im'][level])
        assert np.array_equal(Bp[level], want['Bp'][level])
    # without a previous state: hole filling
    Bp = _copy(e0['Bp'])
    S, IM = ia_amd.resynthesize_pyramid(z1['A_pyr'], z1['Ap_pyr'], z1['B_pyr'], Bp, None, None, m, c, ctx=ctx, grow=1)
    hole = MI.resynthesize(z1, _copy(e0['Bp']), masks)
    for level in range(1, L):
        assert np.array_equal(S[level], hole['s'][level]) and np.array_equal(IM[level], hole['im'][level])
        assert np.array_equal(Bp[level], hole['Bp'][level])

"""GPU parity for exact levels of other window sizes (include/ia.h ia_synthesize_levels_nbhd, DESIGN.md
section 11).  Every comparison is bit for bit, without a tolerance: at (3, 5) against the reference's recorded
runs, at every other size against the numpy restatement in tests/windows_inputs.py, which
tests/test_windows_cpu.py pins to the oracle and to the package's own feature rows.

Shapes are the smallest at which the kernels can go wrong (windows_inputs: A 25 x 19 / B 16 x 20 over three
levels, 475 DB rows = 15 tiles with a partial last one; borders narrower than the pad; a 1 x 1 A; steps of 1 to
9 query tiles, i.e. one to three scan blocks)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

import windows_inputs as WI
from golden_util import load_e2e

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    """a context of this module's own: the session's may be left recording (pipeline_record) or
    shard-emulating by the tests before, which this call refuses"""
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


def _run(ctx, Z, win, st=None):
    """every level of the jobs Z (one A side), one call per level.  Returns ([{level: (s, im)}], [B' pyramid], Stats)"""
    from ia_amd import _native
    st = st if st is not None else _native.Stats()
    z0 = Z[0]
    Bp = [[x.copy() for x in z['Bp_init']] for z in Z]
    out = [dict() for _ in Z]
    for level in range(1, z0['L']):
        A, Ac = _a_side(z0, level)
        res = ctx.synthesize_levels(A, Ac, [p[level] for p in z0['Ap_pyr']], [p[level - 1] for p in z0['Ap_pyr']],
                                    [_job(z, level, Bp[j]) for j, z in enumerate(Z)], st, windows=win)
        for j, r in enumerate(res):
            out[j][level] = r
    return out, Bp, st


def _same(out, Bp, e, L, what=''):
    for level in range(1, L):
        assert np.array_equal(out[level][0], e['s'][level]), (what, level)
        assert np.array_equal(out[level][1], e['im'][level]), (what, level)
        assert np.array_equal(Bp[level], e['Bp'][level]), (what, level)


def _check_case(ctx, name):
    z, e = WI.make(name), WI.expected(name)
    out, Bp, st = _run(ctx, [z], z['win'])
    _same(out[0], Bp[0], e, z['L'], name)
    assert st.nbhd_levels == z['L'] - 1 and st.kappa_ambiguous == 0
    assert st.coherence_wins == sum(1 for x in e['log'] if x[4] is not None and x[4][1] <= x[4][0] * x[5])
    assert st.pixels == sum(z['B_pyr'][l].shape[0] * z['B_pyr'][l].shape[1] for l in range(1, z['L']))
    return st


# ---- 1. (3, 5) through the new call = the reference's recorded runs ----------------------------------------
@pytest.mark.parametrize('case', ['g32', 'rect', 'multiap', 'rgb3', 'ties', 'noinit'])
def test_3_5_equals_the_recorded_reference_runs(ctx, case):
    z = load_e2e(case)
    z['k'] = float(z['k'])
    out, Bp, st = _run(ctx, [z], (3, 5))
    _same(out[0], Bp[0], dict(s=z['s'], im=z['im'], Bp=z['Bp_final']), z['L'], case)
    assert st.nbhd_levels == z['L'] - 1 and st.f16_levels == 0 and st.kcoh_levels == 0
    assert st.dist_launches >= st.steps - 2 * (z['L'] - 1)   # a scan per step that holds a pixel


# ---- 2. sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', WI.SIZE_CASES)
def test_sizes_equal_the_restatement(ctx, name):
    st = _check_case(ctx, name)
    print('NBHD', name, 'coherence wins', st.coherence_wins, 'of', st.pixels)


# ---- 3. borders -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', WI.BORDER_CASES)
def test_borders_equal_the_restatement(ctx, name):
    _check_case(ctx, name)


# ---- 4. wide steps ----------------------------------------------------------------------------------------
def test_wide_32_jobs_three_scan_blocks(ctx):
    """32 jobs (job j = variant j mod 4) on B 9 x 45 at (3, 9): 288 queries = 9 tiles at the widest, three blocks
    of KH 84's three tiles with qt0 = 0, 3, 6.  Every job equals its variant's restatement and a separate call."""
    names = ['wide45_v%d' % v for v in range(4)]
    V, E = [WI.make(n) for n in names], [WI.expected(n) for n in names]
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(E[i]['s'][1], E[j]['s'][1])
    out, Bp, st = _run(ctx, [V[j % 4] for j in range(32)], (3, 9))
    for j in range(32):
        _same(out[j], Bp[j], E[j % 4], 2, 'job %d' % j)
    T, mmax, tiles = WI.step_shape(9, 45, 4, 32)
    assert mmax * 32 == 288 and st.steps == T and st.nbhd_levels == 32
    assert st.dist_launches == sum(-(-(-(-32 * len(v) // 32)) // 3) for v in WI.steps(9, 45, 4).values()) > T
    out1, Bp1, _ = _run(ctx, [V[1]], (3, 9))
    _same(out1[0], Bp1[0], E[1], 2, 'separate')


def test_wide_2_jobs_two_tiles_kh56(ctx):
    names = ['wide70_v0', 'wide70_v1']
    V, E = [WI.make(n) for n in names], [WI.expected(n) for n in names]
    assert WI.step_shape(17, 70, 3, 2)[1] * 2 == 34
    out, Bp, st = _run(ctx, V, (3, 7))
    for j in range(2):
        _same(out[j], Bp[j], E[j], 2, 'job %d' % j)
        o1, b1, _ = _run(ctx, [V[j]], (3, 7))
        _same(o1[0], b1[0], E[j], 2, 'separate %d' % j)


# ---- 5. certification edges at (3, 7) ---------------------------------------------------------------------
@pytest.mark.parametrize('name', ['edge_' + n for n in WI.EDGE_CASES] + ['x1000'])
def test_certification_edges_equal_the_restatement(ctx, name):
    _check_case(ctx, name)


@pytest.mark.parametrize('mem', ['host', 'device'])
def test_big_db_rows_past_the_first_grid_trip(ctx, mem):
    """edge_bigA_3_9: 8,280 rows x 139 = 1,150,920 DB elements, 102,344 more than k_nbhd_rows' 4,096 x 256 grid,
    so its grid-stride loop takes a second trip for the rows from 7,543 on (tests/test_windows_cpu.py pins that
    5 final sources and 12 NN rows lie there).  It runs after calls that leave other rows in the context's DB
    buffer - the cases above, and first, here, bigA_neartie at the same sizes, whose result is not looked at -
    so a tail that was not written holds another A's rows at these very places: wrong, not accidentally right."""
    from ia_amd import _native
    name = 'edge_bigA_3_9'
    z, e = WI.make(name), WI.expected(name)
    _run(ctx, [WI.sized(WI.AI.make('bigA_neartie'), 3, 9)], (3, 9))
    T, mmax, tiles = WI.step_shape(12, 16, 4)
    if mem == 'host':
        st = _check_case(ctx, name)
        assert st.nbhd_levels == 1 and st.steps == T == 71 and st.dist_launches == tiles == T    # one query tile a step
        return
    st = _native.Stats()
    Bp = [x.copy() for x in z['Bp_init']]
    D = _device_level(z, 1, Bp)
    ctx.synthesize_level_device(1, 1, z['A_pyr'][1].shape[:2], z['B_pyr'][1].shape[:2], {k: v.data_ptr() for k, v in D.items()},
                                1 + (2 ** (1 - z['L'])) * z['k'], st, windows=(3, 9))
    torch.cuda.synchronize()
    assert np.array_equal(D['s_out'].cpu().numpy(), e['s'][1]) and np.array_equal(D['im_out'].cpu().numpy(), e['im'][1])
    assert np.array_equal(D['Bp'].cpu().numpy(), e['Bp'][1])
    assert st.nbhd_levels == 1 and st.steps == T and st.dist_launches == tiles


# ---- 6. training pairs ------------------------------------------------------------------------------------
def test_pairs_equal_the_restatement(ctx):
    z = WI.make('pairs2')
    assert len(z['A_pairs']) == len(z['Ap_pyr']) == 2
    _check_case(ctx, 'pairs2')
    assert set(WI.expected('pairs2')['im'][1]) == {0, 1}


# ---- 7. memory kinds --------------------------------------------------------------------------------------
def _device_level(z, level, Bp):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to('cuda:0')
    h, w = z['B_pyr'][level].shape[:2]
    T = dict(A=t(z['A_pyr'][level]), Ac=t(z['A_pyr'][level - 1]), Ap=t(np.stack([p[level] for p in z['Ap_pyr']])),
             Apc=t(np.stack([p[level - 1] for p in z['Ap_pyr']])), B=t(z['B_pyr'][level]), Bc=t(z['B_pyr'][level - 1]),
             Bpc=t(Bp[level - 1]), Bp=t(Bp[level]), weights=t(z['weights']),
             s_out=torch.zeros((h * w, 2), dtype=torch.int32, device='cuda:0'),
             im_out=torch.zeros(h * w, dtype=torch.int32, device='cuda:0'))
    torch.cuda.synchronize()
    return T


def test_device_memory_equals_host_memory(ctx):
    name = 'size_c1_3_7'
    z, e = WI.make(name), WI.expected(name)
    Bp = [x.copy() for x in z['Bp_init']]
    for level in range(1, z['L']):
        T = _device_level(z, level, Bp)
        ctx.synthesize_level_device(1, 1, z['A_pyr'][level].shape[:2], z['B_pyr'][level].shape[:2],
                                    {k: v.data_ptr() for k, v in T.items()}, 1 + (2 ** (level - z['L'])) * z['k'], windows=(3, 7))
        torch.cuda.synchronize()
        Bp[level] = T['Bp'].cpu().numpy()
        assert np.array_equal(T['s_out'].cpu().numpy(), e['s'][level]) and np.array_equal(T['im_out'].cpu().numpy(), e['im'][level])
        assert np.array_equal(Bp[level], e['Bp'][level])


# ---- 8. refusals ------------------------------------------------------------------------------------------
def _level_args(z, level, Bp, s, im, dbg=None):
    """one host-memory ia_level_args for level `level` (the arrays are kept alive by the caller's z / Bp)"""
    from ia_amd import _native
    c64 = lambda x: np.array(x, dtype=np.float64, order='C')   # copies: a test may poison them
    ch = 1 if z['A_pyr'][level].ndim == 2 else z['A_pyr'][level].shape[2]
    keep = [c64(z['A_pyr'][level]), c64(z['A_pyr'][level - 1]), c64(np.stack([p[level] for p in z['Ap_pyr']])),
            c64(np.stack([p[level - 1] for p in z['Ap_pyr']])), c64(z['B_pyr'][level]), c64(z['B_pyr'][level - 1]),
            c64(Bp[level - 1]), Bp[level], c64(z['weights'])]
    p = [_native._ptr(x) for x in keep]
    a = _native.LevelArgs(ch, len(z['Ap_pyr']), z['A_pyr'][level].shape[0], z['A_pyr'][level].shape[1],
                          z['B_pyr'][level].shape[0], z['B_pyr'][level].shape[1], p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7],
                          p[8], 1.25, _native._ptr(s), _native._ptr(im), _native.IA_MEM_HOST,
                          None if dbg is None else _native._ptr(dbg[0]), None if dbg is None else _native._ptr(dbg[1]), 0)
    return a, keep


def _refused(ctx, z, win, match, dbg=False, mutate=None):
    import ctypes
    from ia_amd import _native
    level = z['L'] - 1
    Bp = [np.ascontiguousarray(x.copy()) for x in z['Bp_init']]
    n = Bp[level].shape[0] * Bp[level].shape[1]
    s, im = np.full((n, 2), -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    d = (np.full((n, 6), -7, dtype=np.int32), np.full((n, 2), -7.0)) if dbg else None
    a, keep = _level_args(z, level, Bp, s, im, d)
    if mutate is not None:
        mutate(keep)
    arr = (_native.LevelArgs * 1)(a)
    st = _native.Stats()
    rc = _native.lib().ia_synthesize_levels_nbhd(ctx.handle, arr, 1, win[0], win[1], ctypes.byref(st))
    assert rc == -1, rc                                        # IA_EINVAL
    msg = _native.lib().ia_last_error().decode()
    assert match in msg, msg
    assert (s == -7).all() and (im == -7).all() and np.array_equal(Bp[level], z['Bp_init'][level])   # nothing written
    assert st.nbhd_levels == 0 and st.pixels == 0
    return msg


def test_refusals_leave_outputs_and_context_intact(ctx):
    from ia_amd import _native
    z1 = WI.rand_case(380, 3, 7, geo=dict(a_hw=(12, 10), b_hw=(6, 7), L=2))
    z3 = WI.rand_case(381, 3, 3, geo=dict(a_hw=(12, 10), b_hw=(6, 7), L=2), ch=3)
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
        e = WI.run(z1)                                        # the dependency was consumed: the next call runs
        out, Bp, _ = _run(c2, [z1], (3, 7))
        _same(out[0], Bp[0], e, 2, 'after the refusals')
    finally:
        c2.close()
        c3.close()

    def poison(keep):
        keep[2][0, 3, 4] = np.inf                             # one A' value

    _refused(ctx, z1, (3, 7), 'finite', mutate=poison)

    def poison_nan(keep):
        keep[1][1, 2] = np.nan                                # one coarse A value

    _refused(ctx, z1, (3, 7), 'finite', mutate=poison_nan)
    out, Bp, _ = _run(ctx, [z1], (3, 7))                      # the session's context is still usable
    _same(out[0], Bp[0], WI.run(z1), 2, 'after the refusals')


def test_side_calls_share_one_refusal_rule():
    """The window, masked and k-coherence calls refuse a shard-emulating context and a pending ia_pipeline_depend
    by one rule: IA_EINVAL, a message naming the entry point and the reason, nothing written - and the refusal
    consumes the dependency, so the same call on the same context then runs.  One 8 x 8 level, one job."""
    import ctypes
    from ia_amd import _native
    L = _native.lib()
    z = WI.rand_case(382, 3, 5, geo=dict(a_hw=(8, 8), b_hw=(8, 8), L=2))
    assert z['A_pyr'][1].shape == z['B_pyr'][1].shape == (8, 8)
    sim = ((np.arange(64, dtype=np.int32) + 1) % 64).reshape(64, 1).copy()        # valid sets, sim_k = 1
    mask, s_in, im_in = np.ones(64, dtype=np.uint8), np.zeros((64, 2), dtype=np.int32), np.full(64, -1, dtype=np.int32)
    one = lambda x: (ctypes.c_void_p * 1)(x.ctypes.data)
    calls = [
        ('ia_synthesize_levels_nbhd', lambda c, arr, st: L.ia_synthesize_levels_nbhd(c.handle, arr, 1, 3, 5, st)),
        ('ia_synthesize_levels_masked', lambda c, arr, st: L.ia_synthesize_levels_masked(c.handle, arr, 1, 3, 5, one(mask),
                                                                                         one(s_in), one(im_in), st)),
        ('ia_synthesize_level: k-coherence', lambda c, arr, st: L.ia_synthesize_levels_kcoh(c.handle, arr, 1, _native._ptr(sim),
                                                                                            1, st)),
    ]

    def attempt(c, call):
        Bp = [np.ascontiguousarray(x.copy()) for x in z['Bp_init']]
        s, im = np.full((64, 2), -7, dtype=np.int32), np.full(64, -7, dtype=np.int32)
        a, keep = _level_args(z, 1, Bp, s, im)
        rc = call(c, (_native.LevelArgs * 1)(a), ctypes.byref(_native.Stats()))
        untouched = bool((s == -7).all() and (im == -7).all() and np.array_equal(Bp[1], z['Bp_init'][1]))
        return rc, L.ia_last_error().decode() if rc else '', untouched, im

    def refused(c, who, call, reason):
        rc, msg, untouched, _ = attempt(c, call)
        assert rc == -1, (who, rc)                                                # IA_EINVAL
        assert who in msg and reason in msg, msg
        assert untouched, who

    c2, c3 = _native.Context(0), _native.Context(0)
    try:
        c3.set_option('pipeline_record', 1)
        for who, call in calls:
            c2.set_option('shard_emulate', 2)
            refused(c2, who, call, 'shard')
            c2.set_option('shard_emulate', 1)
            c2.pipeline_depend(c3, 1)
            refused(c2, who, call, 'pipelined')
            rc, msg, _, im = attempt(c2, call)                                    # the dependency was consumed
            assert rc == 0, (who, rc, msg)
            assert (im >= 0).all(), who                                           # every pixel took a source
    finally:
        c2.close()
        c3.close()


# ---- 9. end to end ----------------------------------------------------------------------------------------
def test_set_windows_and_synthesize_pyramid(ctx):
    from ia_amd import config, image_analogies as IAm
    z = WI.rand_case(390, 3, 7, geo=dict(a_hw=(24, 24), b_hw=(24, 24), L=3))
    keep = (config.n_sm, config.n_lg, config.max_levels, config.k, config.weights, config.num_ch, config.kcoh_k)
    try:
        config.max_levels, config.k = z['L'], z['k']
        config.n_lg = 7
        with pytest.raises(ValueError, match='set_windows'):
            IAm.synthesize_pyramid(z['A_pyr'], z['Ap_pyr'], z['B_pyr'], [x.copy() for x in z['Bp_init']], config, ctx=ctx)
        config.set_windows(3, 7)
        assert (config.n_half, config.pad_sm, config.pad_lg) == (24, 1, 3)
        config.num_ch, _, _, config.weights = config.setup_vars(z['A_pyr'][-1])
        assert np.array_equal(config.weights, z['weights'])
        config.kcoh_k = 2
        with pytest.raises(ValueError, match='n_sm = 3, n_lg = 5 only'):
            IAm.synthesize_pyramid(z['A_pyr'], z['Ap_pyr'], z['B_pyr'], [x.copy() for x in z['Bp_init']], config, ctx=ctx)
        config.kcoh_k = 0
        with pytest.raises(ValueError, match='n_sm = 3, n_lg = 5 only'):
            IAm.synthesize_pyramid(z['A_pyr'], z['Ap_pyr'], z['B_pyr'], [x.copy() for x in z['Bp_init']], config, ctx=ctx,
                                   debug={})
        Bp = [x.copy() for x in z['Bp_init']]
        S, IM = IAm.synthesize_pyramid(z['A_pyr'], z['Ap_pyr'], z['B_pyr'], Bp, config, ctx=ctx)
        e = WI.run(z)
        for level in range(1, z['L']):
            assert np.array_equal(S[level], e['s'][level]) and np.array_equal(IM[level], e['im'][level])
            assert np.array_equal(Bp[level], e['Bp'][level])
    finally:
        config.set_windows(keep[0], keep[1])
        config.max_levels, config.k, config.weights, config.num_ch, config.kcoh_k = keep[2:]


def test_image_analogies_main_after_a_job_of_other_channels(ctx, tmp_path):
    """the driver end to end: a 3-channel job at (1, 3), then a 1-channel job at (3, 9), which 3 channels could
    not take (417 features): the sizes are checked against the job's own images.  Both equal the restatement run
    on the pyramids img_setup made."""
    from ia_amd import algorithms, config, image_analogies as IAm
    rs = np.random.RandomState(5)
    names = ['n_sm', 'n_lg', 'max_levels', 'weights', 'num_ch', 'seed', 'padding_sm', 'padding_lg', 'convert', 'remap_lum',
             'init_rand', 'AB_weight', 'k', 'n_levels', 'level_align', 'gpu_preprocess', 'kcoh_k']
    keep = {n: getattr(config, n) for n in names}          # (the module is the reference's mutable namespace)
    keep_ctx = algorithms._CTX
    try:
        algorithms._CTX = ctx                              # the driver's context: this module's
        config.seed, config.convert, config.remap_lum, config.init_rand, config.AB_weight, config.k = 3, False, False, True, 1, 0.5
        config.n_levels, config.level_align, config.gpu_preprocess, config.kcoh_k = None, 'coarse', True, 0
        for win, shp in [((1, 3), (20, 17, 3)), ((3, 9), (24, 24))]:
            A, Ap, B = rs.rand(*shp), rs.rand(*shp), rs.rand(*shp)
            config.set_windows(*win)
            out = str(tmp_path) + '/%d_%d/' % win
            A_pyr, Ap_l, B_pyr, Bp_pyr, _, c = IAm.img_setup(A, [Ap], B, out, config)
            z = dict(A_pyr=A_pyr, Ap_pyr=Ap_l, B_pyr=B_pyr, Bp_init=Bp_pyr, L=c.max_levels, k=c.k, weights=c.weights, win=win)
            e = WI.run(z)
            r = IAm.image_analogies_main(A, [Ap], B, out, config)
            assert r['stats']['nbhd_levels'] == z['L'] - 1 >= 3
            for level in range(1, z['L']):
                assert np.array_equal(r['s'][level], e['s'][level]) and np.array_equal(r['im'][level], e['im'][level])
                assert np.array_equal(r['Bp_pyr'][level], e['Bp'][level])
    finally:
        algorithms._CTX = keep_ctx
        config.set_windows(keep['n_sm'], keep['n_lg'])
        for n in names[2:]:
            setattr(config, n, keep[n])

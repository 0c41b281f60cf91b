"""GPU parity for k-coherence search (include/ia.h ia_synthesize_levels_kcoh, ia_index_similarity;
DESIGN.md section 10).  Every comparison is bit-exact against the numpy restatement of the rule in
tests/kcoh_inputs.py, which tests/test_kcoh_cpu.py pins to the oracle.

The shapes are the smallest at which the step kernel can go wrong: 120 DB rows and a 11 x 13 B (more
than one pixel per step, three or more fallback pixels), K = 1, 4, 5 and 15 for one, two and three
rounds of 64 candidate lanes, 2 and 3 channels (their own kernel instances), two A' images on one A
and two pairs, B widths 1 to 3 (steps without a pixel), a 1 x 1 A where every pixel falls back, a
constant A (every distance ties: the (d, row) rule alone decides) and kappa 0 and 25.
A rank of a multi-process shard cannot be made on one GPU: that refusal shares its check with the
emulated shard's, which is tested."""
import types

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

import kcoh_inputs as KI

pytestmark = pytest.mark.gpu


def _a_side(z, level):
    if 'A_pairs' in z:
        return [p[level] for p in z['A_pairs']], [p[level - 1] for p in z['A_pairs']]
    return z['A_pyr'][level], z['A_pyr'][level - 1]


def _job(z, level, Bp):
    return dict(B=z['B_pyr'][level], Bc=z['B_pyr'][level - 1], Bpc=Bp[level - 1], Bp=Bp[level], weights=z['weights'],
                kappa_factor=1 + (2 ** (level - z['L'])) * z['k'])


def _run(ctx, Z, sims, st=None):
    """every level of the jobs Z (one A side), one synthesize_levels call per level; sims: {level: sim}
    (a level it lacks runs exactly).  Returns ([{level: (s, im)}] per job, [B' pyramid] per job, Stats)"""
    from ia_amd import _native
    st = st if st is not None else _native.Stats()
    z0 = Z[0]
    Bp = [[x.copy() for x in z['Bp_init']] for z in Z]
    out = [dict() for _ in Z]
    for level in range(1, z0['L']):
        A, Ac = _a_side(z0, level)
        res = ctx.synthesize_levels(A, Ac, [p[level] for p in z0['Ap_pyr']], [p[level - 1] for p in z0['Ap_pyr']],
                                    [_job(z, level, Bp[j]) for j, z in enumerate(Z)], st, sim=sims.get(level))
        for j, r in enumerate(res):
            out[j][level] = r
    return out, Bp, st


def _same(out, Bp, e, levels):
    for level in levels:
        assert np.array_equal(out[level][0], e['s'][level]) and np.array_equal(out[level][1], e['im'][level]), level
        assert np.array_equal(Bp[level], e['Bp'][level]), level


# ---- 1. similarity sets -----------------------------------------------------------------------------------
def _index_rows(kind):
    rs = np.random.RandomState(70)
    if kind == 'rand300':
        return rs.rand(300, 55)
    if kind == 'equal':
        return np.full((40, 55), 0.25)
    if kind == 'pairs':                       # rows 2i and 2i + 1 are equal
        return np.repeat(rs.rand(20, 55), 2, axis=0)
    return rs.rand(int(kind[1:]), 55)         # 'n5': n = K + 1 with K = 4


@pytest.mark.parametrize('kind,K', [('rand300', 1), ('rand300', 4), ('rand300', 15), ('equal', 4), ('equal', 15),
                                    ('pairs', 1), ('pairs', 4), ('n5', 4), ('n16', 15), ('n2', 1)])
def test_index_similarity_equals_numpy(ctx, kind, K):
    from ia_amd import _native
    rows = _index_rows(kind)
    index = _native.ExactIndex(ctx, rows)
    sim = index.similarity(K)
    assert sim.dtype == np.int32 and sim.shape == (len(rows), K)
    assert np.array_equal(sim, KI.similarity_sets(rows, K))
    for bad in (0, -1, 16, len(rows)):
        before = sim.copy()
        with pytest.raises(_native.IAError, match='IA_EINVAL'):
            index.similarity(bad)
        assert np.array_equal(sim, before)
    index.close()


# ---- 2. level parity --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,K', KI.LEVEL_RUNS, ids=['%s-K%d' % r for r in KI.LEVEL_RUNS])
def test_level_equals_the_restatement(ctx, case, K):
    z, e = KI.make(case), KI.expected(case, K)
    assert e['kcoh_levels'] == [1]
    out, Bp, st = _run(ctx, [z], e['sim'])
    n_px = z['B_pyr'][1].shape[0] * z['B_pyr'][1].shape[1]
    print('KCOH %-7s K %2d: fallbacks %d of %d pixels, candidates %d, coherence wins %d'
          % (case, K, st.kcoh_fallbacks, n_px, st.kcoh_candidates, st.coherence_wins))
    _same(out[0], Bp[0], e, [1])
    assert st.kcoh_levels == 1 and st.pixels == n_px
    assert st.kcoh_fallbacks == e['fallbacks'][1] and st.kcoh_candidates == e['candidates'][1]
    assert st.dist_launches == 0 and st.f16_levels == 0 and st.reranked == 0 and st.fallbacks == 0   # no scan ran
    if case == 't11':
        assert st.kcoh_fallbacks == n_px


def test_similarity_of_the_level_rows_is_what_the_level_takes(ctx):
    """ExactIndex.similarity on create_index's rows of the level = the restatement's sets, shared A and pairs"""
    from ia_amd import _native
    for case in ('main', 'pairs2', 'c3'):
        z, e = KI.make(case), KI.expected(case, 4)
        index = _native.ExactIndex(ctx, KI.PI.build_db(z, 1))
        assert np.array_equal(index.similarity(4), e['sim'][1])
        index.close()


def test_fallback_scan_on_256_waves(ctx):
    """16,510 DB rows: the pixels without a base row are scanned by 256 waves of 65 rows each (the last
    two without a row), the last one in reducing their minima.  The sets come from the GPU index
    (pinned to numpy above: a brute force of this size takes too long here); the level is the
    restatement's on those sets."""
    from ia_amd import _native
    z = KI.rand_case(15, dict(a_hw=(130, 127), b_hw=(5, 7), L=2))
    As = KI.PI.build_db(z, 1)
    assert len(As) == 16510
    index = _native.ExactIndex(ctx, As)
    sim = index.similarity(4)
    index.close()
    Bp = [x.copy() for x in z['Bp_init']]
    with KI.blas_order():
        s, im, fallbacks, candidates = KI.synthesize_level(z['Ap_pyr'], KI.O.feature_array(z['B_pyr'], 1, True), Bp, 1, z['L'],
                                                           z['k'], z['weights'], As, sim)
    out, Bp_g, st = _run(ctx, [z], {1: sim})
    assert np.array_equal(out[0][1][0], s) and np.array_equal(out[0][1][1], im) and np.array_equal(Bp_g[0][1], Bp[1])
    assert st.kcoh_fallbacks == fallbacks >= 1 and st.kcoh_candidates == candidates


# ---- 3. K = N_A - 1 is the exact path ---------------------------------------------------------------------
@pytest.mark.parametrize('case,K', KI.FULL_K[:2], ids=['t44', 't23'])
def test_full_sets_equal_the_exact_gpu_path_and_the_oracle(ctx, case, K):
    z, e, ex = KI.make(case), KI.expected(case, K), KI.expected(case, K, exact=True)
    out_k, Bp_k, st_k = _run(ctx, [z], e['sim'])
    out_e, Bp_e, st_e = _run(ctx, [z], {})
    assert st_k.kcoh_levels == 1 and st_e.kcoh_levels == 0 and st_e.dist_launches > 0
    for out, Bp in ((out_k, Bp_k), (out_e, Bp_e)):
        _same(out[0], Bp[0], ex, [1])
    assert st_k.kcoh_fallbacks == e['fallbacks'][1]


# ---- 4. batches -------------------------------------------------------------------------------------------
def test_batch_of_three_jobs_equals_separate_calls(ctx):
    names = ['main', 'main_job1', 'main_job2']
    Z = [KI.make(n) for n in names]
    E = [KI.expected(n, 4) for n in names]
    assert all(np.array_equal(e['sim'][1], E[0]['sim'][1]) for e in E)   # one A side
    out, Bp, st = _run(ctx, Z, E[0]['sim'])
    for j, z in enumerate(Z):
        _same(out[j], Bp[j], E[j], [1])
        o1, b1, _ = _run(ctx, [z], E[0]['sim'])
        _same(o1[0], b1[0], E[j], [1])
    assert st.kcoh_levels == 3 and st.kcoh_fallbacks == sum(e['fallbacks'][1] for e in E)
    assert st.kcoh_candidates == sum(e['candidates'][1] for e in E)


def test_wide_32_jobs_fallbacks_beyond_the_first_64_queries(ctx):
    """32 jobs on main's A side (job j = variant j mod 4, K = 4) in one call: steps of up to 160 queries, which
    the scan waves test 64 at a time.  tests/test_kcoh_cpu.py pins pixels without a base row at queries 64 ..
    115 of step 9 and at 130 and 150 of step 21: the second and third trip find them, scan the DB for them and
    finish them.  Every job equals its variant's restatement.
    The call runs after one that leaves other, valid sources in all 32 jobs' s / im buffers (the jobs rotated by one
    variant, on the exact path, result not looked at): a pixel that no wave finished then keeps another job's
    source - wrong, and not whatever a fresh allocation holds."""
    names = ['wide32_v%d' % v for v in range(4)]
    V, E = [KI.make(n) for n in names], [KI.expected(n, KI.WIDE32_K) for n in names]
    assert all(np.array_equal(e['sim'][1], E[0]['sim'][1]) for e in E)   # one A side
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(E[i]['s'][1], E[j]['s'][1])
    _run(ctx, [V[(j + 1) % 4] for j in range(32)], {})
    out, Bp, st = _run(ctx, [V[j % 4] for j in range(32)], E[0]['sim'])
    for j in range(32):
        _same(out[j], Bp[j], E[j % 4], [1])
    assert st.kcoh_levels == 32 and st.pixels == 32 * 143 and st.dist_launches == 0
    assert st.kcoh_fallbacks == 8 * sum(e['fallbacks'][1] for e in E) == 136
    assert st.kcoh_candidates == 8 * sum(e['candidates'][1] for e in E)


# ---- 5. device pointers -----------------------------------------------------------------------------------
def _device_level(z, level, Bp, sim):
    """the tensors of one level on cuda:0, sim included"""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to('cuda:0')
    h, w = z['B_pyr'][level].shape[:2]
    A = z['A_pairs'] if 'A_pairs' in z else [z['A_pyr']]
    T = dict(A=t(np.stack([p[level] for p in A])), Ac=t(np.stack([p[level - 1] for p in A])),
             Ap=t(np.stack([p[level] for p in z['Ap_pyr']])), Apc=t(np.stack([p[level - 1] for p in z['Ap_pyr']])),
             B=t(z['B_pyr'][level]), Bc=t(z['B_pyr'][level - 1]), Bpc=t(Bp[level - 1]), Bp=t(Bp[level]),
             weights=t(z['weights']), s_out=torch.zeros((h * w, 2), dtype=torch.int32, device='cuda:0'),
             im_out=torch.zeros(h * w, dtype=torch.int32, device='cuda:0'),
             sim=torch.from_numpy(np.ascontiguousarray(sim, dtype=np.int32)).to('cuda:0'))
    torch.cuda.synchronize()
    return T


@pytest.mark.parametrize('case', ['main', 'pairs2'])
def test_device_pointers_equal_the_restatement(ctx, case):
    from ia_amd import _native
    z, e = KI.make(case), KI.expected(case, 4)
    Bp = [x.copy() for x in z['Bp_init']]
    T = _device_level(z, 1, Bp, e['sim'][1])
    st = _native.Stats()
    n_ap = len(z['Ap_pyr'])
    ctx.synthesize_level_device(1, n_ap, z['A_pyr'][1].shape[:2], z['B_pyr'][1].shape[:2], {k: v.data_ptr() for k, v in T.items()},
                                1 + (2 ** (1 - z['L'])) * z['k'], st, n_a=n_ap if 'A_pairs' in z else 0,
                                sim=T['sim'].data_ptr(), sim_k=4)
    torch.cuda.synchronize()
    assert np.array_equal(T['s_out'].cpu().numpy(), e['s'][1]) and np.array_equal(T['im_out'].cpu().numpy(), e['im'][1])
    assert np.array_equal(T['Bp'].cpu().numpy(), e['Bp'][1])
    assert st.kcoh_levels == 1 and st.kcoh_fallbacks == e['fallbacks'][1]


# ---- 6. refusals ------------------------------------------------------------------------------------------
def test_refusals_return_einval_and_write_nothing(ctx):
    from ia_amd import _native
    z, e = KI.make('main'), KI.expected('main', 4)
    sim = e['sim'][1]
    n = len(sim)
    Bp = [x.copy() for x in z['Bp_init']]
    a_hw, b_hw = z['A_pyr'][1].shape[:2], z['B_pyr'][1].shape[:2]
    T = _device_level(z, 1, Bp, np.hstack([sim, sim, sim, sim]))     # (n, 16): room for every sim_k tried
    ptrs = {k: v.data_ptr() for k, v in T.items()}

    def untouched():
        torch.cuda.synchronize()
        assert int(T['s_out'].abs().sum()) == 0 and int(T['im_out'].abs().sum()) == 0
        assert np.array_equal(T['Bp'].cpu().numpy(), z['Bp_init'][1])

    def refused(sim=ptrs['sim'], **kw):
        with pytest.raises(_native.IAError, match='IA_EINVAL'):
            ctx.synthesize_level_device(1, 1, a_hw, b_hw, ptrs, 1.25, sim=sim, **kw)
        untouched()

    refused(sim_k=16)
    refused(sim_k=-1)
    refused(None, sim_k=4)                                           # sim NULL with sim_k > 0
    # sim_k above N_A - 1: the 2 x 3 A has 6 rows
    z6 = KI.make('t23')
    T6 = _device_level(z6, 1, [x.copy() for x in z6['Bp_init']], np.zeros((6, 6), dtype=np.int32))
    with pytest.raises(_native.IAError, match='IA_EINVAL'):
        ctx.synthesize_level_device(1, 1, (2, 3), z6['B_pyr'][1].shape[:2], {k: v.data_ptr() for k, v in T6.items()}, 1.25,
                                    sim=T6['sim'].data_ptr(), sim_k=6)
    torch.cuda.synchronize()
    assert int(T6['s_out'].abs().sum()) == 0 and np.array_equal(T6['Bp'].cpu().numpy(), z6['Bp_init'][1])
    # a sim entry outside [0, N_A): N_A in the last place, -1 in the first
    for where, v in (((n - 1, 3), n), ((0, 0), -1)):
        bad = sim.copy()
        bad[where] = v
        Tb = torch.from_numpy(bad).to('cuda:0')
        refused(Tb.data_ptr(), sim_k=4)
        with pytest.raises(_native.IAError, match='IA_EINVAL'):     # host memory too
            ctx.synthesize_level(z['A_pyr'][1], z['A_pyr'][0], [p[1] for p in z['Ap_pyr']], [p[0] for p in z['Ap_pyr']],
                                 sim=bad, **_job(z, 1, Bp))
        assert np.array_equal(Bp[1], z['Bp_init'][1])
    # debug buffers
    with pytest.raises(_native.IAError, match='IA_EINVAL'):
        ctx.synthesize_level(z['A_pyr'][1], z['A_pyr'][0], [p[1] for p in z['Ap_pyr']], [p[0] for p in z['Ap_pyr']],
                             sim=sim, debug={}, **_job(z, 1, Bp))
    assert np.array_equal(Bp[1], z['Bp_init'][1])
    # an emulated shard, a recording context, a pending ia_pipeline_depend
    try:
        ctx.set_option('shard_emulate', 2)
        refused(sim_k=4)
    finally:
        ctx.set_option('shard_emulate', 1)
    try:
        ctx.set_option('pipeline_record', 1)
        refused(sim_k=4)
    finally:
        ctx.set_option('pipeline_record', 0)
    prev = _native.Context(0)
    try:
        prev.set_option('pipeline_record', 1)
        ctx.pipeline_depend(prev, 1)
        refused(sim_k=4)
    finally:
        prev.close()
    T2 = _device_level(z, 1, Bp, sim)
    # and the same arguments, unrefused, run (the pending dependency was consumed by its refusal)
    ctx.synthesize_level_device(1, 1, a_hw, b_hw, ptrs, 1 + (2 ** (1 - z['L'])) * z['k'], sim=T2['sim'].data_ptr(), sim_k=4)
    torch.cuda.synchronize()
    assert np.array_equal(T['s_out'].cpu().numpy(), e['s'][1]) and np.array_equal(T['Bp'].cpu().numpy(), e['Bp'][1])


# ---- 7. the drivers ---------------------------------------------------------------------------------------
def _cfg(**kw):
    from ia_amd import config
    c = types.SimpleNamespace(**{k: getattr(config, k) for k in dir(config) if not k.startswith('_')})
    c.convert, c.remap_lum, c.init_rand, c.AB_weight, c.k, c.seed = False, False, True, 1, 0.5, 3
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_synthesize_pyramid_honours_kcoh_k_and_min_rows(ctx, tmp_path):
    import ia_amd
    from ia_amd import _native, config
    from ia_amd.image_analogies import img_setup, synthesize_pyramid
    assert config.kcoh_k == 0 and config.kcoh_min_rows == 1024           # off by default
    rs = np.random.RandomState(80)
    A, Ap, B = rs.rand(24, 20), rs.rand(24, 20), rs.rand(24, 20)
    c = _cfg(kcoh_k=4, kcoh_min_rows=1)
    A_pyr, Ap_pyrs, B_pyr, Bp0, _, c = img_setup(A, [Ap], B, str(tmp_path) + '/o/', c)
    L = c.max_levels
    assert L >= 4
    z = dict(A_pyr=A_pyr, Ap_pyr=Ap_pyrs, B_pyr=B_pyr, Bp_init=Bp0, L=L, k=float(c.k), weights=c.weights)
    rows = [KI.n_rows(z, level) for level in range(L)]
    for min_rows in (1, 100):
        c.kcoh_min_rows = min_rows
        e = KI.run(z, 4, min_rows=min_rows)
        want = [level for level in range(1, L) if rows[level] >= max(2, min_rows)]
        assert e['kcoh_levels'] == want and 1 <= len(want) and (min_rows == 1 or len(want) < L - 1)
        st = _native.Stats()
        Bp = [x.copy() for x in Bp0]
        S, IM = synthesize_pyramid(A_pyr, Ap_pyrs, B_pyr, Bp, c, ctx=ctx, stats=st)
        for level in range(1, L):
            assert np.array_equal(S[level], e['s'][level]) and np.array_equal(IM[level], e['im'][level]), level
            assert np.array_equal(Bp[level], e['Bp'][level]), level
        assert st.kcoh_levels == len(want) and st.kcoh_fallbacks == sum(e['fallbacks'].values())
        # the sets computed once and passed in: the same run
        sims = ia_amd.build_similarity(A_pyr, Ap_pyrs, c, ctx)
        assert sorted(sims) == want and all(np.array_equal(sims[level], e['sim'][level]) for level in want)
        Bp2 = [x.copy() for x in Bp0]
        S2, _ = synthesize_pyramid(A_pyr, Ap_pyrs, B_pyr, Bp2, c, ctx=ctx, sim=sims)
        assert all(np.array_equal(S2[level], S[level]) and np.array_equal(Bp2[level], Bp[level]) for level in range(1, L))
    # the coarse levels of the second run are the exact path's
    ex = KI.run(z, 4, exact=True)
    first_exact = [level for level in range(1, L) if rows[level] < 100]
    assert first_exact and all(np.array_equal(S[level], ex['s'][level]) for level in first_exact)
    # kcoh_k = 0: every level exact
    c.kcoh_k = 0
    st = _native.Stats()
    Bp = [x.copy() for x in Bp0]
    S, IM = synthesize_pyramid(A_pyr, Ap_pyrs, B_pyr, Bp, c, ctx=ctx, stats=st)
    assert st.kcoh_levels == 0 and all(np.array_equal(S[level], ex['s'][level]) for level in range(1, L))

"""GPU parity for training pairs (A_i, A'_i): an A image of its own per A' image
(include/ia.h ia_level_args.n_a = n_ap; Context.synthesize_level with a list for A / Ac).

Only the DB build reads the A images (K0 means, K1b fp64 rows, K1 fp32 tiles; the split-f16 tiles are
made from K1b's rows), so the shapes here are the smallest at which that code can go wrong: images of
475 rows, so that 32-row tiles and K1b's 64-row waves straddle two images, at 1, 2 and 3 channels on
every scan a level can take; 518 tiles on 8 workgroups and sharded; the +-64 gate with its value at
the last element of the stacked A / Ac arrays; an A_1 far from A_0 (the centring); a batch; device
pointers; the argument errors; and the drivers.

The expected values are the oracle's (tests/pairs_inputs.py run_oracle: oracle/ia_oracle.py on a DB
built per pair), bit for bit, as in tests/test_gpu_channels.py; tests/test_pairs_cpu.py pins that
every image is picked, that the result differs from the shared-A_0 run and that the oracle's
decisions on these inputs are robust.
"""
import types

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

import pairs_inputs as PI
from golden_util import PRUNE_MIN_ROWS_DEFAULT, check_debug_records, load_e2e, sharded_scan_launches

pytestmark = pytest.mark.gpu

PRUNED = dict(prune_min_rows=1)
SHARD = dict(shard_unpruned=1, shard_emulate=2)
SETTINGS = {
    'default': {},
    'f32': dict(matcher='f32'),
    'pruned_v24': dict(PRUNED, k3p_variant=24),
    'pruned_v25': dict(PRUNED, k3p_variant=25),
    'wgs8': dict(scan_wgs=8),
    'shard2_allgather': dict(SHARD, exchange=0),
    'shard2_peerwrite': dict(SHARD, exchange=1),
    'pruned_shard2': dict(PRUNED, shard_emulate=2),
}


def _a_side(z, level):
    """the A side of a level as synthesize_level(s) takes it: lists for a pairs case"""
    if 'A_pairs' in z:
        return [p[level] for p in z['A_pairs']], [p[level - 1] for p in z['A_pairs']]
    return z['A_pyr'][level], z['A_pyr'][level - 1]


def _run_jobs(ctx, Z, setting='default', debug=True):
    """every level of the jobs Z (one A side) in one synthesize_levels call per level:
    ([out[level] = (s, im, dbg)] per job, [B' pyramid] per job, Stats)"""
    from ia_amd import _native
    opts = dict(SETTINGS[setting])
    if 'matcher' in opts:
        opts['matcher'] = _native.IA_MATCH_F32
    z0, L = Z[0], Z[0]['L']
    Bp = [[x.copy() for x in z['Bp_init']] for z in Z]
    out = [dict() for _ in Z]
    st = _native.Stats()
    try:
        for name, v in opts.items():
            ctx.set_option(name, v)
        for level in range(1, L):
            dbg = [{} if debug else None for _ in Z]
            specs = [dict(B=z['B_pyr'][level], Bc=z['B_pyr'][level - 1], Bpc=Bp[j][level - 1], Bp=Bp[j][level],
                          weights=z['weights'], kappa_factor=1 + (2 ** (level - L)) * z['k'], debug=dbg[j])
                     for j, z in enumerate(Z)]
            A, Ac = _a_side(z0, level)
            res = ctx.synthesize_levels(A, Ac, [p[level] for p in z0['Ap_pyr']], [p[level - 1] for p in z0['Ap_pyr']],
                                        specs, st)
            for j, (s, im) in enumerate(res):
                out[j][level] = (s, im, dbg[j])
    finally:
        ctx.set_option('prune_min_rows', PRUNE_MIN_ROWS_DEFAULT)
        ctx.set_option('k3p_variant', 24)
        ctx.set_option('matcher', _native.IA_MATCH_F16X3)
        ctx.set_option('scan_wgs', 256)
        ctx.set_option('shard_emulate', 1)
        ctx.set_option('shard_unpruned', 0)
        ctx.set_option('exchange', 0)
    return out, Bp, st


def _check_plain(z, out, Bp):
    for level in range(1, z['L']):
        assert np.array_equal(out[level][0], z['s'][level]) and np.array_equal(out[level][1], z['im'][level])
        assert np.array_equal(Bp[level], z['Bp_final'][level])


def _check_path(st, Z, ch, setting, gate=False):
    L = Z[0]['L']
    f16 = ch in (1, 2) and setting != 'f32' and not gate
    assert st.pixels == sum(x.shape[0] * x.shape[1] for z in Z for x in z['B_pyr'][1:])
    assert st.bound_violations == 0 and st.kappa_ambiguous == 0
    assert st.f16_levels == (len(Z) * (L - 1) if f16 else 0)
    assert st.pruned_levels == (len(Z) * (L - 1) if setting.startswith('pruned') and f16 and ch == 1 else 0)


# ---- 1. straddling rows -----------------------------------------------------------------------------------
RUNS = ([('p%d_c1' % n, s) for n in (2, 3) for s in ('default', 'f32', 'pruned_v24', 'pruned_v25')] +
        [('p%d_c2' % n, s) for n in (2, 3) for s in ('default', 'f32')] +
        [('p%d_c3' % n, 'default') for n in (2, 3)])


@pytest.mark.parametrize('case,setting', RUNS, ids=['%s-%s' % r for r in RUNS])
def test_pairs_case_matches_oracle(ctx, case, setting):
    """475 rows per image: tile 14 holds rows 448 .. 479 and K1b's wave 7 rows 448 .. 511, of two
    images (of three with 3 pairs: 950 = 29 * 32 + 22).  s, im, B', every NN row, every coherence
    pick and both compute_distance values equal the oracle's, on the path the setting names."""
    z = PI.oracle(case)
    out, Bp, st = _run_jobs(ctx, [z], setting)
    print('PAIRS %-8s %-11s fallbacks %5d reranked %5d f16_levels %d pruned_levels %d bound_violations %d'
          % (case, setting, st.fallbacks, st.reranked, st.f16_levels, st.pruned_levels, st.bound_violations))
    check_debug_records(z, out[0], Bp[0], st, case)
    _check_path(st, [z], PI.case_ch(case), setting)
    picked = set(np.concatenate([out[0][level][1] for level in range(1, z['L'])]))
    assert picked == set(range(len(z['Ap_pyr'])))   # every image is a source


# ---- 2. many tiles ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('setting', ['wgs8', 'shard2_allgather', 'shard2_peerwrite', 'pruned_shard2'])
def test_pairs_many_tiles(ctx, setting):
    """2 pairs of 92 x 90: 16,560 rows = 518 tiles, the last partial, image 1 starting inside tile 258;
    on 8 workgroups (65 tiles each, with debug records), and as two shards of the unpruned and of the
    pruned scan (sharded runs give no debug records: s, im and B')"""
    z = PI.oracle('big2')
    sharded = 'shard_emulate' in SETTINGS[setting]
    out, Bp, st = _run_jobs(ctx, [z], setting, debug=not sharded)
    print('PAIRS big2 %-17s fallbacks %5d reranked %5d dist_launches %d pruned_levels %d'
          % (setting, st.fallbacks, st.reranked, st.dist_launches, st.pruned_levels))
    if sharded:
        _check_plain(z, out[0], Bp[0])
    else:
        check_debug_records(z, out[0], Bp[0], st, 'big2')
    _check_path(st, [z], 1, setting)
    if setting.startswith('shard2'):
        assert st.dist_launches == sharded_scan_launches(z, 1, 2) == 2 * sharded_scan_launches(z, 1, 1)   # it did shard


# ---- 3. equal copies are the old path ---------------------------------------------------------------------
def test_equal_copies_reproduce_the_multiap_fixture(ctx):
    """the reference's own run with two A' images, A passed as [A, A]: the fixture, and the shared-A
    call's output bit for bit (records included)"""
    z = load_e2e('multiap')
    assert len(z['Ap_pyr']) == 2
    zp = dict(z, A_pairs=[z['A_pyr'], z['A_pyr']])
    out_p, Bp_p, st_p = _run_jobs(ctx, [zp])
    out_s, Bp_s, st_s = _run_jobs(ctx, [z])
    check_debug_records(z, out_p[0], Bp_p[0], st_p, 'multiap as pairs')
    for level in range(1, z['L']):
        for a, b in zip(out_p[0][level][:2], out_s[0][level][:2]):
            assert np.array_equal(a, b)
        assert np.array_equal(out_p[0][level][2]['src'], out_s[0][level][2]['src'])
        assert np.array_equal(out_p[0][level][2]['dist'], out_s[0][level][2]['dist'])
        assert np.array_equal(Bp_p[0][level], Bp_s[0][level])
    assert (st_p.f16_levels, st_p.reranked, st_p.fallbacks) == (st_s.f16_levels, st_s.reranked, st_s.fallbacks)


# ---- 4. the +-64 gate sees every image --------------------------------------------------------------------
@pytest.mark.parametrize('ch,kind', PI.GATE_KINDS, ids=['c%d-%s' % k for k in PI.GATE_KINDS])
def test_gate_sees_the_last_value_of_the_last_a_image(ctx, ch, kind):
    """64.5 at the last element of A_1 (kind 'A') or of its coarse level ('Ac'): the last value of the
    stacked array, which a scan sized for one image never reaches.  No split-f16 level, and the
    oracle's result; the same case without the value runs split-f16."""
    z = PI.oracle('gate_c%d_%s' % (ch, kind))
    arr = z['A_pairs'][1][1 if kind == 'A' else 0]
    assert arr[(-1,) * arr.ndim] == 64.5 and sum(int((np.abs(x) > 64).sum()) for p in z['A_pairs'] for x in p) == 1
    out, Bp, st = _run_jobs(ctx, [z])
    check_debug_records(z, out[0], Bp[0], st, 'gate %d %s' % (ch, kind))
    _check_path(st, [z], ch, 'default', gate=True)
    assert st.f16_levels == 0
    z_in = PI.oracle('gate_c%d_in' % ch)
    out, Bp, st = _run_jobs(ctx, [z_in])
    check_debug_records(z_in, out[0], Bp[0], st, 'gate %d in range' % ch)
    assert st.f16_levels == z_in['L'] - 1


# ---- 5. centring ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setting', ['default', 'f32', 'pruned_v24'])
def test_centring_over_both_images(ctx, setting):
    """A_0 = rand, A_1 = 50 + 1e-3 rand (B's right half at A_1's offset): rows of |a'| ~ 150 about the
    mean of both images, decided by 1e-3 of contrast.  Exact, and no scan value outside its bound."""
    z = PI.oracle('centring')
    out, Bp, st = _run_jobs(ctx, [z], setting)
    print('PAIRS centring %-10s fallbacks %5d reranked %5d' % (setting, st.fallbacks, st.reranked))
    check_debug_records(z, out[0], Bp[0], st, 'centring')
    _check_path(st, [z], 1, setting)


# ---- 6. batch ---------------------------------------------------------------------------------------------
def test_batch_on_one_pair_a_side(ctx):
    """two jobs with their own B side and kappa on one 2-pair A side in one call equal their separate
    calls (and the oracle)"""
    Z = [PI.oracle('p2_c1'), PI.oracle('p2_c1_job1')]
    assert Z[0]['k'] != Z[1]['k'] and not np.array_equal(Z[0]['B_pyr'][1], Z[1]['B_pyr'][1])
    out, Bp, st = _run_jobs(ctx, Z)
    for j, z in enumerate(Z):
        check_debug_records(z, out[j], Bp[j], st, 'batch job %d' % j)
        o1, B1, _ = _run_jobs(ctx, [z])
        for level in range(1, z['L']):
            assert np.array_equal(out[j][level][0], o1[0][level][0]) and np.array_equal(out[j][level][1], o1[0][level][1])
            assert np.array_equal(out[j][level][2]['dist'], o1[0][level][2]['dist'])
            assert np.array_equal(Bp[j][level], B1[0][level])
    _check_path(st, Z, 1, 'default')


# ---- 7 / 8. device pointers, argument errors --------------------------------------------------------------
def _device_level(z, level, Bp, n_img_a):
    """the tensors of one level on cuda:0; A / Ac stack n_img_a images"""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to('cuda:0')
    h, w = z['B_pyr'][level].shape[:2]
    T = dict(A=t(np.stack([p[level] for p in z['A_pairs'][:n_img_a]])), Ac=t(np.stack([p[level - 1] for p in z['A_pairs'][:n_img_a]])),
             Ap=t(np.stack([p[level] for p in z['Ap_pyr']])), Apc=t(np.stack([p[level - 1] for p in z['Ap_pyr']])),
             B=t(z['B_pyr'][level]), Bc=t(z['B_pyr'][level - 1]), Bpc=t(Bp[level - 1]), Bp=t(Bp[level]),
             weights=t(z['weights']), s_out=torch.zeros((h * w, 2), dtype=torch.int32, device='cuda:0'),
             im_out=torch.zeros(h * w, dtype=torch.int32, device='cuda:0'))
    torch.cuda.synchronize()
    return T


def test_device_pointers_equal_the_host_form(ctx):
    from ia_amd import _native
    z = PI.oracle('p2_c1')
    L = z['L']
    Bp = [x.copy() for x in z['Bp_init']]
    st = _native.Stats()
    for level in range(1, L):
        T = _device_level(z, level, Bp, 2)
        ctx.synthesize_level_device(1, 2, z['A_pyr'][level].shape[:2], z['B_pyr'][level].shape[:2],
                                    {k: v.data_ptr() for k, v in T.items()}, 1 + (2 ** (level - L)) * z['k'], st, n_a=2)
        torch.cuda.synchronize()
        Bp[level] = T['Bp'].cpu().numpy()
        assert np.array_equal(T['s_out'].cpu().numpy(), z['s'][level]) and np.array_equal(T['im_out'].cpu().numpy(), z['im'][level])
    out, Bp_h, _ = _run_jobs(ctx, [z], debug=False)
    for level in range(1, L):
        assert np.array_equal(Bp[level], Bp_h[0][level]) and np.array_equal(Bp[level], z['Bp_final'][level])
    assert st.bound_violations == 0 and st.f16_levels == L - 1


def test_n_a_that_is_not_n_ap_and_mixed_batches_are_refused(ctx):
    """IA_EINVAL from the argument checks, before anything is staged or launched.  Every buffer is
    as large as the largest reading of the arguments needs."""
    from ia_amd import _native
    z = PI.oracle('p3_c1')
    level = 1
    Bp = [x.copy() for x in z['Bp_init']]
    T = _device_level(z, level, Bp, 3)
    ptrs = {k: v.data_ptr() for k, v in T.items()}
    a_hw, b_hw = z['A_pyr'][level].shape[:2], z['B_pyr'][level].shape[:2]
    with pytest.raises(_native.IAError, match='IA_EINVAL'):
        ctx.synthesize_level_device(1, 3, a_hw, b_hw, ptrs, 1.25, n_a=2)          # n_a = 2 with n_ap = 3
    with pytest.raises(_native.IAError, match='IA_EINVAL'):
        ctx.synthesize_level_device(1, 3, a_hw, b_hw, ptrs, 1.25, n_a=-1)
    with pytest.raises(_native.IAError, match='IA_EINVAL'):                        # one batch, two n_a
        ctx.synthesize_levels_device(1, 3, a_hw, b_hw, [ptrs, ptrs], [1.25, 1.25], n_a=[3, 0])
    torch.cuda.synchronize()
    assert int(T['s_out'].abs().sum()) == 0 and int(T['im_out'].abs().sum()) == 0   # nothing ran
    assert np.array_equal(T['Bp'].cpu().numpy(), Bp[level])
    # host form: lists that do not pair up never reach the library
    A, Ac = _a_side(z, level)
    job = dict(B=z['B_pyr'][level], Bc=z['B_pyr'][level - 1], Bpc=Bp[level - 1], Bp=Bp[level], weights=z['weights'],
               kappa_factor=1.25)
    for bad_A, bad_Ac in ((A[:2], Ac[:2]), (A, Ac[0]), ([A[0], A[1], A[2][:-1]], Ac)):
        with pytest.raises(ValueError):
            ctx.synthesize_levels(bad_A, bad_Ac, [p[level] for p in z['Ap_pyr']], [p[level - 1] for p in z['Ap_pyr']], [job])
    assert np.array_equal(Bp[level], z['Bp_init'][level])


# ---- 9. drivers -------------------------------------------------------------------------------------------
def _cfg(**kw):
    from ia_amd import config
    c = types.SimpleNamespace(**{k: getattr(config, k) for k in dir(config) if not k.startswith('_')})
    c.convert, c.remap_lum, c.init_rand, c.AB_weight, c.k, c.seed = False, False, True, 1, 0.5, 3
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _driver_vs_oracle(tmp_path, A, Ap, B, c):
    from ia_amd.image_analogies import image_analogies_main, img_setup
    res = image_analogies_main(A, Ap, B, str(tmp_path) + '/out/', c)
    A_pyrs, Ap_pyrs, B_pyr, Bp0, _, c = img_setup(A, Ap, B, str(tmp_path) + '/o2/', c)
    S, IM, Bp = PI.oracle_pyramids(A_pyrs, Ap_pyrs, B_pyr, Bp0, c.k, c.weights)
    assert c.max_levels >= 3
    for level in range(1, c.max_levels):
        assert np.array_equal(res['s'][level], S[level]) and np.array_equal(res['im'][level], IM[level])
        assert np.array_equal(res['Bp_pyr'][level], Bp[level])
    assert res['stats']['bound_violations'] == 0
    return res


@pytest.mark.parametrize('yiq', [False, True], ids=['gray', 'yiq'])
def test_driver_with_a_pair_list_matches_oracle(tmp_path, yiq):
    """image_analogies_main on arrays, A_fname a list of two images: s, im and B' of every level equal
    the oracle run on the pyramids img_setup returned; metadata.txt names every A"""
    d = PI._driver_images(yiq)
    res = _driver_vs_oracle(tmp_path, d['A'], d['Ap'], d['B'], _cfg(convert=yiq))
    assert set(res['im'][max(res['im'])]) == {0, 1}
    meta = (tmp_path / 'out' / 'metadata.txt').read_text()
    assert "A_fname: ['<array>', '<array>']" in meta


def test_augment_pairs_end_to_end_picks_from_both_images(tmp_path):
    import ia_amd
    d = PI._driver_images(False)
    A, Ap = ia_amd.augment_pairs(d['A'][0], d['Ap'][0], ('lr',))
    res = _driver_vs_oracle(tmp_path, A, Ap, d['B'], _cfg())
    finest = max(res['im'])
    share = [int((res['im'][finest] == i).sum()) for i in (0, 1)]
    print('augment_pairs lr: finest level picks per image', share)
    assert min(share) * 8 >= sum(share)


def test_per_pixel_loop_on_pairs_reproduces_the_fast_path(ctx):
    """the reference's per-pixel level loop (tests/test_gpu_flann_api.py _reference_loop) on
    create_index's DB of pairs, GpuFLANN and best_coherence_match: the fast path's level"""
    from ia_amd import algorithms
    from test_gpu_flann_api import _cfg as loop_cfg, _reference_loop
    z = PI.oracle('gate_c1_in')
    c = loop_cfg(1, z['L'])
    c.weights, c.k = z['weights'], z['k']
    flann, params, As, As_size = algorithms.create_index(z['A_pairs'], z['Ap_pyr'], c)
    assert np.array_equal(np.asarray(As[1]), PI.build_db(z, 1)) and As_size[1] == (2 * 9 * 7, 55)
    out = {}
    Bp, app_ix, coh = _reference_loop(z, c, flann, params, As, out)
    fast, Bp_f, st = _run_jobs(ctx, [z])
    assert np.array_equal(np.array(app_ix), z['app_ix']) and np.array_equal(np.array(coh), z['coh'])
    for level in range(1, z['L']):
        assert np.array_equal(out[level][0], fast[0][level][0]) and np.array_equal(out[level][1], fast[0][level][1])
        assert np.array_equal(Bp[level], Bp_f[0][level]) and np.array_equal(Bp[level], z['Bp_final'][level])


def test_sweep_on_pairs_host_and_device(ctx):
    """sweep.Sweep with a list of A images: two jobs (their own kappa and B' seed) batched on one
    2-pair A side equal the oracle on the sweep's pyramids; DeviceSweep (A stacked on the device,
    n_a = 2) equals the host run"""
    from ia_amd import _native, sweep
    d = PI._driver_images(False)
    sw = sweep.Sweep(d['A'], d['Ap'], d['B'], [sweep.SweepJob(0.5, seed=3), sweep.SweepJob(5.0, seed=4)])
    assert sw.pairs and sw.Lf == 4
    res = sw.run(ctx)
    for j in (0, 1):
        S, IM, Bp = PI.oracle_pyramids(sw.A_pyr, sw.Ap_pyr_list, sw.B_pyr, sw.Bp_init[j], sw.jobs[j].k, sw.weights)
        for level in range(1, sw.Lf):
            assert np.array_equal(res[j][1][level], S[level]) and np.array_equal(res[j][2][level], IM[level])
            assert np.array_equal(res[j][0][level], Bp[level])
        assert set(res[j][2][sw.Lf - 1]) == {0, 1}
    ds = sweep.DeviceSweep(sw, [0, 1], torch, torch.device('cuda', 0))
    st = _native.Stats()
    ds.run(ctx, st)
    torch.cuda.synchronize()
    for j in (0, 1):
        for level in range(1, sw.Lf):
            assert np.array_equal(ds.S[j][level].cpu().numpy(), res[j][1][level])
            assert np.array_equal(ds.IM[j][level].cpu().numpy(), res[j][2][level])
            assert np.array_equal(ds.Bp[j][level].cpu().numpy(), res[j][0][level])
    assert st.bound_violations == 0

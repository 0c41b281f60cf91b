"""Training pairs (A_i, A'_i), the parts that need no GPU.

* The conditions tests/test_gpu_pairs.py relies on, pinned on the oracle's own runs of its inputs
  (tests/pairs_inputs.py): every image of every case is picked, the result differs from the run
  that shares A_0 (so a build that ignores A_1.. cannot pass), no NN decision is an exact tie and
  no kappa comparison is within a relative 1e-6 of its threshold (the bar of
  tests/test_adversarial_inputs_cpu.py test_kappa_decisions_are_robust).
* The host side of the feature: augment_pairs, the pair-list checks, img_setup on a list of A
  images (per-pair pyramids, per-pair luminance remap), the ctypes layout, Job / Sweep.
"""
import ctypes
import types

import numpy as np
import pytest

import ia_amd
import pairs_inputs as PI
from ia_amd import _native, algorithms, config, img_preprocess, synth, sweep
from ia_amd.image_analogies import img_setup
from oracle import ia_oracle as O


# ---- conditions on the inputs -----------------------------------------------------------------------
@pytest.mark.parametrize('name', PI.PAIR_CASES)
def test_every_image_is_picked_and_a1_matters(name):
    r, sh = PI.oracle(name), PI.oracle(name, shared=True)
    n = len(r['Ap_pyr'])
    npx = sum(len(r['im'][l]) for l in r['im'])
    share = [sum(int((r['im'][l] == i).sum()) for l in r['im']) for i in range(n)]
    diff = sum(int((r['s'][l] != sh['s'][l]).any(axis=1).sum()) + int((r['im'][l] != sh['im'][l]).sum()) for l in r['im'])
    print('%s: shares %s of %d, %d of %d s / im entries differ from the shared-A_0 run' % (name, share, npx, diff, 2 * npx))
    assert min(share) * 8 >= npx
    assert diff > npx // 2
    assert all(not np.array_equal(r['Bp_final'][l], sh['Bp_final'][l]) for l in r['im'])


@pytest.mark.parametrize('name', PI.PAIR_CASES)
def test_decisions_are_robust(name):
    r = PI.oracle(name)
    assert len(r['nn']) == sum(len(r['im'][l]) for l in r['im'])
    assert all(exact == 1 for _, exact, _ in r['nn'])          # no exact NN tie
    assert len(r['kappa']) > 0
    margin = min(abs(dc - da * kf) / (da * kf) for da, dc, kf in r['kappa'])
    print('%s: smallest relative kappa margin %.3g' % (name, margin))
    assert margin > 1e-6


def test_oracle_runner_equals_the_oracle_on_a_shared_a():
    """the written-out level loop is adversarial_inputs.run_oracle's on a case without pairs"""
    import adversarial_inputs as AI
    z = PI.shared_a0(PI.make('p2_c1'))
    a, b = PI.run_oracle(z), AI.run_oracle(z)
    for key in ('app_ix', 'coh', 'dist'):
        assert np.array_equal(a[key], b[key])
    for l in a['s']:
        assert np.array_equal(a['s'][l], b['s'][l]) and np.array_equal(a['Bp_final'][l], b['Bp_final'][l])


def test_pair_db_rows():
    """image i's rows are [A_i 3x3 | A_i 5x5 | A'_i 3x3 | A'_i first 12]"""
    z = PI.make('p3_c2')
    As = PI.build_db(z, 2)
    hw = 25 * 19
    assert As.shape == (3 * hw, 110)
    for i in range(3):
        one = O.build_db(z['A_pairs'][i], [z['Ap_pyr'][i]], 2)
        assert np.array_equal(As[i * hw:(i + 1) * hw], one)


# ---- augment_pairs ------------------------------------------------------------------------------------
def test_augment_pairs_shapes_order_and_transforms():
    rs = np.random.RandomState(0)
    A, Ap = rs.rand(6, 9, 3), rs.rand(6, 9, 3)
    As, Aps = ia_amd.augment_pairs(A, Ap)
    assert len(As) == len(Aps) == 4
    assert As[0] is not None and np.array_equal(As[0], A) and np.array_equal(Aps[0], Ap)   # the original pair first
    assert np.array_equal(As[1], A[:, ::-1]) and np.array_equal(Aps[1], Ap[:, ::-1])
    assert np.array_equal(As[2], A[::-1]) and np.array_equal(Aps[2], Ap[::-1])
    assert np.array_equal(As[3], A[::-1, ::-1]) and np.array_equal(Aps[3], Ap[::-1, ::-1])
    assert all(x.shape == A.shape and x.flags.c_contiguous for x in As + Aps)
    As, Aps = ia_amd.augment_pairs(A, Ap, ('ud',))
    assert len(As) == 2 and np.array_equal(Aps[1], Ap[::-1])
    assert ia_amd.augment_pairs(A, Ap, ())[0][0].shape == A.shape


def test_augment_pairs_transposing_transforms_need_square_images():
    rs = np.random.RandomState(1)
    A, Ap = rs.rand(5, 7), rs.rand(5, 7)
    for t in ('rot90', 'rot270', 'transpose', 'transverse'):
        with pytest.raises(ValueError):
            ia_amd.augment_pairs(A, Ap, (t,))
    S, Sp = rs.rand(5, 5, 2), rs.rand(5, 5, 2)
    As, Aps = ia_amd.augment_pairs(S, Sp, ('rot90', 'rot270', 'transpose', 'transverse'))
    assert np.array_equal(As[1], np.rot90(S)) and np.array_equal(Aps[1], np.rot90(Sp))
    assert np.array_equal(As[2], np.rot90(S, 3)) and np.array_equal(Aps[2], np.rot90(Sp, 3))
    assert np.array_equal(As[3], S.transpose(1, 0, 2)) and np.array_equal(Aps[3], Sp.transpose(1, 0, 2))
    assert np.array_equal(As[4], np.rot90(S, 2).transpose(1, 0, 2))
    # the eight images are the eight symmetries: all different, all of the original's shape
    eight = ia_amd.augment_pairs(S, Sp, ('lr', 'ud', 'rot180', 'rot90', 'rot270', 'transpose', 'transverse'))[0]
    assert all(x.shape == S.shape for x in eight)
    assert all(not np.array_equal(eight[i], eight[j]) for i in range(8) for j in range(i))
    with pytest.raises(ValueError):
        ia_amd.augment_pairs(S, Sp, ('flip',))
    with pytest.raises(ValueError):
        ia_amd.augment_pairs(S, rs.rand(5, 6, 2))


# ---- pair lists that do not pair up ---------------------------------------------------------------------
def test_pair_list_of_wrong_length_or_unequal_shapes_raises(tmp_path):
    rs = np.random.RandomState(2)
    A, Ac = [rs.rand(8, 6), rs.rand(8, 6)], [rs.rand(4, 3), rs.rand(4, 3)]
    a, ac = _native.stack_pairs(A, Ac, 2)
    assert a.shape == (2, 8, 6) and ac.shape == (2, 4, 3) and a.flags.c_contiguous
    with pytest.raises(ValueError):
        _native.stack_pairs(A, Ac, 3)
    with pytest.raises(ValueError):
        _native.stack_pairs(A[:1], Ac, 2)
    with pytest.raises(ValueError):
        _native.stack_pairs([A[0], rs.rand(8, 7)], Ac, 2)
    with pytest.raises(ValueError):
        _native.stack_pairs(A, [Ac[0], rs.rand(3, 3)], 2)
    with pytest.raises(ValueError):
        _native.stack_pairs(A, Ac[0], 2)      # a list for A, one array for Ac
    assert issubclass(_native.IAShapeError, _native.IAError)

    c = _cfg()
    imgs = [rs.rand(12, 12) for _ in range(5)]
    with pytest.raises(ValueError):
        img_setup(imgs[:2], imgs[2:5], imgs[0], str(tmp_path) + '/a/', c)            # 2 A for 3 A'
    with pytest.raises(ValueError):
        img_setup([imgs[0], rs.rand(12, 10)], imgs[2:4], imgs[0], str(tmp_path) + '/b/', c)
    z = PI.make('p3_c1')
    cc = types.SimpleNamespace(n_sm=3, n_lg=5, n_half=12, max_levels=3)
    with pytest.raises(ValueError):
        algorithms.create_index(z['A_pairs'][:2], z['Ap_pyr'], cc)
    with pytest.raises(ValueError):
        synth.Job(z['A_pairs'][:2], z['Ap_pyr'], z['B_pyr'], z['Bp_init'], 0.5, z['weights'])
    with pytest.raises(ValueError):
        sweep.Sweep(imgs[:2], imgs[2:5], imgs[0], [sweep.SweepJob()])


# ---- img_setup ------------------------------------------------------------------------------------------
def _cfg(**kw):
    c = types.SimpleNamespace(**{k: getattr(config, k) for k in dir(config) if not k.startswith('_')})
    c.convert, c.remap_lum, c.init_rand, c.AB_weight, c.k, c.seed, c.gpu_preprocess = False, False, True, 1, 0.5, 3, False
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize('ch3', [False, True])
def test_img_setup_returns_per_pair_pyramids(tmp_path, ch3):
    """a list for A_fname: one pyramid per A_i, each what img_setup makes of (A_i, [A'_i]) alone;
    YIQ (ch3) keeps the luminance of each A_i"""
    d = PI._driver_images(ch3)
    c = _cfg(convert=ch3, AB_weight=0.5)
    A_pyrs, Ap_pyrs, B_pyr, Bp, _, c = img_setup(d['A'], d['Ap'], d['B'], str(tmp_path) + '/p/', c)
    assert algorithms.is_pyramid_list(A_pyrs) and len(A_pyrs) == len(Ap_pyrs) == 2
    assert A_pyrs[0][-1].shape == PI.DRIVER_HW
    for i in range(2):
        one = img_setup(d['A'][i], [d['Ap'][i]], d['B'], str(tmp_path) + '/s%d/' % i, _cfg(convert=ch3, AB_weight=0.5))
        assert not algorithms.is_pyramid_list(one[0])
        assert all(np.array_equal(x, y) for x, y in zip(A_pyrs[i], one[0]))
        assert all(np.array_equal(x, y) for x, y in zip(Ap_pyrs[i], one[1][0]))
        assert all(np.array_equal(x, y) for x, y in zip(B_pyr, one[2]))
    assert not np.array_equal(A_pyrs[0][-1], A_pyrs[1][-1])
    # a tuple is a list of pairs too; one array stays the shared A (first return value: one pyramid)
    assert algorithms.is_pyramid_list(img_setup(tuple(d['A']), d['Ap'], d['B'], str(tmp_path) + '/t/', _cfg(convert=ch3))[0])


def test_img_setup_remaps_luminance_per_pair(tmp_path):
    """remap_lum: (A_i, A'_i) go to B's mean and deviation with A_i's OWN statistics"""
    rs = np.random.RandomState(5)
    A = [rs.rand(16, 16), 0.3 + 0.2 * rs.rand(16, 16)]
    Ap = [rs.rand(16, 16), rs.rand(16, 16)]
    B = 0.5 * rs.rand(16, 16)
    A_pyrs, Ap_pyrs = img_setup(A, Ap, B, str(tmp_path) + '/r/', _cfg(remap_lum=True))[:2]
    for i in range(2):
        a, ap = img_preprocess.remap_luminance(A[i], [Ap[i]], B)
        assert np.array_equal(A_pyrs[i][-1], a) and np.array_equal(Ap_pyrs[i][-1], ap[0])
        assert abs(A_pyrs[i][-1].mean() - B.mean()) < 1e-12 and abs(A_pyrs[i][-1].std() - B.std()) < 1e-12
    # the shared-A remap would have used A_0's statistics for A'_1
    shared = img_preprocess.remap_luminance(A[0], Ap, B)[1][1]
    assert not np.array_equal(Ap_pyrs[1][-1], shared)


@pytest.mark.parametrize('kind', ['gray', 'yiq', 'augment_lr'])
def test_driver_inputs_pick_both_images(tmp_path, kind):
    """the inputs of tests/test_gpu_pairs.py's driver tests, through img_setup on the host: the oracle
    takes at least 1/8 of the finest level from each image, without an exact tie or a close kappa call"""
    d = PI._driver_images(kind == 'yiq')
    A, Ap = ia_amd.augment_pairs(d['A'][0], d['Ap'][0], ('lr',)) if kind == 'augment_lr' else (d['A'], d['Ap'])
    A_pyrs, Ap_pyrs, B_pyr, Bp0, _, c = img_setup(A, Ap, d['B'], str(tmp_path) + '/d/', _cfg(convert=kind == 'yiq'))
    assert c.max_levels == 4
    r = PI.run_oracle(dict(A_pyr=A_pyrs[0], A_pairs=A_pyrs, Ap_pyr=Ap_pyrs, B_pyr=B_pyr, Bp_init=Bp0, L=4, k=c.k,
                           weights=c.weights), nn_stats=True)
    share = [int((r['im'][3] == i).sum()) for i in (0, 1)]
    assert min(share) * 8 >= sum(share) == 24 * 24
    assert all(exact == 1 for _, exact, _ in r['nn'])
    assert min(abs(dc - da * kf) / (da * kf) for da, dc, kf in r['kappa']) > 1e-6


# ---- layout and pass-through ----------------------------------------------------------------------------
def test_level_args_ends_with_n_a():
    assert _native.LevelArgs._fields_[-1] == ('n_a', ctypes.c_int)
    assert _native.LevelArgs._fields_[-2][0] == 'dbg_dist'
    a = _native.LevelArgs(1, 2, 3, 4, 5, 6)     # a positional construction that stops early: shared A
    assert a.n_a == 0 and a.dbg_dist is None
    assert _native.LevelArgs.n_a.offset == _native.LevelArgs.dbg_dist.offset + 8


def test_pyramid_list_rule_and_pass_through():
    z = PI.make('p2_c1')
    assert algorithms.is_pyramid_list(z['A_pairs']) and not algorithms.is_pyramid_list(z['A_pyr'])
    assert algorithms.is_pyramid_list(tuple(tuple(p) for p in z['A_pairs']))
    lv = algorithms.a_levels(z['A_pairs'], 2)
    assert isinstance(lv, list) and len(lv) == 2 and lv[1] is z['A_pairs'][1][2]
    assert algorithms.a_levels(z['A_pyr'], 2) is z['A_pyr'][2]
    job = synth.Job(z['A_pairs'], z['Ap_pyr'], z['B_pyr'], z['Bp_init'], 0.5, z['weights'])
    assert job.pairs and job.L == 3 and job.A_levels(1)[1] is z['A_pairs'][1][1]
    one = synth.Job(z['A_pyr'], z['Ap_pyr'], z['B_pyr'], z['Bp_init'], 0.5, z['weights'])
    assert not one.pairs and one.L == 3 and one.A_levels(1) is z['A_pyr'][1] and one.flops() == job.flops()
    rs = np.random.RandomState(7)
    imgs = [rs.rand(20, 20) for _ in range(5)]
    sw = sweep.Sweep(imgs[:2], imgs[2:4], imgs[4], [sweep.SweepJob()])
    assert sw.pairs and algorithms.is_pyramid_list(sw.A_pyr) and len(sw.A_pyr) == 2
    assert all(len(p) == sw.Lf for p in sw.A_pyr) and sw.A_pyr[1][-1].shape == (20, 20)
    assert np.array_equal(sw.A_pyr[1][-1], imgs[1])
    sw1 = sweep.Sweep(imgs[0], imgs[2:4], imgs[4], [sweep.SweepJob()])
    assert not sw1.pairs and all(np.array_equal(x, y) for x, y in zip(sw1.A_pyr, sw.A_pyr[0]))

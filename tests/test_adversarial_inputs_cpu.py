"""Each case of tests/adversarial_inputs.py is what it claims to be, and the reference's own
decisions on it are robust - checked with the oracle alone (fp64, brute force; compute_distance in
the explicit BLAS dot order), so a GPU mismatch in tests/test_gpu_adversarial.py can never be
excused as a near-tie of the reference.

These are conditions on the inputs, not measurements: a generator that misses one is changed (or
reseeded), never the condition.
"""
import numpy as np
import pytest

import adversarial_inputs as AI

ALL = AI.BASE_CASES + ['k0'] + AI.BIG_CASES + AI.GATE_CASES


def _rel_kappa(r, with_kf):
    return np.array([abs(dc - (kf if with_kf else 1.0) * da) / ((kf if with_kf else 1.0) * da)
                     for da, dc, kf in r['kappa']])


@pytest.mark.parametrize('name', ALL)
def test_shapes_follow_the_level_contract(name):
    z = AI.make(name)
    geo = AI.GATE if name in AI.GATE_CASES else AI.BIG if name in AI.BIG_CASES else AI.BASE
    assert z['L'] == geo['L'] == len(z['A_pyr']) == len(z['B_pyr']) == len(z['Bp_init']) == len(z['Ap_pyr'][0])
    assert z['A_pyr'][-1].shape == z['Ap_pyr'][0][-1].shape == geo['a_hw']
    assert z['B_pyr'][-1].shape == z['Bp_init'][-1].shape == geo['b_hw']
    for pyr in (z['A_pyr'], z['Ap_pyr'][0], z['B_pyr'], z['Bp_init']):
        assert all(x.dtype == np.float64 for x in pyr)
        for l in range(1, z['L']):
            h, w = pyr[l].shape
            assert pyr[l - 1].shape == (-(-h // 2), -(-w // 2))
    again = AI.make(name)   # deterministic
    assert all(np.array_equal(a, b) for k in ('A_pyr', 'B_pyr', 'Bp_init') for a, b in zip(z[k], again[k]))
    assert z['k'] == (0.0 if name == 'k0' else 0.5)


def test_db_sizes():
    """base: 475 rows = 15 tiles, the last partial; bigA: 8,280 rows = 259 tiles (> 256 workgroups),
    the last with 24 rows; 400 / 192 synthesised pixels"""
    z = AI.make('x60')
    assert z['A_pyr'][-1].size == 475 and -(-475 // 32) == 15 and 475 % 32 != 0
    assert sum(x.size for x in z['B_pyr'][1:]) == 400
    z = AI.make('bigA')
    assert z['A_pyr'][-1].size == 8280 and -(-8280 // 32) == 259 and 8280 % 32 == 24
    assert sum(x.size for x in z['B_pyr'][1:]) == 192


@pytest.mark.parametrize('name,lo,hi', [('x60', 0, 60), ('x64edge', 0, 64), ('signed', -60, 60), ('tiny', 0, 2.0 ** -14),
                                        ('offset', -50, 50.001), ('constA', 0, 1)])
def test_value_ranges(name, lo, hi):
    """x64edge: every value < 64, so the split-f16 matcher must be used; x60 / x64edge / signed reach
    the top of that range, tiny stays under 2^-14"""
    arrs = [a for v in AI.all_arrays(AI.make(name)).values() for a in v]
    mn, mx = min(a.min() for a in arrs), max(a.max() for a in arrs)
    print(name, mn, mx)
    assert lo <= mn and mx <= hi
    assert max(abs(mn), abs(mx)) <= 64
    if name in ('x60', 'x64edge', 'signed'):
        assert max(abs(mn), abs(mx)) > 0.99 * max(abs(lo), abs(hi))
    if name == 'offset':
        a = AI.make(name)
        assert all(x.min() >= 50 for x in a['A_pyr'] + a['Ap_pyr'][0]) and all(x.max() <= -49.999 for x in a['B_pyr'] + a['Bp_init'])
    if name == 'constA':
        a = AI.make(name)
        assert all((x == 0.25).all() for x in a['A_pyr'] + a['Ap_pyr'][0])


@pytest.mark.parametrize('i', range(8))
def test_gate_has_one_value_out_of_range_in_array_i(i):
    arrs = AI.all_arrays(AI.make('gate%d' % i))
    over = {k: int(sum((np.abs(a) > 64).sum() for a in v)) for k, v in arrs.items()}
    assert over == {k: int(k == AI.GATE_ARRAYS[i]) for k in AI.GATE_ARRAYS}
    if AI.GATE_ARRAYS[i] == 'Bp':   # read by the raster loop before it is overwritten: not pixel (0, 0)
        assert abs(arrs['Bp'][0][0, 0]) <= 64


@pytest.mark.parametrize('name', ['neartie26', 'neartie36', 'bigA_neartie'])
def test_near_ties_are_decided_by_fp64_and_not_by_index(name):
    """>= 100 pixels whose runner-up is within a relative 2^-20 of the NN while the NN is not the
    lowest index among the rows within that gap; no exact tie anywhere"""
    nn = AI.oracle(name)['nn']
    n = sum(1 for gap, exact, lowest in nn if gap < AI.REL_TIE and not lowest)
    ties = sum(1 for gap, exact, lowest in nn if exact > 1)
    print('%s: %d of %d pixels near-tied with the winner not the lowest index; %d exact ties' % (name, n, len(nn), ties))
    assert n >= 100 and ties == 0


def test_offset_every_nn_gap_is_tiny():
    nn = AI.oracle('offset')['nn']
    assert len(nn) == 400 and all(gap < AI.REL_TIE for gap, _, _ in nn)
    assert all(exact == 1 for _, exact, _ in nn)


def test_const_a_every_pixel_ties_over_all_rows():
    r = AI.oracle('constA')
    assert len(r['nn']) == 400
    rows = {1: r['A_pyr'][1].size, 2: r['A_pyr'][2].size}
    at = 0
    for level in (1, 2):
        n = r['B_pyr'][level].size
        assert all(exact == rows[level] for _, exact, _ in r['nn'][at:at + n])
        at += n
    assert (r['app_ix'] == 0).all()   # the winner is row 0 of image 0


def test_k0_kappa_comparisons_are_equalities_or_far_apart():
    """kappa = 0: kappa_factor is exactly 1 and d_coh <= d_app holds with equality whenever the
    coherence candidate is the NN row; no comparison is decided by the last bits otherwise"""
    r = AI.oracle('k0')
    assert all(kf == 1.0 for _, _, kf in r['kappa'])
    rel = _rel_kappa(r, False)
    eq = int((rel == 0).sum())
    print('k0: %d of %d kappa comparisons with d_coh == d_app' % (eq, len(rel)))
    assert eq >= 100 and eq == sum(1 for da, dc, _ in r['kappa'] if da == dc)
    assert not ((rel > 0) & (rel < 1e-9)).any()


@pytest.mark.parametrize('name', [c for c in ALL if c != 'k0'])
def test_kappa_decisions_are_robust(name):
    r = AI.oracle(name)
    rel = _rel_kappa(r, True)
    print('%s: smallest |d_coh - kf d_app| / (kf d_app) = %.3g over %d comparisons' % (name, rel.min(), len(rel)))
    assert len(rel) > 0 and rel.min() > 1e-6

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


# ---- the generators stay what they were at 1 channel ----------------------------------------------
# sha1 (first 16 hex digits) over the eight kinds of arrays (all_arrays, sorted by kind; bytes and
# shape of each), the weights and k, taken before the generators learned ch and n_ap
PINNED_1CH = {
    'x60': '6bbf949823500fa3', 'x64edge': 'c648e5e9559d19cb', 'signed': 'f15ed283b5919afb', 'tiny': '33849a8ec34a44f1',
    'offset': 'a6b23a4307116907', 'constA': 'f55bc413738af46d', 'neartie26': 'aec0b827cc9783c8',
    'neartie36': 'dba0b7be46201bb9', 'k0': '4e162de4a2f592e4', 'bigA': '31f481798df2b0ba',
    'bigA_neartie': '84a1a62f483cf22c', 'gate0': '2254363a695aac47', 'gate1': '929474eabb3b4d0b',
    'gate2': '094cf6967b3521b5', 'gate3': '7d82543d2874c61f', 'gate4': '094e9f1f4d0552d9', 'gate5': 'febe96c5a2e4df96',
    'gate6': 'de58d0ce8896bad1', 'gate7': '2a37fe94e2a3e20b',
}


def test_one_channel_cases_are_unchanged():
    """same seeds, same order of rs.rand calls: every 1-channel case is the arrays it was"""
    import hashlib
    assert sorted(PINNED_1CH) == sorted(ALL)
    for name in ALL:
        z = AI.make(name)
        h = hashlib.sha1()
        for _, v in sorted(AI.all_arrays(z).items()):
            for a in v:
                h.update(np.ascontiguousarray(a).tobytes())
                h.update(str(a.shape).encode())
        h.update(z['weights'].tobytes())
        h.update(repr(z['k']).encode())
        assert h.hexdigest()[:16] == PINNED_1CH[name], name


# ---- 2 and 3 channels (tests/test_gpu_channels.py) ------------------------------------------------
def _geo(name):
    return (AI.GATE if name.startswith('gate') else AI.BIG if name.startswith('bigA') else
            AI.WIDE if name.startswith('wide') else AI.BASE)


@pytest.mark.parametrize('name', AI.CH_CASES)
def test_channel_case_shapes(name):
    z = AI.make(name)
    ch, geo = AI.case_ch(name), _geo(name)
    n_ap = 2 if name.startswith('multiap') else 1
    assert ch in (2, 3) and len(z['Ap_pyr']) == n_ap and z['weights'].shape == (55 * ch,)
    assert z['L'] == geo['L'] == len(z['A_pyr']) == len(z['B_pyr']) == len(z['Bp_init'])
    assert z['A_pyr'][-1].shape == geo['a_hw'] + (ch,) and z['B_pyr'][-1].shape == z['Bp_init'][-1].shape == geo['b_hw'] + (ch,)
    for pyr in [z['A_pyr'], z['B_pyr'], z['Bp_init']] + z['Ap_pyr']:
        assert len(pyr) == z['L'] and all(x.dtype == np.float64 for x in pyr)
        for l in range(1, z['L']):
            h, w, c = pyr[l].shape
            assert pyr[l - 1].shape == (-(-h // 2), -(-w // 2), c)
    assert all(p[-1].shape == z['A_pyr'][-1].shape for p in z['Ap_pyr'])
    again = AI.make(name)   # deterministic
    assert all(np.array_equal(a, b) for k in ('A_pyr', 'B_pyr', 'Bp_init') for a, b in zip(z[k], again[k]))
    assert all(np.array_equal(a, b) for p, q in zip(z['Ap_pyr'], again['Ap_pyr']) for a, b in zip(p, q))
    assert z['k'] == (AI.WIDE_K[int(name[6])] if name.startswith('wide') else 0.5)
    # channels are not copies of each other (a kernel that reads channel 0 for every channel fails)
    assert all((x[..., 0] != x[..., c]).any() for x in (z['A_pyr'][-1], z['B_pyr'][-1]) for c in range(1, ch)
               if not name.startswith('constA') or x is not z['A_pyr'][-1])


def test_channel_db_sizes():
    """multiap: 950 rows in 30 tiles, the last partial; bigA: 259 tiles, 33 per workgroup on 8
    workgroups and >= 64 per shard of 2; wide: 243 pixels per job in steps of up to 9 queries"""
    z = AI.make('multiap_c2')
    rows = len(z['Ap_pyr']) * z['A_pyr'][-1].shape[0] * z['A_pyr'][-1].shape[1]
    assert rows == 950 and -(-rows // 32) == 30 and rows % 32 != 0
    z = AI.make('bigA_c3')
    assert -(-z['A_pyr'][-1].shape[0] * z['A_pyr'][-1].shape[1] // 32) == 259 >= 2 * 64 and -(-259 // 8) == 33
    h, w = AI.WIDE['b_hw']
    assert min(h, w // 3) == 9 and h * w == 243 and AI.WIDE['L'] == 2
    assert 0.0 not in AI.WIDE_K and len(set(AI.WIDE_K)) == 4


RANGES = {'x60': (0, 60), 'x64edge': (0, 64), 'signed': (-60, 60), 'tiny': (0, 2.0 ** -14), 'offset': (-50, 50.001),
          'constA': (0, 1)}


@pytest.mark.parametrize('case', [c for c in AI.BASE_CH_CASES if c[:-3] in RANGES])
def test_channel_value_ranges(case):
    name, (lo, hi) = case[:-3], RANGES[case[:-3]]
    arrs = [a for v in AI.all_arrays(AI.make(case)).values() for a in v]
    mn, mx = min(a.min() for a in arrs), max(a.max() for a in arrs)
    assert lo <= mn and mx <= hi and max(abs(mn), abs(mx)) <= 64
    if name in ('x60', 'x64edge', 'signed'):
        assert max(abs(mn), abs(mx)) > 0.99 * max(abs(lo), abs(hi))


@pytest.mark.parametrize('name', AI.GATE_LAST_CASES + AI.GATE_JOB1_CASES + [AI.GATE_JOB0])
def test_gate_last_element_is_the_one_value_out_of_range(name):
    arrs = AI.all_arrays(AI.make(name))
    over = {k: int(sum((np.abs(a) > 64).sum() for a in v)) for k, v in arrs.items()}
    if name == AI.GATE_JOB0:
        assert not any(over.values())
        return
    kind = AI.GATE_ARRAYS[int(name[5])] if name.startswith('gateL') else name[len('gate_job1_'):-3]
    assert over == {k: int(k == kind) for k in AI.GATE_ARRAYS}
    (a,) = arrs[kind]
    assert a.ndim == 3 and a.shape[2] == 2 and a[-1, -1, -1] == 64.5 and np.abs(a).argmax() == a.size - 1


def test_gate_job1_shares_the_a_side_of_job0():
    z0 = AI.make(AI.GATE_JOB0)
    for name in AI.GATE_JOB1_CASES:
        z1 = AI.make(name)
        assert all(np.array_equal(a, b) for a, b in zip(z0['A_pyr'] + z0['Ap_pyr'][0], z1['A_pyr'] + z1['Ap_pyr'][0]))
        assert not np.array_equal(z0['B_pyr'][-1], z1['B_pyr'][-1])


# (exact ties, winner not the lowest index within a relative 2^-20, runner-up within 2^-20) of the
# oracle's NN decisions, out of 400 pixels; measured with the committed oracle and pinned
NEAR_TIE_PINS = {'offset_c2': (0, 400, 400), 'offset_c3': (0, 400, 400), 'neartie26_c2': (0, 129, 249),
                 'neartie36_c2': (0, 270, 377), 'neartie36_c3': (0, 287, 375)}


def _tie_figures(nn):
    return (sum(1 for gap, exact, lowest in nn if exact > 1), sum(1 for gap, exact, lowest in nn if gap < AI.REL_TIE and not lowest),
            sum(1 for gap, exact, lowest in nn if gap < AI.REL_TIE))


@pytest.mark.parametrize('name', [c for c in AI.CH_CASES if not c.startswith('constA')])
def test_channel_cases_have_no_exact_nn_tie(name):
    """and the cases that are not built from near-ties have none: a GPU mismatch is never a tie"""
    fig = _tie_figures(AI.oracle(name)['nn'])
    print(name, fig)
    if name in NEAR_TIE_PINS:
        assert fig == NEAR_TIE_PINS[name] and fig[1] >= 100   # at least a quarter of the pixels
    else:
        assert fig == (0, 0, 0)


@pytest.mark.parametrize('name', AI.NO_FALLBACK_C2)
def test_third_row_is_beyond_the_split_f16_window(name):
    """d3 - d1 > 4 eps at every pixel, eps the KS = 7 bound at 1.1 x the case's norms: the condition
    under which tests/test_gpu_channels.py asserts fallbacks == 0 (AI.certify_margin)"""
    m = AI.certify_margin(AI.oracle(name), 7)
    print('%s: min (d3 - d1) / (4 eps) = %.3g' % (name, m))
    assert m > 1.5


def test_tiny_cannot_certify_at_two_channels():
    """every distance is far below the absolute term of the bound: no pixel's third row is outside
    the window (and none of its other rows), so every chunk of every pixel is rescanned"""
    r = AI.oracle('tiny_c2')
    assert max(g3 / (4 * AI.split_f16_eps(7, R / 1.1, qn / 1.1)) for g3, R, qn in r['third']) < 1e-3
    assert 110 * 2.0 ** -28 < 0.1 * AI.split_f16_eps(7, 0.0, 0.0)   # the largest distance against the bound's floor


def test_neartie26_three_channels_figures():
    """the one near-tie input no GPU run uses: 214 of 400 winners not the lowest index"""
    r = AI.run_oracle(AI._GEN['neartie26'](ch=3), nn_stats=True)
    assert _tie_figures(r['nn']) == (0, 214, 281)


@pytest.mark.parametrize('ch', [2, 3])
def test_channel_const_a_every_pixel_ties_over_all_rows(ch):
    r = AI.oracle('constA_c%d' % ch)
    rows = [r['A_pyr'][l].shape[0] * r['A_pyr'][l].shape[1] for l in (1, 2) for _ in range(r['B_pyr'][l][..., 0].size)]
    assert [exact for _, exact, _ in r['nn']] == rows and (r['app_ix'] == 0).all()


@pytest.mark.parametrize('name', AI.CH_CASES)
def test_channel_kappa_decisions_are_robust(name):
    """no kappa comparison at or near equality (the wide variants avoid k = 0 for this)"""
    r = AI.oracle(name)
    rel = _rel_kappa(r, True)
    print('%s: smallest |d_coh - kf d_app| / (kf d_app) = %.3g over %d comparisons' % (name, rel.min(), len(rel)))
    assert len(rel) > 0 and rel.min() > 1e-6


@pytest.mark.parametrize('ch', [2, 3])
def test_multiap_uses_both_images(ch):
    r = AI.oracle('multiap_c%d' % ch)
    im = r['im'][r['L'] - 1]
    n1 = int((im == 1).sum())
    print('multiap ch %d: %d of %d finest-level pixels from image 1' % (ch, n1, im.size))
    assert set(im.tolist()) == {0, 1} and min(n1, im.size - n1) >= im.size // 8
    h, w = r['A_pyr'][-1].shape[:2]
    assert (r['app_ix'] >= h * w).any() and (r['app_ix'] < h * w).any()


@pytest.mark.parametrize('ch', [2, 3])
def test_wide_variants_differ(ch):
    """one A side, four B sides and kappas: no two variants share s at the finest level, nor a
    kappa factor, so a job that reads its neighbour's queries, B' or kappa cannot pass"""
    R = [AI.oracle(n) for n in AI.WIDE_CASES[ch]]
    for i in range(4):
        assert all(np.array_equal(a, b) for a, b in zip(R[0]['A_pyr'] + R[0]['Ap_pyr'][0], R[i]['A_pyr'] + R[i]['Ap_pyr'][0]))
        for j in range(i):
            differ = int((R[i]['s'][1] != R[j]['s'][1]).any(axis=1).sum())
            assert differ > 243 // 2, (i, j, differ)
            assert not np.array_equal(R[i]['B_pyr'][1], R[j]['B_pyr'][1]) and not np.array_equal(R[i]['Bp_init'][0], R[j]['Bp_init'][0])
            assert R[i]['kappa'][0][2] != R[j]['kappa'][0][2]


def test_wide_kappa_changes_decisions():
    """the kappa rule decides differently under a neighbour's kappa factor on every variant (else
    a merge that reads job 0's kappa_factor for every job could pass)"""
    for ch in (2, 3):
        R = [AI.oracle(n) for n in AI.WIDE_CASES[ch]]
        for v in range(1, 4):
            kf0 = R[0]['kappa'][0][2]
            flips = sum(1 for da, dc, kf in R[v]['kappa'] if (dc <= da * kf) != (dc <= da * kf0))
            print('wide ch %d variant %d: %d kappa decisions differ under job 0\'s factor' % (ch, v, flips))
            assert flips > 0


def test_blas_ddot_sq_110_columns():
    """compute_distance at 2 channels is a 110-element dot: blas_ddot_sq must follow np.dot there
    (three 32-blocks, no 16-block, a 14-element tail), on hosts whose BLAS has the order the
    golden vectors were made with (oracle/gen_golden.py _check_blas_order)."""
    from oracle import gen_golden
    from oracle.ia_oracle import blas_ddot_sq
    try:
        gen_golden._check_blas_order()
    except SystemExit as e:
        pytest.skip('np.dot on this host does not follow the SkylakeX ddot order: %s' % e)
    rs = np.random.RandomState(110)
    w = AI.O.compute_weights(2)
    for scale in (1.0, 64.0, 2.0 ** -14, 1e-3):
        for _ in range(10):
            x = (rs.rand(110) - rs.rand(110)) * scale * w
            assert np.dot(x, x) == blas_ddot_sq(x)

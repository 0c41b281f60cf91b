"""The numpy restatement of k-coherence search (tests/kcoh_inputs.py) against the oracle, without a
GPU: with K = N_A - 1 every candidate list is the whole DB, so the level is the exact path's, bit
for bit; the duplicate rule of the similarity sets; and that the cases exercise what the GPU tests
compare (fallbacks stay few, the result differs from the exact path when K is far below N_A)."""
import numpy as np
import pytest

import kcoh_inputs as KI
from oracle import ia_oracle as O


@pytest.mark.parametrize('case,K', KI.FULL_K, ids=[c for c, _ in KI.FULL_K])
def test_full_similarity_sets_reproduce_the_exact_level(case, K):
    z = KI.make(case)
    assert K == KI.n_rows(z, 1) - 1
    kc, ex = KI.expected(case, K), KI.expected(case, K, exact=True)
    assert kc['kcoh_levels'] == [1] and ex['kcoh_levels'] == []
    assert np.array_equal(kc['s'][1], ex['s'][1]) and np.array_equal(kc['im'][1], ex['im'][1])
    assert np.array_equal(kc['Bp'][1], ex['Bp'][1])
    n_px = z['B_pyr'][1].shape[0] * z['B_pyr'][1].shape[1]
    assert 1 <= kc['fallbacks'][1] <= n_px
    if case == 't11':
        assert kc['fallbacks'][1] == n_px == 20 and kc['candidates'][1] == 0   # a 1 x 1 A: no shifted source inside


def test_p_app_of_a_full_set_is_the_exact_nn():
    """per pixel, not only in the outcome: the restatement's p_app rows equal nn_exact's"""
    z = KI.make('t44')
    As = KI.PI.build_db(z, 1)
    B_feat = O.feature_array(z['B_pyr'], 1, True)
    sim = KI.similarity_sets(As, 15)
    log_k, log_e = [], []
    with KI.blas_order():
        Bp = [x.copy() for x in z['Bp_init']]
        KI.synthesize_level(z['Ap_pyr'], B_feat, Bp, 1, z['L'], z['k'], z['weights'], As, sim, log=log_k)
        Bp = [x.copy() for x in z['Bp_init']]
        O.synthesize_level(None, z['Ap_pyr'], B_feat, Bp, 1, z['L'], z['k'], z['weights'], As=As, log=log_e)
    assert log_k == [p for p, _ in log_e]


def test_similarity_sets_of_a_constant_db_are_the_lowest_other_rows():
    """every distance ties at 0: row j's K + 1 nearest are rows 0..K, j deleted where present"""
    As = KI.PI.build_db(KI.make('const'), 1)
    assert len(As) == 120 and (As == As[0]).all()
    for K in (1, 4, 15):
        sim = KI.similarity_sets(As, K)
        for j in (0, 1, K - 1, K, K + 1, 119):
            assert list(sim[j]) == [i for i in range(K + 1) if i != j][:K]


def test_similarity_sets_keep_lower_duplicates_in_front():
    rs = np.random.RandomState(0)
    As = rs.rand(40, 55)
    As[30] = As[7]
    sim = KI.similarity_sets(As, 3)
    assert sim[30][0] == 7 and 30 not in sim[30]     # the duplicate with the lower index comes first, at distance 0
    assert sim[7][0] == 30 and 7 not in sim[7]
    assert all(j not in sim[j] for j in range(40)) and sim.dtype == np.int32


def test_small_k_leaves_few_fallbacks_and_is_not_the_exact_path():
    z = KI.make('main')
    n_px = z['B_pyr'][1].shape[0] * z['B_pyr'][1].shape[1]
    ex = KI.expected('main', 1, exact=True)
    for K in (1, 4, 15):
        kc = KI.expected('main', K)
        print('main K %2d: fallbacks %d of %d, candidates %d, pixels equal to the exact path %d'
              % (K, kc['fallbacks'][1], n_px, kc['candidates'][1], int((kc['s'][1] == ex['s'][1]).all(axis=1).sum())))
        assert 1 <= kc['fallbacks'][1] < n_px // 10      # few: the first pixel, and under a tenth of the level
        assert kc['candidates'][1] <= 12 * (K + 1) * n_px
        assert not np.array_equal(kc['s'][1], ex['s'][1])


# the pixels without a base row of wide32's four variants (K = 4), as KI.no_base_pixels finds them in the
# restatement's final s / im
WIDE32_NO_BASE = {0: [(0, 0), (0, 3), (0, 8), (0, 9), (3, 0)], 1: [(0, 0), (0, 7)],
                  2: [(0, 0), (0, 5), (0, 10), (1, 0), (3, 12), (6, 10)], 3: [(0, 0), (0, 10), (8, 10), (8, 12)]}


def test_wide32_puts_fallback_pixels_into_the_scan_waves_second_and_third_trip():
    """32 jobs on main's A side, job j = variant j mod 4: steps of up to 160 queries, which k_kcoh_step's scan
    waves test 64 at a time; a pixel without a base row at query m >= 64 and at m >= 128 makes their second and
    third trip do work (part[m H + h] and cnt[m] there)"""
    b_hw, a_hw = (11, 13), (12, 10)
    fb = {}
    for v in range(4):
        z, e = KI.make('wide32_v%d' % v), KI.expected('wide32_v%d' % v, KI.WIDE32_K)
        assert z['B_pyr'][1].shape == b_hw and z['A_pyr'][1].shape == a_hw and KI.n_rows(z, 1) == 120
        assert np.array_equal(z['A_pyr'][1], KI.make('main')['A_pyr'][1]) and e['kcoh_levels'] == [1]
        fb[v] = KI.no_base_pixels(e['s'][1], e['im'][1], b_hw, a_hw)
        assert fb[v] == WIDE32_NO_BASE[v] and len(fb[v]) == e['fallbacks'][1]
    assert -(-120 // 64) == 2                                       # H: the scan waves at 120 rows
    steps = KI.step_queries(b_hw, 32)
    assert len(steps) == 43 and max(len(q) for q in steps.values()) == 160
    at = {t: sorted(m for (j, r, c), m in q.items() if (r, c) in fb[j % 4]) for t, q in steps.items()}
    # step 9, (0, 9) (1, 6) (2, 3) (3, 0): two fallbacks per variant-0 job, jobs 16 .. 28 in the second trip
    assert at[9] == sorted(m for j in range(0, 32, 4) for m in (4 * j, 4 * j + 3))
    assert [m for m in at[9] if 64 <= m < 128] == [64, 67, 80, 83, 96, 99, 112, 115]
    # step 10, (0, 10) (1, 7) (2, 4) (3, 1): variants 2 and 3 in one ballot
    assert at[10] == sorted(4 * j for j in range(32) if j % 4 in (2, 3)) and {8, 12} <= set(at[10])
    # step 21, (3, 12) .. (7, 0): variant 2's (3, 12) at m = 5 j, up to the third trip
    assert at[21] == [5 * j for j in range(2, 32, 4)] == [10, 30, 50, 70, 90, 110, 130, 150]
    assert any(64 <= m < 128 for ms in at.values() for m in ms) and any(m >= 128 for ms in at.values() for m in ms)
    assert sum(len(ms) for ms in at.values()) == 8 * sum(len(v) for v in fb.values()) == 136


def test_chained_levels_switch_at_min_rows():
    """the pyramid case: 30 and 120 DB rows; min_rows = 100 leaves level 1 exact"""
    both, fine = KI.expected('pyr', 4), KI.expected('pyr', 4, min_rows=100)
    assert both['kcoh_levels'] == [1, 2] and fine['kcoh_levels'] == [2]
    ex = KI.expected('pyr', 4, exact=True)
    assert np.array_equal(fine['s'][1], ex['s'][1]) and np.array_equal(fine['Bp'][1], ex['Bp'][1])

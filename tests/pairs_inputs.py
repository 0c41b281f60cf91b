"""Inputs and the oracle runner for training pairs (A_i, A'_i): an A image of its own per A' image
(include/ia.h ia_level_args.n_a = n_ap).  Pure numpy, no GPU import.

A case is shaped like tests/adversarial_inputs.py's: A_pyr, Ap_pyr (n A' pyramids), B_pyr, Bp_init,
L, k, weights - plus 'A_pairs', the list of the n A pyramids.  A_pyr is A_pairs[0], so every helper
that reads shapes from A_pyr (golden_util.check_debug_records, scan_counts) applies, and so that the
run which shares A_0 among all A' images (the reference's DB, algorithms.py:63-67) is the same case
without 'A_pairs'.

The oracle needs no change for pairs: oracle.ia_oracle.synthesize_level takes a prebuilt DB (As=).
run_oracle is adversarial_inputs.run_oracle with the level loop written out and
    As = vstack_i hstack(feature_array(A_i, l, True), feature_array(A'_i, l, False)).
"""
import numpy as np

import adversarial_inputs as AI
from oracle import ia_oracle as O

BASE, BIG, GATE = AI.BASE, AI.BIG, AI.GATE
DRIVER_HW = (24, 24)


def _rand_pairs(seed, n, geo=BASE, ch=1, k=0.5, a_side=None):
    """every level rand, in the style of adversarial_inputs._affine: the n A pyramids, then the n A'
    pyramids, then B and the B' initialisation.  a_side[i] (optional) maps A_i's levels."""
    rs = np.random.RandomState(seed)
    sa, sb = AI.level_shapes(geo['a_hw'], geo['L'], ch), AI.level_shapes(geo['b_hw'], geo['L'], ch)
    A = [[rs.rand(*s) for s in sa] for _ in range(n)]
    Ap = [[rs.rand(*s) for s in sa] for _ in range(n)]
    B = [rs.rand(*s) for s in sb]
    Bp = [rs.rand(*s) for s in sb]
    if a_side is not None:
        A = [[f(x) for x in p] for f, p in zip(a_side, A)]
    z = AI._case(A[0], Ap, B, Bp, k, ch)
    z['A_pairs'] = A
    return z


def _centring(seed=46):
    """A_0 = rand, A_1 = 50 + 1e-3 rand: the (part, channel) means of parts 0 and 1 must be taken over
    both images (25.25, not A_0's 0.5).  B's right half sits at A_1's offset, so both images are
    picked: there only the 1e-3 of contrast decides."""
    z = _rand_pairs(seed, 2, a_side=[lambda x: x, lambda x: 50 + 1e-3 * x])
    for x in z['B_pyr']:
        x[:, x.shape[1] // 2:] = 50 + 1e-3 * x[:, x.shape[1] // 2:]
    return z


def _gate(ch, kind):
    """GATE geometry, 2 pairs; kind None: every value in range; 'A' / 'Ac': 64.5 at the LAST element
    of the fine / coarse level of A_1, the last value of the stacked A / Ac arrays"""
    z = _rand_pairs(130 + ch, 2, geo=GATE, ch=ch)
    if kind is not None:
        arr = z['A_pairs'][1][1 if kind == 'A' else 0]
        arr[(-1,) * arr.ndim] = 64.5
    return z


def _driver_images(ch3):
    """two (A, A') pairs and a B of DRIVER_HW for image_analogies_main (RGB in [0, 1] when ch3)"""
    rs = np.random.RandomState(60 + int(ch3))
    shp = DRIVER_HW + ((3,) if ch3 else ())
    return dict(A=[rs.rand(*shp), rs.rand(*shp)], Ap=[rs.rand(*shp), rs.rand(*shp)], B=rs.rand(*shp))


CASES = {}
# straddling rows: 475 rows per image, 32-row tiles and K1b's 64-row waves straddle two images
BASE_CASES = []
for _ch in (1, 2, 3):
    for _n in (2, 3):
        CASES['p%d_c%d' % (_n, _ch)] = (lambda n, ch: lambda: _rand_pairs(40 + ch, n, ch=ch))(_n, _ch)
        BASE_CASES.append('p%d_c%d' % (_n, _ch))
# 2 x 8,280 rows = 518 tiles, the last partial
CASES['big2'] = lambda: _rand_pairs(47, 2, geo=BIG)
CASES['centring'] = _centring
# a second job for the 2-pair A side of p2_c1: its own B side and kappa
CASES['p2_c1_job1'] = lambda: AI.with_b_side(CASES['p2_c1'](), _rand_pairs(48, 2), 5.0)
GATE_KINDS = [(1, 'A'), (1, 'Ac'), (2, 'A'), (2, 'Ac')]
for _ch in (1, 2):
    for _kind in (None, 'A', 'Ac'):
        CASES['gate_c%d_%s' % (_ch, _kind or 'in')] = (lambda ch, kind: lambda: _gate(ch, kind))(_ch, _kind)
PAIR_CASES = BASE_CASES + ['big2', 'centring', 'p2_c1_job1'] + [n for n in CASES if n.startswith('gate')]


def make(name):
    return CASES[name]()


def case_ch(name):
    """channel count of a case, from the '_c<ch>' in its name (none: 1)"""
    return int(name.split('_c')[1][0]) if '_c' in name else 1


def shared_a0(z):
    """the case with A_0 shared by every A' image: what a build that ignores A_1.. computes"""
    r = {k: v for k, v in z.items() if k != 'A_pairs'}
    return r


def build_db(z, level):
    """the DB of a level: per image [A_i full | A'_i half] (A_i = A_pyr without 'A_pairs')"""
    A = z.get('A_pairs') or [z['A_pyr']] * len(z['Ap_pyr'])
    return np.vstack([np.hstack([O.feature_array(a, level, True), O.feature_array(p, level, False)])
                      for a, p in zip(A, z['Ap_pyr'])])


def run_oracle(z, nn_stats=False):
    """adversarial_inputs.run_oracle on a pairs case (or, without 'A_pairs', on its shared-A run):
    compute_distance in the explicit BLAS order, NN rows, coherence picks and distances logged as
    golden_util.check_debug_records compares them; with nn_stats 'nn' = per pixel (gap, exact,
    lowest) as there."""
    nn = []
    nn_exact, compute_distance = O.nn_exact, O.compute_distance

    def nn_logged(As, q):
        i, d = nn_exact(As, q)
        two = np.partition(d, 1)[:2]
        gap = (two[1] - two[0]) / two[0] if two[0] > 0 else (0.0 if two[1] == 0 else np.inf)
        near = np.flatnonzero(d <= d[i] * (1 + AI.REL_TIE))
        nn.append((gap, int((d == d[i]).sum()), bool(near[0] == i)))
        return i, d

    L = z['L']
    O.compute_distance = O.compute_distance_blas
    if nn_stats:
        O.nn_exact = nn_logged
    try:
        Bp = [x.copy() for x in z['Bp_init']]
        log, S, IM = [], {}, {}
        for level in range(1, L):
            B_feat = O.feature_array(z['B_pyr'], level, True)
            S[level], IM[level] = O.synthesize_level(None, z['Ap_pyr'], B_feat, Bp, level, L, z['k'], z['weights'],
                                                     As=build_db(z, level), log=log)
    finally:
        O.nn_exact, O.compute_distance = nn_exact, compute_distance
    r = dict(z)
    r.update(s=S, im=IM, Bp_final=Bp, app_ix=np.array([p for p, _ in log], dtype=np.int64), nn=nn)
    coh, dist, kappa, at = [], [], [], 0
    for level in range(1, L):
        n = z['B_pyr'][level].shape[0] * z['B_pyr'][level].shape[1]
        kf = 1 + (2 ** (level - L)) * z['k']
        for qi in range(1, n):     # the level's first pixel never consults coherence
            rec = log[at + qi][1]
            if rec is None:
                coh.append((-1, -1, 0))
            else:
                coh.append((rec[0][0], rec[0][1], rec[1]))
                dist.extend(rec[2:])
                kappa.append((rec[2], rec[3], kf))
        assert log[at][1] is None
        at += n
    assert at == len(log)
    r.update(coh=np.array(coh, dtype=np.int64), dist=np.array(dist), kappa=kappa)
    return r


_ORACLE = {}


def oracle(name, shared=False):
    """run_oracle(make(name), nn_stats=True) - or of its shared-A_0 run - once per process; read-only"""
    if (name, shared) not in _ORACLE:
        z = make(name)
        _ORACLE[name, shared] = run_oracle(shared_a0(z) if shared else z, nn_stats=not shared)
    return _ORACLE[name, shared]


def oracle_pyramids(A_pairs, Ap_pyr, B_pyr, Bp_init, k, weights):
    """the oracle on pyramids a driver built (img_setup): (S, IM, B' pyramid)"""
    z = dict(A_pyr=A_pairs[0], A_pairs=A_pairs, Ap_pyr=Ap_pyr, B_pyr=B_pyr, Bp_init=Bp_init, L=len(B_pyr), k=float(k),
             weights=weights)
    r = run_oracle(z)
    return r['s'], r['im'], r['Bp_final']

"""Adversarial inputs for the certified matchers (pure numpy, no GPU import): image values at the
top and the bottom of the split-f16 range, a large common offset with tiny contrast, DB rows that
are near-ties but not ties, a constant A side, kappa = 0, a DB of more than 256 tiles and the
+-64 gate of the split-f16 matcher with its one out-of-range value in each array in turn.

Every generator is deterministic (np.random.RandomState) and returns a dict shaped like
golden_util.load_e2e's: A_pyr, Ap_pyr (a list of one A' pyramid), B_pyr, Bp_init as lists of fp64
arrays, coarsest first, with L, k and the feature weights.  Levels need not be real pyramids; only
the shape contract of oracle.ia_oracle.feature_array holds: level l-1 is ceil(h/2) x ceil(w/2).

run_oracle(z) runs oracle/ia_oracle.py (fp64, brute force) on a case and returns what
golden_util.check_debug_records compares a GPU run with, plus per-pixel figures on how close the
reference's own decisions are (tests/test_adversarial_inputs_cpu.py pins them).
"""
import numpy as np

from oracle import ia_oracle as O

BASE = dict(a_hw=(25, 19), b_hw=(16, 20), L=3)   # 475 DB rows = 15 tiles of 32, the last partial
BIG = dict(a_hw=(92, 90), b_hw=(12, 16), L=2)    # 8,280 rows = 259 tiles, the last with 24 rows
GATE = dict(a_hw=(9, 7), b_hw=(8, 6), L=2)
GATE_ARRAYS = ['A', 'Ac', 'Ap', 'Apc', 'B', 'Bc', 'Bpc', 'Bp']   # the order probe_matcher scans them
REL_TIE = 2.0 ** -20


def level_shapes(hw, L):
    """[(h, w)] of L levels, coarsest first"""
    out = [tuple(hw)]
    for _ in range(L - 1):
        out.insert(0, (-(-out[0][0] // 2), -(-out[0][1] // 2)))
    return out


def _case(A, Ap, B, Bp, k):
    return dict(A_pyr=A, Ap_pyr=[Ap], B_pyr=B, Bp_init=Bp, L=len(A), k=float(k), weights=O.compute_weights(1))


def _affine(seed, a_side, b_side, geo=BASE, k=0.5):
    """every level f(rand): a_side for A and A', b_side for B and the B' initialisation"""
    rs = np.random.RandomState(seed)
    sa, sb = level_shapes(geo['a_hw'], geo['L']), level_shapes(geo['b_hw'], geo['L'])
    A = [a_side(rs.rand(*s)) for s in sa]
    Ap = [a_side(rs.rand(*s)) for s in sa]
    B = [b_side(rs.rand(*s)) for s in sb]
    Bp = [b_side(rs.rand(*s)) for s in sb]
    return _case(A, Ap, B, Bp, k)


def _periodic(patch, hw):
    P = patch.shape[0]
    return np.tile(patch, (-(-hw[0] // P), -(-hw[1] // P)))[:hw[0], :hw[1]]


def _neartie(seed, delta, geo=BASE, k=0.5):
    """A and A' levels: a random P x P patch repeated (P = 8 at the finest level, halved per coarser
    level, so interior windows of different copies hold the same values on every level) plus
    delta * rand: DB rows in groups equal to within delta.  B: the same patch pattern at B's shape
    plus 1e-3 * rand, so each query's nearest rows are one such group; B' initialisation rand."""
    rs = np.random.RandomState(seed)
    L = geo['L']
    sa, sb = level_shapes(geo['a_hw'], L), level_shapes(geo['b_hw'], L)
    A, Ap, B, Bp = [], [], [], []
    for l in range(L):
        P = 8 >> (L - 1 - l)
        assert P >= 1
        pa, pp = rs.rand(P, P), rs.rand(P, P)
        A.append(_periodic(pa, sa[l]) + delta * rs.rand(*sa[l]))
        Ap.append(_periodic(pp, sa[l]) + delta * rs.rand(*sa[l]))
        B.append(_periodic(pa, sb[l]) + 1e-3 * rs.rand(*sb[l]))
        Bp.append(rs.rand(*sb[l]))
    return _case(A, Ap, B, Bp, k)


def _const_a(seed):
    z = _affine(seed, lambda x: x, lambda x: x)
    z['A_pyr'] = [np.full_like(x, 0.25) for x in z['A_pyr']]
    z['Ap_pyr'] = [[np.full_like(x, 0.25) for x in z['Ap_pyr'][0]]]
    return z


def _gate(i):
    """rand everywhere, element (1, 2) of array i (GATE_ARRAYS) set to 64.5.  In the B' initialisation
    row 0's queries read it through the reflected rows above the image before it is overwritten."""
    z = _affine(100 + i, lambda x: x, lambda x: x, geo=GATE)
    arr = {'A': z['A_pyr'][1], 'Ac': z['A_pyr'][0], 'Ap': z['Ap_pyr'][0][1], 'Apc': z['Ap_pyr'][0][0],
           'B': z['B_pyr'][1], 'Bc': z['B_pyr'][0], 'Bpc': z['Bp_init'][0], 'Bp': z['Bp_init'][1]}[GATE_ARRAYS[i]]
    arr[1, 2] = 64.5
    return z


CASES = {
    'x60': lambda: _affine(1, lambda x: 60 * x, lambda x: 60 * x),
    'x64edge': lambda: _affine(2, lambda x: 64 * x, lambda x: 64 * x),
    'signed': lambda: _affine(3, lambda x: 120 * x - 60, lambda x: 120 * x - 60),
    'tiny': lambda: _affine(4, lambda x: 2.0 ** -14 * x, lambda x: 2.0 ** -14 * x),
    # q - a = -100 - 1e-3 (u_a - u_q) in every column: d_i - d_j = 200e-3 sum (u_i - u_j) whatever the
    # query, so a handful of DB rows (the smallest noise sums) win every pixel by a relative ~1e-7
    'offset': lambda: _affine(45, lambda x: 50 + 1e-3 * x, lambda x: -50 + 1e-3 * x),
    'constA': lambda: _const_a(6),
    'neartie26': lambda: _neartie(7, 2.0 ** -26),
    'neartie36': lambda: _neartie(8, 2.0 ** -36),
    'k0': lambda: _affine(9, lambda x: x, lambda x: x, k=0.0),
    'bigA': lambda: _affine(10, lambda x: x, lambda x: x, geo=BIG),
    'bigA_neartie': lambda: _neartie(11, 2.0 ** -26, geo=BIG),
}
for _i in range(8):
    CASES['gate%d' % _i] = (lambda i: lambda: _gate(i))(_i)
BASE_CASES = ['x60', 'x64edge', 'signed', 'tiny', 'offset', 'constA', 'neartie26', 'neartie36']
BIG_CASES = ['bigA', 'bigA_neartie']
GATE_CASES = ['gate%d' % i for i in range(8)]


def make(name):
    return CASES[name]()


def all_arrays(z):
    """the eight arrays of GATE_ARRAYS' kinds, over every level: {kind: [arrays]}"""
    L = z['L']
    fine, coarse = range(1, L), range(0, L - 1)
    return {'A': [z['A_pyr'][l] for l in fine], 'Ac': [z['A_pyr'][l] for l in coarse],
            'Ap': [p[l] for p in z['Ap_pyr'] for l in fine], 'Apc': [p[l] for p in z['Ap_pyr'] for l in coarse],
            'B': [z['B_pyr'][l] for l in fine], 'Bc': [z['B_pyr'][l] for l in coarse],
            'Bpc': [z['Bp_init'][l] for l in coarse], 'Bp': [z['Bp_init'][l] for l in fine]}


_ORACLE = {}


def oracle(name):
    """run_oracle(make(name), nn_stats=True), computed once per process; read-only"""
    if name not in _ORACLE:
        _ORACLE[name] = run_oracle(make(name), nn_stats=True)
    return _ORACLE[name]


def run_oracle(z, nn_stats=False):
    """The oracle's run of every level of z, with compute_distance in the explicit BLAS dot order
    (compute_distance_blas), so the kappa rule's inputs do not depend on the host's BLAS.  Returns a
    copy of z with s, im, Bp_final, app_ix, coh and dist as golden_util.load_e2e gives them, 'kappa'
    = [(d_app, d_coh, kf)] per kappa comparison, and with nn_stats 'nn' = per pixel
    (gap, exact, lowest): the runner-up's relative distance gap to the winner, how many rows are at
    exactly the winner's distance, and whether the winner is the lowest-index row within a
    relative REL_TIE of it."""
    nn = []
    nn_exact, compute_distance = O.nn_exact, O.compute_distance

    def nn_logged(As, q):
        i, d = nn_exact(As, q)
        two = np.partition(d, 1)[:2] if len(d) > 1 else np.array([d[0], np.inf])
        gap = (two[1] - two[0]) / two[0] if two[0] > 0 else (0.0 if two[1] == 0 else np.inf)
        near = np.flatnonzero(d <= d[i] * (1 + REL_TIE))
        nn.append((gap, int((d == d[i]).sum()), bool(near[0] == i)))
        return i, d

    O.compute_distance = O.compute_distance_blas
    if nn_stats:
        O.nn_exact = nn_logged
    try:
        Bp = [x.copy() for x in z['Bp_init']]
        log = []
        S, IM = O.run_all_levels(z['A_pyr'], z['Ap_pyr'], z['B_pyr'], Bp, z['k'], z['weights'], log=log)
    finally:
        O.nn_exact, O.compute_distance = nn_exact, compute_distance
    r = dict(z)
    r.update(s=S, im=IM, Bp_final=Bp, app_ix=np.array([p for p, _ in log], dtype=np.int64), nn=nn)
    coh, dist, kappa, at = [], [], [], 0
    for level in range(1, z['L']):
        n = z['B_pyr'][level].shape[0] * z['B_pyr'][level].shape[1]
        kf = 1 + (2 ** (level - z['L'])) * z['k']
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

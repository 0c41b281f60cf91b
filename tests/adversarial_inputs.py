"""Adversarial inputs for the certified matchers (pure numpy, no GPU import): image values at the
top and the bottom of the split-f16 range, a large common offset with tiny contrast, DB rows that
are near-ties but not ties, a constant A side, kappa = 0, a DB of more than 256 tiles and the
+-64 gate of the split-f16 matcher with its one out-of-range value in each array in turn - at 1
channel, and again at 2 and 3 channels (name + '_c2' / '_c3'), where every kernel stage is another
instance with its own bound constants, plus two A' images, a wide batch and the gate's last element.

Every generator is deterministic (np.random.RandomState) and returns a dict shaped like
golden_util.load_e2e's: A_pyr, Ap_pyr (a list of n_ap A' pyramids), B_pyr, Bp_init as lists of fp64
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
# steps of min(9, 27 / 3) = 9 queries at the widest, ramping 1, 1, 1, 2, 2, 2, ... 9: 32 batched jobs put
# 32, 64, ... 288 queries = 1 to 9 query tiles in a step (tests/test_gpu_channels.py wide32)
WIDE = dict(a_hw=(25, 19), b_hw=(9, 27), L=2)
GATE_ARRAYS = ['A', 'Ac', 'Ap', 'Apc', 'B', 'Bc', 'Bpc', 'Bp']   # the order probe_matcher scans them
REL_TIE = 2.0 ** -20


def level_shapes(hw, L, ch=1):
    """[(h, w)] of L levels, coarsest first; (h, w, ch) with ch > 1"""
    out = [tuple(hw)]
    for _ in range(L - 1):
        out.insert(0, (-(-out[0][0] // 2), -(-out[0][1] // 2)))
    return out if ch == 1 else [s + (ch,) for s in out]


def _case(A, Ap, B, Bp, k, ch=1):
    """Ap: a list of n_ap A' pyramids"""
    return dict(A_pyr=A, Ap_pyr=Ap, B_pyr=B, Bp_init=Bp, L=len(A), k=float(k), weights=O.compute_weights(ch))


def _affine(seed, a_side, b_side, geo=BASE, k=0.5, ch=1, n_ap=1):
    """every level f(rand): a_side for A and the n_ap A' images, b_side for B and the B' initialisation"""
    rs = np.random.RandomState(seed)
    sa, sb = level_shapes(geo['a_hw'], geo['L'], ch), level_shapes(geo['b_hw'], geo['L'], ch)
    A = [a_side(rs.rand(*s)) for s in sa]
    Ap = [[a_side(rs.rand(*s)) for s in sa] for _ in range(n_ap)]
    B = [b_side(rs.rand(*s)) for s in sb]
    Bp = [b_side(rs.rand(*s)) for s in sb]
    return _case(A, Ap, B, Bp, k, ch)


def _periodic(patch, shape):
    P = patch.shape[0]
    return np.tile(patch, (-(-shape[0] // P), -(-shape[1] // P)) + (1,) * (patch.ndim - 2))[:shape[0], :shape[1]]


def _neartie(seed, delta, geo=BASE, k=0.5, ch=1, n_ap=1):
    """A and A' levels: a random P x P (x ch) patch repeated (P = 8 at the finest level, halved per
    coarser level, so interior windows of different copies hold the same values on every level) plus
    delta * rand: DB rows in groups equal to within delta.  B: the same patch pattern at B's shape
    plus 1e-3 * rand, so each query's nearest rows are one such group; B' initialisation rand.
    Every A' image has its own patch and its own noise."""
    rs = np.random.RandomState(seed)
    L = geo['L']
    sa, sb = level_shapes(geo['a_hw'], L, ch), level_shapes(geo['b_hw'], L, ch)
    A, Ap, B, Bp = [], [[] for _ in range(n_ap)], [], []
    for l in range(L):
        P = 8 >> (L - 1 - l)
        assert P >= 1
        ps = (P, P) + sa[l][2:]
        pa, pp = rs.rand(*ps), [rs.rand(*ps) for _ in range(n_ap)]
        A.append(_periodic(pa, sa[l]) + delta * rs.rand(*sa[l]))
        for j in range(n_ap):
            Ap[j].append(_periodic(pp[j], sa[l]) + delta * rs.rand(*sa[l]))
        B.append(_periodic(pa, sb[l]) + 1e-3 * rs.rand(*sb[l]))
        Bp.append(rs.rand(*sb[l]))
    return _case(A, Ap, B, Bp, k, ch)


def _const_a(seed, ch=1, n_ap=1):
    z = _affine(seed, lambda x: x, lambda x: x, ch=ch, n_ap=n_ap)
    z['A_pyr'] = [np.full_like(x, 0.25) for x in z['A_pyr']]
    z['Ap_pyr'] = [[np.full_like(x, 0.25) for x in p] for p in z['Ap_pyr']]
    return z


def _gate_array(z, kind):
    """the array of GATE_ARRAYS' kind in a 2-level case (of the last A' image)"""
    return {'A': z['A_pyr'][1], 'Ac': z['A_pyr'][0], 'Ap': z['Ap_pyr'][-1][1], 'Apc': z['Ap_pyr'][-1][0],
            'B': z['B_pyr'][1], 'Bc': z['B_pyr'][0], 'Bpc': z['Bp_init'][0], 'Bp': z['Bp_init'][1]}[kind]


def _gate(i, ch=1, n_ap=1, last=False):
    """rand everywhere, one element of array i (GATE_ARRAYS) set to 64.5: element (1, 2), or with
    `last` the array's last element [h-1, w-1, ch-1], which a scan sized in pixels instead of
    values never reaches.  In the B' initialisation row 0's queries read element (1, 2) through the
    reflected rows above the image before it is overwritten; its last element is overwritten unread,
    and still decides the matcher."""
    z = _affine(100 + i, lambda x: x, lambda x: x, geo=GATE, ch=ch, n_ap=n_ap)
    arr = _gate_array(z, GATE_ARRAYS[i])
    arr[(-1,) * arr.ndim if last else (1, 2)] = 64.5
    return z


def with_b_side(za, zb, k):
    """the job of zb's B side (B pyramid and B' initialisation) on za's A side"""
    z = dict(za)
    z.update(B_pyr=zb['B_pyr'], Bp_init=zb['Bp_init'], k=float(k))
    return z


WIDE_K = (0.5, 1.0, 5.0, 25.0)   # a kappa factor of its own per variant; not 0 (no kappa comparison at equality)


def _wide(v, ch):
    """variant v of the wide batch: the A side of seed 30, the B side of seed 30 + v, k = WIDE_K[v]"""
    ident = lambda x: x
    za = _affine(30, ident, ident, geo=WIDE, ch=ch)
    return za if v == 0 else with_b_side(za, _affine(30 + v, ident, ident, geo=WIDE, ch=ch), WIDE_K[v])


GATE_JOB1_KINDS = GATE_ARRAYS[4:]


def _gate_job1(kind, ch):
    """job 1 of a two-job batch on the A side of seed 120: every value in range (kind None: this is
    also job 0, with the B side of seed 120) or 64.5 at the last element of its array `kind`"""
    ident = lambda x: x
    za = _affine(120, ident, ident, geo=GATE, ch=ch)
    if kind is None:
        return za
    z = with_b_side(za, _affine(121, ident, ident, geo=GATE, ch=ch), 0.5)
    arr = _gate_array(z, kind)
    arr[(-1,) * arr.ndim] = 64.5
    return z


# name -> generator(ch=, n_ap=); CASES[name] is the 1-channel case, CASES[name + '_c2' / '_c3'] the 2- / 3-channel one
_GEN = {
    'x60': lambda **kw: _affine(1, lambda x: 60 * x, lambda x: 60 * x, **kw),
    'x64edge': lambda **kw: _affine(2, lambda x: 64 * x, lambda x: 64 * x, **kw),
    'signed': lambda **kw: _affine(3, lambda x: 120 * x - 60, lambda x: 120 * x - 60, **kw),
    'tiny': lambda **kw: _affine(4, lambda x: 2.0 ** -14 * x, lambda x: 2.0 ** -14 * x, **kw),
    # q - a = -100 - 1e-3 (u_a - u_q) in every column: d_i - d_j = 200e-3 sum (u_i - u_j) whatever the
    # query, so a handful of DB rows (the smallest noise sums) win every pixel by a relative ~1e-7
    'offset': lambda **kw: _affine(45, lambda x: 50 + 1e-3 * x, lambda x: -50 + 1e-3 * x, **kw),
    'constA': lambda **kw: _const_a(6, **kw),
    'neartie26': lambda **kw: _neartie(7, 2.0 ** -26, **kw),
    'neartie36': lambda **kw: _neartie(8, 2.0 ** -36, **kw),
    'k0': lambda **kw: _affine(9, lambda x: x, lambda x: x, k=0.0, **kw),
    'bigA': lambda **kw: _affine(10, lambda x: x, lambda x: x, geo=BIG, **kw),
    'bigA_neartie': lambda **kw: _neartie(11, 2.0 ** -26, geo=BIG, **kw),
}
CASES = {n: (lambda f: lambda: f())(f) for n, f in _GEN.items()}
for _i in range(8):
    CASES['gate%d' % _i] = (lambda i: lambda: _gate(i))(_i)
BASE_CASES = ['x60', 'x64edge', 'signed', 'tiny', 'offset', 'constA', 'neartie26', 'neartie36']
BIG_CASES = ['bigA', 'bigA_neartie']
GATE_CASES = ['gate%d' % i for i in range(8)]

# ---- 2 and 3 channels (tests/test_gpu_channels.py).  The reference writes colour back for 3 channels
# only, so 2-channel images have no reference run: the oracle, channel-generic, is their one reference.
CH3_BASE = ['offset', 'tiny', 'neartie36', 'constA']


def _add(name, ch, gen):
    CASES['%s_c%d' % (name, ch)] = gen
    return '%s_c%d' % (name, ch)


BASE_CH_CASES = ([_add(n, 2, (lambda f: lambda: f(ch=2))(_GEN[n])) for n in BASE_CASES] +
                 [_add(n, 3, (lambda f: lambda: f(ch=3))(_GEN[n])) for n in CH3_BASE])
# two A' images: 950 rows in 30 tiles, DB row -> (image, r, c), writeback from the second image
MULTIAP_CASES = [_add('multiap', ch, (lambda ch: lambda: _affine(12, lambda x: x, lambda x: x, ch=ch, n_ap=2))(ch))
                 for ch in (2, 3)]
BIG_CH_CASES = [_add('bigA', ch, (lambda ch: lambda: _GEN['bigA'](ch=ch))(ch)) for ch in (2, 3)]
WIDE_CASES = {ch: [_add('wide_v%d' % v, ch, (lambda v, ch: lambda: _wide(v, ch))(v, ch)) for v in range(4)]
              for ch in (2, 3)}
GATE_LAST_CASES = [_add('gateL%d' % i, 2, (lambda i: lambda: _gate(i, ch=2, last=True))(i)) for i in range(8)]
GATE_JOB0 = _add('gate_job0', 2, lambda: _gate_job1(None, 2))
GATE_JOB1_CASES = [_add('gate_job1_%s' % kd, 2, (lambda kd: lambda: _gate_job1(kd, 2))(kd)) for kd in GATE_JOB1_KINDS]
CH_CASES = (BASE_CH_CASES + MULTIAP_CASES + BIG_CH_CASES + WIDE_CASES[2] + WIDE_CASES[3] + GATE_LAST_CASES +
            [GATE_JOB0] + GATE_JOB1_CASES)


# 2-channel cases whose third-nearest row is so far from the winner that a correct split-f16 run
# rescans nothing (certify_margin > 1, pinned by tests/test_adversarial_inputs_cpu.py)
NO_FALLBACK_C2 = ['x60_c2', 'x64edge_c2', 'signed_c2', 'offset_c2', 'multiap_c2', 'bigA_c2'] + WIDE_CASES[2]


def case_ch(name):
    """channel count of a case, from its name"""
    return int(name[-1]) if name[-3:-1] == '_c' else 1


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


def part_channel_means(As, ch):
    """per DB column, the mean over the rows and over the columns of its part (A coarse 3 x 3, A fine
    5 x 5, A' coarse 3 x 3, A' fine first 12) and channel: what the matchers centre rows and queries
    by, up to the weight of the reflected border pixels (the kernels average the images)"""
    mu = np.empty(As.shape[1])
    at = 0
    for n in (9, 25, 9, 12):
        for c in range(ch):
            mu[at + c:at + n * ch:ch] = As[:, at + c:at + n * ch:ch].mean()
        at += n * ch
    assert at == As.shape[1]
    return mu


def split_f16_eps(KS, R, qn):
    """the certified bound of a split-f16 scan value, packed epilogue (ia_internal.h ia_eps_c_h,
    ia_eps_a_h): eps_c (R^2 + 2 R |q'|) + eps_a (R^2 + 14 R + 28 |q'| + 260)"""
    nu = (48.0 * KS + 4) * 2.0 ** -23
    eps_c = 1.05 * (nu / (1.0 - nu) * (1.0 + 1.0 / 512) + 3.5 * 2.0 ** -22) + 1.01 * 2.0 ** -19
    return eps_c * (R * R + 2 * R * qn) + 1.05 * 2.0 ** -25 * (R * R + 14 * R + 28 * qn + 260)


def certify_margin(r, KS):
    """min over the pixels of (d3 - d1) / (4 eps), eps at 1.1 R and 1.1 |q'| (the margin covers the
    border weighting of part_channel_means, ~1% of R here).  A scan value is within eps of exact, a
    row is a rerank candidate when its value is <= the best value + 2 eps, and a chunk is rescanned
    when a third row of it is: above 1, no chunk of any pixel can need a rescan, however the DB is
    split into chunks or shards - a correct split-f16 run has fallbacks == 0."""
    return min(g3 / (4 * split_f16_eps(KS, 1.1 * R, 1.1 * qn)) for g3, R, qn in r['third'])


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
    relative REL_TIE of it; and 'third' = per pixel (d3 - d1, R, |q'|): the third-nearest row's distance
    above the winner's, and the two norms the certified bounds scale with (split_f16_eps)."""
    nn, third = [], []
    nn_exact, compute_distance = O.nn_exact, O.compute_distance
    centre = {}

    def nn_logged(As, q):
        i, d = nn_exact(As, q)
        two = np.partition(d, 1)[:2] if len(d) > 1 else np.array([d[0], np.inf])
        gap = (two[1] - two[0]) / two[0] if two[0] > 0 else (0.0 if two[1] == 0 else np.inf)
        near = np.flatnonzero(d <= d[i] * (1 + REL_TIE))
        nn.append((gap, int((d == d[i]).sum()), bool(near[0] == i)))
        if id(As) not in centre:   # one DB per level: its (part, channel) means and largest centred row norm
            mu = part_channel_means(As, z['weights'].size // 55)
            centre[id(As)] = (As, mu, float(np.sqrt(((As - mu) ** 2).sum(axis=1).max())))
        _, mu, R = centre[id(As)]
        third.append((float(np.partition(d, 2)[2] - d[i]), R, float(np.sqrt(((q - mu) ** 2).sum()))))
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
    r.update(s=S, im=IM, Bp_final=Bp, app_ix=np.array([p for p, _ in log], dtype=np.int64), nn=nn, third=third)
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

"""k-coherence search (include/ia.h ia_synthesize_levels_kcoh): a numpy restatement of
the rule built from oracle/ia_oracle.py's functions, and the cases.  Pure numpy, no GPU import.

The rule, per level with DB rows As (N_A x 55 ch) and similarity sets sim (N_A x K):
  * sim[j]: the K + 1 nearest rows of row j in ascending (fp64 pairwise squared L2, row index), the
    entry equal to j deleted if present, the first K of the rest;
  * a pixel's base rows are best_coherence_match's candidates (oracle coherence(): the causal cells
    in window order whose shifted source lies inside A); its candidates are every base row b and
    sim[b]; p_app = the candidate with the smallest (d, row), d = ((As[row] - q) ** 2).sum();
  * p_coh = the first argmin of sqrt(d) over the base rows; kappa rule and writeback as the oracle's;
  * a pixel without a base row takes nn_exact over the whole DB and has no coherence candidate.

A case is shaped like tests/adversarial_inputs.py's (A_pyr, Ap_pyr, B_pyr, Bp_init, L, k, weights, and
'A_pairs' for one A per A').  compute_distance runs in the explicit BLAS order (blas_order), as in
every GPU parity test here.
"""
import contextlib

import numpy as np

import adversarial_inputs as AI
import pairs_inputs as PI
from oracle import ia_oracle as O

KCOH_MAX = 15
MAIN = dict(a_hw=(12, 10), b_hw=(11, 13), L=2)    # 120 DB rows; 3 or 4 fallback pixels of 143
T44 = dict(a_hw=(4, 4), b_hw=(9, 7), L=2)         # the issue's table: K = N_A - 1 is the exact path
T23 = dict(a_hw=(2, 3), b_hw=(6, 5), L=2)
T11 = dict(a_hw=(1, 1), b_hw=(5, 4), L=2)         # three A': N_A = 3, every pixel falls back
PYR = dict(a_hw=(12, 10), b_hw=(11, 13), L=3)     # two synthesised levels (30 and 120 rows)
ident = lambda x: x


@contextlib.contextmanager
def blas_order():
    """oracle compute_distance in the explicit OpenBLAS order (machine-independent), as pairs_inputs.run_oracle"""
    keep = O.compute_distance
    O.compute_distance = O.compute_distance_blas
    try:
        yield
    finally:
        O.compute_distance = keep


def similarity_sets(As, K):
    """sim (N_A, K) int32 by brute force"""
    n = len(As)
    assert 1 <= K <= min(KCOH_MAX, n - 1)
    out = np.empty((n, K), dtype=np.int32)
    idx = np.arange(n)
    for j in range(n):
        d = ((As - As[j]) ** 2).sum(axis=1)
        order = idx[np.lexsort((idx, d))][:K + 1]      # ascending (distance, row index)
        out[j] = order[order != j][:K]
    return out


def synthesize_level(Ap_pyr_list, B_feat_l, Bp_pyr, level, L, k, weights, As, sim, log=None):
    """One k-coherence level; Bp_pyr[level] is updated in place.  Returns (s, im, fallbacks, candidates):
    pixels without a base row, and candidate rows whose distance was computed (base rows and their
    similar rows, repeats included; a fallback pixel's DB scan is not counted).  log (a list) receives
    each pixel's p_app row."""
    h, w = Bp_pyr[level].shape[:2]
    A_h, A_w = Ap_pyr_list[0][level].shape[:2]
    s = np.zeros((h * w, 2), dtype=np.int64)
    im = np.zeros(h * w, dtype=np.int64)
    kf = 1 + (2 ** (level - L)) * k
    fallbacks = candidates = 0
    for qi in range(h * w):
        r, c = divmod(qi, w)
        q = O.query_feature(B_feat_l, Bp_pyr[level - 1], Bp_pyr[level], r, c, w)
        base, src = [], []
        for rr in range(max(0, r - 2), r + 1):                  # best_coherence_match's window order
            for rc in range(max(0, c - 2), min(w, c + 3)):
                ri = rr * w + rc
                if ri >= qi:
                    continue
                pr, pc = s[ri, 0] + r - rr, s[ri, 1] + c - rc
                if 0 <= pr < A_h and 0 <= pc < A_w:
                    base.append(int((A_h * im[ri] + pr) * A_w + pc))
                    src.append(((int(pr), int(pc)), int(im[ri])))
        if base:
            rows = np.array([x for b in base for x in [b] + [int(v) for v in sim[b]]], dtype=np.int64)
            d = ((As[rows] - q) ** 2).sum(axis=1)
            p_ix = int(rows[np.lexsort((rows, d))[0]])          # smallest (d, row index)
            candidates += len(rows)
            x = As[np.array(base)] - q
            p_coh, i_coh = src[int(np.argmin(np.sqrt(np.add.reduce(x * x, axis=1))))]
        else:
            p_ix, _ = O.nn_exact(As, q)
            fallbacks += 1
            p_coh = None
        i_app, rem = divmod(p_ix, A_h * A_w)
        p, i = divmod(rem, A_w), i_app
        if p_coh is not None:
            d_app = O.compute_distance(As[p_ix], q, weights)
            d_coh = O.compute_distance(As[(A_h * i_coh + p_coh[0]) * A_w + p_coh[1]], q, weights)
            if d_coh <= d_app * kf:
                p, i = p_coh, i_coh
        if log is not None:
            log.append(p_ix)
        Bp_pyr[level][r, c] = Ap_pyr_list[i][level][p]
        s[qi] = p
        im[qi] = i
    return s, im, fallbacks, candidates


def run(z, K, min_rows=1, exact=False):
    """Every level of case z, chained: levels with at least min_rows DB rows (and more than one) by
    k-coherence search with min(K, N_A - 1) similar rows, the others - all of them with exact - by the
    oracle's exact level.  Returns dict(s, im, Bp, fallbacks, candidates, kcoh_levels, sim) per level."""
    L = z['L']
    Bp = [x.copy() for x in z['Bp_init']]
    r = dict(s={}, im={}, Bp=Bp, fallbacks={}, candidates={}, kcoh_levels=[], sim={})
    with blas_order():
        for level in range(1, L):
            As = PI.build_db(z, level)
            B_feat = O.feature_array(z['B_pyr'], level, True)
            n = len(As)
            if exact or n < max(2, min_rows):
                r['s'][level], r['im'][level] = O.synthesize_level(None, z['Ap_pyr'], B_feat, Bp, level, L, z['k'],
                                                                   z['weights'], As=As)
                continue
            sim = similarity_sets(As, min(K, n - 1))
            r['s'][level], r['im'][level], r['fallbacks'][level], r['candidates'][level] = synthesize_level(
                z['Ap_pyr'], B_feat, Bp, level, L, z['k'], z['weights'], As, sim)
            r['kcoh_levels'].append(level)
            r['sim'][level] = sim
    return r


# ---- the cases --------------------------------------------------------------------------------------------
def rand_case(seed, geo=MAIN, ch=1, n_ap=1, k=0.5):
    return AI._affine(seed, ident, ident, geo=geo, k=k, ch=ch, n_ap=n_ap)


def const_a(seed=7, geo=MAIN):
    z = rand_case(seed, geo)
    z['A_pyr'] = [np.full_like(x, 0.25) for x in z['A_pyr']]
    z['Ap_pyr'] = [[np.full_like(x, 0.25) for x in p] for p in z['Ap_pyr']]
    return z


def narrow(w):
    """B of width w (1, 2, 3: steps without a pixel, rows of one step apart) and 7 rows"""
    return rand_case(20 + w, dict(a_hw=MAIN['a_hw'], b_hw=(7, w), L=2))


CASES = {
    'main': lambda: rand_case(1),
    'c2': lambda: rand_case(2, ch=2),
    'c3': lambda: rand_case(3, ch=3),
    'ap2': lambda: rand_case(4, n_ap=2),
    'pairs2': lambda: PI._rand_pairs(5, 2, geo=MAIN),
    'w1': lambda: narrow(1),
    'w2': lambda: narrow(2),
    'w3': lambda: narrow(3),
    't11': lambda: rand_case(6, T11, n_ap=3),
    'const': const_a,
    'k0': lambda: rand_case(8, k=0.0),
    'k25': lambda: rand_case(9, k=25.0),
    't44': lambda: rand_case(10, T44),
    't23': lambda: rand_case(11, T23),
    'pyr': lambda: rand_case(12, PYR),
    # a batch on main's A side: their own B sides and kappa
    'main_job1': lambda: AI.with_b_side(rand_case(1), rand_case(13), 5.0),
    'main_job2': lambda: AI.with_b_side(rand_case(1), rand_case(14), 0.0),
}
# (case, K) of the level parity runs; main's four K give 24, 60, 72 and 192 candidate lanes at most
LEVEL_RUNS = [('main', 1), ('main', 4), ('main', 5), ('main', 15), ('c2', 4), ('c3', 4), ('ap2', 4), ('pairs2', 4),
              ('w1', 4), ('w2', 4), ('w3', 4), ('t11', 2), ('const', 4), ('k0', 4), ('k25', 4)]
FULL_K = [('t44', 15), ('t23', 5), ('t11', 2)]   # K = N_A - 1: the exact path


def make(name):
    return CASES[name]()


def n_rows(z, level):
    return len(z['Ap_pyr']) * z['Ap_pyr'][0][level].shape[0] * z['Ap_pyr'][0][level].shape[1]


_RUNS = {}


def expected(name, K, min_rows=1, exact=False):
    """run(make(name), ...) once per process; read-only"""
    key = (name, K, min_rows, exact)
    if key not in _RUNS:
        _RUNS[key] = run(make(name), K, min_rows, exact)
    return _RUNS[key]


# ---- wide32: steps of more than 64 and more than 128 queries ---------------------------------------------------
WIDE32_K = 4
for _v in range(4):
    CASES['wide32_v%d' % _v] = (lambda v: lambda: rand_case(1) if v == 0 else
                                AI.with_b_side(rand_case(1), rand_case(40 + v), AI.WIDE_K[v]))(_v)


def no_base_pixels(s, im, b_hw, a_hw):
    """the pixels (r, c) of a level without a base row, from its final s / im: a pixel reads raster-earlier
    pixels only, and those hold their final sources when it is visited"""
    (h, w), (A_h, A_w) = b_hw, a_hw
    out = []
    for qi in range(h * w):
        r, c = divmod(qi, w)
        found = False
        for rr in range(max(0, r - 2), r + 1):
            for rc in range(max(0, c - 2), min(w, c + 3)):
                ri = rr * w + rc
                if ri < qi and 0 <= s[ri, 0] + r - rr < A_h and 0 <= s[ri, 1] + c - rc < A_w:
                    found = True
        if not found:
            out.append((r, c))
    return out


def step_queries(b_hw, J):
    """{t: {(job, r, c): m}} of the schedule t = col + 3 row with J jobs: k_kcoh_step's query m = job M + (r - r0),
    M the step's pixels and r0 its first row"""
    h, w = b_hw
    out = {}
    for t in range(w + 3 * (h - 1)):
        px = [(r, t - 3 * r) for r in range(h) if 0 <= t - 3 * r < w]
        out[t] = {(j, r, c): j * len(px) + i for j in range(J) for i, (r, c) in enumerate(px)}
    return out

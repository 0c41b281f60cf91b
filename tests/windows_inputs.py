"""Exact levels for window sizes other than 3x3 / 5x5 (include/ia.h ia_synthesize_levels_nbhd, DESIGN.md
section 11): a size-parametrised numpy restatement of oracle.ia_oracle.synthesize_level, and the cases.
Pure numpy, no GPU import.

The fixtures hold no reference run at other sizes and oracle/ is fixed at 3 / 5, so the rule is restated
here with n_sm, n_lg as parameters (p_s = n_sm // 2, p_l = n_lg // 2, n_half = n_lg ** 2 // 2):
  * DB / query row: [n_sm x n_sm at (r // 2, c // 2) of level l - 1 | n_lg x n_lg at (r, c) | the same two of
    the primed image, the fine one cut to its first n_half cells], row-major, channel-minor, symmetric padding;
  * NN: O.nn_exact (fp64 pairwise, first argmin);
  * coherence: rows r - p_l .. r, cols c - p_l .. c + p_l in product order, raster-earlier, shifted source
    inside A, first argmin of sqrt(add.reduce(x * x));
  * kappa rule: O.compute_distance_blas (the explicit BLAS order) with weights(n_sm, n_lg, ch).
tests/test_windows_cpu.py pins it twice: at (3, 5) to the oracle itself, and at other sizes its rows to the
package's compute_feature_array / extract_pixel_feature (written independently).

A case is shaped like tests/adversarial_inputs.py's, with 'weights' of the sizes' width and 'win' =
(n_sm, n_lg).
"""
import numpy as np

import adversarial_inputs as AI
import pairs_inputs as PI
from oracle import ia_oracle as O

N_SM, N_LG, MAX_D = (1, 3, 5), (3, 5, 7, 9), 167
ident = lambda x: x


def width(n_sm, n_lg, ch):
    return ch * (2 * n_sm * n_sm + n_lg * n_lg + (n_lg * n_lg) // 2)


def supported(n_sm, n_lg, ch):
    return n_sm in N_SM and n_lg in N_LG and 1 <= ch <= 3 and width(n_sm, n_lg, ch) <= MAX_D


def weights(n_sm, n_lg, ch):
    """config.py:68-79 for any sizes: [w_sm, w_lg, w_sm, w_half], channel-minor"""
    n_half = (n_lg * n_lg) // 2
    g_sm = np.repeat(O.matlab_style_gauss2D((n_sm, n_sm), 0.5).ravel(), ch)
    g_lg = np.repeat(O.matlab_style_gauss2D((n_lg, n_lg), 1).ravel(), ch)
    return np.hstack([(1. / (n_sm * n_sm)) * g_sm, (1. / (n_lg * n_lg)) * g_lg, (1. / (n_sm * n_sm)) * g_sm,
                      (1. / n_half) * g_lg[:n_half * ch]])


def patch(img, r, c, n, cells=None):
    """n x n patches of the symmetric-padded img at (r, c) (int arrays), flattened row-major / channel-minor,
    cut to the first `cells` cells"""
    s = img if img.ndim == 3 else img[:, :, None]
    h, w = s.shape[:2]
    off = np.arange(n) - n // 2
    rr = O.reflect(r[:, None] + off[None, :], h)
    cc = O.reflect(c[:, None] + off[None, :], w)
    p = s[rr[:, :, None], cc[:, None, :]].reshape(len(r), -1)
    return p if cells is None else p[:, :cells * s.shape[2]]


def feature_array(pyr, level, full, n_sm, n_lg):
    """compute_feature_array (algorithms.py:11-47) of one level >= 1, raster-order rows"""
    h, w = pyr[level].shape[:2]
    r, c = np.divmod(np.arange(h * w), w)
    return np.hstack([patch(pyr[level - 1], r // 2, c // 2, n_sm),
                      patch(pyr[level], r, c, n_lg, None if full else (n_lg * n_lg) // 2)])


def build_db(z, level, n_sm, n_lg):
    A = z.get('A_pairs') or [z['A_pyr']] * len(z['Ap_pyr'])
    return np.vstack([np.hstack([feature_array(a, level, True, n_sm, n_lg), feature_array(p, level, False, n_sm, n_lg)])
                      for a, p in zip(A, z['Ap_pyr'])])


def query_feature(B_feat_l, Bp_sm, Bp_lg, r, c, w, n_sm, n_lg):
    ra, ca = np.array([r]), np.array([c])
    return np.hstack([B_feat_l[r * w + c], patch(Bp_sm, ra // 2, ca // 2, n_sm)[0],
                      patch(Bp_lg, ra, ca, n_lg, (n_lg * n_lg) // 2)[0]])


def coherence(As, A_h, A_w, q, s, im, r, c, w, p_l):
    """best_coherence_match (algorithms.py:92-130) with pad p_l: ((pr, pc), img) or None"""
    cand, src = [], []
    qi = r * w + c
    for rr in range(max(0, r - p_l), r + 1):
        for rc in range(max(0, c - p_l), min(w, c + p_l + 1)):
            ri = rr * w + rc
            if ri >= qi:
                continue
            pr, pc = s[ri, 0] + r - rr, s[ri, 1] + c - rc
            if 0 <= pr < A_h and 0 <= pc < A_w:
                cand.append((A_h * im[ri] + pr) * A_w + pc)
                src.append(((int(pr), int(pc)), int(im[ri])))
    if not cand:
        return None
    x = As[np.array(cand)] - q
    return src[int(np.argmin(np.sqrt(np.add.reduce(x * x, axis=1))))]


def synthesize_level(z, level, n_sm, n_lg, Bp, log=None):
    """One level; Bp[level] is updated in place.  Returns (s, im).  log receives per pixel
    (p_ix, d[p_ix], exact ties, relative gap to the runner-up, None or (d_app, d_coh))."""
    As = build_db(z, level, n_sm, n_lg)
    B_feat = feature_array(z['B_pyr'], level, True, n_sm, n_lg)
    h, w = Bp[level].shape[:2]
    A_h, A_w = z['Ap_pyr'][0][level].shape[:2]
    L, wt = z['L'], z['weights']
    s = np.zeros((h * w, 2), dtype=np.int64)
    im = np.zeros(h * w, dtype=np.int64)
    kf = 1 + (2 ** (level - L)) * z['k']
    for qi in range(h * w):
        r, c = divmod(qi, w)
        q = query_feature(B_feat, Bp[level - 1], Bp[level], r, c, w, n_sm, n_lg)
        p_ix, d = O.nn_exact(As, q)
        i_app, rem = divmod(p_ix, A_h * A_w)
        p, i = divmod(rem, A_w), i_app
        rec = None
        if qi > 0:
            ck = coherence(As, A_h, A_w, q, s, im, r, c, w, n_lg // 2)
            if ck is not None:
                p_coh, i_coh = ck
                d_app = O.compute_distance_blas(As[p_ix], q, wt)
                d_coh = O.compute_distance_blas(As[(A_h * i_coh + p_coh[0]) * A_w + p_coh[1]], q, wt)
                if d_coh <= d_app * kf:
                    p, i = p_coh, i_coh
                rec = (d_app, d_coh)
        if log is not None:
            two = np.partition(d, 1)[:2] if len(d) > 1 else np.array([d[0], np.inf])
            gap = (two[1] - two[0]) / two[0] if two[0] > 0 else (0.0 if two[1] == 0 else np.inf)
            log.append((p_ix, float(d[p_ix]), int((d == d[p_ix]).sum()), float(gap), rec, kf))
        Bp[level][r, c] = z['Ap_pyr'][i][level][p]
        s[qi] = p
        im[qi] = i
    return s, im


def run(z, n_sm=None, n_lg=None):
    """Every level of z, chained.  Returns dict(s, im, Bp, log)."""
    n_sm, n_lg = (n_sm, n_lg) if n_sm else z['win']
    Bp = [x.copy() for x in z['Bp_init']]
    r = dict(s={}, im={}, Bp=Bp, log=[])
    for level in range(1, z['L']):
        r['s'][level], r['im'][level] = synthesize_level(z, level, n_sm, n_lg, Bp, r['log'])
    return r


# ---- the cases --------------------------------------------------------------------------------------------
BASE = AI.BASE                                        # A 25 x 19 / B 16 x 20, three levels
WIDE45 = dict(a_hw=(25, 19), b_hw=(9, 45), L=2)       # (3, 9): min(9, 45 / 5) = 9 queries a step at the widest
WIDE70 = dict(a_hw=(25, 19), b_hw=(17, 70), L=2)      # (3, 7): min(17, ceil(70 / 4)) = 17


def sized(z, n_sm, n_lg):
    """z with the sizes' weights"""
    ch = 1 if z['A_pyr'][-1].ndim == 2 else z['A_pyr'][-1].shape[2]
    assert supported(n_sm, n_lg, ch), (n_sm, n_lg, ch)
    z = dict(z)
    z.update(weights=weights(n_sm, n_lg, ch), win=(n_sm, n_lg))
    return z


def rand_case(seed, n_sm, n_lg, geo=BASE, ch=1, n_ap=1, k=0.5, f=ident):
    return sized(AI._affine(seed, f, f, geo=geo, k=k, ch=ch, n_ap=n_ap), n_sm, n_lg)


def border(seed, b_hw, n_sm, n_lg):
    return rand_case(seed, n_sm, n_lg, geo=dict(a_hw=(12, 10), b_hw=b_hw, L=2))


SIZE_RUNS = [(1, (1, 3)), (1, (3, 3)), (1, (3, 7)), (1, (5, 5)), (1, (5, 7)), (1, (3, 9)), (1, (1, 9)), (3, (3, 3)), (2, (1, 7))]
BORDER_B = [(5, 1), (6, 2), (1, 7), (2, 11)]
BORDER_WIN = [(3, 9), (5, 7)]
EDGE_CASES = ['neartie36', 'constA', 'tiny', 'offset', 'x64edge', 'bigA']

CASES = {}
for _ch, (_s, _l) in SIZE_RUNS:
    CASES['size_c%d_%d_%d' % (_ch, _s, _l)] = (lambda ch, s, l: lambda: rand_case(200 + 10 * s + l + 100 * ch, s, l, ch=ch))(_ch, _s, _l)
for _b in BORDER_B:
    for _w in BORDER_WIN:
        CASES['border_%dx%d_%d_%d' % (_b + _w)] = (lambda b, w: lambda: border(300 + 20 * b[0] + b[1], b, *w))(_b, _w)
for _w in BORDER_WIN:
    CASES['smallA23_%d_%d' % _w] = (lambda w: lambda: rand_case(340, *w, geo=dict(a_hw=(2, 3), b_hw=(6, 5), L=2)))(_w)
    CASES['smallA11_%d_%d' % _w] = (lambda w: lambda: rand_case(341, *w, geo=dict(a_hw=(1, 1), b_hw=(5, 4), L=2), n_ap=3))(_w)
for _n in EDGE_CASES:
    CASES['edge_' + _n] = (lambda n: lambda: sized(AI.make(n), 3, 7))(_n)
# bigA at (3, 9): D = 139, so the 8,280-row DB has 1,150,920 elements and k_nbhd_rows' 4,096 x 256 grid takes a
# second trip for the rows from BIG_CUT on (run after another call on the same context: test_gpu_windows.py)
CASES['edge_bigA_3_9'] = lambda: sized(AI.make('bigA'), 3, 9)
ROWS_GRID = 4096 * 256                                                   # ia_launch_nbhd_rows: workgroups x threads
BIG_CUT = ROWS_GRID // 139                                               # the first DB row with an element past the grid
CASES['x1000'] = lambda: rand_case(350, 3, 7, f=lambda x: 1000 * x)      # far outside the default path's +-64 gate
CASES['pairs2'] = lambda: sized(PI._rand_pairs(351, 2, geo=dict(a_hw=(12, 10), b_hw=(11, 13), L=2)), 3, 7)
WIDE_K = AI.WIDE_K


def _wide(v, geo, win, seed):
    za = rand_case(seed, *win, geo=geo)
    return za if v == 0 else sized(AI.with_b_side(za, AI._affine(seed + v, ident, ident, geo=geo), WIDE_K[v]), *win)


for _v in range(4):
    CASES['wide45_v%d' % _v] = (lambda v: lambda: _wide(v, WIDE45, (3, 9), 360))(_v)
for _v in range(2):
    CASES['wide70_v%d' % _v] = (lambda v: lambda: _wide(v, WIDE70, (3, 7), 370))(_v)
SIZE_CASES = [n for n in CASES if n.startswith('size_')]
BORDER_CASES = [n for n in CASES if n.startswith('border_') or n.startswith('smallA')]


def make(name):
    return CASES[name]()


_RUNS = {}


def expected(name):
    """run(make(name)) once per process; read-only"""
    if name not in _RUNS:
        _RUNS[name] = run(make(name))
    return _RUNS[name]


# ---- the schedule t = col + (pad + 1) row -----------------------------------------------------------------
def steps(h, w, pad):
    """{t: [(r, c)]} by brute force"""
    out = {}
    for r in range(h):
        for c in range(w):
            out.setdefault(c + (pad + 1) * r, []).append((r, c))
    return out


def reads(r, c, h, w, pad):
    """the B' pixels of the level that pixel (r, c) reads: its causal half window under reflection (the first
    n_half cells of the (2 pad + 1)^2 window) and its coherence cells"""
    n = 2 * pad + 1
    out = set()
    for k in range((n * n) // 2):
        rr, cc = int(O.reflect(r + k // n - pad, h)), int(O.reflect(c + k % n - pad, w))
        out.add((rr, cc))
    for rr in range(max(0, r - pad), r + 1):
        for cc in range(max(0, c - pad), min(w, c + pad + 1)):
            if rr * w + cc < r * w + c:
                out.add((rr, cc))
    return out


def step_shape(h, w, pad, J=1):
    """(steps, widest step's queries, query tiles summed over the steps) for J jobs"""
    st = steps(h, w, pad)
    return w + (pad + 1) * (h - 1), max(len(v) for v in st.values()), sum(-(-J * len(v) // 32) for v in st.values())

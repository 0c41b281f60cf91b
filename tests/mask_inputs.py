"""Masked resynthesis (include/ia.h ia_synthesize_levels_masked): a numpy restatement of
the rule, of the step compaction (ia_masked_step_list) and of mask_pyramid, and the cases.  Pure numpy, no GPU
import.

The rule, built on tests/windows_inputs.py's pieces: visit the masked pixels in raster order; each takes
windows_inputs.synthesize_level's per-pixel rule on the current state (the same query row, O.nn_exact, the
kappa rule by O.compute_distance_blas, the same writeback) with one change: a coherence cell is a candidate only
if it is raster-earlier, its im >= 0 and its shifted source lies inside A.  Kept pixels are never written.
tests/test_mask_cpu.py pins it: an all-ones mask without sources is windows_inputs.run (hence the oracle and
the reference's recorded runs at (3, 5)), and a finished run's state is a fixed point of every mask inside rows
and columns >= p_l.
"""
import numpy as np

import windows_inputs as WI
from oracle import ia_oracle as O


def coherence(As, A_h, A_w, q, s, im, r, c, w, p_l):
    """windows_inputs.coherence with the extra condition im >= 0 (a kept pixel without a source is no
    candidate, and its s is not read): ((pr, pc), img) or None"""
    cand, src = [], []
    qi = r * w + c
    for rr in range(max(0, r - p_l), r + 1):
        for rc in range(max(0, c - p_l), min(w, c + p_l + 1)):
            ri = rr * w + rc
            if ri >= qi or im[ri] < 0:
                continue
            pr, pc = s[ri, 0] + r - rr, s[ri, 1] + c - rc
            if 0 <= pr < A_h and 0 <= pc < A_w:
                cand.append((A_h * im[ri] + pr) * A_w + pc)
                src.append(((int(pr), int(pc)), int(im[ri])))
    if not cand:
        return None
    x = As[np.array(cand)] - q
    return src[int(np.argmin(np.sqrt(np.add.reduce(x * x, axis=1))))]


def resynthesize_level(z, level, n_sm, n_lg, Bp, mask, s_in=None, im_in=None, log=None):
    """One level: Bp[level] is updated in place at the masked pixels.  s_in / im_in None: no kept pixel has a
    source.  Returns the complete (s, im), int64.  log receives per masked pixel (qi, None or (d_app, d_coh), kf)."""
    As = WI.build_db(z, level, n_sm, n_lg)
    B_feat = WI.feature_array(z['B_pyr'], level, True, n_sm, n_lg)
    h, w = Bp[level].shape[:2]
    A_h, A_w = z['Ap_pyr'][0][level].shape[:2]
    L, wt = z['L'], z['weights']
    mask = np.asarray(mask).astype(bool)
    assert mask.shape == (h, w)
    s = np.zeros((h * w, 2), dtype=np.int64) if s_in is None else np.array(s_in, dtype=np.int64)
    im = np.full(h * w, -1, dtype=np.int64) if im_in is None else np.array(im_in, dtype=np.int64)
    kf = 1 + (2 ** (level - L)) * z['k']
    for qi in np.flatnonzero(mask.ravel()):
        r, c = divmod(int(qi), w)
        q = WI.query_feature(B_feat, Bp[level - 1], Bp[level], r, c, w, n_sm, n_lg)
        p_ix, _ = O.nn_exact(As, q)
        i, rem = divmod(p_ix, A_h * A_w)
        p = divmod(rem, A_w)
        rec = None
        ck = coherence(As, A_h, A_w, q, s, im, r, c, w, n_lg // 2)
        if ck is not None:
            p_coh, i_coh = ck
            d_app = O.compute_distance_blas(As[p_ix], q, wt)
            d_coh = O.compute_distance_blas(As[(A_h * i_coh + p_coh[0]) * A_w + p_coh[1]], q, wt)
            if d_coh <= d_app * kf:
                p, i = p_coh, i_coh
            rec = (d_app, d_coh)
        if log is not None:
            log.append((int(qi), rec, kf))
        Bp[level][r, c] = z['Ap_pyr'][i][level][p]
        s[qi] = p
        im[qi] = i
    return s, im


def resynthesize(z, Bp, masks, S=None, IM=None, win=None):
    """Every level 1..L-1 of z, chained: Bp (a list of levels: the kept values) is updated in place at
    masks[level]; S / IM: {level: state}, a missing level has no sources.  Returns dict(s, im, Bp, log)."""
    n_sm, n_lg = win or z['win']
    S, IM = S or {}, IM or {}
    r = dict(s={}, im={}, Bp=Bp, log={})
    for level in range(1, z['L']):
        r['log'][level] = []
        r['s'][level], r['im'][level] = resynthesize_level(z, level, n_sm, n_lg, Bp, masks[level], S.get(level), IM.get(level),
                                                          r['log'][level])
    return r


def wins(log):
    """coherence wins of a level's log"""
    return sum(1 for _, rec, kf in log if rec is not None and rec[1] <= rec[0] * kf)


# ---- the step compaction ------------------------------------------------------------------------------------
def step_list(mask, pad):
    """ia_masked_step_list by brute force: (offsets (T + 1,), pixels): step t = col + (pad + 1) row holds
    pixels[offsets[t]:offsets[t + 1]], the masked raster indices of the step, rows ascending"""
    mask = np.asarray(mask).astype(bool)
    h, w = mask.shape
    T = w + (pad + 1) * (h - 1)
    by_step = [[] for _ in range(T)]
    for r in range(h):                                  # rows ascending within every step
        for c in range(w):
            if mask[r, c]:
                by_step[c + (pad + 1) * r].append(r * w + c)
    offsets = np.zeros(T + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(v) for v in by_step])
    return offsets, np.array([q for v in by_step for q in v], dtype=np.int64)


def nonempty_steps(masks, pad):
    """steps of the schedule that hold a masked pixel of at least one of the jobs' masks (one shape)"""
    any_mask = np.any(np.stack([np.asarray(m).astype(bool) for m in masks]), axis=0)
    off, _ = step_list(any_mask, pad)
    return int(np.count_nonzero(np.diff(off)))


# ---- mask_pyramid -------------------------------------------------------------------------------------------
def mask_pyramid(mask, shapes, grow=0):
    """image_analogies.mask_pyramid by loops: the finest level is mask; level l - 1 at (r, c) is the any over
    rows 2r .. 2r + 1, columns 2c .. 2c + 1 of level l, clipped; then every level dilated by a (2 grow + 1) square"""
    L = len(shapes)
    chain = [None] * L
    chain[L - 1] = np.asarray(mask).astype(bool)
    for l in range(L - 1, 0, -1):
        h, w = shapes[l - 1][:2]
        fine = chain[l]
        m = np.zeros((h, w), dtype=bool)
        for r in range(h):
            for c in range(w):
                m[r, c] = fine[2 * r:2 * r + 2, 2 * c:2 * c + 2].any()
        chain[l - 1] = m
    out = []
    for m in chain:
        h, w = m.shape
        d = np.zeros_like(m)
        for r in range(h):
            for c in range(w):
                d[r, c] = m[max(0, r - grow):r + grow + 1, max(0, c - grow):c + grow + 1].any()
        out.append(d)
    return out


# ---- the cases ----------------------------------------------------------------------------------------------
def base(win, seed=400, **kw):
    """windows_inputs' small shape (A 25 x 19 / B 16 x 20 over three levels) at sizes win"""
    return WI.rand_case(seed + 10 * win[0] + win[1], win[0], win[1], **kw)


def shapes(z):
    return [x.shape[:2] for x in z['B_pyr'][:z['L']]]


def full_masks(z):
    return {l: np.ones(s, dtype=bool) for l, s in enumerate(shapes(z))}


def level_masks(z, p_l, kind):
    """interior_masks' mask `kind` for every synthesised level of z (1 .. L - 1)"""
    return {l: interior_masks(s, p_l)[kind] for l, s in enumerate(shapes(z)) if l >= 1}


def interior_masks(shape, p_l, seed=7):
    """the idempotence masks of one level, all inside rows / columns >= p_l: an interior rectangle, one pixel,
    a checkerboard, a random 30 %, the level's last pixel alone"""
    h, w = shape
    rs = np.random.RandomState(seed)
    inner = np.zeros((h, w), dtype=bool)
    inner[p_l:, p_l:] = True
    rect = np.zeros((h, w), dtype=bool)
    rect[p_l + 1:max(p_l + 2, h - 2), p_l + 2:max(p_l + 3, w - 3)] = True
    one = np.zeros((h, w), dtype=bool)
    one[h // 2, w // 2] = True
    rr, cc = np.divmod(np.arange(h * w), w)
    checker = ((rr + cc) % 2 == 0).reshape(h, w) & inner
    rand = (rs.rand(h, w) < 0.3) & inner
    last = np.zeros((h, w), dtype=bool)
    last[h - 1, w - 1] = True
    out = dict(rect=rect, one=one, checker=checker, rand30=rand, last=last)
    assert all(m.any() and not (m & ~inner).any() for m in out.values())
    return out


def edited(z, rect=(5, 11, 6, 14), seed=9, grow=1):
    """case 3: z with its B pyramid changed inside a rectangle of the finest level (rows r0 .. r1 - 1, columns
    c0 .. c1 - 1) and inside that rectangle's mask_pyramid(grow = 0) cells of the coarser levels.  Returns
    (z1, masks): masks = mask_pyramid(., grow) as a list by level"""
    r0, r1, c0, c1 = rect
    shp = shapes(z)
    m = np.zeros(shp[-1], dtype=bool)
    m[r0:r1, c0:c1] = True
    exact = mask_pyramid(m, shp, 0)
    rs = np.random.RandomState(seed)
    z1 = dict(z)
    z1['B_pyr'] = [np.where(exact[l] if b.ndim == 2 else exact[l][:, :, None], rs.rand(*b.shape), b)
                   for l, b in enumerate(z['B_pyr'][:z['L']])]
    return z1, mask_pyramid(m, shp, grow)


# ---- tall: more than 256 steps, and a step of more than 64 rows ------------------------------------------------
TALL_WIN = (3, 5)
TALL_GEO = dict(a_hw=(25, 19), b_hw=(66, 200), L=2)
TALL_T = 200 + 3 * 65            # 395 steps: k_mask_scan's 256 threads take per = 2 steps each
TALL_LINE_STEP = 197             # the step of the pixels (r, 197 - 3 r), r = 0 .. 65: all 66 rows
TALL_MASKS = ('line', 'sparse', 'both')
_TALL = {}


def tall():
    """The case and its kept state, once per process, read-only: dict(z, Bp, s, im, masks).  The state is no
    finished run (the call's contract takes any valid one): a seeded random source map inside A, im = 0 except
    about 5 % of the pixels without a source (im = -1), B' = A' at the source and the initial B' where there is
    none.  masks: 'line' (one step of 66 queries), 'sparse' (a seeded 2 % of the pixels), 'both' (their union)"""
    if not _TALL:
        z = WI.rand_case(450, *TALL_WIN, geo=TALL_GEO)
        h, w = TALL_GEO['b_hw']
        a_h, a_w = TALL_GEO['a_hw']
        rs = np.random.RandomState(451)
        s = np.stack([rs.randint(0, a_h, h * w), rs.randint(0, a_w, h * w)], axis=1).astype(np.int64)
        im = np.where(rs.rand(h * w) < 0.05, -1, 0).astype(np.int64)
        Bp = [x.copy() for x in z['Bp_init']]
        Bp[1] = np.where(im.reshape(h, w) >= 0, z['Ap_pyr'][0][1][s[:, 0], s[:, 1]].reshape(h, w), z['Bp_init'][1])
        line = np.zeros((h, w), dtype=bool)
        line[np.arange(h), TALL_LINE_STEP - 3 * np.arange(h)] = True
        sparse = rs.rand(h, w) < 0.02
        for x in (s, im, line, sparse, *Bp):
            x.setflags(write=False)
        _TALL.update(z=z, Bp=Bp, s=s, im=im, masks=dict(line=line, sparse=sparse, both=line | sparse))
    return _TALL


_TALL_RUNS = {}


def tall_expected(kind):
    """resynthesize() of tall's state under mask `kind`, once per process; read-only"""
    if kind not in _TALL_RUNS:
        t = tall()
        _TALL_RUNS[kind] = resynthesize(t['z'], [x.copy() for x in t['Bp']], {1: t['masks'][kind]}, {1: t['s']}, {1: t['im']})
    return _TALL_RUNS[kind]


def scan_shares(T, threads=256):
    """k_mask_scan's split of the T step counts: (per, [(a, b)] per thread), thread i sums offsets[a:b]"""
    per = -(-T // threads)
    return per, [(min(T, i * per), min(T, min(T, i * per) + per)) for i in range(threads)]

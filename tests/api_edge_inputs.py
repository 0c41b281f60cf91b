"""Edge and size cases for the half of the C ABI off the level path (pure numpy / scipy, no GPU
import): ia_index_build / ia_index_query, ia_coherence_batch, ia_gaussian_pyramid and
ia_color_matrix; with the plain references tests/test_gpu_api_edges.py compares them with bit for
bit.  Every generator is deterministic (np.random.RandomState) and
tests/test_api_edge_inputs_cpu.py pins, without a GPU, that each case is what it claims to be.

References:
  index       numpy fp64 ((pts - q) ** 2).sum(axis=1), first argmin and its value, per query
              (tests/test_gpu_adversarial.py _check_index restated so that it returns the arrays)
  coherence   oracle.ia_oracle.coherence per pixel; coherence_pad restates it with the window's
              pad as a parameter (pinned equal to the oracle's at pad = 2)
  pyramid     ia_amd.img_preprocess._pyramid_reduce applied n_reduce times; reduce_variant
              restates it with the clip global (pinned equal), per channel or absent
  colour      np.einsum('ij,klj->kli', M, img)
"""
import numpy as np
from scipy import ndimage as ndi

from oracle import ia_oracle as O

TILE = 32          # IA_TILE
WG_TARGET = 512    # IA_WG_TARGET
BATCH = 4096       # ia_index_query's batch
PY_THREADS = 4096 * 256   # py_grid's cap: 4,096 workgroups of 256 threads
REL_TIE = 2.0 ** -20      # tests/adversarial_inputs.py REL_TIE


# ---- the exact index ---------------------------------------------------------------------------
def index_geometry(n, d=55):
    """(n_tiles, tpw, nwg, tiles of the last chunk, rows of the last tile, KH, query tiles of one scan launch) of
    ia_index_build / ia_index_query (ia_index.cpp), restated"""
    n_tiles = -(-n // TILE)
    tpw = max(4, -(-n_tiles // WG_TARGET))
    nwg = -(-n_tiles // tpw)
    kh = 28 if d + 1 <= 56 else 56 if d + 1 <= 112 else 84
    return dict(n_tiles=n_tiles, tpw=tpw, nwg=nwg, last_chunk=n_tiles - (nwg - 1) * tpw,
                last_rows=n - (n_tiles - 1) * TILE, KH=kh, qtmax={28: 11, 56: 5, 84: 3}[kh])


def query_blocks(nq, d):
    """query tiles of each scan launch of every batch of an nq-row query"""
    qtmax = index_geometry(1, d)['qtmax']
    out = []
    for b0 in range(0, nq, BATCH):
        qtt = -(-min(BATCH, nq - b0) // TILE)
        out.append([min(qtmax, qtt - t) for t in range(0, qtt, qtmax)])
    return out


def index_reference(pts, q):
    """(argmin, distance) per query of ((pts - q) ** 2).sum(axis=1), numpy fp64"""
    q = np.atleast_2d(q)
    idx = np.empty(len(q), dtype=np.int64)
    dist = np.empty(len(q), dtype=np.float64)
    for j in range(len(q)):
        dd = ((pts - q[j]) ** 2).sum(axis=1)
        idx[j] = int(np.argmin(dd))
        dist[j] = dd[idx[j]]
    return idx, dist


def _half_hits(pts, q):
    h = min(len(q), len(pts)) // 2
    q[:h] = pts[:h]   # exact hits (distance 0), as tests/test_gpu_adversarial.py does
    return pts, q


def _rand_index(seed, n, d, nq):
    rs = np.random.RandomState(seed)
    return _half_hits(rs.rand(n, d), rs.rand(nq, d))


NEARTIE_BASES, NEARTIE_COPIES, NEARTIE_EXTRA, NEARTIE_NQ = 1750, 40, 5, 64


def _neartie_index():
    """1,750 base rows x 40 copies, each copy with its own 2^-30 rand, + 5 rows, shuffled: 70,005
    rows; a query is a base + 1e-3 rand, so its 40 nearest rows differ by a relative ~2^-30"""
    rs = np.random.RandomState(23)
    base = rs.rand(NEARTIE_BASES, 55)
    pts = np.vstack([base] * NEARTIE_COPIES + [rs.rand(NEARTIE_EXTRA, 55)])
    pts[:NEARTIE_BASES * NEARTIE_COPIES] += 2.0 ** -30 * rs.rand(NEARTIE_BASES * NEARTIE_COPIES, 55)
    rs.shuffle(pts)
    q = base[:NEARTIE_NQ] + 1e-3 * rs.rand(NEARTIE_NQ, 55)
    return pts, q


# name -> () -> (pts, q).  Chunk shapes: d = 55, 64 queries; query loops: 700 (or 100) rows
INDEX_CASES = {
    'n10000': lambda: _rand_index(1, 10000, 55, 64),
    'n65536': lambda: _rand_index(2, 65536, 55, 64),
    'n70005': lambda: _rand_index(3, 70005, 55, 64),
    'n70005_neartie': _neartie_index,
    'nq4096': lambda: _rand_index(4, 100, 8, 4096),
    'nq4097': lambda: _rand_index(5, 100, 8, 4097),
    'nq8200': lambda: _rand_index(6, 100, 8, 8200),
    'd55_nq353': lambda: _rand_index(7, 700, 55, 353),
    'd56_nq161': lambda: _rand_index(8, 700, 56, 161),
    'd111_nq200': lambda: _rand_index(9, 700, 111, 200),
    'd112_nq97': lambda: _rand_index(10, 700, 112, 97),
}
REUSE_NQ = (4200, 3, 400)


def reuse_index():
    """one index (700 x 55) and the three queries it answers in turn"""
    rs = np.random.RandomState(11)
    pts = rs.rand(700, 55)
    return pts, [_half_hits(pts, rs.rand(nq, 55))[1] for nq in REUSE_NQ]


# 2^-70 / 2^-80: squares are fp32 subnormals / zero; 2^62: (float)norm just below FLT_MAX; 2^70: every
# norm past it; 2^63 / 2^64: the squared norms of 'signed' (|a'|^2 ~ 4.6 * 4^k against FLT_MAX = 2^128)
# cross FLT_MAX for most rows but not all, and the products of 'offset1000' stay finite
RANGE_LOG2 = (-70, -80, 62, 63, 64, 70)
RANGE_FAMILIES = ('signed', 'offset1000')


def range_index(family, log2_scale=0):
    """700 x 55 points and 40 queries (half exact hits), scaled by 2^log2_scale (exact in fp64)"""
    rs = np.random.RandomState(12 + RANGE_FAMILIES.index(family))
    if family == 'signed':
        pts, q = rs.rand(700, 55) - 0.5, rs.rand(40, 55) - 0.5
    else:
        pts, q = 1000 + 1e-3 * rs.rand(700, 55), 1000 + 1e-3 * rs.rand(40, 55)
    pts, q = _half_hits(pts, q)
    return pts * 2.0 ** log2_scale, q * 2.0 ** log2_scale


# ---- ia_coherence_batch ------------------------------------------------------------------------
def coherence_pad(As, A_h, A_w, q, s, im, r, c, w, pad=2, trace=None):
    """oracle.ia_oracle.coherence with the window's pad as a parameter (its two range bounds).
    trace: a dict that receives the candidates' cells, DB rows, sums of squares and the cells
    dropped because their shifted source leaves A ('dropped': (cell, pr, pc))."""
    cand, src = [], []
    dropped = []
    qi = r * w + c
    for rr in range(max(0, r - pad), r + 1):
        for rc in range(max(0, c - pad), min(w, c + pad + 1)):
            ri = rr * w + rc
            if ri >= qi:
                continue
            pr, pc = s[ri, 0] + r - rr, s[ri, 1] + c - rc
            if 0 <= pr < A_h and 0 <= pc < A_w:
                cand.append(((A_h * im[ri] + pr) * A_w + pc))
                src.append(((pr, pc), int(im[ri]), (rr, rc)))
            else:
                dropped.append(((rr, rc), int(pr), int(pc)))
    if trace is not None:
        trace['dropped'] = dropped
        trace['cells'] = [x[2] for x in src]
        trace['rows'] = [int(x) for x in cand]
    if not cand:
        return (-1, -1), 0, (0, 0)
    x = As[np.array(cand)] - q
    sums = np.add.reduce(x * x, axis=1)
    if trace is not None:
        trace['sums'] = sums
    k = int(np.argmin(np.sqrt(sums)))
    return src[k]


def coherence_reference(z, pad=2, oracle=False):
    """(p (nq, 2), img (nq,), r_star (nq, 2)) of every pixel of the case, raster order; oracle =
    True: from oracle.ia_oracle.coherence itself (pad 2 only)"""
    (a_h, a_w), (b_h, b_w) = z['a_hw'], z['b_hw']
    p, img, rs = [], [], []
    for qi in range(b_h * b_w):
        r, c = divmod(qi, b_w)
        if oracle:
            got = O.coherence(z['pts'], a_h, a_w, z['q'][qi], z['s'], z['im'], r, c, b_w)
        else:
            got = coherence_pad(z['pts'], a_h, a_w, z['q'][qi], z['s'], z['im'], r, c, b_w, pad)
        p.append(got[0])
        img.append(got[1])
        rs.append(got[2])
    return np.array(p, dtype=np.int32), np.array(img, dtype=np.int32), np.array(rs, dtype=np.int32)


def _coherence_case(seed, a_hw, b_hw, n_ap, d, pts=None, s_row_lo=0):
    """random rows, queries and source map: s uniform over A (rows from s_row_lo: a causal window only adds
    to a source's row, so a candidate can leave A above it only from a source above A), im over n_ap"""
    rs = np.random.RandomState(seed)
    n = n_ap * a_hw[0] * a_hw[1]
    nq = b_hw[0] * b_hw[1]
    z = dict(a_hw=a_hw, b_hw=b_hw, n_ap=n_ap, d=d)
    z['pts'] = rs.rand(n, d) if pts is None else pts(rs, n, d)
    z['q'] = rs.rand(nq, d)
    z['s'] = np.stack([rs.randint(s_row_lo, a_hw[0], nq), rs.randint(0, a_hw[1], nq)], axis=1).astype(np.int32)
    z['im'] = rs.randint(0, n_ap, nq).astype(np.int32)
    z['px'] = np.stack(np.divmod(np.arange(nq), b_hw[1]), axis=1).astype(np.int32)
    return z


def _no_candidate_at_pixel_1(z):
    """pixel (0, 1)'s only causal cell is (0, 0); from A's last column its shifted source leaves A"""
    z['s'][0] = (0, z['a_hw'][1] - 1)
    return z


def _root_collapse_pairs(rs, d, count):
    """count (x, y, q): rows x, y equal but for one ulp in one column, with sum((x - q)^2) >
    sum((y - q)^2) in numpy's summation and equal square roots; q = y + 0.05 rand"""
    out = []
    while len(out) < count:
        y = rs.rand(d)
        q = y + 0.05 * rs.rand(d)
        col = rs.randint(d)
        for toward in (2.0, -1.0):
            x = y.copy()
            x[col] = np.nextafter(y[col], toward)
            sx, sy = (np.add.reduce((np.stack([x, y]) - q) ** 2, axis=1))
            if sx > sy and np.sqrt(sx) == np.sqrt(sy):
                out.append((x, y, q))
                break
    return out


ROOT_PIXELS = [(r, c) for r in (3, 8, 13) for c in (3, 8, 13)]   # 9 planted pixels of a 16 x 20 B'


def _root_collapse_case(seed, d):
    """A 25 x 19, B' 16 x 20: at each ROOT_PIXELS pixel (r, c) the cell (r-1, c-1) leads to row x and
    the later cell (r-1, c) to row y of a root-collapse pair; every other candidate is a random row
    (squared distance ~ d / 6 against the pair's ~ d * 0.05^2 / 3)"""
    z = _coherence_case(seed, (25, 19), (16, 20), 1, d)
    rs = np.random.RandomState(seed + 1000)
    a_w, b_w = z['a_hw'][1], z['b_hw'][1]
    z['planted'] = []
    for k, ((r, c), (x, y, q)) in enumerate(zip(ROOT_PIXELS, _root_collapse_pairs(rs, d, len(ROOT_PIXELS)))):
        tx, ty = (5, 1 + 2 * k), (10, 1 + 2 * k)          # A pixels of x and y
        z['pts'][tx[0] * a_w + tx[1]] = x
        z['pts'][ty[0] * a_w + ty[1]] = y
        z['q'][r * b_w + c] = q
        z['s'][(r - 1) * b_w + c - 1] = (tx[0] - 1, tx[1] - 1)   # s[r'] + (q - r') = tx
        z['s'][(r - 1) * b_w + c] = (ty[0] - 1, ty[1])
        z['planted'].append(dict(px=(r, c), cell_x=(r - 1, c - 1), cell_y=(r - 1, c), row_x=tx[0] * a_w + tx[1],
                                 row_y=ty[0] * a_w + ty[1]))
    return z


COHERENCE_CASES = {
    'A9x7_d55': lambda: _no_candidate_at_pixel_1(_coherence_case(31, (9, 7), (16, 20), 1, 55, s_row_lo=-2)),
    'A25x19_ap2_d110': lambda: _coherence_case(32, (25, 19), (16, 20), 2, 110),
    'A25x19_ap2_d165': lambda: _coherence_case(33, (25, 19), (16, 20), 2, 165),
    'A5x40_B12x9_d55': lambda: _coherence_case(34, (5, 40), (12, 9), 1, 55),
    # exact distance ties: every row equal / rows drawn from 4 distinct ones
    'ties_all_equal': lambda: _coherence_case(35, (9, 7), (16, 20), 1, 55,
                                              pts=lambda rs, n, d: np.tile(rs.rand(1, d), (n, 1))),
    'ties_4_rows': lambda: _coherence_case(36, (9, 7), (16, 20), 1, 55,
                                           pts=lambda rs, n, d: rs.rand(4, d)[rs.randint(0, 4, n)]),
    'root_collapse_d55': lambda: _root_collapse_case(37, 55),
    'root_collapse_d165': lambda: _root_collapse_case(38, 165),
}
PAD_CASE = 'A9x7_d55'   # the first random case: pad = 0, 1, 3, 4 run on it


# ---- GPU preprocessing -------------------------------------------------------------------------
def reduce_variant(img, clip='global'):
    """ia_amd.img_preprocess._pyramid_reduce restated, with the final clip to the smoothed level's
    range 'global' (as the package and skimage do: img.min() / img.max() over all channels),
    'channel' (per channel) or 'none'"""
    sigma = 2 * 2 / 6.0
    sm = ndi.gaussian_filter(img, (sigma, sigma, 0) if img.ndim == 3 else sigma, mode='reflect')
    h, w = sm.shape[:2]
    out_h, out_w = -(-h // 2), -(-w // 2)
    rr = (h / float(out_h)) * (np.arange(out_h) + 0.5) - 0.5
    cc = (w / float(out_w)) * (np.arange(out_w) + 0.5) - 0.5
    r0, c0 = np.floor(rr).astype(int), np.floor(cc).astype(int)
    r1, c1 = np.ceil(rr).astype(int), np.ceil(cc).astype(int)
    dr, dc = rr - r0, cc - c0
    if sm.ndim == 3:
        dr, dc = dr[:, None, None], dc[None, :, None]
    else:
        dr, dc = dr[:, None], dc[None, :]
    tl, tr = sm[r0][:, c0], sm[r0][:, c1]
    bl, br = sm[r1][:, c0], sm[r1][:, c1]
    top = (1 - dc) * tl + dc * tr
    bottom = (1 - dc) * bl + dc * br
    v = (1 - dr) * top + dr * bottom
    if clip == 'none':
        return v, sm
    if clip == 'channel':
        return np.clip(v, sm.min(axis=(0, 1)), sm.max(axis=(0, 1))), sm
    return np.clip(v, sm.min(), sm.max()), sm


def pyramid_reference(img, n_reduce):
    """the n_reduce successive _pyramid_reduce levels of img, finest first (the host loop of
    compute_gaussian_pyramid stops at a 1 x 1 level; the C entry does not, so neither does this)"""
    from ia_amd import img_preprocess as ip
    out, cur = [], np.asarray(img, dtype=np.float64)
    for _ in range(n_reduce):
        cur = ip._pyramid_reduce(cur)
        out.append(cur)
    return out


SMALL_SHAPES = [(1, 1), (1, 2), (2, 1), (1, 7), (7, 1), (2, 7), (5, 1), (3, 3), (3, 2, 3), (1, 1, 3), (4, 5, 2),
                (6, 6, 4)]
# more than PY_THREADS values: in k_gauss1d / k_minmax for all three, in k_bilinear_half only for the
# last (its level-1 output is 1025 x 1026 = 1,051,650 values; the others' outputs are a quarter of the input)
LARGE_SHAPES = [(1025, 1031), (600, 601, 3), (2049, 2051)]
LARGE_REDUCE = {(1025, 1031): 2, (600, 601, 3): 2, (2049, 2051): 1}
COLOR_LARGE = (700, 600, 3)


def small_image(shape):
    return np.random.RandomState(41 + SMALL_SHAPES.index(shape)).rand(*shape)


def large_image(shape):
    return np.random.RandomState(61 + LARGE_SHAPES.index(shape)).rand(*shape)


def _plateau(seed, shape, sign):
    """0.8 rand with a block of 0.83, the level's maximum (negated: -0.83, its minimum)"""
    img = 0.8 * np.random.RandomState(seed).rand(*shape)
    h, w = shape[:2]
    img[4:h - 6, 5:w - 4] = 0.83
    return sign * img


def _disjoint_channels(seed):
    """37 x 51 x 3, channel k in [k, k + 0.8] with a plateau at k + 0.83: the interpolation of a
    channel's plateau can round past that channel's range but never past the global one"""
    img = _plateau(seed, (37, 51, 3), 1.0)
    return img + np.arange(3.0)


CLIP_ENGAGED = ['plateau_37x51', 'plateau_45x45', 'plateau_37x51x3', 'neg_plateau_37x51', 'neg_plateau_45x45',
                'neg_plateau_37x51x3']
CLIP_CASES = {
    'plateau_37x51': lambda: _plateau(71, (37, 51), 1.0),
    'plateau_45x45': lambda: _plateau(72, (45, 45), 1.0),
    'plateau_37x51x3': lambda: _plateau(73, (37, 51, 3), 1.0),
    'neg_plateau_37x51': lambda: _plateau(71, (37, 51), -1.0),
    'neg_plateau_45x45': lambda: _plateau(72, (45, 45), -1.0),
    'neg_plateau_37x51x3': lambda: _plateau(73, (37, 51, 3), -1.0),
    'constant_0p7': lambda: np.full((37, 51), 0.7),
    'range_1e6': lambda: 2e6 * np.random.RandomState(74).rand(37, 51) - 1e6,
    'tiny_2m14': lambda: 2.0 ** -14 * np.random.RandomState(75).rand(37, 51),
    'disjoint_channels': lambda: _disjoint_channels(76),
    'ch2_33x47': lambda: np.random.RandomState(77).rand(33, 47, 2),
    'ch4_33x47': lambda: np.random.RandomState(78).rand(33, 47, 4),
}
DEVICE_SHAPE, DEVICE_REDUCE = (117, 180, 3), 3


def device_image():
    return np.random.RandomState(81).rand(*DEVICE_SHAPE)


def color_inputs(shape=(33, 47, 3)):
    """a random signed matrix and an image in [-5, 5]"""
    rs = np.random.RandomState(91 + shape[0])
    return rs.rand(3, 3) * 4 - 2, rs.rand(*shape) * 10 - 5


def color_reference(M, img):
    return np.einsum('ij,klj->kli', M, img)

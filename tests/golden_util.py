"""Helpers to read the golden end-to-end fixtures written by oracle/gen_golden.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
E2E_CASES = ['g32', 'g24k5', 'rect', 'g64', 'yiq', 'remap', 'rgb3', 'multiap', 'noinit', 'ties']
# round-2 reference runs at larger sizes (oracle/gen_golden.py big_cases; 'lean' fixtures):
# cfg1 = BASELINE config 1's 117x180 YIQ stand-in, g128 / g256 = the bench generator,
# ties128 = piecewise-constant (duplicate DB rows), k25 = kappa 25
BIG_CASES = [c for c in ['cfg1', 'g128', 'ties128', 'k25', 'g256']
             if os.path.exists(os.path.join(GOLDEN, 'e2e_%s.npz' % c))]


def load_e2e(name):
    z = np.load(os.path.join(GOLDEN, 'e2e_%s.npz' % name))
    L = int(z['L'])
    nap = z['Ap'].shape[0]
    nB = len([k for k in z.keys() if k.startswith('Bp0_')])
    d = {k: z[k] for k in z.keys()}
    d['L'] = L
    d['A_pyr'] = [z['A_%d' % l] for l in range(L)]
    d['Ap_pyr'] = [[z['Ap%d_%d' % (j, l)] for l in range(L)] for j in range(nap)]
    d['B_pyr'] = [z['B_%d' % l] for l in range(nB)]
    d['Bp_init'] = [z['Bp0_%d' % l] for l in range(nB)]
    d['Bp_final'] = [z['Bp_%d' % l] for l in range(nB)]
    d['s'] = {l: z['s_%d' % l].astype(np.int64) for l in range(1, L)}
    d['im'] = {l: z['im_%d' % l].astype(np.int64) for l in range(1, L)}
    d['app_ix'] = z['app_ix'].astype(np.int64)
    d['coh'] = z['coh'].astype(np.int64)
    return d


def check_debug_records(z, out, Bp, st, name='', kappa_equalities=False):
    """The assertions of tests/test_gpu_debug.py on one run of every level with debug records:
    out[level] = (s, im, dbg), Bp = the synthesised pyramid, st = the run's Stats.  s, im and B' of
    every level, every NN index ('app_ix'), every coherence pick ('coh', (-1, -1, 0) for "no
    candidate") and every compute_distance value ('dist', d_app then d_coh) must equal the
    reference's, bit for bit.  kappa_equalities: the case compares equal distances under kappa = 0
    (tests/test_gpu_adversarial.py 'k0'), the one input on which kappa_ambiguous is not pinned."""
    assert st.bound_violations == 0 and (kappa_equalities or st.kappa_ambiguous == 0)
    app, coh, dist = [], [], []
    for level in range(1, z['L']):
        s, im, dbg = out[level]
        assert np.array_equal(s, z['s'][level]) and np.array_equal(im, z['im'][level])
        assert np.array_equal(Bp[level], z['Bp_final'][level])
        src, d = dbg['src'], dbg['dist']
        a_h, a_w = z['A_pyr'][level].shape[:2]
        h, w = z['B_pyr'][level].shape[:2]
        app.extend((src[:, 2].astype(np.int64) * a_h + src[:, 0]) * a_w + src[:, 1])
        for qi in range(1, h * w):
            if src[qi, 5]:
                nb = src[qi, 3] * w + src[qi, 4]
                r, c = divmod(qi, w)
                coh.append((s[nb, 0] + r - src[qi, 3], s[nb, 1] + c - src[qi, 4], im[nb]))
                dist.extend(d[qi])
            else:
                assert src[qi, 3] == 0 and src[qi, 4] == 0 and d[qi, 0] == 0 and d[qi, 1] == 0
                coh.append((-1, -1, 0))
        assert src[0, 5] == 0   # the level's first pixel never consults coherence (:186-189)
    assert np.array_equal(np.array(app), z['app_ix'])
    assert np.array_equal(np.array(coh), z['coh'])
    dist = np.array(dist)
    assert dist.shape == z['dist'].shape
    print('%s: %d of %d compute_distance values bit-identical' % (name, int((dist == z['dist']).sum()), dist.size))
    assert np.array_equal(dist, z['dist'])


# library defaults of include/ia.h (ia_set_option has no getter: tests restore these by name)
PRUNE_MIN_ROWS_DEFAULT = 1 << 19


# query tiles one scan launch takes (a wider step runs in blocks), by matcher and channel count:
# the split-f16 scan's ia_k3h_qtmax(KS) with KS = ia_ks_for(ch) = 4 / 7, the fp32 scan's
# ia_k3_qtmax(KH) with KH = 28 / 56 / 84 (image-analogies-python_amd/csrc/ia_k3.hip).  3 channels
# have no split-f16 instance (ia_ks_for(3) = 0): either matcher setting runs the fp32 scan.
QTMAX = {('f16x3', 1): 11, ('f16x3', 2): 8, ('f16x3', 3): 3, ('f32', 1): 11, ('f32', 2): 5, ('f32', 3): 3}


def scan_counts(z, J, matcher='f16x3'):
    """What the scan launch counters of one run over every level of fixture z with J batched jobs
    must add up to, per level: n = DB tiles of 32 rows, steps = the wavefront steps that hold a
    query, qtt / nqb = their query tiles and query blocks (QTMAX tiles per block, for the scan the
    matcher - 'f16x3' or 'f32' - and z's channel count select) summed over those steps.  Every scan
    path visits each (DB tile, query tile) pair and each (DB tile, query block) once per step, so
    dist_pairs_full = sum n qtt and dist_tiles_full = sum n nqb whatever kernel runs; only the
    launch count tells the paths apart (one per block, or one per step and shard)."""
    from ia_amd import _native
    out = []
    for level in range(1, z['L']):
        a_h, a_w = z['A_pyr'][level].shape[:2]
        h, w = z['B_pyr'][level].shape[:2]
        qtmax = QTMAX[matcher, 1 if z['A_pyr'][level].ndim == 2 else z['A_pyr'][level].shape[2]]
        T, _ = _native.wavefront_shape(h, w)
        M = [m for m in (_native.wavefront_step(h, w, t)[1] for t in range(T)) if m > 0]
        qtt = [-(-J * m // 32) for m in M]
        out.append(dict(n=-(-len(z['Ap_pyr']) * a_h * a_w // 32), steps=len(M), qtt=sum(qtt),
                        nqb=sum(-(-q // qtmax) for q in qtt)))
    return out


def sharded_scan_launches(z, J, W):
    """dist_launches of a run whose steps each take one scan launch per shard: W on the levels
    that shard (>= 64 DB tiles per shard), 1 on those that replicate."""
    return sum(c['steps'] * (W if c['n'] >= 64 * W else 1) for c in scan_counts(z, J))

# round 6: reference run at BASELINE config 2's shape (512^2, the finest 5 levels), the size at
# which the product's default path prunes; 'slim' fixture (oracle/gen_golden.py run_case slim=True)
SLIM_CASES = [c for c in ['g512', 'g64slim'] if os.path.exists(os.path.join(GOLDEN, 'e2e_%s.npz' % c))]


def sha1_f64(x):
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()


def load_slim(name):
    """A slim fixture: the reference's pyramids, s / im of every level, and the sha1 of every B'
    initialisation / final B' level.  Bp_init is rebuilt with the product's seeded
    initialize_Bp and checked against the reference's hashes here."""
    from ia_amd.img_preprocess import initialize_Bp
    z = np.load(os.path.join(GOLDEN, 'e2e_%s.npz' % name))
    L = int(z['L'])
    nap = int(z['n_ap'])
    d = {'L': L, 'k': float(z['k']), 'weights': z['weights']}
    d['A_pyr'] = [z['A_%d' % l] for l in range(L)]
    d['Ap_pyr'] = [[z['Ap%d_%d' % (j, l)] for l in range(L)] for j in range(nap)]
    d['B_pyr'] = [z['B_%d' % l] for l in range(L)]
    d['sha1'] = dict(zip([str(k) for k in z['sha1_keys']], [str(v) for v in z['sha1_vals']]))
    d['Bp_init'] = initialize_Bp(d['B_pyr'], init_rand=True, seed=int(z['seed']))
    for l in range(L):
        assert sha1_f64(d['Bp_init'][l]) == d['sha1']['Bp0_%d' % l], 'B\' init of level %d differs' % l
    d['s'] = {l: z['s_%d' % l].astype(np.int64) for l in range(1, L)}
    d['im'] = {l: z['im_%d' % l].astype(np.int64) for l in range(1, L)}
    return d

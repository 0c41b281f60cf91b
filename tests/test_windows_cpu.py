"""Window sizes other than 3x3 / 5x5 without a GPU (include/ia.h ia_synthesize_levels_nbhd, DESIGN.md
section 11): the restatement of tests/windows_inputs.py pinned to the oracle and to the package's own
feature rows, the schedule t = col + (pad + 1) row against a brute force, config.set_windows /
image_analogies.level_windows, and that every case of tests/test_gpu_windows.py is what it claims to be."""
import types

import numpy as np
import pytest

import adversarial_inputs as AI
import kcoh_inputs as KI
import windows_inputs as WI
from oracle import ia_oracle as O


# ---- the restatement at (3, 5) is the oracle ---------------------------------------------------------------
@pytest.mark.parametrize('which', ['base', 'main'])
def test_restatement_at_3_5_equals_the_oracle(which):
    z = AI._affine(1, WI.ident, WI.ident) if which == 'base' else KI.rand_case(1)
    assert np.array_equal(WI.weights(3, 5, 1), z['weights'])
    o = AI.run_oracle(z)
    e = WI.run(z, 3, 5)
    for level in range(1, z['L']):
        assert np.array_equal(e['s'][level], o['s'][level]) and np.array_equal(e['im'][level], o['im'][level])
        assert np.array_equal(e['Bp'][level], o['Bp_final'][level])
        assert np.array_equal(WI.build_db(z, level, 3, 5), O.build_db(z['A_pyr'], z['Ap_pyr'], level))
    assert np.array_equal([x[0] for x in e['log']], o['app_ix'])                    # every NN row ...
    dist = [d for x in e['log'] if x[4] is not None for d in x[4]]
    assert len(dist) > 100 and np.array_equal(dist, o['dist'])                      # ... and every kappa distance


# ---- its rows at other sizes are the package's --------------------------------------------------------------
def _config(n_sm, n_lg, ch):
    return types.SimpleNamespace(n_sm=n_sm, n_lg=n_lg, n_half=(n_lg * n_lg) // 2, pad_sm=n_sm // 2, pad_lg=n_lg // 2, num_ch=ch)


@pytest.mark.parametrize('n_sm,n_lg,ch', [(1, 3, 1), (3, 7, 1), (5, 5, 1), (3, 9, 1), (1, 7, 2)])
def test_rows_equal_the_packages_feature_functions(n_sm, n_lg, ch):
    from ia_amd import algorithms, config
    # (B 5 x 4 over a 3 x 2 coarse level: windows wider than the images, the periodic padding)
    z = WI.rand_case(77, n_sm, n_lg, geo=dict(a_hw=(7, 6), b_hw=(5, 4), L=2), ch=ch, n_ap=2)
    c = _config(n_sm, n_lg, ch)
    D = WI.width(n_sm, n_lg, ch)
    assert np.array_equal(config.compute_weights(n_sm, n_lg, c.n_half, ch), z['weights']) and z['weights'].shape == (D,)
    A_feat = algorithms.compute_feature_array(z['A_pyr'], c, True)[1]
    As = np.vstack([np.hstack([A_feat, algorithms.compute_feature_array(p, c, False)[1]]) for p in z['Ap_pyr']])
    assert As.shape == (2 * 42, D) and np.array_equal(As, WI.build_db(z, 1, n_sm, n_lg))
    pad = lambda x, p: np.pad(x, ((p, p), (p, p)) + (((0, 0),) if x.ndim == 3 else ()), mode='symmetric')
    B_pair = (pad(z['B_pyr'][0], c.pad_sm), pad(z['B_pyr'][1], c.pad_lg))
    Bp_pair = (pad(z['Bp_init'][0], c.pad_sm), pad(z['Bp_init'][1], c.pad_lg))
    B_feat = WI.feature_array(z['B_pyr'], 1, True, n_sm, n_lg)
    for r in range(5):
        for col in range(4):
            q = np.hstack([algorithms.extract_pixel_feature(B_pair, (r, col), c, True),
                           algorithms.extract_pixel_feature(Bp_pair, (r, col), c, False)])
            assert np.array_equal(q, WI.query_feature(B_feat, z['Bp_init'][0], z['Bp_init'][1], r, col, 4, n_sm, n_lg))


def test_supported_sizes():
    ok = {1: [(s, l) for s in WI.N_SM for l in WI.N_LG if (s, l) != (5, 9)],
          2: [(1, 3), (1, 5), (1, 7), (3, 3), (3, 5), (5, 3)], 3: [(1, 3), (1, 5), (3, 3), (3, 5)]}
    for ch in (1, 2, 3):
        assert [(s, l) for s in WI.N_SM for l in WI.N_LG if WI.supported(s, l, ch)] == sorted(ok[ch])
    assert WI.width(5, 9, 1) == 171 and WI.width(3, 5, 3) == 165 and WI.width(3, 7, 3) == 273


# ---- the schedule ------------------------------------------------------------------------------------------
def test_wavefront_pad_equals_brute_force_and_keeps_the_dependencies():
    from ia_amd import _native
    violations = 0
    for pad in range(5):
        for h in range(1, 8):
            for w in range(1, 12):
                st = WI.steps(h, w, pad)
                T, mmax = _native.wavefront_shape_pad(h, w, pad)
                assert T == w + (pad + 1) * (h - 1) == max(st) + 1 and mmax == max(len(v) for v in st.values())
                seen = []
                for t in range(T):
                    r0, M = _native.wavefront_step_pad(h, w, pad, t)
                    assert M == len(st.get(t, [])) and 0 <= M <= mmax
                    px = [(r, t - (pad + 1) * r) for r in range(r0, r0 + M)]
                    assert px == st.get(t, [])
                    seen += px
                    if pad == 2:
                        assert (r0, M) == _native.wavefront_step(h, w, t)
                assert sorted(seen) == [(r, c) for r in range(h) for c in range(w)]      # every pixel exactly once
                if pad == 2:
                    assert (T, mmax) == _native.wavefront_shape(h, w)
                # a read pixel other than itself: raster-earlier => an earlier step, raster-later => a later one
                for r in range(h):
                    for c in range(w):
                        t = c + (pad + 1) * r
                        for rr, cc in WI.reads(r, c, h, w, pad):
                            if (rr, cc) == (r, c):
                                continue
                            t2 = cc + (pad + 1) * rr
                            violations += not (t2 < t if rr * w + cc < r * w + c else t2 > t)
    assert violations == 0
    with pytest.raises(_native.IAError, match='IA_EINVAL'):
        _native.wavefront_shape_pad(3, 3, 5)
    with pytest.raises(_native.IAError, match='IA_EINVAL'):
        _native.wavefront_step_pad(3, 3, 1, 7)     # steps 0 .. 6


# ---- config.set_windows, image_analogies.level_windows -------------------------------------------------------
def test_set_windows_and_level_windows():
    from ia_amd import _native, config
    from ia_amd.image_analogies import check_windows, level_windows, require_default_windows
    keep = (config.n_sm, config.n_lg, config.num_ch)
    try:
        assert level_windows(config) == (3, 5)
        for s in WI.N_SM:
            for l in WI.N_LG:
                config.set_windows(s, l)
                assert (config.n_sm, config.n_lg, config.n_half, config.pad_sm, config.pad_lg) == (s, l, (l * l) // 2, s // 2, l // 2)
                for ch in (None, 1, 2, 3):
                    config.num_ch = ch
                    if WI.supported(s, l, ch or 1):
                        assert level_windows(config) == (s, l)
                    else:
                        with pytest.raises(ValueError, match='supported window sizes'):
                            level_windows(config)
        config.num_ch = None
        config.set_windows(3, 5)
        config.n_lg = 7                                   # the reference's two-line edit: the derived three are stale
        with pytest.raises(ValueError, match='set_windows'):
            level_windows(config)
        for bad in [(0, 5), (2, 5), (7, 5), (3, 1), (3, 4), (3, 11)]:
            config.set_windows(*bad)
            with pytest.raises(ValueError, match='supported window sizes'):
                level_windows(config)
        config.set_windows(3, 7)
        with pytest.raises(ValueError, match='n_sm = 3, n_lg = 5 only'):
            require_default_windows(config, 'x')
        with pytest.raises(ValueError):                   # check_windows keeps refusing everything but 3 / 5 / 12
            check_windows(config)
    finally:
        config.set_windows(keep[0], keep[1])
        config.num_ch = keep[2]
    check_windows(config)
    assert level_windows(types.SimpleNamespace(n_sm=3, n_lg=5, n_half=12)) == (3, 5)
    with pytest.raises(ValueError, match='set_windows'):
        level_windows(types.SimpleNamespace(n_sm=3, n_lg=7, n_half=12.0, pad_sm=1, pad_lg=3))
    # the bindings: the weights' length follows the windows; the positional form keeps refusing other lengths
    A, Ac = np.zeros((6, 5)), np.zeros((3, 3))
    args = (A, Ac, A[None], Ac[None], A, Ac, Ac, A.copy())
    assert _native.check_level_shapes(*args, np.zeros(91), windows=(3, 7)) == 1
    for w, kw in [(np.zeros(31), {}), (np.zeros(91), {}), (np.zeros(55), dict(windows=(3, 7)))]:
        with pytest.raises(_native.IAError, match='weights'):
            _native.check_level_shapes(*args, w, **kw)
    assert _native.Stats().nbhd_levels == 0 and _native.Stats._fields_[-1][0] == 'nbhd_levels'
    assert _native.lib().ia_version() == 4


def test_img_setup_checks_the_sizes_against_the_images_channels(tmp_path):
    """a num_ch left over from an earlier job must not decide: the images' own channel count does"""
    from ia_amd import config
    from ia_amd.image_analogies import img_setup
    rs = np.random.RandomState(3)
    names = ['n_sm', 'n_lg', 'num_ch', 'gpu_preprocess', 'weights', 'max_levels', 'padding_sm', 'padding_lg', 'convert',
             'remap_lum', 'init_rand', 'AB_weight', 'n_levels', 'level_align', 'seed']
    keep = {n: getattr(config, n) for n in names}          # (the module is the reference's mutable namespace)
    try:
        config.gpu_preprocess, config.convert, config.remap_lum, config.init_rand, config.AB_weight = False, False, False, True, 1
        config.n_levels, config.level_align, config.seed = None, 'coarse', 3
        config.set_windows(3, 9)
        config.num_ch = 3                                  # stale: (3, 9) has 417 features at 3 channels
        g = lambda: rs.rand(12, 12)
        out = img_setup(g(), [g()], g(), str(tmp_path) + '/', config)
        assert config.num_ch == 1 and config.weights.shape == (139,) and len(out[0]) == config.max_levels
        rgb = lambda: rs.rand(12, 12, 3)
        with pytest.raises(ValueError, match='417 features'):
            img_setup(rgb(), [rgb()], rgb(), str(tmp_path) + '/', config)
    finally:
        config.set_windows(keep['n_sm'], keep['n_lg'])
        for n in names[2:]:
            setattr(config, n, keep[n])


# ---- the GPU cases are what they claim ------------------------------------------------------------------------
# per case: (pixels with an exact NN tie, pixels whose runner-up is within a relative 2^-20, kappa comparisons,
# coherence wins) of the restatement's run
COUNTS = {
    'size_c1_1_3': (0, 0, 394, 206), 'size_c1_3_3': (0, 0, 389, 250), 'size_c1_3_7': (0, 0, 395, 314),
    'size_c1_5_5': (0, 0, 397, 334), 'size_c1_5_7': (0, 0, 398, 329), 'size_c1_3_9': (0, 0, 397, 340),
    'size_c1_1_9': (0, 0, 396, 331), 'size_c3_3_3': (0, 0, 397, 328), 'size_c2_1_7': (0, 0, 396, 331),
    'border_5x1_3_9': (0, 0, 4, 3), 'border_5x1_5_7': (0, 0, 4, 0), 'border_6x2_3_9': (0, 0, 10, 5),
    'border_6x2_5_7': (0, 0, 10, 8), 'border_1x7_3_9': (0, 0, 4, 3), 'border_1x7_5_7': (0, 0, 4, 3),
    'border_2x11_3_9': (0, 0, 21, 15), 'border_2x11_5_7': (0, 0, 20, 16), 'smallA23_3_9': (0, 0, 25, 20),
    'smallA11_3_9': (0, 0, 0, 0), 'smallA23_5_7': (0, 0, 18, 13), 'smallA11_5_7': (0, 0, 0, 0),
    'edge_neartie36': (0, 320, 397, 395), 'edge_constA': (400, 400, 397, 397), 'edge_tiny': (0, 0, 397, 307),
    'edge_offset': (0, 400, 393, 393), 'edge_x64edge': (0, 0, 395, 300), 'edge_bigA': (0, 0, 191, 133),
    'edge_bigA_3_9': (0, 0, 191, 147),
    'x1000': (0, 0, 392, 300), 'pairs2': (0, 0, 141, 100), 'wide45_v0': (0, 0, 403, 314), 'wide45_v1': (0, 0, 404, 336),
    'wide45_v2': (0, 0, 404, 371), 'wide45_v3': (0, 0, 396, 390), 'wide70_v0': (0, 0, 1188, 894), 'wide70_v1': (0, 0, 1185, 937),
}


def test_every_gpu_case_is_counted():
    assert sorted(COUNTS) == sorted(WI.CASES)


def test_big_db_reaches_the_row_kernels_second_grid_trip():
    """edge_bigA_3_9: k_nbhd_rows runs at most 4,096 workgroups of 256 threads, and this DB has 102,344 elements
    more; the restatement takes final sources among the rows those elements belong to, so a DB whose tail was not
    written cannot give its result"""
    z, e = WI.make('edge_bigA_3_9'), WI.expected('edge_bigA_3_9')
    a_h, a_w = z['A_pyr'][1].shape[:2]
    D, rows = WI.width(*z['win'], 1), a_h * a_w
    assert z['L'] == 2 and z['win'] == (3, 9) and D == 139 and rows == 8280
    assert WI.ROWS_GRID == 1048576 and rows * D == 1150920 > WI.ROWS_GRID and rows * D - WI.ROWS_GRID == 102344
    assert WI.BIG_CUT == WI.ROWS_GRID // D == 7543
    assert -(-rows // 32) == 259                                   # bigA's DB tiles
    src = (a_h * e['im'][1] + e['s'][1][:, 0]) * a_w + e['s'][1][:, 1]
    assert len(src) == 192 and int((src >= WI.BIG_CUT).sum()) == 5              # final source rows in the second trip
    assert sum(1 for x in e['log'] if x[0] >= WI.BIG_CUT) == 12    # and the NN rows there, before the kappa rule


@pytest.mark.parametrize('name', sorted(WI.CASES))
def test_gpu_case_is_what_it_claims(name):
    z, e = WI.make(name), WI.expected(name)
    log = e['log']
    ties = sum(1 for x in log if x[2] > 1)
    near = sum(1 for x in log if x[3] < AI.REL_TIE)
    kap = [(x[4][0], x[4][1], x[5]) for x in log if x[4] is not None]
    wins = sum(1 for da, dc, kf in kap if dc <= da * kf)
    assert (ties, near, len(kap), wins) == COUNTS[name]
    assert ties == 0 or name == 'edge_constA'                      # no exact NN tie, except on the constant A
    for da, dc, kf in kap:                                         # no kappa comparison near its threshold
        assert da * kf == 0 or abs(dc - da * kf) > 1e-6 * da * kf
    if name == 'smallA11_3_9':
        assert len(kap) == 0                                       # a 1 x 1 A: no shifted source stays inside it
    # geometry: DB tiles of the finest level, the widest step and the query tiles over the steps
    n_sm, n_lg = z['win']
    h, w = z['B_pyr'][-1].shape[:2]
    rows = len(z['Ap_pyr']) * z['Ap_pyr'][0][-1].shape[0] * z['Ap_pyr'][0][-1].shape[1]
    T, mmax, tiles = WI.step_shape(h, w, n_lg // 2)
    geo = (-(-rows // 32), rows % 32, T, mmax)
    want = {'size': (15, 27, 20 + (n_lg // 2 + 1) * 15, min(16, -(-20 // (n_lg // 2 + 1)))), 'edge_bigA': (259, 24, 60, 4),
            'edge_bigA_3_9': (259, 24, 71, 4), 'wide45': (15, 27, 85, 9), 'wide70': (15, 27, 134, 17), 'pairs2': (8, 16, 53, 4)}
    keys = [key for key in want if name.startswith(key)]
    if keys:
        assert geo == want[max(keys, key=len)], geo                # (the longest prefix: edge_bigA_3_9 has p_l = 4)
    if name.startswith('wide45'):
        assert WI.step_shape(h, w, 4, 32)[1] * 32 == 288           # 9 query tiles: three blocks of KH 84's three
        assert WI.width(3, 9, 1) == 139
    if name.startswith('border') or name.startswith('smallA'):
        assert min(h, w) <= n_lg // 2 or rows <= 6                 # narrower than the pad, or a tiny A
        if w <= n_lg // 2:
            assert any(len(v) == 0 for v in [WI.steps(h, w, n_lg // 2).get(t, []) for t in range(T)]) or h == 1

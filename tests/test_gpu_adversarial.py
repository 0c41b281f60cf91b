"""GPU parity on adversarial inputs (tests/adversarial_inputs.py): every exactness claim rests on
certified error bounds - the split-f16 value bound (ia_eps_c_h / ia_eps_a_h), the fp32 bound
(ia_eps_c), cert_theta, the hi x hi block filter limit and the pruning radius U' - and a bound
that is slightly too tight returns a wrong nearest neighbour only where its slack runs out.  The
golden fixtures are all photo-like images in [0, 1]; these cases sit at the edges instead: values
up to the +-64 gate of the split-f16 matcher (and one value past it, in each of the eight arrays
the gate scans), values of 2^-14 where the absolute (f16-subnormal) term decides, a common offset
of +-50 with 1e-3 of contrast, DB rows equal to within 2^-26 / 2^-36 whose winner only fp64 decides
(and which is mostly not the lowest index), a constant A side (zero covariance, every row an exact
tie), kappa = 0 and a DB of 259 tiles.

The expected values are the oracle's (oracle/ia_oracle.py, fp64, brute force, computed at test
time, once per case); tests/test_adversarial_inputs_cpu.py pins that its own decisions are robust
on these inputs.  Everything is compared bit for bit, and each run must have taken the path it
is meant to test (Stats.f16_levels / pruned_levels / fallbacks / reranked).
"""
import numpy as np
import pytest

import adversarial_inputs as AI
from golden_util import PRUNE_MIN_ROWS_DEFAULT, check_debug_records

pytestmark = pytest.mark.gpu

PRUNED = dict(prune_min_rows=1)
SETTINGS = {
    'default': {},
    'f32': dict(matcher='f32'),
    'pruned_v24': dict(PRUNED, k3p_variant=24),
    'pruned_v25': dict(PRUNED, k3p_variant=25),
    'pruned_v22': dict(PRUNED, k3p_variant=22),
    'pruned_v21': dict(PRUNED, k3p_variant=21),
    'pruned_v20': dict(PRUNED, k3p_variant=20),
    'pruned_min_rows_1': dict(PRUNED),
    # several DB tiles per workgroup: 259 tiles on 64 workgroups
    'pruned_v24_wgs64': dict(PRUNED, k3p_variant=24, scan_wgs=64),
    # 259 tiles >= 64 * 2: the level shards (debug records are single-rank only: s, im and B' are checked)
    'pruned_shard2': dict(PRUNED, shard_emulate=2),
}
PATHS = ['default', 'f32', 'pruned_v24', 'pruned_v25', 'pruned_v22', 'pruned_v21', 'pruned_v20']
RUNS = ([(c, s) for c in AI.BASE_CASES for s in PATHS] +
        [('k0', s) for s in ('default', 'f32', 'pruned_v24')] +
        [(c, s) for c in AI.BIG_CASES for s in PATHS + ['pruned_v24_wgs64', 'pruned_shard2']] +
        [(c, s) for c in AI.GATE_CASES for s in ('default', 'pruned_min_rows_1')])


def _run(ctx, z, setting):
    from ia_amd import _native
    opts = dict(SETTINGS[setting])
    if 'matcher' in opts:
        opts['matcher'] = _native.IA_MATCH_F32
    debug = 'shard_emulate' not in opts
    L, k = z['L'], z['k']
    Bp = [x.copy() for x in z['Bp_init']]
    out = {}
    st = _native.Stats()
    try:
        for name, v in opts.items():
            ctx.set_option(name, v)
        for level in range(1, L):
            kf = 1 + (2 ** (level - L)) * k
            dbg = {} if debug else None
            s, im = ctx.synthesize_level(z['A_pyr'][level], z['A_pyr'][level - 1], [p[level] for p in z['Ap_pyr']],
                                         [p[level - 1] for p in z['Ap_pyr']], z['B_pyr'][level],
                                         z['B_pyr'][level - 1], Bp[level - 1], Bp[level], z['weights'], kf, st,
                                         debug=dbg)
            out[level] = (s, im, dbg)
    finally:
        ctx.set_option('prune_min_rows', PRUNE_MIN_ROWS_DEFAULT)
        ctx.set_option('k3p_variant', 24)
        ctx.set_option('matcher', _native.IA_MATCH_F16X3)
        ctx.set_option('scan_wgs', 256)
        ctx.set_option('shard_emulate', 1)
    return out, Bp, st


@pytest.mark.parametrize('case,setting', RUNS, ids=['%s-%s' % r for r in RUNS])
def test_adversarial_case_matches_oracle(ctx, case, setting):
    """s, im and B' of every level, every NN row, every coherence pick and both compute_distance
    values of every kappa comparison equal the oracle's, on the path the setting names.

    fallbacks > 0 on 'tiny' is derived, not measured: every squared distance there is
    < 55 * 2^-28 ~ 2e-7 while the split-f16 matcher's absolute term over a chunk is ~ 8e-6, so no
    chunk of >= 3 rows can certify a winner and all of them are rescanned exactly."""
    z = AI.oracle(case)
    out, Bp, st = _run(ctx, z, setting)
    L = z['L']
    print('ADV %-13s %-18s fallbacks %6d reranked %6d f16_levels %d pruned_levels %d kappa_ambiguous %d'
          % (case, setting, st.fallbacks, st.reranked, st.f16_levels, st.pruned_levels, st.kappa_ambiguous))
    if out[1][2] is not None:
        check_debug_records(z, out, Bp, st, case, kappa_equalities=(case == 'k0'))
    else:
        for level in range(1, L):
            assert np.array_equal(out[level][0], z['s'][level]) and np.array_equal(out[level][1], z['im'][level])
            assert np.array_equal(Bp[level], z['Bp_final'][level])
        assert st.bound_violations == 0 and st.kappa_ambiguous == 0
    gate, f32, pruned = case in AI.GATE_CASES, setting == 'f32', setting.startswith('pruned')
    assert st.pixels == sum(x.size for x in z['B_pyr'][1:])
    # one value past +-64 leaves the split-f16 scan, and with it the pruned scan
    assert st.f16_levels == (0 if gate or f32 else L - 1)
    assert st.pruned_levels == (L - 1 if pruned and not gate else 0)
    if case == 'tiny' and not f32:
        assert st.fallbacks > 0
    if case in ('neartie26', 'neartie36', 'bigA_neartie', 'constA'):
        assert st.reranked > 0


# ---- the exact index (ia_index_*: fp32 MFMA + fp64 rerank, arbitrary user points) -----------------
def _check_index(ctx, pts, q):
    """argmin and distance of ((pts - q) ** 2).sum(axis=1) in numpy fp64, bit for bit"""
    from ia_amd import _native
    idx = _native.ExactIndex(ctx, pts)
    try:
        i_gpu, d_gpu = idx.query(q)
    finally:
        idx.close()
    q = np.atleast_2d(q)
    assert i_gpu.shape == d_gpu.shape == (len(q),)
    for j in range(len(q)):
        dd = ((pts - q[j]) ** 2).sum(axis=1)
        assert i_gpu[j] == int(np.argmin(dd)), (j, int(i_gpu[j]), int(np.argmin(dd)))
        assert d_gpu[j] == dd[i_gpu[j]], j


def _offset_pts(rs, n, d):
    return 1000 + 1e-3 * rs.rand(n, d)


INDEX_INPUTS = {
    'offset1000': lambda rs: (_offset_pts(rs, 700, 55), _offset_pts(rs, 40, 55)),
    'offset1000_x2p20': lambda rs: (_offset_pts(rs, 700, 55) * 2.0 ** 20, _offset_pts(rs, 40, 55) * 2.0 ** 20),
    'offset1000_x2m20': lambda rs: (_offset_pts(rs, 700, 55) * 2.0 ** -20, _offset_pts(rs, 40, 55) * 2.0 ** -20),
    'rand_x2p20': lambda rs: (rs.rand(700, 55) * 2.0 ** 20, rs.rand(40, 55) * 2.0 ** 20),
    'rand_x2m20': lambda rs: (rs.rand(700, 55) * 2.0 ** -20, rs.rand(40, 55) * 2.0 ** -20),
    'signed': lambda rs: (rs.rand(700, 55) - 0.5, rs.rand(40, 55) - 0.5),
    'n31': lambda rs: (rs.rand(31, 55), rs.rand(40, 55)),
    'n32': lambda rs: (rs.rand(32, 55), rs.rand(40, 55)),
    'n33': lambda rs: (rs.rand(33, 55), rs.rand(40, 55)),
    'n1_signed': lambda rs: (rs.rand(1, 55) - 0.5, rs.rand(40, 55) - 0.5),
    'd1': lambda rs: (rs.rand(700, 1), rs.rand(40, 1)),
    'd1_offset1000': lambda rs: (_offset_pts(rs, 700, 1), _offset_pts(rs, 40, 1)),
    'd167': lambda rs: (rs.rand(700, 167), rs.rand(40, 167)),
    'd167_offset1000': lambda rs: (_offset_pts(rs, 700, 167), _offset_pts(rs, 40, 167)),
    'nq1': lambda rs: (rs.rand(700, 55), rs.rand(1, 55)),
    'n5000_offset1000': lambda rs: (_offset_pts(rs, 5000, 55), _offset_pts(rs, 33, 55)),
}


@pytest.mark.parametrize('name', list(INDEX_INPUTS))
def test_exact_index_adversarial_points(ctx, name):
    rs = np.random.RandomState(list(INDEX_INPUTS).index(name))
    pts, q = INDEX_INPUTS[name](rs)
    h = min(len(q), len(pts)) // 2
    q[:h] = pts[:h]   # exact hits (distance 0)
    _check_index(ctx, pts, q)


@pytest.mark.parametrize('log2_delta', [-30, -40])
def test_exact_index_near_duplicates_are_decided_in_fp64(ctx, log2_delta):
    """50 base rows, 40 copies of each, every copy with its own delta * rand: the 40 rows nearest a
    query differ by a relative ~delta, far below fp32, and the nearest is mostly not the first"""
    rs = np.random.RandomState(17)
    base = rs.rand(50, 55)
    pts = np.vstack([base] * 40) + 2.0 ** log2_delta * rs.rand(2000, 55)
    rs.shuffle(pts)
    q = base + 1e-3 * rs.rand(*base.shape)
    not_lowest = 0
    for j in range(len(q)):
        dd = ((pts - q[j]) ** 2).sum(axis=1)
        i = int(np.argmin(dd))
        near = np.flatnonzero(dd <= dd[i] * (1 + AI.REL_TIE))
        assert len(near) >= 40 and (dd == dd[i]).sum() == 1   # near-ties, none exact
        not_lowest += int(near[0] != i)
    assert not_lowest > len(q) // 2
    _check_index(ctx, pts, q)


def test_exact_index_refuses_168_columns(ctx):
    from ia_amd import _native
    with pytest.raises(_native.IAError, match='IA_EINVAL'):
        _native.ExactIndex(ctx, np.random.RandomState(0).rand(40, 168))

"""GPU parity at 2 and 3 channels, on every scan instance a level can launch.

Every kernel stage is compiled per channel count.  2 channels (D = 110) run the split-f16 scan with
KS = 7 k-steps (ia_k3h.hip, QT = 1 .. 8) or the fp32 scan with KH = 56 (ia_k3.hip, QT = 1 .. 5), with
their own tile format, DB build, gathers, merges, sharded merges and certified bounds
(ia_eps_c_h(7, .), ia_eps_c at D = 110); 3 channels (D = 165) always run the fp32 scan with KH = 84
(QT = 1 .. 3).  The reference writes colour back for 3 channels only, so 2-channel images have no
reference run and no golden fixture: the expected values are the oracle's (oracle/ia_oracle.py,
fp64, brute force, channel-generic), computed once per case per process;
tests/test_adversarial_inputs_cpu.py pins that its decisions on these inputs are robust.

The inputs are those of tests/test_gpu_adversarial.py at 2 and 3 channels (tests/adversarial_inputs.py,
name + '_c2' / '_c3'), plus: two A' images; a DB of 259 tiles on 8 workgroups (33 tiles per
workgroup: each wave loops with prefetch) and sharded two ways; a batch of 32 jobs whose steps hold
1 .. 9 query tiles, so every QT instance and a multi-block step run; and the +-64 gate with its
out-of-range value at the LAST element of each array, of a single job and of job 1 of a batch.

Everything is compared bit for bit (golden_util.check_debug_records: s, im, B', every NN row, every
coherence pick, both compute_distance values; sharded runs refuse debug records: s, im and B'), and
each run must have taken the path it is meant to test.
"""
import numpy as np
import pytest

import adversarial_inputs as AI
from golden_util import PRUNE_MIN_ROWS_DEFAULT, check_debug_records, scan_counts, sharded_scan_launches

pytestmark = pytest.mark.gpu

SHARD = dict(shard_unpruned=1, shard_emulate=2)
SETTINGS = {
    'default': {},
    'f32': dict(matcher='f32'),
    # 259 tiles on 8 workgroups: 33 tiles per workgroup
    'wgs8': dict(scan_wgs=8),
    # 259 tiles >= 64 * 2: the unpruned level shards (debug records are single-rank only)
    'shard2_allgather': dict(SHARD, exchange=0),
    'shard2_peerwrite': dict(SHARD, exchange=1),
    # 2 channels never prune (the ring kernel is KS = 4 only): the option must change nothing
    'prune_min_rows_1': dict(prune_min_rows=1),
}
NEAR_TIE = ('neartie26', 'neartie36', 'constA')
RUNS = ([(c, s) for c in AI.BASE_CH_CASES if c.endswith('_c2') for s in ('default', 'f32')] +
        [(c, 'default') for c in AI.BASE_CH_CASES if c.endswith('_c3')] +
        [('multiap_c2', 'default'), ('multiap_c2', 'f32'), ('multiap_c3', 'default')] +
        [('bigA_c2', s) for s in ('default', 'f32', 'wgs8', 'shard2_allgather', 'shard2_peerwrite')] +
        [('bigA_c3', s) for s in ('default', 'shard2_allgather', 'shard2_peerwrite')] +
        [(c, 'default') for c in AI.GATE_LAST_CASES] +
        [('x60_c2', 'prune_min_rows_1')])


def _set(ctx, setting):
    from ia_amd import _native
    opts = dict(SETTINGS[setting])
    if 'matcher' in opts:
        opts['matcher'] = _native.IA_MATCH_F32
    for name, v in opts.items():
        ctx.set_option(name, v)


def _restore(ctx):
    from ia_amd import _native
    ctx.set_option('prune_min_rows', PRUNE_MIN_ROWS_DEFAULT)
    ctx.set_option('matcher', _native.IA_MATCH_F16X3)
    ctx.set_option('scan_wgs', 256)
    ctx.set_option('shard_emulate', 1)
    ctx.set_option('shard_unpruned', 0)
    ctx.set_option('exchange', 0)


def _run_jobs(ctx, Z, setting, debug=True):
    """every level of the jobs Z (cases sharing one A side) in one synthesize_levels call per
    level: ([out[level] = (s, im, dbg)] per job, [B' pyramid] per job, Stats)"""
    from ia_amd import _native
    z0, L = Z[0], Z[0]['L']
    Bp = [[x.copy() for x in z['Bp_init']] for z in Z]
    out = [dict() for _ in Z]
    st = _native.Stats()
    try:
        _set(ctx, setting)
        for level in range(1, L):
            dbg = [{} if debug else None for _ in Z]
            specs = [dict(B=z['B_pyr'][level], Bc=z['B_pyr'][level - 1], Bpc=Bp[j][level - 1], Bp=Bp[j][level],
                          weights=z['weights'], kappa_factor=1 + (2 ** (level - L)) * z['k'], debug=dbg[j])
                     for j, z in enumerate(Z)]
            res = ctx.synthesize_levels(z0['A_pyr'][level], z0['A_pyr'][level - 1], [p[level] for p in z0['Ap_pyr']],
                                        [p[level - 1] for p in z0['Ap_pyr']], specs, st)
            for j, (s, im) in enumerate(res):
                out[j][level] = (s, im, dbg[j])
    finally:
        _restore(ctx)
    return out, Bp, st


def _f16(case, setting):
    """the run scans split-f16: 2 channels (KS = 7; 3 channels have no instance), the default
    matcher, every value within +-64"""
    return AI.case_ch(case) == 2 and setting != 'f32' and not case.startswith('gate')


def _check_path(st, Z, case, setting):
    L, J = Z[0]['L'], len(Z)
    assert st.pixels == sum(x.shape[0] * x.shape[1] for z in Z for x in z['B_pyr'][1:])
    assert st.f16_levels == (J * (L - 1) if _f16(case, setting) else 0)
    assert st.pruned_levels == 0
    assert st.bound_violations == 0 and st.kappa_ambiguous == 0
    if case.startswith('tiny') and _f16(case, setting):
        # nothing certifies: every chunk (8 tiles, one per wave of a scan workgroup) of every pixel
        assert st.fallbacks == sum(x.shape[0] * x.shape[1] * -(-c['n'] // 8)
                                   for x, c in zip(Z[0]['B_pyr'][1:], scan_counts(Z[0], 1))) > 0
    if _f16(case, setting) and (case in AI.NO_FALLBACK_C2 or case == 'wide_c2'):
        # the third-nearest row of every pixel is more than 4 eps above the winner (pinned on the
        # CPU, AI.certify_margin): a scan whose values are within eps rescans no chunk, on any
        # decomposition of the DB.  Wrong scan values show here first: the exact rescans keep the
        # decisions right
        assert st.fallbacks == 0
    if case.startswith(NEAR_TIE):
        # rows within a relative 2^-26 are beyond either matcher's precision: some pixel must have
        # taken more than one exact (fp64) evaluation
        assert st.reranked > st.pixels


@pytest.mark.parametrize('case,setting', RUNS, ids=['%s-%s' % r for r in RUNS])
def test_channel_case_matches_oracle(ctx, case, setting):
    """s, im and B' of every level, every NN row, every coherence pick and both compute_distance
    values of every kappa comparison equal the oracle's, on the path the setting names.

    The fallbacks of 'tiny' under split-f16 are derived as at 1 channel: every squared distance is
    < 110 * 2^-28 while the absolute (f16-subnormal) term of the bound is ~ 8e-6, so no chunk can
    certify a winner and all of them are rescanned exactly."""
    z = AI.oracle(case)
    sharded = setting.startswith('shard')
    out, Bp, st = _run_jobs(ctx, [z], setting, debug=not sharded)
    print('CH %-14s %-17s fallbacks %6d reranked %6d f16_levels %d pruned_levels %d dist_launches %d bound_violations %d'
          % (case, setting, st.fallbacks, st.reranked, st.f16_levels, st.pruned_levels, st.dist_launches,
             st.bound_violations))
    if sharded:
        for level in range(1, z['L']):
            assert np.array_equal(out[0][level][0], z['s'][level]) and np.array_equal(out[0][level][1], z['im'][level])
            assert np.array_equal(Bp[0][level], z['Bp_final'][level])
        assert st.dist_launches == sharded_scan_launches(z, 1, 2)
        assert st.dist_launches == 2 * sharded_scan_launches(z, 1, 1)   # the level did shard
    else:
        check_debug_records(z, out[0], Bp[0], st, case)
    _check_path(st, [z], case, setting)


@pytest.mark.parametrize('kind', AI.GATE_JOB1_KINDS)
def test_gate_scans_every_job_to_its_last_element(ctx, kind):
    """two jobs in one call, 2 channels: job 0 in range, job 1 with 64.5 at the last element of its
    B, Bc, B' coarse or B' array.  The one matcher decision of the call must see it (no split-f16
    level), and both jobs equal their oracle runs."""
    case = 'gate_job1_%s_c2' % kind
    Z = [AI.oracle(AI.GATE_JOB0), AI.oracle(case)]
    out, Bp, st = _run_jobs(ctx, Z, 'default')
    for j, z in enumerate(Z):
        check_debug_records(z, out[j], Bp[j], st, '%s job %d' % (case, j))
    _check_path(st, Z, case, 'default')


WIDE_RUNS = [(2, 'default'), (2, 'f32'), (3, 'default')]


@pytest.mark.parametrize('ch,setting', WIDE_RUNS, ids=['c%d-%s' % r for r in WIDE_RUNS])
def test_wide32_every_query_tile_count(ctx, ch, setting):
    """32 jobs in one call: job j is variant j mod 4 (one A side; own B, Bc, B' and kappa each),
    with its own B' buffers and debug records.  Steps hold 32, 64, ... 288 queries = 1 .. 9 query
    tiles: split-f16 KS = 7 launches QT 1 .. 8 and a 9-tile step in two blocks, fp32 KH = 56 QT
    1 .. 5 then two blocks, KH = 84 QT 1 .. 3 then up to three blocks.  Every job must equal its
    variant's oracle run (4 oracle runs, not 32): one that reads a neighbour's queries, B' or
    kappa factor fails."""
    V = [AI.oracle(n) for n in AI.WIDE_CASES[ch]]
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(V[i]['s'][1], V[j]['s'][1])
    Z = [V[j % 4] for j in range(32)]
    out, Bp, st = _run_jobs(ctx, Z, setting)
    for j, z in enumerate(Z):
        check_debug_records(z, out[j], Bp[j], st, 'wide32 ch %d job %d' % (ch, j))
    _check_path(st, Z, 'wide_c%d' % ch, setting)
    cnt = scan_counts(V[0], 32, matcher=setting if setting == 'f32' else 'f16x3')
    print('wide32', ch, setting, st.dist_pairs_full, st.dist_tiles_full, st.dist_launches, cnt)
    assert st.dist_pairs_full == sum(c['n'] * c['qtt'] for c in cnt)
    assert st.dist_tiles_full == sum(c['n'] * c['nqb'] for c in cnt)
    assert st.dist_launches == sum(c['nqb'] for c in cnt) > sum(c['steps'] for c in cnt)   # some step ran in blocks
    # the steps of this geometry, by query tiles: three each of 1 .. 9 and of 8 .. 1
    qtmax = {(2, 'default'): 8, (2, 'f32'): 5, (3, 'default'): 3}[ch, setting]
    tiles = [t for t in range(1, 10) for _ in range(3)] + [t for t in range(8, 0, -1) for _ in range(3)]
    assert len(cnt) == 1 and cnt[0]['steps'] == len(tiles) and cnt[0]['qtt'] == sum(tiles)
    assert cnt[0]['nqb'] == sum(-(-t // qtmax) for t in tiles)

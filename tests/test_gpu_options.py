"""The scan and merge options no other test sets (include/ia.h ia_set_option), pinned to the
reference's recorded runs: "early_gather" (gather_p_early, ia_gather.h: a second copy of the
query gather with its own summation orders and a U' without the row above's candidates),
"rec_wt" (write-through record stores of the pruned scan, ia_k3h.hip), "prefetch_next" (without
it early_gather does not apply) and "stamps" (every pruned-scan and merge workgroup stores its
s_memrealtime ticks) - and the composition bench.py times: four pipelined contexts with stream
priorities, the coarser ones with scan_wgs 128, a lowered prune_min_rows and stamps on.

All of them are "identical results for every setting" by contract, so every comparison here is
bit-exact against the golden fixtures (real reference runs): no tolerances.  With prune_min_rows =
1 every 1-channel level of the small cases runs the certified pruned scan and the fused merge +
gather; the pyramids of g32 and rect go down to 1x2, 2x3 and 4x4 levels, where the fused chain is
refused (bw < 3) and the early gather's late pixel reflects into several window slots.

The module makes its own contexts (the session context keeps its defaults) and restores every
option it sets."""
import contextlib

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

from golden_util import (BIG_CASES, PRUNE_MIN_ROWS_DEFAULT, SLIM_CASES, check_debug_records, load_e2e, load_slim,
                         sha1_f64)

pytestmark = pytest.mark.gpu

# library defaults (include/ia.h) of every option this module touches
DEFAULTS = dict(early_gather=1, rec_wt=1, prefetch_next=1, nn_bound=1, stamps=0, prune_min_rows=PRUNE_MIN_ROWS_DEFAULT,
                k3p_variant=24, fuse_gather=1, fuse_sort=0, time_dist=0, shard_emulate=1, exchange=0)
BENCH_PRUNE_MIN_ROWS = 262144   # bench.py --prune-min-rows of the pipelined cfg3 / cfg4 and cfg5 runs


@contextlib.contextmanager
def _options(ctxs, **opts):
    """set options on every context; on exit each gets back the value it had (the library default
    where it was never set)"""
    assert set(opts) <= set(DEFAULTS)
    prev = [{k: c.option(k, DEFAULTS[k]) for k in opts} for c in ctxs]
    try:
        for c in ctxs:
            for k, v in opts.items():
                c.set_option(k, v)
        yield
    finally:
        for c, p in zip(ctxs, prev):
            for k, v in p.items():
                c.set_option(k, v)


@pytest.fixture(scope='module')
def octx():
    from ia_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def bench4():
    """four contexts as bench.py's make_context + pipe_contexts make them with the default command
    line: k3p_variant 24, rec_wt and early_gather set explicitly, the finest level's context
    (the first) on the high-priority stream, the three others low with scan_wgs 128"""
    from ia_amd import _native
    cs = [_native.Context(0) for _ in range(4)]
    for c in cs:
        c.set_option('matcher', _native.IA_MATCH_F16X3)
        c.set_option('prune', 1)
        c.set_option('k3p_variant', 24)
        c.set_option('rec_wt', 1)
        c.set_option('early_gather', 1)
    cs[0].set_option('stream_priority', 1)
    for c in cs[1:]:
        c.set_option('stream_priority', 2)
        c.set_option('scan_wgs', 128)
    yield cs
    for c in cs:
        c.close()


def _have(names):
    import os
    from golden_util import GOLDEN
    return [n for n in names if os.path.exists(os.path.join(GOLDEN, 'e2e_%s.npz' % n))]


_CACHE = {}


def _load(name):
    """each fixture read once per module run (never modified: runs copy Bp_init)"""
    if name not in _CACHE:
        _CACHE[name] = load_slim(name) if name in ('g512', 'g64slim') else load_e2e(name)
    return _CACHE[name]


def _run(ctx, z, debug=False):
    """every level in sequence, one Stats per level (the stamp fields of a shared Stats keep the
    largest pruned level only).  Returns out[level] = (s, im, dbg), the B' pyramid, the per-level
    Stats and their plain sum over the additive fields."""
    from ia_amd import _native
    L, k = z['L'], float(z['k'])
    Bp = [x.copy() for x in z['Bp_init']]
    out, sts = {}, {}
    for level in range(1, L):
        dbg = {} if debug else None
        sts[level] = _native.Stats()
        s, im = ctx.synthesize_level(z['A_pyr'][level], z['A_pyr'][level - 1], [p[level] for p in z['Ap_pyr']],
                                     [p[level - 1] for p in z['Ap_pyr']], z['B_pyr'][level], z['B_pyr'][level - 1],
                                     Bp[level - 1], Bp[level], z['weights'], 1 + 2.0 ** (level - L) * k, sts[level],
                                     debug=dbg)
        out[level] = (s, im, dbg)
    tot = _native.Stats()
    for k_, _ in _native.Stats._fields_:
        if k_ not in ('build_rows', 'prune_rows'):
            setattr(tot, k_, sum(getattr(st, k_) for st in sts.values()))
    return out, Bp, sts, tot


def _check_levels(z, out, Bp, st):
    for level in range(1, z['L']):
        s, im = out[level][0], out[level][1]
        assert np.array_equal(s, z['s'][level]) and np.array_equal(im, z['im'][level]), level
        assert np.array_equal(Bp[level], z['Bp_final'][level]), level
    assert st.bound_violations == 0 and st.kappa_ambiguous == 0


# ---- 1. the option matrix against the reference's per-pixel records --------------------------------

# (early_gather, rec_wt, prefetch_next, nn_bound)
MATRIX = [(1, 1, 1, 1),                                            # control: the defaults
          (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0),  # each one alone off
          (0, 0, 0, 0),
          (0, 1, 0, 1),   # with (1, 1, 0, 1): early_gather is inert without prefetch
          (0, 1, 1, 0)]   # with (1, 1, 1, 0): U' from the coherence candidates alone, early and plain
MATRIX_CASES = _have(['g32', 'rect', 'g64', 'ties128', 'k25', 'g256'])


def _matrix_id(m):
    return 'early%d_wt%d_pre%d_nn%d' % m


@pytest.mark.parametrize('setting', MATRIX, ids=_matrix_id)
@pytest.mark.parametrize('name', MATRIX_CASES)
def test_option_matrix_matches_reference_records(octx, name, setting):
    """Every level on the pruned scan + fused merge / gather (prune_min_rows 1, k3p_variant 24)
    under each setting of (early_gather, rec_wt, prefetch_next, nn_bound): s, im, B', every NN
    index, coherence pick and compute_distance value of the reference run.  With nn_bound 0 the
    coherence candidates are the only bound U' has left, without (early) and with (plain) the row
    above's.  fallbacks is NOT compared between settings: it depends on the dynamic tile hand-out."""
    z = _load(name)
    e, wt, pre, nn = setting
    with _options([octx], prune_min_rows=1, k3p_variant=24, early_gather=e, rec_wt=wt, prefetch_next=pre, nn_bound=nn):
        out, Bp, _, st = _run(octx, z, debug=True)
    check_debug_records(z, out, Bp, st, name)
    assert st.pruned_levels == z['L'] - 1
    if name in ('g256', 'ties128'):   # pruning engages, so a too-small U' would drop the true NN
        print('%s %s: dist_pairs %.0f of %.0f' % (name, _matrix_id(setting), st.dist_pairs, st.dist_pairs_full))
        assert st.dist_pairs < st.dist_pairs_full


# ---- 2. the same switches where they meet other paths ----------------------------------------------

SMALL = _have(['g64', 'ties128'])


@pytest.mark.parametrize('variant', [20, 21, 22, 24, 25])
@pytest.mark.parametrize('rec_wt', [0, 1])
@pytest.mark.parametrize('name', SMALL)
def test_rec_wt_every_scan_variant(octx, name, rec_wt, variant):
    """the record store is per scan kernel instance; 21 / 25 launch the presorted forms"""
    z = _load(name)
    with _options([octx], prune_min_rows=1, k3p_variant=variant, rec_wt=rec_wt):
        out, Bp, _, st = _run(octx, z, debug=True)
    check_debug_records(z, out, Bp, st, name)
    assert st.pruned_levels == z['L'] - 1


@pytest.mark.parametrize('fuse_sort', [0, 1])
@pytest.mark.parametrize('early', [0, 1])
@pytest.mark.parametrize('name', SMALL)
def test_early_gather_with_sampled_steps(octx, name, early, fuse_sort):
    """time_dist 3: every third step and the one before it run the separate gather and merge
    launches, so early gathers (fused steps) and plain gathers alternate within a level and hand
    off row to row.  fuse_sort 1: the gathers that also sort the step publish their records and
    take the plain path (k_merge_gather: early needs no key slots)."""
    z = _load(name)
    with _options([octx], prune_min_rows=1, early_gather=early, time_dist=3, fuse_sort=fuse_sort):
        out, Bp, _, st = _run(octx, z, debug=True)
    check_debug_records(z, out, Bp, st, name)
    assert st.pruned_levels == z['L'] - 1
    assert st.dist_launches_timed > 0 and st.merge_launches_timed > 0   # the sampled steps ran


@pytest.mark.parametrize('name', SMALL)
def test_early_gather_inert_without_fused_gather(octx, name):
    z = _load(name)
    with _options([octx], prune_min_rows=1, early_gather=1, fuse_gather=0):
        out, Bp, _, st = _run(octx, z, debug=True)
    check_debug_records(z, out, Bp, st, name)
    assert st.pruned_levels == z['L'] - 1


def _jobs_g32(z, kappas=(0.5, 5.0, 25.0, 1.0)):
    """as test_gpu_batch._jobs_g32: the golden g32 job (k = 0.5, the reference's B' init) + three
    variants with other kappas and B' inits"""
    from ia_amd.img_preprocess import initialize_Bp
    return [(k, [x.copy() for x in z['Bp_init']] if n == 0 else initialize_Bp(z['B_pyr'], True, seed=100 + n))
            for n, k in enumerate(kappas)]


def _run_jobs(ctx, z, jobs, batched):
    from ia_amd import _native
    L = z['L']
    S, IM = [dict() for _ in jobs], [dict() for _ in jobs]
    st = _native.Stats()
    for level in range(1, L):
        specs = [dict(B=z['B_pyr'][level], Bc=z['B_pyr'][level - 1], Bpc=Bp[level - 1], Bp=Bp[level],
                      weights=z['weights'], kappa_factor=1 + 2.0 ** (level - L) * k) for k, Bp in jobs]
        side = (z['A_pyr'][level], z['A_pyr'][level - 1], [p[level] for p in z['Ap_pyr']],
                [p[level - 1] for p in z['Ap_pyr']])
        res = ctx.synthesize_levels(*side, specs, st) if batched else \
            [ctx.synthesize_levels(*side, [sp], st)[0] for sp in specs]
        for j, (s, im) in enumerate(res):
            S[j][level], IM[j][level] = s, im
    return S, IM, st


@pytest.fixture(scope='module')
def g32_alone(octx):
    """the four g32 jobs run one at a time under the library defaults (computed once)"""
    z = _load('g32')
    jobs = _jobs_g32(z)
    with _options([octx], prune_min_rows=1):
        S, IM, _ = _run_jobs(octx, z, jobs, False)
    return S, IM, [Bp for _, Bp in jobs]


@pytest.mark.parametrize('setting', [(0, 0, 0), (1, 1, 1)], ids=['all_off', 'all_on'])
def test_batched_jobs_under_options(octx, g32_alone, setting):
    """ia_synthesize_levels, 4 jobs of g32, every level pruned: one handoff row set per job"""
    z = _load('g32')
    e, wt, pre = setting
    jobs = _jobs_g32(z)
    with _options([octx], prune_min_rows=1, early_gather=e, rec_wt=wt, prefetch_next=pre):
        S, IM, st = _run_jobs(octx, z, jobs, True)
    Sa, IMa, Bpa = g32_alone
    for j in range(len(jobs)):
        for level in range(1, z['L']):
            assert np.array_equal(S[j][level], Sa[j][level]) and np.array_equal(IM[j][level], IMa[j][level]), (j, level)
            assert np.array_equal(jobs[j][1][level], Bpa[j][level]), (j, level)
    for level in range(1, z['L']):   # job 0 is the reference's own run
        assert np.array_equal(S[0][level], z['s'][level]) and np.array_equal(IM[0][level], z['im'][level])
        assert np.array_equal(jobs[0][1][level], z['Bp_final'][level])
    assert st.bound_violations == 0 and st.kappa_ambiguous == 0
    assert st.pruned_levels == 4 * (z['L'] - 1)


@pytest.mark.parametrize('exchange', [0, 1], ids=['allgather', 'peerwrite'])
def test_emulated_shards_plain_record_stores(octx, exchange):
    """shard_emulate 2 with rec_wt 0: the multi-rank merge forms read the same records"""
    z = _load('g64')
    with _options([octx], prune_min_rows=1, rec_wt=0, shard_emulate=2, exchange=exchange):
        out, Bp, sts, st = _run(octx, z)
    _check_levels(z, out, Bp, st)
    assert st.pruned_levels == z['L'] - 1
    # the 64^2 level (128 DB tiles >= 64 W) really ran as two shards: two scans per step
    assert sts[z['L'] - 1].dist_launches == 2 * sts[z['L'] - 1].steps


# ---- 3. stamps = 1 changes nothing and reports sane numbers ----------------------------------------

STAMP_FIELDS = ('k3p_stamp_ms', 'k3p_stamp_launches', 'merge_stamp_ms', 'merge_stamp_launches', 'stamp_gap_ms',
                'stamp_gaps', 'stamp_window_ms', 'k3p_stamp_start_ms', 'k3p_stamp_wg_ms', 'stamp_gap_sm_ms',
                'stamp_gaps_sm')


def _check_stamps(sts):
    """The per-launch identities of include/ia.h on every level's own Stats (one job, one stream,
    k3p_variant 24, steps of <= 352 queries).  ia_level_run.cpp launches one pruned scan and one merge
    (fused or separate) per wavefront step on the context's stream, so k3p_stamp_launches ==
    dist_launches and merge_stamp_launches == steps; kernels of one stream do not overlap, so
    neither kind's summed device time can exceed the level's window (first scan start -> last
    kernel end)."""
    for level, st in sorted(sts.items()):
        print('level %d: %s' % (level, ' '.join('%s=%.6g' % (k, getattr(st, k)) for k in STAMP_FIELDS)),
              'dist_launches=%d steps=%d synth_ms=%.4f' % (st.dist_launches, st.steps, st.synth_ms))
        assert st.pruned_levels == 1
        assert st.k3p_stamp_launches > 0 and st.merge_stamp_launches > 0
        assert st.k3p_stamp_launches == st.dist_launches
        assert st.merge_stamp_launches == st.steps
        assert 0 <= st.k3p_stamp_start_ms <= st.k3p_stamp_ms
        assert 0 < st.k3p_stamp_wg_ms <= st.k3p_stamp_ms
        assert st.merge_stamp_ms > 0
        assert 0 <= st.stamp_gap_sm_ms <= st.stamp_gap_ms
        assert 0 <= st.stamp_gaps_sm <= st.stamp_gaps <= st.k3p_stamp_launches + st.merge_stamp_launches
        assert st.k3p_stamp_ms <= st.stamp_window_ms
        assert st.merge_stamp_ms <= st.stamp_window_ms


@pytest.mark.parametrize('setting', [(1, 1, 1, 1), (0, 0, 0, 0)], ids=_matrix_id)
@pytest.mark.parametrize('name', _have(['g256', 'ties128']))
def test_stamps_change_nothing(octx, name, setting):
    z = _load(name)
    e, wt, pre, nn = setting
    with _options([octx], prune_min_rows=1, stamps=1, early_gather=e, rec_wt=wt, prefetch_next=pre, nn_bound=nn):
        out, Bp, sts, st = _run(octx, z)
    _check_levels(z, out, Bp, st)
    _check_stamps(sts)


@pytest.mark.skipif(not _have(['g256']), reason='fixture g256 absent')
def test_stamp_slots_are_clean_for_the_next_run(octx):
    """The slots a level wrote are cleared when its call returns (StampSlots): after the stamped
    g256 (256 scan workgroups per launch) the stamped g64 (128 at most) on the same context must
    report its own launches only.  A stale slot shows up as a launch that "started" during the
    earlier run: a window reaching back over that run and the host time in between."""
    from ia_amd import _native
    z1, z2 = _load('g256'), _load('g64')
    with _options([octx], prune_min_rows=1, stamps=1):
        out1, Bp1, sts1, st1 = _run(octx, z1)
        out2, Bp2, sts2, st2 = _run(octx, z2)
    _check_levels(z1, out1, Bp1, st1)
    _check_levels(z2, out2, Bp2, st2)
    _check_stamps(sts2)
    print('stamp_window_ms %.4f, synth_ms %.4f after %.4f' % (st2.stamp_window_ms, st2.synth_ms, st1.synth_ms))
    assert st2.stamp_window_ms <= st2.synth_ms + st1.synth_ms
    # and with stamps off again every stamp field of a fresh Stats stays 0
    with _options([octx], prune_min_rows=1, stamps=0):
        L, k = z2['L'], float(z2['k'])
        Bp = [x.copy() for x in z2['Bp_init']]
        st = _native.Stats()
        for level in range(1, L):
            octx.synthesize_level(z2['A_pyr'][level], z2['A_pyr'][level - 1], [p[level] for p in z2['Ap_pyr']],
                                  [p[level - 1] for p in z2['Ap_pyr']], z2['B_pyr'][level], z2['B_pyr'][level - 1],
                                  Bp[level - 1], Bp[level], z2['weights'], 1 + 2.0 ** (level - L) * k, st)
    assert st.pruned_levels == L - 1
    for f in STAMP_FIELDS:
        assert getattr(st, f) == 0, f


# ---- 4. the composition the benchmark times, pinned to the reference -------------------------------

def _run_pipelined(ctxs, z):
    """as test_gpu_pipeline._run: device-resident levels through run_levels_pipelined"""
    from ia_amd import _native
    from ia_amd.pipeline import run_levels_pipelined
    from test_gpu_pipeline import _device_job, _level_fn
    d = _device_job(z, torch.device('cuda', 0))
    st = _native.Stats()
    run_levels_pipelined(_level_fn(z, d), ctxs, z['L'], st)
    torch.cuda.synchronize()
    L = z['L']
    return ([d['S'][l].cpu().numpy() for l in range(L)], [d['IM'][l].cpu().numpy() for l in range(L)],
            [d['Bp'][l].cpu().numpy() for l in range(L)], st)


def _check_pipelined(z, S, IM, Bp, st, pruned):
    for l in range(1, z['L']):
        assert np.array_equal(S[l], z['s'][l]) and np.array_equal(IM[l], z['im'][l]), l
        if 'Bp_final' in z:
            assert np.array_equal(Bp[l], z['Bp_final'][l]), l
        else:
            assert sha1_f64(Bp[l]) == z['sha1']['Bp_%d' % l], l
    assert st.bound_violations == 0
    assert st.pixels == sum(int(np.prod(z['B_pyr'][l].shape[:2])) for l in range(1, z['L']))
    assert st.pruned_levels == pruned


@pytest.mark.parametrize('stamps', [0, 1])
@pytest.mark.parametrize('name', _have(['g64', 'k25', 'ties128', 'g256']))
def test_bench_composition_matches_reference(bench4, name, stamps):
    z = _load(name)
    with _options(bench4, prune_min_rows=1, stamps=stamps):
        S, IM, Bp, st = _run_pipelined(bench4, z)
    _check_pipelined(z, S, IM, Bp, st, z['L'] - 1)


@pytest.mark.skipif('g512' not in SLIM_CASES, reason='fixture g512 absent')
def test_bench_composition_512_default_pruned(bench4):
    """bench.py's option set (prune_min_rows 262144, stamps 1 as in its timed steps) on the level
    size at which the product path prunes, against the reference run itself (slim fixture: s and
    im of every level, sha1 of every B' level)"""
    z = _load('g512')
    with _options(bench4, prune_min_rows=BENCH_PRUNE_MIN_ROWS, stamps=1):
        S, IM, Bp, st = _run_pipelined(bench4, z)
    _check_pipelined(z, S, IM, Bp, st, 1)


@pytest.mark.skipif(not _have(['g256']), reason='fixture g256 absent')
def test_bench_composition_coarse_separate_launches(bench4):
    """bench.py --coarse-fuse-gather 0: the three coarser contexts merge and gather separately"""
    z = _load('g256')
    with _options(bench4[1:], fuse_gather=0), _options(bench4, prune_min_rows=1, stamps=1):
        S, IM, Bp, st = _run_pipelined(bench4, z)
    _check_pipelined(z, S, IM, Bp, st, z['L'] - 1)

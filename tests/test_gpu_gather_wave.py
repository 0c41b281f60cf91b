"""Option "gather_wave" (include/ia.h; ia_kernels.hip merge_gather_pair, ia_gather.h
gather_wave_pre / gather_wave_post): the one-job, one-rank pruned early path of the fused merge +
gather launch as workgroups of a merge wave and a gather wave, against the reference's recorded
runs.  "Identical results for every setting" is the contract, so every comparison is bit-exact
against the golden fixtures (real reference runs): no tolerances but the one stated for a counter
that depends on the scan's dynamic tile hand-out.

With prune_min_rows = 1 every 1-channel level runs the pruned scan and the fused chain; the
pyramids of g32 and rect go down to 1x2, 2x3 and 4x4 levels, where the chain is refused (bw < 3)
or BOTH late pixels of the gather wave (its workgroup's own and the row above's) reflect into
several window slots: the smallest shapes at which the two-wave code can go wrong.

The module makes its own context and restores every option it sets."""
import contextlib
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

from golden_util import GOLDEN, PRUNE_MIN_ROWS_DEFAULT, check_debug_records, load_e2e

pytestmark = pytest.mark.gpu

# library defaults (include/ia.h) of every option this module touches
DEFAULTS = dict(gather_wave=1, early_gather=1, prefetch_next=1, nn_bound=1, prune_min_rows=PRUNE_MIN_ROWS_DEFAULT,
                k3p_variant=24, fuse_gather=1, fuse_sort=0, time_dist=0)


@contextlib.contextmanager
def _options(c, **opts):
    """set options; on exit each gets back the value it had (the library default where never set)"""
    assert set(opts) <= set(DEFAULTS)
    prev = {k: c.option(k, DEFAULTS[k]) for k in opts}
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        yield
    finally:
        for k, v in prev.items():
            c.set_option(k, v)


@pytest.fixture(scope='module')
def gctx():
    from ia_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _have(names):
    return [n for n in names if os.path.exists(os.path.join(GOLDEN, 'e2e_%s.npz' % n))]


_CACHE = {}


def _load(name):
    """each fixture read once per module run (never modified: runs copy Bp_init)"""
    if name not in _CACHE:
        _CACHE[name] = load_e2e(name)
    return _CACHE[name]


def _run(ctx, z):
    """every level in sequence with debug records; out[level] = (s, im, dbg), the B' pyramid and
    the Stats summed over the levels"""
    from ia_amd import _native
    L, k = z['L'], float(z['k'])
    Bp = [x.copy() for x in z['Bp_init']]
    out = {}
    st = _native.Stats()
    for level in range(1, L):
        dbg = {}
        s, im = ctx.synthesize_level(z['A_pyr'][level], z['A_pyr'][level - 1], [p[level] for p in z['Ap_pyr']],
                                     [p[level - 1] for p in z['Ap_pyr']], z['B_pyr'][level], z['B_pyr'][level - 1],
                                     Bp[level - 1], Bp[level], z['weights'], 1 + 2.0 ** (level - L) * k, st, debug=dbg)
        out[level] = (s, im, dbg)
    return out, Bp, st


# ---- 1. the option matrix against the reference's per-pixel records --------------------------------

MATRIX_CASES = _have(['g32', 'rect', 'g64', 'ties128', 'k25', 'g256'])
_TILE_SHARE = {}   # (gather_wave, nn_bound) -> g256's dist_tiles_rows / dist_tiles, for the tile-share test


@pytest.mark.parametrize('nn', [0, 1])
@pytest.mark.parametrize('gw', [0, 1])
@pytest.mark.parametrize('name', MATRIX_CASES)
def test_option_matrix_matches_reference_records(gctx, name, gw, nn):
    """gather_wave x nn_bound, every level on the pruned scan + fused merge / gather: s, im, B',
    every NN index, coherence pick and compute_distance value of the reference run.  With nn_bound 0
    the own pixel has one U' candidate row (its shifted source) instead of two."""
    z = _load(name)
    with _options(gctx, prune_min_rows=1, k3p_variant=24, gather_wave=gw, nn_bound=nn):
        out, Bp, st = _run(gctx, z)
    check_debug_records(z, out, Bp, st, name)
    assert st.pruned_levels == z['L'] - 1
    if name in ('g256', 'ties128'):   # pruning engages, so a too-small U' would drop the true NN
        print('%s gw%d nn%d: dist_pairs %.0f of %.0f' % (name, gw, nn, st.dist_pairs, st.dist_pairs_full))
        assert st.dist_pairs < st.dist_pairs_full
    if name == 'g256':
        _TILE_SHARE[(gw, nn)] = st.dist_tiles_rows / st.dist_tiles


@pytest.mark.skipif(not _have(['g256']), reason='fixture g256 absent')
@pytest.mark.parametrize('nn', [0, 1])
def test_tile_share_unchanged(gctx, nn):
    """U' of the gather wave runs over the same candidate rows as the one-wave early gather's (only
    the summation order of the own pixel's terms differs), so the share of DB tiles whose rows the
    scan visits does not move.  1 % relative: the slack granted to counters that depend on the
    scan's dynamic tile hand-out, not a measurement."""
    z = _load('g256')
    for gw in (0, 1):
        if (gw, nn) not in _TILE_SHARE:   # (run alone: the matrix test did not fill it)
            with _options(gctx, prune_min_rows=1, k3p_variant=24, gather_wave=gw, nn_bound=nn):
                _, _, st = _run(gctx, z)
            _TILE_SHARE[(gw, nn)] = st.dist_tiles_rows / st.dist_tiles
    one, two = _TILE_SHARE[(0, nn)], _TILE_SHARE[(1, nn)]
    print('g256 nn%d: dist_tiles_rows / dist_tiles one-wave %.6f two-wave %.6f' % (nn, one, two))
    assert 0 < one <= 1
    assert abs(two - one) <= 0.01 * one


# ---- 2. where the two-wave launches meet other paths -----------------------------------------------

SMALL = _have(['g64', 'ties128'])


@pytest.mark.parametrize('name', SMALL)
def test_gather_wave_with_sampled_steps(gctx, name):
    """time_dist 3: every third step and the one before it run the separate gather and merge
    launches, so two-wave fused steps and separate launches alternate within a level and hand off
    row to row"""
    z = _load(name)
    with _options(gctx, prune_min_rows=1, gather_wave=1, time_dist=3):
        out, Bp, st = _run(gctx, z)
    check_debug_records(z, out, Bp, st, name)
    assert st.pruned_levels == z['L'] - 1
    assert st.dist_launches_timed > 0 and st.merge_launches_timed > 0   # the sampled steps ran


@pytest.mark.skipif(not _have(['g64']), reason='fixture g64 absent')
@pytest.mark.parametrize('other', [dict(fuse_gather=0), dict(fuse_sort=1), dict(early_gather=0), dict(prefetch_next=0)],
                         ids=lambda d: '%s%d' % next(iter(d.items())))
def test_gather_wave_inert(gctx, other):
    """settings under which the early path does not run: gather_wave 1 changes nothing, the
    one-wave launches (or the separate ones) run"""
    z = _load('g64')
    with _options(gctx, prune_min_rows=1, gather_wave=1, **other):
        out, Bp, st = _run(gctx, z)
    check_debug_records(z, out, Bp, st, 'g64')
    assert st.pruned_levels == z['L'] - 1


def _jobs_g32(z, kappas=(0.5, 5.0, 25.0, 1.0)):
    """as test_gpu_options._jobs_g32: the golden g32 job (k = 0.5, the reference's B' init) + three
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


@pytest.mark.skipif(not _have(['g32']), reason='fixture g32 absent')
def test_batched_jobs_equal_per_job_runs(gctx):
    """ia_synthesize_levels, 4 jobs of g32 in one batch (the multi-job instance, one wave per query)
    against the same jobs one at a time (two-wave workgroups), every level pruned"""
    z = _load('g32')
    alone, batch = _jobs_g32(z), _jobs_g32(z)
    with _options(gctx, prune_min_rows=1, gather_wave=1):
        Sa, IMa, _ = _run_jobs(gctx, z, alone, False)
        S, IM, st = _run_jobs(gctx, z, batch, True)
    for j in range(len(batch)):
        for level in range(1, z['L']):
            assert np.array_equal(S[j][level], Sa[j][level]) and np.array_equal(IM[j][level], IMa[j][level]), (j, level)
            assert np.array_equal(batch[j][1][level], alone[j][1][level]), (j, level)
    for level in range(1, z['L']):   # job 0 is the reference's own run
        assert np.array_equal(S[0][level], z['s'][level]) and np.array_equal(IM[0][level], z['im'][level])
        assert np.array_equal(batch[0][1][level], z['Bp_final'][level])
    assert st.bound_violations == 0 and st.kappa_ambiguous == 0
    assert st.pruned_levels == 4 * (z['L'] - 1)

"""Time masked resynthesis against the window call on the finest level of
synth.make_job(size), in one process on one context.  The coarser levels run once through the default
call and give the finest level's B' level l - 1; then, per window sizes of --wins:

  * nbhd       ia_synthesize_levels_nbhd on the finest level (the baseline, and the state the regions start from);
  * full       ia_synthesize_levels_masked, an all-ones mask from the initial B' without sources;
  * c256, c128, c32   centred square regions of those sides, from nbhd's finished state;
  * rand1      a random 1 % mask (seeded), from that state.

The runs alternate round by round after one warm-up round; reported per run: the median over the rounds of the
device time between the level's events (ia_stats.synth_ms: the step loop, the list's fill pass included; db_ms:
the DB build), of the step lists' device time (ia_masked_stats: count, scan and fill passes) and of the host
clock around the synchronous call (uploads and read-backs of host arrays included), the spread of synth_ms, and
the steps run, scans launched and pixels.  Regions are also checked to leave the state unchanged (the
idempotence property), so the numbers belong to a correct run.

Prints one JSON line.
  python3 tools/mask_timing.py [--size 1024] [--wins 3x5,3x7] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ia_amd  # noqa: F401,E402
from ia_amd import _native, config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=1024)
ap.add_argument('--wins', default='3x5,3x7')
ap.add_argument('--rounds', type=int, default=3)
a = ap.parse_args()
WINS = [tuple(int(v) for v in x.split('x')) for x in a.wins.split(',')]

job = synth.make_job(a.size)
L, fin = job.L, job.L - 1
ctx = _native.Context(0)
Bp0 = [np.ascontiguousarray(x, dtype=np.float64).copy() for x in job.Bp_init]
for level in range(1, fin):          # B' level fin - 1, once, by the default call
    ctx.synthesize_level(job.A_levels(level), job.A_levels(level - 1), [p[level] for p in job.Ap_pyr_list],
                         [p[level - 1] for p in job.Ap_pyr_list], job.B_pyr[level], job.B_pyr[level - 1], Bp0[level - 1],
                         Bp0[level], job.weights, job.kappa_factor(level))
h, w = job.B_pyr[fin].shape[:2]
a_side = (job.A_levels(fin), job.A_levels(fin - 1), [p[fin] for p in job.Ap_pyr_list], [p[fin - 1] for p in job.Ap_pyr_list])


def centred(side):
    m = np.zeros((h, w), dtype=bool)
    side = min(side, h, w)
    m[(h - side) // 2:(h - side) // 2 + side, (w - side) // 2:(w - side) // 2 + side] = True
    return m


MASKS = [('full', np.ones((h, w), dtype=bool)), ('c256', centred(256)), ('c128', centred(128)), ('c32', centred(32)),
         ('rand1', np.random.RandomState(17).rand(h, w) < 0.01)]
MASKS[-1][1][:4, :] = MASKS[-1][1][:, :4] = False      # (inside rows and columns >= p_l, as the property asks)


def level_job(weights, Bp):
    return dict(B=job.B_pyr[fin], Bc=job.B_pyr[fin - 1], Bpc=Bp0[fin - 1], Bp=Bp, weights=weights,
                kappa_factor=job.kappa_factor(fin))


def timed(call):
    """(result, dict of the call's times and counters)"""
    st = _native.Stats()
    n0, l0 = ctx.masked_stats()
    t0 = time.perf_counter()
    res = call(st)
    wall = 1e3 * (time.perf_counter() - t0)
    return res, dict(wall_ms=wall, synth_ms=st.synth_ms, db_ms=st.db_ms, list_ms=ctx.masked_stats()[1] - l0, steps=int(st.steps),
                     scans=int(st.dist_launches), pixels=int(st.pixels))


report = {}
for win in WINS:
    weights = config.compute_weights(win[0], win[1], (win[1] * win[1]) // 2, 1)
    state = {}

    def run_nbhd():
        Bp = Bp0[fin].copy()
        (s, im), t = timed(lambda st: ctx.synthesize_levels(*a_side, [level_job(weights, Bp)], st, windows=win)[0])
        state.update(s=s, im=im, Bp=Bp)
        return t

    def run_mask(name, mask):
        full = name == 'full'
        Bp = (Bp0[fin] if full else state['Bp']).copy()
        jb = dict(level_job(weights, Bp), mask=mask, s=None if full else state['s'], im=None if full else state['im'])
        (s, im), t = timed(lambda st: ctx.resynthesize_levels(*a_side, [jb], windows=win, stats=st)[0])
        # full: the window call's result; a region (rows and columns >= p_l): the state is a fixed point
        t['equals_state'] = bool(np.array_equal(s, state['s']) and np.array_equal(im, state['im']) and np.array_equal(Bp, state['Bp']))
        return t

    runs = [('nbhd', run_nbhd)] + [(n, (lambda n, m: lambda: run_mask(n, m))(n, m)) for n, m in MASKS]
    for _, f in runs:                # warm every shape
        f()
    times = {n: [] for n, _ in runs}
    for _ in range(a.rounds):
        for n, f in runs:
            times[n].append(f())
    med = lambda xs: round(float(np.median(xs)), 3)
    rep = {}
    for n, _ in runs:
        ts = times[n]
        rep[n] = dict(synth_ms=med([t['synth_ms'] for t in ts]), synth_ms_min_max=[round(min(t['synth_ms'] for t in ts), 3),
                                                                                   round(max(t['synth_ms'] for t in ts), 3)],
                      db_ms=med([t['db_ms'] for t in ts]), list_ms=med([t['list_ms'] for t in ts]),
                      wall_ms=med([t['wall_ms'] for t in ts]), steps=ts[-1]['steps'], scans=ts[-1]['scans'], pixels=ts[-1]['pixels'])
        if n != 'nbhd':
            rep[n]['equals_state'] = all(t['equals_state'] for t in ts)
    report['%dx%d' % win] = rep
    print('%dx%d: %s' % (win + (json.dumps(rep),)), file=sys.stderr, flush=True)
ctx.close()
print(json.dumps({'size': a.size, 'level': [h, w], 'rounds': a.rounds, 'runs': report}), flush=True)

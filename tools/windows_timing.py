"""Time the exact level for other window sizes (ia_synthesize_levels_nbhd) on the finest
level of synth.make_job(size): one process, one context, levels one after the other.

Per variant - (3, 5) through the default call, (3, 5) through the new call, then each of --windows through
the new call - the coarser levels run once (their B' feeds the finest level), the finest level once to warm
up and then --rounds times from the same initial B'; the device time between the level's events
(ia_stats.synth_ms, db_ms), median and spread.  Beside it what the new path's cost model predicts from:
launches per step (gather, query prep, scan blocks, merge, finish) and the fp32 tile DB a step streams.

Prints one JSON line.
  python3 tools/windows_timing.py [--size 1024] [--windows 3x3,3x7,3x9] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ia_amd  # noqa: F401,E402
from ia_amd import _native, config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=1024)
ap.add_argument('--windows', default='3x3,3x7,3x9')
ap.add_argument('--rounds', type=int, default=3)
a = ap.parse_args()
WINS = [tuple(int(v) for v in x.split('x')) for x in a.windows.split(',')]

job = synth.make_job(a.size)
L = job.L
fin = L - 1
ctx = _native.Context(0)


def level(lv, Bp, st, win, wts):
    Bp[lv] = np.ascontiguousarray(Bp[lv], dtype=np.float64)
    return ctx.synthesize_level(job.A_levels(lv), job.A_levels(lv - 1), [p[lv] for p in job.Ap_pyr_list],
                                [p[lv - 1] for p in job.Ap_pyr_list], job.B_pyr[lv], job.B_pyr[lv - 1], Bp[lv - 1], Bp[lv], wts,
                                job.kappa_factor(lv), st, windows=win)


def variant(win, new_call):
    wts = job.weights if win == (3, 5) else config.compute_weights(win[0], win[1], (win[1] * win[1]) // 2, 1)
    w = win if new_call else None
    Bp = [x.copy() for x in job.Bp_init]
    for lv in range(1, fin):
        level(lv, Bp, _native.Stats(), w, wts)
    runs, last = [], None
    for i in range(a.rounds + 1):        # the first one warms up
        Bp[fin] = job.Bp_init[fin].copy()
        st = _native.Stats()
        s, im = level(fin, Bp, st, w, wts)
        if i:
            runs.append((st.synth_ms, st.db_ms))
        last = (s, st)
    syn, db = [r[0] for r in runs], [r[1] for r in runs]
    st = last[1]
    h, wd = job.B_pyr[fin].shape[:2]
    rows = len(job.Ap_pyr_list) * int(np.prod(job.Ap_pyr_list[0][fin].shape[:2]))
    out = dict(windows='%dx%d' % win, call='nbhd' if new_call else 'default', D=_native.feature_width(win[0], win[1], 1),
               finest_synth_ms=round(float(np.median(syn)), 3), finest_synth_ms_min_max=[round(min(syn), 3), round(max(syn), 3)],
               finest_db_ms=round(float(np.median(db)), 3), steps=int(st.steps), pixels=int(st.pixels),
               coherence_wins=int(st.coherence_wins), us_per_step=round(1e3 * float(np.median(syn)) / max(int(st.steps), 1), 2))
    if new_call:
        D = out['D']
        KH = 28 if D + 1 <= 56 else 56 if D + 1 <= 112 else 84
        T, _ = _native.wavefront_shape_pad(h, wd, win[1] // 2)
        full = sum(1 for t in range(T) if _native.wavefront_step_pad(h, wd, win[1] // 2, t)[1] > 0)
        out.update(KH=KH, launches_per_step=round(4 + st.dist_launches / max(full, 1), 3),
                   db_bytes_per_step=-(-rows // 32) * 32 * 2 * KH * 4,
                   db_gb_per_s=round(-(-rows // 32) * 32 * 2 * KH * 4 * st.dist_launches / (float(np.median(syn)) * 1e6), 1))
    return out, last[0]


report = []
r0, s0 = variant((3, 5), False)
r1, s1 = variant((3, 5), True)
r1['equals_default_call'] = bool(np.array_equal(s0, s1))
report += [r0, r1]
for win in WINS:
    report.append(variant(win, True)[0])
ctx.close()
print(json.dumps({'size': a.size, 'levels': L, 'rounds': a.rounds, 'runs': report}), flush=True)

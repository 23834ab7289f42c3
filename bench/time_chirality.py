"""Time of the chirality veto on one GPU.

  bench/time_chirality.py kernel [C1 C3 C4 ...]   device events around the depth kernels: the full pass of point_depths()
                                                  (depths scattered to IP order, minima per image, argmin) and the
                                                  veto's own pass (count and minimum only), per scene
  bench/time_chirality.py loop [C3] [--reps N]    the shipped 'lm' loop from the scene's start, veto off and veto on,
                                                  alternating, N solves each after one warm-up of each: median and
                                                  range of the solve's wall time (dbat_hip_result.time_s), iterations,
                                                  trial points tested
  bench/time_chirality.py loop C3 --plain         the same loop through the calls every earlier build has as well
                                                  (no veto): run from a checkout of the parent commit, with this file
                                                  copied in, it times the parent's loop on the same scene
Repetitions and spread follow the house rules for these machines: warm-up first, the two variants interleaved so that
clock and cache drift hit both, medians with their range, nothing compared across processes without saying so."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from dbat_amd import synth, _hip


def med(v):
    v = np.asarray(v, float)
    return '%.3f (%.3f .. %.3f)' % (np.median(v), v.min(), v.max())


def kernel(names):
    for name in names:
        s = synth.make_scene(name)[0]
        h = _hip.Handle(s)
        try:
            x = h.serialize()
            full, light = [], []
            for i in range(6):                         # (the first call builds the depth plan and its scratch arrays)
                depth, image_min, n_behind, min_depth, argmin = h.point_depths(x)
                if i:
                    full.append(h.point_depths_ms())
                    light.append(h.chirality_pass_ms(x, 20)[0])
            print('%s images %d nObs %d: point_depths kernels %s ms, veto pass %s ms (median, range of 5; the veto pass a mean '
                  'of 20 each); n_behind %d min_depth %.4f at column %d'
                  % (name, len(image_min), len(depth), med(full), med(light), n_behind, min_depth, argmin), flush=True)
        finally:
            h.close()


def loop(name, reps, plain):
    s = synth.make_scene(name)[0]
    h = _hip.Handle(s)
    try:
        x0 = h.serialize()
        opt = _hip.default_options('lm')
        opt.store_trace = 0
        rows = {False: [], True: []}
        for i in range(reps + 1):
            for on in ((False,) if plain else (False, True)):
                if not plain:
                    h.set_chirality(on)
                x, res, rr, damp, aux, T = h.solve(x0, opt)
                tested = 0 if plain else h.chirality_stats()[0]
                if i:
                    rows[on].append((res.time_s * 1e3, res.iters, res.code, tested, res.n_residual_evals))
        for on, r in rows.items():
            if not r:
                continue
            t = [a[0] for a in r]
            print("%s 'lm' loop, veto %s: %s ms (median, range of %d); iterations %d code %d residual evaluations %d "
                  'trial points tested %d; per iteration %.3f ms'
                  % (name, 'on' if on else ('off' if not plain else 'absent'), med(t), len(t), r[0][1], r[0][2], r[0][4], r[0][3],
                     np.median(t) / max(r[0][1], 1)), flush=True)
        if rows[True]:
            d = np.median([a[0] for a in rows[True]]) - np.median([a[0] for a in rows[False]])
            print('%s veto on - veto off: %.3f ms over %d trial points = %.4f ms per trial point'
                  % (name, d, rows[True][0][3], d / max(rows[True][0][3], 1)), flush=True)
    finally:
        h.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('kernel', 'loop'))
    ap.add_argument('scenes', nargs='*')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--plain', action='store_true')
    a = ap.parse_args()
    if a.mode == 'kernel':
        kernel(a.scenes or ['C1', 'C3'])
    else:
        for nm in a.scenes or ['C3']:
            loop(nm, a.reps, a.plain)

"""Cost of robust bundle() (dbat_hip_solve_robust) on one GPU: one reweighting (residual pass, norm, exact median by
radix select, weights, apply) from the difference of two robust solves with 1 and 3 reweightings (tol 0, so every
evaluation is applied), the step time with per-observation weights (set_obs_weights(ones), then bench_step) against
the uniform path, and the device memory the promotion adds.
bench/time_robust.py [C3 | C1 | camcal ...] (several scenes in one run)."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from dbat_amd import synth, _hip


def scene(name):
    if name == 'camcal':
        from helpers import camcal_struct
        return camcal_struct()
    return synth.make_scene(name)[0]


def step_ms(h, n=20):
    h.bench_step()
    ms = [h.bench_step()[:4].sum() for _ in range(n)]
    return float(np.median(ms))


for name in sys.argv[1:] or ['C3']:
    s = scene(name)
    h = _hip.Handle(s)
    try:
        x0 = h.serialize()
        no = s.IP.val.shape[1]
        h.set_x(x0)
        uni = [step_ms(h)]
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        h.set_obs_weights(np.ones(no))
        free1 = torch.cuda.mem_get_info()[0]
        h.set_x(x0)
        pw = [step_ms(h)]
        h.set_obs_weights(None)
        h.set_x(x0)
        uni.append(step_ms(h))
        h.set_obs_weights(np.ones(no))
        h.set_x(x0)
        pw.append(step_ms(h))
        opt = _hip.default_options('gna')
        opt.store_trace = 0
        t = {}
        for mo in (1, 3):
            rs = []
            for _ in range(2):
                ro = _hip.robust_options('cauchy', scale='mad', max_outer=mo, weight_tol=0.0)
                out = h.solve_robust(x0, opt, ro)
                rs.append(out[6].reweight_s)
            t[mo] = min(rs)
        per = (t[3] - t[1]) / 2
        print('%s nObs %d: reweight %.3f ms  step uniform %.3f ms  per-observation weights %.3f ms (x %.3f)  '
              'promotion +%.0f MB' % (name, no, 1e3 * per, np.mean(uni), np.mean(pw), np.mean(pw) / np.mean(uni),
                                       (free0 - free1) / 2 ** 20), flush=True)
    finally:
        h.close()

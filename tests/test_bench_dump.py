"""bench.py --dump-outputs DIR: what the timed step computes, written as .npy files so that two builds can be compared
output for output -- the sampling of long vectors on the host, and (GPU) the dumped step of a real run against the oracle's
full sparse solve of the same damped normal equations."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


class _FakeHandle:
    """linearize_solve / residual of a problem with n parameters and m residuals (no GPU)."""

    def __init__(self, n, m):
        self.n, self.m, self.calls = n, m, []

    def linearize_solve(self, x, lam, scale):
        self.calls.append(('linearize_solve', lam, scale))
        return np.arange(self.n, dtype=np.float64) * 0.5, dict(f=2.0, JpJp=3.0, rJp=-4.0, pp=5.0, trace=6.0)

    def residual(self, x):
        self.calls.append(('residual',))
        return -np.arange(self.m, dtype=np.float64) - x[0], 1.5


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_samples_long_vectors_with_a_fixed_seed(tmp_path):
    bench = _bench_module()
    cap = bench.DUMP_MAX_ELEMENTS
    n, m = 1000, cap + 12345
    x0 = np.full(n, 7.0)
    h = _FakeHandle(n, m)
    info = bench.dump_outputs(h, x0, 1e-3, str(tmp_path / 'a'), True)
    assert h.calls == [('linearize_solve', 1e-3, False), ('residual',)]
    a = tmp_path / 'a'
    sc = np.load(a / 'scalars.npy')
    assert sc.dtype == np.float64 and list(sc) == [2.0, 3.0, -4.0, 5.0, 6.0, 1.5]
    step = np.load(a / 'step.npy')
    assert step.dtype == np.float64 and np.array_equal(step, np.arange(n) * 0.5)
    assert not (a / 'step_index.npy').exists() and 'sampled' not in info['arrays']['step']
    r, idx = np.load(a / 'trial_residual.npy'), np.load(a / 'trial_residual_index.npy')
    assert r.dtype == np.float64 and idx.dtype == np.float64 and r.size == idx.size == cap
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < m
    # x0 + step: element 0 of the trial point is 7.0
    assert np.array_equal(r, -idx - 7.0)
    assert info['arrays']['trial_residual'] == {'shape': [m], 'sampled': cap}
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert total <= 64 * 2 ** 20
    # the same sample every time
    bench.dump_outputs(_FakeHandle(n, m), x0, 1e-3, str(tmp_path / 'b'), True)
    assert np.array_equal(np.load(tmp_path / 'b' / 'trial_residual_index.npy'), idx)
    # a rank that does not write still takes part in the (collective) calls
    h2 = _FakeHandle(n, m)
    assert bench.dump_outputs(h2, x0, 1e-3, str(tmp_path / 'c'), False) is None
    assert len(h2.calls) == 2 and not (tmp_path / 'c').exists()


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, BENCH, '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and '--steps' in r.stderr


@pytest.mark.gpu
def test_dumped_step_matches_the_oracle(tmp_path):
    """Two runs of the same command dump the same outputs, and the dumped step is the oracle's damped step at the
    bench's start point with the bench's damping 1e-10 * trace(J'J) / n (levenberg_marquardt.m:88-95,119)."""
    import scipy.sparse as sp
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import dbat_oracle as o
    from dbat_amd import synth
    outs = []
    for k in range(2):
        d = tmp_path / ('run%d' % k)
        r = subprocess.run([sys.executable, BENCH, '--config', 'tiny', '--steps', '3', '--warmup', '1', '--no-cpu-baseline',
                            '--no-solve', '--dump-outputs', str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j['steps'] == 3 and j['ms_per_step'] > 0 and j['dump_outputs']['dir'] == str(d)
        outs.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = outs
    assert sorted(a) == ['scalars', 'step', 'trial_residual']
    for k in a:
        assert a[k].dtype == np.float64
        assert np.linalg.norm(a[k] - b[k]) <= 1e-10 * np.linalg.norm(a[k])

    s = copy.deepcopy(synth.make_scene('tiny')[0])
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(s.bundle.est, nm), bool)
    so = o.buildserialindices(s)
    x0, w = o.serialize(so), o.buildweightvector(so)
    r_o, K = o.brown_euler_cam4(x0, so, jac=True)
    R = np.sqrt(w)
    r = R * r_o
    J = (sp.diags(R) @ K).tocsc()
    JTJ = (J.T @ J).tocsc()
    n = J.shape[1]
    lam = 1e-10 * JTJ.diagonal().sum() / n
    p_o, _ = o.normal_solve((JTJ + lam * sp.identity(n)).tocsc(), -(J.T @ r))
    assert np.linalg.norm(a['step'] - p_o) <= 1e-8 * np.linalg.norm(p_o)
    f, JpJp, rJp, pp, trace, f_trial = a['scalars']
    assert abs(f - 0.5 * r @ r) <= 1e-11 * f
    assert abs(trace - JTJ.diagonal().sum()) <= 1e-10 * trace
    r_t = o.brown_euler_cam4(x0 + p_o, so)
    assert np.linalg.norm(a['trial_residual'] - r_t) <= 1e-7 * np.linalg.norm(r_t)
    assert abs(f_trial - 0.5 * np.sum(w * r_t ** 2)) <= 1e-8 * f_trial

"""Host-only checks of the batch layout when most points are seen in ONE image (tests/helpers.py crowded_struct): a
batch is cut at BT observations, and the plan must also close it at Plan::PMAX = 128 points, the per-point room in LDS
of k_build_tile2, k_build_tile3 and k_heavy_z.  closed_by_cap > 0 means that without the cap a batch would have held more
than 128 points: these scenes reach the overflow the cap prevents.  Scenes whose points all have two or more rays never
reach the cap, so their plans are the ones built without it.  No GPU (dbat_hip_debug_batch_stats); the kernels on
these scenes: tests/test_crowded_batches_gpu.py."""
import pytest

from helpers import CROWDED_KINDS, crowded_struct, synth_struct

# route: (environment, self-calibration, cameras of the control point, (cameras, points)).  Heavy routes: few enough points
# (20 cameras: at most 2048 observations besides the control point's) to join the control point on the heavy route.
ROUTES = {
    'sig': ({}, False, 0, (60, 3000)),
    'tile3': ({'DBAT_HIP_SIG': '0'}, False, 0, (60, 3000)),
    'tile2': ({'DBAT_HIP_SIG': '0'}, True, 0, (60, 3000)),
    'heavy': ({'DBAT_HIP_CMAX': '6'}, False, 12, (20, 700)),
    'heavy-selfcal': ({'DBAT_HIP_CMAX': '6'}, True, 12, (20, 700)),
    'columns': ({'DBAT_HIP_CMAX': '6', 'DBAT_HIP_HEAVY': '0', 'DBAT_HIP_SIG': '0'}, False, 12, (60, 3000)),
    'columns-selfcal': ({'DBAT_HIP_CMAX': '6', 'DBAT_HIP_HEAVY': '0', 'DBAT_HIP_SIG': '0'}, True, 12, (60, 3000)),
    'bt128': ({'DBAT_HIP_BT': '128'}, False, 0, (60, 3000)),
}


def _limits(st):
    for part in ('tiled', 'untiled'):
        assert st[part]['max_points'] <= st['PMAX'] == 128, st
        assert st[part]['max_obs'] <= st['BT'], st
    assert st['tiled']['max_tile_batches'] <= min(48, st['tile_bmax']), st


@pytest.mark.parametrize('kind', CROWDED_KINDS)
@pytest.mark.parametrize('route', list(ROUTES))
def test_crowded_batches_stay_within_the_point_cap(route, kind, monkeypatch):
    from dbat_amd import _hip
    env, selfcal, control, size = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, _ = crowded_struct(kind, selfcal=selfcal, control=control, cams=size[0], points=size[1])
    st = _hip.batch_stats(s)
    _limits(st)
    hv = _hip.heavy_plan_selftest(s)
    if route.startswith('heavy'):
        # every point on the heavy route: the batches after the (absent) tiles reach the cap
        assert st['n_batches_tiled'] == 0 and st['untiled']['closed_by_cap'] > 0
        assert hv['on'] and hv['tasks'] > 0 and hv['points'] == s.OP.val.shape[1]
        assert hv['max_diff'] <= 1e-10 * max(hv['max_abs'], 1.0), hv
    elif route == 'bt128':
        # nothing tiled; a 128-observation batch never holds more than 128 points
        assert st['n_batches_tiled'] == 0 and st['untiled']['closed_by_cap'] == 0 and not hv['on']
    else:
        assert st['n_batches_tiled'] > 0 and st['tiled']['closed_by_cap'] > 0 and not hv['on']
        assert st['tiled']['max_points'] == 128
        if control:                                     # the control point alone, by column lists
            assert st['n_batches_untiled'] == 1 and st['untiled']['max_obs'] == control


def test_tiles_count_batches_closed_by_the_cap():
    """A tile is capped at tile_bmax batches whatever closed them: runs of single-ray points close batches on the point
    cap alone, long before the observations would."""
    from dbat_amd import _hip
    for n in (3000, 6000):
        s, _ = crowded_struct('fixed', frac=1.0, cams=30, points=n)
        st = _hip.batch_stats(s)
        _limits(st)
        assert st['tiled']['closed_by_cap'] >= st['n_batches_tiled'] // 2
        assert st['tiled']['max_tile_batches'] == st['tile_bmax']


ORDINARY = ([(n, v, cmax) for n in ('tiny', 'small') for v in ('plain', 'selfcal', 'imagevar', 'priors', 'groups4')
             for cmax in (None, '6')] + [('C1', 'plain', None)])


@pytest.mark.parametrize('name,variant,cmax', ORDINARY)
def test_cap_leaves_ordinary_plans_alone(name, variant, cmax, monkeypatch):
    """Every point with two or more rays: no batch is closed by the cap, so the plan is the one built without it."""
    from dbat_amd import _hip
    if cmax:
        monkeypatch.setenv('DBAT_HIP_CMAX', cmax)
    s, _ = synth_struct(name, variant)
    st = _hip.batch_stats(s)
    _limits(st)
    assert st['tiled']['closed_by_cap'] == 0 and st['untiled']['closed_by_cap'] == 0

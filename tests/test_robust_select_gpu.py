"""The select and weight kernels of the robust reweighting (csrc/robust.hpp: k_rsel_hist, k_rsel_pick, k_rsel_to_f64,
k_robust_weight) and robust_median() on crafted values, through dbat_hip_debug_robust_from_s: the product code of a
solve from the bit patterns on, fed the values of tests/robust_select_cases.py instead of residuals.  The structs
only carry a count: 1800 image points (one select workgroup), 1799 (a ragged last wave) and 32 000 (8 select and 125
weight workgroups); the ranks run on the scenes of test_multishard_gpu.py.

Exact median and scale for ties, the two targets parting in each of the six passes, histograms crowded in one pass,
zeros and subnormals; the weights against the definition; the largest weight change bit for bit wherever it sits in
a wave or workgroup, on a fresh and on a promoted handle; what is refused; that nothing is applied; 2 and 4 ranks,
ranks that hold only one end of the order or nothing at all.

Not reached by tests of a few seconds: counts of 2^31 observations and beyond, and the select's cap of 1024
workgroups (more than 4 M observations on a rank), where a workgroup's stride loop takes further rounds."""
import functools

import numpy as np
import pytest

import robust_select_cases as rc
from helpers import synth_struct
from test_robust_gpu import _drop_last_ip

pytestmark = pytest.mark.gpu

LOSSES = (('huber', 'mad'), ('cauchy', 'mad'), ('huber', 'apriori'))
PARAMS = [(n, c) for n in rc.SIZES for c in rc.case_ids(n)]
IDS = ['%d-%s' % p for p in PARAMS]


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


def _struct(n):
    s = {1800: lambda: synth_struct('tiny', 'plain')[0], 1799: lambda: _drop_last_ip(synth_struct('tiny', 'plain')[0]),
         32000: lambda: synth_struct('small', 'plain')[0]}[n]()
    assert s.IP.val.shape[1] == n
    return s


@pytest.fixture(scope='module')
def handle(hip):
    """handle(n): one handle per size, shared by the tests of this module (left unpromoted by each of them)."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = hip.Handle(_struct(n))
        return made[n]
    yield get
    for h in made.values():
        h.close()


@functools.lru_cache(maxsize=None)
def _cases(n):
    d = dict(rc.cases(n))
    for v in d.values():
        v.setflags(write=False)
    return d


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize('n,case', PARAMS, ids=IDS)
def test_median_and_scale_are_exact(hip, handle, n, case):
    s = _cases(n)[case]
    om, med, sc, chg, owned = handle(n).debug_robust_from_s(s, hip.robust_options('cauchy', scale='mad'))
    ref_med, ref_sc = rc.ref_median(s), rc.ref_scale(s)
    print('%s n=%d: median %r (reference %r), scale %r (reference %r)' % (case, n, med, ref_med, sc, ref_sc))
    assert med == ref_med
    assert sc == ref_sc
    assert sc == 1.0 or ref_med != 0
    assert np.all(owned) and owned.shape == (n,)


@pytest.mark.parametrize('n,case', PARAMS, ids=IDS)
def test_weights_match_the_definition(hip, handle, n, case):
    """omega within 1e-12 (the bound of test_weights_at_x0_match_numpy; omega <= 1) of robust_weight_fn(s / scale), never
    NaN, in [0, 1].  On cluster0 and extremes u = s / scale reaches 2^1000 and beyond: (u / k)^2 overflows and the
    Cauchy weight is exactly 0, outside the (0, 1] of the header -- on the device as in the reference.  Recorded here,
    not a defect of the select."""
    s = _cases(n)[case]
    for loss, sm in LOSSES:
        ro = hip.robust_options(loss, scale=sm)
        om, med, sc, chg, _ = handle(n).debug_robust_from_s(s, ro)
        ref_sc = rc.ref_scale(s, sm)
        ref = rc.ref_weights(s, ref_sc, loss, ro.k)
        err = np.abs(om - ref).max()
        print('%s n=%d %s/%s: scale %r, omega off by %.2e, min omega %r' % (case, n, loss, sm, sc, err, om.min()))
        assert sc == ref_sc and (np.isnan(med) if sm == 'apriori' else med == rc.ref_median(s))
        assert not np.any(np.isnan(om)) and np.all((om >= 0) & (om <= 1))
        assert err <= 1e-12, (loss, sm)
        assert np.all(om[s == 0] == 1.0)
        if loss == 'cauchy' and case in ('cluster0', 'extremes'):
            assert np.any(om == 0) and np.any(ref == 0)


@pytest.mark.parametrize('n', rc.SIZES)
def test_huber_threshold_and_zero_give_one(hip, handle, n):
    s = rc.rayleigh(n) + 1.0
    s[::7] = 1.5
    s[3::11] = 0.0
    om = handle(n).debug_robust_from_s(s, hip.robust_options('huber', k=1.5, scale='apriori'))[0]
    assert np.all(om[s == 1.5] == 1.0) and np.all(om[s == 0] == 1.0) and np.all(om[s > 1.5] < 1.0)
    for loss, sm in (('cauchy', 'apriori'), ('cauchy', 'mad'), ('huber', 'mad')):
        om = handle(n).debug_robust_from_s(s, hip.robust_options(loss, scale=sm))[0]
        assert np.all(om[s == 0] == 1.0) and np.count_nonzero(om == 1.0) >= np.count_nonzero(s == 0)


def _om_prev(n):
    return np.random.default_rng(77).uniform(0.5, 1.0, n)


def _moving_columns(n):
    return [0, 63, 64, 255, 256, n - 1] + sorted(np.random.default_rng(78).choice(n, 5, replace=False).tolist())


def test_max_change_on_a_fresh_handle(hip, handle):
    """Never promoted: the change is measured against 1.  Subtraction, absolute value and maximum are exact, so the
    device's figure is np.abs(omega - 1).max() of its own omega bit for bit."""
    n = 1799
    h = handle(n)
    h.set_obs_weights(None)
    om, _, _, chg, _ = h.debug_robust_from_s(_cases(n)['rayleigh'], hip.robust_options('huber', k=1e30))
    assert chg == 0.0 and np.all(om == 1.0)
    for case in ('rayleigh', 'extremes', 'cluster3', 'split5', 'all-zero', 'zeros-majority'):
        for loss, sm in LOSSES:
            om, _, _, chg, _ = h.debug_robust_from_s(_cases(n)[case], hip.robust_options(loss, scale=sm))
            assert chg == np.abs(om - 1.0).max(), (case, loss, sm)
    ro = hip.robust_options('huber', scale='apriori')
    base = 0.2 * rc.rayleigh(n)
    assert base.max() < ro.k
    for col in _moving_columns(n):
        s = base.copy()
        s[col] = 1e30
        om, _, _, chg, _ = h.debug_robust_from_s(s, ro)
        assert chg == np.abs(om - 1.0).max() and int(np.argmax(np.abs(om - 1.0))) == col and chg == 1.0 - om[col] > 0.99, col


def test_max_change_on_a_promoted_handle(hip, handle):
    """After set_obs_weights(om_prev): the change is measured against om_prev, exactly."""
    n = 1799
    h = handle(n)
    om_prev = _om_prev(n)
    h.set_obs_weights(om_prev)
    try:
        for case in ('rayleigh', 'extremes', 'cluster3', 'split5', 'all-zero', 'zeros-majority'):
            for loss, sm in LOSSES:
                om, _, _, chg, _ = h.debug_robust_from_s(_cases(n)[case], hip.robust_options(loss, scale=sm))
                assert chg == np.abs(om - om_prev).max(), (case, loss, sm)
        ro = hip.robust_options('huber', scale='apriori')
        base = 0.2 * rc.rayleigh(n)
        for col in _moving_columns(n):
            s = base.copy()
            s[col] = 1e30
            om, _, _, chg, _ = h.debug_robust_from_s(s, ro)
            d = np.abs(om - om_prev)
            assert chg == d.max() and int(np.argmax(d)) == col and chg >= 0.5 - 1e-15, col
    finally:
        h.set_obs_weights(None)
    om, _, _, chg, _ = h.debug_robust_from_s(_cases(n)['rayleigh'], hip.robust_options('cauchy', scale='mad'))
    assert chg == np.abs(om - 1.0).max()


@pytest.mark.parametrize('bad', [-1.0, -0.0, float('nan'), float('inf'), -5e-324], ids=['negative', 'minus-zero', 'nan', 'inf', 'minus-subnormal'])
def test_bad_values_are_refused(hip, handle, bad):
    n = 1800
    h = handle(n)
    ro = hip.robust_options('cauchy', scale='mad')
    good = _cases(n)['cluster4']
    for col in (0, 1234, n - 1):
        s = good.copy()
        s[col] = bad
        with pytest.raises(hip.DbatHipError) as e:
            h.debug_robust_from_s(s, ro)
        assert e.value.code == hip.EINVAL and 's_ip[%d]' % col in str(e.value)
    with pytest.raises(ValueError):
        h.debug_robust_from_s(good[:-1], ro)
    om, med, sc, chg, _ = h.debug_robust_from_s(good, ro)
    assert med == rc.ref_median(good) and sc == rc.ref_scale(good)
    assert np.abs(om - rc.ref_weights(good, sc, 'cauchy', ro.k)).max() <= 1e-12


def _lin_bits(h, x0):
    p, st = h.linearize_solve(x0, 0.0, True)
    return np.concatenate([_bits(p), _bits(np.array([float(st[k]) for k in ('f', 'JpJp', 'rJp', 'pp', 'trace', 'rcond')]))])


def test_nothing_is_applied(hip):
    """linearize_solve before and after a debug call gives the same bits (exact sums: deterministic mode), on a fresh
    handle and on a promoted one."""
    n = 1800
    h = hip.Handle(_struct(n))
    try:
        h.set_deterministic(True)
        x0 = h.serialize()
        a = _lin_bits(h, x0)
        for case in ('extremes', 'rayleigh'):
            h.debug_robust_from_s(_cases(n)[case], hip.robust_options('cauchy', scale='mad'))
            assert np.array_equal(_lin_bits(h, x0), a), case
        h.set_obs_weights(_om_prev(n))
        b = _lin_bits(h, x0)
        assert not np.array_equal(a, b)
        for case in ('extremes', 'rayleigh'):
            h.debug_robust_from_s(_cases(n)[case], hip.robust_options('huber', scale='mad'))
            assert np.array_equal(_lin_bits(h, x0), b), case
        h.set_obs_weights(None)
        assert np.array_equal(_lin_bits(h, x0), a)
    finally:
        h.close()


@pytest.mark.parametrize('n', rc.SIZES)
def test_repeat_gives_the_same_bits(hip, handle, n):
    h = handle(n)
    for case in ('cluster5', 'extremes', 'rayleigh'):
        for loss, sm in LOSSES:
            ro = hip.robust_options(loss, scale=sm)
            a, b = h.debug_robust_from_s(_cases(n)[case], ro), h.debug_robust_from_s(_cases(n)[case], ro)
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[4], b[4])
            assert np.array_equal(_bits(np.array(a[1:4])), _bits(np.array(b[1:4])))


@pytest.mark.parametrize('kind,world', [('small-priors', 2), ('small-priors', 4), ('c1', 4)],
                         ids=['small-priors-2', 'small-priors-4', 'c1-4'])
def test_ranks_select_collectively(hip, kind, world):
    """Every rank returns the reference median and scale, and omega and the largest change of the one-rank handle bit
    for bit, for values (a) dealt out in ascending order by owner -- rank 0 holds only the smallest, the last rank that
    holds anything only the largest -- and (b) shuffled.  c1 at four ranks: two of the four camera domains are empty,
    but the points of the top separator's cameras are dealt out to all four ranks, so every rank of these scenes owns
    observations (the counts are printed); a rank with none would only skip k_rsel_hist and k_robust_weight."""
    from test_multishard_gpu import _run_ranks, _scene
    s = _scene(kind)
    n = s.IP.val.shape[1]
    assert n % 2 == 0
    ro = hip.robust_options('cauchy', scale='mad')

    def on_ranks(inputs):
        def work(comm):
            hh = hip.Handle(s, shard_rank=comm.rank, shard_count=comm.world_size)
            try:
                hh.set_allreduce(comm.allreduce_ptr)
                return [hh.debug_robust_from_s(v, ro) for v in inputs]
            finally:
                hh.close()
        return _run_ranks(s, world, work)[0]

    owned = [r[0][4] for r in on_ranks([rc.rayleigh(n)])]
    assert np.array_equal(np.sum(owned, axis=0, dtype=np.int64), np.ones(n, np.int64))
    counts = [int(m.sum()) for m in owned]
    print('%s at %d ranks: observations per rank %s' % (kind, world, counts))
    values = [('split%d' % p, rc.split(n, p)) for p in (0, 3, 5)] + [('cluster5', rc.cluster(n, 5)), ('zeros-half', rc.zeros_half(n))] + \
        [('crowded%d' % p, rc.crowded(n, p)) for p in (0, 3)]
    inputs, names = [], []
    for name, v in values:
        dealt = rc.deal_sorted(v, owned)
        holders = [m for m in owned if m.any()]
        assert len(holders) >= 2 and np.array_equal(np.sort(dealt), np.sort(v))
        assert all(dealt[a].max() <= dealt[b].min() for a, b in zip(holders, holders[1:]))
        inputs += [dealt, v]
        names += [name + '-dealt', name + '-shuffled']
    h1 = hip.Handle(s)
    try:
        single = [h1.debug_robust_from_s(v, ro) for v in inputs]
    finally:
        h1.close()
    out = on_ranks(inputs)
    for rank in range(world):
        for name, v, one, got in zip(names, inputs, single, out[rank]):
            where = (name, rank)
            assert got[1] == rc.ref_median(v) and got[2] == rc.ref_scale(v), where
            assert one[1] == got[1] and one[2] == got[2], where
            assert np.array_equal(_bits(got[0]), _bits(one[0])), where
            assert got[3] == one[3] and got[3] == np.abs(got[0] - 1.0).max(), where
            assert np.array_equal(got[4], owned[rank]), where

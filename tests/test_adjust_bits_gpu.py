"""The bits of dbat_hip_poseadjust, dbat_hip_pointadjust and dbat_hip_pairadjust against tests/golden/adjust_bits.npz, recorded
on the device from an earlier build: the calls of tests/adjust_bits_cases.py, every per-item output equal to the stored one
(NaN equal to NaN), every per-observation output and the inputs by their SHA-256.  A change of these kernels that is meant to
keep their arithmetic passes this unchanged; one that changes numerics on purpose records the fixture anew
(tests/adjust_bits_cases.py says how) and says so."""
import os

import numpy as np
import pytest

import adjust_bits_cases as bc

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'adjust_bits.npz')


@pytest.fixture(scope='module')
def hip():
    from dbat_amd import _hip
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _hip.load()
    return _hip


@pytest.fixture(scope='module')
def golden():
    return bc.load(FIXTURE)


@pytest.fixture(scope='module')
def calls():
    return bc.all_calls()


def test_fixture_and_calls_agree(golden, calls):
    """Every call has its records and digests, and the fixture holds nothing else."""
    items, digests = golden
    assert set(items) == set(calls)
    assert set(digests) == {'%s/%s' % (name, k) for name, (fn, kw) in calls.items() for k in ('inputs',) + bc.OUTPUTS[fn][1]}
    for name, (fn, kw) in calls.items():
        assert items[name].dtype.names == bc.OUTPUTS[fn][0], name
    assert os.path.getsize(FIXTURE) < 100_000


@pytest.mark.parametrize('fn', sorted(bc.OUTPUTS))
def test_bits(hip, golden, calls, fn):
    items, digests = golden
    failed = []
    for name, (f, kw) in calls.items():
        if f != fn:
            continue
        assert digests[name + '/inputs'] == bc.inputs_digest(kw), name + ': the inputs are not the recorded ones'
        got, d = bc.entries(name, fn, kw, getattr(hip, fn)(**kw))
        want = items[name]
        assert got.dtype == want.dtype and got.shape == want.shape, name
        for k in got.dtype.names:
            if not np.array_equal(got[k], want[k], equal_nan=True):
                diff = np.abs(got[k].astype(float) - want[k].astype(float))
                failed.append('%s/%s: %d of %d entries differ, by %.3e at most' % (name, k, int(np.sum(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))),
                                                                              diff.size, np.nanmax(diff)))
        failed += ['%s: digest' % k for k in d if d[k] != digests[k]]
    assert not failed, failed

"""Host-only checks of the product lists of the factorisation's tasks (csrc/chol_df.hpp: order_jobs, apply_lists;
DBAT_HIP_DF_SUMS): a listed task takes the products of its sum in the order the schedule's model expects their tiles to
exist instead of column order.  The schedule a handle would build comes from dbat_hip_debug_df_schedule; what the bit
iteration of an unlisted task visits is recomputed here from the returned tile pattern.  No GPU; the factorisation with the
lists: tests/test_df_product_order_gpu.py."""
import contextlib
import os

import numpy as np
import pytest

from dbat_amd import _hip, synth
from helpers import roma_struct, synth_struct

SCENES = {
    'tiny': lambda: synth.make_scene('tiny')[0],                      # 12 cameras: one dense block
    'C1': lambda: synth.make_scene('C1')[0],
    'grid1000': lambda: synth.make_scene('C3', points=100000)[0],     # the camera grid of the benchmark scene
    'roma': roma_struct,                                              # real data: irregular visibility
    'small-selfcal': lambda: synth_struct('small', 'selfcal')[0],     # IO rows close the system
}
SWITCH = [None, '1', '2', '3']
_structs, _cache = {}, {}


@contextlib.contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def schedule(name, sums, merge=None):
    """dbat_hip_debug_df_schedule of a scene with DBAT_HIP_DF_SUMS = sums and DBAT_HIP_DF_MERGE = merge (None: unset),
    computed once."""
    key = (name, sums, merge)
    if key not in _cache:
        if name not in _structs:
            _structs[name] = SCENES[name]()
        with environment(DBAT_HIP_DF_SUMS=sums, DBAT_HIP_DF_MERGE=merge):
            _cache[key] = _hip.df_schedule(_structs[name])
    return _cache[key]


def has(sch, i, k):
    return bool((int(sch['rowbits'][i, k >> 6]) >> (k & 63)) & 1)


def common_columns(sch, i, k, jlo, jhi):
    """What the bit iteration of task (i, k) visits: the columns of [jlo, jhi) with a tile in both tile rows."""
    return [j for j in range(jlo, jhi) if has(sch, i, j) and has(sch, k, j)]


def parent_choice(cand):
    """The time of the schedule without lists: sums cut where that is more than 1 % shorter in the model."""
    return cand[1] if cand[1] >= 0 and cand[1] < 0.99 * cand[0] else cand[0]


def check_dependencies(sch, products):
    """Every input of a task belongs to a task with a smaller number (the tiles of the chain role's diagonal tasks, which
    are taken by ticket: the sums they start from)."""
    bit = sch['listed_bit']
    jobs = sch['jobs']
    plain, sumonly, diag, presum, helper = {}, {}, {}, {}, {}
    for t, (i, k, jlo, jhi, part, npieces, mode, p) in enumerate(jobs.tolist()):
        mode &= ~bit
        if npieces < 0:
            helper[part] = t
        elif mode == 1:
            sumonly[(i, k)] = t
        elif mode == 16:
            presum[k] = t
        elif i == k:
            diag[k] = t
        else:
            plain[(i, k)] = t
    for t, (i, k, jlo, jhi, part, npieces, mode, p) in enumerate(jobs.tolist()):
        mode &= ~bit
        for j in products[t]:
            for r in {i, k}:
                assert r > j
                if (r, j) in plain:
                    assert plain[(r, j)] < t, (t, r, j)
                else:                                             # the link of column j: its diagonal task publishes it
                    assert sumonly[(r, j)] < t, (t, r, j)
                    assert j in diag or j in presum
                    assert diag.get(j, -1) < t and presum.get(j, -1) < t, (t, r, j)
        if npieces > 0:
            assert all(helper[part + h] < t for h in range(npieces)), t
        if npieces >= 0 and mode == 0 and i != k:
            assert k in diag or k in presum
            assert diag.get(k, -1) < t and presum.get(k, -1) < t, t
        if npieces >= 0 and mode == 2:
            assert sumonly[(p, k)] < t, t


@pytest.mark.parametrize('sums', SWITCH, ids=['unset', '1', '2', '3'])
@pytest.mark.parametrize('name', sorted(SCENES))
def test_lists_are_permutations_and_the_other_tasks_are_the_parents(name, sums):
    sch = schedule(name, sums)
    # the schedule without lists that this one was made from: the same cut of the sums at the merge columns
    base = schedule(name, '0', '1' if sch['taken'] & 1 else '0')
    bit = sch['listed_bit']
    assert base['n_listed'] == 0 and base['taken'] == (sch['taken'] & 1) and len(base['plist']) == 0
    assert (base['rowbits'] == sch['rowbits']).all() and base['nT'] == sch['nT']
    assert len(base['jobs']) == len(sch['jobs']) and base['nparts'] == sch['nparts'] and base['products'] == sch['products']
    assert sch['taken'] >= 2 if sums is not None and sch['chain_role'] else sums is None or sch['taken'] < 2
    # (the task order may be another one: the lists are scored with several and the best is kept)
    parents = {(b[0], b[1], b[4], b[5], b[6], b[7]): b for b in base['jobs'].tolist()}
    assert len(parents) == len(base['jobs'])
    products, nlisted, used = [], 0, 0
    for t, job in enumerate(sch['jobs'].tolist()):
        i, k, jlo, jhi, part, npieces, mode, p = job
        ref = parents.pop((i, k, part, npieces, mode & ~bit, p))
        want = common_columns(base, ref[0], ref[1], ref[2], ref[3])
        if not mode & bit:
            assert job == ref, (t, job, ref)                      # a task without a list is the parent's task
            products.append(want)
            assert sums not in ('2', '3') or not want or not sch['chain_role']      # (control: every task with products is listed)
            continue
        nlisted += 1
        assert sch['taken'] >= 2
        assert [i, k, part, npieces, mode & ~bit, p] == [ref[0], ref[1], ref[4], ref[5], ref[6], ref[7]], (t, job, ref)
        assert jlo == used and jhi > jlo                          # the lists lie one after the other
        used = jhi
        lst = sch['plist'][jlo:jhi].tolist()
        assert sorted(lst) == want and len(set(lst)) == len(lst), (t, job, lst, want)
        if sums == '2':
            assert lst == want
        elif sums == '3':
            assert lst == want[::-1]
        else:
            assert lst != want                                    # a list in column order is no list
        products.append(lst)
    assert not parents and nlisted == sch['n_listed'] and used == len(sch['plist'])
    check_dependencies(sch, products)


@pytest.mark.parametrize('name', sorted(SCENES))
def test_the_model_decides(name):
    sch = schedule(name, None)
    cand, taken = sch['cand_us'], sch['taken']
    print(name, 'column order %.1f us, sums cut %.1f us, lists %.1f us, lists and cut sums %.1f us -> %d (%d of %d tasks listed)'
          % (cand[0], cand[1], cand[2], cand[3], taken, sch['n_listed'], len(sch['jobs'])))
    assert cand[0] > 0 and cand[taken] > 0
    parent = parent_choice(cand)
    assert cand[taken] <= parent
    if cand[1] >= 0:
        assert cand[taken] <= cand[1]                             # at most column order with the sums cut
    if taken >= 2:
        assert cand[taken] < 0.99 * parent
        assert sch['n_listed'] > 0
    else:
        assert cand[taken] == parent and sch['n_listed'] == 0
    # the switch at 0 is the parent's schedule, and the forced lists are scored as fixed lists
    off, on = schedule(name, '0'), schedule(name, '1')
    assert off['cand_us'][0] == cand[0] and off['cand_us'][1] == cand[1] and off['cand_us'][off['taken']] == parent
    ctl = schedule(name, '2')
    assert on['cand_us'] == cand
    if sch['chain_role']:
        assert on['taken'] >= 2 and ctl['taken'] >= 2
        assert ctl['cand_us'][ctl['taken']] == ctl['cand_us'][ctl['taken'] - 2]  # the control costs nothing in the model
    else:                                                         # lists only where the chain decides the time
        assert taken < 2 and on['taken'] < 2 and ctl['taken'] < 2 and cand[2] < 0 and cand[3] < 0


def test_one_dense_block_has_no_list():
    sch = schedule('tiny', None)
    assert sch['taken'] < 2 and sch['n_listed'] == 0 and len(sch['plist']) == 0
    assert not (sch['jobs'][:, 6] & sch['listed_bit']).any()


def test_grid_of_1000_cameras_takes_the_lists():
    sch = schedule('grid1000', None)
    cand, taken = sch['cand_us'], sch['taken']
    print('grid1000: column order %.1f us, sums cut at the merge columns %.1f us, product lists %.1f us, lists and cut sums %.1f us'
          ' -> candidate %d, %d of %d tasks listed, %d partial sums' % (cand[0], cand[1], cand[2], cand[3], taken, sch['n_listed'],
                                                                      len(sch['jobs']), sch['nparts']))
    assert taken in (2, 3)
    assert cand[taken] < 0.99 * parent_choice(cand)


@pytest.mark.parametrize('case', ['small-selfcal', 'C1'])
def test_plan_identical_for_any_number_of_threads(case, monkeypatch):
    """As tests/test_nd_separators_cpu.py: the digest of every array of the plan (the dissection is chosen through the
    schedule's model, lists included) is the same for 1, 2, 3 and 7 threads, with the lists forced."""
    s = SCENES[case]()
    monkeypatch.setenv('DBAT_HIP_DF_SUMS', '1')
    monkeypatch.setenv('DBAT_HIP_PLAN_GRAIN', '1' if case != 'C1' else '64')
    ref = None
    for threads in ('1', '2', '3', '7'):
        monkeypatch.setenv('DBAT_HIP_PLAN_THREADS', threads)
        d = (_hip.plan_digest(s, 0, 1), _hip.plan_digest(s, 1, 3), _hip.df_schedule(s))
        assert len(d[0]) > 40 and 'nd.order' in d[0]
        if ref is None:
            ref = d
        assert d[0] == ref[0] and d[1] == ref[1]
        assert (d[2]['jobs'] == ref[2]['jobs']).all() and (d[2]['plist'] == ref[2]['plist']).all()


def test_switch_values_are_checked(monkeypatch):
    s = SCENES['tiny']()
    monkeypatch.setenv('DBAT_HIP_DF_SUMS', '4')
    with pytest.raises(_hip.DbatHipError) as e:
        _hip.plan(s)
    assert e.value.code == _hip.EINVAL and 'DBAT_HIP_DF_SUMS' in str(e.value)
    with pytest.raises(_hip.DbatHipError) as e:
        _hip.df_schedule(s)
    assert e.value.code == _hip.EINVAL

"""Host-only checks of the separators of the nested dissection (csrc/nd.hpp) and of how one is chosen: the order of every
mode (DBAT_HIP_ND_SEP: 0 the lower half's boundary at the median, 1 the minimum vertex cover at the median, 2 the minimum
cover with slid cuts) is laid out in tiles and scored on the CPU by dbat_hip_debug_nd_stats, which also runs an
independent check of the order against the camera graph.  No GPU; the factorisation with these orders:
tests/test_nd_separators_gpu.py."""
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
_cache = {}


def stats(name):
    """{mode: requested}, chosen -- computed once per scene."""
    if name not in _cache:
        s = SCENES[name]()
        per, chosen = {}, None
        for mode in (0, 1, 2):
            per[mode], c = _hip.nd_stats(s, mode)
            assert chosen is None or c == chosen              # the choice does not depend on the mode asked for
            chosen = c
        _cache[name] = (per, chosen)
        print(name, 'chosen: mode %d' % chosen['mode'])
        for mode in (0, 1, 2):
            print('  mode %d:' % mode, per[mode])
    return _cache[name]


@pytest.mark.parametrize('name', sorted(SCENES))
def test_every_order_is_valid_and_the_choice_is_never_worse(name):
    per, chosen = stats(name)
    for mode in (0, 1, 2):
        st = per[mode]
        assert st['valid'] and st['mode'] == mode, (mode, st)
        assert st['tile_columns'] >= 1 and st['tiles'] >= st['tile_columns'] and 1 <= st['chain'] <= st['tile_columns']
    assert chosen['valid'] and chosen['mode'] in (0, 1, 2)
    assert chosen == per[chosen['mode']]
    assert chosen['model_us'] <= per[0]['model_us']
    assert chosen['chain'] <= per[0]['chain']
    if chosen['mode'] != 0:                                   # the order of mode 0 stays unless beaten by more than 1 %
        assert chosen['model_us'] < 0.99 * per[0]['model_us']


def test_one_dense_block_stays_one_block():
    per, chosen = stats('tiny')
    assert all(per[m]['blocks'] == 1 for m in (0, 1, 2)) and chosen['mode'] == 0


def test_grid_of_1000_cameras_gets_a_shorter_chain():
    per, chosen = stats('grid1000')
    print('chain of tile columns: mode 0 %d, mode 1 %d, mode 2 %d, chosen (mode %d) %d'
          % (per[0]['chain'], per[1]['chain'], per[2]['chain'], chosen['mode'], chosen['chain']))
    assert per[0]['cameras'] == 1000
    assert chosen['chain'] < per[0]['chain']


@pytest.mark.parametrize('sep', ['1', '2'])
@pytest.mark.parametrize('case', ['small-selfcal', 'C1'])
def test_plan_identical_for_any_number_of_threads(case, sep, monkeypatch):
    """As tests/test_abi_cpu.py does it for the default: the digest of every array of the plan (nd.order and nd.block_end
    among them) is the same for 1, 2, 3 and 7 threads, one rank and rank 1 of 3, with the separators forced."""
    s = SCENES[case]()
    monkeypatch.setenv('DBAT_HIP_ND_SEP', sep)
    monkeypatch.setenv('DBAT_HIP_PLAN_GRAIN', '1' if case != 'C1' else '64')
    ref = None
    for threads in ('1', '2', '3', '7'):
        monkeypatch.setenv('DBAT_HIP_PLAN_THREADS', threads)
        d = (_hip.plan_digest(s, 0, 1), _hip.plan_digest(s, 1, 3))
        assert len(d[0]) > 40 and 'nd.order' in d[0] and 'nd.block_end' in d[0]
        if ref is None:
            ref = d
        assert d == ref, [k for k in ref[0] if d[0][k] != ref[0][k]] + [k for k in ref[1] if d[1][k] != ref[1][k]]


def test_switch_values_are_checked(monkeypatch):
    s = SCENES['tiny']()
    monkeypatch.setenv('DBAT_HIP_ND_SEP', '3')
    with pytest.raises(_hip.DbatHipError) as e:
        _hip.plan(s)
    assert e.value.code == _hip.EINVAL and 'DBAT_HIP_ND_SEP' in str(e.value)

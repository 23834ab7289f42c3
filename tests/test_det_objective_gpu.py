"""The objective f that a linearisation reports in deterministic mode (dbat_hip_set_deterministic): the same bits from
call to call, and the value of the default mode.

On the signature route the default f adds the squared residuals wave by wave over whichever chunks a wave of k_build_sig
took, so its last bit follows the timing; deterministic mode takes the camera side's sum instead, which it forms over every
observation in a fixed order, the prior rows' squares included.  Scenes: plain, with prior observations, and a larger
one; each with the plan's weights and with one weight per observation.

The bound of the agreement, 1e-10 relative: the two sums take their residuals from two kernels that each evaluate the
camera model in float64.  An image coordinate of up to 1e3 px that carries a residual of a pixel loses three digits to
cancellation, so a term may differ by 1e3 x a few units in the last place, about 1e-12 of itself, and the sums of some
1e3 .. 1e5 non-negative terms by no more in relative terms; 1e-10 leaves two digits.  One observation or prior row left
out, or one weight not applied, moves f by 1e-5 of itself and more."""
import numpy as np
import pytest

from helpers import synth_struct

pytestmark = pytest.mark.gpu


def f_of(h, x0):
    return float(h.linearize_solve(x0, 0.0, True)[1]['f'])


@pytest.mark.parametrize('size,variant', [('tiny', 'plain'), ('tiny', 'priors'), ('small', 'plain')])
def test_deterministic_f_repeats_and_agrees(size, variant):
    from dbat_amd import _hip as hip
    s = synth_struct(size, variant)[0]
    h = hip.Handle(s)
    try:
        x0 = h.serialize()
        omega = np.random.default_rng(5).uniform(0.3, 1.0, s.IP.val.shape[1])
        for weights in (None, omega):
            h.set_obs_weights(weights)
            h.set_deterministic(False)
            f_default = f_of(h, x0)
            h.set_deterministic(True)
            f = [f_of(h, x0) for _ in range(8)]
            print('%s %s, %s: f %r, default mode %r (%.1e apart)' % (size, variant, 'plan weights' if weights is None else 'per-observation weights',
                                                                      f[0], f_default, abs(f[0] / f_default - 1)))
            assert f_default > 0 and len(set(np.array(f).view(np.uint64).tolist())) == 1, f
            assert abs(f[0] - f_default) <= 1e-10 * f_default
    finally:
        h.close()

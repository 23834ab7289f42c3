"""CPU tests of bundle_reliability's boundary and statistics: the C entry dbat_hip_redundancy is declared, bound and
refuses a NULL handle; reliability_stats (the pure host half) against direct NumPy on Qvv = I - J inv(J'J) J' formed
densely from the oracle's weighted Jacobian.  No GPU compute calls."""
import copy
import os
import re

import numpy as np
import pytest

import dbat_oracle as o
import dbat_amd
from dbat_amd import _hip
from dbat_amd.driver import reliability_critical, reliability_stats
from helpers import camcal_struct, sxb_prior_eo_struct, synth_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_setup(s):
    s = copy.deepcopy(s)
    for nm in ('IO', 'EO', 'OP'):
        pr = getattr(s.prior, nm)
        pr.use = np.asarray(pr.use, bool) & np.asarray(getattr(s.bundle.est, nm), bool)
    s = o.buildserialindices(s)
    return s, o.serialize(s), o.buildweightvector(s)


def _maps(so, n):
    """x index of every IO / EO / OP entry (-1: not an unknown), from the oracle's deserial indices."""
    big = 1e15
    IO, EO, OP = o.deserialize(so, big + np.arange(n, dtype=float))
    f = lambda a: np.where(a >= big / 2, np.rint(a - big), -1).astype(np.int64)
    return f(IO), f(EO), f(OP)


def dense_reliability(s, x=None):
    """(so, rw, qvv (3, nObs), r_prior, r (m,), maps) at x (default: the struct's own values), densely from the
    oracle's weighted Jacobian: H = J inv(J'J) J'."""
    so, x0, w = _oracle_setup(s)
    x = x0 if x is None else x
    r, K = o.brown_euler_cam4(x, so, jac=True)
    R = np.sqrt(w)
    J = (K.T.multiply(R).T).toarray()
    N = J.T @ J
    L = np.linalg.cholesky(N)
    G = np.linalg.solve(L, J.T)                                  # H = G' G
    h = np.einsum('ij,ij->j', G, G)
    no = s.IP.val.shape[1]
    ix = so.post.res.ix
    assert np.array_equal(np.asarray(ix.IP).ravel(), np.arange(2 * no))      # image rows first, priors after
    huv = np.einsum('ij,ij->j', G[:, 0:2 * no:2], G[:, 1:2 * no:2])
    qvv = np.vstack([1 - h[0:2 * no:2], -huv, 1 - h[1:2 * no:2]])
    return so, R * r, qvv, 1 - h[2 * no:], 1 - h, _maps(so, J.shape[1]), J.shape[1]


def test_redundancy_symbol_declared_bound_exported():
    hdr = open(os.path.join(ROOT, 'include', 'dbat_hip.h')).read()
    assert re.search(r'int\s+dbat_hip_redundancy\s*\(\s*dbat_hip_handle\s*\*h,\s*const double \*x,\s*double \*qvv_ip,'
                     r'[^;]*double \*r_prior\)', hdr)
    assert re.search(r'#define DBAT_HIP_ABI_VERSION 5\b', hdr)
    assert 'dbat_hip_redundancy' in _hip.SYMBOLS and _hip.ABI_VERSION == 5
    assert callable(dbat_amd.bundle_reliability) and callable(_hip.Handle.redundancy)
    lib = _hip.load()
    assert lib.dbat_hip_abi_version() == 5
    x = np.zeros(4)
    q = np.zeros(3)
    assert lib.dbat_hip_redundancy(None, _hip.dptr(x), _hip.dptr(q), _hip.dptr(q)) == _hip.EINVAL
    assert 'null' in _hip.last_error()


def test_critical_values():
    c = reliability_critical()
    assert abs(c.chi2_2 - 13.815510557964274) < 1e-12          # chi2inv(0.999, 2)
    assert abs(c.normal - 3.2905267314918945) < 1e-9            # norminv(1 - 0.0005)
    assert abs(c.delta0 - 4.132) < 5e-3 and round(c.delta0, 2) == 4.13
    c = reliability_critical(0.05, 0.5)
    assert abs(c.chi2_2 - 5.991464547107979) < 1e-12 and abs(c.delta0 - 1.959963984540054) < 1e-9
    with pytest.raises(dbat_amd.BadInput):
        reliability_critical(0.0, 0.8)


def _check_stats(s, perturb=0.0, seed=0):
    so, x0, _ = _oracle_setup(s)
    rng = np.random.default_rng(seed)
    x = x0 + perturb * rng.standard_normal(x0.shape) * np.maximum(np.abs(x0), 1e-3) if perturb else x0
    so, rw, qvv, rp, r, maps, n = dense_reliability(s, x)
    m = r.size
    assert abs(r.sum() - (m - n)) <= 1e-9 * m
    st = reliability_stats(s, rw, qvv, rp, maps)
    no = s.IP.val.shape[1]
    v = rw[:2 * no].reshape(2, no, order='F')
    rr = np.vstack([qvv[0], qvv[2]])
    np.testing.assert_allclose(st.r, r, rtol=0, atol=1e-15)
    assert abs(st.total - (m - n)) <= 1e-9 * m
    np.testing.assert_array_equal(st.IP.r, rr)
    np.testing.assert_array_equal(st.IP.q_uv, qvv[1])
    np.testing.assert_allclose(st.IP.w, v / np.sqrt(rr), rtol=1e-14)
    Tw = np.array([v[:, k] @ np.linalg.solve(np.array([[qvv[0, k], qvv[1, k]], [qvv[1, k], qvv[2, k]]]), v[:, k])
                   for k in range(no)])
    np.testing.assert_allclose(st.IP.T, Tw, rtol=1e-9, atol=1e-12)
    d0 = st.critical.delta0
    np.testing.assert_allclose(st.IP.mdb, d0 * np.asarray(s.IP.std, float) / np.sqrt(rr), rtol=1e-14)
    sel = np.flatnonzero(Tw > st.critical.chi2_2)
    sel = sel[np.argsort(-Tw[sel])]
    np.testing.assert_array_equal(st.suspects.ip, sel)
    np.testing.assert_array_equal(st.suspects.image, s.IP.cam[sel])
    np.testing.assert_array_equal(st.suspects.op_id, np.asarray(s.OP.id)[s.IP.pt[sel]])
    np.testing.assert_allclose(st.suspects.T, Tw[sel], rtol=1e-9)
    np.testing.assert_allclose(st.suspects.w_u, v[0, sel] / np.sqrt(rr[0, sel]), rtol=1e-14)
    return so, st, rw, rp


@pytest.mark.parametrize('variant', ['plain', 'selfcal', 'imagevar', 'priors', 'groups4'])
def test_stats_against_dense_numpy_synthetic(variant):
    s, _ = synth_struct('tiny', variant)
    # a little away from the true values: residuals of every size, some image points above the chi^2 quantile
    _check_stats(s, perturb=0.0)
    so, st, rw, rp = _check_stats(s, perturb=2e-3, seed=3)
    assert np.all(np.isfinite(st.IP.T))


def test_stats_against_dense_numpy_camcal():
    s = camcal_struct()
    so, st, rw, rp = _check_stats(s)
    assert len(st.suspects.ip) >= 0 and np.all(np.diff(st.suspects.T) <= 0)


def test_prior_placement_sxb_prior_eo():
    s, _ = sxb_prior_eo_struct(True)
    so, rw, qvv, rp, r, maps, n = dense_reliability(s)
    assert rp.size > 0
    st = reliability_stats(s, rw, qvv, rp, maps)
    no = s.IP.val.shape[1]
    ofs = 0
    for nm in ('IO', 'EO', 'OP'):
        ser = getattr(so.bundle.serial, nm)
        pos = np.asarray(ser.src)[np.asarray(ser.obs)]           # flat (column-major) val entry of every prior row
        k = len(pos)
        got_r, got_w = getattr(st, nm).r, getattr(st, nm).w
        rows = 6 if nm == 'EO' else getattr(s, nm).val.shape[0]
        assert got_r.shape == (rows, getattr(s, nm).val.shape[1])
        want_r = np.full(got_r.size, np.nan)
        want_w = np.full(got_r.size, np.nan)
        if k:
            # (EO: the flat positions index the full val; the placement keeps the first six rows)
            fr = np.full(getattr(s, nm).val.size, np.nan); fr[pos] = rp[ofs:ofs + k]
            fw = np.full(getattr(s, nm).val.size, np.nan); fw[pos] = rw[2 * no + ofs:2 * no + ofs + k] / np.sqrt(rp[ofs:ofs + k])
            want_r = fr.reshape(getattr(s, nm).val.shape, order='F')[:rows].ravel('F')
            want_w = fw.reshape(getattr(s, nm).val.shape, order='F')[:rows].ravel('F')
        np.testing.assert_allclose(got_r.ravel('F'), want_r, rtol=0, atol=1e-15)
        np.testing.assert_allclose(got_w.ravel('F'), want_w, rtol=1e-14)
        ofs += k
    assert ofs == rp.size
    assert np.isfinite(st.EO.r).any() and np.all(st.EO.r[np.isfinite(st.EO.r)] < 1)


def test_uncontrolled_observation_gives_nan_and_inf():
    s, _ = synth_struct('tiny', 'plain')
    so, rw, qvv, rp, r, maps, n = dense_reliability(s)
    qvv = qvv.copy()
    qvv[0, 3] = 1e-13                                            # r_u of IP column 3 at the threshold
    st = reliability_stats(s, rw, qvv, rp, maps)
    assert np.isnan(st.IP.w[0, 3]) and np.isinf(st.IP.mdb[0, 3]) and np.isnan(st.IP.T[3])
    assert np.isfinite(st.IP.w[1, 3]) and 3 not in st.suspects.ip

"""The NumPy replay of the epsilon-SVR solver (tools/svc_smo_replay.py::svr) pinned on the CPU, so that tests/test_gpu_svr.py
can use it as the step-for-step reference of k_svr: on the seven problems of tests/golden/svr_gradient.npz (the SVR flow
rule of Material.setup_fgrad_SVM on the reduced work-hardening data) it must reproduce libsvm without shrinking -- support
set, iteration count, intercept within 1e-12, coefficients within 1e-6 of the largest, the bars of
tests/test_svc_replay_cpu.py -- and on synthetic problems its fits must satisfy the KKT conditions in FP64.

KKT allowance.  The solver stops when m(a) - M(a) < tol on ITS gradient, which it builds from kernel entries rounded to FP32
(libsvm's Qfloat): an entry K <= 1 carries at most 2^-24 K, so each of the two gradient entries of the gap differs from the
FP64 one by at most sum|coef| 2^-24.  The FP64 gap may therefore reach tol + 2 sum|coef| 2^-24, and no more."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('svc_smo_replay', os.path.join(ROOT, 'tools', 'svc_smo_replay.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


@pytest.fixture(scope='module')
def z(golden_dir):
    return np.load(os.path.join(golden_dir, 'svr_gradient.npz'))


@pytest.mark.parametrize('m', range(7))
def test_replay_matches_libsvm_without_shrinking(z, m):
    pre = 'ns%d_' % m
    r = R.svr(z['x_sc'], z['y_sc'][:, m], float(z['C']), float(z['gamma']), epsilon=float(z['epsilon']), tol=float(z['tol']))
    print('model %d: n_iter %d (libsvm %d), nSV %d, intercept %.17g (libsvm %.17g)' % (
        m, r['n_iter_'], int(z[pre + 'n_iter']), len(r['support_']), r['intercept_'], float(z[pre + 'intercept'])))
    assert r['status'] == 0
    assert np.array_equal(r['support_'], z[pre + 'support'])
    assert r['n_iter_'] == int(z[pre + 'n_iter'])
    assert abs(r['intercept_'] - float(z[pre + 'intercept'])) <= 1e-12
    assert np.max(np.abs(r['dual_coef_'] - z[pre + 'dual'])) <= 1e-6 * np.max(np.abs(z[pre + 'dual']))


def test_fixture_is_the_setup_of_the_reference(z, golden_dir):
    """what the seven fits were handed is the standardised [flow_stress | plastic_strain] of the work-hardening fixture"""
    w = np.load(os.path.join(golden_dir, 'svc_data_training.npz'))
    assert np.array_equal(z['X_gt'], np.concatenate((w['wh_md_flow_stress'], w['wh_md_plastic_strain']), axis=1))
    assert np.array_equal((z['X_gt'] - z['feat_mean']) / z['feat_scale'], z['x_sc'])
    assert z['y_sc'].shape == (len(z['X_gt']), 7) and z['y_kh'][-1] == 0.


@pytest.mark.parametrize('seed,n,d,C,g,eps', [(1, 300, 6, 1., 0.5, 0.1), (2, 200, 12, 10., 0.1, 0.)])
def test_replay_kkt_fp64(seed, n, d, C, g, eps):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    t = np.sin(X[:, 0]) + 0.5 * X[:, -1] + 0.1 * rng.normal(size=n)
    tol = 1e-3
    r = R.svr(X, t, C, g, epsilon=eps, tol=tol)
    a, coef = r['alpha'], r['coef']
    assert r['status'] == 0
    assert np.all(a >= 0.) and np.all(a <= C)
    assert abs(np.sum(coef)) <= 1e-12 * C * n                  # the equality constraint sum(alpha - alpha*) = 0
    if eps > 0.:   # a row is above or below the tube, not both (without a tube the optimum does not forbid it)
        assert np.all((a[:n] == 0.) | (a[n:] == 0.))
    gap = R.svr_kkt_gap(X, t, coef, a, C, g, eps)
    allowed = tol + 2. * np.sum(np.abs(coef)) * 2. ** -24
    print('n %d d %d C %g gamma %g eps %g: n_iter %d, nSV %d, KKT gap %.6g (allowed %.6g)' % (
        n, d, C, g, eps, r['n_iter_'], len(r['support_']), gap, allowed))
    assert gap <= allowed
    # the dual objective from the solver's gradient against 1/2 c'Kc + eps sum|c| - t'c in FP64
    ob = 0.5 * coef @ R.kernel_fp64(X, X, g) @ coef + eps * np.sum(np.abs(coef)) - t @ coef
    assert abs(r['obj'] - ob) <= 1e-6 * abs(ob)

"""The NumPy replay of the SMO solver (tools/svc_smo_replay.py) pinned on the CPU, so that the GPU tests of
tests/test_gpu_svc_smo.py can use it as their step-for-step reference: on the four fixture problems of
tests/golden/svc_training.npz it must reproduce libsvm without shrinking exactly (support set, iteration count,
intercept), and on synthetic problems its fits must satisfy the KKT conditions in FP64."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('svc_smo_replay', os.path.join(ROOT, 'tools', 'svc_smo_replay.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

CASES = ['cfg4', 'shear', 'j2train', 'hill3']


@pytest.fixture(scope='module')
def z(golden_dir):
    return np.load(os.path.join(golden_dir, 'svc_training.npz'))


def ref_X(z, c):
    """features the reference hands to SVC.fit (see tests/test_gpu_svc_train.py)"""
    if c + '_X' in z.files:
        return z[c + '_X'], z[c + '_y']
    sd, seq = z[c + '_sdata'], z[c + '_seq']
    X = (seq[:, None, None] * sd[None, :, :]).reshape(-1, sd.shape[1]) / float(z[c + '_sy'])
    y = np.repeat(np.where(np.arange(len(seq)) < int(z[c + '_Nseq']), -1., 1.), len(sd))
    return X, y


@pytest.mark.parametrize('c', CASES)
def test_replay_matches_libsvm_without_shrinking(z, c):
    X, y = ref_X(z, c)
    r = R.smo(X, y, float(z[c + '_C']), float(z[c + '_gamma']))
    print('%s: n_iter %d (libsvm %d), nSV %d, intercept %.17g (libsvm %.17g)' % (
        c, r['n_iter_'], int(z[c + '_ns_n_iter']), len(r['support_']), r['intercept_'], float(z[c + '_ns_intercept'])))
    assert r['status'] == 0
    assert np.array_equal(r['support_'], z[c + '_ns_support'])
    assert r['n_iter_'] == int(z[c + '_ns_n_iter'])
    assert abs(r['intercept_'] - float(z[c + '_ns_intercept'])) <= 1e-12
    assert np.max(np.abs(r['dual_coef_'] - z[c + '_ns_dual'])) <= 1e-6 * np.max(np.abs(z[c + '_ns_dual']))


def _problem(seed, n, d, noise):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, -1] + noise * rng.normal(size=n) > 0., 1., -1.)
    return X, y


@pytest.mark.parametrize('seed,n,d,noise,C,g', [
    (1, 300, 6, 0.5, 1., 1.),
    (2, 200, 3, 1.0, 100., 5.),
    (3, 150, 1, 0.3, 10., 0.5),
    (4, 250, 16, 0.8, 2., 0.05),
])
def test_replay_kkt_fp64(seed, n, d, noise, C, g):
    X, y = _problem(seed, n, d, noise)
    r = R.smo(X, y, C, g)
    a = np.empty(n)
    a[r['perm']] = r['alpha']
    assert r['status'] == 0
    assert np.all(a >= 0.) and np.all(a <= C)
    assert abs(np.dot(y, a)) <= 1e-12 * C * n
    gap = R.kkt_gap(X, y, a, C, g)
    print('n %d d %d C %g gamma %g: n_iter %d, nSV %d, KKT gap %.6g' % (n, d, C, g, r['n_iter_'], len(r['support_']), gap))
    assert gap <= 1e-3 * (1 + 1e-3)
    assert abs(r['obj'] - R.dual_obj(X, y, a, g)) <= 1e-6 * abs(r['obj'])


def test_replay_max_iter_status():
    X, y = _problem(1, 300, 6, 0.5)
    full = R.smo(X, y, 1., 1.)
    n = full['n_iter_']
    assert R.smo(X, y, 1., 1., max_iter=0)['n_iter_'] == n          # <= 0: libsvm's default
    for m, st in [(1, 1), (n - 1, 1), (n, 1), (n + 1, 0)]:
        r = R.smo(X, y, 1., 1., max_iter=m)
        assert (r['status'], r['n_iter_']) == (st, min(m, n)), m

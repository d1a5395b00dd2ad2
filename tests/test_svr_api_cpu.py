"""The host side of the SVR flow rule (Material.setup_fgrad_SVM) without a GPU: the errors of the façade,
the StandardScaler arithmetic against the scalers scikit-learn fitted for tests/golden/svr_gradient.npz, and the two new
C-ABI symbols in header, library and binding (tests/test_abi.py::test_exports_match_header checks all of them)."""
import os
import re

import numpy as np
import pytest

import pylabfea_amd as FE
from pylabfea_amd import _lib
from pylabfea_amd.material import StdScaler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def z(golden_dir):
    return np.load(os.path.join(golden_dir, 'svr_gradient.npz'))


def hill():
    m = FE.Material(name='Hill')
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=50., hill=[1.2, 1., 0.8, 1., 1., 1.], khard=100., sdim=6)
    return m


def test_setup_needs_work_hardening_data():
    for m in (FE.Material(), hill()):
        with pytest.raises(ValueError, match='No strain hardening data available.'):
            m.setup_fgrad_SVM()
        assert m.ML_grad is False


def test_device_paths_refuse_an_svr_gradient():
    m = hill()
    m.ML_grad = True
    CV = np.asarray(m.CV)
    calls = {'response': lambda: m.response(np.zeros(6), np.zeros(6), np.full(6, 1e-4), CV),
             'response_batch': lambda: m.response_batch(np.zeros((2, 6)), np.zeros((2, 6)), np.full((2, 6), 1e-4), CV),
             'calc_properties': lambda: m.calc_properties()}
    fe = FE.Model(dim=2, planestress=False)
    fe.geom([2.], LY=2.)
    fe.assign([m])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.004, 'disp')
    fe.mesh(NX=2, NY=2)
    calls['Model.solve'] = lambda: fe.solve()
    for name, call in calls.items():
        with pytest.raises(NotImplementedError) as e:
            call()
        msg = str(e.value)
        assert 'ML_grad' in msg and 'False' in msg and 'SVC gradient' in msg, (name, msg)
    assert fe.u is None                       # nothing was solved


def test_scaler_arithmetic(z):
    for pre, X in (('feat_', z['X_gt']), ('grad_', z['y_gt']), ('khard_', z['y_kh'].reshape(-1, 1))):
        s = StdScaler(X)
        assert np.all(np.abs(s.mean_ - z[pre + 'mean']) <= 1e-15 * np.abs(z[pre + 'mean']))
        assert np.all(np.abs(s.scale_ - z[pre + 'scale']) <= 1e-15 * z[pre + 'scale'])
    s = StdScaler(z['X_gt'])
    assert np.max(np.abs(s.transform(z['X_gt']) - z['x_sc'])) <= 1e-15 * np.max(np.abs(z['x_sc']))
    back = s.inverse_transform(z['x_sc'])
    assert np.max(np.abs(back - z['X_gt']) / z['feat_scale']) <= 4 * 2. ** -53 * np.max(np.abs(z['x_sc']) + 1.)
    # population standard deviation, and scale 1 for a column without variance (zero, or a constant that np.var
    # returns a rounding residue for)
    rng = np.random.default_rng(0)
    X = np.concatenate((rng.normal(size=(50, 2)), np.zeros((50, 1)), np.full((50, 1), 0.1 + 0.2)), axis=1)
    s = StdScaler(X)
    assert np.array_equal(s.scale_[:2], np.sqrt(np.mean((X[:, :2] - X[:, :2].mean(axis=0)) ** 2, axis=0)))
    assert np.all(s.scale_[2:] == 1.)
    assert np.all(s.transform(X)[:, 2] == 0.) and np.all(np.abs(s.transform(X)[:, 3]) < 1e-15)
    assert np.array_equal(s.inverse_transform(np.zeros((1, 4)))[0], s.mean_)


def test_new_symbols_in_header_library_and_binding():
    with open(os.path.join(ROOT, 'include', 'plfx.h')) as fp:
        declared = set(re.findall(r'\b(plfx_[a-z0-9_]+)\s*\(', fp.read()))
    lib = _lib.load()
    for name in ('plfx_svr_fit_batch', 'plfx_svr_predict_multi'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)

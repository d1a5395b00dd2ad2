"""What of DESIGN.md §30 needs no GPU: create_test_sig against the arrays recorded from the reference on the small JSON
database carried inside tests/golden/flow_curve.npz, the legacy aliases, the row selection of Material.data_curve, the
refusals and argument checks of Material.flow_curve, and the NumPy transcription's search against a function whose root is
known."""
import os
import warnings

import numpy as np
import pytest

import flow_curve_cases as FC
import pylabfea_amd as FE
from svr_flow_cases import install_svr


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'flow_curve.npz'))


def test_create_test_sig_matches_the_reference(fx, tmp_path):
    path = tmp_path / 'small.json'
    path.write_bytes(fx['ts_json'].tobytes())
    assert FE.create_test_sig is FE.training.create_test_sig
    for tag, kw in (('ts', {}), ('ts2', dict(number_sig_per_strain=2))):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sig, epl, yf = FE.create_test_sig(str(path), **kw)
        assert sig.shape == fx[tag + '_sig'].shape and epl.shape == fx[tag + '_epl'].shape
        assert np.array_equal(yf, fx[tag + '_yf'])                      # the labels: +1 first half, -1 second half
        # the flow stresses come out of Data's interpolation of the database: the façade's Data agrees with the reference's
        # within rounding (tests/test_data_cpu.py holds it to 1e-12 relative); the factors and the order are exact
        scale = np.max(np.abs(fx[tag + '_sig']))
        assert np.max(np.abs(sig - fx[tag + '_sig'])) <= 1e-12 * scale
        assert np.max(np.abs(epl - fx[tag + '_epl'])) <= 1e-12 * np.max(np.abs(fx[tag + '_epl']))
    n = len(sig) // 8
    fs = sig[3:4 * n:4] / 1.01                                         # the data rows, from the factor 1.01
    want = np.concatenate([(fs[:, None, :] * np.array(f)[None, :, None]).reshape(-1, 6)
                           for f in ((1.5, 1.2, 1.1, 1.01), (0.99, 0.9, 0.8, 0.5))])
    assert np.allclose(sig, want, rtol=4e-16, atol=0.)


def test_aliases_are_the_functions_they_name():
    pairs = dict(seq_J2=FE.sig_eq_j2, sprinc=FE.sig_princ, sp_cart=FE.sig_cyl2princ, s_cyl=FE.sig_princ2cyl, sdev=FE.sig_dev,
                 polar_ang=FE.sig_polar_ang)
    for name, fn in pairs.items():
        assert getattr(FE, name) is fn and name in FE.__all__, name
    assert 'create_test_sig' in FE.__all__ and not hasattr(FE, 'svoigt')


def test_data_curve_rows_and_refusals(fx, monkeypatch):
    m, p = FC.wh_material()
    seen = {}

    def fake(su, epl=None, x0=None, return_status=False, tex=None):
        seen.update(su=np.array(su), epl=np.array(epl), x0=x0, calls=seen.get('calls', 0) + 1)
        return np.full(len(su), 2.), np.zeros(len(su), dtype=np.int32)
    monkeypatch.setattr(m, 'yield_scale', fake)
    for ilc in fx['dc_ilc']:
        t = '_%d' % ilc
        seen.clear()
        r = m.data_curve(int(ilc))
        assert seen['calls'] == 1 and seen['x0'] == m.sy                 # ONE yield_scale call, started at sy
        assert np.array_equal(r['index'], fx['dc_index' + t])
        assert np.array_equal(seen['epl'], fx['dc_epl' + t])
        assert np.max(np.abs(r['sig0'] - fx['dc_sig0' + t])) <= 4 * np.finfo(float).eps
        assert np.all(seen['su'] == r['sig0'][None, :])
        assert np.allclose(r['peeq'], fx['dc_peeq' + t], rtol=1e-14, atol=0.)
        assert np.allclose(r['seq_data'], fx['dc_seq_data' + t], rtol=1e-13, atol=0.)
        assert np.allclose(r['seq_ml'], 2., rtol=1e-14) and r['sig_ml'].shape == (len(r['peeq']), 6)
        assert 'status' not in r and 'status' in m.data_curve(np.int64(ilc), return_status=True)
    for bad in (1.0, '1', None, True):
        with pytest.raises(ValueError, match='must be an integer number specifying the load case'):
            m.data_curve(bad)
    m2 = FC.hill_material()
    with pytest.raises(AttributeError):
        m2.data_curve(1)


def test_flow_curve_refusals_and_argument_shapes():
    su = FC.EXAMPLE_DIRS
    m3 = FE.Material()
    m3.elasticity(E=200.e3, nu=0.3)
    m3.plasticity(sy=100., sdim=3)
    mt = FE.Material()
    mt.elasticity(E=200.e3, nu=0.3)
    mt.plasticity(sy=100., tresca=True, sdim=6)
    mb = FC.YC.analytic(FE, 'abarlat')
    for m in (m3, mt, mb):
        with pytest.raises(NotImplementedError, match='flow_curve'):
            m.flow_curve(su)
    mg, _ = FC.wh_material()
    install_svr(mg, np.load(os.path.join(FC.GOLD, 'svr_gradient.npz')))
    with pytest.raises(NotImplementedError, match='flow_curve: ML_grad is set'):
        mg.flow_curve(su)
    mg.enable_svr_flow()
    with pytest.raises(NotImplementedError, match='flow_curve: ML_grad is set'):
        mg.flow_curve(su)
    mx, _ = FC.wh_material()
    mx.txdat = True
    with pytest.raises(NotImplementedError, match='flow_curve: not offered for a texture material'):
        mx.flow_curve(su)
    me = FE.Material()
    me.elasticity(E=200.e3, nu=0.3)
    with pytest.raises(ValueError, match='no yield strength'):
        me.flow_curve(su)
    # argument checks come before any device call
    m, _ = FC.wh_material()
    with pytest.raises(ValueError, match='has zero equivalent stress'):
        m.flow_curve(np.zeros(6))
    with pytest.raises(ValueError, match='has zero equivalent stress'):
        m.flow_curve(np.array([su[0], [2., 2., 2., 0, 0, 0]]))
    for bad in (np.zeros(3), np.zeros((2, 3)), np.zeros((2, 2, 6))):
        with pytest.raises(ValueError, match='must be given as unit Voigt stress tensor'):
            m.flow_curve(bad)
    for bad in (np.zeros(3), np.zeros((3, 6)), np.zeros((4, 5))):
        with pytest.raises(ValueError, match='epl0 must be None'):
            m.flow_curve(su, epl0=bad)
    for kw in (dict(depl=0.), dict(depl=-1e-3), dict(depl=np.nan), dict(max_steps=-1), dict(predictor=np.inf),
               dict(epl_max=np.nan)):
        with pytest.raises(ValueError, match='flow_curve: max_steps >= 0'):
            m.flow_curve(su, **kw)
    assert m.khard == 0.


def test_transcription_search_finds_a_known_root():
    """the NumPy restatement of the ray search on f(x) = x - r: the neighbouring doubles around r, from either side"""
    for r, x0 in ((53.25, 49.6), (53.25, 80.), (1.0, 1.0), (0.3, 20.)):
        st, x = FC.ray_root(lambda t: t - r, x0)
        assert st == 0 and x == r
    assert FC.ray_root(lambda t: 1., 5.) == (1, pytest.approx(np.nan, nan_ok=True))
    assert FC.ray_root(lambda t: -1., 5.)[0] == 1 and FC.ray_root(lambda t: np.nan, 5.)[0] == 1

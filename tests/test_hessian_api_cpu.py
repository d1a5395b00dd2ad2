"""Material.calc_hessian (material.py:860-972): the branches of the façade that need no device -- the reference's refusals
with the reference's messages -- and the fixture tests/golden/svc_hessian.npz (tools/gen_hessian_golden.py)."""
import os

import numpy as np
import pytest

import pylabfea_amd as FE


def analytic(**kw):
    m = FE.Material()
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=100., **kw)
    return m


def ml_material(golden_dir, name):
    z = np.load(os.path.join(golden_dir, 'svc_%s.npz' % name))
    m = FE.Material(name='ML-' + name)
    m.elasticity(CV=z['par_CV'])
    m.plasticity(sy=float(z['par_sy']), sdim=int(z['par_sdim']))
    m.set_svc(z['par_sv'], z['par_dual'], float(z['par_intercept']), float(z['par_gamma']), float(z['par_scale_seq']),
              dev_only=bool(z['par_dev_only']))
    return m


SIG = np.array([[60., -10., 5., 3., 0., 12.], [10., 80., -5., 0., 7., 1.]])


@pytest.mark.parametrize('kw, msg', [
    (dict(sdim=6), 'calc_hessian: analytical hessian for Hill not implemented'),
    (dict(sdim=6, hill=[0.7, 1., 1.4, 1., 1.2, 0.8]), 'calc_hessian: analytical hessian for Hill not implemented'),
    (dict(sdim=3), 'calc_hessian: analytical hessian for Hill not implemented'),
    (dict(sdim=6, tresca=True), 'calc_hessian: analytical hessian for Tresca not implemented'),
    (dict(sdim=6, barlat=np.ones(18), barlat_exp=8), 'calc_hessian: analytical hessian for Barlat not implemented'),
])
def test_analytic_materials_raise_like_the_reference(kw, msg):
    m = analytic(**kw)
    s = SIG[:, :m.sdim]
    for arg in (s, s[0]):
        with pytest.raises(ValueError) as e:
            m.calc_hessian(arg)
        assert str(e.value) == msg


def test_ana_overrides_the_ml_yield_function(golden_dir):
    m = ml_material(golden_dir, 'hill')
    with pytest.raises(ValueError) as e:
        m.calc_hessian(SIG, ana=True)
    assert str(e.value) == 'calc_hessian: analytical hessian for Hill not implemented'


def test_sdim3_ml_material_is_not_implemented(golden_dir):
    m = ml_material(golden_dir, 'hill3d')
    assert m.sdim == 3 and m.ML_yf
    for arg in (SIG[:, :3], SIG[0, :3], SIG[0]):
        with pytest.raises(NotImplementedError) as e:
            m.calc_hessian(arg)
        assert str(e.value) == 'calc_hessian: not  implemented for 3D stress'


def test_texture_is_refused(golden_dir):
    m = ml_material(golden_dir, 'hill')
    with pytest.raises(NotImplementedError):
        m.calc_hessian(SIG, tex=np.zeros(4))


@pytest.mark.parametrize('shape', [(5,), (2, 5), (2, 3), (2, 2, 6), (7, 6, 1)])
def test_bad_shapes(golden_dir, shape):
    m = ml_material(golden_dir, 'hill')
    khard, msg = m.khard, dict(m.msg)
    with pytest.raises(ValueError) as e:
        m.calc_hessian(np.zeros(shape))
    assert str(e.value) == 'Unknown format of stress in calc_fgrad'
    assert m.khard == khard and m.msg == msg


def test_bad_plastic_strain_shape(golden_dir):
    z = np.load(os.path.join(golden_dir, 'svc_workhard.npz'))
    m = FE.Material(name='ML-hardening')
    m.elasticity(CV=z['par_CV'])
    m.plasticity(sy=float(z['par_sy']), sdim=6)
    m.set_svc(z['par_sv'], z['par_dual'], float(z['par_intercept']), float(z['par_gamma']), float(z['par_scale_seq']),
              scale_wh=float(z['par_scale_wh']))
    with pytest.raises(ValueError):
        m.calc_hessian(SIG, epl=np.zeros((3, 6)))
    with pytest.raises(NotImplementedError):
        m.calc_hessian(SIG, accumulated_strain=0.01)


def test_binding_and_header_name_the_entry_point():
    from pylabfea_amd import _lib
    assert 'plfx_hessian_batch' in _lib.SYMBOLS and hasattr(_lib.load(), 'plfx_hessian_batch')
    assert callable(_lib.Context.hessian)


def test_fixture(golden_dir):
    f = np.load(os.path.join(golden_dir, 'svc_hessian.npz'))
    assert os.path.getsize(os.path.join(golden_dir, 'svc_hessian.npz')) < 300 * 1024
    for tag, src in (('hill', 'svc_hill.npz'), ('hilldev', 'svc_hill.npz'), ('wh', 'svc_workhard.npz')):
        z = np.load(os.path.join(golden_dir, src))
        assert float(f[tag + '_sv_sum']) == float(np.sum(z['par_sv']))       # the rows belong to these parameters
        H, n = f[tag + '_hess'], f[tag + '_n']
        assert H.shape == (int(np.sum(n)), 6, 6) and f[tag + '_sig'].shape == f[tag + '_epl'].shape == (len(H), 6)
        # symmetric to the rounding of the reference's products (it forms [a][b] and [b][a] in different orders)
        assert np.max(np.abs(H - H.transpose(0, 2, 1))) <= 1e-14 * np.max(np.abs(H))
        assert np.all(H[-int(n[2]):] == 0.) and np.all(np.any(H[:-int(n[2])] != 0., axis=(1, 2)))   # far rows underflow
        k = int(f[tag + '_single'])
        assert f[tag + '_hess_single'].shape == (1, 6, 6) and np.array_equal(f[tag + '_hess_single'][0], H[k])
        assert 0.1 < float(f[tag + '_r_ref']) < 16.
        assert bool(f[tag + '_dev_only']) == (tag == 'hilldev')
    assert np.any(f['wh_epl'] != 0.) and not np.any(f['hill_epl'] != 0.)

"""Host side of texture materials bound to one texture (Material.at_texture), no GPU: the new kind and call of
the C-ABI in the header and in the built library, the fold identity and its gradient in plain FP64 NumPy against the
longdouble restatement of the texture SVC (tests/texture_flow_cases.py), the shapes of the folded tables, and every error
path of the façade, all raised before the device is touched."""
import os
import re

import numpy as np
import pytest

import texture_bound_cases as TB
import texture_cases as TC
import texture_flow_cases as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITS = [(desc, dev) for desc in TC.DESCRIPTORS for dev in (False, True)]


@pytest.fixture(scope='module')
def z():
    return TC.load()


@pytest.fixture(scope='module')
def mats(z, tmp_path_factory):
    import pylabfea_amd as FE
    d = tmp_path_factory.mktemp('texture_db')
    return {desc: TC.facade(FE, z, d, desc)[0] for desc in TC.DESCRIPTORS}


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to reach the device fails the test"""
    from pylabfea_amd import material

    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(material, '_ctx', boom)


def test_kind_and_call_in_header_and_library():
    from pylabfea_amd import _lib
    lib = _lib.load()
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'plfx.h')).read(), flags=re.S)
    assert re.search(r'\bPLFX_SVC6_COLS\s*=\s*8\b', txt)
    assert _lib.SVC6_COLS == 8
    m = re.search(r'\bint\s+plfx_set_svc_cols\s*\(([^)]*)\)\s*;', txt)
    assert m
    args = [re.sub(r'\s+', ' ', a.strip()) for a in m.group(1).split(',')]
    assert [re.sub(r'\s*\b\w+(\[6\])?$', r'\1', a).replace(' *', '*') for a in args] == ['plfx_ctx*', 'int', 'const double[6]']
    assert hasattr(lib, 'plfx_set_svc_cols') and 'plfx_set_svc_cols' in _lib.SYMBOLS


@pytest.mark.parametrize('desc,dev', FITS)
def test_fold_identity_and_gradient(z, mats, desc, dev, no_device):
    """fold_texture(tau) evaluated in plain FP64 NumPy is calc_yf(sig, tex=tau) of the longdouble restatement within
    value_bar, and the gradient formula on the folded tables is its gradient within grad_bar: the four fixture fits at the
    textures of the training sets (rows 0-4; set 5 is left out with GSH_7, where the function does not change sign), 50
    seeded stresses of size ~40 MPa each."""
    import pylabfea_amd as FE
    p, tex = TC.tables(z, desc, dev), TC.textures(z, desc)
    m = TB.parent(FE, mats[desc], p)
    worst_v = worst_g = 0.
    for t in range(5):
        sig = TB.seeded_stresses(50, 100 + t)
        f = m.fold_texture(tex[t])
        g = TB.fold(p, tex[t])
        for k in ('sv', 'dual', 'scale'):
            assert np.array_equal(f[k], g[k]), k
        assert (f['intercept'], f['gamma'], f['dev_only']) == (g['intercept'], g['gamma'], g['dev_only'])
        ref = TF.decision(p, sig, tex[t])
        cal_v, cal_g = TF.calib(p, sig, tex[t])
        ev = float(np.max(np.abs(TB.folded_yf(f, sig) - ref)))
        assert ev <= TC.value_bar(cal_v, np.asarray(ref, dtype=float)), (t, ev)
        aref = TF.gradient(p, sig, tex[t])
        eg = float(np.max(np.abs(TB.folded_grad(f, sig) - aref)))
        assert eg <= TF.grad_bar(cal_g, aref), (t, eg)
        if dev:
            assert float(np.max(np.abs(np.sum(TB.folded_grad(f, sig)[:, :3], axis=1)))) <= 1e-15 * float(np.max(np.abs(aref)))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    print('%s dev %d: fold |yf - ref| <= %.2e, |grad - ref| <= %.2e' % (desc, dev, worst_v, worst_g))


def test_folded_shapes(z, mats, no_device):
    import pylabfea_amd as FE
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    q10, t10 = TC.widen(p, tex, 10)
    for q, t in ((TC.cut(p, nsv=1), tex[0]), (q10, t10[0]), (TC.cut(p, tdim=1), tex[0][:1])):
        f = TB.parent(FE, mats['GSH_3'], q).fold_texture(t)
        n = len(q['sv'])
        assert f['sv'].shape == (n, 6) and f['dual'].shape == (n,) and f['scale'].shape == (6,)
        assert f['sv'].flags['C_CONTIGUOUS'] and np.all(np.isfinite(f['sv'])) and np.all(np.isfinite(f['dual']))
        assert isinstance(f['intercept'], float) and isinstance(f['gamma'], float) and f['dev_only'] is False
        assert np.array_equal(f['scale'], q['scale'][:6])
        sig = TB.seeded_stresses(4, 7)
        ref = TF.decision(q, sig, t)
        assert float(np.max(np.abs(TB.folded_yf(f, sig) - ref))) <= TC.value_bar(TF.calib(q, sig, t)[0], np.asarray(ref, dtype=float))


def test_at_texture_errors_and_what_it_carries(z, mats, no_device):
    import pylabfea_amd as FE
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    m = TB.parent(FE, mats['GSH_3'], p, khard=50.)
    for bad in (tex[0][:2], tex[:2], np.zeros((1, 3)), np.array([0., np.nan, 0.]), np.array([0., np.inf, 0.])):
        with pytest.raises(ValueError, match='tex must be'):
            m.at_texture(bad)
    j2 = FE.Material('J2')
    j2.elasticity(E=200.e3, nu=0.3)
    j2.plasticity(sy=100., sdim=6)
    with pytest.raises(NotImplementedError, match='texture material'):
        j2.at_texture(tex[0])
    with pytest.raises(AttributeError, match='train_SVC'):
        mats['GSH_3'].at_texture(tex[0])                            # from_data alone: untrained
    key = m._tex_key()
    b = m.at_texture(tex[1], name='bound')
    assert m._tex_key() == key and m._bound is None and m.txdat    # the parent is untouched
    assert b.name == 'bound' and b._bound['parent'] is m and np.array_equal(b._bound['tex'], tex[1])
    assert (b.E, b.nu, b.sy, b.khard, b.sdim) == (m.E, m.nu, m.sy, 50., 6)
    assert np.array_equal(b.CV, m.CV) and np.array_equal(b.hill, m.hill) and b.hill_6p == m.hill_6p
    f = m.fold_texture(tex[1])
    assert np.array_equal(b.svc['sv'], f['sv']) and np.array_equal(b.svc['dual'], f['dual'])
    assert np.array_equal(b._bound['scale'], f['scale'])
    from pylabfea_amd import _lib
    rec, keep = b._record(np.array(b.CV))
    assert rec.kind == _lib.SVC6_COLS and rec.nsv == len(f['dual']) and rec.nfeat == 6 and rec.khard == 50.
    assert np.array_equal(keep[2], f['scale'])
    assert b._record(np.array(b.CV), ana=True)[0].kind == _lib.HILL6
    # the key covers the folded tables and the scales
    k0 = b._content_key()
    b2 = m.at_texture(tex[2])
    assert b2._content_key() != k0 and m.at_texture(tex[1])._content_key() == k0
    b._bound['scale'][3] *= 2.
    assert b._content_key() != k0


def test_gated_methods_and_model_refusals(z, mats, tmp_path, no_device):
    import pylabfea_amd as FE
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    m = TB.parent(FE, mats['GSH_3'], p)
    b = m.at_texture(tex[0])
    sig = z['probe_sig'][0]
    calls = {
        'calc_hessian': lambda: b.calc_hessian(sig),
        'flow_curve': lambda: b.flow_curve(sig[None]),
        'polar_yield_locus': lambda: b.polar_yield_locus(),
        'yield_slices': lambda: b.yield_slices(),
        'setup_fgrad_SVM': lambda: b.setup_fgrad_SVM(),
        'train_SVC': lambda: b.train_SVC(),
        'export_MLparam': lambda: b.export_MLparam('script', path=str(tmp_path)),
        'Committee': lambda: FE.Committee([b]),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match='at_texture') as e:
            call()
        assert name in str(e.value), name
    for call in (lambda: b.calc_yf(sig, tex=tex[0]), lambda: b.calc_fgrad(sig, tex=tex[0]), lambda: b.yield_scale(sig, tex=tex[0])):
        with pytest.raises(ValueError, match='takes no tex'):
            call()
    with pytest.raises(ValueError, match=r'\(N, 6\)'):
        b.response_batch(z['probe_sig'][:4], np.zeros((3, 6)), np.full((4, 6), 1e-4), np.array(b.CV))
    with pytest.raises(ValueError, match='khard_in'):
        b.response_batch(z['probe_sig'][:4], np.zeros((4, 6)), np.full((4, 6), 1e-4), np.array(b.CV), khard_in=np.zeros(4))
    # the host parts of a bound material need no device
    assert b.get_sflow(np.array([1e-3, -5e-4, -5e-4, 0., 0., 0.])) == b.sy + 1e-3 * b.khard
    fe = FE.Model(dim=2, planestress=True)
    fe.geom([2., 1.], LY=2.)
    fe.assign([b, m.at_texture(tex[1])])                            # supported: nothing raised
    with pytest.raises(NotImplementedError, match='Model.distribute'):
        fe.distribute(0, 2, b'x' * 128)
    fe2 = FE.Model(dim=2, planestress=True)
    fe2.geom([2.], LY=2.)
    fe2.distribute(0, 2, b'x' * 128)
    with pytest.raises(NotImplementedError, match='Model.distribute'):
        fe2.assign([b])
    with pytest.raises(NotImplementedError, match='reference'):     # the parent is still refused
        fe.assign([m, m])

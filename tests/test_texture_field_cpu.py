"""Host side of texture fields (Material.at_textures, Model.set_texture_ids), no GPU: the new entry points in
the header and in the built library, fold_textures against fold_texture row by row and bit for bit, and every error path of
the façade, all raised before the device is touched."""
import os
import re

import numpy as np
import pytest

import texture_bound_cases as TB
import texture_cases as TC
import texture_field_cases as TX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITS = [(desc, dev) for desc in TC.DESCRIPTORS for dev in (False, True)]

ENTRY_POINTS = {
    'plfx_set_svc_textures': ['plfx_ctx*', 'int', 'int', 'const double*'],
    'plfx_set_element_textures': ['plfx_ctx*', 'const int32_t*'],
    'plfx_full_yf_batch_tid': ['plfx_ctx*', 'int', 'int', 'const double*', 'const double*', 'const double*', 'double*',
                               'int32_t*', 'const int32_t*'],
    'plfx_response_batch_tid': ['plfx_ctx*', 'int', 'const int32_t*', 'const double*', 'const double*', 'const double*',
                                'double*', 'double*', 'double*', 'double*', 'int32_t*', 'const int32_t*'],
    'plfx_svc_textures_info': ['plfx_ctx*', 'int', 'int*', 'int*', 'int64_t*'],
}


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
    from pylabfea_amd import material, _lib

    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(material, '_ctx', boom)
    monkeypatch.setattr(_lib, 'Context', boom)


def arg_types(txt, name):
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, txt)
    assert m, name
    args = [re.sub(r'\s+', ' ', a.strip()) for a in m.group(1).split(',')]
    return [re.sub(r'\s*\b\w+$', '', a).replace(' *', '*') if not a.endswith('*') else a.replace(' *', '*') for a in args]


def test_entry_points_in_header_and_library():
    from pylabfea_amd import _lib
    lib = _lib.load()
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'plfx.h')).read(), flags=re.S)
    for name, want in ENTRY_POINTS.items():
        assert arg_types(txt, name) == want, name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    # the entry points they extend keep their argument lists
    assert arg_types(txt, 'plfx_full_yf_batch') == ENTRY_POINTS['plfx_full_yf_batch_tid'][:-1]
    assert arg_types(txt, 'plfx_response_batch') == ENTRY_POINTS['plfx_response_batch_tid'][:-1]


@pytest.mark.parametrize('T', [1, 2, 6])
@pytest.mark.parametrize('desc,dev', FITS)
def test_fold_textures_is_fold_texture_row_by_row(z, mats, desc, dev, T, no_device):
    import pylabfea_amd as FE
    p, tex = TC.tables(z, desc, dev), TC.textures(z, desc)[:T]
    m = TB.parent(FE, mats[desc], p)
    F = m.fold_textures(tex)
    assert F['dual'].shape == (T, len(p['sv'])) and F['dual'].flags['C_CONTIGUOUS']
    for t in range(T):
        f = m.fold_texture(tex[t])
        assert np.array_equal(F['dual'][t], f['dual']), t
        for k in ('sv', 'scale'):
            assert np.array_equal(F[k], f[k]), k
        assert (F['intercept'], F['gamma'], F['dev_only']) == (f['intercept'], f['gamma'], f['dev_only'])


def test_fold_textures_shapes(z, mats, no_device):
    import pylabfea_amd as FE
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    q10, t10 = TC.widen(p, tex, 10)
    for q, t in ((TC.cut(p, nsv=1), tex[:3]), (q10, t10[:4]), (TC.cut(p, tdim=1), np.ascontiguousarray(tex[:5, :1]))):
        m = TB.parent(FE, mats['GSH_3'], q)
        F = m.fold_textures(t)
        assert F['dual'].shape == (len(t), len(q['sv'])) and F['sv'].shape == (len(q['sv']), 6)
        for k in range(len(t)):
            assert np.array_equal(F['dual'][k], m.fold_texture(t[k])['dual'])


def test_at_textures_errors_and_what_it_carries(z, mats, no_device):
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    m = TB.parent(FE, mats['GSH_3'], p, khard=50.)
    nanrow = tex[:3].copy()
    nanrow[1, 1] = np.nan
    for bad in (tex[0], tex[:, :2], np.zeros((0, 3)), tex[None, :2], nanrow, np.full((2, 3), np.inf)):
        with pytest.raises(ValueError, match='tex must be'):
            m.at_textures(bad)
        with pytest.raises(ValueError, match='tex must be'):
            m.fold_textures(bad)
    j2 = FE.Material('J2')
    j2.elasticity(E=200.e3, nu=0.3)
    j2.plasticity(sy=100., sdim=6)
    with pytest.raises(NotImplementedError, match='texture material'):
        j2.at_textures(tex[:2])
    with pytest.raises(AttributeError, match='train_SVC'):
        mats['GSH_3'].at_textures(tex[:2])                          # from_data alone: untrained
    key = m._tex_key()
    F = m.at_textures(tex[1:5], name='field')
    assert m._tex_key() == key and m._bound is None and m.txdat    # the parent is untouched
    assert F.name == 'field' and F._bound['parent'] is m and np.array_equal(F._bound['tex'], tex[1:5])
    b = m.at_texture(tex[1])
    for k in ('E', 'nu', 'sy', 'khard', 'sdim', 'gam_yf', 'dev_only', 'scale_seq', 'ML_yf', 'hill_6p'):
        assert getattr(F, k) == getattr(b, k), k
    assert np.array_equal(F.CV, b.CV) and np.array_equal(F.hill, b.hill)
    assert np.array_equal(F.svc['sv'], b.svc['sv']) and np.array_equal(F.svc['dual'], b.svc['dual'])   # row 0
    assert np.array_equal(F._bound['scale'], b._bound['scale'])
    assert F._bound['coef'].shape == (4, len(p['sv']))
    for t in range(4):
        assert np.array_equal(F._bound['coef'][t], m.fold_texture(tex[1 + t])['dual'])
    rec, keep = F._record(np.array(F.CV))
    assert rec.kind == _lib.SVC6_COLS and rec.nsv == len(p['sv']) and rec.khard == 50.
    assert np.array_equal(keep[2], b._bound['scale']) and np.array_equal(keep[3], F._bound['coef'])
    assert len(b._record(np.array(b.CV))[1]) == 3                   # at_texture: the record it had
    # the key covers the coefficient table
    k0 = F._content_key()
    assert m.at_textures(tex[1:5])._content_key() == k0
    assert m.at_textures(tex[1:4])._content_key() != k0 and b._content_key() != k0
    assert m.at_textures(tex[[1, 2, 3, 5]])._content_key() != k0
    F._bound['coef'][3, 0] += 1.
    assert F._content_key() != k0


def test_tex_id_errors(z, mats, no_device):
    import pylabfea_amd as FE
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    m = TB.parent(FE, mats['GSH_3'], p)
    F, b = m.at_textures(tex[:3]), m.at_texture(tex[0])
    sig, CV = z['probe_sig'][:4], np.array(m.CV)
    zero, deps = np.zeros((4, 6)), np.full((4, 6), 1e-4)
    j2 = FE.Material('J2')
    j2.elasticity(E=200.e3, nu=0.3)
    j2.plasticity(sy=100., sdim=6)
    # tex_id on any other material
    for other in (b, m, j2):
        calls = [lambda: other.response(sig[0], zero[0], deps[0], CV, tex_id=1),
                 lambda: other.response_batch(sig, zero, deps, CV, tex_id=np.zeros(4, dtype=int)),
                 lambda: other.ML_full_yf(sig, tex_id=0), lambda: other.calc_yf(sig, tex_id=0),
                 lambda: other.calc_fgrad(sig, tex_id=0), lambda: other.yield_scale(sig, tex_id=0),
                 lambda: other.yield_stress(sig, tex_id=0)]
        for k, call in enumerate(calls):
            with pytest.raises(NotImplementedError, match='at_textures'):
                call()
    # an index outside 0..T-1, a wrong shape, a wrong dtype
    for bad in (3, -1, np.array([0, 1, 2, 3]), np.array([0, -1, 0, 0])):
        for call in (lambda: F.response_batch(sig, zero, deps, CV, tex_id=bad), lambda: F.ML_full_yf(sig, tex_id=bad),
                     lambda: F.calc_yf(sig, tex_id=bad), lambda: F.calc_fgrad(sig, tex_id=bad),
                     lambda: F.yield_scale(sig, tex_id=bad), lambda: F.yield_stress(sig, tex_id=bad)):
            with pytest.raises(ValueError, match='outside 0..2'):
                call()
    for bad in (3, -1):
        with pytest.raises(ValueError, match='outside 0..2'):
            F.response(sig[0], zero[0], deps[0], CV, tex_id=bad)
    for bad in (np.zeros(3, dtype=int), np.zeros((4, 1), dtype=int), np.zeros(4), 1.0):
        with pytest.raises(ValueError, match='tex_id must be'):
            F.response_batch(sig, zero, deps, CV, tex_id=bad)
        with pytest.raises(ValueError, match='tex_id must be'):
            F.ML_full_yf(sig, tex_id=bad)
    with pytest.raises(ValueError, match='tex_id must be'):
        F.response(sig[0], zero[0], deps[0], CV, tex_id=np.array([0, 1]))
    for call in (lambda: F.calc_yf(sig, tex=tex[0]), lambda: F.calc_fgrad(sig, tex=tex[0]), lambda: F.yield_scale(sig, tex=tex[0])):
        with pytest.raises(ValueError, match='takes no tex'):
            call()


def field_model(FE, mats, NX=4, NY=3):
    fe = FE.Model(dim=2, planestress=True)
    fe.geom([2., 1.], LY=2.)
    fe.assign(mats)
    return fe


def test_set_texture_ids_errors(z, mats, no_device):
    import pylabfea_amd as FE
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    m = TB.parent(FE, mats['GSH_3'], p)
    F = m.at_textures(tex[:3])
    fe = field_model(FE, [F, F])
    assert fe.texture_ids is None
    with pytest.raises(RuntimeError, match='mesh'):
        fe.set_texture_ids(np.zeros((4, 3), dtype=int))
    fe.mesh(NX=4, NY=3)
    assert np.array_equal(fe.texture_ids, np.zeros(12, dtype=np.int32))           # without a call: row 0 everywhere
    for bad in (np.zeros((3, 4), dtype=int), np.zeros(11, dtype=int), np.zeros((4, 3, 1), dtype=int), 0):
        with pytest.raises(ValueError, match='ids must be'):
            fe.set_texture_ids(bad)
    for bad in (np.zeros((4, 3)), np.zeros(12, dtype=bool), np.zeros(12, dtype=object)):
        with pytest.raises(TypeError, match='int array'):
            fe.set_texture_ids(bad)
    ids = np.arange(12).reshape(4, 3) % 3
    fe.set_texture_ids(ids)
    assert np.array_equal(fe.texture_ids, ids.reshape(-1)) and fe.texture_ids.dtype == np.int32   # element j*NY + k
    with pytest.raises(ValueError):
        fe.texture_ids[0] = 1                                                      # read-only
    with pytest.raises(AttributeError):
        fe.texture_ids = ids
    fe.set_texture_ids(ids.reshape(-1)[::-1])                                      # flat, element order
    assert np.array_equal(fe.texture_ids, ids.reshape(-1)[::-1])
    fe.mesh(NX=4, NY=3)                                                            # cleared by mesh()
    assert np.array_equal(fe.texture_ids, np.zeros(12, dtype=np.int32))
    # an entry outside 0..T-1 of a field-material element: ValueError when the engine is set up, before the device is reached
    # (the no_device fixture fails the test if a context is created)
    fe.set_texture_ids(np.full(12, 3))
    with pytest.raises(ValueError, match='outside 0..2'):
        fe._send_texture_ids(None)
    # entries of elements of other materials are ignored
    fe2 = field_model(FE, [F, m.at_texture(tex[0])])
    fe2.mesh(NX=4, NY=3)
    ids = np.zeros((4, 3), dtype=int)
    ids[fe2._mat_id.reshape(4, 3) == 1] = 99

    class Eng:
        sent = None

        def set_element_textures(self, a):
            self.sent = a
    eng = Eng()
    fe2._e0, fe2._e1 = 0, 12
    fe2.set_texture_ids(ids)
    fe2._send_texture_ids(eng)
    assert np.array_equal(eng.sent, ids.reshape(-1))
    eng.sent = None
    fe2._send_texture_ids(eng)                                                     # unchanged: not sent again
    assert eng.sent is None


def test_gated_methods_and_model_refusals(z, mats, tmp_path, no_device):
    import pylabfea_amd as FE
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    m = TB.parent(FE, mats['GSH_3'], p)
    F = m.at_textures(tex[:3])
    sig = z['probe_sig'][0]
    calls = {
        'calc_hessian': lambda: F.calc_hessian(sig),
        'flow_curve': lambda: F.flow_curve(sig[None]),
        'polar_yield_locus': lambda: F.polar_yield_locus(),
        'yield_slices': lambda: F.yield_slices(),
        'setup_fgrad_SVM': lambda: F.setup_fgrad_SVM(),
        'train_SVC': lambda: F.train_SVC(),
        'export_MLparam': lambda: F.export_MLparam('script', path=str(tmp_path)),
        'Committee': lambda: FE.Committee([F]),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match='at_texture') as e:
            call()
        assert name in str(e.value), name
    with pytest.raises(NotImplementedError, match='bind one texture with at_texture') as e:
        F.calc_properties()
    assert 'calc_properties' in str(e.value)
    assert F.get_sflow(np.array([1e-3, -5e-4, -5e-4, 0., 0., 0.])) == F.sy + 1e-3 * F.khard
    fe = field_model(FE, [F, m.at_texture(tex[1])])                # supported: nothing raised
    with pytest.raises(NotImplementedError, match='Model.distribute') as e:
        fe.distribute(0, 2, b'x' * 128)
    with pytest.raises(NotImplementedError, match='Model.distribute') as e2:
        field_model(FE, [m.at_texture(tex[1])] * 2).distribute(0, 2, b'x' * 128)
    assert str(e.value) == str(e2.value)                            # the bound material's message
    fe2 = FE.Model(dim=2, planestress=True)
    fe2.geom([2.], LY=2.)
    fe2.distribute(0, 2, b'x' * 128)
    with pytest.raises(NotImplementedError, match='Model.distribute'):
        fe2.assign([F])
    with pytest.raises(NotImplementedError, match='reference'):     # the parent is still refused
        fe.assign([m, m])

"""What of Material.load_path needs no GPU: the entry points in the header and in the built library, every
refusal and argument error of the façade (all raised before the device is touched), the rules by which the number of points
follows from the arguments, the parsing of `control`, and the NumPy restatement of the iteration on the CPU oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flow_curve_cases as FC
import load_path_cases as LP
import pylabfea_amd as FE
from pylabfea_amd import _lib
from svr_flow_cases import install_svr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_in_header_and_library():
    txt = open(os.path.join(ROOT, 'include', 'plfx.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    m = re.search(r'int\s+plfx_load_path\s*\(([^)]*)\)\s*;', code)
    assert m, 'plfx_load_path is not declared'
    args = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args == ['plfx_ctx *ctx', 'int mat', 'int n', 'int K', 'const double *dload', 'int shared', 'const int32_t *control',
                    'const double *sig0', 'const double *epl0', 'const int32_t *tex_id', 'int maxit', 'int newton',
                    'double stol', 'double eps_cap', 'double *sig', 'double *epl', 'double *deps', 'double *fy',
                    'int32_t *nsteps', 'int32_t *newton_out', 'int32_t *ksteps', 'int32_t *status', 'double *ct']
    assert re.search(r'int\s+plfx_load_path_info\s*\(\s*plfx_ctx \*ctx,\s*int64_t \*launches\s*\)\s*;', code)
    lib = _lib.load()
    assert hasattr(lib, 'plfx_load_path') and hasattr(lib, 'plfx_load_path_info')
    assert 'plfx_load_path' in _lib.SYMBOLS and 'plfx_load_path_info' in _lib.SYMBOLS
    assert callable(_lib.Context.load_path) and callable(_lib.Context.load_path_info)
    assert lib.plfx_load_path_info(None, None) == -2                       # no context: an argument error, nothing touched
    assert lib.plfx_load_path(None, 0, 1, 1, None, 0, None, None, None, None, 50, 30, C.c_double(1.), C.c_double(0.05),
                              *([None] * 9)) == -3


class FakeContext:
    """stands in for the point context: records what the façade hands to the library"""
    def __init__(self):
        self.calls = []

    def load_path(self, mat, dload, **kw):
        self.calls.append(dict(kw, mat=mat, dload=dload))
        return dict(ok=True)


@pytest.fixture
def hill(monkeypatch):
    m = FC.hill_material(FE)
    ctx = FakeContext()
    monkeypatch.setattr(m, '_load', lambda CV=None, ana=False: ctx)
    return m, ctx


def test_number_of_points_follows_from_the_arguments(hill):
    m, ctx = hill
    d3, d2 = np.zeros((4, 5, 6)), np.zeros((4, 6))
    state = dict(khard=m.khard, msg=dict(m.msg))

    def n_of(*a, **kw):
        assert m.load_path(*a, **kw) == dict(ok=True)
        return ctx.calls[-1]
    c = n_of(d3)
    assert c['dload'].shape == (4, 5, 6) and c['control'] is None and c['sig0'] is None and c['epl0'] is None and c['tex_id'] is None
    assert c['maxit'] == 50 and c['newton'] == 30 and c['stol'] == 1.e-9 * m.sy and c['eps_cap'] == 0.05 and c['mat'] == 0
    assert c['return_tangent'] is False
    c = n_of(d2)                                                            # a shared path and nothing else: one point
    assert c['dload'].shape == (4, 6) and c['sig0'] is None
    c = n_of(d2, sig0=np.ones(6), epl0=np.zeros(6))                         # (6,) rows do not set N
    assert c['sig0'].shape == (1, 6) and c['epl0'].shape == (1, 6)
    c = n_of(d2, sig0=np.ones((7, 6)))                                      # N from sig0
    assert c['sig0'].shape == (7, 6)
    c = n_of(d2, epl0=np.zeros((3, 6)), sig0=np.ones(6))                    # N from epl0; the (6,) row is repeated
    assert c['epl0'].shape == (3, 6) and c['sig0'].shape == (3, 6) and np.all(c['sig0'] == 1.)
    c = n_of(d2, control=np.array([[True] + [False] * 5] * 4))             # N from a 2-d control
    assert c['control'].tolist() == [1, 1, 1, 1]
    c = n_of(d3, control=[False, True, False, False, False, True], sig0=np.ones(6))   # a (6,) mask is shared
    assert c['control'].tolist() == [34] * 5 and c['sig0'].shape == (5, 6)
    c = n_of(d3, control=[False] * 6)                                       # nothing stress-controlled: strain control
    assert c['control'] is None
    for kw in (dict(sig0=np.ones((4, 6))), dict(epl0=np.ones((6, 6))), dict(control=np.zeros((2, 6), dtype=bool))):
        with pytest.raises(ValueError, match='the number of points differs'):
            m.load_path(d3, **kw)
    with pytest.raises(ValueError, match='the number of points differs'):
        m.load_path(d2, sig0=np.ones((4, 6)), epl0=np.ones((5, 6)))
    assert m.khard == state['khard'] and m.msg == state['msg']             # neither khard nor msg is touched


def test_control_parsing():
    bits, n = FE.Material._path_control(None)
    assert bits is None and n is None
    bits, n = FE.Material._path_control([True, False, False, False, False, True])
    assert bits.tolist() == [33] and n is None and bits.dtype == np.int32
    bits, n = FE.Material._path_control(np.array([[False] * 6, [True] * 6, [False, True, True, True, True, True]]))
    assert bits.tolist() == [0, 63, 62] and n == 3
    for bad in ([1, 0, 0, 0, 0, 0], np.zeros(6), np.zeros(5, dtype=bool), np.zeros((2, 3, 6), dtype=bool), True,
                np.zeros((6, 2), dtype=bool)):
        with pytest.raises(ValueError, match='control must be None'):
            FE.Material._path_control(bad)


def test_argument_errors_come_before_the_device(hill):
    m, ctx = hill
    d = np.zeros((3, 2, 6))
    for bad in (np.zeros(6), np.zeros((3, 2, 5)), np.zeros((2, 3, 2, 6))):
        with pytest.raises(ValueError, match='dload must be'):
            m.load_path(bad)
    for name in ('sig0', 'epl0'):
        for bad in (np.zeros(3), np.zeros((2, 5)), np.zeros((1, 2, 6))):
            with pytest.raises(ValueError, match='%s must be None' % name):
                m.load_path(d, **{name: bad})
    for kw, msg in ((dict(maxit=0), 'maxit must be >= 1'), (dict(newton=-1), 'newton must be >= 0'),
                    (dict(stol=0.), 'stol must be finite and positive'), (dict(stol=-1.), 'stol must be finite and positive'),
                    (dict(stol=np.inf), 'stol must be finite and positive'), (dict(stol=np.nan), 'stol must be finite and positive'),
                    (dict(eps_cap=0.), 'eps_cap must be finite and positive'), (dict(eps_cap=np.inf), 'eps_cap must be finite'),
                    (dict(sig0=np.full(6, np.nan)), 'sig0 must be finite'), (dict(epl0=np.full((2, 6), np.inf)), 'epl0 must be finite'),
                    (dict(tex_id=0), 'tex_id needs a material with a texture field')):
        with pytest.raises((ValueError, NotImplementedError), match=msg):
            m.load_path(d, **kw)
    nan = d.copy()
    nan[1, 0, 2] = np.nan
    with pytest.raises(ValueError, match='dload must be finite'):
        m.load_path(nan)
    big = d.copy()
    big[2, 1, 4] = -0.051
    with pytest.raises(ValueError, match='beyond eps_cap = 0.05'):
        m.load_path(big)
    with pytest.raises(ValueError, match='beyond eps_cap = 0.05'):
        m.load_path(big, control=[[False] * 6, [True, True, True, True, False, True]])
    assert not ctx.calls
    m.load_path(big, control=[[False] * 6, [False, False, False, False, True, False]])   # a stress increment is not capped
    m.load_path(big, eps_cap=0.06)
    m.load_path(big[:, 1], control=[False, False, False, False, True, False])
    assert len(ctx.calls) == 3
    e = LP.elastic_material(FE)
    with pytest.raises(ValueError, match='stol must be given for a material without yield strength'):
        e.load_path(d, control=[True] * 6)


def test_refusals():
    d = np.zeros((2, 6))
    m3, _ = FC.YC.facade_ml('hill')
    m3.sdim = 3
    with pytest.raises(NotImplementedError, match='load_path: not offered for sdim = 3 ML yield functions'):
        m3.load_path(d)
    mw, _ = FC.wh_material()
    with pytest.raises(NotImplementedError, match='load_path: not offered for work-hardening ML yield functions'):
        mw.load_path(d)
    mg, _ = FC.wh_material()
    install_svr(mg, np.load(os.path.join(FC.GOLD, 'svr_gradient.npz')))
    with pytest.raises(NotImplementedError, match='load_path: ML_grad is set'):
        mg.load_path(d)
    mg.enable_svr_flow()
    with pytest.raises(NotImplementedError, match='load_path: ML_grad is set'):
        mg.load_path(d)
    mx, _ = FC.svc6_material()
    mx.txdat = True
    with pytest.raises(NotImplementedError, match='load_path: not offered for a texture material.*at_texture'):
        mx.load_path(d)
    mt = FE.Material()
    mt.elasticity(E=200.e3, nu=0.3)
    mt.plasticity(sy=100., tresca=True, sdim=6)
    with pytest.raises(NotImplementedError, match='load_path: Tresca has no flow rule'):
        mt.load_path(d)
    mb = FC.YC.analytic(FE, 'abarlat')
    with pytest.raises(NotImplementedError, match='load_path: Barlat has no flow rule.*enable_barlat_normal'):
        mb.load_path(d)


def test_the_oracle_iteration_completes_the_recorded_cases():
    """the CPU record behind the mixed-control cases: every path completes, within 30 corrections per step; the r-value of
    the uniaxial path from its second plastic step on"""
    z = np.load(os.path.join(FC.GOLD, 'material_hill6.npz'))
    from oracle import oracle as O
    om = O.Material.from_golden(z)
    sy, E, hill = float(z['par_sy']), float(z['par_E']), z['par_hill']
    dload, control = LP.mixed_paths(sy, E)
    stol = 1.e-9 * sy
    worst = 0
    for i, (name, _, _) in enumerate(LP.MIXED):
        r = LP.oracle_load_path(om, z['rpe_CV'], dload[:, i], control[i], stol)
        assert r['status'] == 0 and r['ksteps'] == LP.K_MIXED, name
        t = np.cumsum(dload[:, i], axis=0)
        assert np.all(np.abs(r['sig'] - t)[:, control[i]] <= stol), name
        assert np.array_equal(r['deps'][:, ~control[i]], dload[:, i][:, ~control[i]])
        worst = max(worst, int(r['newton'].max()))
    assert 1 <= worst <= 30
    r = LP.oracle_load_path(om, z['rpe_CV'], dload[:, 0], control[0], stol)
    q, k0 = LP.r_ratio(r['depl'])
    dev = float(np.max(np.abs(q / (hill[0] / hill[2]) - 1.)))
    print('oracle iteration: worst corrections per step %d, r-value deviation %.3e from step %d' % (worst, dev, k0))
    assert dev < 1.e-8
    # full stress control across the yield point of a weakly hardening material: the documented limit
    d = np.zeros((24, 6))
    d[:, 0] = 5.
    r = LP.oracle_load_path(om, z['rpe_CV'], d, [True] * 6, stol)
    assert r['status'] == 1 and 0 < r['ksteps'] < 24

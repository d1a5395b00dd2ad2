"""Host side of the flow rule and stress update of texture materials, no GPU: the three entry points of the
C-ABI in the header and in the built library, the argument checks of the façade's ``tex=`` branches (all raised before the
device is touched), the unchanged refusals without ``tex``, and the NumPy transcription of the gradient
(tests/texture_flow_cases.py) held against central differences of its own yield function."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

import texture_cases as TC
import texture_flow_cases as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the argument lists of the issue, types only
SIGNATURES = {
    'plfx_tex_svc_fgrad': 'plfx_ctx*, int, const double*, int, const double*, const int32_t*, double*',
    'plfx_tex_svc_full_yf': 'plfx_ctx*, int, const double*, int, const double*, const int32_t*, double*, int32_t*',
    'plfx_tex_svc_response': 'plfx_ctx*, int, int, const double*, const double*, const double*, int, const double*, '
                             'const int32_t*, int, double*, double*, double*, double*, int32_t*',
}


@pytest.fixture(scope='module')
def z():
    return TC.load()


@pytest.fixture(scope='module')
def mats(z, tmp_path_factory):
    import pylabfea_amd as FE
    d = tmp_path_factory.mktemp('texture_db')
    return {desc: TC.facade(FE, z, d, desc) for desc in TC.DESCRIPTORS}


def trained(z, mats, desc='GSH_3'):
    import pylabfea_amd as FE
    m = FE.Material('tex')
    with contextlib.redirect_stdout(io.StringIO()):
        m.from_data(list(mats[desc][0].msparam))
    return TC.install(m, TC.tables(z, desc)), TC.textures(z, desc)


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to reach the device fails the test"""
    from pylabfea_amd import material

    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(material, '_ctx', boom)


def test_symbols_and_argument_lists():
    from pylabfea_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, 'include', 'plfx.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name, want in SIGNATURES.items():
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, txt)
        assert m, name
        types = [re.sub(r'\s*\b\w+$', '', a.strip()).replace(' *', '*') for a in m.group(1).replace('\n', ' ').split(',')]
        assert ', '.join(types) == want, (name, types)
    assert hasattr(lib, 'plfx_tex_svc_flow_info') and hasattr(lib, 'plfx_tex_svc_info')


def test_tex_argument_errors_before_the_device(z, mats, no_device):
    m, tex = trained(z, mats)
    sig, CV = z['probe_sig'], np.array(m.CV)
    e6, d6 = np.zeros(6), np.full(6, 1e-4)
    bad_shapes = (tex[0][:2], tex[:3], np.zeros((2, 2, 3)), np.zeros((4, 4)))
    for bad in bad_shapes:                                      # (tdim,) or (N, tdim) with N the number of stresses
        for call in (lambda: m.calc_fgrad(sig[:4], tex=bad), lambda: m.ML_full_yf(sig[:4], tex=bad),
                     lambda: m.response_batch(sig[:4], np.zeros((4, 6)), np.full((4, 6), 1e-4), CV, tex=bad)):
            with pytest.raises(ValueError, match='tex must be'):
                call()
    for bad in (tex[0][:2], tex[:2], tex[:1].T):
        for call in (lambda: m.response(sig[0], e6, d6, CV, tex=bad), lambda: m.epl_dot(sig[0], e6, CV, d6, tex=bad),
                     lambda: m.C_tan(sig[0], CV, tex=bad)):
            with pytest.raises(ValueError, match='tex must be'):
                call()
    with pytest.raises(NotImplementedError, match='ld'):
        m.ML_full_yf(sig[0], ld=np.ones(6), tex=tex[0])
    with pytest.raises(ValueError, match='maxit'):
        m.response(sig[0], e6, d6, CV, maxit=0, tex=tex[0])
    with pytest.raises(ValueError):
        m.response(sig[:2], e6, d6, CV, tex=tex[0])             # one stress only, as without tex
    with pytest.raises(ValueError, match='same shape'):
        m.calc_fgrad(sig[:4], epl=np.zeros(6), tex=tex[0])
    with pytest.raises(ValueError, match=r'\(N, 6\)'):
        m.response_batch(sig[:4], np.zeros((3, 6)), np.full((4, 6), 1e-4), CV, tex=tex[0])
    with pytest.raises(ValueError, match='khard_in'):
        m.response_batch(sig[:4], np.zeros((4, 6)), np.full((4, 6), 1e-4), CV, khard_in=np.zeros(4), tex=tex[0])
    m.khard = 100.                                              # texture and work hardening are not combined
    with pytest.raises(NotImplementedError, match='hardening'):
        m.ML_full_yf(sig[0], epl=np.full(6, 1e-3), tex=tex[0])
    m.khard = 0.


def test_tex_needs_a_texture_material(z, mats, no_device):
    import pylabfea_amd as FE
    m = FE.Material('J2')
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=100., sdim=6)
    sig, CV, t = z['probe_sig'], np.array(m.CV), np.zeros(3)
    e6, d6 = np.zeros(6), np.full(6, 1e-4)
    for call in (lambda: m.calc_fgrad(sig[0], tex=t), lambda: m.ML_full_yf(sig[0], tex=t),
                 lambda: m.response(sig[0], e6, d6, CV, tex=t),
                 lambda: m.response_batch(sig[:2], np.zeros((2, 6)), np.full((2, 6), 1e-4), CV, tex=t),
                 lambda: m.epl_dot(sig[0], e6, CV, d6, tex=t), lambda: m.C_tan(sig[0], CV, tex=t)):
        with pytest.raises(NotImplementedError, match='texture material'):
            call()


def test_refusals_without_tex_are_unchanged(z, mats, tmp_path, no_device):
    """the calls of tests/test_texture_cpu.py::test_refused_methods: still NotImplementedError that names the method and says
    what the reference does; the four that ``tex=`` runs now say so"""
    import pylabfea_amd as FE
    m, tex = trained(z, mats)
    sig, CV = z['probe_sig'][0], np.array(m.CV)
    calls = {
        'calc_fgrad': lambda: m.calc_fgrad(sig),
        'ML_full_yf': lambda: m.ML_full_yf(sig),
        'response': lambda: m.response(sig, np.zeros(6), np.full(6, 1e-4), CV),
        'response_batch': lambda: m.response_batch(sig[None], np.zeros((1, 6)), np.full((1, 6), 1e-4), CV),
        'calc_hessian': lambda: m.calc_hessian(sig, tex=tex[0]),
        'calc_properties': lambda: m.calc_properties(),
        'setup_fgrad_SVM': lambda: m.setup_fgrad_SVM(),
        'export_MLparam': lambda: m.export_MLparam('script', path=str(tmp_path)),
        'polar_yield_locus': lambda: m.polar_yield_locus(),
        'yield_slices': lambda: m.yield_slices(),
        'flow_curve': lambda: m.flow_curve(sig[None]),
        'Committee': lambda: FE.Committee([m]),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match='reference') as e:
            call()
        assert name in str(e.value), name
        assert ('tex=' in str(e.value)) == (name in ('calc_fgrad', 'ML_full_yf', 'response', 'response_batch')), name
    fe = FE.Model(dim=2, planestress=True)
    fe.geom([2.], LY=2.)
    with pytest.raises(NotImplementedError, match='reference'):
        fe.assign([m])
    with pytest.raises(ValueError, match='no texture data is given'):      # epl_dot / C_tan without tex: as before
        m.epl_dot(sig, np.zeros(6), CV, np.full(6, 1e-4))
    with pytest.raises(NotImplementedError, match='calc_fgrad'):
        m.C_tan(sig, CV)


@pytest.mark.parametrize('dev', [False, True])
@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_gradient_transcription_against_central_differences(z, desc, dev):
    """The transcription's gradient is the derivative of the transcription's calc_yf: central differences at h = 1e-4 sy differ
    from it by their truncation error -- below the bound of fd_truncation_bound, and four times smaller at half the step.
    fd_gap, the worst gap, is what the GPU test of the device's own differences adds to its bar."""
    p, tex = TC.tables(z, desc, dev), TC.textures(z, desc)
    sy = float(z['fd_%s_sy' % desc])
    sig, tid = z['probe_sig'][:16], z['probe_tex_id'][:16]
    h = 1e-4 * sy
    a = TF.gradient(p, sig, tex[tid])
    gap = TF.fd_gap(p, sig, tex[tid], h)
    half = TF.fd_gap(p, sig, tex[tid], 0.5 * h)
    bound = TF.fd_truncation_bound(p, h)
    print('%s dev %d: fd_gap %.3e (h / 2: %.3e), bound %.3e, max|a| %.3e' % (desc, dev, gap, half, bound, float(np.max(np.abs(a)))))
    assert np.all(np.isfinite(np.asarray(a, dtype=float))) and float(np.max(np.abs(a))) > 0.
    assert gap <= bound
    assert half <= 0.3 * gap                                               # second order: the gradient is the derivative
    if dev:                                                                # no hydrostatic part
        assert float(np.max(np.abs(np.sum(a[:, :3], axis=1)))) <= 1e-15 * float(np.max(np.abs(a)))
    # the FP64 form of the same formulas agrees with the longdouble one within the calibration
    a64 = TF.gradient(p, sig, tex[tid], LD=np.float64)
    assert float(np.max(np.abs(a64 - a))) <= TF.grad_bar(TF.calib(p, sig, tex[tid])[1], a)

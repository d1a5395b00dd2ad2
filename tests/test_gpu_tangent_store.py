"""The element tangent store: tangents kept as a form tag plus what the form needs -- nothing for the
elastic CV, 7 factors for a one-step plastic return, 21 entries otherwise -- must look to every reader exactly like the
21-entry store it replaced: state_set / state_get, the change test of the sweep, and whole solves against the CPU oracle."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1.e-6


def FE():
    import pylabfea_amd
    return pylabfea_amd


def hill(num=1, sy=100.):
    m = FE().Material(num=num)
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=sy, hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=100., sdim=6)
    return m


def mixed_model(n, eps):
    """Hill | elastic | softer Hill sections"""
    el = FE().Material(num=3)
    el.elasticity(E=50.e3, nu=0.25)
    fe = FE().Model(dim=2, planestress=False)
    fe.geom([2, 1, 2], LY=5.)
    fe.assign([hill(1), el, hill(2, 60.)])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(eps * fe.leny, 'disp')
    fe.mesh(NX=n, NY=n)
    return fe


def element_CV(fe):
    cv = np.stack([fe._element_CV(m).reshape(36) for m in fe.mat])
    return cv[np.asarray(fe._mat_id)]


def close(a, b, scale=None, rtol=RTOL):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    s = np.max(np.abs(b)) if scale is None else scale
    return np.max(np.abs(a - b)) <= rtol * max(s, 1e-300)


def test_state_set_get_roundtrip():
    from pylabfea_amd import _lib
    fe = mixed_model(12, 0.001)
    eng = fe._ensure_engine()
    D0 = eng.state_get(_lib.ST_ELSTIFF).reshape(-1, 36)
    assert np.array_equal(D0, element_CV(fe))         # after the reset every tangent is its material's CV
    rng = np.random.default_rng(5)
    A = rng.standard_normal((fe.Nel, 6, 6)) * 1.e5
    A = A + A.transpose(0, 2, 1)                       # arbitrary symmetric tangents
    eng.state_set(_lib.ST_ELSTIFF, A.reshape(-1, 36))
    assert np.array_equal(eng.state_get(_lib.ST_ELSTIFF).reshape(-1, 6, 6), A)


@pytest.mark.parametrize('nit', [1, 15])
def test_sweep_sees_set_tangents(nit):
    """A sweep with du = 0 answers every plastic element with an elastic step (new tangent CV): exactly the elements whose
    tangent state_set moved away from CV are rewritten -- with CV, or at K-iteration >= 15 with the average of both."""
    from pylabfea_amd import _lib
    fe = mixed_model(12, 0.001)
    eng = fe._ensure_engine()
    cv = element_CV(fe)
    plastic = np.asarray(fe._mat_id) != 1
    moved = plastic & (np.arange(fe.Nel) % 3 == 0)
    D = cv.copy()
    D[moved, 1] += 1.e-2                               # entries (0, 1) and (1, 0): Frobenius change 1.4e-2 > 1e-3
    D[moved, 6] += 1.e-2
    D[~plastic, 5] += 1.e-2                            # elastic-material elements are skipped by the sweep: kept as set
    D[~plastic, 30] += 1.e-2
    eng.state_set(_lib.ST_ELSTIFF, D)
    eng.state_set(_lib.ST_DU, np.zeros_like(eng.state_get(_lib.ST_DU)))
    r0 = eng.sweep_info()[1]
    changed, _ = eng.sweep(nit)
    assert changed
    assert eng.sweep_info()[1] - r0 == int(moved.sum())
    want = D.copy()
    want[moved] = cv[moved] if nit < 15 else 0.5 * (cv[moved] + D[moved])
    assert np.array_equal(eng.state_get(_lib.ST_ELSTIFF), want)
    # and a second sweep finds nothing to rewrite
    r1 = eng.sweep_info()[1]
    eng.sweep(1)
    assert eng.sweep_info()[1] - r1 == (int(moved.sum()) if nit >= 15 else 0)


def test_mixed_model_vs_oracle():
    """Elastic-material section, one-step Hill elements and 50-sub-step corrector elements in one solve, against the CPU
    oracle's sparse direct solve at the bars of test_gpu_model.test_full_size_vs_oracle_inclusion."""
    from oracle.solve_ref import RefSolver
    from pylabfea_amd import _lib
    fe = mixed_model(24, 0.01)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=2)
        ref = RefSolver(mixed_model(24, 0.01)).solve(min_step=2)
    eng = fe._ensure_engine()
    assert np.sum(eng.state_get(_lib.ST_MAXSTEPS) >= 49) > 0          # the corrector ran
    assert np.sum(np.asarray(fe._mat_id) == 1) > 0
    assert fe.nsteps == ref.nsteps and list(fe.niter) == list(ref.niter)
    assert close(fe.u, ref.u) and close(fe._state('sig'), ref.sig)
    assert close(fe._state('epl'), ref.epl, scale=np.max(np.abs(ref.eps)))
    assert close(fe._state('elstiff').reshape(-1, 36), ref.elstiff, rtol=10 * RTOL)
    assert close(fe.sgl, ref.sgl)

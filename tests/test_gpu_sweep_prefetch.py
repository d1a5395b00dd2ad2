"""The streaming sweep and the end-of-step update issue every load that depends on the element index alone up front, and the
sweep has the streams of a thread's next tile in flight while it works on the current one.  None of that
may be seen in a result: a small mixed model -- an elastic-material section (tangents stay TAN_CV) and two Hill sections --
goes through whole solves, every sweep and every end-of-step update of them, against the CPU oracle, in the regime of
tests/test_gpu_tangent_store.py (eps 0.01: 6-13 stiffness iterations per load step, returns in one step and on the
50-sub-step corrector, i.e. factored and full tangents beside the elastic ones in front of the later sweeps).  A tag cannot
be read back, so only the elastic section and the corrector's visits are asserted; that factored tangents were in the store
is not.  (At eps 0.004 the last load step of the 15 x 15 and 25 x 25 meshes ends one stiffness iteration later than the
oracle's with the parent commit's library too -- a 1e-3 threshold met by a PCG solve here and an LU solve there -- so that
strain is no case of this test.)
The element grid has one block per 256-element tile up to 1024 blocks, so on a small mesh every thread runs one pass of the
tile loop and the prefetched tile is always wholly beyond the arrays.  test_mixed_model_edge_tiles_vs_oracle (225, 625, 1160
elements: a partial only tile, partial last tiles) therefore covers the hoisted loads and the predicated-off prefetch only.
test_live_prefetch_vs_oracle caps the grid with PLFX_SWEEP_BLOCKS (read when a mesh is set), so that threads run two or
three passes on heterogeneous data, consume the carried registers with live values, and prefetch a partial last tile:
one block over 625 elements (tiles 0, 1, 2), two blocks over 1160 (tiles 0, 2, 4 and 1, 3), three over 1160."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1.e-6   # the bar of tests/test_gpu_tangent_store.py for the same comparison


def FE():
    import pylabfea_amd
    return pylabfea_amd


def hill(num=1, sy=100.):
    m = FE().Material(num=num)
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=sy, hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=100., sdim=6)
    return m


def mixed_model(nx, ny, eps):
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
    fe.mesh(NX=nx, NY=ny)
    return fe


def close(a, b, scale=None, rtol=RTOL):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    s = np.max(np.abs(b)) if scale is None else scale
    return np.max(np.abs(a - b)) <= rtol * max(s, 1e-300)


def solve_vs_oracle(nx, ny, eps=0.01):
    from oracle.solve_ref import RefSolver
    from pylabfea_amd import _lib
    fe = mixed_model(nx, ny, eps)
    assert fe.Nel % 256 != 0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=2)
        ref = RefSolver(mixed_model(nx, ny, eps)).solve(min_step=2)
    eng = fe._ensure_engine()
    ms = eng.state_get(_lib.ST_MAXSTEPS).ravel()
    mat = np.asarray(fe._mat_id)
    cv = np.stack([fe._element_CV(m).reshape(36) for m in fe.mat])[mat]
    D = fe._state('elstiff').reshape(-1, 36)
    is_cv = np.all(D == cv, axis=1)
    assert np.all(is_cv[mat == 1]) and np.sum(mat == 1) > 0          # the elastic-material section: never rewritten
    assert np.sum(ms >= 49) > 0                                       # the corrector ran
    assert fe.nsteps == ref.nsteps and fe.nsteps >= 7 and list(fe.niter) == list(ref.niter)
    assert close(fe.u, ref.u) and close(fe._state('sig'), ref.sig)
    assert close(fe._state('eps'), ref.eps)
    assert close(fe._state('epl'), ref.epl, scale=np.max(np.abs(ref.eps)))
    assert close(D, ref.elstiff, rtol=10 * RTOL)
    assert close(fe.sgl, ref.sgl) and close(fe.egl, ref.egl)


@pytest.mark.parametrize('nx,ny', [(15, 15), (25, 25), (40, 29)])
def test_mixed_model_edge_tiles_vs_oracle(nx, ny):
    solve_vs_oracle(nx, ny)


@pytest.mark.parametrize('blocks,nx,ny', [(1, 25, 25), (2, 40, 29), (3, 40, 29)])
def test_live_prefetch_vs_oracle(monkeypatch, blocks, nx, ny):
    monkeypatch.setenv('PLFX_SWEEP_BLOCKS', str(blocks))
    assert (nx * ny + 255) // 256 > blocks      # more tiles than blocks: a thread takes a second pass
    solve_vs_oracle(nx, ny)

"""The multigrid V-cycle on the device (plfx_precond_apply) against the NumPy reference rebuilt from its definition
(tests/mg_reference.py), entry for entry, in every form the cycle has: which form ran is asserted through
plfx_mg_info, and the reference's level list must equal the reported one.

One model family: plane strain and plane stress, a Hill matrix with a softer Hill inclusion, left and bottom fixed, top
displaced, eight load steps, so that the tangents are plastic and differ from element to element.  The tangents come from
`_state('elstiff')`, the prescribed DOFs from the model.

Measured on an MI355X, worst test vector, max|z_dev - z_ref| / max|z_ref| (profiles/r21a_vcycle_vs_reference.txt):

    case                                          strain     stress     tail kernel, coarsest solver
    16 x 12 default                               1.8e-15    8.0e-16    tail_mf, dense
    16 x 12 nu = 1 / nu = 3 / omega = 0.5 / 0.8   2.0e-15    1.0e-15    tail (nu != 2), tail_mf; dense
    16 x 12 PLFX_MATFREE=0                        1.6e-15    1.7e-15    tail_lds, dense
    16 x 12 whole matrix, 442 columns             1.7e-15    8.9e-16    tail_mf, dense
    8 x 8 default / other smoothers / assembled   1.2e-15    7.1e-16    as 16 x 12
    35 x 33                                       7.7e-16    1.1e-15    tail_mf_ragged, dense
    36 x 33                                       6.2e-16    6.1e-16    tail_mf_ragged, dense
    35 x 33 PLFX_MATFREE=0                        1.1e-15    6.1e-16    tail_lds (four cell classes), dense
    36 x 33 PLFX_MATFREE=0                        8.4e-16    6.6e-16    tail_lds, dense
    70 x 66, PLFX_MG_GRAPH 0 and 1 (bit-equal)    1.2e-15    7.4e-16    launched level 1, tail_mf_ragged from level 2
    70 x 66 PLFX_MG_ODD=0, 35 steps, kappa 612.5  5.7e-15               no tail, Chebyshev    <- worst linear case
    70 x 66 PLFX_MG_ODD=0, 20 steps, kappa 100    1.5e-15               no tail, Chebyshev
    70 x 66 / 35 x 33, PLFX_MARCH 0 and 1         1.2e-15 / 7.7e-16     marching = gather form bit for bit
    40 x 36 PLFX_MG_ODD=0                         1.1e-11    1.2e-11    tail, in-LDS PCG      <- bound of its own

Bounds: tests/vcycle_cases.py (100 x the worst measured value: 5.7e-13, and 1.2e-9 for the in-LDS PCG; caps 1e-8 and 1e-6).
"""
import contextlib
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import mg_reference as R
import vcycle_cases as V

pytestmark = pytest.mark.gpu

STATES = ['strain', 'stress']


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def solved_model(nx, ny, state):
    """the model family of this file after eight load steps (call inside `environ`: the library reads its knobs when the
    engine and its hierarchy are made)"""
    import pylabfea_amd as FE
    m = FE.Material(name='matrix', num=1)
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=100., hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=100., sdim=6)
    s = FE.Material(name='inclusion', num=2)
    s.elasticity(E=60.e3, nu=0.25)
    s.plasticity(sy=60., hill=[1.2, 1., 0.8, 1., 1., 1.1], khard=300., sdim=6)
    fe = FE.Model(dim=2, planestress=(state == 'stress'))
    fe.geom(sect=2, LX=4., LY=4. * ny / nx)
    fe.assign([m, s])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.005 * fe.leny, 'disp')
    el = np.ones((nx, ny), dtype=int)
    el[nx // 3:2 * (nx // 3) + 1, ny // 4:ny // 4 + ny // 3] = 2
    fe.mesh(elmts=el, NX=nx, NY=ny)
    fe._max_load_steps = 8
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=40)
    assert np.max(np.abs(fe._state('epl'))) > 0.
    return fe


def model_inputs(fe):
    """(generators, kappa per element, prescribed DOFs) for the reference"""
    D = fe._state('elstiff').reshape(-1, 6, 6)
    assert np.max(np.abs(D - D.transpose(0, 2, 1))) <= 1e-12 * np.max(np.abs(D))
    kap = np.zeros(len(fe.mat))
    if fe.planestress:   # eps_zz = kappa (exx + eyy) with the plane-stress elastic matrix of the element's material
        for i, mat in enumerate(fe.mat):
            CV = fe._element_CV(mat)
            kap[i] = -mat.nu * (CV[0, 0] + CV[0, 1]) / mat.E
    kappa = kap[fe._grid['mat_el']]
    M = R.generators(D, kappa)
    main = M[:, [0, 1, 3, 5]]                                   # the generators really vary, and the plastic ones couple to shear
    assert np.all(np.std(main, axis=0) > 0.05 * np.abs(np.mean(main, axis=0))) and np.max(np.abs(M[:, [2, 4]])) > 1e-3 * M[:, 0].max()
    presc = np.setdiff1d(np.arange(fe.Ndof), fe.free_dofs())
    return M, presc


def refresh(fe, presc, omega=0., nu=0):
    """bring operator, hierarchy and masks up to the tangents of the state (and to a new smoother)"""
    eng = fe._engine
    if omega or nu:
        eng.set_precond(1, omega, nu)
    eng.assemble()
    eng.apply_bc(presc, np.zeros(len(presc)), np.zeros(len(presc)))
    return eng.mg_info()


def reference(fe, M, presc, info, omega=0.65, nu=2, odd_mode=1):
    nx, ny = fe._NX, fe._NY
    coarse = 'exact' if info['coarse_solver'] != 'cheby' else ('cheby', info['cheby_steps'], info['cheby_kappa'])
    assembled = [l for l, L in enumerate(info['levels']) if l >= 1 and not L[4]]
    cyc = R.VCycle(nx, ny, M, fe.lenx / nx, fe.leny / ny, fe.thick, presc, omega=omega, nu=nu, odd_mode=odd_mode, coarse=coarse,
                   true_diag_levels=assembled)
    assert cyc.dims == [L[:4] for L in info['levels']]
    return cyc


def device_apply(eng, vec):
    return np.stack([eng.precond_apply(vec[:, q]) for q in range(vec.shape[1])], axis=1)


def compare(tag, fe, M, presc, info, bound, **kw):
    cyc = reference(fe, M, presc, info, **kw)
    vec = V.probe_vectors(fe._NX, fe._NY, presc, cyc.levels, cyc.levels[0].K)
    z = device_apply(fe._engine, vec)
    zr = cyc.apply(vec)
    per = np.max(np.abs(z - zr), axis=0) / np.max(np.abs(zr), axis=0)
    print('VCYCLE %-44s vectors=%d worst=%.3e %s' % (tag, vec.shape[1], per.max(), info['tail_kernel']))
    assert np.all(np.isfinite(z))
    worst = float(per.max())
    assert worst < bound, (tag, 'vector %d' % int(per.argmax()))
    return cyc, vec, z


def check_fine_operator(fe, cyc):
    """anchor of the reference on the device: its fine matrix is the assembled one, and element matrices agree"""
    K = fe._engine.get_csr()
    Kr = cyc.levels[0].K
    assert abs(K - Kr).max() < 1e-12 * abs(Kr).max()
    ny = fe._NY
    for e in (0, fe.Nel // 2 + ny // 3, fe.Nel - 1):
        ke = R.element_stiffness(cyc.levels[0].M[e], fe.lenx / fe._NX, fe.leny / ny, fe.thick)[0]
        assert np.max(np.abs(fe._engine.get_kel(e) - ke)) < 1e-12 * np.max(np.abs(ke))


# ------------------------------------------------------------------------------------------------ plain hierarchies, all in the tail
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('nx, ny', [(16, 12), (8, 8)])
def test_plain_tail_matrix_free_and_every_smoother(nx, ny, state):
    """default settings: k_mg_tail_mf<false>, dense coarsest level; nu = 1 and 3: k_mg_tail with the generic sweep loop and the
    copy-back of an odd nu; a second omega"""
    with environ(PLFX_MG_ODD=1):
        fe = solved_model(nx, ny, state)
        M, presc = model_inputs(fe)
        info = refresh(fe, presc)
        assert info['tail_kernel'] == 'tail_mf' and info['tail_level'] == 1 and info['coarse_solver'] == 'dense'
        assert len(info['levels']) == 3 and not info['march'] and [L[4] for L in info['levels']] == [True, True, False]
        cyc, _, _ = compare('%dx%d %s default' % (nx, ny, state), fe, M, presc, info, V.LINEAR_BOUND)
        for omega, nu in ((0.65, 1), (0.65, 3), (0.5, 2), (0.8, 3)):
            info = refresh(fe, presc, omega, nu)
            want = 'tail_mf' if nu == 2 else 'tail'
            assert info['tail_kernel'] == want and info['coarse_solver'] == 'dense'
            compare('%dx%d %s omega=%g nu=%d' % (nx, ny, state, omega, nu), fe, M, presc, info, V.LINEAR_BOUND, omega=omega, nu=nu)
        check_fine_operator(fe, cyc)
        fe._drop_engine()


@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('nx, ny', [(16, 12), (8, 8)])
def test_plain_tail_assembled(nx, ny, state):
    """PLFX_MATFREE=0: block-ELL levels, k_mg_tail_lds"""
    with environ(PLFX_MATFREE=0):
        fe = solved_model(nx, ny, state)
        M, presc = model_inputs(fe)
        info = refresh(fe, presc)
        assert info['tail_kernel'] == 'tail_lds' and info['coarse_solver'] == 'dense' and not any(L[4] for L in info['levels'])
        cyc, _, _ = compare('%dx%d %s assembled' % (nx, ny, state), fe, M, presc, info, V.LINEAR_BOUND)
        check_fine_operator(fe, cyc)
        fe._drop_engine()


@pytest.mark.parametrize('state', STATES)
def test_whole_cycle_matrix_16x12(state):
    """all 442 columns of the device's B against the reference matrix; B is symmetric, positive definite on the free DOFs (what
    PCG needs) and zero on prescribed rows and columns"""
    fe = solved_model(16, 12, state)
    M, presc = model_inputs(fe)
    info = refresh(fe, presc)
    assert info['tail_kernel'] == 'tail_mf'
    cyc = reference(fe, M, presc, info)
    B = device_apply(fe._engine, np.eye(fe.Ndof))
    Br = cyc.matrix()
    free = cyc.levels[0].free
    colmax = np.max(np.abs(Br), axis=0)
    worst = np.max(np.max(np.abs(B - Br), axis=0)[free] / colmax[free])
    print('VCYCLE %-44s columns=%d worst=%.3e' % ('16x12 %s whole matrix' % state, fe.Ndof, worst))
    assert worst < V.LINEAR_BOUND
    assert not B[~free].any() and not B[:, ~free].any()
    assert np.max(np.abs(B - B.T)) < 1e-13 * np.max(np.abs(B))
    Bf = B[free][:, free]
    assert np.linalg.eigvalsh(0.5 * (Bf + Bf.T)).min() > 0.
    fe._drop_engine()


# ------------------------------------------------------------------------------------------------ ragged hierarchies
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('nx, ny', [(35, 33), (36, 33)])
@pytest.mark.parametrize('matfree', [1, 0])
def test_ragged_levels_in_the_tail(nx, ny, state, matfree):
    """1224 / 1258 nodes: the odd finest level is coarsened with triple children, then pairs with the weight 1 / (1 + r);
    matrix-free: k_mg_tail_mf<true> and the area-scaled smoothing diagonal; PLFX_MATFREE=0: four cell classes per level in
    k_mg_tail_lds, whose assembled levels smooth with the true diagonal"""
    with environ(PLFX_MATFREE=matfree, PLFX_MG_ODD=1):
        fe = solved_model(nx, ny, state)
        M, presc = model_inputs(fe)
        info = refresh(fe, presc)
        assert info['tail_kernel'] == ('tail_mf_ragged' if matfree else 'tail_lds') and info['tail_level'] == 1
        assert info['coarse_solver'] == 'dense' and len(info['levels']) == 5 and info['levels'][1][:2] == (nx // 2, 16)
        assert info['levels'][1][3] == 1.5 and info['levels'][2][:4] == ((8, 8, 1.75, 1.25) if nx == 35 else (9, 8, 1., 1.25))
        assert [L[4] for L in info['levels']] == ([True] * 4 + [False] if matfree else [False] * 5)
        cyc, _, _ = compare('%dx%d %s matfree=%d' % (nx, ny, state, matfree), fe, M, presc, info, V.LINEAR_BOUND)
        check_fine_operator(fe, cyc)
        fe._drop_engine()


@pytest.mark.parametrize('state', STATES)
def test_ragged_level_above_the_tail_with_and_without_graph(state):
    """70 x 66: level 1 is 35 x 33 and runs kernel by kernel (generators from the fused set-up pass, ragged transfers to level
    2); the replayed graph gives the bits of the launches"""
    out = {}
    for graph in (0, 1):
        with environ(PLFX_MG_GRAPH=graph, PLFX_MG_ODD=1):
            fe = solved_model(70, 66, state)
            M, presc = model_inputs(fe)
            info = refresh(fe, presc)
            assert info['tail_kernel'] == 'tail_mf_ragged' and info['tail_level'] == 2 and len(info['levels']) == 6
            assert info['levels'][1][:4] == (35, 33, 1., 1.) and info['levels'][2][:4] == (17, 16, 1.5, 1.5)
            assert [L[4] for L in info['levels']] == [True] * 5 + [False]
            cyc, vec, z = compare('70x66 %s graph=%d' % (state, graph), fe, M, presc, info, V.LINEAR_BOUND)
            out[graph] = (M, vec, z)
            if graph:
                check_fine_operator(fe, cyc)
            fe._drop_engine()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize('cheby', [None, (20, 100.)])
def test_chebyshev_coarsest_level(cheby):
    """70 x 66 with PLFX_MG_ODD=0: the hierarchy stops at 35 x 33, too large for the tail and for a dense inverse: 35 Chebyshev
    steps with kappa = 612.5 (or what PLFX_MG_CHEBY / PLFX_MG_CHEBY_KAPPA say)"""
    kw = {} if cheby is None else dict(PLFX_MG_CHEBY=cheby[0], PLFX_MG_CHEBY_KAPPA=cheby[1])
    with environ(PLFX_MG_ODD=0, **kw):
        fe = solved_model(70, 66, 'strain')
        M, presc = model_inputs(fe)
        info = refresh(fe, presc)
        assert info['tail_kernel'] == 'none' and info['tail_level'] == -1 and info['coarse_solver'] == 'cheby'
        assert (info['cheby_steps'], info['cheby_kappa']) == ((35, 612.5) if cheby is None else cheby)
        assert [L[:2] for L in info['levels']] == [(70, 66), (35, 33)] and all(L[4] for L in info['levels'])
        compare('70x66 strain ODD=0 cheby=%s' % (cheby,), fe, M, presc, info, V.LINEAR_BOUND, odd_mode=0)
        fe._drop_engine()


@pytest.mark.parametrize('state', STATES)
def test_pcg_coarsest_level_in_the_generic_tail(state):
    """40 x 36 with PLFX_MG_ODD=0: 20 x 18 -> 10 x 9, 220 DOFs > 128: no dense inverse, k_mg_tail solves the coarsest level by
    Jacobi-PCG in LDS to 1e-10 -- not exactly linear, so the exact-solve reference is met to a bound of its own"""
    with environ(PLFX_MG_ODD=0):
        fe = solved_model(40, 36, state)
        M, presc = model_inputs(fe)
        info = refresh(fe, presc)
        assert info['tail_kernel'] == 'tail' and info['tail_level'] == 1 and info['coarse_solver'] == 'pcg'
        assert [L[:2] for L in info['levels']] == [(40, 36), (20, 18), (10, 9)]
        compare('40x36 %s ODD=0 pcg' % state, fe, M, presc, info, V.PCG_BOUND, odd_mode=0)
        fe._drop_engine()


# ------------------------------------------------------------------------------------------------ marching fine-level kernels
MARCH_MESHES = ((70, 66), (35, 33))


def march_child(path_in, path_out):
    """run in a process of its own (PLFX_MARCH is read once per process): V-cycles and operator products of both meshes on the
    tangents the parent hands over.  (Whole solves are not equal bit for bit between the two forms: the marching PCG operator
    kernel sums its p.q partials over other nodes per block.)"""
    from pylabfea_amd import _lib
    inp = np.load(path_in)
    out = {}
    for nx, ny in MARCH_MESHES:
        k = '%dx%d_' % (nx, ny)
        fe = solved_model(nx, ny, 'strain')
        fe._engine.state_set(_lib.ST_ELSTIFF, inp[k + 'D'])
        info = refresh(fe, inp[k + 'presc'])
        vec = inp[k + 'vec']
        out[k + 'march'] = np.array(info['march'])
        out[k + 'levels'] = np.array([L[:4] for L in info['levels']])
        out[k + 'z'] = device_apply(fe._engine, vec)
        out[k + 'q'] = np.stack([fe._engine.matvec(vec[:, q]) for q in range(vec.shape[1])], axis=1)
        fe._drop_engine()
    np.savez(path_out, **out)


def test_marching_form_gives_the_bits_of_the_gather_form(tmp_path):
    """PLFX_MARCH=1 and =0 in fresh processes on the same tangents: V-cycles and operator products are equal bit for bit, and
    the gather form meets the reference"""
    inp, ref = {}, {}
    for nx, ny in MARCH_MESHES:
        k = '%dx%d_' % (nx, ny)
        fe = solved_model(nx, ny, 'strain')
        M, presc = model_inputs(fe)
        info = refresh(fe, presc)
        cyc = reference(fe, M, presc, info)
        vec = V.probe_vectors(nx, ny, presc, cyc.levels, cyc.levels[0].K)
        inp[k + 'D'], inp[k + 'presc'], inp[k + 'vec'] = fe._state('elstiff'), presc, vec
        ref[k] = (cyc.apply(vec), cyc.levels[0].K @ vec, cyc.dims)
        fe._drop_engine()
    path_in = str(tmp_path / 'tangents.npz')
    np.savez(path_in, **inp)
    got = {}
    for march in (0, 1):
        path = str(tmp_path / ('march%d.npz' % march))
        env = dict(os.environ, PLFX_MARCH=str(march), PLFX_MG_ODD='1')
        subprocess.run([sys.executable, os.path.abspath(__file__), path_in, path], env=env, check=True, timeout=300)
        got[march] = np.load(path)
    for k, (zref, qref, dims) in ref.items():
        assert bool(got[1][k + 'march']) and not bool(got[0][k + 'march'])
        assert [tuple(r) for r in got[0][k + 'levels']] == [tuple(map(float, d)) for d in dims]
        for name in ('z', 'q', 'levels'):
            assert np.array_equal(got[0][k + name], got[1][k + name]), (k, name)
        d, dq = V.rel_diff(got[0][k + 'z'], zref), V.rel_diff(got[0][k + 'q'], qref)
        print('VCYCLE %-44s worst=%.3e (matvec %.3e)' % (k + ' strain PLFX_MARCH=0/1 child processes', d, dq))
        assert d < V.LINEAR_BOUND and dq < 1e-12    # (18 terms per row x 2.2e-16 x |K||x| / max|K x| of at most a few hundred)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    march_child(sys.argv[1], sys.argv[2])

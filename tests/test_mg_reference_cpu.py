"""The NumPy reference of the multigrid V-cycle (tests/mg_reference.py) checked against what the cycle is defined to be, and
shown to tell a right cycle from the wrong ones that a solve would never notice.  No GPU.

Measured effect max|z_wrong - z| / max|z| of every wrong reference on the test vectors of tests/test_gpu_vcycle.py (worst
vector; synthetic plastic tangents with a soft inclusion; required: >= 1e4 x the bound of the GPU comparison = 5.7e-9, and
1.2e-5 where the coarsest level is solved by the in-LDS PCG; with the bounds at their caps it would be 1e-4 and 1e-2):

    mesh, plane state          pair 1/2   triple swapped  plain mean  true diagonal  mask shifted  omega + 10 %
    35 x 33 strain             8.1e-2     1.5e-1          1.8e-2      3.2e-2         1.2           2.6e-2
    35 x 33 stress             8.0e-2     1.4e-1          1.9e-2      2.8e-2         1.1           2.3e-2
    36 x 33 strain             6.7e-2     7.1e-2          1.3e-2      1.8e-2         1.2           3.0e-2
    36 x 33 stress             6.5e-2     6.9e-2          1.3e-2      1.6e-2         1.1           2.6e-2
    70 x 66 strain             7.2e-2     1.1e-1          2.6e-2      5.3e-2         1.1           2.9e-2
    40 x 36 strain, ODD=0      0          0               0           0              0             2.5e-2
                               (no level of another cell size there: only omega applies)

The same two errors made in the device code (scratch builds: 0.5 for 1 / (1 + r) in mg_tr1d_last; w = 1 in k_mg_coarsen_M)
move the device's 35 x 33 output by 8.3e-2 and 8.2e-3 from the reference, as predicted here.
"""
import numpy as np
import pytest

import mg_reference as R
import vcycle_cases as V

KAPPA = {'strain': 0., 'stress': -0.3 / 0.7}     # plane stress of an isotropic body: eps_zz = -nu / (1 - nu) (exx + eyy)
LX, LY, THICK = 4. / 35, 4. / 33 * 0.9, 1.3


def make(nx, ny, state='strain', homogeneous=False, presc=None, **kw):
    D = V.synthetic_tangents(nx, ny)
    if homogeneous:
        D = np.broadcast_to(D[0], D.shape)
    M = R.generators(D, KAPPA[state])
    presc = V.fixed_dofs(nx, ny) if presc is None else presc
    return R.VCycle(nx, ny, M, LX, LY, THICK, presc, **kw)


def test_element_stiffness_is_the_integral_of_BtDB():
    """generators + closed-form shape integrals against 2 x 2 Gauss quadrature of B^T D B with the full 6 x 6 tangent"""
    D = V.synthetic_tangents(6, 5)
    lx, ly, t = 0.37, 0.21, 1.3
    for kappa in KAPPA.values():
        K = R.element_stiffness(R.generators(D, kappa), lx, ly, t)
        Kq = np.zeros_like(K)
        px, py = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])
        for gx in (-1, 1):
            for gy in (-1, 1):
                xi, eta = 0.5 + 0.5 * gx / np.sqrt(3.), 0.5 + 0.5 * gy / np.sqrt(3.)
                Nx = (2 * px - 1) * np.where(py, eta, 1 - eta) / lx
                Ny = (2 * py - 1) * np.where(px, xi, 1 - xi) / ly
                B = np.zeros((6, 8))
                B[0, 0::2] = Nx
                B[1, 1::2] = Ny
                B[2, 0::2], B[2, 1::2] = kappa * Nx, kappa * Ny
                B[5, 0::2], B[5, 1::2] = Ny, Nx
                Kq += 0.25 * lx * ly * t * np.einsum('ia,eij,jb->eab', B, D, B)
        assert np.max(np.abs(K - Kq)) < 1e-13 * np.max(np.abs(Kq))
        assert np.max(np.abs(K - K.transpose(0, 2, 1))) < 1e-13 * np.max(np.abs(K))


@pytest.mark.parametrize('nx, ny, odd, want', [
    (8, 8, 1, [(8, 8, 1., 1.), (4, 4, 1., 1.), (2, 2, 1., 1.)]),
    (16, 12, 1, [(16, 12, 1., 1.), (8, 6, 1., 1.), (4, 3, 1., 1.)]),
    (35, 33, 1, [(35, 33, 1., 1.), (17, 16, 1.5, 1.5), (8, 8, 1.75, 1.25), (4, 4, 1.375, 1.125), (2, 2, 1.1875, 1.0625)]),
    (36, 33, 1, [(36, 33, 1., 1.), (18, 16, 1., 1.5), (9, 8, 1., 1.25), (4, 4, 1.5, 1.125), (2, 2, 1.25, 1.0625)]),
    (70, 66, 1, [(70, 66, 1., 1.), (35, 33, 1., 1.), (17, 16, 1.5, 1.5), (8, 8, 1.75, 1.25), (4, 4, 1.375, 1.125),
                 (2, 2, 1.1875, 1.0625)]),
    (70, 66, 0, [(70, 66, 1., 1.), (35, 33, 1., 1.)]),
    (40, 36, 0, [(40, 36, 1., 1.), (20, 18, 1., 1.), (10, 9, 1., 1.)]),
    (33, 31, 1, [(33, 31, 1., 1.)]),          # 1088 nodes: an odd level is coarsened only above 1089 nodes (or with a ratio != 1)
    (33, 32, 1, [(33, 32, 1., 1.), (16, 16, 1.5, 1.), (8, 8, 1.25, 1.), (4, 4, 1.125, 1.), (2, 2, 1.0625, 1.)]),   # 1122
])
def test_hierarchy_rule(nx, ny, odd, want):
    got = [(len(xs) - 1, len(ys) - 1, R.ratio(xs), R.ratio(ys)) for xs, ys in R.hierarchy_dims(nx, ny, odd)]
    assert got == want
    for (xs, ys) in R.hierarchy_dims(nx, ny, odd):
        assert xs[-1] == nx and ys[-1] == ny          # the last node line of every level is the edge of the grid
        assert 1. <= R.ratio(xs) < 2. and 1. <= R.ratio(ys) < 2.


@pytest.mark.parametrize('nx, ny', [(16, 12), (35, 33), (36, 33)])
def test_interpolation_reproduces_bilinear_fields(nx, ny):
    cyc = make(nx, ny)
    f = lambda x, y: 0.3 + 1.7 * x - 0.6 * y + 0.05 * x * y
    for L, C in zip(cyc.levels[:-1], cyc.levels[1:]):
        fc = np.repeat(f(C.xs[:, None], C.ys[None, :]).ravel(), 2)
        ff = np.repeat(f(L.xs[:, None], L.ys[None, :]).ravel(), 2)
        assert np.max(np.abs(L.P @ fc - ff)) < 1e-13 * np.max(np.abs(ff))
        assert np.max(np.abs(np.asarray(L.P.sum(axis=1)).ravel() - 1.)) < 1e-15


@pytest.mark.parametrize('nx, ny', [(16, 12), (35, 33), (36, 33)])
@pytest.mark.parametrize('state', ['strain', 'stress'])
def test_coarse_operator_of_a_homogeneous_body_is_the_galerkin_one(nx, ny, state):
    """the claim of DESIGN 10.7: re-assembly from the (equal) generators gives P^T K P on plain and on ragged level pairs"""
    cyc = make(nx, ny, state, homogeneous=True, presc=[])
    for L, C in zip(cyc.levels[:-1], cyc.levels[1:]):
        G = (L.P.T @ L.K @ L.P).toarray()
        assert np.max(np.abs(G - C.K.toarray())) < 1e-12 * np.max(np.abs(G)), (L.nx, L.ny)


def test_coarse_operator_of_a_heterogeneous_body_is_not_the_galerkin_one():
    cyc = make(16, 12, presc=[])
    L, C = cyc.levels[0], cyc.levels[1]
    G = (L.P.T @ L.K @ L.P).toarray()
    assert np.max(np.abs(G - C.K.toarray())) > 1e-3 * np.max(np.abs(G))


@pytest.mark.parametrize('nx, ny, kw', [(16, 12, {}), (16, 12, dict(nu=3, omega=0.5)), (35, 33, {}),
                                        (35, 33, dict(odd_mode=0, coarse=('cheby', 20, 80.)))])
def test_cycle_matrix_is_symmetric_positive_definite_and_masked(nx, ny, kw):
    cyc = make(nx, ny, 'stress', **kw)
    B = cyc.matrix()
    free = cyc.levels[0].free
    assert np.max(np.abs(B - B.T)) < 1e-13 * np.max(np.abs(B))
    assert not B[~free].any() and not B[:, ~free].any()
    Bf = B[free][:, free]
    np.linalg.cholesky(0.5 * (Bf + Bf.T))                 # raises unless positive definite


def test_two_level_cycle_without_smoothing_is_the_coarse_grid_correction():
    cyc = make(8, 6)
    assert len(cyc.levels) == 2
    L, C = cyc.levels
    rng = np.random.default_rng(0)
    r = L.free * rng.standard_normal(len(L.free))
    f = np.nonzero(C.free)[0]
    xc = np.zeros(len(C.free))
    xc[f] = np.linalg.solve(C.K.toarray()[np.ix_(f, f)], (L.P.T @ r)[f])
    want = L.free * (L.P @ xc)
    assert np.max(np.abs(cyc.apply(r, skip_smoothing=True) - want)) < 1e-13 * np.max(np.abs(want))


def test_area_scaled_diagonal_is_not_below_the_true_one_and_equal_on_plain_levels():
    cyc = make(35, 33)
    for l, L in enumerate(cyc.levels):
        true = L.K.diagonal()
        if L.ragged and l >= 1:
            assert np.all(L.diag >= true * (1 - 1e-14)) and np.max(L.diag / true) > 1.2
        else:
            assert np.array_equal(L.diag, true)


def effects(nx, ny, state, **kw):
    right = make(nx, ny, state, **kw)
    L0 = right.levels[0]
    vec = V.probe_vectors(nx, ny, np.nonzero(~L0.free)[0], right.levels, L0.K)
    z = right.apply(vec)
    out = {}
    for m in R.MUTATIONS:
        wrong = make(nx, ny, state, mutate=(m,), **kw)
        out[m] = V.rel_diff(wrong.apply(vec), z)
    return out


@pytest.mark.parametrize('nx, ny, state', [(35, 33, 'strain'), (35, 33, 'stress'), (36, 33, 'strain'), (36, 33, 'stress'),
                                           (70, 66, 'strain')])
def test_wrong_references_are_told_apart_on_ragged_hierarchies(nx, ny, state):
    """see the table in the module docstring"""
    eff = effects(nx, ny, state)
    print(nx, ny, state, ' '.join('%s=%.2e' % kv for kv in eff.items()))
    for m, e in eff.items():
        assert e >= V.SENSITIVITY * V.LINEAR_BOUND, (m, e)


def test_wrong_omega_is_told_apart_where_the_coarsest_level_is_solved_by_pcg():
    """40 x 36 with PLFX_MG_ODD=0 has no level of another cell size, so of the wrong references only omega differs at all"""
    eff = effects(40, 36, 'strain', odd_mode=0)
    print(40, 36, ' '.join('%s=%.2e' % kv for kv in eff.items()))
    assert all(e == 0. for m, e in eff.items() if m != 'omega_10pc')
    assert eff['omega_10pc'] >= V.SENSITIVITY * V.PCG_BOUND

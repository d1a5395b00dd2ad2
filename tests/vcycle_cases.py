"""What tests/test_mg_reference_cpu.py and tests/test_gpu_vcycle.py share: the bounds, the test vectors, the measure, and the
synthetic plastic tangents the CPU tests use where the GPU tests take the tangents of a solved model."""
import numpy as np

# max|z_dev - z_ref| / max|z_ref| per test vector: 100 x the worst value measured on an MI355X over all linear
# cases (5.7e-15, 70 x 66 plane strain with PLFX_MG_ODD=0, 35 Chebyshev steps on the coarsest level) and over the case whose
# coarsest level is solved by the in-LDS PCG to 1e-10 (1.2e-11, 40 x 36 plane stress).  Neither may exceed its cap.
LINEAR_BOUND = 5.7e-13
PCG_BOUND = 1.2e-9
assert LINEAR_BOUND <= 1e-8 and PCG_BOUND <= 1e-6
SENSITIVITY = 1e4     # a wrong reference differs from the right one by at least this many bounds


def rel_diff(z, zref):
    """worst max|dz| / max|zref| over the columns"""
    z, zref = z.reshape(len(z), -1), zref.reshape(len(zref), -1)
    return float(np.max(np.max(np.abs(z - zref), axis=0) / np.max(np.abs(zref), axis=0)))


def fixed_dofs(nx, ny):
    """left edge: u_x, bottom edge: u_y, top edge: u_y (displaced); the right edge carries a force"""
    node = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    return np.unique(np.concatenate([2 * node[0, :], 2 * node[:, 0] + 1, 2 * node[:, ny] + 1]))


def probe_vectors(nx, ny, presc, levels, K, seed=7):
    """columns: three seeded random vectors; a unit vector (x and y) on the fine node line next to every line where a coarse
    level's cell of another size begins, and next to every edge; the residual of the field u_x = X / L, u_y = 0, which is
    uniform along y.  All of them zero on the prescribed DOFs.  levels: those of the reference (node lines xs, ys in fine-grid
    units, ratios rx, ry); K: the fine matrix."""
    ndof = 2 * (nx + 1) * (ny + 1)
    free = np.ones(ndof)
    free[presc] = 0.
    rng = np.random.default_rng(seed)
    cols = [free * rng.standard_normal(ndof) for _ in range(3)]

    def unit(j, k):
        for comp in (0, 1):
            v = np.zeros(ndof)
            v[2 * (j * (ny + 1) + k) + comp] = 1.
            if free @ v:
                cols.append(v)

    jm, km = nx // 2 - 1, ny // 2 + 1
    for L in levels[1:]:
        if L.rx != 1.:
            unit(min(int(L.xs[-2]) + 1, nx - 1), km)
        if L.ry != 1.:
            unit(jm, min(int(L.ys[-2]) + 1, ny - 1))
    unit(1, km)            # next to the left edge
    unit(nx - 1, km)       # right
    unit(jm, 1)            # bottom
    unit(jm, ny - 1)       # top
    g = np.zeros((nx + 1, ny + 1, 2))
    g[:, :, 0] = np.arange(nx + 1)[:, None] / nx
    cols.append(free * (K @ (free * g.ravel())))
    return np.stack(cols, axis=1)


def synthetic_tangents(nx, ny, seed=11):
    """D[nel, 6, 6]: the elastic matrix of E = 200 GPa, nu = 0.3 with a soft (E / 5) inclusion in the middle, minus a rank-one
    plastic part w a a^T whose direction and weight vary from element to element (the form of a one-step return), plastic in
    a band across the body"""
    E, nu = 200.e3, 0.3
    lam, mu = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))
    CV = np.zeros((6, 6))
    CV[:3, :3] = lam
    CV[[0, 1, 2], [0, 1, 2]] = lam + 2 * mu
    CV[[3, 4, 5], [3, 4, 5]] = mu
    rng = np.random.default_rng(seed)
    ej, ek = np.divmod(np.arange(nx * ny), ny)
    x, y = (ej + 0.5) / nx, (ek + 0.5) / ny
    soft = (np.abs(x - 0.55) < 0.2) & (np.abs(y - 0.45) < 0.2)
    D = np.where(soft[:, None, None], 0.2, 1.) * CV
    plastic = np.abs(x + 0.6 * y - 0.9) < 0.35
    a = np.zeros((nx * ny, 6))
    a[:, [0, 1, 2, 5]] = rng.standard_normal((nx * ny, 4)) + np.array([1., -0.5, -0.5, 0.8])
    a /= np.linalg.norm(a, axis=1)[:, None]
    Da = np.einsum('eij,ej->ei', D, a)
    w = plastic * rng.uniform(0.3, 0.9, nx * ny) / np.einsum('ei,ei->e', a, Da)
    return D - w[:, None, None] * Da[:, :, None] * Da[:, None, :]

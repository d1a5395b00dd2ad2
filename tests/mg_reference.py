"""The multigrid V-cycle of the structured Q4 grid, rebuilt in NumPy / SciPy from its definition: no GPU,
no library.  `VCycle(...)` holds the hierarchy; `apply(r)` is one cycle, `matrix()` the cycle as a dense matrix B.

Geometry first, everything else from it.  A level is two lists of node coordinates.  Coarsening a direction keeps every second
node line and always the last one (the edge of the grid); with an odd number of cells the line before the last goes too, so the
last coarse cell has three children.  The transfer weights are linear interpolation between those coordinates, the ratio r of a
level is the width of its last cell over that of the others, the children of a coarse cell are the fine cells it covers and
their weights in the mean of the generators are their areas.

Numbering (Model.mesh): node (j, k) has id j * (ny + 1) + k, its DOFs are 2 id (x) and 2 id + 1 (y); element (j, k) has id
j * ny + k and the nodes (j, k), (j, k + 1), (j + 1, k), (j + 1, k + 1) in this order.
"""
import numpy as np
import scipy.sparse as sp

TAIL_NODES = 1089        # a non-plain level with more nodes than this, or with a ratio != 1, is coarsened raggedly
CHEBY_BMAX = 3.0

# deliberately wrong references (tests/test_mg_reference_cpu.py shows that the test vectors tell each from the right one)
MUTATIONS = ('pair_weight_half', 'triple_swapped', 'plain_mean', 'true_diag', 'mask_shift', 'omega_10pc')


# ------------------------------------------------------------------------------------------------ element level
def generators(D, kappa):
    """The six generators XX XY XS YY YS SS of elements with tangents D[nel, 6, 6] (Voigt order xx yy zz yz zx xy): the
    in-plane strain state is eps = X exx + Y eyy + S gxy with X = e0 + kappa e2, Y = e1 + kappa e2, S = e5 (plane strain:
    kappa = 0; plane stress: eps_zz = kappa (exx + eyy)), and M = [X Y S]^T D [X Y S]."""
    D = np.asarray(D, dtype=float).reshape(-1, 6, 6)
    kappa = np.broadcast_to(np.asarray(kappa, dtype=float), (len(D),))
    G = np.zeros((len(D), 6, 3))
    G[:, 0, 0] = 1.
    G[:, 2, 0] = kappa
    G[:, 1, 1] = 1.
    G[:, 2, 1] = kappa
    G[:, 5, 2] = 1.
    M = np.einsum('eia,eij,ejb->eab', G, D, G)
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], axis=1)


def shape_integrals(lx, ly, thick=1.):
    """Sxx[a, b] = t int N_a,x N_b,x dA, Syy likewise, Sxy[a, b] = t int N_a,x N_b,y dA of the bilinear shape functions of a
    rectangle lx x ly (closed form; local nodes (0,0) (0,1) (1,0) (1,1))."""
    px = np.array([0, 0, 1, 1])
    py = np.array([0, 1, 0, 1])
    sx, sy = 2. * px - 1., 2. * py - 1.
    same_y = np.where(py[:, None] == py[None, :], 1. / 3., 1. / 6.)    # int_0^1 of the two linear factors along y
    same_x = np.where(px[:, None] == px[None, :], 1. / 3., 1. / 6.)
    Sxx = thick * (ly / lx) * np.outer(sx, sx) * same_y
    Syy = thick * (lx / ly) * np.outer(sy, sy) * same_x
    Sxy = thick * np.outer(sx, sy) / 4.
    return Sxx, Syy, Sxy


def element_stiffness(M, lx, ly, thick=1.):
    """K_e[nel, 8, 8] of rectangles lx x ly from the generators M[nel, 6]"""
    M = np.asarray(M, dtype=float).reshape(-1, 6)
    Sxx, Syy, Sxy = shape_integrals(lx, ly, thick)
    Syx = Sxy.T
    XX, XY, XS, YY, YS, SS = (M[:, c, None, None] for c in range(6))
    K = np.zeros((len(M), 8, 8))
    K[:, 0::2, 0::2] = XX * Sxx + XS * (Sxy + Syx) + SS * Syy
    K[:, 0::2, 1::2] = XY * Sxy + XS * Sxx + YS * Syy + SS * Syx
    K[:, 1::2, 0::2] = XY * Syx + XS * Sxx + YS * Syy + SS * Sxy
    K[:, 1::2, 1::2] = YY * Syy + YS * (Sxy + Syx) + SS * Sxx
    return K


def element_dofs(nx, ny):
    j, k = np.divmod(np.arange(nx * ny), ny)
    n0 = j * (ny + 1) + k
    nodes = np.stack([n0, n0 + 1, n0 + ny + 1, n0 + ny + 2], axis=1)
    return np.stack([2 * nodes, 2 * nodes + 1], axis=2).reshape(-1, 8)


# ------------------------------------------------------------------------------------------------ geometry of the hierarchy
def ratio(xs):
    return 1. if len(xs) < 3 else (xs[-1] - xs[-2]) / (xs[1] - xs[0])


def coarse_lines(n):
    """indices of the node lines of a direction with n cells that the next level keeps"""
    keep = list(range(0, n - 1, 2)) if n % 2 == 0 else list(range(0, n - 2, 2))
    return np.array(keep + [n])


def interpolation_1d(xf, xc, mutate=()):
    """P[j, J]: linear interpolation from the coarse node lines xc to the fine ones xf"""
    P = np.zeros((len(xf), len(xc)))
    for j, x in enumerate(xf):
        J = min(np.searchsorted(xc, x, side='right') - 1, len(xc) - 2)
        w1 = (x - xc[J]) / (xc[J + 1] - xc[J])
        P[j, J], P[j, J + 1] = 1. - w1, w1
    n = len(xf) - 1
    ragged = ratio(xf) != 1.
    if 'pair_weight_half' in mutate and n % 2 == 0 and ragged:
        P[n - 1, -2:] = 0.5
    if 'triple_swapped' in mutate and n % 2 == 1:
        P[[n - 2, n - 1], -2:] = P[[n - 1, n - 2], -2:]
    P[np.abs(P) < 1e-15] = 0.
    return P


def hierarchy_dims(nx, ny, odd_mode=1):
    """[(nx, ny, rx, ry), ...] of the levels, with their node coordinates"""
    xs, ys = np.arange(nx + 1, dtype=float), np.arange(ny + 1, dtype=float)
    out = [(xs, ys)]
    while True:
        xs, ys = out[-1]
        fx, fy, rx, ry = len(xs) - 1, len(ys) - 1, ratio(xs), ratio(ys)
        if fx * fy <= 4:
            break
        plain = fx % 2 == 0 and fy % 2 == 0 and rx == 1. and ry == 1.
        if not plain and not (odd_mode == 1 and ((fx + 1) * (fy + 1) > TAIL_NODES or rx != 1. or ry != 1.) and fx >= 2 and fy >= 2):
            break
        out.append((xs[coarse_lines(fx)], ys[coarse_lines(fy)]))
    return out


# ------------------------------------------------------------------------------------------------ the cycle
class Level:
    pass


class VCycle:
    """M0[nel, 6]: generators of the finest level; lx, ly, thick: its element size; presc: prescribed DOFs of the finest level;
    omega, nu: damped Jacobi, nu sweeps before and after; odd_mode: PLFX_MG_ODD; coarse: 'exact' or ('cheby', steps, kappa) or
    'cheby' (default steps and kappa); true_diag_levels: ragged levels >= 1 that smooth with the true diagonal (the assembled
    ones) instead of the area-scaled one; mutate: names from MUTATIONS."""

    def __init__(self, nx, ny, M0, lx, ly, thick, presc, omega=0.65, nu=2, odd_mode=1, coarse='exact', true_diag_levels=(),
                 mutate=()):
        for m in mutate:
            assert m in MUTATIONS, m
        self.mutate = tuple(mutate)
        self.omega = omega * (1.1 if 'omega_10pc' in mutate else 1.)
        self.nu = nu
        self.lx, self.ly, self.thick = lx, ly, thick
        lines = hierarchy_dims(nx, ny, odd_mode)
        free = np.ones(2 * (nx + 1) * (ny + 1), dtype=bool)
        free[np.asarray(presc, dtype=int)] = False
        self.levels = []
        M = np.asarray(M0, dtype=float).reshape(nx * ny, 6)
        for l, (xs, ys) in enumerate(lines):
            L = Level()
            L.xs, L.ys = xs, ys
            L.nx, L.ny, L.rx, L.ry = len(xs) - 1, len(ys) - 1, ratio(xs), ratio(ys)
            L.ragged = L.rx != 1. or L.ry != 1.
            L.M = M
            L.free = free
            L.K = self._assemble(L)
            true_diag = L.K.diagonal()
            if L.ragged and l >= 1 and l not in true_diag_levels and 'true_diag' not in mutate:
                L.diag = self._area_diagonal(L)
            else:
                L.diag = true_diag
            L.dinv = np.where(free, 1. / np.abs(L.diag), 0.)
            self.levels.append(L)
            if l + 1 < len(lines):
                xc, yc = lines[l + 1]
                kx, ky = coarse_lines(L.nx), coarse_lines(L.ny)
                Px, Py = interpolation_1d(xs, xc, mutate), interpolation_1d(ys, yc, mutate)
                L.P = sp.kron(sp.kron(sp.csr_matrix(Px), sp.csr_matrix(Py)), sp.identity(2), format='csr')
                M = self._coarse_generators(L, xc, yc)
                if 'mask_shift' in mutate and L.ragged:   # the last coarse line takes its mask one fine line early
                    kx, ky = kx.copy(), ky.copy()
                    kx[-1] -= 1
                    ky[-1] -= 1
                node = (kx[:, None] * (L.ny + 1) + ky[None, :]).ravel()
                free = np.stack([free[2 * node], free[2 * node + 1]], axis=1).ravel()
        Lc = self.levels[-1]
        if coarse == 'cheby':
            n = max(Lc.nx, Lc.ny)
            coarse = ('cheby', min(max(n, 16), 160), max(4., 0.5 * n * n))
        self.coarse = coarse

    @property
    def dims(self):
        return [(L.nx, L.ny, L.rx, L.ry) for L in self.levels]

    def _cell_sizes(self, L):
        return np.diff(L.xs) * self.lx, np.diff(L.ys) * self.ly

    def _assemble(self, L):
        wx, wy = self._cell_sizes(L)
        nel, ndof = L.nx * L.ny, 2 * (L.nx + 1) * (L.ny + 1)
        Ke = np.zeros((nel, 8, 8))
        ej, ek = np.divmod(np.arange(nel), L.ny)
        for a in np.unique(wx):
            for b in np.unique(wy):
                sel = (wx[ej] == a) & (wy[ek] == b)
                Ke[sel] = element_stiffness(L.M[sel], a, b, self.thick)
        dofs = element_dofs(L.nx, L.ny)
        rows = np.repeat(dofs, 8, axis=1).ravel()
        cols = np.tile(dofs, (1, 8)).ravel()
        return sp.csr_matrix((Ke.ravel(), (rows, cols)), shape=(ndof, ndof))

    def _area_diagonal(self, L):
        """every cell enters with the Sxx and Syy integrals of the level's regular cell times its relative area; Sxy has no size"""
        wx, wy = self._cell_sizes(L)
        Sxx, Syy, Sxy = shape_integrals(wx[0], wy[0], self.thick)
        ej, ek = np.divmod(np.arange(L.nx * L.ny), L.ny)
        area = (wx[ej] / wx[0]) * (wy[ek] / wy[0])
        XX, XY, XS, YY, YS, SS = L.M.T
        d = np.zeros((L.nx * L.ny, 8))
        for a in range(4):
            d[:, 2 * a] = XX * Sxx[a, a] * area + 2. * XS * Sxy[a, a] + SS * Syy[a, a] * area
            d[:, 2 * a + 1] = YY * Syy[a, a] * area + 2. * YS * Sxy[a, a] + SS * Sxx[a, a] * area
        out = np.zeros(2 * (L.nx + 1) * (L.ny + 1))
        np.add.at(out, element_dofs(L.nx, L.ny).ravel(), d.ravel())
        return out

    def _coarse_generators(self, L, xc, yc):
        """mean of the children (the fine cells a coarse cell covers), weighted with their areas"""
        wx, wy = np.diff(L.xs), np.diff(L.ys)
        if 'plain_mean' in self.mutate:
            wx, wy = np.ones_like(wx), np.ones_like(wy)
        cj = np.searchsorted(xc, 0.5 * (L.xs[1:] + L.xs[:-1])) - 1     # coarse column of every fine column
        ck = np.searchsorted(yc, 0.5 * (L.ys[1:] + L.ys[:-1])) - 1
        nyc = len(yc) - 1
        ej, ek = np.divmod(np.arange(L.nx * L.ny), L.ny)
        parent = cj[ej] * nyc + ck[ek]
        w = wx[ej] * wy[ek]
        num = np.zeros(((len(xc) - 1) * nyc, 6))
        den = np.zeros(len(num))
        np.add.at(num, parent, w[:, None] * L.M)
        np.add.at(den, parent, w)
        return num / den[:, None]

    # ---- one cycle; r may carry several columns
    def _smooth(self, L, b, x, sweeps):
        for _ in range(sweeps):
            x = x + self.omega * L.dinv[:, None] * (b - L.K @ x)
        return x

    def _coarsest(self, L, b):
        if self.coarse == 'exact':
            f = np.nonzero(L.free)[0]
            x = np.zeros_like(b)
            x[f] = np.linalg.solve(L.K[f][:, f].toarray(), b[f])
            return x
        _, m, kappa = self.coarse
        amin = CHEBY_BMAX / kappa
        theta, delta = 0.5 * (CHEBY_BMAX + amin), 0.5 * (CHEBY_BMAX - amin)
        sigma = theta / delta
        rho = 1. / sigma
        d = L.dinv[:, None] * b / theta
        x = d.copy()
        for _ in range(1, m):
            rho_new = 1. / (2. * sigma - rho)
            d = rho_new * rho * d + (2. * rho_new / delta) * L.dinv[:, None] * (b - L.K @ x)
            x = x + d
            rho = rho_new
        return x

    def _cycle(self, l, b, skip_smoothing=False):
        L = self.levels[l]
        if l == len(self.levels) - 1:
            return self._coarsest(L, b)
        nu = 0 if skip_smoothing else self.nu
        x = self._smooth(L, b, np.zeros_like(b), nu)
        res = L.free[:, None] * (b - L.K @ x)
        C = self.levels[l + 1]
        bc = C.free[:, None] * (L.P.T @ res)
        x = x + L.free[:, None] * (L.P @ self._cycle(l + 1, bc, skip_smoothing))
        return self._smooth(L, b, x, nu)

    def apply(self, r, skip_smoothing=False):
        r = np.asarray(r, dtype=float)
        z = self._cycle(0, r.reshape(len(r), -1), skip_smoothing)
        return z.reshape(r.shape)

    def matrix(self):
        return self.apply(np.eye(len(self.levels[0].free)))

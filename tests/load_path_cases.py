"""Helpers of the load-path tests (Material.load_path): the materials, the seeded strain paths, the yardstick of
check 1 -- K response_batch calls with epl += depl in NumPy between them --, the mixed-control cases, and the iteration of
load_path restated in NumPy around the CPU oracle's response (no GPU), which sets the bar of the r-value check.

Voigt order: xx, yy, zz, yz, xz, xy."""
import numpy as np

import flow_curve_cases as FC

K_PATH, N_PATH = 12, 65
NAMES = ('sig', 'epl', 'fy', 'nsteps')


def j2_material(FE, khard=0., sy=100.):
    m = FE.Material(name='J2')
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=sy, khard=khard, sdim=6)
    return m


def hill3_material(FE):
    m = FE.Material(name='Hill-3')
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=100., hill=[0.7, 1., 1.4], khard=500., sdim=3)
    return m


def elastic_material(FE):
    m = FE.Material(name='elastic')
    m.elasticity(E=200.e3, nu=0.3)
    return m


def strain_paths(sy, E, K=K_PATH, N=N_PATH, seed=0, zero=()):
    """dload (K, N, 6): seeded directions, steps of 0.2 sy / E per unit of a component, the sign of the path reversed for
    steps 8-11.  The directions have components in (-1, 1) times a size of 0.5, 1, 2 or 4 per path: small ones stay elastic
    for some steps, large ones yield at once, sub-divide, and yield again in the reversed part.  zero: components left out."""
    rng = np.random.default_rng(4000 + seed)
    d = rng.uniform(-1., 1., size=(N, 6)) * rng.choice([0.5, 1., 2., 4.], size=(N, 1))
    d[:, list(zero)] = 0.
    k = np.arange(K)
    sign = np.where((k >= 8) & (k < 12), -1., 1.)
    return np.ascontiguousarray(0.2 * sy / E * sign[:, None, None] * d[None, :, :])


def yardstick(m, CV, dload, maxit, tex_id=None, sig0=None, epl0=None):
    """the host loop: K calls of the point response on all N points, epl += depl in NumPy between them; dict of sig, epl,
    depl (K,N,6), fy, nsteps (K,N) and ct (N,6,6) after the last step"""
    K, N = dload.shape[:2]
    ctx = m._load(CV)
    sig = np.zeros((N, 6)) if sig0 is None else np.array(sig0, dtype=float)
    epl = np.zeros((N, 6)) if epl0 is None else np.array(epl0, dtype=float)
    out = dict(sig=np.empty((K, N, 6)), epl=np.empty((K, N, 6)), depl=np.empty((K, N, 6)), fy=np.empty((K, N)),
               nsteps=np.empty((K, N), dtype=np.int32))
    ct = None
    for k in range(K):
        fy, so, dp, ct, ns = ctx.response(sig, epl, np.ascontiguousarray(dload[k]), maxit=maxit, tex_id=tex_id)
        sig, epl = so, epl + dp
        out['sig'][k], out['epl'][k], out['depl'][k], out['fy'][k], out['nsteps'][k] = sig, epl, dp, fy, ns
    out['ct'] = np.array(ct).reshape(N, 6, 6)
    return out


def events(Y):
    """what occurs on a yardstick: dict of counts -- elastic and plastic steps, steps with nsteps = 0 and > 0, and paths that
    yield, then take an elastic step, then yield again"""
    plastic = np.any(Y['depl'] != 0., axis=2)                  # (K, N)
    re = 0
    for i in range(plastic.shape[1]):
        p = plastic[:, i]
        first = np.argmax(p) if p.any() else len(p)
        gap = [k for k in range(first + 1, len(p)) if not p[k]]
        re += bool(gap) and bool(p[gap[0]:].any())
    return dict(elastic=int(np.sum(~plastic)), plastic=int(np.sum(plastic)), ns0=int(np.sum(Y['nsteps'] == 0)),
                nspos=int(np.sum(Y['nsteps'] > 0)), reyield=int(re))


def assert_same_bits(name, P, Y, K=None, N=None, cols=None, ct=True):
    """load_path's dict P against the yardstick Y cut to its first K steps and N points (or its points `cols`)"""
    K = Y['sig'].shape[0] if K is None else K
    cols = np.arange(Y['sig'].shape[1] if N is None else N) if cols is None else np.asarray(cols)
    assert np.all(P['status'] == 0) and np.all(P['ksteps'] == K), (name, P['status'], P['ksteps'])
    for what in NAMES:
        a, b = P[what], Y[what][:K][:, cols]
        assert a.shape == b.shape, (name, what, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=what != 'nsteps'), '%s: %s differs at (step, point) %s (largest difference %.3e)' % (
            name, what, np.argwhere(np.reshape(a != b, (K, len(cols), -1)).any(axis=2))[:6].tolist(),
            float(np.nanmax(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float)))))
    if ct and K == Y['sig'].shape[0]:
        assert np.array_equal(P['ct'], Y['ct'][cols], equal_nan=True), '%s: ct differs (largest difference %.3e)' % (
            name, float(np.max(np.abs(P['ct'] - Y['ct'][cols]))))


# ------------------------------------------------------------------------------------------------ mixed control
K_MIXED = 24
# (name, control, driven components): driven strain components take the step 0.2 sy / E, every other entry of dload is zero
MIXED = (
    ('eps_xx driven, others stress-free', (0, 1, 1, 1, 1, 1), (0,)),
    ('eps_yy driven, others stress-free', (1, 0, 1, 1, 1, 1), (1,)),
    ('eps_xx = eps_yy driven, others stress-free', (0, 0, 1, 1, 1, 1), (0, 1)),
    ('shear xy driven, stress-free normals', (1, 1, 1, 0, 0, 0), (5,)),
    ('only sig_xx free, eps_yy driven', (1, 0, 0, 0, 0, 0), (1,)),
    ('all strain, eps_xx driven', (0, 0, 0, 0, 0, 0), (0,)),
)


def mixed_paths(sy, E, K=K_MIXED):
    """(dload (K, 6, 6), control (6, 6) bool): the six cases as six points of one call"""
    h = 0.2 * sy / E
    d = np.zeros((K, len(MIXED), 6))
    for i, (_, _, driven) in enumerate(MIXED):
        d[:, i, list(driven)] = h
    return d, np.array([c for _, c, _ in MIXED], dtype=bool)


def targets(dload, control, sig0=None):
    """t (K, N, 6): the stress targets as np.cumsum forms them from sig0; meaningful on the stress-controlled components"""
    K, N = dload.shape[:2]
    s0 = np.zeros((N, 6)) if sig0 is None else np.asarray(sig0, dtype=float)
    return np.cumsum(np.concatenate((s0[None], dload), axis=0), axis=0)[1:]


def assert_mixed(name, m, CV, dload, control, stol, tex_id=None, newton=30):
    """checks 2 (a)-(d) on the paths dload (K,N,6) under control (N,6); returns the result"""
    P = m.load_path(dload, control=control, CV=CV, tex_id=tex_id, newton=newton, return_tangent=True)
    K, N = dload.shape[:2]
    print('%s: status %s, corrections per step at most %d, largest residual %.3e (stol %.3e)'
          % (name, P['status'].tolist(), int(P['newton'].max()),
             float(np.nanmax(np.where(control[None], np.abs(P['sig'] - targets(dload, control)), 0.))), stol))
    assert np.all(P['status'] == 0) and np.all(P['ksteps'] == K), (name, P['status'], P['ksteps'])            # (a)
    assert P['newton'].min() >= 0 and P['newton'].max() <= newton, (name, P['newton'].max())
    t = targets(dload, control)
    F = np.broadcast_to(control[None], P['sig'].shape)
    assert np.all(np.abs(P['sig'] - t)[F] <= stol), (name, float(np.max(np.abs(P['sig'] - t)[F])), stol)   # (b)
    assert np.array_equal(P['deps'][~F], np.broadcast_to(dload, P['deps'].shape)[~F]), name                   # (c)
    R = m.load_path(P['deps'], CV=CV, tex_id=tex_id, return_tangent=True)                                     # (d)
    for what in NAMES + ('ct',):
        assert np.array_equal(R[what], P[what]), '%s: the replay differs in %s' % (name, what)
    assert np.all(R['newton'] == 0) and np.array_equal(R['deps'], P['deps'])
    return P


# ------------------------------------------------------------------------------------------------ the iteration on the CPU oracle
def oracle_material(m):
    """the CPU oracle's record of an analytic façade material"""
    from oracle import oracle as O
    return O.Material(kind=O.HILL6, E=float(m.E), nu=float(m.nu), sy=float(m.sy), khard=float(m.khard), hill=np.array(m.hill),
                      drucker=float(m.drucker or 0.), sdim=6)


def oracle_load_path(om, CV, dload, control, stol, sig0=None, epl0=None, newton=30, eps_cap=0.05):
    """load_path's iteration for ONE point in NumPy around the oracle's response (maxit = 50), the masked system solved by LU
    (np.linalg.solve on Ct_FF): dict of sig, epl, depl, deps (K,6), newton (K,), ksteps, status"""
    from oracle import oracle as O
    CV = np.asarray(CV, dtype=float).reshape(6, 6)
    K = len(dload)
    F = np.asarray(control, dtype=bool)
    S = ~F
    sig = np.zeros(6) if sig0 is None else np.array(sig0, dtype=float)
    epl = np.zeros(6) if epl0 is None else np.array(epl0, dtype=float)
    t, Ct = sig.copy(), CV.copy()
    out = dict(sig=np.full((K, 6), np.nan), epl=np.full((K, 6), np.nan), depl=np.full((K, 6), np.nan),
               deps=np.full((K, 6), np.nan), newton=np.full(K, -1), ksteps=0, status=0)

    def solve(A, b):
        with np.errstate(all='ignore'):
            try:
                x = np.linalg.solve(A, b)
            except np.linalg.LinAlgError:
                return None
        return x if np.all(np.isfinite(x)) else None
    for k in range(K):
        t[F] = t[F] + dload[k][F]
        deps = np.where(S, dload[k], 0.)
        if F.any():
            x = solve(Ct[np.ix_(F, F)], (t - sig)[F] - Ct[np.ix_(F, S)] @ deps[S])
            if x is None:
                out['status'] = 2
                break
            deps[F] = x
        nw = 0
        while True:
            if not np.all(np.isfinite(deps)) or np.max(np.abs(deps)) > eps_cap:
                out['status'] = 3
                break
            fy, so, dp, ct, ns = O.response(om, CV.reshape(1, 36), sig[None], epl[None], deps[None])
            s2, Ct2 = so[0], ct[0].reshape(6, 6)
            r = (s2 - t)[F]
            if not F.any() or np.max(np.abs(r)) <= stol:
                break
            if nw == newton:
                out['status'] = 1
                break
            x = solve(Ct2[np.ix_(F, F)], r)
            if x is None:
                out['status'] = 2
                break
            deps[F] -= x
            nw += 1
        if out['status']:
            break
        sig, epl, Ct = s2, epl + dp[0], Ct2
        out['sig'][k], out['epl'][k], out['depl'][k], out['deps'][k], out['newton'][k] = sig, epl, dp[0], deps, nw
        out['ksteps'] = k + 1
    return out


def r_ratio(depl):
    """(deviations, first step): |depl_yy / depl_zz| per step of a uniaxial-x path from its second plastic step on"""
    plastic = np.nonzero(np.any(depl != 0., axis=1))[0]
    k0 = int(plastic[1])
    return depl[k0:, 1] / depl[k0:, 2], k0


def hill_material():
    return FC.hill_material()

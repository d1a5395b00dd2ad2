"""Shared by the tests of the flow rule and stress update of texture materials: the gradient of the texture SVC
as a NumPy transcription, its calibration figures, the 6-feature material restated as a texture set, and a NumPy
transcription of the reference's response() that drives the façade's own texture functions.

Parameter dict p as in texture_cases.py.  Specification of the gradient (`gradient`), in the notation of texture_cases.py:
    w_i     = dual_i exp(-gamma d2_i)
    S_j     = [sum of w_i (f_j - v_ij) in the order of the 16-lane row],  j < 6
    a_j     = (-2 gamma S_j) / scale_j;   dev_only: (a_0 + a_1 + a_2) / 3 taken off a_0 .. a_2
`gradient` and `decision` run in np.longdouble from the double inputs (LD=np.float64: the same formulas in FP64)."""
import numpy as np

import texture_cases as TC

LD = np.longdouble
YF_TOL = 5.e-3   # basic.py:26


def row_sum(terms):
    """sum of the terms (nsv,) or (nsv, m) in the order of the 16-lane row (texture_cases.row_sum), in the terms' own precision"""
    terms = np.asarray(terms)
    n = len(terms)
    zero = np.zeros(terms.shape[1:], dtype=terms.dtype)
    lane = []
    for L in range(16):
        acc = [zero.copy(), zero.copy()]
        for k in range(L, n, 32):
            acc[0] = acc[0] + terms[k]
            if k + 16 < n:
                acc[1] = acc[1] + terms[k + 16]
        lane.append(acc[0] + acc[1])
    v = np.array(lane)
    v = v + v[np.arange(16) ^ 1]
    v = v + v[np.arange(16) ^ 2]
    v = v + v[np.array([7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8])]
    v = v + v[::-1]
    return v[0]


def _close(p, S, LD):
    """sums S (N,6) to the gradient: scaling and, for a dev_only set, the projection"""
    a = (LD(-2.) * LD(p['gamma']) * S) / p['scale'][:6].astype(LD)
    if p['dev_only']:
        a = a.copy()
        a[:, :3] -= (np.sum(a[:, :3], axis=1) / LD(3))[:, None]
    return a


def decision(p, sig, tex, LD=LD):
    """calc_yf(sig, tex) (N,) with the terms summed in row order"""
    f = TC.features(p, sig, tex, LD=LD)
    sv, dual, g = p['sv'].astype(LD), p['dual'].astype(LD), LD(p['gamma'])
    out = np.empty(len(f), dtype=LD)
    for i in range(len(f)):
        d = f[i][None, :] - sv
        d2 = np.zeros(len(sv), dtype=LD)
        for j in range(f.shape[1]):
            d2 = d2 + d[:, j] * d[:, j]
        out[i] = row_sum(dual * np.exp(-g * d2)) + LD(p['intercept'])
    return out


def gradient(p, sig, tex, LD=LD):
    """calc_fgrad(sig, tex) (N,6) as specified in the module docstring"""
    f = TC.features(p, sig, tex, LD=LD)
    sv, dual, g = p['sv'].astype(LD), p['dual'].astype(LD), LD(p['gamma'])
    S = np.empty((len(f), 6), dtype=LD)
    for i in range(len(f)):
        d = f[i][None, :] - sv
        d2 = np.zeros(len(sv), dtype=LD)
        for j in range(f.shape[1]):
            d2 = d2 + d[:, j] * d[:, j]
        w = dual * np.exp(-g * d2)
        S[i] = row_sum(w[:, None] * d[:, :6])
    return _close(p, S, LD)


def _plain(p, F):
    """(yf (N,), gradient (N,6)) from the standardised features F (N, 6 + tdim): plain FP64 NumPy sums"""
    y, S = np.empty(len(F)), np.empty((len(F), 6))
    for i in range(len(F)):
        d = F[i][None, :] - p['sv']
        w = p['dual'] * np.exp(-p['gamma'] * np.sum(d * d, axis=1))
        y[i] = np.sum(w) + p['intercept']
        S[i] = np.sum(w[:, None] * d[:, :6], axis=0)
    return y, _close(p, S, np.float64)


def calib(p, sig, tex):
    """(calib_yf, calib_grad) as DESIGN.md §28 takes calib: a plain FP64 sum against the same sum with every feature moved by
    one unit in the last place -- what an FP64 evaluation cannot resolve at these points"""
    F = np.asarray(TC.features(p, sig, tex), dtype=float)
    y0, a0 = _plain(p, F)
    y1, a1 = _plain(p, np.nextafter(F, np.inf))
    return float(np.max(np.abs(y1 - y0))), float(np.max(np.abs(a1 - a0)))


def grad_bar(cal, a):
    """bar of the gradient checks: 4 max(calib, 1e-12 max|a|)"""
    return 4. * max(float(cal), 1e-12 * float(np.max(np.abs(np.asarray(a, dtype=float)))))


def central_differences(yf, sig, h):
    """(N,6): central differences with step h of yf(sig (M,6)) -> (M,), all 12 N points in one call"""
    sig = np.asarray(sig, dtype=float).reshape(-1, 6)
    n, ax = len(sig), np.arange(6)
    pts = np.tile(sig[:, None, None, :], (1, 6, 2, 1))
    pts[:, ax, 0, ax] += h
    pts[:, ax, 1, ax] -= h
    y = np.asarray(yf(pts.reshape(-1, 6))).reshape(n, 6, 2)
    step = pts[:, ax, 0, ax] - pts[:, ax, 1, ax]   # the step as it was taken, in FP64
    return (y[:, :, 0] - y[:, :, 1]) / step


def fd_gap(p, sig, tex, h):
    """worst |gradient - central differences of decision| over the points, both in np.longdouble: the truncation error of the
    differences at step h (the rounding of np.longdouble is far below it)"""
    a = gradient(p, sig, tex)
    t = np.broadcast_to(np.asarray(tex, dtype=float).reshape(-1, p['tdim']), (len(sig), p['tdim']))
    fd = central_differences(lambda s: decision(p, s, np.repeat(t, 12, axis=0)), sig, h)
    return float(np.max(np.abs(a - fd)))


def fd_truncation_bound(p, h):
    """A bound of the truncation error h^2 / 6 max|f'''| of a central difference of calc_yf along a stress axis: a kernel
    exp(-gamma u^2) has the third derivative (2 gamma)^(3/2) (3 t - t^3) exp(-t^2 / 2), t = sqrt(2 gamma) u, at most
    1.38 (2 gamma)^(3/2) in magnitude; u moves by at most 1 / min(scale) per unit of stress (the deviator projection shortens
    a step), and the other features only scale a term down."""
    return h * h / 6. * 1.38 * (2. * p['gamma']) ** 1.5 / float(np.min(p['scale'][:6])) ** 3 * float(np.sum(np.abs(p['dual'])))


def six_feature_as_texture(p6, c=0.3):
    """The 6-feature SVC of yield_locus_cases.ml_params as a texture set with tdim = 1: the same vectors, coefficients,
    intercept and gamma, mean 0 and scale scale_seq on the six stress columns, a constant texture column c with mean 0 and
    scale 1.  Evaluated at tex = c its features are the 6-feature ones, bit for bit."""
    sv = np.concatenate((p6['sv'], np.full((len(p6['sv']), 1), c)), axis=1)
    return dict(sv=np.ascontiguousarray(sv), dual=np.array(p6['dual']), intercept=float(p6['intercept']), gamma=float(p6['gamma']),
                mean=np.zeros(7), scale=np.concatenate((np.full(6, p6['scale_seq']), [1.])), dev_only=bool(p6['dev_only']),
                tdim=1), np.array([c])


def deviatoric_tables(p6):
    """The dev_only function of the 6-feature tables p6 written on deviatoric vectors: for a deviatoric x,
    |x - v|^2 = |x - dev v|^2 + 3 pm^2 with pm the mean of v's three normal components, so the vectors become dev v and the
    coefficients dual exp(-3 gamma pm^2).  The same function of the stress; its gradient sums have no hydrostatic part, so
    the unprojected gradient of the 6-feature material (material.py:775, 807) is the derivative, as the projected texture
    gradient always is."""
    sv = np.array(p6['sv'])
    pm = np.sum(sv[:, :3], axis=1) / 3.
    sv[:, :3] -= pm[:, None]
    return dict(p6, sv=np.ascontiguousarray(sv), dual=p6['dual'] * np.exp(-3. * p6['gamma'] * pm * pm), dev_only=True)


def eps_eq(e):
    e = np.asarray(e, dtype=float)
    return float(np.sqrt(2. * (np.sum(e[:3] ** 2) + 0.5 * np.sum(e[3:] ** 2)) / 3.))


def replay(m, CV, sig, epl, deps, tex, maxit=50, ulp=False):
    """NumPy transcription of the reference's response (material.py:207-346) for a texture material: the yield function,
    ML_full_yf and the gradient are the façade's own device calls at the texture `tex`.  ulp: every stress handed to them is
    moved by one unit in the last place, which moves the standardised features by about as much."""
    CV = np.asarray(CV, dtype=float)
    epl = np.asarray(epl, dtype=float)
    deps = np.asarray(deps, dtype=float)
    kh = float(m.khard)

    def mv(s):
        return np.nextafter(s, np.inf) if ulp else s

    def yf(s):
        return float(m.calc_yf(mv(s), tex=tex))

    def full(s):
        return float(m.ML_full_yf(mv(s), tex=tex, verb=False))

    def step(s, d):   # epl_dot and C_tan of one (sub-)step
        yfun = yf(s + CV @ d)
        a = m.calc_fgrad(mv(s), tex=tex)
        m.khard = kh                                     # (calc_fgrad sets khard = 0; the device keeps the record's value)
        ca = CV @ a
        hh = a @ ca + kh
        pdot = np.zeros(6) if yfun <= YF_TOL else (a @ CV @ d / hh) * a
        return pdot, CV - np.outer(ca, ca) / hh

    sig = np.array(sig, dtype=float)
    depl = np.zeros(6)
    toler = YF_TOL * (m.sy + eps_eq(epl) * kh)
    dsig = CV @ deps
    st_scal, niter = 1., 0
    fy1 = full(sig + dsig)
    if fy1 < toler:
        return dict(fy1=fy1, sig=sig + dsig, depl=depl, ct=np.array(CV), nsteps=0)
    fy0 = yf(sig)
    if fy0 < -0.15:
        fy0 = full(sig)
        st_scal += fy0 / float(m.calc_seq(dsig))
        deps_el = deps * (1. - st_scal)
        sig = sig + CV @ deps_el
        grad_stiff = CV * (1. - st_scal)
        deps_r = deps - deps_el
    else:
        deps_r = np.array(deps, dtype=float)
        grad_stiff = np.zeros((6, 6))
    ddepl, t_stiff = step(sig, deps_r)
    fy1 = full(sig + t_stiff @ deps_r)
    nsteps = 1
    if fy1 > toler:
        deps_r = deps_r / maxit
        nsteps = maxit
    SV = np.zeros((6, 6))
    SV[0:3, 0:3] = np.linalg.inv(CV[0:3, 0:3])
    for i in range(3, 6):
        SV[i, i] = 1. / CV[i, i]
    for niter in range(nsteps):
        ddepl, t_stiff = step(sig, deps_r)
        sig = sig + t_stiff @ deps_r
        fy1 = full(sig)
        if fy1 > toler:
            ds = sig * fy1 / float(m.calc_seq(sig))
            sig = sig - ds
            ddepl = ddepl + SV @ ds
            A = np.array([[deps_r[0], 0., 0., 0., deps_r[2], deps_r[1]],
                          [0., deps_r[1], 0., deps_r[2], 0., deps_r[0]],
                          [0., 0., deps_r[2], deps_r[1], deps_r[0], 0.]])
            x = np.linalg.lstsq(A, ds[0:3], rcond=None)[0]
            Ct = np.zeros((6, 6))
            Ct[0:3, 0:3] = np.array([[x[0], x[5], x[4]], [x[5], x[1], x[3]], [x[4], x[3], x[2]]])
            t_stiff = t_stiff - Ct
            fy1 = full(sig)
        grad_stiff = grad_stiff + t_stiff * st_scal / nsteps
        depl = depl + ddepl
    return dict(fy1=fy1, sig=sig, depl=depl, ct=grad_stiff, nsteps=niter)

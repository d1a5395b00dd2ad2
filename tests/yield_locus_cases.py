"""Shared by tools/gen_yield_locus.py and the yield-locus tests: the cases of tests/golden/yield_locus.npz, the materials
they belong to (as parameter dicts and as façade Materials) and the np.longdouble restatement of the SVC decision function
along a ray with its derivative and its gauge.

Restatement, from the material's own tables (sv, dual, intercept, gamma, scale_seq, scale_wh): with x the factor along su
    6 features    phi = x u,               u = (su - p 1 if dev_only) / scale_seq
    15 features   phi = (x u, epl / scale_wh, 0, 0, 0)
    2 features    phi = (x seq_J2(su) / scale_seq - 1, polar angle(su) / pi)          (su: principal stresses)
    f_L(x) = sum_i c_i k_i + b,  k_i = exp(-gamma |phi - v_i|^2),   A = sum_i |c_i| k_i + |b|   (the gauge of svc_hessian.npz)
    f_L'(x) = -2 gamma sum_i c_i k_i (phi - v_i) . dphi/dx
all in np.longdouble from the double inputs."""
import os

import numpy as np

from ray_cases import march_replay as _march_replay, ulp

LD = np.longdouble
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS53 = LD(2.) ** -53

# ML cases: tag -> (table file, dev_only)
ML_CASES = {'hill': ('svc_hill.npz', False), 'hilldev': ('svc_hill.npz', True), 'hill3d': ('svc_hill3d.npz', False),
            'wh': ('svc_workhard.npz', False)}
# analytic cases with khard > 0: tag -> plasticity arguments (Barlat's coefficients come from seq_extra.npz)
ANA_CASES = {
    'ahill6': dict(sy=80., khard=1500., hill=[0.7, 1., 1.4, 1., 1.2, 0.8], sdim=6),
    'ahill3': dict(sy=120., khard=900., hill=[1.3, 0.8, 1.1], sdim=3),
    'aj2p': dict(sy=100., khard=500., sdim=3),
    'atresca': dict(sy=100., khard=700., tresca=True, sdim=6),
    'abarlat': dict(sy=46.76, khard=300., sdim=6),
}
# relative tolerance of calc_seq per analytic family, as tests/test_gpu_material.py holds it (1e-13 relative for Hill on Voigt
# stresses; 1e-10 absolute for principal-stress Hill / J2 and Tresca, i.e. relative to seq(su); 1e-11 relative for Barlat)
ANA_SEQ_TOL = {'ahill6': ('rel', 1e-13), 'ahill3': ('abs', 1e-10), 'aj2p': ('abs', 1e-10), 'atresca': ('abs', 1e-10),
               'abarlat': ('rel', 1e-11)}
WH_EPL = (None, 0.002 * np.array([1., -0.5, -0.5, 0., 0., 0.]), 0.01 * np.array([0.3, -0.8, 0.5, 0.4, 0., -0.2]))
ANA_EPL = (None, 0.002 * np.array([1., -0.5, -0.5, 0., 0., 0.]))
SLICES = ((0, 1), (3, 3))   # axis codes of the two slices; the second is p = sigma_1 = sigma_2 against sigma_3
NA_POLAR, NA_SLICE, NMESH, NP_FIELD = 72, 24, 21, 9


def ml_params(tag):
    """parameter dict of an ML case from its table file"""
    src, dev_only = ML_CASES[tag]
    z = np.load(os.path.join(GOLD, src))
    p = dict(sv=np.array(z['par_sv']), dual=np.array(z['par_dual']), intercept=float(z['par_intercept']),
             gamma=float(z['par_gamma']), scale_seq=float(z['par_scale_seq']), dev_only=bool(dev_only),
             E=float(z['par_E']), nu=float(z['par_nu']), sy=float(z['par_sy']), hill=np.array(z['par_hill']),
             sdim=int(z['par_sdim']), Ndof=int(z['par_Ndof']), khard=float(z['par_khard']))
    if p['Ndof'] == 15:
        p['scale_wh'], p['ind_wh'] = float(z['par_scale_wh']), int(z['par_ind_wh'])
    return p


def facade_ml(tag, nsv=None, pad=0, intercept=None):
    """façade Material of an ML case; nsv: the table cut to its first nsv vectors; pad: that many vectors with a zero dual
    coefficient appended (a table of another size that defines the same function); intercept: another intercept (mirrored
    in the returned parameters, so that `restate` sees the function the device evaluates)"""
    import pylabfea_amd as FE
    p = ml_params(tag)
    if intercept is not None:
        p['intercept'] = float(intercept)
    sv, dual = p['sv'][:nsv], p['dual'][:nsv]
    if pad:
        sv = np.vstack((sv, np.tile(sv[:1], (pad, 1))))
        dual = np.concatenate((dual, np.zeros(pad)))
    m = FE.Material(name=tag)
    m.elasticity(E=p['E'], nu=p['nu'])
    m.plasticity(sy=p['sy'], hill=list(p['hill']), sdim=p['sdim'])
    m.set_svc(sv, dual, p['intercept'], p['gamma'], p['scale_seq'], dev_only=p['dev_only'], scale_wh=p.get('scale_wh'))
    p = dict(p, sv=sv, dual=dual)
    return m, p


def analytic(FE, tag):
    """Material of package FE (the façade or the reference) of an analytic case"""
    kw = dict(ANA_CASES[tag])
    if tag == 'abarlat':
        z = np.load(os.path.join(GOLD, 'seq_extra.npz'))
        kw.update(barlat=list(z['barlat_par']), barlat_exp=int(z['barlat_exp']))
    m = FE.Material(name=tag)
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(**kw)
    return m


def j2(s):
    s = np.asarray(s)
    v = 0.5 * ((s[:, 0] - s[:, 1]) ** 2 + (s[:, 1] - s[:, 2]) ** 2 + (s[:, 2] - s[:, 0]) ** 2)
    if s.shape[1] == 6:
        v = v + 3 * (s[:, 3] ** 2 + s[:, 4] ** 2 + s[:, 5] ** 2)
    return np.sqrt(v)


def restate(p, su, epl, x, LD=LD):
    """(f_L, f_L', A) at the factors x (N,) along su (N,6) with plastic strains epl (N,6), np.longdouble; with
    LD=np.float64 the same formula in plain FP64 NumPy (what an FP64 evaluation that is not the device's makes of it)"""
    su, x = np.asarray(su, dtype=LD), np.asarray(x, dtype=LD)
    sv, dual = p['sv'].astype(LD), p['dual'].astype(LD)
    g, sc = LD(p['gamma']), LD(p['scale_seq'])
    n = len(su)
    f, df, A = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for i in range(n):
        if p['Ndof'] == 2:
            sp = su[i, :3]
            seq = j2(sp[None])[0]
            dev = sp - np.sum(sp) / 3
            vn = np.sqrt(np.sum(dev * dev))
            dn = dev / (vn if vn >= 1.e-4 else LD(1.))
            a = np.array([2, -1, -1], dtype=LD) / np.sqrt(LD(6))
            b = np.array([0, 1, -1], dtype=LD) / np.sqrt(LD(2))
            phi = np.array([x[i] * seq / sc - 1, np.arctan2(np.sum(dn * b), np.sum(dn * a)) / LD(np.pi)])
            dphi = np.array([seq / sc, LD(0)])
        else:
            s = su[i].copy()
            if p['dev_only']:
                s[:3] -= np.sum(s[:3]) / 3
            u = s / sc
            phi, dphi = x[i] * u, u
            if p['Ndof'] == 15:
                e = np.asarray(epl[i], dtype=LD) / LD(p['scale_wh'])
                z3 = np.zeros(3, dtype=LD)
                phi, dphi = np.concatenate((phi, e, z3)), np.concatenate((dphi, 0 * e, z3))
        d = phi[None, :] - sv
        k = np.exp(-g * np.sum(d * d, axis=1))
        f[i] = np.sum(dual * k) + LD(p['intercept'])
        df[i] = -2 * g * np.sum(dual * k * (d @ dphi))
        A[i] = np.sum(np.abs(dual) * k) + abs(LD(p['intercept']))
    return f, df, A


def residual_bar(U, df, A, x):
    """bar (1): evaluation noise at termination plus the resolution of x"""
    return LD(U) * A * EPS53 + np.abs(df) * 2 * ulp(x)


def root_bar(U, df, A, x):
    """bar (2): both roots sit in the noise band around the true one"""
    return 2 * LD(U) * A * EPS53 / np.abs(df) + 4 * ulp(x)


def default_x0(p, su):
    """start value of yield_scale without x0 and without plastic strain: sy / seq_J2(su)"""
    su = np.asarray(su, dtype=float)
    return p['sy'] / j2(su[:, :3] if p['Ndof'] == 2 else su)


def crossing_intercept(p, su, ep, x0s):
    """An intercept with which a CUT table has the marched crossing along many of the rays: the kernel sum S(x) = f_L - b
    is sampled at the points of the march from each start value (x0 0.98^k down to 0.01 x0, x0 1.02^k up to 5 x0) and b is
    taken from -S's quantiles such that most (ray, start) pairs see f_L(x0) >= 0 and f_L < 0 further down, or f_L(x0) < 0
    and f_L >= 0 further up.  Computed from the tables alone."""
    q = dict(p, intercept=0.)
    dn, up = 0.98 ** np.arange(0, 229, 4), 1.02 ** np.arange(0, 83, 2)
    S0, Sd, Su = [], [], []
    for x0 in x0s:
        S0.append(restate(q, su, ep, x0)[0])
        Sd.append(np.array([restate(q, su, ep, x0 * f)[0] for f in dn[1:]]))
        Su.append(np.array([restate(q, su, ep, x0 * f)[0] for f in up[1:]]))
    S0, Sd, Su = np.concatenate(S0), np.concatenate(Sd, axis=1), np.concatenate(Su, axis=1)
    vals = np.concatenate((S0, Sd.ravel(), Su.ravel())).astype(float)
    best, best_b = -1, 0.
    for b in -np.quantile(vals, np.linspace(0.02, 0.98, 49)):
        ok = ((S0 + b >= 0) & np.any(Sd + b < 0, axis=0)) | ((S0 + b < 0) & np.any(Su + b >= 0, axis=0))
        if np.sum(ok) > best:
            best, best_b = int(np.sum(ok)), float(b)
    return best_b


def march_replay(p, su, ep, x0):
    """status per ray (0 bracket found, 1 none) of the march of yield_scale, replayed with the restatement
    (ray_cases.march_replay); `clear` is False where some |f_L| of the march is within 1e-9 A of zero, i.e. where FP64 noise
    could decide otherwise"""
    clear = np.ones(len(su), dtype=bool)

    def seen(act, f, A):
        clear[act] &= np.asarray(np.abs(f) > 1e-9 * A)
    return _march_replay(lambda act, x: restate(p, su[act], ep[act], x)[::2], x0, seen), clear

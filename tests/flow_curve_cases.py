"""Shared by tools/gen_flow_curve.py, tools/flow_curve_bench.py and the flow-curve tests: the materials of
tests/golden/flow_curve.npz as façade Materials with their parameter dicts (the dicts of tests/yield_locus_cases.py), and a
NumPy transcription of the device's flow-curve chain: the search of plfx_rayroot.hpp statement by statement, the step rule,
and the gradient of the decision function with its gauges.

Gradient and gauges, from the tables: with phi the features at su * xs and k_i = exp(-gamma |phi - v_i|^2)
    a_f  = -2 gamma / scale_seq   sum_i c_i k_i (phi_f - v_if),  f < 6        G_f = 2 gamma / scale_seq  sum_i |c_i| k_i |phi_f - v_if|
    hk   =  2 gamma scale_seq / scale_wh  sum_i c_i k_i sum_{6<=f<12} (phi_f - v_if)     Gh likewise with absolute values
An FP64 evaluation of a_f in any order of summation is off by a few units of G_f 2^-53."""
import os
import warnings

import numpy as np

import yield_locus_cases as YC

LD = np.longdouble
GOLD = YC.GOLD
CAP_DOWN, CAP_UP, CAP_BISECT = 240, 90, 80
EXAMPLE_DIRS = np.array([[-1., 0, 0, 0, 0, 0], [0, -1., 0, 0, 0, 0], [-1., 1., 0, 0, 0, 0], [1., 1., 0, 0, 0, 0]])


def eps_eq(e):
    e = np.asarray(e)
    return np.sqrt(2. * (np.sum(e[..., :3] ** 2, axis=-1) + 0.5 * np.sum(e[..., 3:] ** 2, axis=-1)) / 3.)


def params_of(m):
    """parameter dict (tests/yield_locus_cases.py) of a façade ML material with sdim = 6"""
    p = dict(sv=np.array(m.svc['sv']), dual=np.array(m.svc['dual']), intercept=float(m.svc['intercept']),
             gamma=float(m.gam_yf), scale_seq=float(m.scale_seq), dev_only=bool(m.dev_only), sy=float(m.sy),
             Ndof=int(m.svc['sv'].shape[1]))
    if p['Ndof'] == 15:
        p['scale_wh'] = float(m.scale_wh)
    return p


def wh_material(nsv=None, intercept=None, dev_only=False):
    """(material, parameters): the work-hardening material of tests/svr_flow_cases.py::svc_material(), with the load-case
    indices of its data set, ML_grad = False; nsv cuts the table, intercept replaces its intercept"""
    import pylabfea_amd as FE
    w = np.load(os.path.join(GOLD, 'svc_data_training.npz'))
    md = dict(sdim=6, wh_data=True, Name='ML_Hill_hardening')
    for k in ('flow_stress', 'plastic_strain', 'elast_const', 'sy_av', 'peeq_max', 'lc_indices'):
        md[k] = np.array(w['wh_md_' + k]) if w['wh_md_' + k].ndim else float(w['wh_md_' + k])
    md['Nlc'] = int(w['wh_md_Nlc'])
    m = FE.Material(name='ML_Hill_hardening_C2.0_G1.5', num=2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m.from_data(md)
    Nseq, ss, sw = int(w['wh_Nseq']), float(w['wh_scale_seq']), float(w['wh_scale_wh'])
    X = np.zeros((2 * Nseq * len(w['wh_md_flow_stress']), 15))
    X[:, 0:6] = (w['wh_seq'][:, None, None] * w['wh_md_flow_stress'][None]).reshape(-1, 6) / ss
    X[:, 6:12] = np.tile(w['wh_md_plastic_strain'], (2 * Nseq, 1)) / sw
    sup = w['wh_ns_support'][:nsv]
    b = float(w['wh_ns_intercept']) if intercept is None else float(intercept)
    m.set_svc(X[sup], w['wh_ns_dual'][:nsv], b, float(w['wh_gamma']), ss, C=float(w['wh_C']), scale_wh=sw, dev_only=dev_only)
    m.ML_grad = False
    return m, params_of(m)


def hill_material(FE=None):
    """the Hill reference material of the work-hardening data (tools/gen_svc_data_training.py::wh_lc_data)"""
    if FE is None:
        import pylabfea_amd as FE
    m = FE.Material(name='Hill-reference', num=1)
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=50., rv=[1.2, 1.0, 0.8, 1.0, 1.0, 1.0], khard=1000.0, sdim=6)
    return m


def svc6_material(nsv=None, intercept=None, dev_only=False):
    """(material, parameters): the 6-feature material of tests/golden/svc_hill.npz"""
    m, p = YC.facade_ml('hilldev' if dev_only else 'hill', nsv=nsv, intercept=intercept)
    return m, dict(p, Ndof=6)


def directions(load_cases):
    """the twelve directions of the fixture: the example's four and eight rows of load_cases(0, 8) mixed by default_rng(31),
    all of unit J2 stress"""
    rng = np.random.default_rng(31)
    lc = load_cases(0, 8)
    mix = lc * rng.uniform(0.5, 1.5, size=(8, 6)) * rng.choice([-1., 1.], size=(8, 6))
    d = np.vstack((EXAMPLE_DIRS, mix))
    return d / YC.j2(d)[:, None]


def features(p, su, epl, xs, LD=np.float64):
    s = np.asarray(su, dtype=LD).copy()
    if p['dev_only']:
        s[:3] -= np.sum(s[:3]) / 3
    phi = LD(xs) * s / LD(p['scale_seq'])
    if p['Ndof'] == 15:
        phi = np.concatenate((phi, np.asarray(epl, dtype=LD) / LD(p['scale_wh']), np.zeros(3, dtype=LD)))
    return phi


def decision(p, su, epl, x, LD=np.float64):
    d = features(p, su, epl, x, LD)[None, :] - p['sv'].astype(LD)
    return np.sum(p['dual'].astype(LD) * np.exp(-LD(p['gamma']) * np.sum(d * d, axis=1))) + LD(p['intercept'])


def gradient(p, su, epl, xs, LD=np.float64):
    """(a (6,), hk, G (6,), Gh) at su * xs: gradient w.r.t. the stress, raw hardening value (NaN without work-hardening
    features) and their gauges"""
    d = features(p, su, epl, xs, LD)[None, :] - p['sv'].astype(LD)
    g, sc = LD(p['gamma']), LD(p['scale_seq'])
    w = p['dual'].astype(LD) * np.exp(-g * np.sum(d * d, axis=1))
    a = -2 * g / sc * np.sum(w[:, None] * d[:, :6], axis=0)
    G = 2 * g / sc * np.sum(np.abs(w)[:, None] * np.abs(d[:, :6]), axis=0)
    if p['Ndof'] != 15:
        return a, LD(np.nan), G, LD(np.nan)
    c = 2 * g * sc / LD(p['scale_wh'])
    return a, c * np.sum(w * np.sum(d[:, 6:12], axis=1)), G, c * np.sum(np.abs(w) * np.sum(np.abs(d[:, 6:12]), axis=1))


def ray_root(f, x0):
    """(status, root) of plfx_rayroot.hpp on the scalar function f"""
    phase, cnt = 0, 0
    x, lo, hi, flo, fhi = x0, 0., 0., 0., 0.
    while True:
        fx = f(x)
        if fx != fx:
            return 1, np.nan
        if phase == 0:
            phase = 1 if fx >= 0. else 2
        if phase == 1:
            if fx < 0.:
                lo, flo, phase = x, fx, 3
            else:
                hi, fhi = x, fx
                cnt += 1
                if x < 0.01 * x0 or cnt > CAP_DOWN:
                    return 1, np.nan
                x *= 0.98
                continue
        elif phase == 2:
            if fx >= 0.:
                hi, fhi, phase = x, fx, 3
            else:
                lo, flo = x, fx
                cnt += 1
                if x > 5. * x0 or cnt > CAP_UP:
                    return 1, np.nan
                x *= 1.02
                continue
        elif fx < 0.:
            lo, flo = x, fx
        else:
            hi, fhi = x, fx
        if phase == 3:
            phase, cnt = 4, 0
        mid = lo + 0.5 * (hi - lo)
        if not (lo < mid < hi):
            return 0, (lo if -flo < fhi else hi)
        cnt += 1
        if cnt > CAP_BISECT:
            return 2, np.nan
        x = mid


def flow_curve(p, su, epl0=None, max_steps=300, depl=1.e-3, epl_max=0.02, predictor=0., dec=None, grad=None):
    """One curve of the device's chain in FP64 NumPy: dict of x (K+1,), epl (K+1, 6), yf (K+1,), hk (K,), nsteps, status
    with K = max_steps and NaN past the last recorded point.  dec(su, epl, x) / grad(su, epl, xs) -> (a, hk) replace the
    plain sums (the fixture generator passes the reference's functions)."""
    dec = dec or (lambda s, e, x: float(decision(p, s, e, x)))
    grad = grad or (lambda s, e, xs: gradient(p, s, e, xs)[:2])
    K = int(max_steps)
    out = dict(x=np.full(K + 1, np.nan), epl=np.full((K + 1, 6), np.nan), yf=np.full(K + 1, np.nan), hk=np.full(K, np.nan))
    su = np.asarray(su, dtype=float)
    e = np.zeros(6) if epl0 is None else np.array(epl0, dtype=float)
    x, k, rec = float(p['sy']), 0, 0
    st = 0 if (np.all(np.isfinite(su)) and np.all(np.isfinite(e)) and np.any(su != 0.)) else 3
    while st == 0:
        st, root = ray_root(lambda t: dec(su, e, t), x)
        if st:
            break
        x = root
        out['x'][k], out['epl'][k], out['yf'][k] = x, e, dec(su, e, x)
        rec = k + 1
        peeq = eps_eq(e) + depl
        if k >= K or not peeq <= epl_max:
            break
        a, hk = grad(su, e, x + peeq * predictor)
        a = np.asarray(a, dtype=float)
        ea = eps_eq(a)
        if not ea > 0. or not np.isfinite(ea):
            st = 4
            break
        out['hk'][k] = hk
        e = e + a * depl / ea
        k += 1
    out['nsteps'], out['status'] = max(rec - 1, 0), st
    return out

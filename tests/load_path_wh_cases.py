"""Helpers of the load-path tests of the work-hardening SVC (Material.load_path(khard0=)): the materials on the
tables of tests/golden/svc_workhard.npz -- whole, cut to 1 / 63 / 64 / 65 vectors, padded past the LDS of a CU --, the
yardstick of the thread form -- K calls of Context.response(khard_in, return_khard=True, maxit) with the modulus carried and
epl += depl in NumPy --, the measured bar of the wave form, and §40's iteration restated in NumPy around the CPU oracle's
response_wh with the same carry.

Voigt order: xx, yy, zz, yz, xz, xy."""
import os

import numpy as np

import load_path_cases as LP
import yield_locus_cases as YC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAMES = ('sig', 'epl', 'fy', 'nsteps', 'khard')
CUTS = (1, 63, 64, 65)          # 63 / 64 / 65 straddle the lane split of the wave form
N_PADDED = 1400                 # 1400 x 16 doubles = 175 KiB: more than the LDS of a CU, the tables stay in device memory
K_PATH = 12


def golden():
    return np.load(os.path.join(GOLD, 'svc_workhard.npz'))


def params(z, nsv=None, pad_to=None, intercept=None, reverse=False):
    """parameter dict (tests/yield_locus_cases.py) of the tables cut to their first nsv vectors, padded with zero-coefficient
    rows to pad_to rows, or with their rows in reverse order (the same function summed in another order)"""
    sv, dual = np.array(z['par_sv'])[:nsv], np.array(z['par_dual'])[:nsv]
    if pad_to:
        sv = np.vstack((sv, np.tile(sv[:1], (pad_to - len(sv), 1))))
        dual = np.concatenate((dual, np.zeros(pad_to - len(dual))))
    if reverse:
        sv, dual = sv[::-1], dual[::-1]
    return dict(sv=np.ascontiguousarray(sv), dual=np.ascontiguousarray(dual),
                intercept=float(z['par_intercept']) if intercept is None else float(intercept), gamma=float(z['par_gamma']),
                scale_seq=float(z['par_scale_seq']), scale_wh=float(z['par_scale_wh']), dev_only=bool(z['par_dev_only']),
                sy=float(z['par_sy']), Ndof=15)


def facade(FE, z, p, name='ML-hardening'):
    """façade material on the tables p: tests/test_workhard_svc.py::facade_material with the tables handed in"""
    m = FE.Material(name=name)
    m.elasticity(CV=z['par_CV'])
    m.plasticity(sy=float(z['par_sy']), sdim=6)
    m.set_svc(p['sv'], p['dual'], p['intercept'], p['gamma'], p['scale_seq'], dev_only=p['dev_only'], scale_wh=p['scale_wh'])
    return m


def table(FE, z, which, reverse=False):
    """(material, parameters) of a table by name: 'full', 'padded', or a cut size of CUTS, which gets an intercept from its own
    tables with which it has a locus along most rays (yield_locus_cases.crossing_intercept)"""
    if which == 'full':
        p = params(z, reverse=reverse)
    elif which == 'padded':
        p = params(z, pad_to=N_PADDED, reverse=reverse)
    else:
        p = params(z, nsv=int(which))
        su = FE.load_cases(0, 20)
        b = YC.crossing_intercept(p, su, np.zeros((20, 6)), [np.full(20, p['sy'])])
        p = params(z, nsv=int(which), intercept=b, reverse=reverse)
    return facade(FE, z, p, name='ML-hardening-%s' % which), p


def yardstick(m, CV, dload, maxit, khard0, sig0=None, epl0=None):
    """the host loop: K calls of the point response on all N points with khard_in / return_khard, the modulus carried and
    epl += depl in NumPy between them; dict of sig, epl, depl (K,N,6), fy, nsteps, khard (K,N) and ct (N,6,6) after the last"""
    K, N = dload.shape[:2]
    ctx = m._load(CV)
    sig = np.zeros((N, 6)) if sig0 is None else np.array(sig0, dtype=float)
    epl = np.zeros((N, 6)) if epl0 is None else np.array(epl0, dtype=float)
    kh = np.ascontiguousarray(np.broadcast_to(np.asarray(khard0, dtype=float), (N,)))
    out = dict(sig=np.empty((K, N, 6)), epl=np.empty((K, N, 6)), depl=np.empty((K, N, 6)), fy=np.empty((K, N)),
               nsteps=np.empty((K, N), dtype=np.int32), khard=np.empty((K, N)))
    ct = None
    for k in range(K):
        fy, so, dp, ct, ns, kh = ctx.response(sig, epl, np.ascontiguousarray(dload[k]), khard_in=kh, return_khard=True, maxit=maxit)
        sig, epl = so, epl + dp
        out['sig'][k], out['epl'][k], out['depl'][k], out['fy'][k], out['nsteps'][k], out['khard'][k] = sig, epl, dp, fy, ns, kh
    out['ct'] = np.array(ct).reshape(N, 6, 6)
    return out


def events(Y, khard0):
    """LP.events plus the steps after which the carried modulus differs from the one before"""
    ev = LP.events(Y)
    before = np.concatenate((np.broadcast_to(np.asarray(khard0, dtype=float), Y['khard'][:1].shape), Y['khard'][:-1]), axis=0)
    ev['khard_changed'] = int(np.sum(Y['khard'] != before))
    return ev


def assert_same_bits(name, P, Y, K=None, N=None, cols=None, ct=True):
    """load_path's dict P against the yardstick Y cut to its first K steps and N points (or its points `cols`), khard included"""
    LP.assert_same_bits(name, P, Y, K=K, N=N, cols=cols, ct=ct)
    K = Y['sig'].shape[0] if K is None else K
    cols = np.arange(Y['sig'].shape[1] if N is None else N) if cols is None else np.asarray(cols)
    a, b = P['khard'], Y['khard'][:K][:, cols]
    assert a.shape == b.shape and np.array_equal(a, b), '%s: khard differs at (step, point) %s' % (name, np.argwhere(a != b)[:6].tolist())


# ------------------------------------------------------------------------------------------------ the bar of the wave form
def calibration(Ya, Yb):
    """Two yardstick runs of the same paths that differ only in the order of the support-vector sums (the table and the table
    with its rows reversed).  Returns (calib, first): calib[what] (K,N) the difference per output and step (the largest over
    the components), first (N,) the first step at which the two runs differ in nsteps (K where they never do): a path is
    compared only before that step."""
    K, N = Ya['nsteps'].shape
    differ = Ya['nsteps'] != Yb['nsteps']
    first = np.where(differ.any(axis=0), np.argmax(differ, axis=0), K)
    calib = {}
    for what in ('sig', 'epl', 'fy', 'khard'):
        d = np.abs(Ya[what] - Yb[what])
        calib[what] = d.reshape(K, N, -1).max(axis=2)
    return calib, first


def assert_within_bar(name, P, Y, calib, first, cols=None):
    """P (load_path's dict, any form) against the yardstick Y on the stable steps: equal nsteps, every output within
    4 max(calib, 1e-12 max|output|) -- the rule of DESIGN.md §21.  Returns the worst ratio to the bar."""
    K = P['sig'].shape[0]
    cols = np.arange(P['sig'].shape[1]) if cols is None else np.asarray(cols)
    stable = np.arange(K)[:, None] < first[cols][None, :]                     # (K, n)
    assert np.all(P['ksteps'] >= np.minimum(first[cols], K)), (name, P['ksteps'], first[cols])
    assert np.array_equal(P['nsteps'][stable], Y['nsteps'][:K][:, cols][stable]), '%s: nsteps differs on a stable step' % name
    worst = 0.
    for what in ('sig', 'epl', 'fy', 'khard'):
        y = Y[what][:K][:, cols]
        d = np.abs(P[what] - y).reshape(K, len(cols), -1).max(axis=2)
        bar = 4. * np.maximum(calib[what][:K][:, cols], 1.e-12 * float(np.max(np.abs(Y[what]))))
        r = float(np.max((d / bar)[stable])) if stable.any() else 0.
        worst = max(worst, r)
        assert r <= 1., '%s: %s is %.2f times the bar on a stable step (difference %.3e)' % (name, what, r, float(np.max(d[stable])))
    return worst


# ------------------------------------------------------------------------------------------------ the iteration on the CPU oracle
def oracle_load_path(om, CV, dload, control, stol, khard0=0., sig0=None, epl0=None, newton=30, eps_cap=0.05):
    """load_path_cases.oracle_load_path with the modulus as state: every trial of a step is response_wh(khard_in = the step's
    entry modulus); on acceptance the modulus is the accepted trial's.  Adds khard, nsteps (K,) and newton to the dict."""
    from oracle import oracle as O
    CV = np.asarray(CV, dtype=float).reshape(6, 6)
    K = len(dload)
    F = np.asarray(control, dtype=bool)
    S = ~F
    sig = np.zeros(6) if sig0 is None else np.array(sig0, dtype=float)
    epl = np.zeros(6) if epl0 is None else np.array(epl0, dtype=float)
    t, Ct, kh = sig.copy(), CV.copy(), float(khard0)
    out = dict(sig=np.full((K, 6), np.nan), epl=np.full((K, 6), np.nan), depl=np.full((K, 6), np.nan),
               deps=np.full((K, 6), np.nan), khard=np.full(K, np.nan), newton=np.full(K, -1), nsteps=np.full(K, -1),
               ksteps=0, status=0)

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
            fy, so, dp, ct, ns, ko = O.response_wh(om, CV.reshape(1, 36), sig[None], epl[None], deps[None], khard_in=[kh])
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
        sig, epl, Ct, kh = s2, epl + dp[0], Ct2, float(ko[0])
        out['sig'][k], out['epl'][k], out['depl'][k], out['deps'][k] = sig, epl, dp[0], deps
        out['khard'][k], out['newton'][k], out['nsteps'][k] = kh, nw, int(ns[0])
        out['ksteps'] = k + 1
    return out


def mixed_paths(sy, E, K=K_PATH):
    """(dload (K, 6, 6), control (6, 6) bool): the six cases of load_path_cases.MIXED as six points of one call"""
    return LP.mixed_paths(sy, E, K=K)

#!/usr/bin/env python3
"""GPU time per SMO iteration of the two single-fit paths: k_smo (one workgroup, plfx_svc_fit_batch) and k_smo_wide (many
workgroups, plfx_svc_fit_wide).  Problems: config 4's 15 000 x 6 fit (Hill reference of examples/train_hill.py, C = 2,
gamma = 1) and the full-size work-hardening problem of examples/train_hardening.py (Nlc = 300, depl = 1e-3 up to
epl_max = 0.03, Nseq = 25, C = 2, gamma = 1.5), whose data is built natively: load-case curves of the hardening Hill
material, Data, from_data and the training rows of train_SVC.  The wide path fits it to convergence; k_smo runs it with
max_iter = --cap so that it ends.  Random subsets of 1 024 .. 8 192 rows of the config-4 problem give the crossover.
Prints one JSON line with, per path, n, d, iterations, seconds, us per iteration.

    python tools/svc_data_train_bench.py [--cap 4096] [--reps 2]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def hardening_data(FE, Nlc=300, epl_max=0.03, depl=1.e-3, khard=1000.):
    """examples/train_hardening.py::create_data with the package's own Material"""
    mat = FE.Material(name='Hill-reference', num=1)
    mat.elasticity(E=200.e3, nu=0.3)
    mat.plasticity(sy=50., rv=[1.2, 1.0, 0.8, 1.0, 1.0, 1.0], khard=khard, sdim=6)
    nl3d = int(Nlc / 3)
    sunit = FE.load_cases(nl3d, Nlc - nl3d)
    sig_ideal = sunit * mat._yield_scale(sunit)[:, None]
    SV = np.linalg.inv(mat.CV)
    lc = {}
    for i, st in enumerate(sig_ideal):
        epl, peeq = np.zeros(6), 0.
        seq = FE.sig_eq_j2(st)
        su = st / seq
        sl = [su * j * seq / 5 for j in range(6)]
        el = [np.zeros(6)] * 6
        while peeq < epl_max:
            peeq = FE.eps_eq(epl) + depl
            sg = su * (seq + peeq * khard)
            epl = epl + mat.calc_fgrad(sg, epl=epl) * depl
            sl.append(sg)
            el.append(np.array(epl))
        s, e = np.array(sl), np.array(el)
        lc['Us_lc%03d_x_y_z' % i] = {'Stress': s, 'Eq_Stress': FE.sig_eq_j2(s), 'Strain_Plastic': e,
                                     'Eq_Strain_Plastic': FE.eps_eq(e), 'Strain_Total': e + s @ SV.T}
    return lc


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t)
    return min(ts), r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--cap', type=int, default=4096, help='max_iter of the k_smo run of the full-size problem')
    ap.add_argument('--reps', type=int, default=2)
    a = ap.parse_args()
    import pylabfea_amd as FE
    from pylabfea_amd.material import _ctx
    ctx = _ctx()
    res = {}

    def run(tag, X, y, C, g, wide, max_iter=-1, reps=a.reps):
        if wide:
            t, r = timed(lambda: ctx.svc_fit_wide(X, y, C, g, max_iter=max_iter), reps)
        else:
            t, r = timed(lambda: ctx.svc_fit_batch(X, y, [np.arange(len(y))], C, g, max_iter=max_iter)[0], reps)
        res[tag] = dict(n=len(y), d=X.shape[1], iters=r['n_iter'], status=r['status'], s=t,
                        us_per_iter=1e6 * t / max(r['n_iter'], 1))
        return r

    ref = FE.Material('Hill-reference')
    ref.elasticity(E=200.e3, nu=0.3)
    ref.plasticity(sy=50., rv=[1.2, 1.0, 0.8, 1.0, 1.0, 1.0], sdim=6)
    ml = FE.Material('ML')
    ml.elasticity(CV=ref.CV)
    ml.plasticity(sy=50., sdim=6)
    st, y = ml.create_sig_data(N=300, mat_ref=ref, Nseq=25, Fe=0.1, Ce=0.99)
    X = st / 50.
    rw = run('cfg4_wide', X, y, 2., 1., True)
    rb = run('cfg4_k_smo', X, y, 2., 1., False)
    res['cfg4_identical'] = bool(np.array_equal(rw['alpha'], rb['alpha']) and rw['rho'] == rb['rho'])
    rng = np.random.default_rng(0)   # crossover: random row subsets of the config-4 problem
    for n in (1024, 2048, 4096, 8192):
        sel = np.sort(rng.choice(len(y), n, replace=False))
        run('sub%d_wide' % n, X[sel], y[sel], 2., 1., True)
        run('sub%d_k_smo' % n, X[sel], y[sel], 2., 1., False)

    t = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        lc = hardening_data(FE)
        dd = FE.Data(lc, epl_start=0.0, epl_crit=0.0, epl_max=0.03, depl=1.e-3, wh_data=True)
        mw = FE.Material('ML-hardening')
        mw.from_data(dd.mat_data)
        xt, yt = mw._create_data_for_ms(Ce=0.99, Fe=0.1, Nseq=25, extend=False)[2:]
    mw.scale_seq, mw.scale_wh = float(dd.mat_data['sy_av']), float(dd.mat_data['peeq_max'])
    Xw = mw.create_scaled_input(xt[:, 0:6], xt[:, 6:12], xt[:, 12], xt[:, 13], xt[:, 14])
    res['wh_data_s'] = time.perf_counter() - t
    rw = run('wh_full_wide', Xw, yt, 2., 1.5, True, reps=1)
    cap = min(a.cap, rw['n_iter'])
    rc = run('wh_full_wide_capped', Xw, yt, 2., 1.5, True, max_iter=cap, reps=1)
    rk = run('wh_full_k_smo_capped', Xw, yt, 2., 1.5, False, max_iter=cap, reps=1)
    res['wh_capped_identical'] = bool(np.array_equal(rc['alpha'], rk['alpha']) and rc['rho'] == rk['rho'])
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python3
"""GPU time of the SVR flow rule on the fixture of tests/golden/svr_gradient.npz (305 rows, 12 features, seven
models): the seven-model fit in one plfx_svr_fit_batch call (wall time of the call: upload, k_svr launches, download; one
warm-up call first, then the median of --reps calls), and the fused prediction of the seven models on N points
(k_svr_predict alone, from the library's HIP events on its stream, timing family 0; one warm-up, median of --reps).  The
fixture also holds the wall time of scikit-learn's seven fits on the machine that generated it (another machine, a CPU):
it is printed beside the GPU time as ``fit_seconds_cpu_other_machine``, not as a ratio.  Prints one JSON line.

``--response`` times Material.response_batch under the SVR flow rule instead: the sub-divided rows of
tests/golden/svr_response.npz tiled to N = 1 and N = --n plastic points, k_response_svr alone through the family-0 timers
(one warm-up, median of --reps), and beside it the same points with ``ML_grad = False`` (SVC gradient,
k_response_batch<7>) for scale.  The fixture's ``seconds_per_call`` is the reference's wall time per call on the CPU of
the machine that generated it.

    timeout -k 10 300 python tools/svr_bench.py [--n 100000] [--reps 11] [--response]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def svc_material():
    """the work-hardening material of tests/golden/svc_data_training.npz with the reference's SVC yield function installed"""
    import warnings
    import pylabfea_amd as FE
    w = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_data_training.npz'))
    md = dict(sdim=6, wh_data=True, Name='ML_Hill_hardening', Nlc=int(w['wh_md_Nlc']))
    for k in ('flow_stress', 'plastic_strain', 'elast_const', 'sy_av', 'peeq_max'):
        md[k] = np.array(w['wh_md_' + k]) if w['wh_md_' + k].ndim else float(w['wh_md_' + k])
    m = FE.Material(name='ML_Hill_hardening_C2.0_G1.5', num=2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m.from_data(md)
    Nseq, ss, sw = int(w['wh_Nseq']), float(w['wh_scale_seq']), float(w['wh_scale_wh'])
    X = np.zeros((2 * Nseq * len(w['wh_md_flow_stress']), 15))
    X[:, 0:6] = (w['wh_seq'][:, None, None] * w['wh_md_flow_stress'][None]).reshape(-1, 6) / ss
    X[:, 6:12] = np.tile(w['wh_md_plastic_strain'], (2 * Nseq, 1)) / sw
    m.set_svc(X[w['wh_ns_support']], w['wh_ns_dual'], float(w['wh_ns_intercept']), float(w['wh_gamma']), ss,
              C=float(w['wh_C']), scale_wh=sw)
    return m


def response_leg(a):
    from pylabfea_amd import _lib
    zr = np.load(os.path.join(ROOT, 'tests', 'golden', 'svr_response.npz'))
    CV = np.array(zr['CV'])
    mat = svc_material()
    mat.setup_fgrad_SVM()
    mat.enable_svr_flow()
    rows = np.nonzero((zr['nsteps'] == 49) & (zr['maxit'] == 50))[0]
    rng = np.random.default_rng(0)
    res = dict(rows=int(len(mat._svr['X'])), nsv_svc=int(len(mat.svc['dual'])), reps=a.reps,
               reference_seconds_per_call_cpu_other_machine=float(zr['seconds_per_call']))
    for N in (1, a.n):
        idx = rows[np.arange(N) % len(rows)]
        sig, epl = zr['sig'][idx], zr['epl'][idx]
        deps = zr['deps'][idx] * (1. + 0.02 * rng.uniform(-1., 1., size=(N, 1)))
        kin = np.zeros(N)
        for tag, grad in (('svr', True), ('svc', False)):
            mat.ML_grad = grad
            mat.khard = 0.
            ctx = mat._load(CV)
            assert ctx.svr_flow_info(0)[0] == (len(mat._svr['X']) if grad else 0)
            ctx.timing_enable(True)
            ctx.timing_select([_lib.T_SWEEP])
            out = ctx.response(sig, epl, deps, khard_in=kin, return_khard=True)
            ms = []
            for _ in range(a.reps):
                ctx.timing_reset()
                ctx.response(sig, epl, deps, khard_in=kin, return_khard=True)
                t, launches = ctx.timing_get(_lib.T_SWEEP)
                assert launches == 1
                ms.append(t)
            ctx.timing_enable(False)
            t = float(np.median(ms))
            res['%s_n%d' % (tag, N)] = dict(ms=t, ms_min_max=[min(ms), max(ms)], us_per_point=1e3 * t / N,
                                            subdivided=int(np.sum(out[4] == 49)))
        mat.ML_grad = True
    name, cus, _ = ctx.device_info()
    res.update(device=name, cus=cus)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--response', action='store_true', help='time response_batch under the SVR flow rule (DESIGN §21)')
    a = ap.parse_args()
    if a.reps < 10:
        ap.error('--reps must be at least 10 (median of >= 10 calls)')
    if a.response:
        return response_leg(a)
    from pylabfea_amd import _lib
    from pylabfea_amd.material import _ctx
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'svr_gradient.npz'))
    X, Y = z['x_sc'], z['y_sc']
    C, g, eps, tol = float(z['C']), float(z['gamma']), float(z['epsilon']), float(z['tol'])
    ctx = _ctx()
    name, cus, _ = ctx.device_info()
    rows = np.arange(len(X))

    def fit():
        return ctx.svr_fit_batch(X, [rows] * 7, [Y[:, m] for m in range(7)], C, g, epsilon=eps, tol=tol)

    fits = fit()
    assert [r['n_iter'] for r in fits] == [int(z['ns%d_n_iter' % m]) for m in range(7)]
    t_fit = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fit()
        t_fit.append(time.perf_counter() - t0)
    coef = np.ascontiguousarray(np.stack([r['coef'] for r in fits], axis=1))
    icpt = np.array([-r['rho'] for r in fits])
    rng = np.random.default_rng(0)
    Q = X[rng.integers(len(X), size=a.n)] + 0.05 * rng.normal(size=(a.n, X.shape[1]))
    ctx.timing_enable(True)
    ctx.timing_select([_lib.T_SWEEP])
    ctx.svr_predict_multi(X, coef, icpt, g, Q)
    ms = []
    for _ in range(a.reps):
        ctx.timing_reset()
        ctx.svr_predict_multi(X, coef, icpt, g, Q)
        t, launches = ctx.timing_get(_lib.T_SWEEP)
        assert launches == 1
        ms.append(t)
    ctx.timing_enable(False)
    t_p = float(np.median(ms))
    res = dict(device=name, cus=cus, rows=int(len(X)), nfeat=int(X.shape[1]), models=7, reps=a.reps,
               n_iter=[r['n_iter'] for r in fits], fit_ms=1e3 * float(np.median(t_fit)),
               fit_ms_min_max=[1e3 * min(t_fit), 1e3 * max(t_fit)],
               fit_seconds_cpu_other_machine=dict(shrinking=float(z['fit_seconds_cpu']),
                                                  without=float(z['fit_seconds_cpu_ns'])),
               n=a.n, predict_ms=t_p, predict_ms_min_max=[min(ms), max(ms)], predict_ns_per_point=1e6 * t_p / a.n,
               predict_ns_per_pair=1e6 * t_p / a.n / len(X))
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())

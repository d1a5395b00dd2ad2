#!/usr/bin/env python3
"""GPU time of the SVR flow rule on the fixture of tests/golden/svr_gradient.npz (305 rows, 12 features, seven
models): the seven-model fit in one plfx_svr_fit_batch call (wall time of the call: upload, k_svr launches, download; one
warm-up call first, then the median of --reps calls), and the fused prediction of the seven models on N points
(k_svr_predict alone, from the library's HIP events on its stream, timing family 0; one warm-up, median of --reps).  The
fixture also holds the wall time of scikit-learn's seven fits on the machine that generated it (another machine, a CPU):
it is printed beside the GPU time as ``fit_seconds_cpu_other_machine``, not as a ratio.  Prints one JSON line.

    timeout -k 10 300 python tools/svr_bench.py [--n 100000] [--reps 11]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=11)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error('--reps must be at least 10 (median of >= 10 calls)')
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

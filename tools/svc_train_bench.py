#!/usr/bin/env python3
"""GPU time of SVC training (plfx_svc_fit_batch): one config-4 fit (Hill reference of examples/train_hill.py, Nlc = 300,
Nseq = 25: 15 000 x 6 features, C = 2, gamma = 1) and the default grid search of setup_yf_SVM_6D extended by C = 15,
gamma = 4 (5 x 7 = 35 candidates x 5 folds = 175 SMO problems in one batched call, plus scoring).  Where scikit-learn is
installed, the same fit and grid search with it on --threads threads for comparison.  Prints one JSON line.

    python tools/svc_train_bench.py [--reps 3] [--threads 16] [--no-grid]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--no-grid', action='store_true')
    a = ap.parse_args()
    import pylabfea_amd as FE
    from pylabfea_amd.material import _ctx, svc_grid_search
    from pylabfea_amd.training import param_grid, stratified_folds
    ref = FE.Material('Hill-reference')
    ref.elasticity(E=200.e3, nu=0.3)
    ref.plasticity(sy=50., rv=[1.2, 1.0, 0.8, 1.0, 1.0, 1.0], sdim=6)
    ml = FE.Material('ML')
    ml.elasticity(CV=ref.CV)
    ml.plasticity(sy=50., sdim=6)
    t = time.perf_counter()
    st, y = ml.create_sig_data(N=300, mat_ref=ref, Nseq=25, Fe=0.1, Ce=0.99)
    t_data = time.perf_counter() - t
    X = st / 50.
    ctx = _ctx()
    res = {'n': len(y), 'd': X.shape[1], 'create_sig_data_s': t_data}
    ctx.svc_fit_batch(X, y, [np.arange(len(y))], 2., 1.)   # warm-up (module load, allocations)
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter()
        r = ctx.svc_fit_batch(X, y, [np.arange(len(y))], 2., 1.)[0]
        ts.append(time.perf_counter() - t)
    res.update(fit_s=min(ts), fit_s_all=ts, fit_iters=r['n_iter'], fit_nsv=int(np.sum(r['alpha'] > 0)),
               us_per_iter=1e6 * min(ts) / r['n_iter'])
    cands = param_grid([1, 2, 4, 10, 15], [0.5, 1, 1.5, 2, 2.5, 3, 4])
    folds = stratified_folds(y)
    if not a.no_grid:
        t = time.perf_counter()
        g = svc_grid_search(ctx, X, y, cands, folds)
        res.update(grid_s=time.perf_counter() - t, grid_problems=len(cands) * len(folds),
                   grid_iters_max=int(g['n_iter'].max()), grid_iters_sum=int(g['n_iter'].sum()), grid_best=g['best_params_'])
    try:
        from sklearn import svm
        from sklearn.model_selection import GridSearchCV, StratifiedKFold
    except ImportError:
        res['sklearn'] = None
    else:
        t = time.perf_counter()
        s = svm.SVC(C=2., gamma=1.).fit(X, y)
        res.update(sklearn_fit_s=time.perf_counter() - t, sklearn_fit_iters=int(s.n_iter_[0]))
        if not a.no_grid:
            t = time.perf_counter()
            gs = GridSearchCV(svm.SVC(), {'C': [1, 2, 4, 10, 15], 'gamma': [0.5, 1, 1.5, 2, 2.5, 3, 4]},
                              cv=StratifiedKFold(5), n_jobs=a.threads).fit(X, y)
            res.update(sklearn_grid_s=time.perf_counter() - t, sklearn_threads=a.threads, sklearn_grid_best=gs.best_params_)
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())

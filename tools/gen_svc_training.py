#!/usr/bin/env python3
"""Fixture generator for SVC training -- TEST INFRASTRUCTURE, not product code.

Runs the unmodified reference (pyLabFEA v4.4.2) and scikit-learn on the build box and writes
``tests/golden/svc_training.npz``.  No GPU test reads the reference or imports scikit-learn; they read this file.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_svc_training.py

Per case (prefix ``<case>_``): the reference's training data in compact form -- the yield-locus stresses ``sdata`` that
create_sig_data finds with fsolve and the scale factors ``seq`` it applies, so that the training stresses are exactly
``seq[i] * sdata`` block by block and the 6-d features exactly those over ``sy`` (checked here bit for bit); the features
of the sdim = 3 case (polar angles, periodic copies) are stored as they are.  Then scikit-learn fits with shrinking=True
(the reference's) and shrinking=False (prefixes ``s_`` / ``ns_``: support_, dual_coef_, intercept_, n_iter_, dual
objective), and ``calib``: the largest decision difference between those two fits on the training points plus 10 000
perturbed points (the calibration of the looser bars); 500 of the perturbed points (``probe``) and the non-shrinking
decision values on every 10th training point followed by them (``probe_dec_ns``).  For the literal assertions of the
reference's test_ml_* tests: the values the reference reaches with the shrinking=False SVC installed (``<case>_ns_lit``)
and whether each assertion holds (``<case>_ns_lit_ok``).
A small grid-search case (``gs_``): fold indices, cv_results_['mean_test_score'], best_params_.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'svc_training.npz')
os.environ.setdefault('MPLBACKEND', 'Agg')

import pylabfea as FE  # noqa: E402  (the reference)
import pylabfea.material as FEM  # noqa: E402
from sklearn import svm  # noqa: E402
from sklearn.model_selection import GridSearchCV, StratifiedKFold  # noqa: E402

assert FE.__version__ == '4.4.2'
E, NU = 200.e3, 0.3


def hill_cfg4():
    m = FE.Material(name='Hill-reference')   # config 4 / examples/train_hill.py
    m.elasticity(E=E, nu=NU)
    m.plasticity(sy=50., rv=[1.2, 1.0, 0.8, 1.0, 1.0, 1.0], sdim=6)
    return m


def hill_shear():
    m = FE.Material(name='Hill-shear')
    m.elasticity(E=E, nu=NU)
    m.plasticity(sy=150., hill=[1.4, 1., 0.7, 1.2, .8, 1.], sdim=6)
    return m


def j2_train():
    m = FE.Material(name='J2-reference')
    m.elasticity(E=200000., nu=0.3)
    m.plasticity(sy=60., sdim=6)
    return m


def hill3():
    m = FE.Material(name='anisotropic Hill')
    m.elasticity(E=E, nu=NU)
    m.plasticity(sy=150., hill=[0.7, 1., 1.4], drucker=0., khard=0., sdim=3)
    return m


# name: (reference material, C, gamma, Nlc, Nseq, Fe, Ce, extend)
CASES = {
    'cfg4': (hill_cfg4, 2., 1., 300, 25, 0.1, 0.99, False),
    'shear': (hill_shear, 2., 0.5, 300, 4, 0.7, 0.95, False),
    'j2train': (j2_train, 15., 2.5, 150, 25, 0.1, 0.99, False),
    'hill3': (hill3, 10., 4., 36, 2, 0.1, 0.99, True),
}


def capture_fit(mat_fn, C, gamma, Nlc, Nseq, Fe, Ce, extend, shrinking):
    """run the reference's own training with SVC(shrinking=...) and capture the data handed to SVC.fit"""
    seen = {}
    orig = svm.SVC

    class SVC(orig):
        def __init__(self, **kw):
            kw.setdefault('shrinking', shrinking)
            super().__init__(**kw)

        def fit(self, X, y, sample_weight=None):
            seen['X'], seen['y'] = np.array(X), np.array(y)
            return super().fit(X, y, sample_weight)
    FEM.svm.SVC = SVC
    fsolve = FEM.fsolve

    def fsolve_rec(f, x0, args=(), **kw):   # the yield-locus stresses of create_sig_data (material.py:2020-2021)
        x1 = fsolve(f, x0, args=args, **kw)
        seen['sdata'] = args[0] * x1[:, None]
        return x1
    FEM.fsolve = fsolve_rec
    try:
        mat_ref = mat_fn()
        ml = FE.Material(name='ML')
        if mat_ref.sdim == 3:
            ml.elasticity(E=E, nu=NU)
            ml.plasticity(sy=mat_ref.sy, sdim=3)
            st, yt = ml.create_sig_data(Nlc, mat_ref=mat_ref, extend=extend)
            ml.setup_yf_SVM_3D(st, yt, C=C, gamma=gamma, fs=0.3)
        else:
            ml.dev_only = False
            ml.train_SVC(C=C, gamma=gamma, mat_ref=mat_ref, Nlc=Nlc, Nseq=Nseq, Fe=Fe, Ce=Ce, extend=extend)
            st, yt = ml.create_sig_data(N=Nlc, mat_ref=mat_ref, Nseq=Nseq, Fe=Fe, Ce=Ce, extend=extend)
    finally:
        FEM.svm.SVC = orig
        FEM.fsolve = fsolve
    return ml, st, yt, seen['X'], seen['y'], seen['sdata']


def ref_seq(Nseq, Fe, Ce, extend):
    """the scale factors of create_sig_data (material.py:2037-2048)"""
    if Nseq == 1:
        mid = 0.5 * (Fe + Ce)
        seq = np.array([mid, 2. - mid])
    else:
        seq = np.append(np.linspace(Fe, Ce, Nseq), np.linspace(2. - Ce, 2. - Fe, Nseq))
    return np.append(seq, np.array([2.4, 3., 4., 5.])) if extend else seq


def compact(name, st, yt, X, y, sdata, sdim, sy, Nseq, Fe, Ce, extend):
    """training data as (sdata, seq); asserts that the stresses, labels and 6-d features follow from them exactly"""
    seq = ref_seq(Nseq, Fe, Ce, extend)
    sd = np.ascontiguousarray(sdata[:, 0:sdim])
    assert np.array_equal(st, (seq[:, None, None] * sd[None, :, :]).reshape(-1, sdim)), name
    assert np.array_equal(yt, np.repeat(np.where(np.arange(len(seq)) < Nseq, -1., 1.), len(sd))), name
    out = {name + '_sdata': sd, name + '_seq': seq}
    if sdim == 6:
        assert np.array_equal(X, st / sy) and np.array_equal(y, yt), name
    else:
        out.update({name + '_X': X, name + '_y': y})
    return out


def dual_obj(s, X, y):
    K = np.exp(-s._gamma * np.sum((s.support_vectors_[:, None, :] - s.support_vectors_[None, :, :]) ** 2, axis=2))
    a = s.dual_coef_[0]
    return 0.5 * a @ K @ a - np.sum(np.abs(a))


def literal(name, ml):
    """the reference test's literal values and assertions with this ML material (None: no literal test)"""
    if name == 'shear':
        ml.dev_only = False
        fem = FE.Model(dim=2, planestress=True)
        fem.geom([2], LY=2.)
        fem.assign([ml])
        fem.bcbot(0., bctype='disp', bcdir='y')
        fem.bcbot(0., bctype='disp', bcdir='x')
        fem.bcleft(0., bctype='force')
        fem.bcright(0., bctype='force')
        fem.bctop(0.006 * fem.leny, bctype='disp', bcdir='x')
        fem.bctop(0., bctype='disp', bcdir='y')
        fem.mesh(NX=6, NY=3)
        fem.solve()
        fem.calc_global()
        v = [fem.glob['sig'][5], fem.element[3].epl[5], fem.element[3].sig[1]]
        ref, tol = [77.53778881971623, 0.003942707316047761, 43.9060552472426], [6E-4, 1E-7, 5E-3]
    elif name == 'hill3':
        ml.calc_properties(eps=0.01, sigeps=True, min_step=12)
        v = [ml.propJ2['stx']['ys'], ml.propJ2['sty']['seq'][-1], ml.propJ2['ect']['peeq'][-1]]
        ref, tol = [149.62302821433968, 157.25971534002542, 0.00855380746615942], [1E-5, 1E-5, 1E-7]
    elif name == 'j2train':
        ml.calc_properties(verb=False, eps=0.01, sigeps=True)
        v = [ml.propJ2['et2']['ys'], ml.propJ2['ect']['peeq'][-1]]
        ref, tol = [60.5, 0.00898749114723422], [1.0, 2E-6]
    else:
        return None
    v = np.array(v, dtype=float)
    return v, np.abs(v - np.array(ref)) < np.array(tol), np.array(ref), np.array(tol)


def main():
    out = {}
    rng = np.random.default_rng(7)
    for name, (fn, C, gamma, Nlc, Nseq, Fe, Ce, extend) in CASES.items():
        t0 = time.time()
        fits = {}
        for tag, shr in (('s', True), ('ns', False)):
            ml, st, yt, X, y, sdata = capture_fit(fn, C, gamma, Nlc, Nseq, Fe, Ce, extend, shr)
            s = ml.svm_yf
            fits[tag] = (ml, s)
            out.update({'%s_%s_support' % (name, tag): s.support_.astype(np.int32),
                        '%s_%s_dual' % (name, tag): s.dual_coef_[0],
                        '%s_%s_intercept' % (name, tag): float(s.intercept_[0]),
                        '%s_%s_n_iter' % (name, tag): int(s.n_iter_[0]),
                        '%s_%s_obj' % (name, tag): dual_obj(s, X, y)})
        out.update(compact(name, st, yt, X, y, sdata, fn().sdim, fn().sy, Nseq, Fe, Ce, extend))
        out.update({name + '_C': C,
                    name + '_gamma': gamma, name + '_Nlc': Nlc, name + '_Nseq': Nseq, name + '_Fe': Fe, name + '_Ce': Ce,
                    name + '_extend': extend, name + '_sdim': fn().sdim, name + '_sy': fn().sy})
        P = np.concatenate([X, X[rng.integers(len(X), size=10000)] + 0.05 * rng.normal(size=(10000, X.shape[1]))])
        d1, d2 = fits['s'][1].decision_function(P), fits['ns'][1].decision_function(P)
        out[name + '_calib'] = float(np.max(np.abs(d1 - d2)))
        out[name + '_calib_flips'] = int(np.sum(np.sign(d1) != np.sign(d2)))
        out[name + '_probe'] = P[len(X):len(X) + 500]
        out[name + '_probe_dec_ns'] = np.concatenate([d2[:len(X):10], d2[len(X):len(X) + 500]])
        lit = literal(name, fits['ns'][0])
        if lit is not None:
            out[name + '_ns_lit'], out[name + '_ns_lit_ok'], out[name + '_lit_ref'], out[name + '_lit_tol'] = lit
        print('%s: n=%d nSV %d / %d, n_iter %d / %d, calib %.2e (%d flips), %s  [%.1f s]' % (
            name, len(X), len(out[name + '_s_support']), len(out[name + '_ns_support']), out[name + '_s_n_iter'],
            out[name + '_ns_n_iter'], out[name + '_calib'], out[name + '_calib_flips'],
            None if lit is None else list(lit[1]), time.time() - t0))
    # grid search: small Hill case, the reference's default grid of setup_yf_SVM_6D (C=2, gamma=1 already in it)
    ml, st, yt, X, y, sdata = capture_fit(hill_cfg4, 2., 1., 60, 10, 0.1, 0.99, False, True)
    out.update(compact('gs', st, yt, X, y, sdata, 6, 50., 10, 0.1, 0.99, False))
    grid = GridSearchCV(svm.SVC(), {'C': [1, 2, 4, 10], 'gamma': [0.5, 1, 1.5, 2, 2.5, 3]}, cv=5, n_jobs=1)
    grid.fit(X, y)
    folds = [te for _, te in StratifiedKFold(5).split(X, y)]
    out.update({'gs_sy': 50., 'gs_Nseq': 10, 'gs_cvals': np.array([1, 2, 4, 10], dtype=float),
                'gs_gvals': np.array([0.5, 1, 1.5, 2, 2.5, 3]),
                'gs_mean_test_score': grid.cv_results_['mean_test_score'],
                'gs_best_C': float(grid.best_params_['C']), 'gs_best_gamma': float(grid.best_params_['gamma']),
                'gs_fold_of': np.concatenate([np.full(len(f), k) for k, f in enumerate(folds)])[np.argsort(np.concatenate(folds))]})
    print('grid search: best', grid.best_params_, 'scores', np.round(grid.cv_results_['mean_test_score'], 4))
    # load_cases of the reference for the CPU test
    out['lc_30_60'] = FE.load_cases(30, 60)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, '%.0f kB' % (os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python3
"""Fixture generator for the SVR flow rule (Material.setup_fgrad_SVM, the ML_grad branch of calc_fgrad) -- TEST
INFRASTRUCTURE, not product code.

Runs the unmodified reference (pyLabFEA v4.4.2) and scikit-learn on the build box and writes
``tests/golden/svr_gradient.npz``.  No test reads the reference or imports scikit-learn; they read this file.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_svr_gradient.py

The data is the reduced work-hardening case ``wh_`` of tools/gen_svc_data_training.py (Nlc 40); its Data.mat_data is
already in tests/golden/svc_data_training.npz (``wh_md_*``, checked equal here) and is not stored again.  The reference
material is trained as there (train_SVC, C 2, gamma 1.5, without shrinking: that yield function is ``wh_ns_*`` of that
file) and then setup_fgrad_SVM is called twice: as the reference has it (SVR with shrinking, ``s_``) and with
shrinking=False (``ns_``), which is what the device solver follows step for step.

Keys:
  X_gt (ndata, 12), y_gt (ndata, 6), y_kh (ndata,)      features and targets as setup_fgrad_SVM builds them
  feat_/grad_/khard_ + mean, scale                      the three StandardScalers
  x_sc, y_sc (ndata, 7)                                 what the seven SVR.fit calls were handed (column 6: hardening)
  C, gamma, epsilon, tol
  ns<m>_ / s<m>_ + support, dual, intercept, n_iter     the fits of model m = 0 .. 6 (6: svm_khard)
  calib_m (7,)      largest |predict_s - predict_ns| on the training rows plus 10 000 perturbed points (scaled units)
  p_sig, p_epl (50, 6), p_fgrad (50, 6), p_khard (50,)  reference calc_fgrad (s_ fits) point by point, with khard
  b_fgrad (5, 6), b_khard                               one (5, 6) call on the first five pairs
  e_idx (5,), e_deps (5, 6), e_yfun, e_pdot (5, 6), e_ctan (5, 6, 6), e_khard_pdot, e_khard_ctan      epl_dot and C_tan
  none_exc          type name of the exception calc_fgrad(sig) raises without epl ('' when it raises none), none_fgrad
  fit_seconds_cpu   wall time of the seven scikit-learn fits (shrinking=True) on the machine that ran this generator
"""
import contextlib
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden', 'svr_gradient.npz')
os.environ.setdefault('MPLBACKEND', 'Agg')
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import pylabfea as FE  # noqa: E402  (the reference)
import pylabfea.material as FEM  # noqa: E402
from sklearn import svm  # noqa: E402

from gen_svc_data_training import quiet, sklearn_svc, wh_lc_data  # noqa: E402

assert FE.__version__ == '4.4.2'


@contextlib.contextmanager
def sklearn_svr(shrinking, seen):
    """the reference's SVR with shrinking forced, recording the data handed to fit and the time spent in it"""
    orig = svm.SVR

    class SVR(orig):
        def __init__(self, **kw):
            kw['shrinking'] = shrinking
            super().__init__(**kw)

        def fit(self, X, y, sample_weight=None):
            seen.setdefault('X', []).append(np.array(X))
            seen.setdefault('y', []).append(np.array(y))
            t0 = time.perf_counter()
            r = super().fit(X, y, sample_weight)
            seen['t'] = seen.get('t', 0.) + time.perf_counter() - t0
            return r
    osc = FEM.StandardScaler

    class Scaler(osc):
        def fit(self, X, y=None, sample_weight=None):
            seen.setdefault('fit', []).append(np.array(X))
            return super().fit(X, y, sample_weight)
    FEM.svm.SVR, FEM.StandardScaler = SVR, Scaler
    try:
        yield
    finally:
        FEM.svm.SVR, FEM.StandardScaler = orig, osc


def models(m):
    return [m.svm_grad0, m.svm_grad1, m.svm_grad2, m.svm_grad3, m.svm_grad4, m.svm_grad5, m.svm_khard]


def main():
    rng = np.random.default_rng(23)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_data_training.npz'))
    epl_max, depl, Nseq, C, gamma = 0.03, 3.e-3, 8, 2.0, 1.5
    lc = wh_lc_data(epl_max=epl_max, depl=depl)
    with quiet():
        dd = FE.Data(lc, mat_name='ML_Hill_hardening', epl_start=0.0, epl_crit=0.0, epl_max=epl_max, depl=depl,
                     wh_data=True)
    assert np.array_equal(dd.mat_data['flow_stress'], z['wh_md_flow_stress'])
    assert np.array_equal(dd.mat_data['plastic_strain'], z['wh_md_plastic_strain'])
    mats, seen = {}, {}
    for tag, shr in (('ns', False), ('s', True)):
        seen[tag] = {}
        with sklearn_svc(False, {}), sklearn_svr(shr, seen[tag]), quiet(), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m = FE.Material(name='ML_Hill_hardening_C2.0_G1.5', num=2)
            m.from_data(dd.mat_data)
            m.train_SVC(C=C, gamma=gamma, Ce=0.99, Fe=0.1, Nseq=Nseq, gridsearch=False)
            m.setup_fgrad_SVM()
        mats[tag] = m
    ms, mns = mats['s'], mats['ns']
    assert np.array_equal(ms.svm_yf.support_, z['wh_ns_support']) and np.array_equal(ms.svm_yf.dual_coef_[0], z['wh_ns_dual'])
    assert ms.ML_grad and ms.C_yf == C and ms.gam_yf == gamma
    x_sc = seen['s']['X'][0]
    assert all(np.array_equal(x_sc, x) for x in seen['s']['X'] + seen['ns']['X'])
    y_sc = np.stack(seen['s']['y'], axis=1)
    assert np.array_equal(y_sc, np.stack(seen['ns']['y'], axis=1))
    sig, eps = np.array(dd.mat_data['flow_stress']), np.array(dd.mat_data['plastic_strain'])
    X_gt = np.concatenate((sig, eps), axis=1)
    assert np.array_equal(ms.sc_feat.transform(X_gt), x_sc)
    assert np.array_equal(seen['s']['fit'][0], X_gt)
    y_gt, y_kh = seen['s']['fit'][1], seen['s']['fit'][2][:, 0]
    assert np.array_equal(ms.sc_grad.transform(y_gt), y_sc[:, :6])
    out = dict(X_gt=X_gt, y_gt=y_gt, y_kh=y_kh, x_sc=x_sc, y_sc=y_sc, C=C, gamma=gamma, epsilon=0.01, tol=1e-4,
               fit_seconds_cpu=float(seen['s']['t']), fit_seconds_cpu_ns=float(seen['ns']['t']))
    for pre, sc in (('feat_', ms.sc_feat), ('grad_', ms.sc_grad), ('khard_', ms.sc_khard)):
        out[pre + 'mean'], out[pre + 'scale'] = np.array(sc.mean_), np.array(sc.scale_)
    P = np.concatenate([x_sc, x_sc[rng.integers(len(x_sc), size=10000)] + 0.05 * rng.normal(size=(10000, 12))])
    cal = np.zeros(7)
    for k, (a, b) in enumerate(zip(models(ms), models(mns))):
        for pre, s in (('s%d_' % k, a), ('ns%d_' % k, b)):
            assert s.shrinking == (pre[0] == 's') and s.epsilon == 0.01 and s.tol == 1e-4 and s.C == C and s._gamma == gamma
            out.update({pre + 'support': s.support_.astype(np.int32), pre + 'dual': s.dual_coef_[0],
                        pre + 'intercept': float(s.intercept_[0]), pre + 'n_iter': int(np.ravel(s.n_iter_)[0])})
        cal[k] = np.max(np.abs(a.predict(P) - b.predict(P)))
    out['calib_m'] = cal
    # ~50 (sig, epl) pairs: 25 rows of the data, 25 perturbed
    pick = rng.choice(len(sig), 25, replace=False)
    p_sig = np.concatenate([sig[pick], sig[pick] * rng.uniform(0.9, 1.1, size=(25, 1)) + 0.5 * rng.normal(size=(25, 6))])
    p_epl = np.concatenate([eps[pick], eps[pick] * rng.uniform(0.8, 1.2, size=(25, 1)) + 2e-4 * rng.normal(size=(25, 6))])
    fg, kh = np.zeros((50, 6)), np.zeros(50)
    for i in range(50):
        fg[i] = ms.calc_fgrad(p_sig[i], epl=p_epl[i])
        kh[i] = np.ravel(ms.khard)[0]
    assert ms.msg['gradient'] == 'SVR gradient'
    out.update(p_sig=p_sig, p_epl=p_epl, p_fgrad=fg, p_khard=kh)
    out['b_fgrad'] = ms.calc_fgrad(p_sig[:5], epl=p_epl[:5])
    out['b_khard'] = float(np.ravel(ms.khard)[0])
    out['khard_shape'] = np.array(np.shape(ms.khard), dtype=np.int64)
    # epl_dot and C_tan on five data rows, strain increments that leave the yield locus
    CV = np.array(ms.CV)
    e_idx = np.arange(0, 25, 5)
    e_deps = np.zeros((5, 6))
    pd, ct, yf, k1, k2 = np.zeros((5, 6)), np.zeros((5, 6, 6)), np.zeros(5), np.zeros(5), np.zeros(5)
    for n, i in enumerate(e_idx):
        d = np.linalg.solve(CV, p_sig[i])
        noise = 1e-5 * rng.normal(size=6)
        for f in (0.1, 0.2, 0.4, 0.8):   # the smallest of these steps along the stress that ends outside the yield locus
            e_deps[n] = f * d + noise
            yf[n] = ms.calc_yf(p_sig[i] + CV @ e_deps[n], epl=p_epl[i])
            if yf[n] > 1.:
                break
        assert yf[n] > 1., yf[n]
        pd[n] = ms.epl_dot(p_sig[i], p_epl[i], CV, e_deps[n])
        k1[n] = np.ravel(ms.khard)[0]
        ct[n] = ms.C_tan(p_sig[i], CV, epl=p_epl[i])
        k2[n] = np.ravel(ms.khard)[0]
    out.update(e_idx=e_idx, e_deps=e_deps, e_yfun=yf, e_pdot=pd, e_ctan=ct, e_khard_pdot=k1, e_khard_ctan=k2, CV=CV)
    try:
        out['none_fgrad'] = ms.calc_fgrad(p_sig[0])
        out['none_exc'] = ''
    except Exception as e:   # noqa: BLE001  (the type is what is recorded)
        out['none_exc'] = type(e).__name__
        out['none_fgrad'] = np.zeros(0)
    np.savez_compressed(OUT, **out)
    print('ndata %d; n_iter ns %s / s %s; nSV ns %s' % (len(sig), [out['ns%d_n_iter' % k] for k in range(7)],
          [out['s%d_n_iter' % k] for k in range(7)], [len(out['ns%d_support' % k]) for k in range(7)]))
    print('calib_m', cal, 'scales', out['grad_scale'], out['khard_scale'])
    print('epl=None:', out['none_exc'] or 'no exception', '; seven fits %.3f s (shrinking) / %.3f s (without)' % (
        seen['s']['t'], seen['ns']['t']))
    print('wrote', OUT, '%.0f kB' % (os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    sys.exit(main())

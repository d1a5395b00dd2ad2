#!/usr/bin/env python3
"""Fixture generator for Material.load_path on a work-hardening SVC (check 5) -- TEST INFRASTRUCTURE, not
product code.

Runs the unmodified reference (pyLabFEA v4.4.2) and scikit-learn on the build box and writes
``tests/golden/load_path_wh.npz``.  No test reads the reference or imports scikit-learn; they read this file.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_load_path_wh.py

The material is the one of ``oracle/gen_golden.py::train_hardening`` -- the data set and the fit behind
tests/golden/svc_workhard.npz --, trained again here and checked to have the fixture's tables.  Six strain-controlled chains of
12 consecutive calls ``response(sig, epl, deps, CV, maxit)`` with ``epl += depl`` in between, each on ONE material object, so
the hardening modulus is carried by the reference's own attribute ``khard`` from call to call (set to ``khard0`` = 0 before
the first).  With the SVC gradient that attribute stays a NumPy scalar (material.py:811-814), so the in-place marches of
``ML_full_yf`` work on values, not on one shared array as under the SVR flow rule (§21).  Each chain runs twice as a whole:
with scikit-learn's ``decision_function``, and with it replaced by a plain FP64 NumPy sum over the support vectors in row
order.  The difference of the two runs is the reference's own noise floor, ``calib``; a chain is *unstable* from the first
step at which the two runs differ in ``nsteps``.

Keys (C = 6 chains, K = 12 steps):
  CV (6, 6); names (C,); dload (C, K, 6); sig0, epl0 (C, 6); khard0 (C,); maxit (C,)         the inputs
  sig, epl (C, K, 6); fy, khard (C, K); nsteps (C, K); ct (C, 6, 6) after the last step       reference results (first run)
  nsteps2 (C, K)                                       sub-step counts of the second run
  calib_sig, calib_epl, calib_fy, calib_khard (C, K)   largest |run 1 - run 2| per chain, step and output
  first (C,)                                           first step at which the runs differ in nsteps (K: never)
  seconds_per_call                                     mean wall time of a reference call on the machine that ran this
"""
import contextlib
import copy
import io
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden', 'load_path_wh.npz')
os.environ.setdefault('MPLBACKEND', 'Agg')
sys.path.insert(0, ROOT)

from oracle.gen_golden import train_hardening  # noqa: E402  (imports the reference)

K = 12
# name, direction of the strain step (Voigt xx, yy, zz, yz, xz, xy) in units of 0.2 sy / E, steps 8-11 reversed, epl0, maxit
CHAINS = (
    ('uniaxial strain x', (2., 0., 0., 0., 0., 0.), False, None, 50),
    ('biaxial', (1.5, 1.5, 0., 0., 0., 0.), False, None, 50),
    ('shear xy', (0., 0., 0., 0., 0., 2.), False, None, 50),
    ('steps 8-11 reversed', (1.6, -0.8, -0.3, 0., 0., 0.7), True, None, 50),
    ('from a non-zero epl0', (-0.6, 2.2, -0.4, 0.3, 0., 0.), False, 0.004 * np.array([-0.5, 1., -0.5, 0., 0., 0.]), 50),
    ('maxit = 5', (2.2, 0.3, -0.2, 0., 0.3, 0.), False, None, 5),
)


def material():
    """the reference material behind svc_workhard.npz, trained again and checked against the fixture's tables"""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_workhard.npz'))
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter('ignore')
        ml, _ = train_hardening()
    assert np.array_equal(ml.svm_yf.support_vectors_, z['par_sv']) and np.array_equal(ml.svm_yf.dual_coef_[0], z['par_dual'])
    assert float(ml.svm_yf.intercept_[0]) == float(z['par_intercept']) and float(ml.gam_yf) == float(z['par_gamma'])
    assert float(ml.scale_seq) == float(z['par_scale_seq']) and float(ml.scale_wh) == float(z['par_scale_wh'])
    # the elastic constants come out of the data set through a matrix inverse and agree with the fixture's to rounding only:
    # the chains run on the fixture's, which is what the device is given
    assert np.max(np.abs(np.asarray(ml.CV) - z['par_CV'])) <= 1e-14 * np.max(np.abs(z['par_CV']))
    ml.CV = np.array(z['par_CV'], dtype=float)
    assert float(ml.sy) == float(z['par_sy']), (float(ml.sy), float(z['par_sy']))
    return ml


def plain_decision(m):
    """replace decision_function of the SVC by the FP64 sum over the support vectors in row order (np.cumsum adds in sequence)"""
    sv, dc = np.array(m.svm_yf.support_vectors_), np.array(m.svm_yf.dual_coef_[0])
    g, b = float(m.gam_yf), float(m.svm_yf.intercept_[0])

    def f(x):
        x = np.atleast_2d(np.asarray(x, dtype=float))
        out = np.empty(len(x))
        for i, xi in enumerate(x):
            ss = np.zeros(len(sv))
            for c in range(sv.shape[1]):   # the distance feature by feature
                d = xi[c] - sv[:, c]
                ss = ss + d * d
            out[i] = np.cumsum(dc * np.exp(-g * ss))[-1] + b
        return out
    m.svm_yf.decision_function = f


def run(ml, CV, dload, epl0, maxit, plain):
    m = copy.deepcopy(ml)   # one object per chain: its attribute khard carries the modulus
    if plain:
        plain_decision(m)
    m.khard = 0.
    sig, epl = np.zeros(6), np.array(epl0, dtype=float)
    out = dict(sig=np.empty((K, 6)), epl=np.empty((K, 6)), fy=np.empty(K), khard=np.empty(K), nsteps=np.empty(K, dtype=np.int32))
    dt = []
    for k in range(K):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t0 = time.perf_counter()
            fy, so, dp, ct = m.response(sig, epl, dload[k], CV, maxit=maxit)
            dt.append(time.perf_counter() - t0)
        sig, epl = np.array(so, dtype=float), epl + np.array(dp, dtype=float)
        out['sig'][k], out['epl'][k], out['fy'][k] = sig, epl, float(np.ravel(fy)[0])
        out['khard'][k], out['nsteps'][k] = float(np.ravel(m.khard)[0]), int(m.msg['nsteps'])
        assert np.ndim(m.khard) == 0, 'khard left as an array: the chain would take the aliased path of ML_full_yf'
    out['ct'] = np.array(ct, dtype=float)
    return out, dt


def main():
    ml = material()
    CV = np.array(ml.CV, dtype=float)
    h = 0.2 * float(ml.sy) / CV[0, 0]
    C = len(CHAINS)
    rec = dict(CV=CV, names=np.array([c[0] for c in CHAINS]), dload=np.empty((C, K, 6)), sig0=np.zeros((C, 6)), epl0=np.zeros((C, 6)),
               khard0=np.zeros(C), maxit=np.array([c[4] for c in CHAINS], dtype=np.int32), sig=np.empty((C, K, 6)),
               epl=np.empty((C, K, 6)), fy=np.empty((C, K)), khard=np.empty((C, K)), nsteps=np.empty((C, K), dtype=np.int32),
               nsteps2=np.empty((C, K), dtype=np.int32), ct=np.empty((C, 6, 6)), first=np.empty(C, dtype=np.int32))
    for w in ('sig', 'epl', 'fy', 'khard'):
        rec['calib_' + w] = np.empty((C, K))
    times = []
    for i, (name, d, rev, e0, maxit) in enumerate(CHAINS):
        sign = np.where((np.arange(K) >= 8) & rev, -1., 1.)
        rec['dload'][i] = h * sign[:, None] * np.array(d)[None, :]
        if e0 is not None:
            rec['epl0'][i] = e0
        A, dt = run(ml, CV, rec['dload'][i], rec['epl0'][i], maxit, False)
        B, _ = run(ml, CV, rec['dload'][i], rec['epl0'][i], maxit, True)
        times += dt
        for w in ('sig', 'epl', 'fy', 'khard', 'nsteps', 'ct'):
            rec[w][i] = A[w]
        rec['nsteps2'][i] = B['nsteps']
        for w in ('sig', 'epl', 'fy', 'khard'):
            rec['calib_' + w][i] = np.abs(A[w] - B[w]).reshape(K, -1).max(axis=1)
        differ = A['nsteps'] != B['nsteps']
        rec['first'][i] = int(np.argmax(differ)) if differ.any() else K
        print('%-22s nsteps %s  khard after the last step %.2f  first unstable step %d' % (name, A['nsteps'].tolist(), A['khard'][-1], rec['first'][i]))
    rec['seconds_per_call'] = float(np.mean(times))
    unstable = int(np.sum(rec['first'] < K))
    assert 6 * unstable <= C, 'more than 1 chain in 6 is unstable: %d of %d' % (unstable, C)
    np.savez_compressed(OUT, **rec)
    print('unstable chains: %d of %d' % (unstable, C))
    for w in ('sig', 'epl', 'fy', 'khard'):
        print('largest calib_%-5s %.3e' % (w, float(np.max(rec['calib_' + w]))))
    print('plastic steps %d, sub-divided %d, steps that change khard %d; %.2f s per call' % (
        int(np.sum(np.any(np.diff(np.concatenate((rec['epl0'][:, None], rec['epl']), axis=1), axis=1) != 0., axis=2))),
        int(np.sum(rec['nsteps'] > 0)), int(np.sum(np.diff(np.concatenate((rec['khard0'][:, None], rec['khard']), axis=1), axis=1) != 0.)),
        rec['seconds_per_call']))
    print('wrote', OUT, '%.0f kB' % (os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    sys.exit(main())

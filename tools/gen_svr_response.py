#!/usr/bin/env python3
"""Fixture generator for Material.response under the SVR flow rule (enable_svr_flow) -- TEST
INFRASTRUCTURE, not product code.

Runs the unmodified reference (pyLabFEA v4.4.2) and scikit-learn on the build box and writes
``tests/golden/svr_response.npz``.  No test reads the reference or imports scikit-learn; they read this file.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_svr_response.py

The material is the one of tools/gen_svr_gradient.py with the SVC and the seven SVRs fitted WITHOUT shrinking: the fits
the device reproduces bit for bit (``ns<m>_*`` of tests/golden/svr_gradient.npz, checked equal here), so the rows are made
by the model the device holds.  Every row is one call ``response(sig, epl, deps, CV[, maxit])`` with ``khard`` set to
the recorded entry value first.  Each row is computed twice: with scikit-learn's ``predict`` and with ``predict`` of the
seven SVRs replaced by a plain FP64 NumPy sum over ALL training rows in row order (dense coefficients, zeros included),
which is the device's arithmetic.  The difference of the two runs is the reference's own noise floor for that row.

Keys (n rows):
  CV (6, 6); sig, epl, deps (n, 6); maxit (n,); khard_in (n,)               the inputs
  fy1 (n,), sig_out, depl (n, 6), grad_stiff (n, 6, 6), nsteps (n,), khard_out (n,)    reference results (first run)
  nsteps2 (n,), ncorr, ncorr2 (n,)     sub-step count of the second run; correction steps taken in either run
  nyf, nfull (n,)                      calls of calc_yf / ML_full_yf inside the call (first run)
  plastic (n,)                         the call left the elastic branch (grad_stiff differs from CV)
  calib_fy1, calib_sig, calib_depl, calib_ct, calib_khard (n,)   largest |run 1 - run 2| per row and output
  stable (n,)       both runs took the same number of sub-steps and agree on whether any correction step was taken
  branch (n,)       0 elastic, 1 on the yield locus, 2 split (fy0 < -0.15), 3 tiny plastic step (not sub-divided),
                    4 maxit = 5, 5 second call of a chain
  prev (n,)         row whose results are this row's inputs (chains), else -1
  khard_shape, fy1_shape               shapes the reference leaves (khard and fy1 are (1,) arrays after a plastic call)
  array_chain_*     the chain rows as true consecutive reference calls (khard left a (1,) array in between): fy1,
                    sig_out, depl, grad_stiff, nsteps, khard_out; not what the rows pin, recorded to measure the gap
  tiny_found        1 if a plastic step that is not sub-divided was found
  seconds_per_call  mean wall time of a plastic reference call on the machine that ran this generator
"""
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden', 'svr_response.npz')
os.environ.setdefault('MPLBACKEND', 'Agg')
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import pylabfea as FE  # noqa: E402  (the reference)

from gen_svc_data_training import quiet, sklearn_svc, wh_lc_data  # noqa: E402
from gen_svr_gradient import models, sklearn_svr  # noqa: E402

BRANCH = ('elastic', 'on the yield locus', 'split', 'tiny plastic step', 'maxit = 5', 'second call of a chain')


def material():
    """the reference material of gen_svr_gradient.py, SVC and SVRs without shrinking; checked against its records"""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'svr_gradient.npz'))
    epl_max, depl, Nseq, C, gamma = 0.03, 3.e-3, 8, 2.0, 1.5
    lc = wh_lc_data(epl_max=epl_max, depl=depl)
    with quiet():
        dd = FE.Data(lc, mat_name='ML_Hill_hardening', epl_start=0.0, epl_crit=0.0, epl_max=epl_max, depl=depl,
                     wh_data=True)
    with sklearn_svc(False, {}), sklearn_svr(False, {}), quiet(), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = FE.Material(name='ML_Hill_hardening_C2.0_G1.5', num=2)
        m.from_data(dd.mat_data)
        m.train_SVC(C=C, gamma=gamma, Ce=0.99, Fe=0.1, Nseq=Nseq, gridsearch=False)
        m.setup_fgrad_SVM()
    for k, s in enumerate(models(m)):
        assert np.array_equal(s.support_, z['ns%d_support' % k]) and np.array_equal(s.dual_coef_[0], z['ns%d_dual' % k])
        assert float(s.intercept_[0]) == float(z['ns%d_intercept' % k])
    assert np.array_equal(m.sc_feat.mean_, z['feat_mean']) and np.array_equal(m.sc_feat.scale_, z['feat_scale'])
    return m, np.array(dd.mat_data['flow_stress']), np.array(dd.mat_data['plastic_strain']), z


def plain_predict(m, z):
    """replace predict of the seven SVRs by the FP64 sum over all rows in row order (np.cumsum adds sequentially)"""
    X, g = np.array(z['x_sc']), float(z['gamma'])
    memo = {}

    def kernel(x):
        key = x.tobytes()
        if key not in memo:
            memo.clear()
            ss = np.zeros(len(X))
            for f in range(X.shape[1]):   # the distance feature by feature
                df = x[f] - X[:, f]
                ss = ss + df * df
            memo[key] = np.exp(-g * ss)
        return memo[key]
    for k, s in enumerate(models(m)):
        coef = np.zeros(len(X))
        coef[s.support_] = s.dual_coef_[0]
        icpt = float(s.intercept_[0])
        s.predict = (lambda xsc, coef=coef, icpt=icpt:
                     np.array([np.cumsum(coef * kernel(np.asarray(xsc, dtype=float)[0]))[-1] + icpt]))


class Counter(object):
    """branch decisions of one response call: calls of calc_yf / ML_full_yf and correction steps (one lstsq each)"""

    def __init__(self, m):
        self.m, self.n = m, dict(yf=0, full=0, corr=0)

    def __enter__(self):
        import pylabfea.material as FEM
        m, n = self.m, self.n
        self.orig = (m.calc_yf, m.ML_full_yf, FEM.np.linalg.lstsq)

        def count(name, fn):
            def f(*a, **kw):
                n[name] += 1
                return fn(*a, **kw)
            return f
        m.calc_yf, m.ML_full_yf = count('yf', self.orig[0]), count('full', self.orig[1])
        FEM.np.linalg.lstsq = count('corr', self.orig[2])
        return n

    def __exit__(self, *a):
        import pylabfea.material as FEM
        del self.m.calc_yf, self.m.ML_full_yf
        FEM.np.linalg.lstsq = self.orig[2]


def call(m, CV, row):
    sig, epl, deps, maxit, kh = row
    m.khard = kh
    with Counter(m) as n, warnings.catch_warnings():
        warnings.simplefilter('ignore')
        t0 = time.perf_counter()
        fy1, so, dp, ct = m.response(sig, epl, deps, CV, maxit=maxit)
        dt = time.perf_counter() - t0
    return dict(fy1=float(np.ravel(fy1)[0]), sig_out=np.array(so), depl=np.array(dp), grad_stiff=np.array(ct),
                nsteps=int(m.msg['nsteps']), khard_out=float(np.ravel(m.khard)[0]), ncorr=n['corr'], nyf=n['yf'],
                nfull=n['full'], plastic=not np.array_equal(ct, CV), khard_shape=np.shape(m.khard), fy1_shape=np.shape(fy1), dt=dt)


def main():
    rng = np.random.default_rng(29)
    m, sig, eps, z = material()
    CV = np.array(m.CV)
    kh0 = float(np.ravel(m.khard)[0])
    rows, branch, prev = [], [], []

    def add(b, s, e, d, maxit=50, kh=kh0, p=-1):
        rows.append((np.array(s, dtype=float), np.array(e, dtype=float), np.array(d, dtype=float), maxit, float(kh)))
        branch.append(b)
        prev.append(p)
        return len(rows) - 1
    pick = rng.choice(len(sig), 16, replace=False)
    el = [np.linalg.solve(CV, sig[i]) for i in pick]   # elastic strain of the data row's stress
    # elastic steps: from zero, and from half a data row's stress
    for n in range(2):
        add(0, np.zeros(6), np.zeros(6), 0.3 * el[n])
        add(0, 0.5 * sig[pick[n]], eps[pick[n]], 0.2 * el[n])
    def first_plastic(s, e, d, fs):
        """f d + t for the smallest factor f of fs for which the call leaves the elastic branch; t: a transverse part"""
        t = 2e-5 * rng.normal(size=6)
        for f in fs:
            if call(m, CV, (s, e, f * d + t, 50, kh0))['plastic']:
                return f * d + t
        raise AssertionError('no plastic step among %s' % (fs,))
    # on the yield locus (data rows; they lie a few per cent inside the SVC's locus): the smallest of the increments along
    # the stress that yields, and a large one, both with a transverse part
    for n in range(2, 9):
        i = pick[n]
        add(1, sig[i], eps[i], first_plastic(sig[i], eps[i], el[n], (0.03, 0.06, 0.12, 0.24)))
        add(1, sig[i], eps[i], 0.4 * el[n] + 2e-5 * rng.normal(size=6))
    # start inside (fy0 < -0.15), end outside
    for n in range(9, 16):
        i = pick[n]
        assert m.calc_yf(0.5 * sig[i], epl=eps[i]) < -0.15
        add(2, 0.5 * sig[i], eps[i], first_plastic(0.5 * sig[i], eps[i], el[n], (0.8, 1.2, 1.6)))
    # a plastic step that is NOT sub-divided: bisect for the increment at which the elastic branch ends and try the
    # plastic side of it at shrinking distances
    tiny = 0
    for n in (2, 3, 4):
        i = pick[n]
        lo, hi = 0., 0.24
        for _ in range(30):
            mid = 0.5 * (lo + hi)
            if call(m, CV, (sig[i], eps[i], mid * el[n], 50, kh0))['plastic']:
                hi = mid
            else:
                lo = mid
        for k in range(12):
            f = hi * (1. + 10. ** -k)
            r = call(m, CV, (sig[i], eps[i], f * el[n], 50, kh0))
            if r['plastic'] and r['nsteps'] == 0:
                add(3, sig[i], eps[i], f * el[n])
                tiny += 1
                break
    res = [call(m, CV, r) for r in rows]
    # maxit = 5 on four of them: two from the yield locus, two split ones (a step that is not sub-divided first)
    br = np.array(branch)
    split = sorted(np.nonzero(br == 2)[0], key=lambda k: res[k]['nsteps'])
    for k in list(np.nonzero(br == 1)[0][:2]) + [split[0], split[-1]]:
        s, e, d, _, kh = rows[k]
        res.append(call(m, CV, rows[add(4, s, e, d, maxit=5)]))
    # two consecutive calls on one material: the second starts where the first ended, with the khard it left behind
    for k in (np.nonzero(br == 1)[0][1], np.nonzero(br == 1)[0][2], split[-1]):
        s, e, d, _, _ = rows[k]
        j = add(5, res[k]['sig_out'], e + res[k]['depl'], d, kh=res[k]['khard_out'], p=k)
        res.append(call(m, CV, rows[j]))
    # the same chains as TWO CONSECUTIVE reference calls, khard not touched in between: the second call then starts with the
    # (1,) array the first left behind and takes the aliased path of ML_full_yf from its elastic test on.  Not what the
    # rows above pin (a float khard between calls, the facade's convention); recorded so that the gap is known.
    true2 = []
    for j in [k for k in range(len(rows)) if prev[k] >= 0]:
        call(m, CV, rows[prev[j]])
        s, e, d, mi, _ = rows[j]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fy1, so, dp, ct = m.response(s, e, d, CV, maxit=mi)
        true2.append(dict(fy1=float(np.ravel(fy1)[0]), sig_out=np.array(so), depl=np.array(dp), grad_stiff=np.array(ct),
                          nsteps=int(m.msg['nsteps']), khard_out=float(np.ravel(m.khard)[0])))
    plain_predict(m, z)
    res2 = [call(m, CV, r) for r in rows]
    n = len(rows)
    out = dict(CV=CV, sig=np.stack([r[0] for r in rows]), epl=np.stack([r[1] for r in rows]),
               deps=np.stack([r[2] for r in rows]), maxit=np.array([r[3] for r in rows], dtype=np.int32),
               khard_in=np.array([r[4] for r in rows]), branch=np.array(branch, dtype=np.int32),
               prev=np.array(prev, dtype=np.int32), tiny_found=int(tiny > 0))
    for key in ('fy1', 'sig_out', 'depl', 'grad_stiff', 'khard_out'):
        out[key] = np.array([r[key] for r in res])
    out['plastic'] = np.array([r['plastic'] for r in res])
    for key in ('nsteps', 'ncorr', 'nyf', 'nfull'):
        out[key] = np.array([r[key] for r in res], dtype=np.int32)
    out['nsteps2'] = np.array([r['nsteps'] for r in res2], dtype=np.int32)
    out['ncorr2'] = np.array([r['ncorr'] for r in res2], dtype=np.int32)
    for key, name in (('fy1', 'fy1'), ('sig_out', 'sig'), ('depl', 'depl'), ('grad_stiff', 'ct'), ('khard_out', 'khard')):
        out['calib_' + name] = np.array([np.max(np.abs(np.asarray(a[key]) - np.asarray(b[key]))) for a, b in zip(res, res2)])
    out['stable'] = np.array([a['nsteps'] == b['nsteps'] and (a['ncorr'] > 0) == (b['ncorr'] > 0) for a, b in zip(res, res2)])
    plastic = [r for r in res if r['plastic']]
    out['khard_shape'] = np.array(plastic[-1]['khard_shape'], dtype=np.int64)
    out['fy1_shape'] = np.array(plastic[-1]['fy1_shape'], dtype=np.int64)
    out['seconds_per_call'] = float(np.mean([r['dt'] for r in plastic if r['nsteps'] > 0]))
    chain = [k for k in range(n) if prev[k] >= 0]
    for key in ('fy1', 'sig_out', 'depl', 'grad_stiff', 'khard_out'):
        out['array_chain_' + key] = np.array([r[key] for r in true2])
    out['array_chain_nsteps'] = np.array([r['nsteps'] for r in true2], dtype=np.int32)
    nun = int(np.sum(~out['stable']))
    assert 8 * nun <= n, 'more than 1 row in 8 is unstable: %d of %d' % (nun, n)
    np.savez_compressed(OUT, **out)
    print('%d rows; per branch: %s' % (n, ', '.join('%s %d' % (BRANCH[b], branch.count(b)) for b in range(6))))
    print('nsteps', out['nsteps'].tolist())
    print('correction steps', out['ncorr'].tolist())
    print('plastic', out['plastic'].astype(int).tolist())
    print('unstable rows: %d of %d %s; such a step FROM the yield locus: %s' % (
        nun, n, np.nonzero(~out['stable'])[0].tolist(), 'found' if tiny else 'none exists: the plastic side of the elastic limit is sub-divided down to a relative distance of 1e-11'))
    print('plastic calls that end after the trial step (not sub-divided): rows %s' % np.nonzero(out['plastic'] & (out['nsteps'] == 0) & (out['maxit'] == 50))[0].tolist())
    st = out['stable']
    for name in ('fy1', 'sig', 'depl', 'ct', 'khard'):
        print('largest calib_%-5s stable rows %.3e   all rows %.3e' % (name, np.max(out['calib_' + name][st]),
                                                                        np.max(out['calib_' + name])))
    print('khard on entry %.6g; khard left behind %.6g .. %.6g, shape %s; fy1 shape %s; %.2f s per sub-divided call' % (
        kh0, np.min(out['khard_out']), np.max(out['khard_out']), tuple(out['khard_shape']), tuple(out['fy1_shape']),
        out['seconds_per_call']))
    print('chains as consecutive reference calls (khard a (1,) array on entry) against the rows above: nsteps %s / %s; '
          'largest difference sig %.3e, depl %.3e, grad_stiff %.3e, khard %.3e' % (
              out['array_chain_nsteps'].tolist(), out['nsteps'][chain].tolist(),
              np.max(np.abs(out['array_chain_sig_out'] - out['sig_out'][chain])),
              np.max(np.abs(out['array_chain_depl'] - out['depl'][chain])),
              np.max(np.abs(out['array_chain_grad_stiff'] - out['grad_stiff'][chain])),
              np.max(np.abs(out['array_chain_khard_out'] - out['khard_out'][chain]))))
    print('wrote', OUT, '%.0f kB' % (os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    sys.exit(main())

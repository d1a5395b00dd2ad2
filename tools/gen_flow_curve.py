#!/usr/bin/env python3
"""Fixture generator for Material.flow_curve, Material.data_curve and create_test_sig -- TEST
INFRASTRUCTURE, not product code.

Runs the unmodified reference (pyLabFEA v4.4.2), scikit-learn and SciPy on the build box and writes
``tests/golden/flow_curve.npz``.  No test reads the reference or imports scikit-learn; they read this file.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_flow_curve.py

The material is the one of tools/gen_svr_response.py::material() (the ``ML_Hill_hardening`` fit of DESIGN §21, fitted
without shrinking, whose tables the device reproduces bit for bit) with ``ML_grad = False``.  The step rule of DESIGN §30
is written out here and calls only the reference's ``find_yloc_scalar``, ``calc_fgrad``, ``calc_yf`` and ``eps_eq``.
Every curve is run three times:
  (a) loose   every point of the locus is ``fsolve(find_yloc_scalar, mat.sy, xtol=1e-5)``, as in the example; for information
  (b) tight   every fsolve answer x polished by ``brentq`` on [x (1 - 1e-3), x (1 + 1e-3)] to rtol = 4 eps: what the tests pin
  (c) plain   (b) with ``decision_function`` and the gradient replaced by plain FP64 NumPy sums over the support vectors
              in row order (np.cumsum adds sequentially): the device's arithmetic
``calib_*`` is the largest |b - c| per curve and output: the reference's own noise floor.

Keys (24 SVC curves = 12 directions x predictor 0 / 1000; K = 21 recorded steps at most, NaN past a curve's end):
  su (12, 6); predictor (24,); dir (24,) the direction of a curve; depl, epl_max
  nsteps (24,); x_a, x, x_c (24, K+1); epl_a, epl, epl_c (24, K+1, 6); yf_a, yf, yf_c (24, K+1)
  hk, hk_c (24, K)     Material.khard after each gradient evaluation, i.e. the hardening value CLIPPED at 0 (run b), and
                       the raw value before the clip from the plain sums (run c)
  calib_x, calib_epl, calib_yf, calib_hk (24,)    (hk: between the clipped values)
  march_dev (24,)      largest |marched root - x| / x per curve: ray_root (tests/flow_curve_cases.py) on find_yloc_scalar
                       from the previous root of run (b)
  hill_nsteps (12,), hill_x (12, K+1), hill_epl (12, K+1, 6), hill_yf (12, K+1)   the Hill reference material, predictor 0,
                       roots by the same tight search
  dc_ilc (2,), dc_index_<i>, dc_sig0_<i>, dc_peeq_<i>, dc_seq_data_<i>, dc_x_fsolve_<i>, dc_x_march_<i>    plot_lc of the
                       example for two load cases: kept rows, unit stress, the example's fsolve answers and the marched roots
  ts_json (bytes), ts_sig, ts_epl, ts_yf, ts2_*    a small JSON database (four load cases of the example's, every second
                       sample) and what create_test_sig returns for it with number_sig_per_strain = 4 and 2
"""
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden', 'flow_curve.npz')
os.environ.setdefault('MPLBACKEND', 'Agg')
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pylabfea as FE  # noqa: E402  (the reference)
from scipy.optimize import brentq, fsolve  # noqa: E402

import flow_curve_cases as FC  # noqa: E402
from gen_svc_data_training import JSON_REF, quiet  # noqa: E402
from gen_svr_response import material  # noqa: E402

DEPL, EPL_MAX, MAX_STEPS, KREC = 1.e-3, 0.0205, 300, 21
EPS = np.finfo(float).eps


def tight_root(m, su, epl, loose=False):
    x = float(fsolve(m.find_yloc_scalar, m.sy, args=(su, epl), xtol=1.e-5)[0])
    if loose:
        return x
    return float(brentq(lambda t: float(np.ravel(m.find_yloc_scalar(t, su, epl))[0]), x * (1. - 1.e-3), x * (1. + 1.e-3),
                        xtol=1e-300, rtol=4 * EPS))


def chain(m, su, predictor, loose=False, march=None):
    """the step rule of DESIGN §30 on the reference material m; march: list that collects |marched root - root| / root"""
    e = np.zeros(6)
    xs, es, ys, hs, margins = [], [], [], [], []
    k = 0
    x_prev = float(m.sy)
    while True:
        x = tight_root(m, su, e, loose)
        if march is not None:
            st, xm = FC.ray_root(lambda t: float(np.ravel(m.find_yloc_scalar(t, su, e))[0]), x_prev)
            assert st == 0
            march.append(abs(xm - x) / x)
        x_prev = x
        xs.append(x), es.append(np.array(e)), ys.append(float(np.ravel(m.calc_yf(su * x, epl=e))[0]))
        peeq = float(FE.eps_eq(e)) + DEPL
        margins.append(abs(peeq - EPL_MAX))
        if not (peeq <= EPL_MAX and k < MAX_STEPS):
            break
        a = np.ravel(np.array(m.calc_fgrad(su * (x + peeq * predictor), epl=e), dtype=float))
        hs.append(float(np.ravel(m.khard)[0]))
        e = e + a * DEPL / float(FE.eps_eq(a))
        k += 1
    assert min(margins) > 1.e-6, 'a stop decision is not clear of the limit: %g' % min(margins)
    return dict(nsteps=k, x=np.array(xs), epl=np.array(es), yf=np.array(ys), hk=np.array(hs))


def plain_sums(m):
    """replace decision_function of the SVC by the FP64 sum in row order; returns the raw-gradient function"""
    s = m.svm_yf
    sv, dc, g, b = np.array(s.support_vectors_), np.array(s.dual_coef_[0]), float(m.gam_yf), float(s.intercept_[0])

    def kern(x):
        ss = np.zeros(len(sv))
        for f in range(sv.shape[1]):
            df = x[f] - sv[:, f]
            ss = ss + df * df
        return np.exp(-g * ss)
    s.decision_function = lambda X: np.array([np.cumsum(dc * kern(np.asarray(x, dtype=float)))[-1] + b
                                              for x in np.atleast_2d(X)])
    orig = m.calc_fgrad

    def fgrad(sig, epl=None, **kw):
        x = np.ravel(m.create_scaled_input(np.asarray(sig, dtype=float), epl, 0., 0., 0.))
        w = dc * kern(x)
        dK = np.array([np.cumsum(w * (-2. * g) * (x[f] - sv[:, f]))[-1] for f in range(12)])
        raw = -float(np.cumsum(dK[6:12])[-1]) * m.scale_seq / m.scale_wh
        m._raw_hk = raw
        m.khard = max(0., raw)
        return dK[0:6] / m.scale_seq
    m.calc_fgrad = fgrad
    return orig


def pad(rows, width, tail=()):
    out = np.full((len(rows), width) + tuple(tail), np.nan)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def main():
    t0 = time.time()
    m, sig_dat, eps_dat, z = material()
    m.ML_grad = False
    w = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_data_training.npz'))
    assert np.array_equal(m.svm_yf.support_, w['wh_ns_support']) and np.array_equal(m.svm_yf.dual_coef_[0], w['wh_ns_dual'])
    assert float(m.svm_yf.intercept_[0]) == float(w['wh_ns_intercept']) and len(w['wh_ns_support']) == 1018
    su = FC.directions(FE.load_cases)
    out = dict(su=su, depl=DEPL, epl_max=EPL_MAX)
    curves = [(d, p) for p in (0., 1000.) for d in range(len(su))]
    out['dir'] = np.array([c[0] for c in curves], dtype=np.int32)
    out['predictor'] = np.array([c[1] for c in curves])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ra = [chain(m, su[d], p, loose=True) for d, p in curves]
        march = [[] for _ in curves]
        rb = [chain(m, su[d], p, march=march[i]) for i, (d, p) in enumerate(curves)]
        t_chain = (time.time() - t0)
        # data_curve: plot_lc of the example for two load cases (before the sums are replaced)
        out['dc_ilc'] = np.array([1, 10], dtype=np.int32)
        for ilc in (1, 10):
            lci = m.msparam[0]['lc_indices']
            i0, i1 = int(lci[ilc]), int(lci[ilc + 1])
            sd, ed = m.msparam[0]['flow_stress'][i0:i1, :], m.msparam[0]['plastic_strain'][i0:i1, :]
            keep = np.nonzero(FE.eps_eq(ed) >= 0.002)[0]
            sf, ef = sd[keep], ed[keep]
            s0 = sf[-1] / FE.sig_eq_j2(sf[-1])
            xf = np.array([float(fsolve(m.find_yloc, m.sy, args=(s0, ef[i]), xtol=1.e-5)[0]) for i in range(len(ef))])
            xm = []
            for i in range(len(ef)):
                st, r = FC.ray_root(lambda t: float(np.ravel(m.find_yloc_scalar(t, s0, ef[i]))[0]), float(m.sy))
                xm.append(r if st == 0 else np.nan)
            t = '_%d' % ilc
            out.update({'dc_index' + t: (i0 + keep).astype(np.int64), 'dc_sig0' + t: s0, 'dc_peeq' + t: FE.eps_eq(ef),
                        'dc_seq_data' + t: FE.sig_eq_j2(sf), 'dc_x_fsolve' + t: xf, 'dc_x_march' + t: np.array(xm),
                        'dc_epl' + t: ef})
        # Hill reference material
        mh = FC.hill_material(FE)
        rh = [chain(mh, su[d], 0.) for d in range(len(su))]
        plain_sums(m)
        rc = []
        for d, p in curves:
            r = chain(m, su[d], p)
            rc.append(r)
        # the raw values of run (c): the chain again would give the same numbers; collect them from a second pass
        raw = []
        for (d, p), r in zip(curves, rc):
            h = []
            for k in range(r['nsteps']):
                peeq = float(FE.eps_eq(r['epl'][k])) + DEPL
                m.calc_fgrad(su[d] * (r['x'][k] + peeq * p), epl=r['epl'][k])
                h.append(m._raw_hk)
            raw.append(np.array(h))
    for a, b, c in zip(ra, rb, rc):
        assert b['nsteps'] == c['nsteps'], 'runs (b) and (c) differ in their number of steps'
    out['nsteps'] = np.array([r['nsteps'] for r in rb], dtype=np.int32)
    out['nsteps_a'] = np.array([r['nsteps'] for r in ra], dtype=np.int32)
    assert KREC == int(np.max(out['nsteps']))
    for tag, rr in (('_a', ra), ('', rb), ('_c', rc)):
        out['x' + tag] = pad([r['x'] for r in rr], KREC + 1)
        out['epl' + tag] = pad([r['epl'] for r in rr], KREC + 1, (6,))
        out['yf' + tag] = pad([r['yf'] for r in rr], KREC + 1)
    out['hk'] = pad([r['hk'] for r in rb], KREC)
    out['hk_c'] = pad(raw, KREC)
    for key in ('x', 'epl', 'yf', 'hk'):
        out['calib_' + key] = np.array([float(np.max(np.abs(np.asarray(b[key]) - np.asarray(c[key])))) for b, c in zip(rb, rc)])
    out['march_dev'] = np.array([max(v) for v in march])
    assert np.all(out['march_dev'] <= 1e-9), 'a marched root is not the root of run (b): %g' % np.max(out['march_dev'])
    out['hill_nsteps'] = np.array([r['nsteps'] for r in rh], dtype=np.int32)
    out['hill_x'] = pad([r['x'] for r in rh], KREC + 1)
    out['hill_epl'] = pad([r['epl'] for r in rh], KREC + 1, (6,))
    out['hill_yf'] = pad([r['yf'] for r in rh], KREC + 1)
    # create_test_sig on a small database
    with open(JSON_REF) as fp:
        db = json.load(fp)
    small = {}
    for key in list(db)[:4]:
        lc = dict(db[key])
        lc['Results'] = {c: v[::2] for c, v in db[key]['Results'].items()}
        small[key] = lc
    txt = json.dumps(small)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'small.json')
        with open(path, 'w') as fp:
            fp.write(txt)
        with quiet(), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ts = FE.create_test_sig(path)
            ts2 = FE.create_test_sig(path, number_sig_per_strain=2)
    out['ts_json'] = np.frombuffer(txt.encode(), dtype=np.uint8)
    out['ts_sig'], out['ts_epl'], out['ts_yf'] = ts
    out['ts2_sig'], out['ts2_epl'], out['ts2_yf'] = ts2
    np.savez_compressed(OUT, **out)
    la = max(float(np.nanmax(np.abs(a['x'] - b['x'][:len(a['x'])]))) for a, b in zip(ra, rb) if a['nsteps'] == b['nsteps'])
    le = max(float(np.nanmax(np.abs(a['epl'] - b['epl']))) for a, b in zip(ra, rb) if a['nsteps'] == b['nsteps'])
    print('%d SVC curves, steps %s; %d Hill curves, steps %s' % (len(rb), out['nsteps'].tolist(), len(rh), out['hill_nsteps'].tolist()))
    print('loose run: steps %s; against the tight run, largest difference x %.3e, epl %.3e' % (out['nsteps_a'].tolist(), la, le))
    print('x in %.4g .. %.4g; largest |yf| tight %.3e, loose %.3e; hk (clipped) up to %.6g, raw %.6g .. %.6g' % (
        np.nanmin(out['x']), np.nanmax(out['x']), np.nanmax(np.abs(out['yf'])), np.nanmax(np.abs(out['yf_a'])),
        np.nanmax(out['hk']), np.nanmin(out['hk_c']), np.nanmax(out['hk_c'])))
    for key in ('x', 'epl', 'yf', 'hk'):
        print('largest calib_%-4s %.3e' % (key, np.max(out['calib_' + key])))
    print('largest |marched root - root| / root %.3e' % np.max(out['march_dev']))
    for ilc in (1, 10):
        t = '_%d' % ilc
        xf, xm = out['dc_x_fsolve' + t], out['dc_x_march' + t]
        print('load case %d: %d rows kept, fsolve against the marched root: largest relative difference %.3e' % (
            ilc, len(xf), np.max(np.abs(xf - xm) / xm)))
    print('create_test_sig: database of %d load cases, %.0f kB of JSON; shapes %s %s %s' % (
        len(small), len(txt) / 1e3, ts[0].shape, ts[1].shape, ts[2].shape))
    print('a tight chain of 20 steps takes %.2f s here; the generator ran %.0f s' % (t_chain / (2 * len(curves)), time.time() - t0))
    print('wrote', OUT, '%.0f kB' % (os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python3
"""Fixture generator for texture-dependent SVC yield functions (Data(tx_data=True) -> Material.from_data([...]) ->
train_SVC(train_index=, test_index=) -> calc_yf(tex=) / find_yloc(tex=)) -- TEST INFRASTRUCTURE, not product code.

Runs the unmodified reference (pyLabFEA v4.4.2) and scikit-learn on the build box and writes
``tests/golden/texture_svc.npz``.  No test reads the reference or imports scikit-learn; they read this file.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_texture_svc.py

Data: six data sets.  Descriptors: name, texture_index and the 38 gsh_coeff_reconstructed_random values of the reference's
four examples/Texture/Texture_Files/*.json, and two drawn from default_rng(7).uniform(-0.6, 0.6) (first coefficient 1).
Yield stresses of set k: the 48 load cases of load_cases(24, 24) scaled onto the locus of a Hill material with
hill = 1 + 0.4 [t0, t1, t2, -t0, -t1, -t2] and sy = 100 (1 + 0.15 t0), t = gsh[1:4].  Each set is written as a JSON database
(tests/texture_cases.py::database_json: a short stress-strain path per load case and the `Texture` entry) and read by the
reference's Data(..., tx_data=True), once with GSH_3 and once with GSH_7.

Keys (``<d>`` = GSH_3 / GSH_7; ``<v>`` = full / dev for dev_only False / True):
  db_0 .. db_5              the JSON databases (bytes); gsh (6, 38), tx_name, tx_index
  md<k>_<field>             mat_data of set k (tests/texture_cases.py: MD_SCALAR, MD_ARRAY; MD_BIG for set 0), equal for both
                            descriptors except texture / tdim, which are md<k>_<d>_texture, md<k>_<d>_tdim
  fd_<d>_*                  attributes from_data leaves (Nset, txdat, tdim, ind_tx, Ndof, sy, sdim, whdat, epc, CV)
  rows_stress (1152, 6), y_train (960,), y_all (1152,)      unscaled stress columns of all six sets in set order, labels
  <d>_<v>_mean / _scale     StandardScaler on the 960 training rows; _gap_mean / _gap_scale: |scikit-learn - two-pass NumPy|
  <d>_<v>_support, _dual, _intercept, _n_iter               the non-shrinking fit of train_SVC(C=10, gamma=1, Fe=0.8,
                            Ce=0.95, Nseq=2, train_index=0..4, test_index=[5]); X is (rows - mean) / scale, asserted to the bit
  <d>_<v>_acc, _mcc (2,)    train and hold-out score; _min_dec: smallest |decision| over the scored rows
  <d>_<v>_calib             largest |decision_function - plain FP64 NumPy sum in row order| over the probes and scored rows, and
                            the same with every feature moved by one unit in the last place
  probe_sig (64, 6), probe_tex_id (64,); <d>_<v>_yf_one (64,), _yf_rows (64,)   calc_yf at texture 2 / at texture
                            probe_tex_id[i] per row
  gs_<d>_*                  grid search (cvals [1, 10], gvals [0.5, 1], six sets): fold test indices, per-fold train / test
                            scores (candidates x folds), best C / gamma, refit support / dual / intercept / n_iter / score
  ray_<d>_status, _x_ref (6, 72)   marched and bisected search (the search of yield_scale) on scikit-learn's decision function
                            through the reference's find_yloc_scalar, from x0 = sy / seq_J2(snorm)
  ray_<d>_x_fsolve (6, 72), _fsolve_ok     the example's coupled fsolve per texture; ok where it converged to the marched root
  ray_<d>_r_ref             worst |calc_yf - longdouble restatement| at the roots in units of A 2^-53
"""
import contextlib
import glob
import io
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
os.environ.setdefault('MPLBACKEND', 'Agg')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pylabfea as FE  # noqa: E402  (the reference)
import pylabfea.material as FEM  # noqa: E402
from scipy.optimize import fsolve  # noqa: E402
from sklearn import svm  # noqa: E402
from sklearn.metrics import matthews_corrcoef  # noqa: E402
from sklearn.model_selection import KFold  # noqa: E402

import texture_cases as TC  # noqa: E402

assert FE.__version__ == '4.4.2'
REF_SRC = os.path.dirname(os.path.dirname(FE.__file__))
TEX_FILES = os.path.join(os.path.dirname(REF_SRC), 'examples', 'Texture', 'Texture_Files', '*.json')


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


@contextlib.contextmanager
def sklearn_svc(seen):
    """the reference's SVC with shrinking=False, recording the data handed to fit"""
    orig = svm.SVC

    class SVC(orig):
        def __init__(self, **kw):
            kw.setdefault('shrinking', False)
            super().__init__(**kw)

        def fit(self, X, y, sample_weight=None):
            seen['X'], seen['y'] = np.array(X), np.array(y)
            return super().fit(X, y, sample_weight)
    FEM.svm.SVC = SVC
    try:
        yield
    finally:
        FEM.svm.SVC = orig


def descriptors():
    names, index, gsh = [], [], []
    for f in sorted(glob.glob(TEX_FILES)):
        with open(f) as fp:
            d = json.load(fp)
        names.append(d['name']), index.append(float(d['texture_index'])), gsh.append(d['gsh_coeff_reconstructed_random'])
    assert len(names) == 4 and all(len(g) == 38 for g in gsh)
    extra = np.random.default_rng(7).uniform(-0.6, 0.6, size=(2, 38))
    extra[:, 0] = 1.
    for k in range(2):
        names.append('synthetic%d' % k), index.append(float(k + 1)), gsh.append(extra[k].tolist())
    return names, np.array(index), np.array(gsh, dtype=float)


def hill_material(t):
    m = FE.Material(name='Hill-texture')
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=100. * (1. + 0.15 * t[0]), hill=list(1. + 0.4 * np.array([t[0], t[1], t[2], -t[0], -t[1], -t[2]])), sdim=6)
    return m


def plain_decision(s, X):
    """decision function as a plain FP64 NumPy sum in row order"""
    sv, dc, g, b = s.support_vectors_, s.dual_coef_[0], s._gamma, s.intercept_[0]
    return np.array([np.sum(dc * np.exp(-g * np.sum((sv - x) ** 2, axis=1))) for x in X]) + b


def marched_root(f, x0):
    """(root, status) of the search of yield_scale on f: march by 0.98 / 1.02 from x0, then bisection to neighbours"""
    x, fx = x0, f(x0)
    if fx >= 0.:
        n = 0
        while fx >= 0.:
            hi, fhi = x, fx
            n += 1
            if x < 0.01 * x0 or n > 240:
                return np.nan, 1
            x *= 0.98
            fx = f(x)
        lo, flo = x, fx
    else:
        n = 0
        while fx < 0.:
            lo, flo = x, fx
            n += 1
            if x > 5. * x0 or n > 90:
                return np.nan, 1
            x *= 1.02
            fx = f(x)
        hi, fhi = x, fx
    for _ in range(81):
        mid = lo + 0.5 * (hi - lo)
        if not (lo < mid < hi):
            return (lo if -flo < fhi else hi), 0
        fm = f(mid)
        if fm < 0.:
            lo, flo = mid, fm
        else:
            hi, fhi = mid, fm
    return np.nan, 2


def main():
    out = {}
    rng = np.random.default_rng(11)
    names, tx_index, gsh = descriptors()
    out.update(gsh=gsh, tx_name=np.array(names), tx_index=tx_index)
    sunit = FE.load_cases(number_3d=24, number_6d=24)
    tmp = tempfile.mkdtemp()
    hills = []
    for k in range(TC.NSET):
        mh = hill_material(gsh[k, 1:4])
        hills.append(mh)
        sig_y = sunit * (mh.sy / mh.calc_seq(sunit))[:, None]
        normal = np.array([mh.calc_fgrad(s) for s in sig_y])
        out['db_%d' % k] = np.frombuffer(TC.database_json(names[k], tx_index[k], gsh[k], sig_y, normal, np.array(mh.CV)),
                                         dtype=np.uint8)
    print('databases: %s bytes' % [len(out['db_%d' % k]) for k in range(TC.NSET)])

    probe_tex_id = rng.integers(0, TC.NSET, size=64)
    u = rng.normal(size=(64, 6))
    probe_sig = u / FE.sig_eq_j2(u)[:, None] * (100. * rng.uniform(0.5, 1.5, size=64))[:, None]
    out.update(probe_sig=probe_sig, probe_tex_id=probe_tex_id.astype(np.int32))
    theta, snorm = TC.snorm()
    assert np.array_equal(snorm[:, :3], FE.sig_cyl2princ(np.array([np.ones(TC.NA), theta]).T))

    for desc in TC.DESCRIPTORS:
        tdim = int(desc.split('_')[1])
        sets = TC.read_sets(FE, out, tmp, desc)
        mds = [d.mat_data for d in sets]
        for k, md in enumerate(mds):
            assert md['tx_name'] == names[k] and md['tx_data'] and md['tx_descriptor'] == desc
            rec = {}
            for f in TC.MD_SCALAR:
                rec[f] = np.array(md[f], dtype=float)
            for f in TC.MD_ARRAY + (TC.MD_BIG if k == 0 else ()):
                rec[f] = np.array(md[f], dtype=float)
            rec['flow_shape'] = np.array(np.shape(md['flow_stress']))
            for f, v in rec.items():
                key = 'md%d_%s' % (k, f) if f not in ('texture', 'tdim') else 'md%d_%s_%s' % (k, desc, f)
                if key in out:
                    assert np.array_equal(out[key], v), key
                out[key] = v
            assert np.array_equal(md['texture'], gsh[k, 1:1 + tdim])
            err = np.max(np.abs(FE.sig_eq_j2(md['sig_ideal']) / hills[k].calc_seq(md['sig_ideal']) * 0 +
                                hills[k].calc_seq(md['sig_ideal']) / hills[k].sy - 1.))
            assert err < 1e-4, err   # sig_ideal lies on the generating Hill locus (to the rounding of the database)
        tex = TC.textures(out, desc)

        def make(dev):
            m = FE.Material(name='ML-texture-' + desc)
            m.dev_only = dev
            with quiet():
                m.from_data(mds)
            return m
        m0 = make(False)
        out.update({'fd_%s_Nset' % desc: m0.Nset, 'fd_%s_txdat' % desc: bool(m0.txdat), 'fd_%s_tdim' % desc: m0.tdim,
                    'fd_%s_ind_tx' % desc: m0.ind_tx, 'fd_%s_Ndof' % desc: m0.Ndof, 'fd_%s_sy' % desc: float(m0.sy),
                    'fd_%s_sdim' % desc: m0.sdim, 'fd_%s_whdat' % desc: bool(m0.whdat), 'fd_%s_epc' % desc: float(m0.epc),
                    'fd_%s_CV' % desc: np.array(m0.CV)})
        assert m0.Nset == 6 and m0.txdat and m0.ind_tx == 6 and m0.Ndof == 6 + tdim and m0.sy == mds[0]['sy_av']

        models = {}
        for dev in (False, True):
            pre = '%s_%s' % (desc, 'dev' if dev else 'full')
            scores = {}
            for metric in ('acc', 'mcc'):
                seen = {}
                ml = make(dev)
                with sklearn_svc(seen), quiet(), warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    scores[metric] = ml.train_SVC(train_index=list(TC.TRAIN), test_index=list(TC.HOLD), metric=metric,
                                                  **TC.TRAIN_KW)
            rows = np.concatenate([ml._create_data_for_ms(Ce=TC.TRAIN_KW['Ce'], Fe=TC.TRAIN_KW['Fe'], Nseq=TC.TRAIN_KW['Nseq'],
                                                          extend=False, idx_ms=k)[2] for k in range(TC.NSET)])
            yall = np.concatenate([ml._create_data_for_ms(Ce=TC.TRAIN_KW['Ce'], Fe=TC.TRAIN_KW['Fe'], Nseq=TC.TRAIN_KW['Nseq'],
                                                          extend=False, idx_ms=k)[3] for k in range(TC.NSET)])
            ntr = len(seen['y'])
            if not dev:   # (with dev_only the reference's rows hold the deviator of sig_ideal; the façade starts from these)
                if 'rows_stress' in out:
                    assert np.array_equal(out['rows_stress'], rows[:, :6])
                out.update(rows_stress=rows[:, :6], y_train=seen['y'], y_all=yall)
                assert np.array_equal(rows, TC.all_rows(out, desc))
            else:
                assert np.array_equal(rows, np.concatenate((TC.stress_dev(out['rows_stress']), rows[:, 6:]), axis=1)) or \
                    np.max(np.abs(rows[:, :6] - TC.stress_dev(out['rows_stress']))) < 1e-12
            sc = ml.std_scaler
            xtr = rows[:ntr]
            out.update({pre + '_mean': sc.mean_, pre + '_scale': sc.scale_,
                        pre + '_gap_mean': np.abs(sc.mean_ - np.mean(xtr, axis=0)),
                        pre + '_gap_scale': np.abs(sc.scale_ - np.sqrt(np.var(xtr, axis=0)))})
            s = ml.svm_yf
            out.update({pre + '_support': s.support_.astype(np.int32), pre + '_dual': s.dual_coef_[0],
                        pre + '_intercept': float(s.intercept_[0]), pre + '_n_iter': int(np.ravel(s.n_iter_)[0]),
                        pre + '_acc': np.array(scores['acc'], dtype=float), pre + '_mcc': np.array(scores['mcc'], dtype=float)})
            p = TC.tables(out, desc, dev)
            if dev:   # the training rows of the reference are the deviator already; taking it again is exact or 1 ulp
                print(pre, 'X from the recorded stress rows against the reference X: max diff %.2e'
                      % np.max(np.abs(p['X'] - seen['X'])))
            else:
                assert np.array_equal(p['X'], seen['X']), pre
            if not np.array_equal(p['sv'], s.support_vectors_):   # dev: store the vectors themselves
                out[pre + '_sv'] = s.support_vectors_
            Xall = ml.create_scaled_input(rows[:, :6], tex=rows[:, 6:])
            dec = s.decision_function(Xall)
            out[pre + '_min_dec'] = float(np.min(np.abs(dec)))
            # calc_yf on the probes
            with quiet():
                y_one = ml.calc_yf(probe_sig, tex=tex[2])
                y_rows = ml.calc_yf(probe_sig, tex=tex[probe_tex_id])
            out.update({pre + '_yf_one': y_one, pre + '_yf_rows': y_rows})
            P = np.concatenate((ml.create_scaled_input(probe_sig, tex=tex[2]),
                                ml.create_scaled_input(probe_sig, tex=tex[probe_tex_id]), Xall))
            c0 = np.max(np.abs(s.decision_function(P) - plain_decision(s, P)))
            c1 = np.max(np.abs(s.decision_function(P) - plain_decision(s, np.nextafter(P, np.inf))))
            out[pre + '_calib'] = float(max(c0, c1))
            assert out[pre + '_min_dec'] > 100. * out[pre + '_calib'], (pre, out[pre + '_min_dec'], out[pre + '_calib'])
            models[dev] = ml
            print('%s: nSV %d, n_iter %d, acc %s, mcc %s, min|dec| %.3e, calib %.2e (plain %.2e, ulp-moved %.2e)' % (
                pre, len(s.support_), out[pre + '_n_iter'], scores['acc'], scores['mcc'], out[pre + '_min_dec'],
                out[pre + '_calib'], c0, c1))

        # ---- grid search over the textures
        ml = make(False)
        calls = []
        cls_train = FEM.Material.train_SVC

        def spy(*a, **kw):
            r = cls_train(ml, *a, **kw)
            calls.append((kw.get('C'), kw.get('gamma'), kw.get('train_index'), kw.get('test_index'), r))
            return r
        ml.train_SVC = spy
        seen = {}
        t0 = time.time()
        with sklearn_svc(seen), quiet(), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            r = cls_train(ml, gridsearch=True, verbose=0, Fe=TC.TRAIN_KW['Fe'], Ce=TC.TRAIN_KW['Ce'], Nseq=TC.TRAIN_KW['Nseq'],
                          C=10, gamma=1, **TC.GRID)
        dt = time.time() - t0
        cv = [c for c in calls if c[3] is not None]
        ncand = len(TC.GRID['cvals']) * len(TC.GRID['gvals'])
        assert len(cv) == 5 * ncand and len(calls) == 5 * ncand + 1
        folds = [np.array(te) for _, te in KFold(n_splits=5, shuffle=True, random_state=42).split(np.zeros(TC.NSET))]
        for k, c in enumerate(cv):
            assert np.array_equal(c[3], folds[k % 5])
        s = ml.svm_yf
        out.update({'gs_%s_fold_of' % desc: np.concatenate([np.full(len(f), k) for k, f in enumerate(folds)])[
                        np.argsort(np.concatenate(folds))].astype(np.int32),
                    'gs_%s_train' % desc: np.array([c[4][0] for c in cv]).reshape(ncand, 5),
                    'gs_%s_test' % desc: np.array([c[4][1] for c in cv]).reshape(ncand, 5),
                    'gs_%s_best_C' % desc: float(ml.C_yf), 'gs_%s_best_gamma' % desc: float(ml.gam_yf),
                    'gs_%s_support' % desc: s.support_.astype(np.int32), 'gs_%s_dual' % desc: s.dual_coef_[0],
                    'gs_%s_intercept' % desc: float(s.intercept_[0]), 'gs_%s_n_iter' % desc: int(np.ravel(s.n_iter_)[0]),
                    'gs_%s_score' % desc: float(r[0])})
        print('gs_%s: folds %s, best C=%g gamma=%g, refit nSV %d, %.1f s' % (
            desc, [f.tolist() for f in folds], ml.C_yf, ml.gam_yf, len(s.support_), dt))
        print('   test scores', out['gs_%s_test' % desc].tolist())

        # ---- rays: every texture x 72 pi-plane rays
        ml = models[False]
        p = TC.tables(out, desc, False)
        ST, XR, XF = np.zeros((TC.NSET, TC.NA), dtype=np.int32), np.full((TC.NSET, TC.NA), np.nan), np.zeros((TC.NSET, TC.NA))
        x0 = ml.sy / FE.sig_eq_j2(snorm)
        for t in range(TC.NSET):
            for r in range(TC.NA):
                XR[t, r], ST[t, r] = marched_root(lambda x: float(ml.find_yloc_scalar(x, snorm[r], tex=tex[t])), x0[r])
            syld = FE.sig_eq_j2(mds[t]['sig_ideal'])
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                XF[t] = fsolve(ml.find_yloc, 0.8 * np.mean(syld) * np.ones(TC.NA), args=(snorm, None, 0., 0., 0., tex[t]),
                               xtol=1.e-5)
        ok = (ST == 0) & (np.abs(XF - XR) <= 1.e-4 * np.abs(XR))
        out.update({'ray_%s_status' % desc: ST, 'ray_%s_x_ref' % desc: XR, 'ray_%s_x_fsolve' % desc: XF,
                    'ray_%s_fsolve_ok' % desc: ok, 'ray_%s_x0' % desc: x0})
        r_ref = 0.
        for t in range(TC.NSET):
            sel = ST[t] == 0
            if not np.any(sel):
                continue
            fr = np.array([float(ml.find_yloc_scalar(XR[t, r], snorm[r], tex=tex[t])) for r in np.nonzero(sel)[0]])
            fl, dfl, A = TC.restate(p, snorm[sel], tex[t], XR[t, sel])
            r_ref = max(r_ref, float(np.max(np.abs(fr.astype(TC.LD) - fl) / (A * TC.EPS53))))
        out['ray_%s_r_ref' % desc] = r_ref
        dist = []
        for t in range(TC.NSET):
            sel = ST[t] == 0
            d = np.abs(hills[t].calc_seq(snorm[sel] * XR[t, sel][:, None]) / hills[t].sy - 1.) if np.any(sel) else np.array([np.nan])
            dist.append(float(np.max(d)))
        print('ray_%s: status-0 rays per texture %s, status counts %s; distance to the Hill locus per texture %s; r_ref %.2f; '
              'fsolve converged to the marched root on %d of %d rays' % (
                  desc, np.sum(ST == 0, axis=1).tolist(), np.bincount(ST.ravel(), minlength=4).tolist(),
                  ['%.3f' % v for v in dist], r_ref, int(np.sum(ok)), ok.size))

    assert np.sum(out['ray_GSH_3_status'] == 0) == 432
    assert np.sum(out['ray_GSH_7_status'][:5] == 0) == 360 and np.all(out['ray_GSH_7_status'][5] == 1)
    path = TC.FIXTURE
    np.savez_compressed(path, **out)
    print('wrote', path, '%.0f kB' % (os.path.getsize(path) / 1e3))
    assert os.path.getsize(path) <= 300 * 1000


if __name__ == '__main__':
    sys.exit(main())

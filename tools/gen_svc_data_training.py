#!/usr/bin/env python3
"""Fixture generator for training from Data (Data -> Material.from_data -> train_SVC) -- TEST INFRASTRUCTURE, not product
code.

Runs the unmodified reference (pyLabFEA v4.4.2) and scikit-learn on the build box and writes
``tests/golden/svc_data_training.npz``.  No GPU test reads the reference or imports scikit-learn; they read this file.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_svc_data_training.py

Cases (key prefixes):
  gb_  Goss-Barlat yield stresses (examples/train_goss_barlat.py): Data(sig, wh_data=False).  The 300 yield stresses
       (checked equal to yield_stresses_barlat of svc_gossbarlat.npz), the scale factors of create_sig_data, mat_data
       fields, the scikit-learn fits with shrinking=False (``ns_``) and shrinking=True (``s_``) and ``calib``, the largest
       decision difference between the two on the training points plus 10 000 perturbed points.
  wh_  reduced work hardening (oracle/gen_golden.py::train_hardening: Nlc 40, depl 3e-3, Nseq 8): the load-case arrays,
       every parse_data output, scale_seq / scale_wh, both fits and calib; with the non-shrinking fit installed in the
       reference material: calc_yf / calc_fgrad (with khard) / response rows and the 4 x 4 plane-strain tension trace;
       a 2 x 2 grid search (folds, mean_test_score, best_params_).
  js_  CPFEM JSON (examples/Train_CPFEM/Data_Random_Texture_Test.json, 30 load cases) stored as its 18 component arrays;
       the reference reads the legacy file and the same data rewritten in the newer layout in GPa, with the arguments
       of tests/test_ml.py::test_ml_data.  mat_data of both runs, the non-shrinking fit of train_SVC(C=4, gamma=0.5,
       Fe=0.7, Ce=0.9, Nseq=2) and one ML_full_yf value.  Python's random is seeded before each read (the reference's
       elastic fit permutes the pairs with random.sample).
"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden', 'svc_data_training.npz')
os.environ.setdefault('MPLBACKEND', 'Agg')
sys.path.insert(0, ROOT)

import pylabfea as FE  # noqa: E402  (the reference)
import pylabfea.material as FEM  # noqa: E402
from sklearn import svm  # noqa: E402
from sklearn.model_selection import GridSearchCV, StratifiedKFold  # noqa: E402

from oracle.gen_golden import SolveTracer, solve_record, tension_model  # noqa: E402

assert FE.__version__ == '4.4.2'
REF_SRC = os.path.dirname(os.path.dirname(FE.__file__))
JSON_REF = os.path.join(os.path.dirname(REF_SRC), 'examples', 'Train_CPFEM', 'Data_Random_Texture_Test.json')
BARLAT = [0.81766901, -0.36431565, 0.31238124, 0.84321164, -0.01812166, 0.8320893, 0.35952332,
          0.08127502, 1.29314957, 1.0956107, 0.90916744, 0.27655112, 1.090482, 1.18282173,
          -0.01897814, 0.90539357, 1.88256105, 0.0127306]
COMP = ('11', '22', '33', '23', '13', '12')
MD_KEYS = ('flow_stress', 'plastic_strain', 'lc_indices', 'epc', 'ep_start', 'ep_max', 'peeq_max', 'elast_const',
           'sy_av', 'Nlc', 'Ncyl', 'sig_ideal', 'transition_ind')


@contextlib.contextmanager
def sklearn_svc(shrinking, seen):
    """the reference's SVC with shrinking=..., recording the data handed to fit"""
    orig = svm.SVC

    class SVC(orig):
        def __init__(self, **kw):
            kw.setdefault('shrinking', shrinking)
            super().__init__(**kw)

        def fit(self, X, y, sample_weight=None):
            seen['X'], seen['y'] = np.array(X), np.array(y)
            return super().fit(X, y, sample_weight)
    FEM.svm.SVC = SVC
    try:
        yield
    finally:
        FEM.svm.SVC = orig


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def dual_obj(s):
    K = np.exp(-s._gamma * np.sum((s.support_vectors_[:, None, :] - s.support_vectors_[None, :, :]) ** 2, axis=2))
    a = s.dual_coef_[0]
    return 0.5 * a @ K @ a - np.sum(np.abs(a))


def fit_record(out, pre, s):
    out.update({pre + '_support': s.support_.astype(np.int32), pre + '_dual': s.dual_coef_[0],
                pre + '_intercept': float(s.intercept_[0]), pre + '_n_iter': int(s.n_iter_[0]), pre + '_obj': dual_obj(s)})


def calib(out, name, X, fs, fns, rng):
    P = np.concatenate([X, X[rng.integers(len(X), size=10000)] + 0.05 * rng.normal(size=(10000, X.shape[1]))])
    d1, d2 = fs.decision_function(P), fns.decision_function(P)
    out[name + '_calib'] = float(np.max(np.abs(d1 - d2)))
    out[name + '_calib_flips'] = int(np.sum(np.sign(d1) != np.sign(d2)))
    out[name + '_probe'] = P[len(X):len(X) + 500]
    out[name + '_probe_dec_ns'] = d2[len(X):len(X) + 500]


def ref_seq(Nseq, Fe, Ce):
    return np.append(np.linspace(Fe, Ce, Nseq), np.linspace(2. - Ce, 2. - Fe, Nseq))


def md_record(out, pre, md):
    for k in MD_KEYS:
        if k in md:
            v = md[k]
            out[pre + k] = np.array(v, dtype=float if k != 'lc_indices' and k != 'transition_ind' and k not in
                                    ('Nlc', 'Ncyl') else np.int64)


def train_both(make, train_kw):
    """build the material with make() and train it twice (shrinking False / True); returns {tag: (ml, X, y)}"""
    res = {}
    for tag, shr in (('ns', False), ('s', True)):
        seen = {}
        with sklearn_svc(shr, seen), quiet(), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ml = make()
            ml.train_SVC(**train_kw)
        res[tag] = (ml, seen['X'], seen['y'])
    return res


# ----------------------------------------------------------------------------------------------------------- gb_
def case_gb(out, rng):
    from scipy.optimize import fsolve
    mat_GB = FE.Material(name='Yld2004-18p_from_Goss')
    mat_GB.elasticity(E=151220., nu=0.3)
    mat_GB.plasticity(sy=46.76, barlat=BARLAT, barlat_exp=8)
    sunit = FE.load_cases(number_3d=100, number_6d=200)
    x1 = fsolve(lambda x, s, m: m.calc_seq(s * x[:, None]) - m.sy, np.ones(len(sunit)) * mat_GB.sy,
                args=(sunit, mat_GB), xtol=1.e-5)
    sig = sunit * x1[:, None]
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_gossbarlat.npz'))
    assert np.array_equal(sig, gold['yield_stresses_barlat'])
    C, gamma, Ce, Fe, Nseq = 3.0, 1.5, 0.99, 0.1, 25
    with quiet():
        data = FE.Data(sig, mat_name="Goss-Barlat", wh_data=False)

    def make():
        m = FE.Material('ML-Goss-Barlat_C3.0_G1.5', num=1)
        m.from_data(data.mat_data)
        m.elasticity(C11=mat_GB.C11, C12=mat_GB.C12, C44=mat_GB.C44)
        return m
    r = train_both(make, dict(C=C, gamma=gamma, Ce=Ce, Fe=Fe, Nseq=Nseq, gridsearch=False))
    ml, X, y = r['ns']
    seq = ref_seq(Nseq, Fe, Ce)
    st = (seq[:, None, None] * sig[None]).reshape(-1, 6)
    assert np.array_equal(X, st / ml.scale_seq)
    assert np.array_equal(y, np.repeat(np.where(np.arange(2 * Nseq) < Nseq, -1., 1.), len(sig)))
    out.update(gb_sig=sig, gb_seq=seq, gb_C=C, gb_gamma=gamma, gb_Nseq=Nseq, gb_Fe=Fe, gb_Ce=Ce,
               gb_sy_av=float(data.mat_data['sy_av']), gb_Nlc=int(data.mat_data['Nlc']),
               gb_peeq_max=float(data.mat_data['peeq_max']), gb_lc_indices=np.array(data.mat_data['lc_indices']),
               gb_scale_seq=float(ml.scale_seq), gb_scale_wh=float(ml.scale_wh), gb_CV=np.array(mat_GB.CV),
               gb_C11=mat_GB.C11, gb_C12=mat_GB.C12, gb_C44=mat_GB.C44)
    fit_record(out, 'gb_ns', ml.svm_yf)
    fit_record(out, 'gb_s', r['s'][0].svm_yf)
    calib(out, 'gb', X, r['s'][0].svm_yf, ml.svm_yf, rng)
    return ml


# ----------------------------------------------------------------------------------------------------------- wh_
def wh_lc_data(Nlc=40, epl_max=0.03, depl=3.e-3, khard=1000.0):
    """the load cases of oracle/gen_golden.py::train_hardening (examples/train_hardening.py::create_data)"""
    from scipy.optimize import fsolve
    mat_h = FE.Material(name='Hill-reference', num=1)
    mat_h.elasticity(E=200.e3, nu=0.3)
    mat_h.plasticity(sy=50., rv=[1.2, 1.0, 0.8, 1.0, 1.0, 1.0], khard=khard, sdim=6)
    nl3d = int(Nlc / 3)
    sunit = FE.load_cases(number_3d=nl3d, number_6d=Nlc - nl3d)
    x1 = fsolve(mat_h.find_yloc, np.ones(Nlc) * mat_h.sy, args=(sunit,), xtol=1.e-5)
    sig_ideal = sunit * x1[:, None]
    SV = np.linalg.inv(mat_h.CV)
    lc_data = dict()
    for i, st in enumerate(sig_ideal):
        epl = np.zeros(6)
        peeq = 0.0
        sig_list, epl_list, etot_list = [], [], []
        seq = FE.sig_eq_j2(st)
        su = st / seq
        ind = np.zeros(6, dtype=int)
        for j, v in enumerate(su):
            ind[j] = 1 if v > 0.0 else (2 if v < 0.0 else 0)
        key = f'Us_A{ind[0]}B{ind[1]}C{ind[2]}D{ind[3]}E{ind[4]}F{ind[5]}_HI{i:03d}_NNNNN_Tx_NN'
        dsig = seq / 5
        for j in range(6):
            sg = su * j * dsig
            sig_list.append(sg)
            epl_list.append(np.array(epl))
            etot_list.append(np.dot(SV, sg))
        while peeq < epl_max:
            peeq = FE.eps_eq(epl) + depl
            sg = su * (seq + peeq * khard)
            epl += mat_h.calc_fgrad(sig=sg, epl=epl) * depl
            sig_list.append(sg)
            epl_list.append(np.array(epl))
            etot_list.append(epl + np.dot(SV, sg))
        sig_, epl_, etot_ = np.array(sig_list), np.array(epl_list), np.array(etot_list)
        lc_data[key] = {"Stress": sig_, "Eq_Stress": FE.sig_eq_j2(sig_), "Strain_Plastic": epl_,
                        "Eq_Strain_Plastic": FE.eps_eq(epl_), "Shifted_Strain_Plastic": None,
                        "Strain_Total": etot_, "Eq_Strain_Total": FE.eps_eq(etot_)}
    return lc_data


def case_wh(out, rng):
    epl_max, depl, Nseq, C, gamma = 0.03, 3.e-3, 8, 2.0, 1.5
    lc = wh_lc_data(epl_max=epl_max, depl=depl)
    keys = list(lc)
    out['wh_keys'] = np.array(keys)
    out['wh_lc_len'] = np.array([len(lc[k]['Stress']) for k in keys])
    for f in ('Stress', 'Eq_Stress', 'Strain_Plastic', 'Eq_Strain_Plastic', 'Strain_Total'):
        out['wh_lc_' + f] = np.concatenate([lc[k][f] for k in keys])
    with quiet():
        dd = FE.Data(lc, mat_name='ML_Hill_hardening', epl_start=0.0, epl_crit=0.0, epl_max=epl_max, depl=depl,
                     wh_data=True)
    md_record(out, 'wh_md_', dd.mat_data)
    out.update(wh_epl_max=epl_max, wh_depl=depl, wh_Nseq=Nseq, wh_C=C, wh_gamma=gamma, wh_Fe=0.1, wh_Ce=0.99)

    def make():
        m = FE.Material(name='ML_Hill_hardening_C2.0_G1.5', num=2)
        m.from_data(dd.mat_data)
        return m
    r = train_both(make, dict(C=C, gamma=gamma, Ce=0.99, Fe=0.1, Nseq=Nseq, gridsearch=False))
    ml, X, y = r['ns']
    assert ml.whdat and ml.Ndof == 15 and ml.ind_wh == 6
    out.update(wh_scale_seq=float(ml.scale_seq), wh_scale_wh=float(ml.scale_wh), wh_seq=ref_seq(Nseq, 0.1, 0.99),
               wh_CV=np.array(ml.CV), wh_sy=float(ml.sy))
    Nd = len(dd.mat_data['flow_stress'])
    assert np.array_equal(X[:, 6:12], np.tile(dd.mat_data['plastic_strain'], (2 * Nseq, 1)) / ml.scale_wh)
    assert not np.any(X[:, 12:])
    assert X.shape == (2 * Nseq * Nd, 15)
    fit_record(out, 'wh_ns', ml.svm_yf)
    fit_record(out, 'wh_s', r['s'][0].svm_yf)
    calib(out, 'wh', X, r['s'][0].svm_yf, ml.svm_yf, rng)
    # point functions of the reference material with the non-shrinking fit
    N = 120
    u = rng.normal(size=(N, 6))
    u /= np.linalg.norm(u, axis=1)[:, None]
    sig = u * (ml.sy * rng.uniform(0.3, 1.6, size=N))[:, None]
    e = rng.normal(size=(N, 6))
    e[:, :3] -= e[:, :3].mean(axis=1)[:, None]
    e *= (rng.uniform(0., 0.02, size=N) / FE.eps_eq(e))[:, None]
    e[:20] = 0.
    out['wh_b_sig'], out['wh_b_epl'] = sig, e
    out['wh_b_yf'] = ml.calc_yf(sig, epl=e)
    fg, kh = np.zeros((N, 6)), np.zeros(N)
    for i in range(N):
        fg[i] = ml.calc_fgrad(sig[i], epl=e[i])
        kh[i] = ml.khard
    out['wh_b_fgrad'], out['wh_b_khard'] = fg, kh
    # response at element level (plane strain): from the stress states above with small strain increments
    CV = np.array(ml.CV)
    n = 40
    s0 = sig[:n] * 0.9
    d = rng.normal(size=(n, 6))
    d[:, 3:5] = 0.
    d *= (rng.uniform(1e-5, 4e-4, size=n) / np.linalg.norm(d, axis=1))[:, None]
    kin = rng.uniform(0., 900., size=n)
    res = [[], [], [], []]
    for i in range(n):
        ml.khard = kin[i]
        fy, so, dp, ct = ml.response(s0[i], e[i], d[i], CV)
        for q, v in zip(res, (fy, so, dp, ml.khard)):
            q.append(v)
    out.update(wh_r_sig=s0, wh_r_epl=e[:n], wh_r_deps=d, wh_r_khard_in=kin, wh_r_fy=np.array(res[0]),
               wh_r_sig_out=np.array(res[1]), wh_r_depl=np.array(res[2]), wh_r_khard_out=np.array(res[3]))
    # 4 x 4 plane-strain tension; khard starts at 0 and is carried through the element loop
    ml.khard = 0.
    fe = tension_model(ml, 4, 0.004)
    with quiet(), warnings.catch_warnings(), SolveTracer():
        warnings.simplefilter('ignore')
        fe.solve(min_step=8)
    rec = {}
    solve_record(fe, 'wh4', rec)
    out.update(rec)
    out['wh4_khard_final'] = float(ml.khard)
    print('wh4', fe.nsteps, fe.niter, 'khard', ml.khard)
    # 2 x 2 grid search on the training rows, as setup_yf_SVM_6D runs it
    cvals, gvals = [1., 2.], [1., 1.5]
    grid = GridSearchCV(svm.SVC(), {'C': cvals, 'gamma': gvals}, cv=5, n_jobs=1)
    grid.fit(X, y)
    folds = [te for _, te in StratifiedKFold(5).split(X, y)]
    out.update(wh_gs_cvals=np.array(cvals), wh_gs_gvals=np.array(gvals),
               wh_gs_mean_test_score=grid.cv_results_['mean_test_score'],
               wh_gs_best_C=float(grid.best_params_['C']), wh_gs_best_gamma=float(grid.best_params_['gamma']),
               wh_gs_fold_of=np.concatenate([np.full(len(f), k) for k, f in enumerate(folds)])[
                   np.argsort(np.concatenate(folds))])
    return ml


# ----------------------------------------------------------------------------------------------------------- js_
def js_layouts(raw, tmp):
    """the legacy file as read, and the same data in the newer layout with stresses in GPa"""
    new = {}
    for key, val in raw.items():
        res = val['Results']
        new[key] = {'stress': {'s' + c: list(np.array(res['S' + c]) / 1000.) for c in COMP},
                    'total_strain': {'e' + c: res['E' + c] for c in COMP},
                    'plastic_strain': {'ep' + c: res['Ep' + c] for c in COMP},
                    'units': {'Stress': 'GPa', 'Strain': 'None'}}
    p = os.path.join(tmp, 'js_new.json')
    with open(p, 'w') as fp:
        json.dump(new, fp)
    return p


def case_js(out, rng):
    with open(JSON_REF) as fp:
        raw = json.load(fp)
    keys = list(raw)
    out['js_keys'] = np.array(keys)
    out['js_len'] = np.array([len(raw[k]['Results']['S11']) for k in keys])
    for pre in ('S', 'E', 'Ep'):
        for c in COMP:
            out['js_%s%s' % (pre, c)] = np.concatenate([np.array(raw[k]['Results'][pre + c], dtype=float) for k in keys])
    kw = dict(epl_crit=2.e-3, epl_start=1.e-3, epl_max=0.03, depl=1.e-3, wh_data=True)
    with tempfile.TemporaryDirectory() as tmp:
        files = {'leg': JSON_REF, 'new': js_layouts(raw, tmp)}
        dbs = {}
        for tag, f in files.items():
            random.seed(0)
            with quiet():
                dbs[tag] = FE.Data(f, **kw)
            md_record(out, 'js_%s_md_' % tag, dbs[tag].mat_data)
    db = dbs['leg']
    seen = {}
    with sklearn_svc(False, seen), quiet(), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ml = FE.Material(db.mat_data['Name'], num=1)
        ml.from_data(db.mat_data)
        ml.train_SVC(C=4, gamma=0.5, Fe=0.7, Ce=0.9, Nseq=2, plot=False)
    fit_record(out, 'js_ns', ml.svm_yf)
    out.update(js_scale_seq=float(ml.scale_seq), js_scale_wh=float(ml.scale_wh), js_n=len(seen['y']))
    k0, i0 = keys[0], 150
    sig, epl = db.lc_data[k0]['Stress'][i0], db.lc_data[k0]['Strain_Plastic'][i0]
    out['js_full_yf_khard'] = float(ml.khard)
    with quiet():
        out['js_full_yf'] = float(ml.ML_full_yf(sig=sig, epl=epl))
    out['js_full_yf_sig'], out['js_full_yf_epl'] = sig, epl
    return ml


def main():
    out = {}
    rng = np.random.default_rng(11)
    for name, fn in (('gb', case_gb), ('wh', case_wh), ('js', case_js)):
        t0 = time.time()
        fn(out, rng)
        print('%s: nSV %d / %d, n_iter %d / %d [%.1f s]' % (
            name, len(out[name + '_ns_support']), len(out.get(name + '_s_support', [])), out[name + '_ns_n_iter'],
            out.get(name + '_s_n_iter', -1), time.time() - t0))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, '%.0f kB' % (os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    sys.exit(main())

"""Training from Data on the GPU: Data -> Material.from_data -> train_SVC for the Goss-Barlat yield stresses (gb_), a reduced
work-hardening data set (wh_) and a CPFEM JSON database (js_), against the reference's scikit-learn fits and outputs in
tests/golden/svc_data_training.npz (tools/gen_svc_data_training.py).

Fits: the same support set and iteration count as SVC(shrinking=False), dual coefficients within 1e-6 and the intercept
within 1e-9 (libsvm's own Qfloat rows make the two solvers agree to rounding), the FP64 KKT gap and dual
objective of the device fit; decision values within 2 x calib of the reference's fit (calib: the spread between
scikit-learn's shrinking and non-shrinking fits).  The work-hardening material then runs on the existing kernels: its
point functions and the 4 x 4 plane-strain model against the reference with the non-shrinking fit installed.  The
bars of test_workhard_svc.py (1e-11 .. 1e-13) assume identical parameters.  Measured on an MI355X, the device fits of
all three cases equal scikit-learn's dual coefficients and intercepts exactly (difference 0), and calc_yf differs by
1.2e-15 relative; the bars below are the upper limits of the issue (1e-6 relative for point quantities, 1e-5 for sgl,
identical step and iteration counts), far above what the measured parameter difference can move."""
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_data_cpu import js_json, wh_lc_data  # noqa: E402


@pytest.fixture(scope='module')
def z(golden_dir):
    return np.load(os.path.join(golden_dir, 'svc_data_training.npz'))


def quiet_train(m, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return m.train_SVC(**kw)


def check_fit(m, z, pre):
    s = m.svm_yf
    print('%s: nSV %d, n_iter %d / %d, |d dual| %.2e, |d icpt| %.2e' % (
        pre, len(s.support_), s.n_iter_[0], int(z[pre + '_ns_n_iter']),
        np.max(np.abs(s.dual_coef_[0] - z[pre + '_ns_dual'])) if len(s.support_) == len(z[pre + '_ns_support']) else -1,
        abs(s.intercept_[0] - float(z[pre + '_ns_intercept']))))
    assert np.array_equal(s.support_, z[pre + '_ns_support'])
    assert int(s.n_iter_[0]) == int(z[pre + '_ns_n_iter'])
    assert np.max(np.abs(s.dual_coef_[0] - z[pre + '_ns_dual'])) < 1e-6
    assert abs(s.intercept_[0] - float(z[pre + '_ns_intercept'])) < 1e-9
    assert abs(s.dual_objective_ - float(z[pre + '_ns_obj'])) < 1e-6 * abs(float(z[pre + '_ns_obj']))


def kkt_gap(m, X, y):
    """FP64 m(a) - M(a) of the device's alpha (libsvm's stopping quantity) with the kernel in FP64"""
    s = m.svm_yf
    a = np.zeros(len(y))
    a[s.support_] = np.abs(s.dual_coef_[0])
    yi = -y   # internal labels
    K = lambda rows: np.exp(-s.gamma * np.sum((X[rows][:, None, :] - X[s.support_][None, :, :]) ** 2, axis=2))
    G = np.concatenate([(K(np.arange(k, min(k + 4096, len(y)))) @ (yi[s.support_] * a[s.support_]))
                        for k in range(0, len(y), 4096)]) * yi - 1.
    up = ((yi > 0) & (a < s.C)) | ((yi < 0) & (a > 0))
    lo = ((yi > 0) & (a > 0)) | ((yi < 0) & (a < s.C))
    return np.max(-yi[up] * G[up]) - np.min(-yi[lo] * G[lo])


@pytest.fixture(scope='module')
def gb(z):
    import pylabfea_amd as FE
    d = FE.Data(z['gb_sig'], mat_name='Goss-Barlat', wh_data=False)
    m = FE.Material('ML-Goss-Barlat_C3.0_G1.5')
    m.from_data(d.mat_data)
    m.elasticity(C11=float(z['gb_C11']), C12=float(z['gb_C12']), C44=float(z['gb_C44']))
    quiet_train(m, C=float(z['gb_C']), gamma=float(z['gb_gamma']), Ce=float(z['gb_Ce']), Fe=float(z['gb_Fe']),
                Nseq=int(z['gb_Nseq']))
    return m


@pytest.fixture(scope='module')
def wh(z):
    import pylabfea_amd as FE
    dd = FE.Data(wh_lc_data(z), mat_name='ML_Hill_hardening', epl_start=0.0, epl_crit=0.0,
                 epl_max=float(z['wh_epl_max']), depl=float(z['wh_depl']), wh_data=True)
    m = FE.Material('ML_Hill_hardening_C2.0_G1.5', num=2)
    m.from_data(dd.mat_data)
    quiet_train(m, C=float(z['wh_C']), gamma=float(z['wh_gamma']), Ce=0.99, Fe=0.1, Nseq=int(z['wh_Nseq']))
    return m


@pytest.mark.gpu
def test_goss_barlat_fit(gb, z):
    check_fit(gb, z, 'gb')
    assert gb.whdat is False and gb.Ndof == 6 and gb.scale_seq == gb.msparam[0]['sy_av']
    dec = gb.svm_yf.decision_function(z['gb_probe'])
    assert np.max(np.abs(dec - z['gb_probe_dec_ns'])) < 2 * float(z['gb_calib'])


@pytest.mark.gpu
def test_work_hardening_fit(wh, z):
    check_fit(wh, z, 'wh')
    assert wh.whdat and wh.Ndof == 15 and wh.ind_wh == 6
    assert abs(wh.scale_wh - float(z['wh_scale_wh'])) < 1e-15 and abs(wh.scale_seq - float(z['wh_scale_seq'])) < 1e-12
    dec = wh.svm_yf.decision_function(z['wh_probe'])
    assert np.max(np.abs(dec - z['wh_probe_dec_ns'])) < 2 * float(z['wh_calib'])
    Nseq = int(z['wh_Nseq'])
    X = np.zeros((2 * Nseq * len(z['wh_md_flow_stress']), 15))
    X[:, 0:6] = (z['wh_seq'][:, None, None] * z['wh_md_flow_stress'][None]).reshape(-1, 6) / float(z['wh_scale_seq'])
    X[:, 6:12] = np.tile(z['wh_md_plastic_strain'], (2 * Nseq, 1)) / float(z['wh_scale_wh'])
    y = np.repeat(np.where(np.arange(2 * Nseq) < Nseq, -1., 1.), len(z['wh_md_flow_stress']))
    assert kkt_gap(wh, X, y) < 1e-3 + 1e-9


@pytest.mark.gpu
def test_work_hardening_point_functions(wh, z):
    sy = wh.sy
    yf = wh.calc_yf(z['wh_b_sig'], epl=z['wh_b_epl'])
    print('calc_yf max rel diff %.2e' % (np.max(np.abs(yf - z['wh_b_yf'])) / sy))
    assert np.max(np.abs(yf - z['wh_b_yf'])) < 1e-6 * sy
    for i in range(0, len(z['wh_b_sig']), 9):
        a = wh.calc_fgrad(z['wh_b_sig'][i], epl=z['wh_b_epl'][i])
        assert np.max(np.abs(a - z['wh_b_fgrad'][i])) < 1e-6 * max(1., np.max(np.abs(z['wh_b_fgrad'][i])))
        assert abs(wh.khard - z['wh_b_khard'][i]) < 1e-6 * max(1., abs(z['wh_b_khard'][i]))
    CV = np.array(wh.CV)
    for i in range(0, len(z['wh_r_sig']), 3):
        wh.khard = float(z['wh_r_khard_in'][i])
        fy, so, dp, ct = wh.response(z['wh_r_sig'][i], z['wh_r_epl'][i], z['wh_r_deps'][i], CV)
        assert np.max(np.abs(so - z['wh_r_sig_out'][i])) < 1e-6 * sy
        assert np.max(np.abs(dp - z['wh_r_depl'][i])) < 1e-6 * max(1e-3, np.max(np.abs(z['wh_r_depl'][i])))
        assert abs(wh.khard - z['wh_r_khard_out'][i]) < 1e-6 * max(1., abs(z['wh_r_khard_out'][i]))
    wh.khard = 0.


@pytest.mark.gpu
def test_work_hardening_model_trace(wh, z):
    import pylabfea_amd as FE
    wh.khard = 0.
    fe = FE.Model(dim=2)
    fe.geom([4.], LY=4.)
    fe.assign([wh])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.004 * fe.leny, 'disp')
    fe.mesh(NX=4, NY=4)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=8)
    d = np.max(np.abs(fe.sgl - z['wh4_sgl'])) / np.max(np.abs(z['wh4_sgl']))
    print('4x4: nsteps %d niter %s, sgl max rel diff %.2e, khard %.6g / %.6g' % (
        fe.nsteps, list(fe.niter), d, wh.khard, float(z['wh4_khard_final'])))
    assert fe.nsteps == int(z['wh4_nsteps'])
    assert list(fe.niter) == list(z['wh4_niter'])
    assert d < 1e-5
    assert abs(wh.khard - float(z['wh4_khard_final'])) < 1e-6 * max(1., abs(float(z['wh4_khard_final'])))


@pytest.mark.gpu
def test_work_hardening_grid_search(z):
    import pylabfea_amd as FE
    dd = FE.Data(wh_lc_data(z), epl_start=0.0, epl_crit=0.0, epl_max=float(z['wh_epl_max']), depl=float(z['wh_depl']))
    m = FE.Material('ML')
    m.from_data(dd.mat_data)
    quiet_train(m, C=float(z['wh_C']), gamma=float(z['wh_gamma']), Ce=0.99, Fe=0.1, Nseq=int(z['wh_Nseq']),
                gridsearch=True, cvals=list(z['wh_gs_cvals']), gvals=list(z['wh_gs_gvals']))
    assert m.grid['best_params_'] == {'C': float(z['wh_gs_best_C']), 'gamma': float(z['wh_gs_best_gamma'])}
    # GridSearchCV fits scikit-learn's default SVC (shrinking=True); its decision values differ from the non-shrinking
    # solver's by up to calib, which can move a held-out point across the boundary: on this fixture one point of one fold
    # of candidate (C 2, gamma 1.5) does (0.85758 vs 0.85738).  Bar: one sample per fold, as test_gpu_svc_train.py's.
    folds = [np.nonzero(z['wh_gs_fold_of'] == k)[0] for k in range(5)]
    diff = np.abs(m.grid['mean_test_score'] - z['wh_gs_mean_test_score'])
    print('grid search: max |mean accuracy - scikit-learn| = %.5f' % diff.max())
    assert diff.max() <= 1. / min(len(f) for f in folds) + 1e-12


@pytest.mark.gpu
def test_cpfem_json_fit(z, tmp_path):
    import pylabfea_amd as FE
    db = FE.Data(js_json(z, str(tmp_path / 'db.json'), 'legacy'), epl_crit=2.e-3, epl_start=1.e-3, epl_max=0.03,
                 depl=1.e-3, wh_data=True)
    m = FE.Material(db.mat_data['Name'], num=1)
    m.from_data(db.mat_data)
    quiet_train(m, C=4, gamma=0.5, Fe=0.7, Ce=0.9, Nseq=2)
    assert len(m.svm_yf.support_) and m.svm_yf.fit_status_ == 0
    check_fit(m, z, 'js')
    m.khard = float(z['js_full_yf_khard'])
    f = m.ML_full_yf(z['js_full_yf_sig'], epl=z['js_full_yf_epl'], verb=False)
    assert abs(f - float(z['js_full_yf'])) < 1e-6 * m.sy

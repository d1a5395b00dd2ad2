"""The SVR flow rule on the GPU: k_svr / plfx_svr_fit_batch against the step-for-step NumPy replay
(tools/svc_smo_replay.py::svr, pinned to libsvm by tests/test_svr_replay_cpu.py), k_svr_predict / plfx_svr_predict_multi
against an FP64 sum in the same order, and Material.setup_fgrad_SVM / calc_fgrad / epl_dot / C_tan against the records of
the unmodified reference in tests/golden/svr_gradient.npz (tools/gen_svr_gradient.py).

Solver bars: those of tests/test_gpu_svc_smo.py -- the same status, iteration count and support set, coefficients
within 1e-9 C, rho within 1e-9 max(1, |rho|).  Against libsvm's records (``ns_``, without shrinking): those of
tests/test_svr_replay_cpu.py.

Prediction bar: per column the gauge is A = sum_r |coef_r| (+ |intercept|); the FP64 NumPy evaluation of the same rows in
the same order deviates from its np.longdouble value by r_ref units of A 2^-53, and the GPU may deviate from the FP64
evaluation by 4 max(r_ref, 1) of those units (the scheme of tests/test_gpu_hessian.py).

calc_fgrad bar: the reference's rows come from its SVR fits WITH shrinking, the device follows the fits without; calib_m
records per model the largest prediction difference between the two kinds of fit, in standardised units.  Allowed per
component: 4 max(calib_m, 1e-12) times the scale of the inverse transform.  calib_m is 1.7e-18 for model 0 (both fits took
the same 2953 steps), 8.0e-5 .. 1.0e-4 for the others, so for model 0 the bar is 4e-12 standardised units and asks for the same fit and a
prediction exact to rounding.  Measured on an MI355X: component 0 deviates by 1.1e-16 (7e-5 of its bar), components
1 - 5 by 3.1e-5 .. 4.4e-5 (0.14 .. 0.22 of their bars), khard by 8.2e-3 (0.14 of its bar).  epl_dot and C_tan: the same bar propagated to first order through
pdot = (a.C.deps / h) a and Ct = C - (Ca)(Ca)' / h, h = a.C.a + khard, with absolute values of the partial derivatives at
the reference's a and khard, times 1.01 for the second-order remainder (the bars are below 1e-3 of the values)."""
import importlib.util
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('svc_smo_replay', os.path.join(ROOT, 'tools', 'svc_smo_replay.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

TOL = 1e-3
U = 2.0 ** -53
PLFX_ERR_ARG = -2   # include/plfx.h


def FE():
    import pylabfea_amd
    return pylabfea_amd


@pytest.fixture(scope='module')
def ctx():
    from pylabfea_amd.material import _ctx
    return _ctx()


@pytest.fixture(scope='module')
def z(golden_dir):
    return np.load(os.path.join(golden_dir, 'svr_gradient.npz'))


# ------------------------------------------------------------------------------------------------ solver against the replay
def _problem(seed, l, d=6, noise=0.1):
    """a smooth target with the LAST feature in it, so that a kernel that drops feature d - 1 cannot fit it"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(l, d))
    return X, np.sin(X[:, 0]) + 0.5 * X[:, -1] + noise * rng.normal(size=l)


def _check_vs_replay(dev, ref, C):
    assert dev['status'] == ref['status']
    assert dev['n_iter'] == ref['n_iter_']
    assert np.array_equal(np.nonzero(np.abs(dev['coef']) > 0.)[0], ref['support_'])
    assert np.max(np.abs(dev['coef'] - ref['coef'])) <= 1e-9 * C
    assert abs(dev['rho'] + ref['intercept_']) <= 1e-9 * max(1., abs(ref['intercept_']))
    assert np.all(np.abs(dev['coef']) <= C)
    assert abs(dev['obj'] - ref['obj']) <= 1e-9 * max(1., abs(ref['obj']))


# l: one row, the wave edges, one row more or less than the 512 threads of a block (2l around 1024), several rows per thread
SHAPES = [('l%d' % l, dict(seed=10 + l, l=l)) for l in (1, 63, 64, 65, 511, 513, 1100)] + \
         [('d%d' % d, dict(seed=30 + d, l=300, d=d)) for d in (1, 12, 16)]


@pytest.mark.parametrize('name,kw', SHAPES, ids=[s[0] for s in SHAPES])
def test_solver_matches_replay(ctx, name, kw):
    X, t = _problem(**kw)
    C, g, eps = 1., 0.5 if X.shape[1] <= 6 else 1. / X.shape[1], 0.1
    dev = ctx.svr_fit_batch(X, [np.arange(len(X))], [t], C, g, epsilon=eps, tol=TOL)[0]
    ref = R.svr(X, t, C, g, epsilon=eps, tol=TOL)
    print('%s: l %d d %d: n_iter %d (replay %d), nSV %d (%d), rho %.17g (%.17g)' % (
        name, len(X), X.shape[1], dev['n_iter'], ref['n_iter_'], np.sum(dev['coef'] != 0.), len(ref['support_']), dev['rho'],
        -ref['intercept_']))
    _check_vs_replay(dev, ref, C)
    assert ref['status'] == 0
    if len(X) > 1:
        assert ref['n_iter_'] > 0 and len(ref['support_']) > 0
        gap = R.svr_kkt_gap(X, t, dev['coef'], ref['alpha'], C, g, eps)
        assert gap <= TOL + 2. * np.sum(np.abs(dev['coef'])) * 2. ** -24, gap   # see tests/test_svr_replay_cpu.py


def test_constant_target_has_no_support_vector(ctx):
    """every |t - rho| < eps: the first selection already meets the stopping rule; rho is the midpoint of the bounds"""
    X, _ = _problem(50, 200)
    t = np.full(200, 0.7)
    dev = ctx.svr_fit_batch(X, [np.arange(200)], [t], 1., 0.5, epsilon=0.1, tol=TOL)[0]
    ref = R.svr(X, t, 1., 0.5, epsilon=0.1, tol=TOL)
    _check_vs_replay(dev, ref, 1.)
    assert dev['n_iter'] == 0 and np.all(dev['coef'] == 0.) and dev['status'] == 0
    assert abs(dev['rho'] + 0.7) <= 1e-15      # bounds eps - t and -(eps + t): their midpoint is -t


def test_epsilon_zero(ctx):
    X, t = _problem(51, 150)
    dev = ctx.svr_fit_batch(X, [np.arange(150)], [t], 1., 0.5, epsilon=0., tol=TOL)[0]
    ref = R.svr(X, t, 1., 0.5, epsilon=0., tol=TOL)
    _check_vs_replay(dev, ref, 1.)
    assert len(ref['support_']) > 140          # without a tube nearly every row is a support vector


def test_max_iter_reports_status_1(ctx):
    X, t = _problem(52, 400)
    full = R.svr(X, t, 10., 0.5, epsilon=0.01, tol=1e-4)
    nc = full['n_iter_']
    assert nc > 2048 + 10                      # more than one launch (SMO_CHUNK iterations each)
    for m in (1, 2048, 2049, nc - 1, nc, nc + 1):
        dev = ctx.svr_fit_batch(X, [np.arange(400)], [t], 10., 0.5, epsilon=0.01, tol=1e-4, max_iter=m)[0]
        ref = R.svr(X, t, 10., 0.5, epsilon=0.01, tol=1e-4, max_iter=m)
        assert ref['status'] == (1 if m <= nc else 0) and ref['n_iter_'] == min(m, nc)
        _check_vs_replay(dev, ref, 10.)


def test_seven_unequal_problems_in_one_call(ctx):
    """seven problems on a shared pool of rows (overlapping subsets in their own order, their own C, gamma and epsilon)
    give what seven single calls give, bit for bit, and what the replay gives"""
    rng = np.random.default_rng(60)
    X, t0 = _problem(60, 900, d=12)
    sizes = [900, 1, 64, 513, 300, 37, 700]
    Cs = np.array([1., 5., 0.1, 2., 10., 1., 0.5])
    gs = np.array([0.1, 1., 0.3, 0.05, 0.2, 2., 0.1])
    es = np.array([0.1, 0.01, 0., 0.2, 0.01, 0.05, 0.1])
    probs = [rng.choice(900, s, replace=False) for s in sizes]
    tg = [(k % 3 + 1.) * t0[ix] + k for k, ix in enumerate(probs)]
    batch = ctx.svr_fit_batch(X, probs, tg, Cs, gs, epsilon=es, tol=TOL)
    assert len(set(r['n_iter'] for r in batch)) == 7
    for p, ix in enumerate(probs):
        one = ctx.svr_fit_batch(X, [ix], [tg[p]], Cs[p], gs[p], epsilon=es[p], tol=TOL)[0]
        assert np.array_equal(one['coef'], batch[p]['coef'])
        assert (one['rho'], one['obj'], one['n_iter'], one['status']) == (
            batch[p]['rho'], batch[p]['obj'], batch[p]['n_iter'], batch[p]['status'])
        _check_vs_replay(batch[p], R.svr(X[ix], tg[p], Cs[p], gs[p], epsilon=es[p], tol=TOL), Cs[p])


def test_c_abi_rejects_bad_arguments(ctx):
    from pylabfea_amd import _lib
    X, t = _problem(70, 20)
    ix = np.arange(20)
    for kw in (dict(C=0.), dict(C=-1.), dict(gamma=0.), dict(gamma=-2.), dict(epsilon=-0.01)):
        a = dict(C=1., gamma=0.5, epsilon=0.1)
        a.update(kw)
        with pytest.raises(_lib.PlfxError):
            ctx.svr_fit_batch(X, [ix], [t], a['C'], a['gamma'], epsilon=a['epsilon'])
    with pytest.raises(_lib.PlfxError):
        ctx.svr_fit_batch(np.zeros((20, 17)), [ix], [t], 1., 0.5)
    with pytest.raises(_lib.PlfxError):
        ctx.svr_predict_multi(X, np.zeros((20, 9)), np.zeros(9), 0.5, X)
    coef, rho = np.empty(20), np.empty(1)
    it = np.empty(2, dtype=np.int32)
    off, one = np.array([0, 20], dtype=np.int32), np.ones(1)
    rc = ctx.lib.plfx_svr_fit_batch(ctx.h, 20, 6, _lib._dp(X), 1, _lib._dp(off), _lib._dp(ix.astype(np.int32)), _lib._dp(t),
                                    _lib._dp(one), _lib._dp(one), _lib._dp(-one), _lib.C.c_double(1e-3),
                                    _lib.C.c_int64(-1), _lib._dp(coef), _lib._dp(rho), None, _lib._dp(it), _lib._dp(it[1:]))
    assert rc == PLFX_ERR_ARG and b'epsilon' in ctx.lib.plfx_last_error(ctx.h)


# ------------------------------------------------------------------------------------------------ the fixture fit
def _md(w):
    md = dict(sdim=6, wh_data=True, Name='ML_Hill_hardening')
    for k in ('flow_stress', 'plastic_strain', 'elast_const', 'sy_av', 'peeq_max'):
        md[k] = np.array(w['wh_md_' + k]) if w['wh_md_' + k].ndim else float(w['wh_md_' + k])
    md['Nlc'] = int(w['wh_md_Nlc'])
    return md


@pytest.fixture(scope='module')
def mat(golden_dir, z):
    """the work-hardening material of svc_data_training.npz with the reference's own SVC yield function installed (``wh_ns``:
    training it again is another test's business), then setup_fgrad_SVM"""
    w = np.load(os.path.join(golden_dir, 'svc_data_training.npz'))
    m = FE().Material(name='ML_Hill_hardening_C2.0_G1.5', num=2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m.from_data(_md(w))
    Nseq, ss, sw = int(w['wh_Nseq']), float(w['wh_scale_seq']), float(w['wh_scale_wh'])
    X = np.zeros((2 * Nseq * len(w['wh_md_flow_stress']), 15))
    X[:, 0:6] = (w['wh_seq'][:, None, None] * w['wh_md_flow_stress'][None]).reshape(-1, 6) / ss
    X[:, 6:12] = np.tile(w['wh_md_plastic_strain'], (2 * Nseq, 1)) / sw
    m.set_svc(X[w['wh_ns_support']], w['wh_ns_dual'], float(w['wh_ns_intercept']), float(w['wh_gamma']), ss,
              C=float(w['wh_C']), scale_wh=sw)
    assert m.C_yf == float(z['C']) and m.gam_yf == float(z['gamma']) and m.ML_grad is False
    m.setup_fgrad_SVM()
    return m


def _models(m):
    return [m.svm_grad0, m.svm_grad1, m.svm_grad2, m.svm_grad3, m.svm_grad4, m.svm_grad5, m.svm_khard]


def test_fixture_fit(mat, z):
    assert mat.ML_grad is True
    for pre, sc in (('feat_', mat.sc_feat), ('grad_', mat.sc_grad), ('khard_', mat.sc_khard)):
        assert np.all(np.abs(sc.mean_ - z[pre + 'mean']) <= 1e-15 * np.abs(z[pre + 'mean']))
        assert np.all(np.abs(sc.scale_ - z[pre + 'scale']) <= 1e-15 * z[pre + 'scale'])
    for k, s in enumerate(_models(mat)):
        pre = 'ns%d_' % k
        print('model %d: n_iter %d (libsvm %d), nSV %d (%d), intercept diff %.3g, coef diff %.3g' % (
            k, s.n_iter_[0], int(z[pre + 'n_iter']), len(s.support_), len(z[pre + 'support']),
            abs(s.intercept_[0] - float(z[pre + 'intercept'])),
            np.max(np.abs(s.dual_coef_[0] - z[pre + 'dual'])) if len(s.support_) == len(z[pre + 'support']) else np.nan))
        assert s.fit_status_ == 0
        assert np.array_equal(s.support_, z[pre + 'support'])
        assert int(s.n_iter_[0]) == int(z[pre + 'n_iter'])
        assert abs(s.intercept_[0] - float(z[pre + 'intercept'])) <= 1e-12
        assert np.max(np.abs(s.dual_coef_[0] - z[pre + 'dual'])) <= 1e-6 * np.max(np.abs(z[pre + 'dual']))
        assert s.dual_coef_.shape == (1, len(s.support_)) and s.support_vectors_.shape == (len(s.support_), 12)
    # a model's own predict is the column of the fused call
    P = z['x_sc'][:9]
    one = mat.svm_grad3.predict(P)
    assert one.shape == (9,)
    from pylabfea_amd.material import _ctx
    v = mat._svr
    assert np.array_equal(one, _ctx().svr_predict_multi(v['X'], v['coef'], v['intercept'], v['gamma'], P)[:, 3])


# ------------------------------------------------------------------------------------------------ the prediction kernel
def _predict_ref(X, coef, icpt, g, Q, L=np.float64):
    """sum_r coef[r, m] exp(-g |q - x_r|^2) + icpt[m]: distance feature by feature, rows in order (cumsum adds in order)"""
    out = np.empty((len(Q), coef.shape[1]), dtype=L)
    X, coef, icpt, g = X.astype(L), coef.astype(L), icpt.astype(L), L(g)
    for q in range(len(Q)):
        ss = np.zeros(len(X), dtype=L)
        for f in range(X.shape[1]):
            df = Q[q, f].astype(L) - X[:, f]
            ss = ss + df * df
        out[q] = np.cumsum(coef * np.exp(-g * ss)[:, None], axis=0)[-1] + icpt
    return out


@pytest.fixture(scope='module')
def fixture_models(z):
    n = len(z['x_sc'])
    coef, icpt = np.zeros((n, 8)), np.zeros(8)
    for k in range(7):
        coef[z['ns%d_support' % k], k] = z['ns%d_dual' % k]
        icpt[k] = float(z['ns%d_intercept' % k])
    icpt[7] = 0.3125                             # column 7: no support vector at all
    rng = np.random.default_rng(80)
    Q = z['x_sc'][rng.integers(n, size=1000)] + 0.05 * rng.normal(size=(1000, 12))
    Q[:300] = z['x_sc'][:300]                    # training rows themselves: K = 1 on the diagonal
    ref = _predict_ref(z['x_sc'], coef, icpt, float(z['gamma']), Q)
    refl = _predict_ref(z['x_sc'], coef, icpt, float(z['gamma']), Q, L=np.longdouble)
    return coef, icpt, Q, ref, refl


@pytest.mark.parametrize('m', [1, 7, 8])
def test_predict_multi_against_fp64(ctx, z, fixture_models, m):
    coef, icpt, Q, ref, refl = fixture_models
    cols = list(range(m))
    A = (np.sum(np.abs(coef[:, cols]), axis=0) + np.abs(icpt[cols])).astype(np.longdouble)
    r_ref = float(np.max(np.abs(ref[:, cols].astype(np.longdouble) - refl[:, cols]) / (A * U)))
    units = 4. * max(r_ref, 1.)
    for nq in (1, 15, 17, 1000):
        out = ctx.svr_predict_multi(z['x_sc'], coef[:, cols], icpt[cols], float(z['gamma']), Q[:nq])
        assert out.shape == (nq, m)
        dev = float(np.max(np.abs(out.astype(np.longdouble) - ref[:nq, cols]) / (A * U)))
        devl = float(np.max(np.abs(out.astype(np.longdouble) - refl[:nq, cols]) / (A * U)))
        print('m %d nq %d: %.3f units of A 2^-53 from the FP64 sum, %.3f from np.longdouble (r_ref %.3f, allowed %.3f)' % (
            m, nq, dev, devl, r_ref, units))
        assert dev <= units
        if m == 8:
            assert np.all(out[:, 7] == icpt[7])   # a column of zeros: the intercept, exactly
    assert np.array_equal(ctx.svr_predict_multi(z['x_sc'], coef[:, cols], icpt[cols], float(z['gamma']), Q[:17]),
                          ctx.svr_predict_multi(z['x_sc'], coef[:, cols], icpt[cols], float(z['gamma']), Q[:1000])[:17])


def test_predict_column_alone_equals_column_among_eight(ctx, z, fixture_models):
    """a model's sum does not depend on what else is evaluated in the pass"""
    coef, icpt, Q, _, _ = fixture_models
    all8 = ctx.svr_predict_multi(z['x_sc'], coef, icpt, float(z['gamma']), Q[:65])
    for k in (0, 6, 7):
        one = ctx.svr_predict_multi(z['x_sc'], coef[:, k:k + 1], icpt[k:k + 1], float(z['gamma']), Q[:65])
        assert np.array_equal(one[:, 0], all8[:, k])


# ------------------------------------------------------------------------------------------------ calc_fgrad and its users
def _bars(z):
    cal = np.maximum(z['calib_m'], 1e-12)
    return 4. * cal[:6] * z['grad_scale'], 4. * cal[6] * float(z['khard_scale'][0])


def test_calc_fgrad_against_reference_rows(mat, z):
    bar_a, bar_k = _bars(z)
    sig, epl = z['p_sig'], z['p_epl']
    a = mat.calc_fgrad(sig, epl=epl)
    assert a.shape == (50, 6) and mat.msg['gradient'] == 'SVR gradient'
    assert isinstance(mat.khard, float)
    da = np.max(np.abs(a - z['p_fgrad']), axis=0)
    print('calc_fgrad: deviation per component', da, 'bars', bar_a, 'ratio', da / bar_a)
    assert np.all(da <= bar_a)
    assert abs(mat.khard - z['p_khard'][-1]) <= bar_k          # the batch call leaves khard of its LAST row
    dk = 0.
    for i in range(0, 50, 7):                                  # the (6,) form, point by point
        a1 = mat.calc_fgrad(sig[i], epl=epl[i])
        assert a1.shape == (6,) and np.array_equal(a1, a[i])
        dk = max(dk, abs(mat.khard - z['p_khard'][i]))
    print('khard: deviation %.3e, bar %.3e, ratio %.3f' % (dk, bar_k, dk / bar_k))
    assert dk <= bar_k
    # two rows that differ: khard is the last row's, in either order
    i, j = int(np.argmax(z['p_khard'])), int(np.argmin(z['p_khard']))
    assert abs(z['p_khard'][i] - z['p_khard'][j]) > 100. * bar_k
    mat.calc_fgrad(sig[[i, j]], epl=epl[[i, j]])
    assert abs(mat.khard - z['p_khard'][j]) <= bar_k
    mat.calc_fgrad(sig[[j, i]], epl=epl[[j, i]])
    assert abs(mat.khard - z['p_khard'][i]) <= bar_k
    # the reference's own (5, 6) call
    b = mat.calc_fgrad(sig[:5], epl=epl[:5])
    assert np.all(np.abs(b - z['b_fgrad']) <= bar_a) and abs(mat.khard - float(z['b_khard'])) <= bar_k
    # without epl the reference takes zeros (it records no exception)
    assert str(z['none_exc']) == ''
    a0 = mat.calc_fgrad(sig[0])
    assert np.all(np.abs(a0 - z['none_fgrad']) <= bar_a) and np.array_equal(a0, mat.calc_fgrad(sig[0], epl=np.zeros(6)))
    with pytest.raises(ValueError):
        mat.calc_fgrad(sig[:3], epl=epl[:2])


def test_other_paths_untouched_by_ml_grad(mat, z):
    """ana=True and ML_grad = False take the paths they took before; the device paths refuse while ML_grad is set"""
    sig, epl = z['p_sig'][:4], z['p_epl'][:4]
    kh = mat.khard
    with pytest.raises(NotImplementedError, match='ML_grad'):
        mat.response(sig[0], epl[0], np.full(6, 1e-5), np.asarray(mat.CV))
    mat.ML_grad = False
    try:
        g_svc = mat.calc_fgrad(sig, epl=epl)
        assert mat.msg['gradient'] == 'gradient to ML_yf'
        fy, so, dp, ct = mat.response(sig[0], epl[0], np.full(6, 1e-5), np.asarray(mat.CV))
        assert np.all(np.isfinite(so))
    finally:
        mat.ML_grad = True
        mat.khard = kh
    g_svr = mat.calc_fgrad(sig, epl=epl)
    assert mat.msg['gradient'] == 'SVR gradient' and not np.array_equal(g_svc, g_svr)


def test_epl_dot_and_c_tan(mat, z):
    bar_a, bar_k = _bars(z)
    C = z['CV']
    # the reference's stiffness as it stood in the generator; it is handed to both calls, so mat.CV does not enter
    assert np.allclose(C, np.asarray(mat.CV), rtol=0., atol=1e-12 * np.max(C))
    for n, i in enumerate(z['e_idx']):
        sig, epl, deps = z['p_sig'][i], z['p_epl'][i], z['e_deps'][n]
        a, kh = z['p_fgrad'][i], float(z['e_khard_pdot'][n])
        Ca = C @ a
        h, num = a @ Ca + kh, Ca @ deps
        # pdot = (num / h) a
        dlam = (C @ deps) / h - num * 2. * Ca / h ** 2
        J = (num / h) * np.eye(6) + np.outer(a, dlam)
        bar_p = 1.01 * (np.abs(J) @ bar_a + np.abs(num / h ** 2 * a) * bar_k)
        pd = mat.epl_dot(sig, epl, C, deps)
        dp = np.abs(pd - z['e_pdot'][n])
        assert np.all(dp <= bar_p), (n, dp / bar_p)
        assert abs(mat.khard - kh) <= bar_k
        # Ct = C - Ca Ca' / h
        bar_c = np.abs(np.outer(Ca, Ca)) / h ** 2 * bar_k
        for k in range(6):
            dk = -(np.outer(C[:, k], Ca) + np.outer(Ca, C[:, k])) / h + np.outer(Ca, Ca) * 2. * Ca[k] / h ** 2
            bar_c = bar_c + np.abs(dk) * bar_a[k]
        bar_c *= 1.01
        ct = mat.C_tan(sig, C, epl=epl)
        dc = np.abs(ct - z['e_ctan'][n])
        print('point %d: epl_dot %.3f of its bar, C_tan %.3f of its bar' % (i, np.max(dp / bar_p), np.max(dc / bar_c)))
        assert np.all(dc <= bar_c), (n, np.max(dc / bar_c))
        assert np.max(bar_c) < 1e-2 * np.max(np.abs(C - z['e_ctan'][n]))      # the bars test the plastic part
        assert np.max(bar_p) < 1e-2 * np.max(np.abs(z['e_pdot'][n]))

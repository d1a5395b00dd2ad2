"""Material.response under the SVR flow rule on the GPU (enable_svr_flow, k_response_svr).

1. Against the unmodified reference: every row of tests/golden/svr_response.npz (tools/gen_svr_response.py) through
   Material.response.  The fixture holds each row twice -- scikit-learn's predict, and a plain FP64 sum in the device's
   order -- and their difference ``calib`` is the reference's own noise for that row and output.  Allowed: the same
   ``nsteps`` and 4 max(calib, floor) per output, floor = 1e-12 times the largest magnitude of that output over the
   fixture (§18's convention and margin).  THIS is the yardstick.
2. Against a NumPy transcription of ``response`` at edge shapes of the SVR tables.  A structural check only: the
   transcription drives the project's own point functions (calc_yf, ML_full_yf, calc_seq, plfx_svr_predict_multi), so it
   shares their arithmetic and can tell whether the kernel wires them together as the reference's code does -- not
   whether they are right.
3. The gradient inside ``response`` is plfx_svr_predict_multi's, bit for bit.
4. response_batch equals the single calls bit for bit, at the grid tails.
5. With no rule attached every result is what it was before a rule was ever attached.

Measured on an MI355X: see DESIGN.md §21."""
import os

import numpy as np
import pytest

import svr_flow_cases as SC

pytestmark = pytest.mark.gpu

YF_TOL = 5.e-3          # basic.yf_tolerance
OUTPUTS = ('fy1', 'sig', 'depl', 'ct', 'khard')


def eps_eq(e):
    from pylabfea_amd.basic import eps_eq as f
    return float(f(np.asarray(e, dtype=float)))


@pytest.fixture(scope='module')
def z(golden_dir):
    return np.load(os.path.join(golden_dir, 'svr_gradient.npz'))


@pytest.fixture(scope='module')
def zr(golden_dir):
    return np.load(os.path.join(golden_dir, 'svr_response.npz'))


@pytest.fixture(scope='module')
def ctx():
    from pylabfea_amd.material import _ctx
    return _ctx()


@pytest.fixture(scope='module')
def mat(z):
    """the material of tests/test_gpu_svr.py: the reference's SVC installed, the seven SVRs trained on the device"""
    m = SC.svc_material()
    m.setup_fgrad_SVM()
    for k, s in enumerate([m.svm_grad0, m.svm_grad1, m.svm_grad2, m.svm_grad3, m.svm_grad4, m.svm_grad5, m.svm_khard]):
        assert np.array_equal(s.support_, z['ns%d_support' % k])        # the model the fixture's rows were made by
    return m.enable_svr_flow()


def _single(m, zr, i, khard=None):
    if khard is not None:
        m.khard = khard
    fy, so, dp, ct = m.response(zr['sig'][i], zr['epl'][i], zr['deps'][i], zr['CV'], maxit=int(zr['maxit'][i]))
    return dict(fy1=float(fy), sig=so, depl=dp, ct=ct, khard=m.khard, nsteps=int(m.msg['nsteps']))


@pytest.fixture(scope='module')
def singles(mat, zr):
    """the fixture's rows through Material.response, once; khard set to the recorded entry value before every call"""
    out = [_single(mat, zr, i, float(zr['khard_in'][i])) for i in range(len(zr['sig']))]
    assert mat.msg['gradient'] == 'SVR gradient' and isinstance(mat.khard, float)
    return out


def _floors(zr):
    return dict(fy1=1e-12 * np.max(np.abs(zr['fy1'])), sig=1e-12 * np.max(np.abs(zr['sig_out'])),
                depl=1e-12 * np.max(np.abs(zr['depl'])), ct=1e-12 * np.max(np.abs(zr['grad_stiff'])),
                khard=1e-12 * np.max(np.abs(zr['khard_out'])))


REF_KEY = dict(fy1='fy1', sig='sig_out', depl='depl', ct='grad_stiff', khard='khard_out')


# ------------------------------------------------------------------------------------------------ 1. the reference
def test_against_reference_rows(mat, zr, singles):
    """Figures of the run this docstring was written after are in DESIGN.md §21 (Checks)."""
    floor = _floors(zr)
    n = len(zr['sig'])
    bad, worst = [], dict((k, 0.) for k in OUTPUTS)
    for i in range(n):
        r = singles[i]
        ratios = {}
        for k in OUTPUTS:
            bar = 4. * max(float(zr['calib_' + k][i]), floor[k])
            ratios[k] = float(np.max(np.abs(np.asarray(r[k]) - zr[REF_KEY[k]][i]))) / bar
        print('row %2d branch %d stable %d: nsteps %d (reference %d / %d), deviation in units of the bar: %s' % (
            i, zr['branch'][i], zr['stable'][i], r['nsteps'], zr['nsteps'][i], zr['nsteps2'][i],
            ' '.join('%s %.3g' % (k, ratios[k]) for k in OUTPUTS)))
        assert all(np.all(np.isfinite(np.asarray(r[k]))) for k in OUTPUTS)
        if zr['stable'][i]:
            if r['nsteps'] != zr['nsteps'][i] or max(ratios.values()) > 1.:
                bad.append(i)
            for k in OUTPUTS:
                worst[k] = max(worst[k], ratios[k])
        else:
            assert r['nsteps'] in (zr['nsteps'][i], zr['nsteps2'][i])
    print('worst ratio per output over the stable rows:', worst)
    # elastic calls: CV itself comes back, khard is left alone
    for i in np.nonzero(~zr['plastic'])[0]:
        assert np.array_equal(singles[i]['ct'], zr['CV']) and singles[i]['khard'] == float(zr['khard_in'][i])
    assert not bad, ('rows outside 4 max(calib, floor) or with another nsteps', bad)


def test_khard_is_carried_from_call_to_call(mat, zr, singles):
    """two consecutive calls on one material: the second reads the khard the first left behind"""
    floor = _floors(zr)
    chains = np.nonzero(zr['prev'] >= 0)[0]
    assert len(chains) >= 2
    for j in chains:
        i = int(zr['prev'][j])
        first = _single(mat, zr, i, float(zr['khard_in'][i]))
        assert first['khard'] == singles[i]['khard'] and first['khard'] != float(zr['khard_in'][i])
        assert abs(mat.khard - float(zr['khard_in'][j])) <= 4. * max(float(zr['calib_khard'][i]), floor['khard'])
        second = _single(mat, zr, j)                      # khard not reset
        assert second['nsteps'] == zr['nsteps'][j]
        if mat.khard == singles[j]['khard'] and first['khard'] == float(zr['khard_in'][j]):
            assert np.array_equal(second['sig'], singles[j]['sig'])


# ------------------------------------------------------------------------------------------------ 2. the host replay
def _replay(m, ctx, tab, CV, sig, epl, deps, kh_in, maxit, ulp=False):
    """NumPy transcription of the reference's response (material.py:207-346) with ML_grad set; the yield functions and
    the SVR sums are the façade's own device calls.  ulp: the standardised features moved by one unit in the last place."""
    X, coef, icpt, g, fm, fs, om, osc = tab
    st = dict(K=float(kh_in))

    def grad(s):   # calc_fgrad(sig, epl=epl), :752-764: the normal, and khard overwritten
        x = (np.concatenate((s, epl)) - fm) / fs
        if ulp:
            x = np.nextafter(x, np.inf)
        out = ctx.svr_predict_multi(X, coef, icpt, g, x[None, :])[0]
        st['K'] = float(out[6] * osc[6] + om[6])
        st['array'] = True
        return out[:6] * osc[:6] + om[:6]

    def full(s, e=None):
        """ML_full_yf (:414-516).  Before the call's first gradient evaluation khard is a float and the root is searched;
        after it khard, and with it sflow, x0 and x1 (:467, :474), is ONE (1,) array: both marches work on it in place,
        the bracket test fails and the conservative estimate with the marched value comes back."""
        if not st.get('array'):
            m.khard = st['K']                               # get_sflow reads the current khard
            return float(m.ML_full_yf(s, epl=e, verb=False))
        seq = float(m.calc_seq(s))
        x = m.sy + eps_eq(e) * st['K']
        if seq < 0.01:
            return seq - 0.85 * x
        su = s / seq
        if su[0] * su[1] < -1.e-5:
            x *= 0.5
        while float(m.calc_yf(x * su, epl=e)) >= 0. and x > 0.01:
            x *= 0.98
        while float(m.calc_yf(x * su, epl=e)) < 0. and x < 5. * x:
            x *= 1.02
        return seq - 0.85 * x

    def step(s, d):   # epl_dot and C_tan of one (sub-)step: one gradient evaluation serves both (same point, same value)
        yfun = float(m.calc_yf(s + CV @ d, epl=epl))
        a = grad(s)
        ca = CV @ a
        hh = a @ ca + st['K']
        pdot = np.zeros(6) if yfun <= YF_TOL else (a @ CV @ d / hh) * a
        return pdot, CV - np.outer(ca, ca) / hh

    sig = np.array(sig, dtype=float)
    depl = np.zeros(6)
    toler = YF_TOL * (m.sy + eps_eq(epl) * kh_in)
    dsig = CV @ deps
    st_scal, niter = 1., 0
    fy1 = full(sig + dsig, epl)
    if fy1 < toler:
        return dict(fy1=fy1, sig=sig + dsig, depl=depl, ct=np.array(CV), khard=st['K'], nsteps=0)
    fy0 = float(m.calc_yf(sig, epl=epl))
    if fy0 < -0.15:
        fy0 = full(sig)
        st_scal += fy0 / float(m.calc_seq(dsig))
        deps_el = deps * (1. - st_scal)
        sig = sig + CV @ deps_el
        grad_stiff = CV * (1. - st_scal)
        deps_r = deps - deps_el
    else:
        deps_r = np.array(deps, dtype=float)
        grad_stiff = np.zeros((6, 6))
    ddepl, t_stiff = step(sig, deps_r)
    fy1 = full(sig + t_stiff @ deps_r, epl + depl + ddepl)
    nsteps = 1
    if fy1 > toler:
        deps_r = deps_r / maxit
        nsteps = maxit
    SV = np.zeros((6, 6))
    SV[0:3, 0:3] = np.linalg.inv(CV[0:3, 0:3])
    for i in range(3, 6):
        SV[i, i] = 1. / CV[i, i]
    for niter in range(nsteps):
        ddepl, t_stiff = step(sig, deps_r)
        eplt = epl + depl + ddepl
        sig = sig + t_stiff @ deps_r
        fy1 = full(sig, eplt)
        if fy1 > toler:
            ds = sig * fy1 / float(m.calc_seq(sig))
            sig = sig - ds
            ddepl = ddepl + SV @ ds
            eplt = epl + depl + ddepl
            A = np.array([[deps_r[0], 0., 0., 0., deps_r[2], deps_r[1]],
                          [0., deps_r[1], 0., deps_r[2], 0., deps_r[0]],
                          [0., 0., deps_r[2], deps_r[1], deps_r[0], 0.]])
            x = np.linalg.lstsq(A, ds[0:3], rcond=None)[0]
            Ct = np.zeros((6, 6))
            Ct[0:3, 0:3] = np.array([[x[0], x[5], x[4]], [x[5], x[1], x[3]], [x[4], x[3], x[2]]])
            t_stiff = t_stiff - Ct
            fy1 = full(sig, eplt)
        grad_stiff = grad_stiff + t_stiff * st_scal / nsteps
        depl = depl + ddepl
    return dict(fy1=fy1, sig=sig, depl=depl, ct=grad_stiff, khard=st['K'], nsteps=niter)


def _tables(z, l, case):
    """the first l rows of the fixture's seven fits with its scalers; case 'zero': model 2 has no support vector at all
    (prediction = intercept); 'scale1': a feature and an output without variance (scale 1)"""
    X, coef, icpt, g = SC.svr_tables(z)
    X, coef = np.ascontiguousarray(X[:l]), np.ascontiguousarray(coef[:l])
    fm, fs = np.array(z['feat_mean']), np.array(z['feat_scale'])
    om = np.concatenate((z['grad_mean'], z['khard_mean']))
    osc = np.concatenate((z['grad_scale'], z['khard_scale']))
    if case == 'zero':
        coef[:, 2] = 0.
    if case == 'scale1':
        fs[4] = osc[1] = 1.
    return X, coef, icpt, g, fm, fs, om, osc


def _points(zr):
    """8 points spanning the branches: (row of the fixture, maxit); one sub-divided step keeps the 50 sub-steps"""
    br, ns = zr['branch'], zr['nsteps']
    el = list(np.nonzero(br == 0)[0][:2])
    loc = list(np.nonzero((br == 1) & (ns == 49))[0][:3])
    sp = list(np.nonzero(br == 2)[0][:3])
    return [(i, 5) for i in el + loc[:2] + sp] + [(loc[2], 50)]


@pytest.mark.parametrize('l,case', [(1, ''), (63, ''), (64, 'zero'), (65, 'scale1'), (305, ''), (305, 'zero')],
                         ids=['l1', 'l63', 'l64-zero-model', 'l65-scale-1', 'l305', 'l305-zero-model'])
def test_against_host_replay(ctx, z, zr, l, case):
    """Structural: the replay is the project's own code (see the module docstring); test 1 is the yardstick."""
    m = SC.svc_material()
    CV = np.array(zr['CV'])
    tab = _tables(z, l, case)
    assert len(tab[0]) == l
    pts = _points(zr)
    dev = {}
    for maxit in (5, 50):
        idx = [i for i, mi in pts if mi == maxit]
        m.khard = 0.
        c = m._load(CV)
        c.set_svr_flow(0, *tab)
        assert c.svr_flow_info(0) == (l, 0)
        kin = np.array([zr['khard_in'][i] for i in idx])
        fy, so, dp, ct, ns, ko = c.response(zr['sig'][idx], zr['epl'][idx], zr['deps'][idx], khard_in=kin,
                                            return_khard=True, maxit=maxit)
        assert c.svr_flow_info(0) == (l, 1)
        c.set_svr_flow(0, None)            # the shared point context goes on to the replay (and other tests) without a rule
        for n, i in enumerate(idx):
            dev[i] = dict(fy1=fy[n], sig=so[n], depl=dp[n], ct=ct[n].reshape(6, 6), khard=ko[n], nsteps=int(ns[n]))
    rep = dict((i, _replay(m, ctx, tab, CV, zr['sig'][i], zr['epl'][i], zr['deps'][i], float(zr['khard_in'][i]), mi))
               for i, mi in pts)
    rep2 = dict((i, _replay(m, ctx, tab, CV, zr['sig'][i], zr['epl'][i], zr['deps'][i], float(zr['khard_in'][i]), mi,
                            ulp=True)) for i, mi in pts)
    floor = dict((k, 1e-12 * max(np.max(np.abs(np.asarray(rep[i][k]))) for i, _ in pts)) for k in OUTPUTS)
    bad = []
    for i, mi in pts:
        ratios = {}
        for k in OUTPUTS:
            calib = float(np.max(np.abs(np.asarray(rep[i][k]) - np.asarray(rep2[i][k]))))
            ratios[k] = float(np.max(np.abs(np.asarray(dev[i][k]) - np.asarray(rep[i][k])))) / (4. * max(calib, floor[k]))
        print('l %d %s row %2d maxit %2d: nsteps %d (replay %d, perturbed %d), deviation in units of the bar: %s' % (
            l, case, i, mi, dev[i]['nsteps'], rep[i]['nsteps'], rep2[i]['nsteps'],
            ' '.join('%s %.3g' % (k, ratios[k]) for k in OUTPUTS)))
        assert all(np.all(np.isfinite(np.asarray(dev[i][k]))) for k in OUTPUTS)
        if dev[i]['nsteps'] != rep[i]['nsteps'] or max(ratios.values()) > 1.:
            bad.append(i)
    assert not bad, bad
    assert any(dev[i]['nsteps'] > 0 for i, _ in pts) and any(dev[i]['nsteps'] == 0 for i, _ in pts)


# ------------------------------------------------------------------------------------------------ 3. same function, same bits
def test_gradient_inside_response_is_predict_multi(mat, ctx, zr):
    """From the yield locus (no split) with maxit = 1 every gradient evaluation of the call -- the trial step's and the one
    sub-step's -- is at the entry (sig, epl): the khard left behind is the seventh prediction of plfx_svr_predict_multi on
    the standardised [sig | epl], scaled back on the host, to the last bit.  (A step from the yield locus of this
    material that ends after the trial step alone does not exist: the fixture's search found none, so maxit = 1 it is.)"""
    rows = np.nonzero((zr['branch'] == 1) & (zr['nsteps'] == 49))[0][:3]
    assert len(rows) == 3
    v = mat._svr
    for i in rows:
        sig, epl = zr['sig'][i], zr['epl'][i]
        assert float(mat.calc_yf(sig, epl=epl)) >= -0.15
        mat.khard = float(zr['khard_in'][i])
        mat.response(sig, epl, zr['deps'][i], zr['CV'], maxit=1)
        assert mat.msg['nsteps'] == 0
        x = mat.sc_feat.transform(np.concatenate((sig, epl))[None, :])
        out = ctx.svr_predict_multi(v['X'], v['coef'], v['intercept'], v['gamma'], x)
        want = float(mat.sc_khard.inverse_transform(out[:, 6:7])[0, 0])
        print('row %d: khard left behind %.17g, predicted %.17g' % (i, mat.khard, want))
        assert mat.khard == want and want != float(zr['khard_in'][i])


def test_normal_inside_response_is_predict_multi(mat, ctx, zr, singles):
    """The six components of the normal.  A split call that ends after the trial step takes no correction step, so its
    plastic strain increment is lam a with a = calc_fgrad at the stress the elastic part of the step ends at,
    sig + CV deps (1 - st_scal), st_scal = 1 + ML_full_yf(sig) / calc_seq(CV deps).  The host forms that stress from the
    facade's own ML_full_yf and calc_seq; it differs from the kernel's by rounding (FMA in the kernel's products), at most
    1e-13 of its size, and an RBF model moves by at most sum|coef| sqrt(2 gamma / e) per unit of a standardised feature.
    Allowed per component of the unit vector depl / |depl| against a / |a|: 4 times that bound."""
    rows = np.nonzero(zr['plastic'] & (zr['nsteps'] == 0) & (zr['maxit'] == 50) & (zr['ncorr'] == 0))[0]
    assert len(rows) >= 2
    v = mat._svr
    CV = np.array(zr['CV'])
    lip = np.sum(np.abs(v['coef'][:, :6]), axis=0) * np.sqrt(2. * v['gamma'] / np.e) * mat.sc_grad.scale_
    for i in rows:
        sig, epl, deps = zr['sig'][i], zr['epl'][i], zr['deps'][i]
        kh = mat.khard
        mat.khard = float(zr['khard_in'][i])
        mat.ML_grad = False                       # the yield functions alone; they do not depend on the flow rule
        try:
            fy0 = float(mat.ML_full_yf(sig, verb=False))
            st_scal = 1. + fy0 / float(mat.calc_seq(CV @ deps))
        finally:
            mat.ML_grad = True
            mat.khard = kh
        smid = sig + CV @ (deps * (1. - st_scal))
        x = mat.sc_feat.transform(np.concatenate((smid, epl))[None, :])
        a = mat.sc_grad.inverse_transform(ctx.svr_predict_multi(v['X'], v['coef'], v['intercept'], v['gamma'], x)[:, :6])[0]
        dp = singles[i]['depl']
        dx = 1e-13 * np.sqrt(np.sum((np.concatenate((smid, epl)) / mat.sc_feat.scale_) ** 2))
        bar = 4. * lip * dx / np.linalg.norm(a)
        dev = np.abs(dp / np.linalg.norm(dp) - a / np.linalg.norm(a) * np.sign(dp @ a))
        print('row %d: direction of depl against the normal: deviation %s, bar %s' % (i, dev, bar))
        assert np.all(dev <= bar + 4. * 2. ** -52)


# ------------------------------------------------------------------------------------------------ 4. batch equals single
@pytest.mark.parametrize('N', [1, 31, 33, 65])
def test_batch_equals_single_calls(mat, zr, singles, N):
    n = len(zr['sig'])
    # response_batch has the default maxit: a row recorded with maxit = 5 stands for its twin with the same inputs
    twin = [i if zr['maxit'][i] == 50 else
            next(j for j in range(n) if zr['maxit'][j] == 50 and np.array_equal(zr['deps'][j], zr['deps'][i])
                 and np.array_equal(zr['sig'][j], zr['sig'][i])) for i in range(n)]
    idx = np.resize(np.roll(np.array(twin), -5), N) if N != 31 else np.array(twin)[1:]   # N = 1: a plastic row
    mat.khard = 123.                                   # must not enter: khard_in is given
    c = mat._load(zr['CV'])
    rows, before = c.svr_flow_info(0)
    assert rows == len(mat._svr['X']) == 305
    fy, so, dp, ct, ns, ko = mat.response_batch(zr['sig'][idx], zr['epl'][idx], zr['deps'][idx], zr['CV'],
                                                khard_in=zr['khard_in'][idx], return_khard=True)
    assert c.svr_flow_info(0) == (305, before + 1)     # the launch took the SVR kernel
    assert mat.khard == 123. and ct.shape == (len(idx), 6, 6)
    for n_, i in enumerate(idx):
        r = singles[i]
        assert ns[n_] == r['nsteps'] and fy[n_] == r['fy1'] and ko[n_] == r['khard'], (N, n_, i)
        assert np.array_equal(so[n_], r['sig']) and np.array_equal(dp[n_], r['depl']) and np.array_equal(ct[n_], r['ct'])
    if N == 33:   # the default call: khard on entry is the material's
        mat.khard = float(zr['khard_in'][0])
        out = mat.response_batch(zr['sig'][idx], zr['epl'][idx], zr['deps'][idx], zr['CV'])
        assert len(out) == 5
        same = zr['khard_in'][idx] == zr['khard_in'][0]
        assert np.array_equal(out[1][same], so[same]) and np.array_equal(out[4][same], ns[same])


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
def test_attach_detach_leaves_the_svc_path_as_it_was(mat, zr, singles):
    from pylabfea_amd import _lib
    MI = 5          # five sub-steps instead of 50 in every call here: bit-identity does not need the long chain
    n = len(zr['sig'])
    sig, epl, deps, kin = zr['sig'], zr['epl'], zr['deps'], np.full(n, 37.5)
    svc = SC.svc_material()                            # the same SVC, never trained for a flow rule
    rec = svc._record(np.array(zr['CV']))
    c = _lib.Context(0)
    try:
        c.set_materials([rec])
        assert c.svr_flow_info(0) == (0, 0)
        r0 = c.response(sig, epl, deps, khard_in=kin, return_khard=True, maxit=MI)
        p0 = c.response(sig, epl, deps, maxit=MI)                # the plain entry point
        c.set_svr_flow(0, *mat._svr_flow_tables())
        r1 = c.response(sig, epl, deps, khard_in=kin, return_khard=True, maxit=MI)
        assert c.svr_flow_info(0) == (305, 1)
        pl = zr['plastic']
        assert not np.array_equal(r1[1][pl], r0[1][pl])                 # the rule is followed ...
        assert all(np.array_equal(a[~pl], b[~pl]) for a, b in zip(r0[:5], r1[:5]))   # ... by the plastic points only
        c.set_svr_flow(0, None)
        assert c.svr_flow_info(0) == (0, 0)
        r2 = c.response(sig, epl, deps, khard_in=kin, return_khard=True, maxit=MI)
        p2 = c.response(sig, epl, deps, maxit=MI)
        assert all(np.array_equal(a, b) for a, b in zip(r0, r2)) and all(np.array_equal(a, b) for a, b in zip(p0, p2))
        c.set_svr_flow(0, *mat._svr_flow_tables())
        c.set_materials([rec])                         # a new set of materials detaches every rule
        assert c.svr_flow_info(0) == (0, 0)
        r3 = c.response(sig, epl, deps, khard_in=kin, return_khard=True, maxit=MI)
        assert all(np.array_equal(a, b) for a, b in zip(r0, r3))
        # a mixed batch: material 1 carries a rule, material 0 (the same SVC) none
        c.set_materials([rec, rec])
        c.set_svr_flow(1, *mat._svr_flow_tables())
        mid = (np.arange(n) % 3 == 1).astype(np.int32)
        rm = c.response(sig, epl, deps, mat_id=mid, khard_in=kin, return_khard=True, maxit=MI)
        assert c.svr_flow_info(1) == (305, 1) and c.svr_flow_info(0) == (0, 0)
        for a, b0, b1 in zip(rm, r0, r1):
            assert np.array_equal(a[mid == 0], b0[mid == 0]) and np.array_equal(a[mid == 1], b1[mid == 1])
        # the rule attaches to a work-hardening SVC material only
        hill = _lib.pack_material(_lib.HILL6, zr['CV'], E=200.e3, nu=0.3, sy=50., khard=10., hill=np.ones(6))
        c.set_materials([hill])
        with pytest.raises(_lib.PlfxError, match='PLFX_SVC_WH'):
            c.set_svr_flow(0, *mat._svr_flow_tables())
        with pytest.raises(_lib.PlfxError):
            c.set_svr_flow(1, *mat._svr_flow_tables())
    finally:
        c.close()
    # the façade with the flag off and ML_grad = False: the SVC gradient, bit for bit what the untrained material gives
    kh = mat.khard
    mat.enable_svr_flow(False)
    mat.ML_grad = False
    try:
        for i in np.nonzero(zr['plastic'])[0][:3]:
            mat.khard = svc.khard = 37.5
            a = mat.response(sig[i], epl[i], deps[i], zr['CV'], maxit=MI)
            b = svc.response(sig[i], epl[i], deps[i], zr['CV'], maxit=MI)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and mat.khard == svc.khard
            assert np.array_equal(a[1], r0[1][i]) and a[0] == r0[0][i] and mat.khard == r0[5][i]
    finally:
        mat.ML_grad = True
        mat.enable_svr_flow()
        mat.khard = kh
    # and the flag off with ML_grad set refuses, as before
    mat.enable_svr_flow(False)
    try:
        with pytest.raises(NotImplementedError, match='ML_grad'):
            mat.response(sig[0], epl[0], deps[0], zr['CV'])
    finally:
        mat.enable_svr_flow()
    assert np.array_equal(_single(mat, zr, 5, float(zr['khard_in'][5]))['sig'], singles[5]['sig'])

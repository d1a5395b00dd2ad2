"""Texture-dependent SVC yield functions on the GPU: k_tex_yf / k_tex_yield_scale through the C-ABI and
through Material.calc_yf(tex=) / yield_scale(tex=) / texture_loci, and train_SVC on texture data sets, against
tests/golden/texture_svc.npz (the unmodified reference and scikit-learn, tools/gen_texture_svc.py).

Bars.  (1) values: 4 max(calib, 1e-12 max|yf|), the bar of §21, calib the fixture's spread between scikit-learn's decision
function and a plain FP64 sum.  (2) roots: residual_bar / root_bar of tests/yield_locus_cases.py with U = 4 max(r_ref, 1),
r_ref this fixture's worst |reference - longdouble restatement| in units of A 2^-53.  Fits: the same support set and
iteration count as SVC(shrinking=False), dual coefficients within 1e-6 and the intercept within 1e-9 (the bars of
tests/test_gpu_svc_data_train.py: libsvm's FP32 kernel rows make the two solvers agree to rounding, §12); the scores are
decided (the smallest |decision| is more than 100 calib, asserted at generation) and must match exactly."""
import contextlib
import io
import warnings

import numpy as np
import pytest

import texture_cases as TC
import yield_locus_cases as YC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def z():
    return TC.load()


@pytest.fixture(scope='module')
def ctx():
    from pylabfea_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def dbdir(tmp_path_factory):
    return tmp_path_factory.mktemp('texture_db')


_mats = {}


def material(z, dbdir, desc, dev=False):
    """façade texture material on the fixture's databases with the recorded tables installed (built once)"""
    if (desc, dev) not in _mats:
        import pylabfea_amd as FE
        m, _ = TC.facade(FE, z, dbdir, desc, dev)
        _mats[desc, dev] = TC.install(m, TC.tables(z, desc, dev))
    return _mats[desc, dev]


def set_tables(ctx, p):
    ctx.tex_svc_set(p['sv'], p['dual'], p['intercept'], p['gamma'], p['mean'], p['scale'], dev_only=p['dev_only'])


# ------------------------------------------------------------------------------------------------ (1) calc_yf
@pytest.mark.parametrize('dev', [False, True])
@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_calc_yf_against_fixture(z, dbdir, desc, dev):
    m = material(z, dbdir, desc, dev)
    pre = '%s_%s' % (desc, 'dev' if dev else 'full')
    tex, sig, tid = TC.textures(z, desc), z['probe_sig'], z['probe_tex_id']
    one = m.calc_yf(sig, tex=tex[2])
    rows = m.calc_yf(sig, tex=tex[tid])
    bar = TC.value_bar(z[pre + '_calib'], np.concatenate((z[pre + '_yf_one'], z[pre + '_yf_rows'])))
    r = max(np.max(np.abs(one - z[pre + '_yf_one'])), np.max(np.abs(rows - z[pre + '_yf_rows']))) / bar
    print('%s: worst |calc_yf - reference| / bar (1) = %.4f (bar %.2e)' % (pre, r, bar))
    assert r <= 1.
    assert m.msg['yield_fct'] == 'ML_yf-decision-fct'
    assert m.calc_yf(sig[3], tex=tex[2]) == one[3]                                    # a single stress returns a float
    assert np.array_equal(m.calc_yf(sig, tex=tex[2], pred=True), np.where(one >= 0., 1., -1.))
    assert np.array_equal(m.find_yloc(np.full(64, 0.9), sig, tex=tex[2]), m.calc_yf(0.9 * sig, tex=tex[2]))
    assert m.find_yloc_scalar(0.9, sig[5], tex=tex[1]) == m.calc_yf(0.9 * sig[5], tex=tex[1])
    assert m.calc_seq(sig[0]) > 0.                                                    # the analytic side still runs


# ------------------------------------------------------------------------------------------------ (2) edge shapes
def edge_tables(z, nsv, tdim):
    """tables of nsv vectors and tdim texture columns from the GSH_7 fit (widened for tdim = 10), intercept adjusted"""
    p, tex = TC.tables(z, 'GSH_7'), TC.textures(z, 'GSH_7')
    if tdim > p['tdim']:
        p, tex = TC.widen(p, tex, tdim)
    p = TC.cut(p, nsv=nsv, tdim=tdim)
    tex = np.ascontiguousarray(tex[:, :tdim])
    return TC.cut(p, intercept=TC.crossing_intercept(p, tex[0])), tex


@pytest.mark.parametrize('tdim', [1, 3, 7, 10])
@pytest.mark.parametrize('nsv', [1, 15, 16, 17, 31, 33])
def test_edge_shapes(z, ctx, nsv, tdim):
    p, tex = edge_tables(z, nsv, tdim)
    set_tables(ctx, p)
    info = ctx.tex_svc_info()
    assert (info['nsv'], info['tdim'], info['staged']) == (nsv, tdim, True)
    rng = np.random.default_rng(100 * nsv + tdim)
    sig = z['probe_sig'][rng.permutation(64)] * rng.uniform(0.2, 1.2, size=(64, 1))
    sig = np.concatenate((sig, sig[:1]))                                               # 65 points
    tid = rng.integers(0, TC.NSET, size=65).astype(np.int32)
    full = ctx.tex_svc_yf(sig, tex, tid)
    want = TC.transcribe(p, sig, tex[tid])
    bar = TC.value_bar(z['GSH_7_full_calib'], want)
    print('nsv %d tdim %d: worst |device - transcription| / bar (1) = %.4f' % (nsv, tdim, np.max(np.abs(full - want)) / bar))
    assert np.max(np.abs(full - want)) <= bar
    for n in (1, 31, 33, 65):
        assert np.array_equal(ctx.tex_svc_yf(sig[:n], tex, tid[:n]), full[:n])                 # any batch size
        assert np.array_equal(ctx.tex_svc_yf(sig[65 - n:], tex, tid[65 - n:]), full[65 - n:])  # any position
        assert np.array_equal(ctx.tex_svc_yf(sig[:n], tex[tid[:n]]), full[:n])                 # tex_id = the expanded form
    assert np.array_equal(ctx.tex_svc_yf(sig[::-1], tex, tid[::-1]), full[::-1])
    perm = rng.permutation(65)
    assert np.array_equal(ctx.tex_svc_yf(sig[perm], tex, tid[perm]), full[perm])
    shared = ctx.tex_svc_yf(sig, tex[3:4])
    assert np.array_equal(shared, ctx.tex_svc_yf(sig, tex, np.full(65, 3, dtype=np.int32)))
    # rays of the cut table: a root on rays from inside, the same bits alone and in the batch
    su = sig[:5] / YC.j2(sig[:5])[:, None]
    x0 = np.full((2, 5), 30.)
    x, st = ctx.tex_svc_yield_scale(su, tex[:2], x0)
    assert x.shape == (2, 5) and np.all((st == 0) | (st == 1)) and np.all(np.isnan(x[st != 0]))
    for t in range(2):
        ok = st[t] == 0
        if np.any(ok):
            f, df, A = TC.restate(p, su[ok], tex[t], x[t, ok])
            U = 4. * max(float(z['ray_GSH_7_r_ref']), 1.)
            assert np.all(np.abs(f) <= YC.residual_bar(U, df, A, x[t, ok]))
        for r in range(5):
            x1, s1 = ctx.tex_svc_yield_scale(su[r:r + 1], tex[t:t + 1], x0[:1, :1])
            assert s1[0, 0] == st[t, r] and np.array_equal(x1[0, :1], x[t, r:r + 1], equal_nan=True)
    assert np.sum(st == 0) >= 5                                                         # the intercept keeps a sign change
    # a table padded with zero-coefficient vectors past the LDS limit: read from device memory, the same bits
    q = TC.cut(p, pad=2200 - nsv)
    set_tables(ctx, q)
    assert ctx.tex_svc_info()['staged'] is False and ctx.tex_svc_info()['nsv'] == 2200
    assert np.array_equal(ctx.tex_svc_yf(sig, tex, tid), full)
    x2, st2 = ctx.tex_svc_yield_scale(su, tex[:2], x0)
    assert np.array_equal(st2, st) and np.array_equal(x2, x, equal_nan=True)


def test_call_conventions(z):
    from pylabfea_amd import _lib
    c = _lib.Context(0)
    try:
        sig, tex = z['probe_sig'][:4], TC.textures(z, 'GSH_3')
        assert c.tex_svc_info()['nsv'] == 0
        with pytest.raises(_lib.PlfxError, match='error -3'):                           # PLFX_ERR_STATE before the set
            c.tex_svc_yf(sig, tex[:1])
        with pytest.raises(_lib.PlfxError, match='error -3'):
            c.tex_svc_yield_scale(sig, tex[:1])
        p = TC.cut(TC.tables(z, 'GSH_3'), nsv=40)
        for bad in (dict(gamma=0.), dict(gamma=-1.), dict(scale=np.r_[p['scale'][:8], 0.]), dict(scale=np.r_[p['scale'][:8], np.inf]),
                    dict(scale=np.r_[-1., p['scale'][1:]])):
            with pytest.raises(_lib.PlfxError, match='error -2'):
                set_tables(c, dict(p, **bad))
        with pytest.raises(_lib.PlfxError, match='error -2'):                           # tdim = 11
            c.tex_svc_set(np.zeros((3, 17)), np.ones(3), 0., 1., np.zeros(17), np.ones(17))
        with pytest.raises(_lib.PlfxError, match='error -2'):                           # tdim = 0
            c.tex_svc_set(np.zeros((3, 6)), np.ones(3), 0., 1., np.zeros(6), np.ones(6))
        assert c.tex_svc_info()['nsv'] == 0
        set_tables(c, p)
        assert c.tex_svc_yf(np.zeros((0, 6)), tex[:1]).shape == (0,)                    # n = 0: nothing launched
        x, st = c.tex_svc_yield_scale(np.zeros((0, 6)), tex[:2])
        assert x.shape == (2, 0) and c.tex_svc_info()['yf_launches'] == 0 and c.tex_svc_info()['ray_launches'] == 0
        with pytest.raises(_lib.PlfxError, match='error -2'):
            c.tex_svc_yf(sig, tex[:2])                                                  # neither shared nor one per point
        with pytest.raises(_lib.PlfxError, match='error -2'):
            c.tex_svc_yf(sig, tex[:2], np.array([0, 1, 2, 0], dtype=np.int32))          # index out of range
        y = c.tex_svc_yf(sig, tex[:1])
        # plfx_set_materials leaves the set alone; a second set replaces it; nsv = 0 releases it
        import pylabfea_amd as FE
        m = FE.Material('J2')
        m.elasticity(E=200.e3, nu=0.3)
        m.plasticity(sy=100., sdim=6)
        c.set_materials([m._record(np.array(m.CV))])
        assert np.array_equal(c.tex_svc_yf(sig, tex[:1]), y) and c.tex_svc_info()['yf_launches'] == 2
        set_tables(c, TC.cut(p, nsv=20))
        assert c.tex_svc_info()['nsv'] == 20 and c.tex_svc_info()['yf_launches'] == 0
        assert not np.array_equal(c.tex_svc_yf(sig, tex[:1]), y)
        c.tex_svc_set(None, None, 0., 0., None, None)
        assert c.tex_svc_info()['nsv'] == 0
        with pytest.raises(_lib.PlfxError, match='error -3'):
            c.tex_svc_yf(sig, tex[:1])
        # a non-finite component makes that point NaN and nothing else
        set_tables(c, p)
        bad = np.array(sig)
        bad[1, 2] = np.nan
        yb = c.tex_svc_yf(bad, tex[:1])
        assert np.isnan(yb[1]) and np.array_equal(yb[[0, 2, 3]], y[[0, 2, 3]])
        # x0 = NULL: the search starts at a J2 stress of one stress unit; a hydrostatic ray is degenerate then
        su = sig / YC.j2(sig)[:, None]
        xn, sn = c.tex_svc_yield_scale(su, tex[:2])
        xe, se = c.tex_svc_yield_scale(su, tex[:2], np.tile(1. / YC.j2(su), (2, 1)))
        assert np.array_equal(sn, se) and np.allclose(xn, xe, rtol=1e-12, atol=0., equal_nan=True)
        assert c.tex_svc_yield_scale(np.array([[2., 2., 2., 0., 0., 0.]]), tex[:1])[1].tolist() == [[3]]
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ (3) roots
@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_texture_loci_roots(z, dbdir, desc):
    from pylabfea_amd.material import _ctx
    m = material(z, dbdir, desc)
    p, tex = TC.tables(z, desc), TC.textures(z, desc)
    theta, snorm = TC.snorm()
    m.calc_yf(snorm[:1], tex=tex[0])                                   # the tables are on the device from here on
    n0 = _ctx().tex_svc_info()['ray_launches']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        th, seq, st = m.texture_loci(return_status=True)               # the textures of msparam, in order
    assert _ctx().tex_svc_info()['ray_launches'] == n0 + 1             # all 432 rays in ONE launch
    assert np.array_equal(th, theta) and seq.shape == st.shape == (TC.NSET, TC.NA)
    x = seq                                                            # seq_J2(snorm) = 1: the root is the equivalent stress
    x0 = z['ray_%s_x0' % desc]
    ref_st, xr = z['ray_%s_status' % desc], z['ray_%s_x_ref' % desc]
    bar1 = TC.value_bar(z[desc + '_full_calib'], z[desc + '_full_yf_one'])
    U = 4. * max(float(z['ray_%s_r_ref' % desc]), 1.)
    nclear, r1, r2 = 0, 0., 0.
    for t in range(TC.NSET):
        rst, clear = TC.march_replay(p, snorm, tex[t], x0)
        ok = clear > bar1
        nclear += int(np.sum(ok))
        assert np.array_equal(rst[ok], ref_st[t, ok])                  # the replay is the fixture's search
        assert np.array_equal(st[t, ok], ref_st[t, ok])
        s0 = st[t] == 0
        assert np.all(np.isnan(x[t, ~s0]))
        if np.any(s0):
            xs = m.yield_scale(snorm[s0], tex=tex[t])
            f, df, A = TC.restate(p, snorm[s0], tex[t], xs)
            r1 = max(r1, float(np.max(np.abs(f) / YC.residual_bar(U, df, A, xs))))
            both = s0 & (ref_st[t] == 0)
            f, df, A = TC.restate(p, snorm[both], tex[t], xr[t, both])
            xb = m.yield_scale(snorm[both], tex=tex[t])
            r2 = max(r2, float(np.max(np.abs(xb - xr[t, both]) / YC.root_bar(U, df, A, xr[t, both]))))
    print('%s: %d of 432 rays clear of bar (1); worst residual / bar %.3f, worst |x - x_ref| / bar (2) %.3f' % (desc, nclear, r1, r2))
    assert r1 <= 1. and r2 <= 1.
    if desc == 'GSH_3':
        assert nclear >= 400
    else:
        assert np.all(st[5] == 1) and np.all(np.isnan(seq[5]))         # the hold-out of GSH_7: no bracket on any ray


@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_loci_alone_and_in_one_call(z, ctx, desc):
    """each texture called alone, and each ray called alone, gives the bits of the one call over all of them"""
    p, tex = TC.tables(z, desc), TC.textures(z, desc)
    set_tables(ctx, p)
    _, snorm = TC.snorm()
    x0 = np.ascontiguousarray(np.broadcast_to(z['ray_%s_x0' % desc], (TC.NSET, TC.NA)))
    x, st = ctx.tex_svc_yield_scale(snorm, tex, x0)
    for t in range(TC.NSET):
        xt, stt = ctx.tex_svc_yield_scale(snorm, tex[t:t + 1], x0[t:t + 1])
        assert np.array_equal(stt[0], st[t]) and np.array_equal(xt[0], x[t], equal_nan=True)
        for r in range(TC.NA):
            x1, s1 = ctx.tex_svc_yield_scale(snorm[r:r + 1], tex[t:t + 1], x0[t:t + 1, r:r + 1])
            assert s1[0, 0] == st[t, r] and np.array_equal(x1[0], x[t, r:r + 1], equal_nan=True)


def test_status_paths(z, dbdir):
    m, md = material(z, dbdir, 'GSH_3'), material(z, dbdir, 'GSH_3', True)
    tex = TC.textures(z, 'GSH_3')
    _, snorm = TC.snorm()
    su = snorm[:8]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        good = m.yield_scale(su, tex=tex[0])
        assert np.all(np.isfinite(good)) and len(w) == 0
        bad = np.array(su[:4])
        bad[0] = 0.
        bad[1, 2] = np.nan
        bad[2, 1] = np.inf
        x, st = m.yield_scale(bad, tex=tex[0], return_status=True)
        assert st.tolist() == [3, 3, 3, 0] and np.all(np.isnan(x[:3])) and x[3] == good[3]
        assert len(w) == 1 and '3 of 4' in str(w[0].message)
        x, st = m.yield_scale(su[:3], tex=tex[0], x0=np.array([0., -1., np.nan]), return_status=True)
        assert st.tolist() == [3, 3, 3] and np.all(np.isnan(x))
        tb = np.array(tex[:2])
        tb[1, 0] = np.nan                                               # a non-finite texture: degenerate, that ray only
        x, st = m.yield_scale(su[:2], tex=tb, return_status=True)
        assert st.tolist() == [0, 3] and x[0] == good[0]
        hyd = np.array([[1., 1., 1., 0., 0., 0.]]) * 50.
        assert m.yield_scale(hyd, tex=tex[0], return_status=True)[1].tolist() == [3]     # no start value: seq_J2 = 0
        x, st = md.yield_scale(hyd, tex=tex[0], x0=1., return_status=True)               # dev_only: nothing changes along it
        assert st.tolist() == [1] and np.isnan(x[0])
        # start inside marches up, outside marches down: the same root within bar (2)
        p = TC.tables(z, 'GSH_3')
        xi, si = m.yield_scale(su, tex=tex[0], x0=0.7 * good, return_status=True)
        xo, so = m.yield_scale(su, tex=tex[0], x0=1.3 * good, return_status=True)
        _, df, A = TC.restate(p, su, tex[0], good)
        b2 = YC.root_bar(4. * max(float(z['ray_GSH_3_r_ref']), 1.), df, A, good)
        assert np.all(si == 0) and np.all(so == 0)
        assert np.all(np.abs(xi - good) <= b2) and np.all(np.abs(xo - good) <= b2)
        # a single stress returns floats; yield_stress scales the rays
        x1, s1 = m.yield_scale(su[2], tex=tex[0], return_status=True)
        assert isinstance(x1, float) and s1 == 0 and x1 == good[2]
        assert np.array_equal(m.yield_stress(su, tex=tex[0]), su * good[:, None])


# ------------------------------------------------------------------------------------------------ (4) training
def check_fit(s, z, pre):
    print('%s: nSV %d, n_iter %d / %d, |d dual| %.2e, |d icpt| %.2e' % (
        pre, len(s.support_), s.n_iter_[0], int(z[pre + '_n_iter']),
        np.max(np.abs(s.dual_coef_[0] - z[pre + '_dual'])) if len(s.support_) == len(z[pre + '_support']) else -1,
        abs(s.intercept_[0] - float(z[pre + '_intercept']))))
    assert np.array_equal(s.support_, z[pre + '_support'])
    assert int(s.n_iter_[0]) == int(z[pre + '_n_iter'])
    assert np.max(np.abs(s.dual_coef_[0] - z[pre + '_dual'])) < 1e-6
    assert abs(s.intercept_[0] - float(z[pre + '_intercept'])) < 1e-9


@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_recorded_X_fits(z, ctx, desc):
    """the X scikit-learn was handed (d = 9 and 13) through SVCModel.fit and through plfx_svc_fit_wide on 1, 2, 3 workgroups"""
    from pylabfea_amd.material import SVCModel
    p = TC.tables(z, desc)
    X, y = p['X'], p['y']
    assert X.shape == (960, 6 + p['tdim'])
    s = SVCModel.fit(ctx, X, y, TC.TRAIN_KW['C'], TC.TRAIN_KW['gamma'])
    check_fit(s, z, desc + '_full')
    one = ctx.svc_fit_batch(X, y, [np.arange(len(y))], TC.TRAIN_KW['C'], TC.TRAIN_KW['gamma'])[0]
    for nwg in (1, 2, 3):
        r = ctx.svc_fit_wide(X, y, TC.TRAIN_KW['C'], TC.TRAIN_KW['gamma'], nwg=nwg)
        assert r['n_iter'] == one['n_iter'] and r['rho'] == one['rho'] and np.array_equal(r['alpha'], one['alpha'])


@pytest.fixture(scope='module')
def trained(z, dbdir):
    """train_SVC through the façade from the databases, per descriptor and metric (trained once)"""
    import pylabfea_amd as FE
    out = {}
    for desc in TC.DESCRIPTORS:
        for metric in ('acc', 'mcc'):
            m, _ = TC.facade(FE, z, dbdir, desc)
            with contextlib.redirect_stdout(io.StringIO()):
                sc = m.train_SVC(train_index=list(TC.TRAIN), test_index=list(TC.HOLD), metric=metric, **TC.TRAIN_KW)
            out[desc, metric] = (m, sc)
    return out


@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_train_SVC_from_databases(z, trained, desc):
    pre = desc + '_full'
    for metric in ('acc', 'mcc'):
        m, sc = trained[desc, metric]
        check_fit(m.svm_yf, z, pre)
        assert sc[0] == z[pre + '_' + metric][0] and sc[1] == z[pre + '_' + metric][1], (metric, sc, z[pre + '_' + metric])
    m = trained[desc, 'acc'][0]
    assert m.ML_yf and m.Ndof == 6 + m.tdim and m.C_yf == TC.TRAIN_KW['C'] and m.gam_yf == TC.TRAIN_KW['gamma']
    assert m.scale_seq == pytest.approx(np.mean([md['sy_av'] for md in m.msparam]), rel=1e-15)
    assert np.array_equal(m.svc['sv'], TC.tables(z, desc)['X'][m.svm_yf.support_])
    # the trained material evaluates like the recorded tables
    tex = TC.textures(z, desc)
    bar = TC.value_bar(z[pre + '_calib'], z[pre + '_yf_one'])
    assert np.max(np.abs(m.calc_yf(z['probe_sig'], tex=tex[2]) - z[pre + '_yf_one'])) <= bar
    # two calls on one material upload once: the set is keyed on a digest of its tables
    from pylabfea_amd.material import _ctx
    n = _ctx().tex_svc_info()['yf_launches']
    m.calc_yf(z['probe_sig'], tex=tex[1])
    assert _ctx().tex_svc_info()['yf_launches'] == n + 1


@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_texture_grid_search(z, dbdir, desc):
    import pylabfea_amd as FE
    m, _ = TC.facade(FE, z, dbdir, desc)
    with contextlib.redirect_stdout(io.StringIO()):
        sc = m.train_SVC(gridsearch=True, C=10, gamma=1, Fe=TC.TRAIN_KW['Fe'], Ce=TC.TRAIN_KW['Ce'], Nseq=TC.TRAIN_KW['Nseq'],
                         **TC.GRID)
    g = m.grid
    fold_of = z['gs_%s_fold_of' % desc]
    assert [te.tolist() for _, te in g['folds']] == [np.nonzero(fold_of == k)[0].tolist() for k in range(5)]
    assert [(q['C'], q['gamma']) for q in g['params']] == [(1, 0.5), (1, 1), (10, 0.5), (10, 1)]
    assert np.array_equal(g['split_test_scores'], z['gs_%s_test' % desc])
    assert np.array_equal(g['split_train_scores'], z['gs_%s_train' % desc])
    assert (m.C_yf, m.gam_yf) == (float(z['gs_%s_best_C' % desc]), float(z['gs_%s_best_gamma' % desc]))
    check_fit(m.svm_yf, z, 'gs_' + desc)
    assert sc[0] == float(z['gs_%s_score' % desc]) and sc[1] is None
    with pytest.raises(ValueError, match='Cannot have number of splits n_splits=5'):
        m4 = FE.Material('four')
        with contextlib.redirect_stdout(io.StringIO()):
            m4.from_data(list(m.msparam[:4]))
        m4.train_SVC(gridsearch=True, **TC.GRID)


# ------------------------------------------------------------------------------------------------ (5) the example's loop
@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_example_loop(z, dbdir, desc):
    m = material(z, dbdir, desc)
    tex = TC.textures(z, desc)
    _, snorm = TC.snorm()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, seq, st = m.texture_loci(tex, return_status=True)
        for t in range(TC.NSET):
            x, s1 = m.yield_scale(snorm, tex=tex[t], return_status=True)
            assert np.array_equal(s1, st[t])
            ok = s1 == 0
            assert np.array_equal(YC.j2(snorm[ok] * x[ok, None]), seq[t, ok]) and np.all(np.isnan(seq[t, ~ok]))
            if t == 2:   # one texture per ray: the same bits as the shared form
                xr, sr = m.yield_scale(snorm, tex=np.tile(tex[t], (TC.NA, 1)), return_status=True)
                assert np.array_equal(sr, s1) and np.array_equal(xr, x, equal_nan=True)
    ok = z['ray_%s_fsolve_ok' % desc]
    xf = z['ray_%s_x_fsolve' % desc]
    assert np.all(st[ok] == 0)
    r = np.max(np.abs(seq[ok] - xf[ok]) / np.abs(xf[ok])) / 1e-5       # fsolve's own xtol, relative to x
    print('%s: fsolve converged to the marched root on %d of 432 rays; worst |x - x_fsolve| / (xtol x) = %.3f'
          % (desc, int(np.sum(ok)), r))
    assert r <= 1.

"""Flow rule and stress update of texture materials on the GPU: k_tex_fgrad, k_tex_full_yf and k_tex_response
through the C-ABI and through Material.calc_fgrad / ML_full_yf / response / response_batch / epl_dot / C_tan with ``tex=``.
The reference has none of these for a texture material, so the checks are: the gradient against its NumPy transcription and
against central differences of the device's own calc_yf(tex=); invariances, bit for bit; the reduction to the 6-feature
SVC material, whose functions are held to the reference elsewhere; a host replay of response() on the façade's own functions
(structural); response_batch against single response calls; the conventions of the library.

Bars.  Gradient: 4 max(calib, 1e-12 max|a|), calib a plain FP64 sum against the same sum with every feature moved by one unit
in the last place (texture_flow_cases.calib, as §28 takes it).  Differences: 4 (fd_gap + calib_yf / h), fd_gap the truncation
error measured on the transcription (tests/test_texture_flow_cpu.py), calib_yf the fixture's.  Reduction and replay: 4 max(calib,
1e-12 max|output|) per output, calib the change of the comparison side's own outputs under a move of one unit in the last place;
a point whose nsteps changes under that move is unstable and left out, at most one in eight."""
import numpy as np
import pytest

import texture_cases as TC
import texture_flow_cases as TF
import yield_locus_cases as YC

pytestmark = pytest.mark.gpu

OUTS = ('fy1', 'sig', 'depl', 'ct')


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


def fresh_material(z, dbdir, p, desc='GSH_3'):
    """a façade texture material of its own with the tables p installed"""
    import pylabfea_amd as FE
    m, _ = TC.facade(FE, z, dbdir, desc, p['dev_only'])
    return TC.install(m, p)


def set_tables(ctx, p):
    ctx.tex_svc_set(p['sv'], p['dual'], p['intercept'], p['gamma'], p['mean'], p['scale'], dev_only=p['dev_only'])


def edge_tables(z, nsv, tdim):
    """tables of nsv vectors and tdim texture columns from the GSH_7 fit (widened for tdim = 10), intercept adjusted so that
    the function still changes sign along rays"""
    p, tex = TC.tables(z, 'GSH_7'), TC.textures(z, 'GSH_7')
    if tdim > p['tdim']:
        p, tex = TC.widen(p, tex, tdim)
    p = TC.cut(p, nsv=nsv, tdim=tdim)
    tex = np.ascontiguousarray(tex[:, :tdim])
    return TC.cut(p, intercept=TC.crossing_intercept(p, tex[0])), tex


def j2_record(sy=40.):
    import pylabfea_amd as FE
    m = FE.Material('J2')
    m.elasticity(E=200.e3, nu=0.3)
    m.plasticity(sy=sy, sdim=6)
    return m._record(np.array(m.CV)), np.array(m.CV)


# ------------------------------------------------------------------------------------------------ (1) the transcription
@pytest.mark.parametrize('dev', [False, True])
@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_gradient_against_transcription(z, dbdir, desc, dev):
    m, p = material(z, dbdir, desc, dev), TC.tables(z, desc, dev)
    tex, sig, tid = TC.textures(z, desc), z['probe_sig'], z['probe_tex_id']
    m.khard = 7.
    one = m.calc_fgrad(sig, tex=tex[2])
    assert m.khard == 0. and m.msg['gradient'] == 'gradient to ML_yf'
    rows = m.calc_fgrad(sig, tex=tex[tid])
    want = np.concatenate((TF.gradient(p, sig, tex[2]), TF.gradient(p, sig, tex[tid])))
    cal = max(TF.calib(p, sig, tex[2])[1], TF.calib(p, sig, tex[tid])[1])
    bar = TF.grad_bar(cal, want)
    r = float(np.max(np.abs(np.concatenate((one, rows)) - want))) / bar
    print('%s dev %d: worst |calc_fgrad - transcription| / bar = %.4f (bar %.2e, calib %.2e)' % (desc, dev, r, bar, cal))
    assert r <= 1.
    a3 = m.calc_fgrad(sig[3], tex=tex[2])                                  # a single stress returns (6,)
    assert a3.shape == (6,) and np.array_equal(a3, one[3])
    # epl_dot and C_tan: the host formulas on calc_yf(tex=) and calc_fgrad(tex=)
    CV = np.array(m.CV)
    s, t = sig[5], tex[1]
    a = m.calc_fgrad(s, tex=t)
    ca = CV @ a
    assert np.array_equal(m.C_tan(s, CV, tex=t), CV - np.outer(ca, ca) / (a @ ca + m.khard))
    d = np.linalg.solve(CV, 0.5 * s)
    want_dot = np.zeros(6) if m.calc_yf(s + CV @ d, tex=t) <= TF.YF_TOL else (a @ CV @ d / (a @ CV @ a + m.khard)) * a
    assert np.array_equal(m.epl_dot(s, np.zeros(6), CV, d, tex=t), want_dot)


# ------------------------------------------------------------------------------------------------ (1), (3) edge shapes
@pytest.mark.parametrize('tdim', [1, 3, 7, 10])
@pytest.mark.parametrize('nsv', [1, 15, 16, 17, 33])
def test_gradient_edge_shapes_and_invariances(z, ctx, nsv, tdim):
    p, tex = edge_tables(z, nsv, tdim)
    set_tables(ctx, p)
    assert ctx.tex_svc_info()['staged'] is True
    rng = np.random.default_rng(200 * nsv + tdim)
    sig = z['probe_sig'][rng.permutation(64)] * rng.uniform(0.2, 1.2, size=(64, 1))
    sig = np.concatenate((sig, sig[:1]))                                               # 65 points
    tid = rng.integers(0, TC.NSET, size=65).astype(np.int32)
    full = ctx.tex_svc_fgrad(sig, tex, tid)
    want = TF.gradient(p, sig, tex[tid])
    cal = TF.calib(p, sig, tex[tid])[1]
    for n in (1, 31, 33, 65):
        bar = TF.grad_bar(cal, want[:n])
        got = ctx.tex_svc_fgrad(sig[:n], tex, tid[:n])
        assert float(np.max(np.abs(got - want[:n]))) <= bar, (n, float(np.max(np.abs(got - want[:n]))) / bar)
        assert np.array_equal(got, full[:n])                                                      # any batch size
        assert np.array_equal(ctx.tex_svc_fgrad(sig[65 - n:], tex, tid[65 - n:]), full[65 - n:])  # any position
        assert np.array_equal(ctx.tex_svc_fgrad(sig[:n], tex[tid[:n]]), full[:n])                 # tex_id = the expanded form
    print('nsv %d tdim %d: worst |device - transcription| / bar = %.4f'
          % (nsv, tdim, float(np.max(np.abs(full - want))) / TF.grad_bar(cal, want)))
    assert np.array_equal(ctx.tex_svc_fgrad(sig[::-1], tex, tid[::-1]), full[::-1])
    perm = rng.permutation(65)
    assert np.array_equal(ctx.tex_svc_fgrad(sig[perm], tex, tid[perm]), full[perm])
    shared = ctx.tex_svc_fgrad(sig, tex[3:4])
    assert np.array_equal(shared, ctx.tex_svc_fgrad(sig, tex, np.full(65, 3, dtype=np.int32)))
    # a NaN in one row -- in the stress, in the texture -- makes that row's six values NaN and leaves the other rows' bits
    bad = np.array(sig)
    bad[7, 4] = np.nan
    g = ctx.tex_svc_fgrad(bad, tex, tid)
    assert np.all(np.isnan(g[7])) and np.array_equal(np.delete(g, 7, axis=0), np.delete(full, 7, axis=0))
    trow = np.array(tex[tid])
    trow[11, tdim - 1] = np.inf
    g = ctx.tex_svc_fgrad(sig, trow)
    assert np.all(np.isnan(g[11])) and np.array_equal(np.delete(g, 11, axis=0), np.delete(full, 11, axis=0))
    # a table padded with zero-coefficient vectors past the LDS (2200 rows): read from device memory, the same bits
    set_tables(ctx, TC.cut(p, pad=2200 - nsv))
    assert ctx.tex_svc_info()['staged'] is False and ctx.tex_svc_info()['nsv'] == 2200
    assert np.array_equal(ctx.tex_svc_fgrad(sig, tex, tid), full)


# ------------------------------------------------------------------------------------------------ (2) central differences
@pytest.mark.parametrize('dev', [False, True])
@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_gradient_against_differences_of_the_device(z, dbdir, desc, dev):
    m, p = material(z, dbdir, desc, dev), TC.tables(z, desc, dev)
    tex = TC.textures(z, desc)
    sig, tid = z['probe_sig'][:16], z['probe_tex_id'][:16]                 # the points of the CPU test
    h = 1e-4 * m.sy
    fd_gap = TF.fd_gap(p, sig, tex[tid], h)
    calib_yf = float(z['%s_%s_calib' % (desc, 'dev' if dev else 'full')])
    a = m.calc_fgrad(sig, tex=tex[tid])
    fd = TF.central_differences(lambda s: m.calc_yf(s, tex=np.repeat(tex[tid], 12, axis=0)), sig, h)
    bar = 4. * (fd_gap + calib_yf / h)
    worst = float(np.max(np.abs(a - fd)))
    print('%s dev %d: worst |calc_fgrad - central differences of calc_yf| = %.3e, bar %.3e (fd_gap %.3e, calib_yf / h %.3e)'
          % (desc, dev, worst, bar, fd_gap, calib_yf / h))
    assert worst <= bar


# ------------------------------------------------------------------------------------------------ (4) the 6-feature material
def branch_points(yscale, CV, n_el, n_loc, n_split, n_sub, seed, directions=None):
    """stresses and strain increments over the branches of response: n_el purely elastic steps, n_loc steps from the locus
    (half of them small and radial, half larger and oblique), n_split steps from inside that cross the locus, n_sub large
    oblique steps from the locus that are sub-divided.  yscale(su) -> the factor of the locus along su, NaN where the search
    finds none; directions: candidate stresses (default: random), those with a point on the locus are used in turn."""
    rng = np.random.default_rng(seed)
    n = n_el + n_loc + n_split + n_sub
    u = rng.normal(size=(4 * n, 6)) * np.array([1., 1., 1., 0.5, 0.5, 0.5]) if directions is None else np.asarray(directions)
    su = u / YC.j2(u)[:, None]
    x = np.asarray(yscale(su), dtype=float)
    ok = np.isfinite(x)
    assert np.sum(ok) >= min(n, 4), int(np.sum(ok))
    use = np.arange(n) % int(np.sum(ok))
    su, x = su[ok][use], x[ok][use]
    v = rng.normal(size=(n, 6))
    v = v / np.linalg.norm(v, axis=1)[:, None]
    sig, deps = np.empty((n, 6)), np.empty((n, 6))
    for i in range(n):
        on = x[i] * su[i]
        if i < n_el:
            sig[i], deps[i] = 0.3 * on, np.linalg.solve(CV, 0.2 * on)
        elif i < n_el + n_loc:
            small = (i - n_el) % 2 == 0
            sig[i], deps[i] = on, np.linalg.solve(CV, 0.02 * on) if small else 2.e-4 * v[i]
        elif i < n_el + n_loc + n_split:
            sig[i], deps[i] = 0.5 * on, np.linalg.solve(CV, 0.8 * on) + 1.e-4 * v[i]
        else:
            sig[i], deps[i] = on, 1.5e-3 * v[i]
    return sig, deps


def stable_compare(name, got, ref, ref_moved, cap):
    """got / ref / ref_moved: dicts of arrays over the points with 'nsteps' and OUTS.  Same nsteps everywhere; a point whose
    nsteps changes under the move is unstable (at most cap); the others within 4 max(calib, 1e-12 max|output|)."""
    assert np.array_equal(got['nsteps'], ref['nsteps']), (name, got['nsteps'], ref['nsteps'])
    stable = ref['nsteps'] == ref_moved['nsteps']
    assert np.sum(~stable) <= cap, (name, int(np.sum(~stable)))
    worst = {}
    for k in OUTS:
        g, r, rm = (np.asarray(d[k], dtype=float)[stable].reshape(int(np.sum(stable)), -1) for d in (got, ref, ref_moved))
        cal = float(np.max(np.abs(rm - r)))
        bar = 4. * max(cal, 1e-12 * float(np.max(np.abs(r))))
        worst[k] = float(np.max(np.abs(g - r))) / bar
        print('%s %s: worst / bar = %.4f (bar %.2e, calib %.2e), %d unstable' % (name, k, worst[k], bar, cal, int(np.sum(~stable))))
    assert all(w <= 1. for w in worst.values()), (name, worst)


@pytest.mark.parametrize('dev', [False, True])
def test_reduction_to_the_six_feature_material(z, dbdir, dev, monkeypatch):
    """A texture set with tdim = 1 whose features are those of a 6-feature SVC material, evaluated at tex = c, against that
    material: calc_fgrad, ML_full_yf and response.  The 6-feature side runs in a context of its own on the
    thread-per-point kernels (PLFX_SVC_WAVE=0), whose ML_full_yf is the search the texture policy shares; the 16-lane form
    replaces the yield function along a ray by a sampled polynomial within its own bound.  dev_only: the 'hill' tables written
    on deviatoric vectors (deviatoric_tables): the 6-feature gradient is not projected (material.py:775, 807), so the two
    gradients agree only where the projection is a no-op up to rounding."""
    from pylabfea_amd import _lib
    m6, p6 = YC.facade_ml('hill')
    if dev:
        p6 = TF.deviatoric_tables(p6)
        m6.set_svc(p6['sv'], p6['dual'], p6['intercept'], p6['gamma'], p6['scale_seq'], dev_only=True)
    CV = np.array(m6.CV)
    p7, c = TF.six_feature_as_texture(p6)
    mt = fresh_material(z, dbdir, p7)
    mt.sy, mt.khard, mt.hill, mt.drucker = m6.sy, m6.khard, np.array(m6.hill), m6.drucker
    monkeypatch.setenv('PLFX_SVC_WAVE', '0')
    c6 = _lib.Context(0)
    try:
        c6.set_materials([m6._record(CV)])
        assert c6.svc_info()[0] == 0                                        # no material on the row kernels
        sig, deps = branch_points(lambda su: c6.yield_scale(0, su)[0], CV, 4, 8, 8, 4, seed=5 + dev)
        epl = np.zeros((24, 6))
        maxit = np.array([50] * 20 + [5] * 4)
        moved = np.nextafter(sig, np.inf)

        def six(s):
            out = dict(nsteps=np.empty(24, dtype=int), fy1=np.empty(24), sig=np.empty((24, 6)), depl=np.empty((24, 6)),
                       ct=np.empty((24, 36)))
            for mi in (50, 5):
                sel = maxit == mi
                fy, so, dp, ct, ns = c6.response(s[sel], epl[sel], deps[sel], maxit=mi)
                out['fy1'][sel], out['sig'][sel], out['depl'][sel], out['ct'][sel], out['nsteps'][sel] = fy, so, dp, ct, ns
            return out
        ref, ref_moved = six(sig), six(moved)
        got = dict(nsteps=np.empty(24, dtype=int), fy1=np.empty(24), sig=np.empty((24, 6)), depl=np.empty((24, 6)),
                   ct=np.empty((24, 36)))
        for i in range(24):
            fy, so, dp, ct = mt.response(sig[i], epl[i], deps[i], CV, maxit=int(maxit[i]), tex=c)
            got['fy1'][i], got['sig'][i], got['depl'][i], got['ct'][i], got['nsteps'][i] = fy, so, dp, ct.reshape(36), mt.msg['nsteps']
        print('dev %d: nsteps %s' % (dev, ref['nsteps'].tolist()))
        assert np.all(ref['nsteps'][:4] == 0) and np.all(ref['nsteps'][20:] == 4) and 49 in ref['nsteps'][:20]
        assert np.all(c6.yf(0, sig[12:20]) < -0.15)                         # the split branch is taken
        stable_compare('response dev %d' % dev, got, ref, ref_moved, cap=3)
        # gradient and ML_full_yf at the stresses the update starts from and ends at
        pts = np.concatenate((sig, ref['sig']))
        pm = np.nextafter(pts, np.inf)
        a, a6, a6m = mt.calc_fgrad(pts, tex=c), c6.fgrad(0, pts), c6.fgrad(0, pm)
        bar = 4. * max(float(np.max(np.abs(a6m - a6))), 1e-12 * float(np.max(np.abs(a6))))
        print('dev %d: worst |calc_fgrad(tex=) - 6-feature| / bar = %.4f (bar %.2e)' % (dev, float(np.max(np.abs(a - a6))) / bar, bar))
        assert float(np.max(np.abs(a - a6))) <= bar
        f, (f6, s6), (f6m, _) = mt.ML_full_yf(pts, tex=c, verb=False), c6.full_yf(0, pts), c6.full_yf(0, pm)
        bar = 4. * max(float(np.max(np.abs(f6m - f6))), 1e-12 * float(np.max(np.abs(f6))))
        print('dev %d: worst |ML_full_yf(tex=) - 6-feature| / bar = %.4f (bar %.2e)' % (dev, float(np.max(np.abs(f - f6))) / bar, bar))
        assert float(np.max(np.abs(f - f6))) <= bar and np.all(s6 == 0)
    finally:
        c6.close()


# ------------------------------------------------------------------------------------------------ (5) host replay
REPLAY_CASES = {'fit': None, 'nsv 1 tdim 1': (1, 1), 'nsv 17 tdim 3': (17, 3), 'nsv 33 tdim 10': (33, 10), 'padded': 'pad'}


@pytest.mark.parametrize('case', list(REPLAY_CASES))
def test_response_against_host_replay(z, dbdir, case):
    """Structural: the replay is the reference's response() on the project's own calc_yf / ML_full_yf / calc_fgrad (tex=)."""
    what = REPLAY_CASES[case]
    if what is None or what == 'pad':
        p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
        if what == 'pad':
            p = TC.cut(p, pad=2200 - len(p['sv']))
    else:
        p, tex = edge_tables(z, *what)
    m = fresh_material(z, dbdir, p)
    if isinstance(what, tuple):
        m.sy = 30.                                                          # where the cut tables change sign along rays
    CV = np.array(m.CV)
    ta, tb = (tex[1], tex[4]) if not isinstance(what, tuple) else (tex[0], tex[1])   # (cut tables cross zero at texture 0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                     # (rays without a root: the warning of yield_scale)
        sig, deps = branch_points(lambda su: m.yield_scale(su, x0=np.full(len(su), m.sy), tex=ta), CV, 2, 2, 2, 2, seed=11,
                                  directions=z['probe_sig'])
    texs = [ta, tb] * 4
    maxit = 5
    keys = ('nsteps',) + OUTS
    got, ref, ref_moved = ({k: [] for k in keys} for _ in range(3))
    for i in range(8):
        fy, so, dp, ct = m.response(sig[i], np.zeros(6), deps[i], CV, maxit=maxit, tex=texs[i])
        for k, v in zip(keys, (m.msg['nsteps'], fy, so, dp, ct)):
            got[k].append(np.asarray(v, dtype=float).reshape(-1))
        for dst, ulp in ((ref, False), (ref_moved, True)):
            r = TF.replay(m, CV, sig[i], np.zeros(6), deps[i], texs[i], maxit=maxit, ulp=ulp)
            for k in keys:
                dst[k].append(np.asarray(r[k], dtype=float).reshape(-1))
    got, ref, ref_moved = ({k: np.array(v) for k, v in d.items()} for d in (got, ref, ref_moved))
    for d in (got, ref, ref_moved):
        d['nsteps'] = d['nsteps'].reshape(-1).astype(int)
    print('%s: nsteps %s' % (case, got['nsteps'].tolist()))
    if what is None:
        assert {0, maxit - 1} <= set(got['nsteps'].tolist())
    stable_compare('replay ' + case, got, ref, ref_moved, cap=1)
    info = m._load_tex().tex_svc_info()
    assert info['staged'] == (what != 'pad') and info['nsv'] == len(p['sv'])


# ------------------------------------------------------------------------------------------------ (6) batch against single calls
def test_response_batch_against_single_calls(z, dbdir):
    """On a table of 64 vectors, at textures around the one where the cut table changes sign along rays: a single call runs
    one thread through every vector at every evaluation (257 of them on the whole fit take ten seconds), and where the
    function has no zero every ML_full_yf marches its 400 steps down."""
    import warnings
    p = TC.cut(TC.tables(z, 'GSH_3'), nsv=64)
    tex = TC.textures(z, 'GSH_3')
    m = fresh_material(z, dbdir, TC.cut(p, intercept=TC.crossing_intercept(p, tex[0])))
    m.sy = 30.
    CV = np.array(m.CV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sig8, deps8 = branch_points(lambda su: m.yield_scale(su, x0=np.full(len(su), m.sy), tex=tex[0]), CV, 2, 2, 2, 2, seed=3,
                                    directions=z['probe_sig'])
    rng = np.random.default_rng(17)
    N = 257
    # (a sub-divided point takes one thread through 50 sub-steps over all vectors: few of them among the single calls)
    pick = rng.choice(8, size=N, p=[0.235] * 4 + [0.015] * 4)
    sig = sig8[pick] * rng.uniform(0.9, 1.0, size=(N, 1))
    deps = deps8[pick] * rng.uniform(0.5, 1.0, size=(N, 1))
    epl = np.abs(rng.normal(size=(N, 6))) * 1e-4
    trow = tex[0] + rng.uniform(-0.02, 0.02, size=(N, tex.shape[1]))
    single = []
    for i in range(N):
        fy, so, dp, ct = m.response(sig[i], epl[i], deps[i], CV, tex=trow[i])
        single.append((fy, so, dp, ct, m.msg['nsteps']))
    assert len({s[4] for s in single}) >= 2                                  # more than one branch
    for n in (1, 33, 65, 257):
        fy, so, dp, ct, ns = m.response_batch(sig[:n], epl[:n], deps[:n], CV, tex=trow[:n])
        assert ct.shape == (n, 6, 6)
        for i in range(n):
            assert fy[i] == single[i][0] and np.array_equal(so[i], single[i][1]) and np.array_equal(dp[i], single[i][2])
            assert np.array_equal(ct[i], single[i][3]) and ns[i] == single[i][4]
    # a shared texture against the same texture repeated per row
    shared = m.response_batch(sig[:65], epl[:65], deps[:65], CV, tex=trow[2])
    rows = m.response_batch(sig[:65], epl[:65], deps[:65], CV, tex=np.tile(trow[2], (65, 1)))
    assert all(np.array_equal(a, b) for a, b in zip(shared, rows))
    # a NaN in deps of one row and in the texture of another: those rows NaN with nsteps = -1, every other row's bits unchanged
    full = m.response_batch(sig[:65], epl[:65], deps[:65], CV, tex=trow[:65])
    dbad, tbad = np.array(deps[:65]), np.array(trow[:65])
    dbad[9, 2] = np.nan
    tbad[40, 0] = np.nan
    bad = m.response_batch(sig[:65], epl[:65], dbad, CV, tex=tbad)
    keep = np.delete(np.arange(65), [9, 40])
    for a, b in zip(bad, full):
        assert np.array_equal(a[keep], b[keep])
    assert bad[4][9] == -1 and bad[4][40] == -1
    for a in bad[:4]:
        assert np.all(np.isnan(a[[9, 40]]))


# ------------------------------------------------------------------------------------------------ (7) conventions of the library
def test_library_conventions(z):
    from pylabfea_amd import _lib
    c = _lib.Context(0)
    try:
        sig, tex = z['probe_sig'][:4], TC.textures(z, 'GSH_3')
        e4, d4 = np.zeros((4, 6)), np.full((4, 6), 1e-5)
        rec, CV = j2_record()
        calls = (lambda: c.tex_svc_fgrad(sig, tex[:1]), lambda: c.tex_svc_full_yf(sig, tex[:1]),
                 lambda: c.tex_svc_response(sig, e4, d4, tex[:1]))
        for call in calls:                                                   # PLFX_ERR_STATE before the set
            with pytest.raises(_lib.PlfxError, match='error -3'):
                call()
        p = TC.cut(TC.tables(z, 'GSH_3'), nsv=40)
        set_tables(c, p)
        for call in calls[1:]:                                               # ... and without materials
            with pytest.raises(_lib.PlfxError, match='error -3'):
                call()
        c.set_materials([rec, YC.facade_ml('hill')[0]._record(CV)])
        z0 = np.zeros((0, 6))
        assert c.tex_svc_fgrad(z0, tex[:1]).shape == (0, 6) and c.tex_svc_full_yf(z0, tex[:1])[0].shape == (0,)
        assert c.tex_svc_response(z0, z0, z0, tex[:1])[4].shape == (0,)
        assert c.tex_svc_flow_info() == dict(fgrad_launches=0, full_yf_launches=0, response_launches=0)   # n = 0: nothing launched
        with pytest.raises(_lib.PlfxError, match='error -4'):                # a material of another kind
            c.tex_svc_response(sig, e4, d4, tex[:1], mat=1)
        with pytest.raises(_lib.PlfxError, match='error -2'):
            c.tex_svc_response(sig, e4, d4, tex[:1], mat=2)
        bad_id = np.array([0, 1, 2, 0], dtype=np.int32)
        for call in (lambda: c.tex_svc_fgrad(sig, tex[:2], bad_id), lambda: c.tex_svc_full_yf(sig, tex[:2], bad_id),
                     lambda: c.tex_svc_response(sig, e4, d4, tex[:2], bad_id), lambda: c.tex_svc_fgrad(sig, tex[:2]),
                     lambda: c.tex_svc_full_yf(sig, tex[:3]), lambda: c.tex_svc_response(sig, e4, d4, tex[:2]),
                     lambda: c.tex_svc_response(sig, e4, d4, tex[:1], maxit=0)):
            with pytest.raises(_lib.PlfxError, match='error -2'):
                call()
        assert c.tex_svc_flow_info() == dict(fgrad_launches=0, full_yf_launches=0, response_launches=0)
        g = c.tex_svc_fgrad(sig, tex[:1])
        f, st = c.tex_svc_full_yf(sig, tex[:1])
        r = c.tex_svc_response(sig, e4, d4, tex[:1])
        c.tex_svc_fgrad(sig, tex[:1])
        assert c.tex_svc_flow_info() == dict(fgrad_launches=2, full_yf_launches=1, response_launches=1)
        assert np.array_equal(c.tex_svc_full_yf(sig, tex[:2], np.zeros(4, dtype=np.int32))[0], f)
        # plfx_set_materials after the set leaves the set usable
        c.set_materials([rec])
        assert np.array_equal(c.tex_svc_fgrad(sig, tex[:1]), g) and np.array_equal(c.tex_svc_full_yf(sig, tex[:1])[0], f)
        assert all(np.array_equal(a, b) for a, b in zip(c.tex_svc_response(sig, e4, d4, tex[:1]), r))
        # a non-finite stress: NaN and status 1 for ML_full_yf, nothing else moves
        bad = np.array(sig)
        bad[2, 0] = np.inf
        fb, sb = c.tex_svc_full_yf(bad, tex[:1])
        assert np.isnan(fb[2]) and sb[2] == 1 and np.array_equal(np.delete(fb, 2), np.delete(f, 2))
        # a second set restarts the counters; releasing the set makes all three calls PLFX_ERR_STATE again
        set_tables(c, TC.cut(p, nsv=20))
        assert c.tex_svc_flow_info() == dict(fgrad_launches=0, full_yf_launches=0, response_launches=0)
        c.tex_svc_set(None, None, 0., 0., None, None)
        for call in calls:
            with pytest.raises(_lib.PlfxError, match='error -3'):
                call()
    finally:
        c.close()

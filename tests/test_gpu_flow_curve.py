"""Material.flow_curve and Material.data_curve on the device against tests/golden/flow_curve.npz
(tools/gen_flow_curve.py: the unmodified reference, run (b)) and against the NumPy transcription of
tests/flow_curve_cases.py.

Bars, none taken from what the device returns:
  (F) fixture      per output o in x, epl, yf, hk: |o - o_ref| <= 4 max(calib_o of the curve, 1e-12 max |o_ref| over the
                   fixture): the project's bar of §21 and §28.  hk is pinned twice: the raw value against the plain sums of
                   run (c), and max(hk, 0) against what the reference leaves in Material.khard (run b).  For the Hill
                   curves there is no run (c) (calib = 0), and yf = seq - sflow is a difference of two numbers of the size
                   of the flow stress, so its 1e-12 is taken of max |sflow| = max |x_ref| (su has unit J2 stress, Hill seq
                   of the same order).
  (R) residual     |f_L(x)| <= U A 2^-53 + |f_L'(x)| 2 ulp(x), bar (1) of tests/yield_locus_cases.py with its np.longdouble
                   restatement; U = 4 max(r_ref, 1), r_ref = the reference's own |decision_function - f_L| at its roots in
                   units of A 2^-53, from the fixture alone (edge shapes: r_np of FP64 NumPy, as tests/test_gpu_yield_locus.py).
  (G) gradient     an FP64 sum for a_f in any order is off by at most U G_f 2^-53 =: da_f (G_f the gauge of
                   tests/flow_curve_cases.py); the step e + a depl / eps_eq(a) then by depl (da_f + |n_f| sum da) / eps_eq(a)
                   + 2 ulp(e), n = a / eps_eq(a), since eps_eq(a + da) differs from eps_eq(a) by at most sum |da|.
Measured on an MI355X (2026-10-19), worst ratio to the bar: see DESIGN.md §30."""
import os
import warnings

import numpy as np
import pytest

import flow_curve_cases as FC
import yield_locus_cases as YC

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
DEPL = 1.e-3


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'flow_curve.npz'))


_cache = {}


def wh():
    if 'wh' not in _cache:
        _cache['wh'] = FC.wh_material()
    return _cache['wh']


def raw_runs(fx):
    """the 24 fixture curves on the device, one call per predictor, through the context (x itself, K = max_steps)"""
    if 'raw' not in _cache:
        m, p = wh()
        su = fx['su']
        ctx = m._load()
        n0 = ctx.flow_info()['launches']
        parts = [ctx.flow_curve(0, su, None, max_steps=300, depl=float(fx['depl']), epl_max=float(fx['epl_max']), predictor=pr)
                 for pr in (0., 1000.)]
        assert ctx.flow_info()['launches'] == n0 + 2
        K = fx['hk'].shape[1]
        r = {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
        assert np.all(np.isnan(r['x'][:, K + 1:])) and np.all(np.isnan(r['hk'][:, K:]))     # NaN past the last point
        for k in ('x', 'epl', 'yf'):
            r[k] = r[k][:, :K + 1]
        r['hk'] = r['hk'][:, :K]
        _cache['raw'] = r
    return _cache['raw']


def fbar(fx, key, ref=None, scale=None):
    ref = fx[key] if ref is None else ref
    scale = np.nanmax(np.abs(ref)) if scale is None else scale
    cal = fx['calib_' + key] if ref is not None and 'calib_' + key in fx.files and len(fx['calib_' + key]) == len(ref) else 0.
    return 4. * np.maximum(cal, 1e-12 * scale)


def worst(name, dev, ref, bar):
    bar = np.asarray(bar, dtype=float)
    while bar.ndim and bar.ndim < np.ndim(ref):
        bar = bar[..., None]
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), name
    ratio = np.nanmax(np.abs(dev - ref) / bar)
    print('%s: worst |device - reference| %.3e, worst ratio to the bar %.3f' % (name, np.nanmax(np.abs(dev - ref)), ratio))
    return ratio


def test_fixture_svc_curves(fx):
    m, p = wh()
    r = raw_runs(fx)
    assert np.array_equal(r['nsteps'], fx['nsteps']) and np.all(r['status'] == 0)
    assert worst('x', r['x'], fx['x'], fbar(fx, 'x')) <= 1.
    assert worst('epl', r['epl'], fx['epl'], fbar(fx, 'epl')) <= 1.
    assert worst('yf', r['yf'], fx['yf'], fbar(fx, 'yf')) <= 1.
    assert worst('hk raw', r['hk'], fx['hk_c'], fbar(fx, 'hk', fx['hk_c'])) <= 1.
    assert worst('hk clipped', np.maximum(r['hk'], 0.), fx['hk'], fbar(fx, 'hk')) <= 1.
    # (R): the residual at the device's roots, U from the reference's own roots
    su = fx['su'][fx['dir']]
    ok = ~np.isnan(fx['x'])
    S = np.broadcast_to(su[:, None, :], fx['epl'].shape)[ok]
    f, df, A = YC.restate(p, S, fx['epl'][ok], fx['x'][ok])
    r_ref = float(np.max(np.abs(fx['yf'][ok] - f) / (A * YC.EPS53)))
    U = 4. * max(r_ref, 1.)
    f, df, A = YC.restate(p, S, r['epl'][ok], r['x'][ok])
    r1 = np.abs(f) / YC.residual_bar(U, df, A, r['x'][ok])
    ry = np.abs(r['yf'][ok] - f) / (U * A * YC.EPS53)          # the recorded yf is the function at the root, within its noise
    print('r_ref %.2f; residual: worst ratio to bar (R) %.3f; recorded yf against f_L in units of U A 2^-53: %.3f'
          % (r_ref, float(np.max(r1)), float(np.max(ry))))
    assert np.all(r1 <= 1.) and np.all(ry <= 1.)


def test_facade_dict_and_khard(fx):
    m, p = wh()
    r = raw_runs(fx)
    su = fx['su']
    kh = m.khard
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        d = m.flow_curve(su * 3.7, epl_max=float(fx['epl_max']), predictor=1000., return_status=True)   # normalised inside
    assert m.khard == kh                                     # left alone, unlike calc_fgrad
    K = int(fx['nsteps'][12:].max())
    x = r['x'][12:, :K + 1]
    sun = (su * 3.7) / YC.j2(su * 3.7)[:, None]
    assert set(d) == {'sig', 'epl', 'seq', 'peeq', 'yf', 'hk', 'nsteps', 'status'}
    assert d['sig'].shape == (12, K + 1, 6) and d['hk'].shape == (12, K) and d['seq'].shape == (12, K + 1)
    xs = m._load().flow_curve(0, sun, None, max_steps=300, depl=DEPL, epl_max=float(fx['epl_max']), predictor=1000.)['x'][:, :K + 1]
    assert np.array_equal(d['sig'], sun[:, None, :] * xs[:, :, None], equal_nan=True)
    assert np.allclose(xs, x, rtol=1e-12, atol=0., equal_nan=True)       # the direction's rounding only
    assert np.allclose(d['seq'], xs, rtol=1e-14, equal_nan=True) and np.array_equal(d['nsteps'], fx['nsteps'][12:])
    assert np.allclose(d['peeq'], FC.eps_eq(d['epl']), rtol=1e-15, equal_nan=True)
    one = m.flow_curve(su[6], epl_max=float(fx['epl_max']), predictor=1000.)
    assert one['sig'].shape == (fx['nsteps'][18] + 1, 6) and one['nsteps'] == fx['nsteps'][18] and 'status' not in one
    assert np.array_equal(one['yf'], d['yf'][6, :len(one['yf'])])


def test_fixture_hill_curves(fx):
    mh = FC.hill_material()
    su = fx['su']
    r = mh._load(ana=True).flow_curve(0, su, None, max_steps=300, depl=DEPL, epl_max=float(fx['epl_max']), predictor=0.)
    K = fx['hill_x'].shape[1] - 1
    assert np.array_equal(r['nsteps'], fx['hill_nsteps']) and np.all(r['status'] == 0) and np.all(np.isnan(r['hk']))
    sx = np.nanmax(np.abs(fx['hill_x']))
    assert worst('hill x', r['x'][:, :K + 1], fx['hill_x'], 4e-12 * sx) <= 1.
    assert worst('hill epl', r['epl'][:, :K + 1], fx['hill_epl'], 4e-12 * np.nanmax(np.abs(fx['hill_epl']))) <= 1.
    assert worst('hill yf', r['yf'][:, :K + 1], fx['hill_yf'], 4e-12 * sx) <= 1.
    d = mh.flow_curve(su[0], epl_max=float(fx['epl_max']))
    assert np.array_equal(d['sig'], su[0][None, :] * r['x'][0, :K + 1][:d['sig'].shape[0], None]) and mh.khard == 1000.
    # the closed form: x = get_sflow(epl) / calc_seq(su), to 2 ulp
    xs = (mh.sy + FC.eps_eq(r['epl'][:, :K]) * mh.khard) / mh.calc_seq(su)[:, None]
    assert np.all(np.abs(r['x'][:, :K] - xs)[~np.isnan(xs)] <= 2 * YC.ulp(xs[~np.isnan(xs)]))


def test_structure_bit_for_bit(fx):
    m, p = wh()
    r = raw_runs(fx)
    su = fx['su'][fx['dir']]
    x0 = m.yield_scale(su, epl=np.zeros_like(su), x0=m.sy)
    assert np.array_equal(x0, r['x'][:, 0])
    ok = ~np.isnan(r['x'][:, 1:])
    S = np.broadcast_to(su[:, None, :], r['epl'][:, 1:].shape)[ok]
    xs = m.yield_scale(S, epl=r['epl'][:, 1:][ok], x0=r['x'][:, :-1][ok])          # every step of every curve in one call
    assert np.array_equal(xs, r['x'][:, 1:][ok])
    okp = ~np.isnan(r['x'])
    Sp = np.broadcast_to(su[:, None, :], r['epl'].shape)[okp]
    yf = m.calc_yf(Sp * r['x'][okp][:, None], epl=r['epl'][okp])
    assert worst('yf against calc_yf', r['yf'][okp], yf, np.max(fbar(fx, 'yf'))) <= 1.


def test_gradient_of_one_step(fx):
    m, p = wh()
    su = fx['su']
    ctx = m._load()
    rng = np.random.default_rng(5)
    e0 = 0.004 * rng.normal(size=(12, 6))
    for pred in (0., 1000.):
        for epl0 in (None, e0):
            r = ctx.flow_curve(0, su, epl0, max_steps=1, depl=DEPL, epl_max=np.inf, predictor=pred)
            e = np.zeros((12, 6)) if epl0 is None else epl0
            assert np.all(r['nsteps'] == 1) and np.array_equal(r['epl'][:, 0], e)
            de = r['epl'][:, 1] - e
            # eps_eq(de) = depl to 4 eps; from a strain that is not zero e + de rounds at the size of e, which is added
            rnd = 0. if epl0 is None else 2 * EPS * np.max(np.abs(r['epl'][:, 1]), axis=1)
            assert np.all(np.abs(FC.eps_eq(de) - DEPL) <= 4 * EPS * DEPL + rnd)
            peeq = FC.eps_eq(e) + DEPL
            a, hk = ctx.fgrad_wh(0, su * (r['x'][:, :1] + (peeq * pred)[:, None]), e)
            n = a / FC.eps_eq(a)[:, None]
            assert worst('direction', de, n * DEPL, np.max(fbar(fx, 'epl'))) <= 1.
            assert worst('hk', r['hk'][:, 0], hk, np.max(fbar(fx, 'hk', fx['hk_c']))) <= 1.


EDGE_N, EDGE_K = (1, 3, 4, 5, 64, 65), (0, 1, 2)


@pytest.mark.parametrize('nsv', [1, 15, 16, 17, 31, 33])
@pytest.mark.parametrize('nf,dev_only', [(6, False), (6, True), (15, False), (15, True)])
def test_edge_shapes_against_the_transcription(nf, dev_only, nsv):
    """Tables cut to nsv vectors (the remainders of the trips), each with an intercept chosen from its own tables so that
    the march finds a bracket along most directions (yield_locus_cases.crossing_intercept), N = 1 .. 65 curves and 0 .. 2
    steps.  The run N = 65, max_steps = 2 is checked against the transcription: status and nsteps equal those of its FP64
    chain; at every recorded point the residual meets bar (R); every step meets bar (G) from the point the device recorded
    before it.  Every other N and max_steps must then give the same bits as its part of that run."""
    import pylabfea_amd as FE
    make = FC.wh_material if nf == 15 else FC.svc6_material
    m0, p0 = make(nsv=nsv, dev_only=dev_only)
    su = FE.load_cases(0, 65)
    rng = np.random.default_rng(nsv + nf)
    e0 = 0.003 * rng.normal(size=(65, 6))
    b = YC.crossing_intercept(p0, su[:20], e0[:20], [np.full(20, p0['sy'])])
    m, p = make(nsv=nsv, dev_only=dev_only, intercept=b)
    assert len(p['sv']) == nsv and p['intercept'] == b and p['dev_only'] == dev_only
    ctx = m._load()
    kw = dict(depl=DEPL, epl_max=np.inf, predictor=300.)
    full = ctx.flow_curve(0, su, e0, max_steps=2, **kw)
    tr = [FC.flow_curve(p, su[i], e0[i], max_steps=2, **kw) for i in range(65)]
    assert np.array_equal(full['status'], [t['status'] for t in tr]) and np.array_equal(full['nsteps'], [t['nsteps'] for t in tr])
    assert int(np.sum(full['status'] == 0)) >= 20 and set(full['status']) <= {0, 1}
    r1, r2, r_np = [0.], [0.], 1.
    for i in range(65):
        rec = full['nsteps'][i] + 1 if full['status'][i] == 0 or full['nsteps'][i] > 0 or not np.isnan(full['x'][i, 0]) else 0
        assert np.all(np.isnan(full['x'][i, rec:])) and np.all(np.isnan(full['epl'][i, rec:])) and np.all(np.isnan(full['yf'][i, rec:]))
        if nf == 6:
            assert np.all(np.isnan(full['hk'][i]))
        for k in range(rec):
            x, e = full['x'][i, k], full['epl'][i, k]
            f, df, A = YC.restate(p, su[i:i + 1], e[None], np.array([x]))
            fn = YC.restate(p, su[i:i + 1], e[None], np.array([x]), LD=np.float64)[0]
            r_np = max(r_np, float(np.abs(fn - f)[0] / (A[0] * YC.EPS53)))
    U = 4. * r_np
    for i in range(65):
        for k in range(full['nsteps'][i] + 1 if not np.isnan(full['x'][i, 0]) else 0):
            x, e = full['x'][i, k], full['epl'][i, k]
            f, df, A = YC.restate(p, su[i:i + 1], e[None], np.array([x]))
            r1.append(float(np.abs(f)[0] / YC.residual_bar(U, df, A, np.array([x]))[0]))
            if k < full['nsteps'][i]:
                peeq = FC.eps_eq(e) + DEPL
                a, hk, G, Gh = FC.gradient(p, su[i], e, x + peeq * kw['predictor'], LD=FC.LD)
                ea = FC.eps_eq(a)
                da = U * G * YC.EPS53
                bar = DEPL * (da + np.abs(a / ea) * np.sum(da)) / ea + 2 * YC.ulp(full['epl'][i, k + 1]) + 2 * YC.ulp(e)
                r2.append(float(np.max(np.abs(full['epl'][i, k + 1] - (e + a * DEPL / ea)) / bar)))
                if nf == 15:
                    r2.append(float(abs(full['hk'][i, k] - hk) / (U * Gh * YC.EPS53 + 2 * YC.ulp(float(hk)))))
    print('nf %d dev_only %d nsv %d, intercept %.3g: %d of 65 curves complete, r_np %.2f, worst ratio to bar (R) %.3f, (G) %.3f'
          % (nf, dev_only, nsv, b, int(np.sum(full['status'] == 0)), r_np, max(r1), max(r2)))
    assert max(r1) <= 1. and max(r2) <= 1.
    for N in EDGE_N:
        for K in EDGE_K:
            if (N, K) == (65, 2):
                continue
            r = ctx.flow_curve(0, su[:N], e0[:N], max_steps=K, **kw)
            assert np.array_equal(r['x'], full['x'][:N, :K + 1], equal_nan=True), (N, K)
            assert np.array_equal(r['epl'], full['epl'][:N, :K + 1], equal_nan=True), (N, K)
            assert np.array_equal(r['yf'], full['yf'][:N, :K + 1], equal_nan=True), (N, K)
            assert np.array_equal(r['hk'], full['hk'][:N, :K], equal_nan=True), (N, K)
            assert np.array_equal(r['nsteps'], np.minimum(full['nsteps'][:N], K))
            done = full['nsteps'][:N] >= K       # a curve the full run ended early ends there with its status; else complete
            assert np.array_equal(r['status'], np.where(done & ~np.isnan(full['x'][:N, 0]), 0, full['status'][:N]))


def test_equal_bits_at_any_n_and_position(fx):
    m, p = wh()
    su = np.tile(fx['su'], (6, 1))[:65]
    ctx = m._load()
    kw = dict(max_steps=4, depl=DEPL, epl_max=np.inf, predictor=1000.)
    full = ctx.flow_curve(0, su, None, **kw)
    assert np.all(full['nsteps'] == 4)                                   # epl_max = inf: exactly max_steps steps
    perm = np.random.default_rng(3).permutation(65)
    for idx in (np.arange(65)[::-1], perm, np.array([7]), np.arange(12, 17)):
        r = ctx.flow_curve(0, su[idx], None, **kw)
        for k in ('x', 'epl', 'yf', 'hk', 'nsteps', 'status'):
            assert np.array_equal(r[k], full[k][idx]), k
    for k in ('x', 'epl', 'yf', 'hk'):
        assert np.array_equal(full[k][:12], full[k][12:24]) and not np.any(np.isnan(full[k]))
    r20 = ctx.flow_curve(0, su[:3], None, max_steps=20, depl=DEPL, epl_max=np.inf, predictor=0.)
    assert np.all(r20['nsteps'] == 20) and np.all(r20['status'] == 0) and not np.any(np.isnan(r20['x']))
    r0 = ctx.flow_curve(0, su[:3], None, max_steps=0, depl=DEPL, epl_max=np.inf, predictor=0.)
    assert np.all(r0['nsteps'] == 0) and r0['hk'].shape == (3, 0) and np.array_equal(r0['x'][:, 0], r20['x'][:, 0])


def test_table_too_large_for_lds(fx):
    """the table padded with zero-weight vectors beyond what the LDS of a CU holds (16 doubles per vector, 20480 doubles at
    most): read from device memory; the padding adds exact zeros to the same partial sums of the decision function and of
    the gradient: the same bits"""
    m, p = wh()
    pad = 1400 - len(p['sv'])
    mp, _ = FC.wh_material()
    mp.set_svc(np.vstack((p['sv'], np.tile(p['sv'][:1], (pad, 1)))), np.concatenate((p['dual'], np.zeros(pad))), p['intercept'],
               p['gamma'], p['scale_seq'], C=mp.C_yf, scale_wh=p['scale_wh'])
    mp.ML_grad = False
    assert len(mp.svc['sv']) * 16 > 20480
    kw = dict(max_steps=3, depl=DEPL, epl_max=np.inf, predictor=1000.)
    a = m._load().flow_curve(0, fx['su'], None, **kw)
    b = mp._load().flow_curve(0, fx['su'], None, **kw)
    for k in ('x', 'epl', 'yf', 'hk', 'nsteps', 'status'):
        assert np.array_equal(a[k], b[k]), k
    assert np.all(a['status'] == 0)


def test_status_paths(fx):
    m, p = wh()
    su = np.array(fx['su'][:5])
    ctx = m._load()
    kw = dict(max_steps=3, depl=DEPL, epl_max=np.inf, predictor=0.)
    good = ctx.flow_curve(0, su, None, **kw)
    bad = np.array(su)
    bad[1] = 0.
    bad[3, 2] = np.nan
    r = ctx.flow_curve(0, bad, None, **kw)
    assert r['status'].tolist() == [0, 3, 0, 3, 0] and r['nsteps'].tolist() == [3, 0, 3, 0, 3]
    for k in ('x', 'epl', 'yf', 'hk'):
        assert np.all(np.isnan(r[k][[1, 3]])) and np.array_equal(r[k][[0, 2, 4]], good[k][[0, 2, 4]])
    e0 = np.zeros((5, 6))
    e0[2, 1] = np.inf
    assert ctx.flow_curve(0, su, e0, **kw)['status'].tolist() == [0, 0, 3, 0, 0]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        d = m.flow_curve(np.vstack((su[:2], [[1., 0, 0, 0, 0, 0]])), epl0=np.array([[0.] * 6, [np.nan] + [0.] * 5, [0.] * 6]),
                         max_steps=2, epl_max=np.inf, return_status=True)
        assert d['status'].tolist() == [0, 3, 0] and len(w) == 1 and '1 of 3 curve(s) ended early' in str(w[0].message)
    # a one-vector table with a positive coefficient and a positive intercept: no sign change anywhere
    m1, p1 = FC.wh_material(nsv=1, intercept=1.)
    m1.svc['dual'][:] = np.abs(m1.svc['dual'])
    m1._version += 1
    r = m1._load().flow_curve(0, su, None, **kw)
    assert np.all(r['status'] == 1) and np.all(r['nsteps'] == 0)
    assert all(np.all(np.isnan(r[k])) for k in ('x', 'epl', 'yf', 'hk'))
    # Hill: a hydrostatic direction has no equivalent stress
    mh = FC.hill_material()
    r = mh._load(ana=True).flow_curve(0, np.array([[1., 1., 1., 0, 0, 0], su[0]]), None, **kw)
    assert r['status'].tolist() == [3, 0] and np.all(np.isnan(r['x'][0])) and r['nsteps'].tolist() == [0, 3]


def test_library_conventions(fx):
    import ctypes as C
    from pylabfea_amd import _lib
    m, p = wh()
    ctx = m._load()
    su = np.tile(fx['su'], (6, 1))[:65]
    n0 = ctx.flow_info()['launches']
    r = ctx.flow_curve(0, np.zeros((0, 6)), None, max_steps=5, depl=DEPL, epl_max=np.inf)
    assert ctx.flow_info()['launches'] == n0 and r['x'].shape == (0, 6)            # n = 0 launches nothing
    for k, (n, K) in enumerate(((1, 0), (65, 20), (4, 300))):
        ctx.flow_curve(0, su[:n], None, max_steps=K, depl=DEPL, epl_max=0.0205 if K == 300 else np.inf)
        assert ctx.flow_info()['launches'] == n0 + k + 1                           # one launch per call, whatever n and K

    def rc(mat, depl=DEPL, K=2, pred=0., emax=np.inf, ctx=ctx):
        n = 2
        x, yf, e = np.empty((n, K + 1 if K >= 0 else 1)), np.empty((n, K + 1 if K >= 0 else 1)), np.empty((n, max(K, 0) + 1, 6))
        ns, st = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        s = np.ascontiguousarray(su[:n])
        return ctx.lib.plfx_flow_curve(ctx.h, mat, n, _lib._dp(s), None, K, C.c_double(depl), C.c_double(emax), C.c_double(pred),
                                       _lib._dp(x), _lib._dp(e), _lib._dp(yf), None, _lib._dp(ns), _lib._dp(st))
    ERR_ARG = -2
    assert rc(0) == 0
    assert rc(0, depl=0.) == ERR_ARG and rc(0, depl=-1.) == ERR_ARG and rc(0, depl=np.nan) == ERR_ARG and rc(0, depl=np.inf) == ERR_ARG
    assert rc(0, K=-1) == ERR_ARG and rc(0, pred=np.nan) == ERR_ARG and rc(0, emax=np.nan) == ERR_ARG and rc(1) == ERR_ARG
    assert ctx.flow_info()['launches'] == n0 + 4
    c2 = _lib.Context(0)
    try:
        CV = np.array(m.CV)
        recs = [_lib.pack_material(_lib.ELASTIC, CV, E=200.e3, nu=0.3),
                _lib.pack_material(_lib.TRESCA, CV, E=200.e3, nu=0.3, sy=100.)]
        c2.set_materials(recs)
        assert rc(0, ctx=c2) == ERR_ARG and rc(1, ctx=c2) == ERR_ARG               # elastic; a kind that is not offered
        assert c2.flow_info()['launches'] == 0
    finally:
        c2.close()


def test_data_curve(fx):
    m, p = wh()
    for ilc in fx['dc_ilc']:
        t = '_%d' % ilc
        r = m.data_curve(int(ilc), return_status=True)
        xf, xm = fx['dc_x_fsolve' + t], fx['dc_x_march' + t]
        assert np.array_equal(r['index'], fx['dc_index' + t]) and np.all(r['status'] == 0)
        conv = np.abs(xf - xm) <= 1e-5 * xm          # rows where the example's fsolve converged to the marched root
        assert np.sum(conv) >= len(xf) - 1
        # sig0 has unit J2 stress: seq_ml is the factor itself
        print('load case %d: %d of %d rows, worst |seq_ml - x_fsolve| / x %.3e' % (
            ilc, int(np.sum(conv)), len(xf), float(np.max(np.abs(r['seq_ml'] - xf)[conv] / xf[conv]))))
        assert np.all(np.abs(r['seq_ml'] - xf)[conv] <= 1e-5 * xf[conv])
        x = m.yield_scale(np.tile(r['sig0'], (len(xf), 1)), epl=fx['dc_epl' + t], x0=m.sy)
        assert np.array_equal(r['sig_ml'], r['sig0'][None, :] * x[:, None])
        assert np.allclose(r['seq_data'], fx['dc_seq_data' + t], rtol=1e-13, atol=0.)

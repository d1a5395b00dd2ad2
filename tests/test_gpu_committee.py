"""Committee / plfx_committee_yf on the device against tests/golden/committee.npz (tools/gen_committee.py: the unmodified
reference) and against the np.longdouble restatement of tests/committee_cases.py.

Bars (all from the fixture and the restatement, none from what the device returns), with A = sum |c_k| k_k + |b| and
G = || grad_x f_L ||_1:
  (1) a value      |y - f_L| <= U A 2^-53 + G 2 ulp(max |x|),  U = 4 max(r_ref, 1); against the reference's yf twice that
  (2) the variance |var - var_ref| <= (4/M) sum_m |y_m - ybar| delta + 4 delta^2 + (M + 2) ulp(var_ref), delta the largest
                   bar (1) over the members at the point; mean and var equal the two-pass FP64 formula bit for bit
Cut and trained tables have no reference run of their own: r_ref is replaced by max(r_ref, r_np) resp. r_np, the error of an
FP64 NumPy evaluation of the same formula (the procedure of the cut tables of test_gpu_yield_locus.py).
Measured on an MI355X (2026-10-19), worst ratio to the bar: (1) 0.028 over the six members (0.127 against the reference's
yf), (2) 0.047; cut tables 0.065, global-memory path 0.012."""
import warnings

import numpy as np
import pytest

import committee_cases as CC

pytestmark = pytest.mark.gpu

_c = {}


def S():
    """fixture, members, restatements and the device pass over the six members, computed once"""
    if not _c:
        import pylabfea_amd as FE
        z = CC.load()
        P = [CC.member_params(z, k) for k in range(CC.NMEM)]
        mats = [CC.facade(P[k], 'm%d' % k) for k in range(CC.NMEM)]
        su = np.ascontiguousarray(z['cand_su'])
        R = [CC.restate(P[k], su, 0.5 * P[k]['sy']) for k in range(CC.NMEM)]
        bars = [np.asarray(CC.value_bar(z['r_ref'][k], *R[k][1:]), dtype=float) for k in range(CC.NMEM)]
        _c.update(FE=FE, z=z, P=P, mats=mats, su=su, R=R, bars=bars, Y6=FE.Committee(mats).calc_yf(su),
                  com5=FE.Committee(mats[:5]))
        _c['Y5'] = _c['com5'].calc_yf(su)
    return _c


def test_values():
    s = S()
    z, Y = s['z'], s['Y6']
    assert Y.shape == (CC.NMEM, 256)
    for k in range(CC.NMEM):
        f = s['R'][k][0]
        r1 = np.abs(Y[k].astype(CC.LD) - f) / s['bars'][k]
        r2 = np.abs(Y[k] - z['yf_ref'][k]) / (2 * s['bars'][k])
        print('member %d: worst ratio to bar (1) %.3f, to the reference %.3f' % (k, float(np.max(r1)), float(np.max(r2))))
        assert np.all(r1 <= 1.), k
        assert np.all(r2 <= 1.), k
    assert np.array_equal(s['Y5'], Y[:5])


def test_variance_and_mean():
    s = S()
    z, com, su, Y = s['z'], s['com5'], s['su'], s['Y5']
    var, mean = com.variance(su, return_mean=True)
    m2, v2 = CC.two_pass(Y)
    assert np.array_equal(mean, m2) and np.array_equal(var, v2)              # (a)
    assert np.array_equal(com.variance(su), var)
    delta = np.max(np.array(s['bars'][:5]), axis=0)
    vbar = CC.variance_bar(z['yf_ref'][:5], delta, z['var_ref'])
    ratio = np.abs(var - z['var_ref']) / vbar
    print('variance: worst ratio to bar (2b) %.3f' % float(np.max(ratio)))
    assert np.all(ratio <= 1.)                                                # (b)
    i, sq, v = com.query(su)
    assert i == int(z['argmax_ref'])                                          # (c)
    assert np.array_equal(sq, su[i]) and v == var[i]


def test_order_independence():
    s = S()
    FE, com, su, mats, Y5 = s['FE'], s['com5'], s['su'], s['mats'], s['Y5']
    alone = [com._run(su[i], want_yf=True, want_mean=True, want_var=True) for i in range(65)]
    ya = np.concatenate([a['yf'] for a in alone], axis=1)
    ma, va = np.concatenate([a['mean'] for a in alone]), np.concatenate([a['var'] for a in alone])
    assert np.array_equal(ya, Y5[:, :65])
    for N in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65):
        r = com._run(su[:N], want_yf=True, want_mean=True, want_var=True)
        assert np.array_equal(r['yf'], ya[:, :N]), N
        assert np.array_equal(r['mean'], ma[:N]) and np.array_equal(r['var'], va[:N]), N
    for k in range(5):
        one = FE.Committee([mats[k]])
        r = one._run(su, want_yf=True, want_var=True)
        assert np.array_equal(r['yf'][0], Y5[k]), k
        assert np.all(r['var'] == 0.)                                         # M = 1: exactly zero
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        y = FE.Committee([mats[k] for k in order]).calc_yf(su)
        assert np.array_equal(y, Y5[order])
    y = FE.Committee([mats[0], mats[1], mats[0]]).calc_yf(su)
    assert np.array_equal(y, Y5[[0, 1, 0]])
    y16 = FE.Committee([mats[k % 5] for k in range(16)]).calc_yf(su)
    assert np.array_equal(y16, Y5[np.arange(16) % 5])


def test_cut_tables():
    """the remainder loops of the lane mapping: tables of 1 to 33 vectors, plain and dev_only, in one committee of twelve"""
    s = S()
    FE, z, su = s['FE'], s['z'], s['su']
    cases = [(n, dev) for n in (1, 15, 16, 17, 31, 33) for dev in (False, True)]
    ps = [CC.cut(s['P'][0], nsv=n, dev_only=dev) for n, dev in cases]
    Y = FE.Committee([CC.facade(p) for p in ps]).calc_yf(su)
    for (n, dev), p, y in zip(cases, ps, Y):
        sc = 0.5 * p['sy']
        f, A, G, xm = CC.restate(p, su, sc)
        r_np = CC.r_units(CC.restate(p, su, sc, LD=np.float64)[0], f, A)
        bar = CC.value_bar(max(float(z['r_ref'][0]), r_np), A, G, xm)
        ratio = float(np.max(np.abs(y.astype(CC.LD) - f) / bar))
        print('nsv %2d dev_only %d: r_np %.2f, worst ratio to bar (1) %.3f' % (n, dev, r_np, ratio))
        assert ratio <= 1., (n, dev)


def test_global_memory_path():
    """a member whose tables do not fit the LDS is read from device memory; a second member of the same call is staged"""
    s = S()
    FE, z, su, mats = s['FE'], s['z'], s['su'], s['mats']
    ctx = s['com5']._load()
    nsv0 = len(s['P'][0]['sv'])

    def staged(total):
        m = CC.facade(CC.cut(s['P'][0], pad=total - nsv0))
        FE.Committee([m, mats[1]]).calc_yf(su[:1])
        return bool(ctx.committee_info()[1] & 1), m

    st, big = staged(1400)
    size = 1400
    if st:   # 1400 vectors of 6 features fit: the smallest size that does not
        lo, hi = 1400, 8192
        assert not staged(hi)[0]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if staged(mid)[0] else (lo, mid)
        size = hi
        st, big = staged(size)
    print('member 0 padded to %d vectors is read from device memory' % size)
    assert not st
    y = FE.Committee([big, mats[1]]).calc_yf(su)
    assert ctx.committee_info()[1] == 0b10
    ratio = np.abs(y[0].astype(CC.LD) - s['R'][0][0]) / s['bars'][0]
    print('global-memory path: worst ratio to bar (1) %.3f' % float(np.max(ratio)))
    assert np.all(ratio <= 1.)
    assert np.array_equal(y[1], s['Y5'][1])
    alone = FE.Committee([big]).calc_yf(su[:37])
    assert ctx.committee_info()[1] == 0 and np.array_equal(alone[0], y[0, :37])


def test_query_reduction():
    s = S()
    com, su, z = s['com5'], s['su'], s['z']
    top = int(z['argmax_ref'])
    rest = np.delete(su, top, axis=0)
    V = com.variance(su)
    # several blocks at every block size the host picks: 128 threads (2048 < N <= 4096 on 256 CUs), 256 (N = 4097), 512
    for N, places in [(n, pl) for n in (3000, 4097, 9000) for pl in ((0,), (n - 1,), (n - 700, 300))]:
        t = np.tile(rest, (N // 255 + 1, 1))[:N]
        for i in places:
            t[i] = su[top]
        orig = np.delete(np.arange(256), top)[np.arange(N) % 255]
        orig[list(places)] = top
        r = com._run(t, want_yf=False, want_var=True, want_best=True)
        assert np.array_equal(r['var'], V[orig]), (N, places)   # the same bits at every block size
        i, v = r['best']
        assert i == min(places) and i == int(np.nanargmax(r['var'])) and v == r['var'][i], (N, places)
        assert com.query(t)[0] == i
    # a candidate with a NaN component: NaN at that index only, never returned
    t = su.copy()
    t[top, 4] = np.nan
    r = com._run(t, want_yf=True, want_mean=True, want_var=True, want_best=True)
    assert np.all(np.isnan(r['yf'][:, top])) and np.isnan(r['mean'][top]) and np.isnan(r['var'][top])
    keep = np.arange(256) != top
    assert np.array_equal(r['yf'][:, keep], s['Y5'][:, keep])
    assert np.all(np.isfinite(r['mean'][keep])) and np.all(np.isfinite(r['var'][keep]))
    assert r['best'][0] == int(np.nanargmax(r['var'])) != top
    t[top, 4] = np.inf
    assert np.isnan(com.variance(t)[top]) and com.query(t)[0] == r['best'][0]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        out = com.query(np.full((70, 6), np.nan))
    assert out[0] == -1 and out[1] is None and np.isnan(out[2])
    assert len(w) == 1


def test_library_behaviour():
    import ctypes as C
    from pylabfea_amd import _lib
    s = S()
    FE, com, su, mats = s['FE'], s['com5'], s['su'], s['mats']
    ctx = com._load()
    for M in (1, 5, 16):
        c = FE.Committee([mats[k % 5] for k in range(M)])
        n0 = ctx.committee_info()[0]
        c.calc_yf(su)
        assert ctx.committee_info()[0] == n0 + 1, M
        c.query(su)
        assert ctx.committee_info()[0] == n0 + 2, M
    n0 = ctx.committee_info()[0]
    e = com._run(np.zeros((0, 6)), want_yf=True, want_mean=True, want_var=True, want_best=True)
    assert e['yf'].shape == (5, 0) and e['var'].shape == (0,) and e['best'][0] == -1 and np.isnan(e['best'][1])
    assert ctx.committee_info()[0] == n0
    # error codes, on the C-ABI itself: material 1 is a Hill material
    hill = FE.Material(name='hill')
    hill.elasticity(E=CC.REF['E'], nu=CC.REF['nu'])
    hill.plasticity(sy=CC.REF['sy'], hill=CC.REF['hill'], sdim=6)
    ctx._point_key = None
    ctx.set_materials([mats[0]._record(mats[0].CV), hill._record(hill.CV)])
    yf = np.empty((2, 4))

    def call(nmem, ids, sc):
        ids, sc = np.asarray(ids, dtype=np.int32), np.asarray(sc, dtype=float)
        return ctx.lib.plfx_committee_yf(ctx.h, nmem, _lib._dp(ids), _lib._dp(sc), 4, _lib._dp(su[:4]), _lib._dp(yf), None,
                                         None, None, None)
    n0 = ctx.committee_info()[0]
    assert call(2, [0, 1], [25., 25.]) == -4                                   # PLFX_ERR_UNSUPPORTED
    assert 'Hill' in ctx.lib.plfx_last_error(ctx.h).decode()
    assert call(0, [0], [25.]) == -2 and call(17, [0] * 17, [25.] * 17) == -2  # PLFX_ERR_ARG
    assert call(1, [0], [0.]) == -2 and call(1, [0], [np.inf]) == -2 and call(1, [0], [np.nan]) == -2
    assert call(1, [2], [25.]) == -2 and call(1, [-1], [25.]) == -2
    assert ctx.committee_info()[0] == n0
    assert call(2, [0, 0], [25., 0.5 * mats[0].sy]) == 0
    assert np.array_equal(yf[1], s['Y5'][0, :4])
    # the shared context's key: a member's own calc_yf before and after a committee call
    sig = su[:50] * 0.5 * mats[2].sy
    before = mats[2].calc_yf(sig)
    com.calc_yf(su[:9])
    after = mats[2].calc_yf(sig)
    assert np.array_equal(before, after)
    assert np.array_equal(com.calc_yf(su), s['Y5'])
    # a member edited in place is re-sent
    m = CC.facade(s['P'][0])
    c2 = FE.Committee([m, mats[1]])
    a = c2.calc_yf(su)
    m.scale_seq *= 1.01
    b = c2.calc_yf(su)
    assert np.array_equal(a, s['Y5'][:2]) and np.array_equal(b[1], a[1]) and not np.any(b[0] == a[0])
    p = dict(s['P'][0], scale_seq=m.scale_seq)
    f, A, G, xm = CC.restate(p, su, 0.5 * p['sy'])
    assert np.all(np.abs(b[0].astype(CC.LD) - f) <= CC.value_bar(s['z']['r_ref'][0], A, G, xm))


def test_driver(capsys):
    s = S()
    FE, z, su = s['FE'], s['z'], s['su']
    ref = FE.Material(name='Hill-reference')
    ref.elasticity(E=CC.REF['E'], nu=CC.REF['nu'])
    ref.plasticity(sy=CC.REF['sy'], hill=CC.REF['hill'], sdim=6)
    sig = z['sig']
    kw = dict(CC.TRAIN, C=3., gamma=1.)
    com = FE.train_committee(sig, nmembers=3, rng=np.random.default_rng(5), mat_ref=ref, **kw)
    rng = np.random.default_rng(5)
    assert len(com) == 3
    for idx in com.subsets:
        assert np.array_equal(idx, rng.choice(42, 33, replace=False))
    Y = com.calc_yf(su)
    for k, m in enumerate(com.members):
        own = m.calc_yf(su * 0.5 * m.sy)
        p = dict(sv=m.svc['sv'], dual=m.svc['dual'], intercept=m.svc['intercept'], gamma=m.gam_yf, scale_seq=m.scale_seq,
                 sy=m.sy, dev_only=m.dev_only)
        f, A, G, xm = CC.restate(p, su, 0.5 * m.sy)
        r_np = CC.r_units(CC.restate(p, su, 0.5 * m.sy, LD=np.float64)[0], f, A)
        bar = CC.value_bar(r_np, A, G, xm)
        ratio = float(np.max(np.abs(Y[k] - own) / (2 * bar)))
        print('trained member %d: nsv %d, worst |committee - own| to the sum of both bars %.3f' % (k, len(p['dual']), ratio))
        assert ratio <= 1.
        assert np.all(np.abs(Y[k].astype(CC.LD) - f) <= bar)
    capsys.readouterr()
    mat, added, var = FE.active_learning(ref, z['sunit'], 2, su, nmembers=3, rng=np.random.default_rng(11), **kw)
    out = capsys.readouterr().out
    assert added.shape == (2, 6) and var.shape == (2,) and np.all(np.isfinite(var)) and np.all(var >= 0.)
    for a in added:
        assert np.any(np.all(su == a, axis=1))
    assert 'with 44 load cases' in out and 'with 45 load cases' not in out
    assert mat.ML_yf and mat.sdim == 6 and np.isfinite(mat.calc_yf(su[0] * 0.5 * mat.sy))

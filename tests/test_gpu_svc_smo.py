"""The SVC training kernels of plfx_svm.hpp at their edges: k_smo against the step-for-step NumPy replay of the same
rules (tools/svc_smo_replay.py, pinned to libsvm by tests/test_svc_replay_cpu.py), and k_svc_decision against an FP64
sum.  Problems come from seeded generators.

k_smo: thread and wave edges of the strided rows (n = 2 ... 2049), 1 to 16 features with the class signal in the last
one, one-sample classes, interleaved labels, duplicate rows, exact ties (constant features, where K = 1), the TAU
branch of the update (gamma = 1e-9), K = I (gamma = 1e4), every alpha at a bound (tiny C: rho from the bounds), and
large C.  Against the replay: the same iteration count, support set and status, alpha within 1e-9 C and rho within
1e-9 max(1, |rho|); on its own in FP64: box and equality constraints, the KKT gap and the returned objective.  Then the
resume across launches (max_iter at and around the chunk boundaries) and the host's batching and row reordering, which
must be bit-identical to single fits."""
import importlib.util
import math
import os
import warnings

import numpy as np
import pytest

from pylabfea_amd.material import SVCModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('svc_smo_replay', os.path.join(ROOT, 'tools', 'svc_smo_replay.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

TOL = 1e-3
CHUNK = 2048   # SMO_CHUNK of plfx_svm.hpp: iterations per launch


@pytest.fixture(scope='module')
def ctx():
    from pylabfea_amd.material import _ctx
    return _ctx()


def _labels(rng, s, noise, n):
    """labels from the signal s plus noise, with at least one sample of each class"""
    y = np.where(s + noise * rng.normal(size=n) > 0., 1., -1.)
    y[np.argmax(s)], y[np.argmin(s)] = 1., -1.
    return y


def _gauss(seed, n, d=6, noise=0.5, scale=1.):
    """X ~ N(0, scale^2); the class depends on the LAST feature only"""
    rng = np.random.default_rng(seed)
    X = scale * rng.normal(size=(n, d))
    return X, _labels(rng, X[:, -1], noise, n)


def _q32(X, y, g):
    """the FP32 kernel matrix Q the solver works with"""
    return ((y[:, None] * y[None, :]) * R.kernel_fp64(X, X, g)).astype(np.float32)


def _at_bounds(a, C):
    return np.all((a == 0.) | (a == C))


def _case_n(n):
    X, y = _gauss(100 + n, n)
    return X, y, 1., 0.5


def _case_d(d):
    X, y = _gauss(200 + d, 700, d=d, noise=0.3)
    return X, y, 2., 1. / d


def _case_balance(kind):
    rng = np.random.default_rng(300)
    X = rng.normal(size=(301, 6))
    y = _labels(rng, X[:, -1], 0.5, len(X))
    if kind == 'one_pos':
        y[:] = -1.
        y[rng.integers(len(y))] = 1.
    elif kind == 'one_neg':
        y[:] = 1.
        y[rng.integers(len(y))] = -1.
    else:   # 150 / 150 (and one more), in random order
        y = np.where(rng.permutation(len(y)) % 2 == 0, 1., -1.)
    return X, y, 1., 0.5


def _case_alternating():
    """labels strictly alternate along the index list"""
    rng = np.random.default_rng(400)
    X = rng.normal(size=(500, 6))
    y = np.where(np.arange(500) % 2 == 0, -1., 1.)
    X[:, -1] += 0.8 * y
    return X, y, 1., 0.5


def _case_duplicates():
    """1300 rows: 900 distinct, 250 exact copies with the same label, 150 with the opposite one, shuffled; so many rows
    share a G, which tests the last-index ties in threads (rows 1024 apart), across lanes and across waves"""
    rng = np.random.default_rng(500)
    X0 = rng.normal(size=(900, 6))
    y0 = _labels(rng, X0[:, -1], 0.5, 900)
    s1, s2 = rng.choice(900, 250), rng.choice(900, 150, replace=False)
    X = np.concatenate([X0, X0[s1], X0[s2]])
    y = np.concatenate([y0, y0[s1], -y0[s2]])
    p = rng.permutation(len(X))
    return X[p], y[p], 1., 0.5


def _case_const():
    """every row the same: K = 1, every Q entry +-1, so quad = 0 (TAU) and all G of a class tie; 1100 rows of label -1
    so the ties also fall inside one thread (rows t and t + 1024)"""
    rng = np.random.default_rng(600)
    X = np.tile(rng.normal(size=(1, 6)), (1500, 1))
    y = np.ones(1500)
    y[rng.choice(1500, 1100, replace=False)] = -1.
    return X, y, 1., 0.5


def _case_gamma(g):
    if g < 1.:
        X, y = _gauss(700, 1200, noise=0.5, scale=0.5)   # |x_i - x_j|^2 < 10: K rounds to 1 in FP32
    else:   # spread out so that every off-diagonal K underflows to 0 in FP32
        X, y = _gauss(701, 400, noise=0.5, scale=3.)
    return X, y, 1., g


def _case_C(C):
    if C < 1.:
        X, y = _gauss(800, 400, noise=2.)   # overlapping classes
    else:
        X, y = _gauss(801, 300, noise=0.3)
    return X, y, C, 1.


CASES = {
    **{'n%d' % n: (lambda n=n: _case_n(n)) for n in [2, 3, 63, 64, 65, 1023, 1024, 1025, 2049]},
    **{'d%d' % d: (lambda d=d: _case_d(d)) for d in [1, 3, 15, 16]},
    **{b: (lambda b=b: _case_balance(b)) for b in ['one_pos', 'one_neg', 'half']},
    'alternating': _case_alternating,
    'duplicates': _case_duplicates,
    'const': _case_const,
    'gamma1e-9': lambda: _case_gamma(1e-9),
    'gamma1e4': lambda: _case_gamma(1e4),
    'C1e-4': lambda: _case_C(1e-4),
    'C1e3': lambda: _case_C(1e3),
}


def _replay(X, y, C, g, max_iter=-1):
    """the replay's fit with alpha in the caller's order and rho in the device's convention"""
    r = R.smo(X, y, C, g, tol=TOL, max_iter=max_iter)
    a = np.empty(len(y))
    a[r['perm']] = r['alpha']
    return dict(alpha=a, rho=-r['intercept_'], n_iter=r['n_iter_'], status=r['status'], support=r['support_'],
                obj=r['obj'])


def _support(y, a):
    """support set in libsvm's order (label -1 first), as SVCModel.support_"""
    order = np.concatenate([np.nonzero(y < 0)[0], np.nonzero(y > 0)[0]])
    return order[a[order] > 0.]


def _check_vs_replay(dev, ref, y, C):
    assert dev['status'] == ref['status']
    assert dev['n_iter'] == ref['n_iter']
    assert np.array_equal(_support(y, dev['alpha']), ref['support'])
    assert np.max(np.abs(dev['alpha'] - ref['alpha'])) <= 1e-9 * C
    assert abs(dev['rho'] - ref['rho']) <= 1e-9 * max(1., abs(ref['rho']))


def _check_fp64(dev, X, y, C, g):
    a = dev['alpha']
    n = len(y)
    assert np.all(a >= 0.) and np.all(a <= C)
    assert abs(math.fsum(y * a)) <= 1e-12 * C * n
    if dev['status'] == 0:
        gap = R.kkt_gap(X, y, a, C, g)
        assert gap <= TOL * (1 + 1e-3), gap
    ob = R.dual_obj(X, y, a, g)
    assert abs(dev['obj'] - ob) <= 1e-6 * abs(ob), (dev['obj'], ob)


@pytest.mark.parametrize('case', list(CASES))
def test_smo_matches_replay(ctx, case):
    X, y, C, g = CASES[case]()
    n = len(y)
    dev = ctx.svc_fit_batch(X, y, [np.arange(n)], C, g, tol=TOL)[0]
    ref = _replay(X, y, C, g)
    print('%s: n %d d %d C %g gamma %g: n_iter %d (replay %d), nSV %d (%d), rho %.17g (%.17g)' % (
        case, n, X.shape[1], C, g, dev['n_iter'], ref['n_iter'], np.sum(dev['alpha'] > 0), len(ref['support']),
        dev['rho'], ref['rho']))
    # each case reaches the path it is named for
    if case in ('const', 'gamma1e-9'):
        assert np.all(np.abs(_q32(X, y, g)) == 1.)          # quad = QD_i + QD_j -+ 2 Q_ij = 0 for every pair
    if case == 'const':
        assert np.sum(y < 0) > 1024                         # last-index ties inside a thread
    if case == 'gamma1e4':
        Q = _q32(X, y, g)
        assert np.all(Q[~np.eye(n, dtype=bool)] == 0.)
    if case == 'C1e-4':
        assert _at_bounds(dev['alpha'], C)                  # no free alpha: rho from the bounds
    if case == 'duplicates':
        _, inv, cnt = np.unique(X, axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        assert np.any(cnt > 1)
        lab = [set(y[inv == u]) for u in np.nonzero(cnt > 1)[0]]
        assert any(len(s) == 1 for s in lab) and any(len(s) == 2 for s in lab)
    if case in ('alternating', 'half', 'n1024'):
        assert np.count_nonzero(np.diff(y)) > n // 4        # labels interleaved along the index list
    _check_vs_replay(dev, ref, y, C)
    _check_fp64(dev, X, y, C, g)


def test_last_feature_carries_the_signal():
    """the d cases would catch a kernel that drops feature d-1: without it, the labels are noise"""
    for d in [3, 15, 16]:
        X, y, _, _ = _case_d(d)
        assert abs(np.corrcoef(X[:, -1], y)[0, 1]) > 0.7
        assert np.max(np.abs(np.corrcoef(X[:, :-1].T, y)[-1, :-1])) < 0.15


# ---- resume across launches and the max_iter stop
@pytest.fixture(scope='module')
def slow():
    """8 516 iterations unconstrained: four full launches and a partial one"""
    X, y = _gauss(5, 600, d=2, noise=1.)
    return X, y, 100., 10.


def test_smo_resume_and_max_iter(ctx, slow):
    X, y, C, g = slow
    n = len(y)
    full = _replay(X, y, C, g)
    nc = full['n_iter']
    assert nc > 2 * CHUNK + 100 and full['status'] == 0
    for m in [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, nc - 1, nc, nc + 1]:
        dev = ctx.svc_fit_batch(X, y, [np.arange(n)], C, g, tol=TOL, max_iter=m)[0]
        ref = _replay(X, y, C, g, max_iter=m)
        print('max_iter %d: n_iter %d (replay %d), status %d (%d)' % (m, dev['n_iter'], ref['n_iter'], dev['status'],
                                                                      ref['status']))
        assert ref['status'] == (1 if m <= nc else 0)
        _check_vs_replay(dev, ref, y, C)
        assert np.all(dev['alpha'] >= 0.) and np.all(dev['alpha'] <= C)
        assert abs(math.fsum(y * dev['alpha'])) <= 1e-12 * C * n


def test_svcmodel_max_iter_warns(ctx, slow):
    X, y, C, g = slow
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        m = SVCModel.fit(ctx, X, y, C, g, max_iter=CHUNK)
    assert m.fit_status_ == 1 and int(m.n_iter_[0]) == CHUNK
    assert any('max_iter' in str(x.message) for x in w)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = SVCModel.fit(ctx, X, y, C, g)
    assert m.fit_status_ == 0


# ---- batching and the host's reordering: bit-identical to single fits
def _same(r1, r2):
    return (np.array_equal(r1['alpha'], r2['alpha']) and r1['rho'] == r2['rho'] and r1['obj'] == r2['obj']
            and r1['n_iter'] == r2['n_iter'] and r1['status'] == r2['status'])


def _batch_problems():
    """40 problems on a shared pool of rows: contiguous ranges that overlap, random subsets, sizes 2 ... 2049, each with
    its own C and gamma"""
    rng = np.random.default_rng(900)
    X = rng.normal(size=(2600, 6))
    y = _labels(rng, X[:, -1] + 0.5 * X[:, 0], 0.6, len(X))
    sizes = [2049, 2, 3, 1025, 64, 65, 1024, 1023, 63, 5] + list(rng.integers(2, 2050, 30))
    probs, Cs, gs = [], [], []
    for k, s in enumerate(sizes):
        s = int(s)
        while True:
            if k % 3 == 0:    # contiguous: neighbouring problems overlap
                st = int(rng.integers(0, len(X) - s + 1))
                ix = np.arange(st, st + s)
            else:
                ix = rng.choice(len(X), s, replace=False)
            if len(set(y[ix])) == 2:
                break
        probs.append(ix)
        Cs.append(float(rng.choice([0.1, 1., 10., 50.])))
        gs.append(float(rng.choice([0.05, 0.3, 1., 3.])))
    probs[-1] = probs[0][100:900]   # a problem inside another one
    return X, y, probs, np.array(Cs), np.array(gs)


def test_batch_equals_single_fits(ctx):
    X, y, probs, Cs, gs = _batch_problems()
    batch = ctx.svc_fit_batch(X, y, probs, Cs, gs, tol=TOL)
    assert len(batch) == 40 and max(r['n_iter'] for r in batch) > CHUNK
    for p, ix in enumerate(probs):
        one = ctx.svc_fit_batch(X, y, [ix], Cs[p], gs[p], tol=TOL)[0]
        assert _same(batch[p], one), (p, len(ix), batch[p]['n_iter'], one['n_iter'])
        assert batch[p]['status'] == 0


def test_reordered_index_list(ctx):
    """the same problem with its index list permuted across classes (order within each class kept) gives the same fit,
    alpha mapped back to the caller's order"""
    X, y = _gauss(910, 800)
    ix = np.arange(len(y))
    rng = np.random.default_rng(911)
    # a random merge of the two class sequences
    neg, pos = list(np.nonzero(y < 0)[0]), list(np.nonzero(y > 0)[0])
    take = rng.permutation(np.r_[np.zeros(len(neg), int), np.ones(len(pos), int)])
    perm = np.array([(pos if t else neg).pop(0) for t in take])
    assert not np.array_equal(perm, ix)
    r0 = ctx.svc_fit_batch(X, y, [ix], 1., 0.5, tol=TOL)[0]
    for q in [perm, np.r_[np.nonzero(y > 0)[0], np.nonzero(y < 0)[0]]]:
        r1 = ctx.svc_fit_batch(X, y, [q], 1., 0.5, tol=TOL)[0]
        back = np.empty(len(y))
        back[q] = r1['alpha']
        assert np.array_equal(back, r0['alpha'])
        assert (r1['rho'], r1['obj'], r1['n_iter']) == (r0['rho'], r0['obj'], r0['n_iter'])


def test_duplicated_index_equals_duplicated_row(ctx):
    X, y = _gauss(920, 500)
    for r in [7, 499]:
        ix = np.r_[np.arange(250), r, np.arange(250, 500)]
        X2, y2 = X[ix], y[ix]
        a = ctx.svc_fit_batch(X, y, [ix], 1., 0.5, tol=TOL)[0]
        b = ctx.svc_fit_batch(X2, y2, [np.arange(len(ix))], 1., 0.5, tol=TOL)[0]
        assert _same(a, b)


# ---- k_svc_decision against an FP64 sum
def _dec_ref(X, sv, coef, b, g, q):
    out = np.empty(len(q))
    for t, r in enumerate(q):
        diff = X[r][None, :] - X[sv]
        ss = np.zeros(len(sv))
        for f in range(X.shape[1]):
            ss = ss + diff[:, f] * diff[:, f]
        terms = coef * np.exp(-g * ss)
        out[t] = math.fsum(terms.tolist()) + b
    return out


def _dec_bar(X, sv, coef, b, g, q):
    out = np.empty(len(q))
    for t, r in enumerate(q):
        out[t] = np.sum(np.abs(coef * np.exp(-g * np.sum((X[r][None, :] - X[sv]) ** 2, axis=1)))) + abs(b)
    return 1e-13 * out


def _cancelling(rng, m):
    """coefficients of both signs whose sum nearly cancels"""
    c = rng.uniform(0.5, 2., m) * np.where(np.arange(m) % 2 == 0, 1., -1.)
    if m > 1:
        c[-1] = -math.fsum(c[:-1].tolist()) * (1. + 1e-9)
    return c


@pytest.mark.parametrize('d', [1, 6, 16])
def test_decision_against_fp64(ctx, d):
    rng = np.random.default_rng(1000 + d)
    nsvs, nqs = [0, 1, 2000], [0, 1, 255, 256, 257, 5000]
    X = rng.normal(size=(2000 + 5000, d))
    g = 0.7 / d
    svl, cfs, bs, gms, qls = [], [], [], [], []
    for nsv in nsvs:
        for nq in nqs:
            svl.append(rng.choice(2000, nsv, replace=False))
            cfs.append(_cancelling(rng, nsv))
            bs.append(float(rng.normal()))
            gms.append(g * float(rng.uniform(0.5, 2.)))
            qls.append(2000 + rng.choice(5000, nq, replace=False))
    dev = ctx.svc_decision_batch(X, svl, cfs, bs, gms, qls)
    for p in range(len(svl)):
        assert len(dev[p]) == len(qls[p])
        if len(qls[p]) == 0:
            continue
        ref = _dec_ref(X, svl[p], cfs[p], bs[p], gms[p], qls[p])
        bar = _dec_bar(X, svl[p], cfs[p], bs[p], gms[p], qls[p])
        err = np.abs(dev[p] - ref)
        assert np.all(err <= bar), (p, len(svl[p]), len(qls[p]), np.max(err / bar))
        if len(svl[p]) == 0:
            assert np.all(dev[p] == bs[p])


def test_decision_many_models(ctx):
    """300 models in one call, empty and non-empty lists mixed, models that share rows"""
    rng = np.random.default_rng(1100)
    X = rng.normal(size=(600, 6))
    svl, cfs, bs, gms, qls = [], [], [], [], []
    for p in range(300):
        nsv = 0 if p % 7 == 0 else int(rng.integers(1, 60))
        nq = 0 if p % 11 == 0 else int(rng.integers(1, 300))
        svl.append(rng.choice(600, nsv, replace=False))
        cfs.append(_cancelling(rng, nsv))
        bs.append(float(rng.normal()))
        gms.append(float(rng.uniform(0.05, 2.)))
        qls.append(rng.integers(0, 600, nq))
    dev = ctx.svc_decision_batch(X, svl, cfs, bs, gms, qls)
    for p in range(300):
        assert len(dev[p]) == len(qls[p])
        ref = _dec_ref(X, svl[p], cfs[p], bs[p], gms[p], qls[p])
        assert np.all(np.abs(dev[p] - ref) <= _dec_bar(X, svl[p], cfs[p], bs[p], gms[p], qls[p])), p


def test_decision_exact_cases(ctx):
    rng = np.random.default_rng(1200)
    g = 2.5
    X = rng.normal(size=(50, 6))
    far = np.full((1, 6), 40. / math.sqrt(g) + 10.)   # more than 40 / sqrt(gamma) from every SV
    Xa = np.concatenate([X, far])
    assert np.min(np.sum((X - far) ** 2, axis=1)) * g > 1600.
    c = _cancelling(rng, 50)
    b = 0.3125
    dev = ctx.svc_decision_batch(Xa, [np.arange(0), np.arange(50), np.array([17])], [np.zeros(0), c, np.array([-1.75])],
                                 [b, b, 0.625], [g, g, g], [np.arange(51), np.array([50]), np.array([17])])
    assert np.all(dev[0] == b)                      # no support vectors: exactly b
    assert dev[1][0] == b                           # every term underflows to 0
    assert dev[2][0] == -1.75 + 0.625               # exp(0) = 1
    # no query points anywhere: nothing is launched, nothing returned
    out = ctx.svc_decision_batch(Xa, [np.arange(50)], [c], [b], [g], [np.arange(0)])
    assert len(out) == 1 and len(out[0]) == 0

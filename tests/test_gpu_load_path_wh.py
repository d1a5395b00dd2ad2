"""Material.load_path on a work-hardening SVC on the GPU: the hardening modulus as state of a path, one thread
or one wave per path.

(1) The thread form has the bits of the host loop -- K calls of Context.response(khard_in, return_khard=True, maxit) with the
    modulus carried and epl += depl in NumPy -- at every step; a difference is a finding, not a tolerance to widen.
(2) The wave form differs from the thread form only in the order of the support-vector sums.  The bar comes from the yardstick
    alone: the loop of (1) on the table and on the table with its rows reversed; 4 max(calib, 1e-12 max|output|), the rule of §21.
(3) The wave form is consistent with itself, bit for bit: shuffles, K-prefixes, a shared path, two calls.
(4) Mixed control in both forms: targets within stol, strain components untouched, the strain-controlled replay bit for bit.
(6) The library's argument checks, launch counts and refusals.
(5) Both forms against the reference's own carry: six chains of 12 consecutive response calls on one reference object each
    (tests/golden/load_path_wh.npz, tools/gen_load_path_wh.py), within the bar of the reference's own two runs."""
import ctypes as C
import os

import numpy as np
import pytest

import flow_curve_cases as FC
import load_path_cases as LP
import load_path_wh_cases as LW
from pylabfea_amd import _lib
from test_gpu_model import FE

pytestmark = pytest.mark.gpu

TABLES = ('1', '63', '64', '65', 'full', 'padded')
MAXIT_WAVE = 5   # of checks (2) and (3): the yardstick of (2) runs one thread per path, 24 calls per table


@pytest.fixture(scope='module')
def z():
    return LW.golden()


@pytest.fixture(scope='module')
def tables(z):
    """(name, reversed) -> (material, CV, sy, E), built on first use"""
    made = {}

    def get(name, reverse=False):
        if (name, reverse) not in made:
            m, _ = LW.table(FE(), z, name, reverse=reverse)
            CV = np.array(z['par_CV'], dtype=float).reshape(6, 6)
            made[(name, reverse)] = (m, CV, float(z['par_sy']), float(CV[0, 0]))
        return made[(name, reverse)]
    return get


def kh_start(N, seed):
    """a per-point positive start modulus"""
    return np.random.default_rng(7000 + seed).uniform(50., 800., size=N)


# ------------------------------------------------------------------------------------------------ (1) the thread form
# (a sub-divided step of maxit = 50 costs ten of maxit = 5 on one thread, and on a cut table nearly every plastic step is
# sub-divided: with maxit = 50 the K = 12 paths are launched once, at N = 257, and the prefixes in N have K <= 2; with maxit = 5
# the prefixes N = 1, 63, 65 run at K = 12 as well)
@pytest.mark.parametrize('maxit,k0', [(5, 'zero'), (5, 'array'), (50, 'zero'), (50, 'array')])
def test_thread_form_has_the_bits_of_the_loop(tables, maxit, k0):
    m, CV, sy, E = tables('64')
    N = 257
    dload = LP.strain_paths(sy, E, K=LW.K_PATH, N=N, seed=11)
    kh0 = np.zeros(N) if k0 == 'zero' else kh_start(N, 1)
    Y = LW.yardstick(m, CV, dload, maxit, kh0)
    ev = LW.events(Y, kh0)
    print('64 vectors, maxit %d, khard0 %s: %s' % (maxit, k0, ev))
    assert np.all(np.isfinite(Y['sig'])) and np.all(Y['nsteps'] >= 0)
    assert ev['elastic'] > 0 and ev['plastic'] > 0 and ev['nspos'] > 0 and ev['khard_changed'] > 0, ev
    ctx = m._load(CV)
    n0, p0 = ctx.load_path_wh_info(), ctx.load_path_info()
    P = m.load_path(dload, CV=CV, maxit=maxit, khard0=kh0, form='thread', return_tangent=True)
    n1 = ctx.load_path_wh_info()
    assert n1 == dict(launches_thread=n0['launches_thread'] + 1, launches_wave=n0['launches_wave'])   # one launch, its form
    assert ctx.load_path_info() == p0
    LW.assert_same_bits('maxit %d %s' % (maxit, k0), P, Y)
    assert np.array_equal(P['deps'], dload) and np.all(P['newton'] == 0)
    for n, K in ((1, 2), (63, 1), (65, 2), (257, 1)):                                # prefixes in N and in K of the one yardstick
        Q = m.load_path(dload[:K, :n], CV=CV, maxit=maxit, khard0=kh0[:n], form='thread', return_tangent=True)
        LW.assert_same_bits('maxit %d %s N %d K %d' % (maxit, k0, n, K), Q, Y, K=K, N=n, ct=False)
    if maxit == 5:
        for n in (1, 63, 65):
            Q = m.load_path(dload[:, :n], CV=CV, maxit=maxit, khard0=kh0[:n], form='thread', return_tangent=True)
            LW.assert_same_bits('maxit %d %s N %d K 12' % (maxit, k0, n), Q, Y, N=n)


def test_thread_form_shared_path_and_restart(tables):
    m, CV, sy, E = tables('64')
    N = 65
    dload = LP.strain_paths(sy, E, K=LW.K_PATH, N=N, seed=12)
    kh0 = kh_start(N, 2)
    shared = np.ascontiguousarray(dload[:, 5])
    sig0 = 0.3 * sy * np.random.default_rng(5).uniform(-1., 1., size=(N, 6))
    Ys = LW.yardstick(m, CV, np.repeat(shared[:, None], N, axis=1), 5, kh0, sig0=sig0)
    P = m.load_path(shared, CV=CV, maxit=5, khard0=kh0, sig0=sig0, form='thread', return_tangent=True)   # a shared (K, 6) path
    LW.assert_same_bits('shared', P, Ys)
    X = m.load_path(np.repeat(shared[:, None], N, axis=1), CV=CV, maxit=5, khard0=kh0, sig0=sig0, form='thread', return_tangent=True)
    for what in LW.NAMES + ('ct', 'deps'):
        assert np.array_equal(P[what], X[what]), what
    # sig0 / epl0 / khard0 from the middle of another path: the rest of that path, bit for bit
    Y = LW.yardstick(m, CV, dload, 5, kh0)
    k = 6
    R = m.load_path(dload[k + 1:], CV=CV, maxit=5, sig0=Y['sig'][k], epl0=Y['epl'][k], khard0=Y['khard'][k], form='thread',
                    return_tangent=True)
    for what in LW.NAMES:
        assert np.array_equal(R[what], Y[what][k + 1:]), 'restart: %s differs' % what
    assert np.array_equal(R['ct'], Y['ct'])


@pytest.mark.parametrize('name,K,N', [('padded', 3, 5), ('full', 3, 5), ('1', 12, 65), ('63', 12, 65), ('65', 12, 65)])
def test_thread_form_on_the_other_tables(tables, name, K, N):
    m, CV, sy, E = tables(name)
    dload = LP.strain_paths(sy, E, K=K, N=N, seed=13)
    if K < 12:
        dload = dload * 3.                                                            # (three steps that reach the yield surface)
    kh0 = kh_start(N, 3)
    Y = LW.yardstick(m, CV, dload, 5, kh0)
    print(name, LW.events(Y, kh0))
    P = m.load_path(dload, CV=CV, maxit=5, khard0=kh0, form='thread', return_tangent=True)
    LW.assert_same_bits(name, P, Y)


# ------------------------------------------------------------------------------------------------ (2) the wave form
@pytest.fixture(scope='module')
def wave_cases(tables):
    """table -> (dload (12, 9, 6), khard0, yardstick, calib, first unstable step per path), computed once; maxit = MAXIT_WAVE"""
    made = {}

    def get(name):
        if name not in made:
            m, CV, sy, E = tables(name)
            mr = tables(name, True)[0]
            N = 9
            dload = LP.strain_paths(sy, E, K=LW.K_PATH, N=N, seed=20 + TABLES.index(name))
            kh0 = kh_start(N, 4)
            Ya, Yb = LW.yardstick(m, CV, dload, MAXIT_WAVE, kh0), LW.yardstick(mr, CV, dload, MAXIT_WAVE, kh0)
            calib, first = LW.calibration(Ya, Yb)
            unstable = int(np.sum(first < LW.K_PATH))
            print('%s: %d of %d paths unstable on the yardstick alone (first steps %s); largest calib %s'
                  % (name, unstable, N, first.tolist(), {k: float(v.max()) for k, v in calib.items()}))
            assert unstable * 8 <= N, (name, first)                                  # at most 1 path in 8
            made[name] = (dload, kh0, Ya, calib, first)
        return made[name]
    return get


@pytest.mark.parametrize('name', TABLES)
def test_wave_form_within_the_measured_bar(tables, wave_cases, name):
    m, CV, sy, E = tables(name)
    dload, kh0, Y, calib, first = wave_cases(name)
    ctx = m._load(CV)
    worst = 0.
    for N in (1, 3, 4, 5, 9):                                                        # 4 paths per block
        n0 = ctx.load_path_wh_info()
        P = m.load_path(dload[:, :N], CV=CV, maxit=MAXIT_WAVE, khard0=kh0[:N], form='wave', return_tangent=True)
        assert ctx.load_path_wh_info() == dict(launches_thread=n0['launches_thread'], launches_wave=n0['launches_wave'] + 1)
        assert np.all(P['status'] == 0) and np.all(P['newton'][:, :] == 0) and np.array_equal(P['deps'], dload[:, :N])
        worst = max(worst, LW.assert_within_bar('%s N %d' % (name, N), P, Y, calib, first, cols=np.arange(N)))
    print('%s: worst ratio to the bar %.3f' % (name, worst))
    if name in ('64', 'padded'):                                                     # ... and the thread form against the wave form
        T = m.load_path(dload, CV=CV, maxit=MAXIT_WAVE, khard0=kh0, form='thread')
        LW.assert_same_bits(name + ' thread', T, Y, ct=False)


# ------------------------------------------------------------------------------------------------ (3) the wave form with itself
@pytest.mark.parametrize('name', ['65', 'full'])
def test_wave_form_is_consistent_with_itself(tables, wave_cases, name):
    m, CV, sy, E = tables(name)
    dload, kh0, _, _, _ = wave_cases(name)
    N = dload.shape[1]
    P = m.load_path(dload, CV=CV, maxit=MAXIT_WAVE, khard0=kh0, form='wave', return_tangent=True)
    keys = LW.NAMES + ('deps', 'newton', 'ksteps', 'status', 'ct')
    Q = m.load_path(dload, CV=CV, maxit=MAXIT_WAVE, khard0=kh0, form='wave', return_tangent=True)      # two calls
    for what in keys:
        assert np.array_equal(P[what], Q[what], equal_nan=True), 'two calls differ in %s' % what
    perm = np.random.default_rng(3).permutation(N)                                   # a shuffle of the paths
    S = m.load_path(np.ascontiguousarray(dload[:, perm]), CV=CV, maxit=MAXIT_WAVE, khard0=kh0[perm], form='wave', return_tangent=True)
    for what in keys:
        a = P[what][perm] if what in ('ksteps', 'status', 'ct') else P[what][:, perm]
        assert np.array_equal(S[what], a, equal_nan=True), 'the shuffle differs in %s' % what
    for K in (1, 2, 7):                                                              # K-prefixes
        R = m.load_path(dload[:K], CV=CV, maxit=MAXIT_WAVE, khard0=kh0, form='wave')
        for what in LW.NAMES + ('deps', 'newton'):
            assert np.array_equal(R[what], P[what][:K], equal_nan=True), 'the prefix K = %d differs in %s' % (K, what)
    shared = np.ascontiguousarray(dload[:, 2])                                       # a shared path against its expansion
    A = m.load_path(shared, CV=CV, maxit=MAXIT_WAVE, khard0=kh0, form='wave', return_tangent=True)
    B = m.load_path(np.repeat(shared[:, None], N, axis=1), CV=CV, maxit=MAXIT_WAVE, khard0=kh0, form='wave', return_tangent=True)
    for what in keys:
        assert np.array_equal(A[what], B[what], equal_nan=True), 'the shared path differs in %s' % what
    U = m.load_path(dload[:, :3], CV=CV, maxit=MAXIT_WAVE, khard0=kh0[:3], form='auto')                # few paths: auto is the wave form
    for what in LW.NAMES:
        assert np.array_equal(U[what], P[what][:, :3], equal_nan=True), 'auto differs in %s' % what


# ------------------------------------------------------------------------------------------------ (4) mixed control
# (one thread per path pays every sub-step of every trial in turn: its case runs with maxit = 5)
@pytest.mark.parametrize('name,form,maxit', [('full', 'wave', 50), ('64', 'wave', 50), ('64', 'thread', 5)])
def test_mixed_control(tables, name, form, maxit):
    m, CV, sy, E = tables(name)
    dload, control = LW.mixed_paths(sy, E)
    K, N = dload.shape[:2]
    stol = 1.e-9 * sy
    kh0 = np.zeros(N)
    P = m.load_path(dload, control=control, CV=CV, maxit=maxit, khard0=kh0, form=form, return_tangent=True)
    ks = P['ksteps']
    print('%s %s: status %s ksteps %s corrections at most %s' % (name, form, P['status'].tolist(), ks.tolist(),
                                                              np.where(P['newton'] >= 0, P['newton'], 0).max(axis=0).tolist()))
    assert np.all((P['status'] == 0) | (P['status'] == 1)), P['status']
    assert np.all((P['status'] == 0) == (ks == K))
    if name == 'full':
        assert np.sum(P['status'] == 0) >= 4, P['status']
    t = LP.targets(dload, control)
    done = np.arange(K)[:, None] < ks[None, :]                                       # (K, N)
    F = np.broadcast_to(control[None], P['sig'].shape) & done[:, :, None]
    S = np.broadcast_to(~control[None], P['sig'].shape) & done[:, :, None]
    assert np.all(np.abs(P['sig'] - t)[F] <= stol), float(np.max(np.abs(P['sig'] - t)[F]))
    assert np.array_equal(P['deps'][S], dload[S])
    assert np.all(P['newton'][done] >= 0) and np.all(P['newton'][done] <= 30)
    for what in ('sig', 'epl', 'deps', 'fy', 'khard'):                              # past ksteps: NaN / -1
        assert np.all(np.isnan(P[what][~done])) and np.all(np.isfinite(P[what][done])), what
    assert np.all(P['nsteps'][~done] == -1) and np.all(P['newton'][~done] == -1) and np.all(P['nsteps'][done] >= 0)
    for i in range(N):                                                               # the strain-controlled replay, path by path
        k = int(ks[i])
        if k == 0:
            continue
        R = m.load_path(np.ascontiguousarray(P['deps'][:k, i:i + 1]), CV=CV, maxit=maxit, khard0=kh0[i:i + 1], form=form, return_tangent=True)
        for what in LW.NAMES:
            assert np.array_equal(R[what], P[what][:k, i:i + 1]), '%s %s path %d: the replay differs in %s' % (name, form, i, what)
        assert np.all(R['newton'] == 0)
        if k == K:
            assert np.array_equal(R['ct'], P['ct'][i:i + 1]), 'path %d: the replay differs in ct' % i
    # a path that ends early leaves its neighbours alone: every path alone returns what it returned among the others
    for i in np.nonzero(ks < K)[0][:1]:
        for j in (i - 1, i + 1):
            if 0 <= j < N:
                A = m.load_path(np.ascontiguousarray(dload[:, j:j + 1]), control=control[j:j + 1], CV=CV, maxit=maxit, khard0=0., form=form)
                for what in LW.NAMES + ('deps', 'newton'):
                    assert np.array_equal(A[what], P[what][:, j:j + 1], equal_nan=True), (i, j, what)


# ------------------------------------------------------------------------------------------------ (5) the reference's own carry
@pytest.mark.parametrize('form', ['thread', 'wave'])
def test_against_the_carry_of_the_reference(tables, form):
    g = np.load(os.path.join(LW.GOLD, 'load_path_wh.npz'))
    m, CV, sy, E = tables('full')
    assert np.array_equal(g['CV'], CV)
    Kc = g['dload'].shape[1]
    first = np.asarray(g['first'])
    assert np.sum(first < Kc) * 6 <= len(first), first                               # at most 1 unstable chain in 6
    worst = 0.
    for maxit in np.unique(g['maxit']):                                              # one launch per maxit
        c = np.nonzero(g['maxit'] == maxit)[0]
        P = m.load_path(np.ascontiguousarray(np.swapaxes(g['dload'][c], 0, 1)), CV=CV, maxit=int(maxit), sig0=g['sig0'][c],
                        epl0=g['epl0'][c], khard0=g['khard0'][c], form=form, return_tangent=True)
        assert np.all(P['status'] == 0) and np.all(P['ksteps'] == Kc)
        Y = {w: np.swapaxes(g[w], 0, 1) for w in ('sig', 'epl', 'fy', 'khard', 'nsteps')}
        calib = {w: np.swapaxes(g['calib_' + w], 0, 1) for w in ('sig', 'epl', 'fy', 'khard')}
        worst = max(worst, LW.assert_within_bar('reference chains %s, %s' % (c.tolist(), form), P, Y, calib, first, cols=c))
    print('%s form against the reference: worst ratio to the bar %.3f' % (form, worst))


# ------------------------------------------------------------------------------------------------ (6) the library
def test_library_checks_and_counts(tables, z):
    m, CV, sy, E = tables('64')
    ctx = m._load(CV)
    lib, h = ctx.lib, ctx.h
    K, N = 3, 4
    d = LP.strain_paths(sy, E, K=K, N=N, seed=30)
    kh0 = np.zeros(N)
    out = dict(sig=np.empty((K, N, 6)), epl=np.empty((K, N, 6)), deps=np.empty((K, N, 6)), fy=np.empty((K, N)),
               khard=np.empty((K, N)), nsteps=np.empty((K, N), dtype=np.int32), newton=np.empty((K, N), dtype=np.int32),
               ksteps=np.empty(N, dtype=np.int32), status=np.empty(N, dtype=np.int32), ct=np.empty((N, 36)))
    p = _lib._dp

    def call(mat=0, n=N, K=K, dload=d, shared=0, control=None, sig0=None, epl0=None, khard0=kh0, form=1, maxit=50, newton=30,
             stol=1.e-7, eps_cap=0.05, **repl):
        o = dict(out, **repl)
        return lib.plfx_load_path_wh(h, mat, n, K, p(dload), shared, p(control), p(sig0), p(epl0), p(khard0), form, maxit, newton,
                                     C.c_double(stol), C.c_double(eps_cap), p(o['sig']), p(o['epl']), p(o['deps']), p(o['fy']),
                                     p(o['khard']), p(o['nsteps']), p(o['newton']), p(o['ksteps']), p(o['status']), p(o['ct']))
    ARG, UNSUP = -2, -4
    n0, p0 = ctx.load_path_wh_info(), ctx.load_path_info()
    bad = d.copy()
    bad[1, 2, 3] = np.nan
    big = d.copy()
    big[0, 0, 0] = 0.06
    neg, nan = kh0.copy(), kh0.copy()
    neg[2], nan[1] = -1., np.nan
    errors = [dict(mat=-1), dict(mat=1), dict(n=-1), dict(K=-1), dict(maxit=0), dict(newton=-1), dict(stol=0.), dict(stol=np.inf),
              dict(eps_cap=0.), dict(eps_cap=np.nan), dict(form=-1), dict(form=3), dict(khard0=None), dict(khard0=neg), dict(khard0=nan),
              dict(khard0=np.full(N, np.inf)), dict(dload=None), dict(dload=bad), dict(dload=big), dict(sig=None), dict(khard=None),
              dict(ksteps=None), dict(control=np.array([0, 64, 0, 0], dtype=np.int32)), dict(sig0=np.full((N, 6), np.inf)),
              dict(epl0=np.full((N, 6), np.nan)), dict(n=60000, K=2000)]
    for kw in errors:
        assert call(**kw) == ARG, kw
        assert ctx.load_path_wh_info() == n0, kw
    assert call(n=0) == 0 and call(n=0, khard0=None, dload=None) == 0 and ctx.load_path_wh_info() == n0      # n = 0: nothing launched
    out['ksteps'][:], out['status'][:] = 7, 7
    assert call(K=0) == 0 and ctx.load_path_wh_info() == n0                                                    # K = 0: ct = CV
    assert np.all(out['ksteps'] == 0) and np.all(out['status'] == 0) and np.array_equal(out['ct'].reshape(N, 6, 6), np.broadcast_to(CV, (N, 6, 6)))
    for form, key in ((1, 'launches_thread'), (2, 'launches_wave'), (0, 'launches_wave')):                     # one launch, its form
        before = ctx.load_path_wh_info()
        assert call(form=form) == 0
        after = ctx.load_path_wh_info()
        assert after[key] == before[key] + 1 and sum(after.values()) == sum(before.values()) + 1, (form, before, after)
        assert np.all(out['status'] == 0) and np.all(out['ksteps'] == K)
    assert ctx.load_path_info() == p0                                               # plfx_load_path_info is untouched
    # separate output arrays (no packed block) against the binding's packed block
    P = ctx.load_path_wh(0, d, kh0, form='thread', stol=1.e-7, return_tangent=True)
    assert call(form=1) == 0
    for what in ('sig', 'epl', 'deps', 'fy', 'khard', 'nsteps', 'newton', 'ksteps', 'status'):
        assert np.array_equal(out[what], P[what]), what
    assert np.array_equal(out['ct'].reshape(N, 6, 6), P['ct'])
    # plfx_load_path on the work-hardening record is still refused, without a launch of either counter
    n1 = ctx.load_path_wh_info()
    rc = lib.plfx_load_path(h, 0, N, K, p(d), 0, None, None, None, None, 50, 30, C.c_double(1.e-7), C.c_double(0.05), p(out['sig']),
                            p(out['epl']), p(out['deps']), p(out['fy']), p(out['nsteps']), p(out['newton']), p(out['ksteps']),
                            p(out['status']), p(out['ct']))
    assert rc == UNSUP and ctx.load_path_info() == p0 and ctx.load_path_wh_info() == n1
    # set_materials between two calls: a Hill record is refused, the work-hardening record runs again with the same bits
    hill = FC.hill_material(FE())
    hctx = hill._load(np.array(hill.CV))
    assert hctx is ctx
    n2 = ctx.load_path_wh_info()
    assert call() == UNSUP and ctx.load_path_wh_info() == n2
    assert m._load(CV) is ctx
    Q = ctx.load_path_wh(0, d, kh0, form='thread', stol=1.e-7, return_tangent=True)
    for what in LW.NAMES + ('ct',):
        assert np.array_equal(Q[what], P[what]), what
    # a work-hardening record with an SVR flow rule attached: refused, nothing launched
    from svr_flow_cases import install_svr
    mg, _ = FC.wh_material()
    install_svr(mg, np.load(os.path.join(FC.GOLD, 'svr_gradient.npz')))
    mg.enable_svr_flow()
    assert mg._load(np.array(mg.CV)) is ctx and ctx.svr_flow_info(0)[0] > 0
    n3 = ctx.load_path_wh_info()
    for form in (0, 1, 2):
        assert call(form=form) == UNSUP and ctx.load_path_wh_info() == n3, form
    assert b'SVR flow rule' in lib.plfx_last_error(h)

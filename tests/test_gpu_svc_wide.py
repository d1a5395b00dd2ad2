"""k_smo_wide (plfx_svc_fit_wide): one SMO problem over many workgroups must give k_smo's fit bit for bit -- the same
alpha, iteration count, status and rho -- for every grid size, row count and branch of the solver."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ctx():
    from pylabfea_amd import _lib
    return _lib.Context(0)


def problem(seed, n, d, dup=False):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) * 0.7
    y = np.where(np.sum(X[:, :2] ** 2, axis=1) + 0.3 * rng.normal(size=n) > 0.9, 1., -1.)
    if n >= 2:
        y[0], y[1] = -1., 1.
    if dup:
        X[n // 2:] = X[:n - n // 2]
        y[n // 2:] = y[:n - n // 2]
    return X, y


def same(ctx, X, y, C, gamma, nwg=0, max_iter=-1):
    w = ctx.svc_fit_wide(X, y, C, gamma, max_iter=max_iter, nwg=nwg)
    b = ctx.svc_fit_batch(X, y, [np.arange(len(y))], C, gamma, max_iter=max_iter)[0]
    assert np.array_equal(w['alpha'], b['alpha'])
    assert w['n_iter'] == b['n_iter'] and w['status'] == b['status']
    assert w['rho'] == b['rho'] and w['obj'] == b['obj']
    return w


@pytest.mark.gpu
@pytest.mark.parametrize('n,d', [(2, 6), (3, 15), (257, 6), (1000, 15), (4097, 6), (15000, 6), (40000, 15)])
def test_auto_grid(ctx, n, d):
    X, y = problem(n + d, n, d)
    w = same(ctx, X, y, 2., 1.)
    assert w['status'] == 0


@pytest.mark.gpu
@pytest.mark.parametrize('nwg', [1, 2, 3, 8, 64])
def test_forced_grid(ctx, nwg):
    # 1 931 rows: not a multiple of any slice; with 64 workgroups of 256 threads most threads and some workgroups own no row
    X, y = problem(nwg, 1931, 6)
    same(ctx, X, y, 4., 0.8, nwg=nwg)
    X, y = problem(nwg + 1, 1931, 15)
    same(ctx, X, y, 1., 1.5, nwg=nwg)


@pytest.mark.gpu
def test_workgroups_without_rows(ctx):
    X, y = problem(9, 300, 6)   # 300 rows over 8 workgroups x 256 threads, R = 1: workgroups 2 .. 7 own nothing
    same(ctx, X, y, 2., 1., nwg=8)


@pytest.mark.gpu
@pytest.mark.parametrize('C,gamma', [(2., 1e-9), (1e-4, 1.)])
def test_tau_branch_and_no_free_alpha(ctx, C, gamma):
    X, y = problem(21, 2000, 6)
    same(ctx, X, y, C, gamma, nwg=5)
    same(ctx, X, y, C, gamma)


@pytest.mark.gpu
def test_duplicate_rows(ctx):
    X, y = problem(33, 3001, 6, dup=True)
    same(ctx, X, y, 10., 2., nwg=4)


@pytest.mark.gpu
@pytest.mark.parametrize('max_iter', [1, 2047, 2048, 2049, 8191, 8192, 8193])
def test_max_iter_around_launch_bounds(ctx, max_iter):
    X, y = problem(5, 6000, 6)
    w = same(ctx, X, y, 10., 3., max_iter=max_iter)
    assert w['n_iter'] <= max_iter


@pytest.mark.gpu
def test_against_numpy_replay(ctx):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import svc_smo_replay as R
    for seed, n, d in ((1, 40, 6), (2, 97, 15), (3, 200, 3)):
        X, y = problem(seed, n, d)
        w = ctx.svc_fit_wide(X, y, 2., 1., nwg=3)
        r = R.smo(X, y, 2., 1.)
        assert w['n_iter'] == r['n_iter_'] and w['status'] == r['status']
        assert np.array_equal(np.sort(np.nonzero(w['alpha'] > 0.)[0]), np.sort(r['support_']))
        assert np.max(np.abs(w['alpha'][r['perm']] - r['alpha'])) < 1e-9


@pytest.mark.gpu
def test_arguments_refused(ctx):
    from pylabfea_amd._lib import PlfxError
    X, y = problem(1, 100, 6)
    with pytest.raises(PlfxError):
        ctx.svc_fit_wide(X, y, 2., 1., nwg=100000)        # more workgroups than can be resident
    with pytest.raises(PlfxError):
        ctx.svc_fit_wide(X, y, 2., 1., nwg=-1)
    with pytest.raises(PlfxError):
        ctx.svc_fit_wide(X, np.ones(100), 2., 1.)         # one class
    with pytest.raises(PlfxError):
        ctx.svc_fit_wide(X, y, 0., 1.)

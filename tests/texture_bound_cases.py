"""Helpers of the tests of texture materials bound to one texture (Material.at_texture): the folded tables
restated in plain FP64 NumPy, and façade materials with given tables installed.

The fold (notation of texture_flow_cases): with f_j = (s_j - mean_j) / scale_j the stress features and ft the standardised
features of the fixed texture, c_k = sum_t (ft_t - v_{k,6+t})^2, d'_k = dual_k exp(-gamma c_k), v'_kj = v_kj + mean_j / scale_j,
x_j = s_j / scale_j, and  calc_yf(sig, tex) = sum_k d'_k exp(-gamma |x - v'_k|^2) + intercept.  The gradient is
a_j = -2 gamma sum_k d'_k K_k (x_j - v'_kj) / scale_j, projected onto the deviator for a dev_only set."""
import contextlib
import io

import numpy as np

import texture_cases as TC


def fold(p, tex):
    """the folded tables of the parameter dict p at the texture tex (tdim,), restated independently of the façade"""
    tex = np.asarray(tex, dtype=float).reshape(-1)
    ft = (tex - p['mean'][6:]) / p['scale'][6:]
    c = np.sum((ft[None, :] - p['sv'][:, 6:]) ** 2, axis=1)
    return dict(sv=p['sv'][:, :6] + (p['mean'][:6] / p['scale'][:6])[None, :], dual=p['dual'] * np.exp(-p['gamma'] * c),
                intercept=float(p['intercept']), gamma=float(p['gamma']), scale=np.array(p['scale'][:6]),
                dev_only=bool(p['dev_only']))


def _x(f, sig):
    s = np.array(sig, dtype=float).reshape(-1, 6)
    if f['dev_only']:
        s[:, :3] -= (np.sum(s[:, :3], axis=1) / 3.)[:, None]
    return s / f['scale'][None, :]


def folded_yf(f, sig):
    """the folded form evaluated in plain FP64 NumPy at the stresses sig (N,6)"""
    x = _x(f, sig)
    out = np.empty(len(x))
    for i in range(len(x)):
        d = x[i][None, :] - f['sv']
        out[i] = np.sum(f['dual'] * np.exp(-f['gamma'] * np.sum(d * d, axis=1))) + f['intercept']
    return out


def folded_grad(f, sig):
    """the gradient formula of the folded form, plain FP64 NumPy, (N,6)"""
    x = _x(f, sig)
    a = np.empty((len(x), 6))
    for i in range(len(x)):
        d = x[i][None, :] - f['sv']
        w = f['dual'] * np.exp(-f['gamma'] * np.sum(d * d, axis=1))
        a[i] = -2. * f['gamma'] * np.sum(w[:, None] * d, axis=0) / f['scale']
    if f['dev_only']:
        a[:, :3] -= (np.sum(a[:, :3], axis=1) / 3.)[:, None]
    return a


def seeded_stresses(n, seed, size=40.):
    """n seeded stresses of size ~ `size` MPa"""
    return np.random.default_rng(seed).standard_normal((n, 6)) * size


def parent(FE, base, p, sy=None, khard=None):
    """a façade texture material of its own on the data sets of `base` (a material that from_data made a texture material)
    with the tables p installed"""
    m = FE.Material('tex')
    m.dev_only = bool(p['dev_only'])
    with contextlib.redirect_stdout(io.StringIO()):
        m.from_data(list(base.msparam))
    TC.install(m, p)
    if sy is not None:
        m.sy = m.sy0 = float(sy)
    if khard is not None:
        m.khard = float(khard)
    return m


def equal_scale_texture_set(p6, rng, tdim=3):
    """A texture set with EQUAL stress-column scales (scale_seq) but non-zero means and a varying texture column, from the
    6-feature tables p6 (sv, dual, intercept, gamma, scale_seq, dev_only): seeded texture columns and a seeded mean.  Bound
    at a texture it is an exact 6-feature SVC with the one scale scale_seq.  The texture columns stay small, so that the
    folded coefficients keep the size of the given ones and the function still changes sign along rays."""
    n = len(p6['sv'])
    mean = np.concatenate((rng.uniform(-0.2, 0.2, 6) * p6['scale_seq'], rng.uniform(-0.1, 0.1, tdim)))
    scale = np.concatenate((np.full(6, float(p6['scale_seq'])), rng.uniform(0.8, 1.2, tdim)))
    sv = np.concatenate((p6['sv'] - (mean[:6] / scale[:6])[None, :], rng.uniform(-0.2, 0.2, (n, tdim))), axis=1)
    return dict(sv=np.ascontiguousarray(sv), dual=np.array(p6['dual']), intercept=float(p6['intercept']),
                gamma=float(p6['gamma']), mean=mean, scale=scale, dev_only=bool(p6['dev_only']), tdim=tdim)


def j2(s):
    s = np.asarray(s, dtype=float)
    d = s[..., :3] - np.mean(s[..., :3], axis=-1, keepdims=True)
    return np.sqrt(1.5 * (np.sum(d * d, axis=-1) + 2. * np.sum(s[..., 3:] ** 2, axis=-1)))


def locus(f, su, lo=0.5, hi=4000.):
    """factor x per unit stress su (N,6) at which the folded form f first turns from negative to non-negative along the ray
    (a geometric scan, then bisection; NaN where it never does): plain NumPy, so that the seeded points need no device"""
    grid = np.geomspace(lo, hi, 160)
    x = np.full(len(su), np.nan)
    for i, u in enumerate(su):
        y = folded_yf(f, grid[:, None] * u[None, :])
        k = np.nonzero((y[:-1] < 0.) & (y[1:] >= 0.))[0]
        if len(k) == 0:
            continue
        a, b = grid[k[0]], grid[k[0] + 1]
        for _ in range(50):
            c = 0.5 * (a + b)
            if folded_yf(f, (c * u)[None, :])[0] < 0.:
                a = c
            else:
                b = c
        x[i] = 0.5 * (a + b)
    return x


def seeded_points(f, CV, n, seed, scale=(0.5, 1.05), amp=0.6):
    """Points as seeded_points of tests/test_gpu_svc_row.py makes them, around the locus of the folded form f instead of a
    trained sy: stresses along seeded directions at U(scale) of the locus, strain increments N(0, amp x the strain that
    reaches the locus): elastic, on the locus, split and sub-divided calls.  Returns (sig, epl, deps, sy) with sy the
    median J2 stress of the locus along the directions, the flow stress the searches start from."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 6))
    d[:, 3:5] = 0.
    su = d / j2(d)[:, None]
    x = locus(f, su)
    ok = np.isfinite(x)
    assert np.sum(ok) >= max(1, n // 2), 'the folded form changes sign along %d of %d rays only' % (int(np.sum(ok)), n)
    use = np.nonzero(ok)[0][np.arange(n) % int(np.sum(ok))]
    su, x = su[use], x[use]
    sy = float(np.median(x))
    sig = su * (x * rng.uniform(scale[0], scale[1], size=n))[:, None]
    deps = rng.normal(size=(n, 6)) * amp * sy / float(CV[0, 0])
    deps[:, 3:5] = 0.
    return sig, np.zeros((n, 6)), deps, sy

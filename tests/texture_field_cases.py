"""Helpers of the tests of texture fields (Material.at_textures): tables of T textures from the six fixture
textures, a field material with seeded points around its locus, and the comparison of a field against the materials bound
to its rows one by one (Material.at_texture), which is exact: with the host fold shared, both sides execute the
same operations in the same order on the same numbers."""
import numpy as np

import texture_bound_cases as TB


def field_textures(tex6, T, seed=0):
    """T textures (T, tdim): the fixture textures first, then seeded convex combinations of them"""
    tex6 = np.asarray(tex6, dtype=float)
    rng = np.random.default_rng(1000 + seed)
    rows = [tex6[t] for t in range(min(T, len(tex6)))]
    while len(rows) < T:
        w = rng.dirichlet(np.ones(len(tex6)))
        rows.append(w @ tex6)
    return np.ascontiguousarray(np.array(rows))


def field_case(FE, base, p, tex, seed, n=65):
    """(parent, field, CV, sig, epl, deps): a texture material with the tables p, its flow stress set to the median of its locus
    at texture row 0, the field material on the rows tex (T, tdim), and n seeded points around that locus"""
    m = TB.parent(FE, base, p)
    CV = np.array(m.CV)
    sig, epl, deps, sy = TB.seeded_points(TB.fold(p, tex[0]), CV, n, seed)
    m.sy = m.sy0 = sy
    return m, m.at_textures(tex), CV, sig, epl, deps


def field_form(F, CV, sig, epl, deps, ids, maxit):
    """(fy, sig, depl, ct, nsteps, full_yf, status) of the field material at the rows ids"""
    ctx = F._load(CV)
    r = ctx.response(sig, epl, deps, maxit=maxit, tex_id=ids)
    return tuple(r) + tuple(ctx.full_yf(0, sig, epl, tex_id=ids))


def bound_form(m, tex, CV, sig, epl, deps, ids, maxit, bound=None):
    """the same outputs from parent.at_texture(tex[t]) on the points with ids == t, for every t that occurs"""
    n = len(sig)
    out = (np.full(n, np.nan), np.full((n, 6), np.nan), np.full((n, 6), np.nan), np.full((n, 36), np.nan),
           np.full(n, -7, dtype=np.int32), np.full(n, np.nan), np.full(n, -7, dtype=np.int32))
    for t in np.unique(ids):
        b = bound[int(t)] if bound is not None else m.at_texture(tex[t])
        k = np.nonzero(ids == t)[0]
        ctx = b._load(CV)
        s, e, d = (np.ascontiguousarray(a[k]) for a in (sig, epl, deps))
        r = tuple(ctx.response(s, e, d, maxit=maxit)) + tuple(ctx.full_yf(0, s, e))
        for o, a in zip(out, r):
            o[k] = a
    return out


NAMES = ('fy', 'sig', 'depl', 'ct', 'nsteps', 'full_yf', 'status')


def assert_same_bits(name, got, want):
    for what, a, b in zip(NAMES, got, want):
        assert np.array_equal(a, b), '%s: %s differs at %s (largest difference %.3e)' % (
            name, what, np.nonzero(np.atleast_1d(np.any(np.reshape(a != b, (len(a), -1)), axis=1)))[0][:8].tolist(),
            float(np.max(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float)))))

"""Material.yield_scale, yield_stress, polar_yield_locus, polar_field and yield_slices on the device against the fixture
tests/golden/yield_locus.npz (tools/gen_yield_locus.py: the unmodified reference) and against the np.longdouble restatement
of tests/yield_locus_cases.py.

Bars, with U = 4 max(r_ref, 1), A = sum |c_i| k_i + |b| and f_L the restatement (all from the fixture and the tables, none
from what the device returns):
  (1) residual        |f_L(x)| <= U A 2^-53 + |f_L'(x)| 2 ulp(x)           evaluation noise at termination + resolution of x
  (2) the reference   |x - x_ref| <= 2 U A 2^-53 / |f_L'| + 4 ulp(x)       both roots sit in that band; equal status
  (3) polar curves    |s - s_ref| <= (|x_fsolve - x_ref| + bar (2)) calc_seq(snorm) + the calc_seq tolerance of
                      tests/test_gpu_material.py for the material the curve is put through (1e-13 relative on Voigt
                      stresses, 1e-10 absolute on principal stresses): the triangle inequality, no margin of its own
  (4) analytic kinds  2 ulp of get_sflow(epl) / calc_seq(su); against x_ref the family's calc_seq tolerance (relative to x)
                      plus brentq's own resolution xtol + rtol x = 1e-15 + 4 eps x
The terms beyond the issue's wording in (3) and (4) are legs of the same triangle inequality, each from a tolerance that
exists apart from this code; DESIGN.md section 25 gives the reasoning.
Measured on an MI355X (2026-10-19), worst ratio to the bar over all fixture rays: (1) 0.175, (2) 0.153."""
import os
import warnings

import numpy as np
import pytest

import yield_locus_cases as YC

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'yield_locus.npz'))


_runs = {}


def run_case(fx, tag):
    """(material, parameters, x, status) of a fixture case, computed once: default start values where the fixture has none"""
    if tag not in _runs:
        import pylabfea_amd as FE
        m, p = YC.facade_ml(tag) if tag in YC.ML_CASES else (YC.analytic(FE, tag), None)
        su, ep, x0 = fx[tag + '_su'], fx[tag + '_epl'], fx[tag + '_x0']
        x, st = np.empty(len(su)), np.empty(len(su), dtype=np.int32)
        dflt = np.isnan(x0)
        x[dflt], st[dflt] = m.yield_scale(su[dflt], epl=ep[dflt], return_status=True)
        x[~dflt], st[~dflt] = m.yield_scale(su[~dflt], epl=ep[~dflt], x0=x0[~dflt], return_status=True)
        _runs[tag] = (m, p, x, st)
    return _runs[tag]


def U_of(fx, tag):
    return 4. * max(float(fx[tag + '_r_ref']), 1.)


@pytest.mark.parametrize('tag', list(YC.ML_CASES))
def test_residual_and_reference(fx, tag):
    m, p, x, st = run_case(fx, tag)
    su, ep, xr = fx[tag + '_su'], fx[tag + '_epl'], fx[tag + '_x_ref']
    assert np.array_equal(st, fx[tag + '_status'])                    # (2): equal status (all 0)
    U = U_of(fx, tag)
    f, df, A = YC.restate(p, su, ep, x)
    r1 = np.abs(f) / YC.residual_bar(U, df, A, x)
    r2 = np.abs(x - xr) / YC.root_bar(U, df, A, x)
    print('%s: %d rays, worst ratio to bar (1) %.3f, to bar (2) %.3f' % (tag, len(x), float(np.max(r1)), float(np.max(r2))))
    assert np.all(r1 <= 1.)
    assert np.all(r2 <= 1.)


@pytest.mark.parametrize('tag', list(YC.ANA_CASES))
def test_analytic_kinds(fx, tag):
    m, _, x, st = run_case(fx, tag)
    su, ep, xr = fx[tag + '_su'], fx[tag + '_epl'], fx[tag + '_x_ref']
    assert np.all(st == 0)
    own = m.get_sflow(ep) / m.calc_seq(su[:, :3] if m.sdim == 3 else su)
    assert np.all(np.abs(x - own) <= 2. * YC.ulp(own))
    kind, tol = YC.ANA_SEQ_TOL[tag]
    rel = tol if kind == 'rel' else tol / (m.get_sflow(ep) / xr)      # absolute tolerance of seq(su) = sflow / x, as relative
    bar = rel * xr + (1e-15 + 4. * EPS * xr)
    print('%s: worst |x - x_ref| / bar %.3f' % (tag, float(np.max(np.abs(x - xr) / bar))))
    assert np.all(np.abs(x - xr) <= bar)
    # the value of x0 does not enter the closed form, but a start value <= 0 or not finite is a degenerate ray here too
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        x3, st3 = m.yield_scale(su[:4], epl=ep[:4], x0=np.array([0.3, 0., -2., np.inf]), return_status=True)
    assert st3.tolist() == [0, 3, 3, 3] and x3[0] == x[0] and np.all(np.isnan(x3[1:]))


def test_yield_stress_and_single(fx):
    m, p, x, st = run_case(fx, 'hill')
    su = fx['hill_su'][:5]
    ys = m.yield_stress(su)
    assert np.array_equal(ys, su * x[:5, None])
    one = m.yield_scale(su[2])
    assert isinstance(one, float) and one == x[2]
    assert np.array_equal(m.yield_stress(su[2]), su[2] * x[2])
    xs, s1 = m.yield_scale(su[2], return_status=True)
    assert xs == x[2] and s1 == 0
    # epl as calc_yf takes it: a PEEQ value is the tensor PEEQ (1, -1/2, -1/2, 0, 0, 0)
    mw, pw, xw, _ = run_case(fx, 'wh')
    g = fx['wh_group'] == 'lc/1'
    assert np.array_equal(mw.yield_scale(fx['wh_su'][g], epl=0.002), xw[g])
    assert np.array_equal(mw.yield_scale(fx['wh_su'][g], epl=YC.WH_EPL[1]), xw[g])


@pytest.mark.parametrize('tag', ['hill', 'hill3d', 'ahill6'])
def test_polar_curves(fx, tag):
    m = run_case(fx, tag)[0]
    cm = [str(t) for t in fx[tag + '_polar_cmat']]
    theta, s = m.polar_yield_locus(Na=YC.NA_POLAR, cmat=[run_case(fx, t)[0] for t in cm])
    assert np.array_equal(theta, fx[tag + '_polar_theta'])
    sref, snorm = fx[tag + '_polar_syld'], fx[tag + '_polar_snorm']
    assert s.shape == sref.shape == (1 + len(cm), YC.NA_POLAR)
    seqn = m.calc_seq(snorm)
    for c, t in enumerate([tag] + cm):
        xr, xf = fx[tag + '_polar_x_ref'][c], fx[tag + '_polar_x_fsolve'][c]
        if t in YC.ML_CASES:
            _, df, A = YC.restate(YC.ml_params(t), np.c_[snorm, np.zeros((len(snorm), 3))], np.zeros((len(snorm), 6)), xr)
            b2 = YC.root_bar(U_of(fx, t), df, A, xr)
        else:
            kind, tol = YC.ANA_SEQ_TOL[t]
            mt = run_case(fx, t)[0]
            b2 = (tol if kind == 'rel' else tol / (mt.sy / xr)) * xr + (1e-15 + 4. * EPS * xr)
        seqtol = 1e-13 * sref[c] if m.sdim == 6 else 1e-10
        bar = (np.abs(xf - xr) + b2.astype(float)) * seqn + seqtol
        print('%s curve %s: worst |s - s_ref| / bar %.3f (largest bar %.2e)'
              % (tag, t, float(np.max(np.abs(s[c] - sref[c]) / bar)), float(np.max(bar))))
        assert np.all(np.abs(s[c] - sref[c]) <= bar)
    if tag == 'hill':   # scaling and sJ2 (this material's calc_seq is J2: the same curve)
        _, s2 = m.polar_yield_locus(Na=YC.NA_POLAR, scaling=m.sy, sJ2=True)
        assert np.allclose(s2[0] * m.sy, s[0], rtol=1e-12, atol=0.)


# ------------------------------------------------------------------ shapes at which the lane mapping can go wrong
@pytest.mark.parametrize('tag', ['hill', 'hill3d', 'wh'])
def test_batch_sizes_bit_identical(fx, tag):
    m, p, xall, _ = run_case(fx, tag)
    g = np.flatnonzero(np.isnan(fx[tag + '_x0']))[:65]
    if tag == 'wh':
        g = np.flatnonzero(fx['wh_group'] == 'lc/2')[:60]
        g = np.concatenate((g, g[:5]))
    su, ep = fx[tag + '_su'][g], fx[tag + '_epl'][g]
    assert len(su) == 65
    full = m.yield_scale(su, epl=ep)
    assert np.array_equal(full, xall[g])
    for n in (1, 3, 4, 5, 15, 16, 17, 65):
        assert np.array_equal(m.yield_scale(su[:n], epl=ep[:n]), full[:n]), n          # the same ray in a shorter batch
    assert np.array_equal(m.yield_scale(su[::-1], epl=ep[::-1])[::-1], full)          # ... at another batch position
    sh = np.roll(np.arange(65), 7)
    assert np.array_equal(m.yield_scale(su[sh], epl=ep[sh]), full[sh])
    for k in range(65):                                                               # ... and alone
        assert m.yield_scale(su[k], epl=ep[k]) == full[k], k


@pytest.mark.parametrize('tag,nsv', [('hill', 1), ('hill', 15), ('hill', 16), ('hill', 17), ('hill', 31), ('hill', 33),
                                     ('wh', 17), ('hill3d', 1), ('hill3d', 33)])
def test_cut_tables_meet_the_residual_bar(fx, tag, nsv):
    """tables cut to nsv vectors (the loop's remainders: one lane with a lone first vector and 15 with no trip, one trip, a
    lone first vector of a second trip, both), checked by bar (1).  A cut table keeps no yield locus under the full table's
    intercept (0 to 4 of 40 rays cross), so each gets an intercept chosen from its own tables (crossing_intercept) with which
    the march finds a bracket along most rays; the replay of the march with the restatement says along which: at least 20
    of the 40 (ray, start value) pairs, the device must agree on every one of them, and every root meets bar (1) with
    U = 4 max(r_ref, r_np, 1), r_np being what plain FP64 NumPy makes of the same function at the same roots."""
    p = YC.ml_params(tag)
    p = dict(p, sv=p['sv'][:nsv], dual=p['dual'][:nsv])
    g = np.flatnonzero(fx[tag + '_group'] == 'lc/0')[:20]
    su, ep = fx[tag + '_su'][g], fx[tag + '_epl'][g]
    x0s = [YC.default_x0(p, su), 0.3 * fx[tag + '_x_ref'][g]]
    b = YC.crossing_intercept(p, su, ep, x0s)
    m, p = YC.facade_ml(tag, nsv=nsv, intercept=b)
    assert p['intercept'] == b and len(p['sv']) == nsv
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        x, st = m.yield_scale(su, epl=ep, return_status=True)                # default start value: x0s[0]
        x2, st2 = m.yield_scale(su, epl=ep, x0=x0s[1], return_status=True)
    rep = [YC.march_replay(p, su, ep, x0) for x0 in x0s]
    x, st, su, ep = np.concatenate((x, x2)), np.concatenate((st, st2)), np.vstack((su, su)), np.vstack((ep, ep))
    want, clear = np.concatenate([r[0] for r in rep]), np.concatenate([r[1] for r in rep])
    assert np.all((st == 0) | (st == 1)) and np.all(np.isnan(x[st == 1]))
    assert int(np.sum((want == 0) & clear)) >= 20
    assert np.array_equal(st[clear], want[clear])
    ok = st == 0
    f, df, A = YC.restate(p, su[ok], ep[ok], x[ok])
    # r_ref of these functions: no reference run exists for them, so it is formed by the fixture's procedure from an FP64
    # NumPy evaluation of the same formula on the roots compared (as for the synthetic tables of test_gpu_hessian.py).  With
    # few vectors the crossing sits far out on a kernel's tail (gamma |d|^2 near 20), where every FP64 evaluation inherits
    # gamma |d|^2 times the rounding of |d|^2: NumPy itself is 10 to 14 units off there, 1.3 to 1.8 at nsv = 33 and 17 of 15
    r_np = float(np.max(np.abs(YC.restate(p, su[ok], ep[ok], x[ok], LD=np.float64)[0] - f) / (A * YC.EPS53)))
    U = 4. * max(float(fx[tag + '_r_ref']), r_np, 1.)
    r1 = np.abs(f) / YC.residual_bar(U, df, A, x[ok])
    print('%s nsv = %d, intercept %.3g: %d of %d rays have a crossing, r_np %.2f, worst |f_L| in units of A 2^-53 %.2f, '
          'worst ratio to bar (1) %.3f' % (tag, nsv, b, int(np.sum(ok)), len(ok), r_np,
                                           float(np.max(np.abs(f) / (A * YC.EPS53))), float(np.max(r1))))
    assert np.all(r1 <= 1.)


def test_table_too_large_for_lds(fx):
    """the work-hardening table padded with zero-weight vectors beyond what the LDS of a CU holds (16 doubles per vector,
    20480 doubles at most): read from global memory; the padding adds exact zeros to the same partial sums: the same bits"""
    m, p, xall, _ = run_case(fx, 'wh')
    g = np.flatnonzero(fx['wh_group'] == 'lc/1')[:33]
    mp, pp = YC.facade_ml('wh', pad=1400 - len(p['sv']))
    assert len(pp['sv']) * 16 > 20480
    assert np.array_equal(mp.yield_scale(fx['wh_su'][g], epl=fx['wh_epl'][g]), xall[g])


# ------------------------------------------------------------------ status paths
def test_status_paths(fx):
    m, p, xall, _ = run_case(fx, 'hill')
    su, xr = fx['hill_su'][:8], fx['hill_x_ref'][:8]
    U = U_of(fx, 'hill')
    _, df, A = YC.restate(p, su, np.zeros((8, 6)), xr)
    b2 = YC.root_bar(U, df, A, xr)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        bad = np.array(su[:4])
        bad[0] = 0.
        bad[1, 2] = np.nan
        bad[2, 4] = np.inf
        x, st = m.yield_scale(bad, return_status=True)
        assert st.tolist() == [3, 3, 3, 0] and np.all(np.isnan(x[:3])) and x[3] == xall[3]
        assert len(w) == 1 and '3 of 4' in str(w[0].message)          # one warning names the count
        x, st = m.yield_scale(su[:3], x0=np.array([0., -1., np.nan]), return_status=True)
        assert st.tolist() == [3, 3, 3] and np.all(np.isnan(x))
        x, st = m.yield_scale(su[:2], epl=np.array([[np.nan, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0.]]), return_status=True)
        assert st.tolist() == [3, 0]
        # a hydrostatic direction: degenerate without a start value (seq_J2 = 0) ...
        hyd = np.array([[1., 1., 1., 0., 0., 0.]]) * 50.
        md = run_case(fx, 'hilldev')[0]
        assert md.yield_scale(hyd, return_status=True)[1].tolist() == [3]
        # ... and with one, a search along which a dev_only function does not change: no bracket
        x, st = md.yield_scale(hyd, x0=1., return_status=True)
        assert st.tolist() == [1] and np.isnan(x[0])
        # an empty table (no vector carries weight): the function is its intercept
        me, _ = YC.facade_ml('hill', nsv=1)
        me.svc['dual'][:] = 0.
        x, st = me.yield_scale(su, return_status=True)
        assert np.all(st == 1) and np.all(np.isnan(x))
        # start inside: marches up; outside: marches down; both to the reference's root
        xi, si = m.yield_scale(su, x0=0.6 * xr, return_status=True)
        xo, so = m.yield_scale(su, x0=1.5 * xr, return_status=True)
        assert np.all(si == 0) and np.all(so == 0)
        assert np.all(np.abs(xi - xr) <= b2) and np.all(np.abs(xo - xr) <= b2)
        # so far out that every kernel value underflows down to 0.01 x0: the intercept (> 0) offers no crossing
        assert p['intercept'] > 0.
        x, st = m.yield_scale(su, x0=1.e5 * xr, return_status=True)
        assert np.all(st == 1) and np.all(np.isnan(x))
        # a mixed batch keeps each ray's result
        mix = np.array([su[0], 0. * su[1], su[2], su[3], su[4]])
        x0 = np.array([xr[0], 1., 1.e5 * xr[2], 0.6 * xr[3], -1.])
        x, st = m.yield_scale(mix, x0=x0, return_status=True)
        assert st.tolist() == [0, 3, 1, 0, 3]
        assert x[0] == m.yield_scale(su[0], x0=xr[0]) and x[3] == xi[3] and np.all(np.isnan(x[[1, 2, 4]]))
    mel = __import__('pylabfea_amd').Material()
    mel.elasticity(E=200.e3, nu=0.3)
    with pytest.raises(ValueError):
        mel.yield_scale(su)


# ------------------------------------------------------------------ slices and the polar field
@pytest.mark.parametrize('tag', ['hill', 'hill3d', 'wh', 'ahill6', 'abarlat'])
def test_yield_slices(fx, tag):
    m, p, xall, _ = run_case(fx, tag)
    peeq = float(fx[tag + '_slice_peeq'])
    a1, a2 = [c[0] for c in YC.SLICES], [c[1] for c in YC.SLICES]
    sl = m.yield_slices(axis1=a1, axis2=a2, peeq=peeq, Nmesh=YC.NMESH, Na=YC.NA_SLICE, iso=True)
    assert (a1, a2) == ([0, 3], [1, 3]) and len(sl) == 2               # axis code 3 is covered; the lists are not rewritten
    ie = 0 if peeq == 0. else 1
    for j, d in enumerate(sl):
        Zref = fx['%s_slice%d_Z' % (tag, j)]
        assert d['Z'].shape == Zref.shape == d['xx'].shape == (YC.NMESH, YC.NMESH)
        if tag in YC.ML_CASES:
            assert np.array_equal(np.sign(d['Z']), np.sign(Zref))       # exact signs
            assert np.allclose(d['Z'], Zref, rtol=1e-15, atol=0.)
        else:
            assert np.max(np.abs(d['Z'] - Zref)) <= 1e-10 / m.sy        # calc_yf's tolerance (test_gpu_material), / sy
        assert np.array_equal(np.array(d['ellipsis']), fx['ellipsis_default'])
        # the locus against the reference's roots along the same in-plane rays
        g = np.flatnonzero(fx[tag + '_group'] == 'slice%d/%d' % (j, ie))
        assert len(g) == YC.NA_SLICE and d['locus'].shape == (YC.NA_SLICE, 2)
        phi = np.linspace(0., 2. * np.pi, YC.NA_SLICE)
        x = np.hypot(d['locus'][:, 0], d['locus'][:, 1])
        assert np.allclose(d['locus'], np.c_[np.cos(phi), np.sin(phi)] * x[:, None], rtol=1e-15, atol=1e-15)
        xr = fx[tag + '_x_ref'][g]
        if p is not None:
            _, df, A = YC.restate(p, fx[tag + '_su'][g], fx[tag + '_epl'][g], xr)
            bar = YC.root_bar(U_of(fx, tag), df, A, xr) + 2. * YC.ulp(xr)    # hypot of the two coordinates
        else:
            kind, tol = YC.ANA_SEQ_TOL[tag]
            bar = (tol if kind == 'rel' else tol / (m.get_sflow(fx[tag + '_epl'][g]) / xr)) * xr + (1e-15 + 6. * EPS * xr)
        assert np.all(np.abs(x - xr) <= bar), (j, float(np.max(np.abs(x - xr) / bar)))
    if tag == 'hill':   # hydrostatic in-plane rays of code 3 meet no yield locus: NaN rows
        d = m.yield_slices(axis1=[3], axis2=[3], Nmesh=5, Na=9)[0]
        nan = np.isnan(d['locus'][:, 0])
        assert nan.tolist() == [False, True, False, False, False, True, False, False, False]
        ref = m.yield_slices(axis1=[0], axis2=[1], Nmesh=5, Na=9, ref_mat=run_case(fx, 'ahill6')[0], scaling=False)[0]
        assert ref['Z_ref'].shape == (5, 5) and ref['xx'][0, 0] == -2. * m.sy


def test_polar_field(fx):
    m, p, _, _ = run_case(fx, 'hill3d')
    th, r, Z = m.polar_field(Np=YC.NP_FIELD)
    Zref = fx['hill3d_field_Z']
    assert th.shape == r.shape == Z.shape == Zref.shape
    lin = np.linspace(-1., 1., YC.NP_FIELD)
    assert np.array_equal(th[0], lin * np.pi) and np.array_equal(r[:, 0], (lin + 1.) * m.scale_seq)
    # the decision function's gauge on the grid of features: U (sum |c_i| k_i + |b|) 2^-53
    LD = YC.LD
    feat = np.c_[np.repeat(lin, YC.NP_FIELD), np.tile(lin, YC.NP_FIELD)].astype(LD)
    d2 = np.sum((feat[:, None, :] - p['sv'].astype(LD)[None, :, :]) ** 2, axis=2)
    A = (np.sum(np.abs(p['dual']).astype(LD) * np.exp(-LD(p['gamma']) * d2), axis=1) + abs(p['intercept'])).reshape(Z.shape)
    bar = (U_of(fx, 'hill3d') * A * YC.EPS53).astype(float)
    print('polar_field: worst |Z - Z_ref| / gauge %.3f' % float(np.max(np.abs(Z - Zref) / bar)))
    # pointwise; the entries that the symmetrisation clipped all carry the value of ONE grid point (the extreme of the other
    # sign), whose gauge is not theirs: the largest gauge of the grid covers it
    clipped = (Zref == np.max(Zref)) | (Zref == np.min(Zref))
    assert 1 < int(np.sum(clipped)) < Zref.size
    assert np.all(np.abs(Z - Zref) <= np.where(clipped, np.max(bar), bar))
    _, _, Zp = m.polar_field(Np=YC.NP_FIELD, predict=True)
    assert np.array_equal(Zp, fx['hill3d_field_Zpred'])
    with pytest.raises(ValueError):
        run_case(fx, 'hill')[0].polar_field()

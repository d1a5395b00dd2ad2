"""Texture materials bound to one texture on the GPU (Material.at_texture): the per-column instantiations of the
16-lane row kernels (PLFX_SVC6_COLS) at the point level against the thread-per-point texture kernels of §32, which share no
code with them above response_point; placement; the pin to the 6-feature row kernels where all six scales are equal; models
against the CPU oracle (an equal-scale set is an exact 6-feature SVC) and on the anisotropic fixture fit; calc_properties;
the conventions of the C-ABI.

Bars (those of tests/test_gpu_svc_row.py): sig and fy 1e-6 sy, depl 1e-9, tangent 1e-5 CV[0,0], ML_full_yf 1e-6 sy with equal
status, model fields 2e-6 relative.  nsteps equal except where the thread form's own fy lies within 1e-5 sy of +-toler
(toler = 5e-3 sflow), at most 2 % of a case.  Measured worst values are in DESIGN.md §34."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import texture_bound_cases as TB
import texture_cases as TC
import texture_flow_cases as TF
import yield_locus_cases as YC
from test_gpu_model import FE, make_material

pytestmark = pytest.mark.gpu

MAXIT = 5
NPTS = 65


@pytest.fixture(scope='module')
def z():
    return TC.load()


@pytest.fixture(scope='module')
def base(z, tmp_path_factory):
    d = tmp_path_factory.mktemp('texture_db')
    return {desc: TC.facade(FE(), z, d, desc)[0] for desc in TC.DESCRIPTORS}


def bound_case(base, p, tex, seed, n=NPTS, desc='GSH_3'):
    """(parent, bound, CV, sig, epl, deps): a texture material with the tables p, its flow stress set to the median of its
    locus at the texture, bound there, and n seeded points around that locus"""
    m = TB.parent(FE(), base[desc], p)
    CV = np.array(m.CV)
    sig, epl, deps, sy = TB.seeded_points(TB.fold(p, tex), CV, n, seed)
    m.sy = m.sy0 = sy
    return m, m.at_texture(tex), CV, sig, epl, deps


def thread_form(m, CV, sig, epl, deps, tex, maxit=MAXIT):
    return m._load_tex_flow(CV).tex_svc_response(sig, epl, deps, np.ascontiguousarray(tex[None, :]), maxit=maxit)


def row_form(b, CV, sig, epl, deps, maxit=MAXIT):
    return b._load(CV).response(sig, epl, deps, maxit=maxit)


def compare(name, row, thr, sy, CV, both_phases=True):
    """the row form against the thread form under the bars of the module docstring; returns the measured worst values"""
    fy, so, dp, ct, ns = row
    fy2, so2, dp2, ct2, ns2 = thr
    toler = 5e-3 * sy
    near = np.abs(np.abs(fy2) - toler) < 1e-5 * sy
    assert np.mean(near) <= 0.02, (name, int(np.sum(near)))
    ok = ~near
    if both_phases:
        assert np.any(ns2[ok] == 0) and np.any(ns2[ok] == MAXIT - 1), (name, np.bincount(ns2 + 1))
    w = dict(sig=float(np.max(np.abs(so - so2)[ok])) / sy, fy=float(np.max(np.abs(fy - fy2)[ok])) / sy,
             depl=float(np.max(np.abs(dp - dp2)[ok])), ct=float(np.max(np.abs(ct - ct2)[ok])) / CV[0, 0])
    print('%s: n %d, excluded %d, nsteps %s, sig %.2e sy, fy %.2e sy, depl %.2e, ct %.2e CV00'
          % (name, len(fy), int(np.sum(near)), np.bincount(ns2 + 1).tolist(), w['sig'], w['fy'], w['depl'], w['ct']))
    assert np.array_equal(ns[ok], ns2[ok]), (name, np.nonzero(ns != ns2)[0])
    assert w['sig'] < 1e-6 and w['fy'] < 1e-6 and w['depl'] < 1e-9 and w['ct'] < 1e-5, (name, w)
    return w


def compare_full_yf(name, m, b, CV, sig, tex, sy):
    f, st = b._load(CV).full_yf(0, sig)
    f2, st2 = m._load_tex_flow(CV).tex_svc_full_yf(sig, np.ascontiguousarray(tex[None, :]))
    print('%s: ML_full_yf %.2e sy, status %s' % (name, float(np.max(np.abs(f - f2))) / sy, np.bincount(st2).tolist()))
    assert np.array_equal(st, st2), name
    assert np.max(np.abs(f - f2)) < 1e-6 * sy, name


def cut64(z, desc, dev, tex):
    p = TC.tables(z, desc, dev)
    q = TC.cut(p, nsv=64)
    return TC.cut(q, intercept=TC.crossing_intercept(q, tex))


# ------------------------------------------------------------------------------------------------ (1) point level
@pytest.mark.parametrize('dev', [False, True])
@pytest.mark.parametrize('desc', TC.DESCRIPTORS)
def test_fits_cut_to_64_vectors_against_the_thread_kernels(z, base, desc, dev):
    tex = TC.textures(z, desc)[1]
    p = cut64(z, desc, dev, tex)
    m, b, CV, sig, epl, deps = bound_case(base, p, tex, 20 + dev, desc=desc)
    assert float(np.max(b._bound['scale']) / np.min(b._bound['scale'])) > 1.5      # anisotropic scales (dev_only: 1.9, else 5.7)
    full = row_form(b, CV, sig, epl, deps)
    compare('%s dev %d' % (desc, dev), full, thread_form(m, CV, sig, epl, deps, tex), m.sy, CV)
    compare_full_yf('%s dev %d' % (desc, dev), m, b, CV, sig, tex, m.sy)
    for n in (1, 31, 33):                                                        # batch sizes: the bits of the full batch
        part = row_form(b, CV, sig[:n], epl[:n], deps[:n])
        assert all(np.array_equal(a, c[:n]) for a, c in zip(part, full)), n


@pytest.mark.parametrize('tdim', [1, 3, 10])
@pytest.mark.parametrize('nsv', [1, 15, 16, 17, 33, 63, 64, 65])
def test_table_sizes_against_the_thread_kernels(z, base, nsv, tdim):
    """the 16-lane trip and the padding to 64 x the padded widths of the texture kernels"""
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    if tdim == 10:
        p, tex = TC.widen(p, tex, 10)
    elif tdim == 1:
        p, tex = TC.cut(p, tdim=1), np.ascontiguousarray(tex[:, :1])
    t = tex[2]
    q = TC.cut(p, nsv=nsv)
    q = TC.cut(q, intercept=TC.crossing_intercept(q, t))
    m, b, CV, sig, epl, deps = bound_case(base, q, t, 1000 + 16 * nsv + tdim)
    n = (1, 31, 33, 65)[(nsv + tdim) % 4]
    full = row_form(b, CV, sig, epl, deps)
    compare('nsv %d tdim %d' % (nsv, tdim), full, thread_form(m, CV, sig, epl, deps, t), m.sy, CV)
    part = row_form(b, CV, sig[:n], epl[:n], deps[:n])
    assert all(np.array_equal(a, c[:n]) for a, c in zip(part, full)), n
    compare_full_yf('nsv %d tdim %d' % (nsv, tdim), m, b, CV, sig[:33], t, m.sy)


@pytest.mark.parametrize('rows,n', [(522, 64), (2240, 16)])
def test_whole_fit_and_tables_past_the_lds(z, base, rows, n):
    """the whole GSH_3 fit, and the fit padded past the LDS of a CU (tables read from device memory)"""
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')[0]
    assert len(p['sv']) == 522
    if rows > 522:
        p = TC.cut(p, pad=rows - 522)
    m, b, CV, sig, epl, deps = bound_case(base, p, tex, 40 + n, n=n)
    full = row_form(b, CV, sig, epl, deps)
    compare('%d rows' % rows, full, thread_form(m, CV, sig, epl, deps, tex), m.sy, CV)
    compare_full_yf('%d rows' % rows, m, b, CV, sig, tex, m.sy)
    # the façade's own calls (maxit = 50) on a few points
    k = 4
    r = b.response_batch(sig[:k], epl[:k], deps[:k], CV)
    t = m.response_batch(sig[:k], epl[:k], deps[:k], CV, tex=tex)
    compare('%d rows, response_batch' % rows, (r[0], r[1], r[2], r[3].reshape(k, 36), r[4]),
            (t[0], t[1], t[2], t[3].reshape(k, 36), t[4]), m.sy, CV, both_phases=False)


# ------------------------------------------------------------------------------------------------ (2) placement
def test_placement_single_calls_and_nan_rows(z, base):
    tex = TC.textures(z, 'GSH_3')[1]
    m, b, CV, sig, epl, deps = bound_case(base, cut64(z, 'GSH_3', False, tex), tex, 20)
    full = b.response_batch(sig, epl, deps, CV)
    assert np.all(full[4] >= 0) and np.all(np.isfinite(full[1]))
    rng = np.random.default_rng(3)
    for perm in (np.arange(NPTS)[::-1], rng.permutation(NPTS), np.array([7]), np.arange(5, 38)):
        part = b.response_batch(sig[perm], epl[perm], deps[perm], CV)
        assert all(np.array_equal(a, c[perm]) for a, c in zip(part, full))
    for i in (0, 13, 64):
        fy, so, dp, ct = b.response(sig[i], epl[i], deps[i], CV)
        assert fy == full[0][i] and np.array_equal(so, full[1][i]) and np.array_equal(dp, full[2][i])
        assert np.array_equal(ct, full[3][i]) and b.msg['nsteps'] == full[4][i]
    bad = deps.copy()
    bad[9, 2] = np.nan
    got = b.response_batch(sig, epl, bad, CV)
    assert got[4][9] == -1 and all(np.all(np.isnan(a[9])) for a in got[:4])
    keep = np.arange(NPTS) != 9
    assert all(np.array_equal(a[keep], c[keep]) for a, c in zip(got, full))
    # the delegated point functions are the parent's at the bound texture
    assert np.array_equal(b.calc_yf(sig), m.calc_yf(sig, tex=tex))
    assert np.array_equal(b.calc_fgrad(sig), m.calc_fgrad(sig, tex=tex))
    su = sig[:8] / TB.j2(sig[:8])[:, None]
    assert np.array_equal(b.yield_scale(su), m.yield_scale(su, tex=tex))
    assert np.array_equal(b.yield_stress(su), m.yield_stress(su, tex=tex))
    assert np.array_equal(b.calc_seq(sig), m.calc_seq(sig))
    a = b.calc_fgrad(sig[0])
    ct = b.C_tan(sig[0], CV)
    ca = CV @ a
    assert np.allclose(ct, CV - np.outer(ca, ca) / (a @ ca + b.khard), rtol=1e-14, atol=0.)


# ------------------------------------------------------------------------------------------------ (3) pin to the 6-feature kernels
@pytest.mark.parametrize('dev', [False, True])
def test_equal_scales_are_the_six_feature_row_kernels(z, base, dev):
    m6, p6 = YC.facade_ml('hill')
    if dev:
        p6 = TF.deviatoric_tables(p6)
        m6.set_svc(p6['sv'], p6['dual'], p6['intercept'], p6['gamma'], p6['scale_seq'], dev_only=True)
    CV = np.array(m6.CV)
    p7, c = TF.six_feature_as_texture(p6)
    mt = TB.parent(FE(), base['GSH_3'], p7)
    mt.elasticity(CV=CV)
    mt.sy, mt.sy0, mt.khard, mt.hill, mt.drucker = m6.sy, m6.sy, m6.khard, np.array(m6.hill), m6.drucker
    mt.hill_6p, mt.hill_3p = m6.hill_6p, m6.hill_3p
    b = mt.at_texture(c)
    assert np.all(b._bound['scale'] == p6['scale_seq']) and np.array_equal(b.svc['dual'], p6['dual'])
    assert np.array_equal(b.svc['sv'], p6['sv'])
    f6 = dict(sv=p6['sv'], dual=p6['dual'], intercept=p6['intercept'], gamma=p6['gamma'], scale=np.full(6, p6['scale_seq']),
              dev_only=bool(dev))
    sig, epl, deps, _ = TB.seeded_points(f6, CV, NPTS, 60 + dev)
    for maxit in (MAXIT, 50):
        row = b._load(CV).response(sig, epl, deps, maxit=maxit)
        six = m6._load(CV).response(sig, epl, deps, maxit=maxit)
        assert m6._load(CV).svc_info()[:2] == (1, 0)                              # the 6-feature side on its row kernels
        assert np.array_equal(row[4], six[4])
        assert np.any(six[4] == 0) and np.any(six[4] == maxit - 1)
        sy = m6.sy
        w = (np.max(np.abs(row[1] - six[1])) / sy, np.max(np.abs(row[0] - six[0])) / sy, np.max(np.abs(row[2] - six[2])),
             np.max(np.abs(row[3] - six[3])) / CV[0, 0])
        print('dev %d maxit %d: sig %.2e sy, fy %.2e sy, depl %.2e, ct %.2e CV00; equal bits: %s'
              % (dev, maxit, w[0], w[1], w[2], w[3], all(np.array_equal(a, c) for a, c in zip(row, six))))
        assert w[0] < 1e-6 and w[1] < 1e-6 and w[2] < 1e-9 and w[3] < 1e-5
    f, st = b._load(CV).full_yf(0, sig)
    f2, st2 = m6._load(CV).full_yf(0, sig)
    assert np.array_equal(st, st2) and np.max(np.abs(f - f2)) < 1e-6 * m6.sy


# ------------------------------------------------------------------------------------------------ (4) model against the oracle
def six_feature_material(parent, f, num):
    """the folded tables as a façade 6-feature SVC material (equal scales): what the CPU oracle can run"""
    assert np.all(f['scale'] == f['scale'][0])
    m = FE().Material(name='folded', num=num)
    m.elasticity(CV=np.array(parent.CV))
    m.plasticity(sy=parent.sy, sdim=6)
    m.hill, m.hill_6p, m.hill_3p = np.array(parent.hill), parent.hill_6p, parent.hill_3p
    m.set_svc(f['sv'], f['dual'], f['intercept'], f['gamma'], float(f['scale'][0]), dev_only=f['dev_only'])
    return m


def laminate(mats):
    fe = FE().Model(dim=2, planestress=False)
    fe.geom([2, 1, 2], LY=4.)
    fe.assign(mats)
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.0014 * fe.leny, 'disp')
    fe.mesh(NX=10, NY=7)
    return fe


_oracle = {}


@pytest.mark.parametrize('big', [False, True])
def test_two_bound_phases_in_one_model_vs_oracle(z, base, golden_dir, big):
    """big: the tables padded past the LDS with zero coefficients, the same function -- one oracle run serves both"""
    from oracle.solve_ref import RefSolver
    p6 = YC.ml_params('hill')
    q = TB.equal_scale_texture_set(p6, np.random.default_rng(11))
    if big:
        q = TC.cut(q, pad=2240 - len(q['sv']))
    par = TB.parent(FE(), base['GSH_3'], q)
    par.elasticity(CV=np.load(os.path.join(golden_dir, 'svc_hill.npz'))['par_CV'])
    par.sy = par.sy0 = p6['sy']
    tA, tB = np.array([0.1, -0.1, 0.05]), np.array([-0.15, 0.1, 0.1])
    fA, fB = par.fold_texture(tA), par.fold_texture(tB)
    assert np.max(np.abs(fA['dual'] - fB['dual'])) > 1e-3 * np.max(np.abs(fA['dual']))
    bA, bB, j2 = par.at_texture(tA), par.at_texture(tB), make_material('j2')
    bA.num, j2.num, bB.num = 1, 2, 3
    fe = laminate([bA, j2, bB])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=6)
        if 'ref' not in _oracle:
            n = len(p6['sv'])
            cutf = lambda f: dict(f, sv=f['sv'][:n], dual=f['dual'][:n])
            assert not np.any(fA['dual'][n:]) and not np.any(fB['dual'][n:])
            _oracle['ref'] = RefSolver(laminate([six_feature_material(par, cutf(fA), 1), make_material('j2'),
                                                 six_feature_material(par, cutf(fB), 3)])).solve(min_step=6)
        ref = _oracle['ref']
    row, thread, nrow, nthread = fe._engine.svc_info()
    assert row == 0b101 and thread == 0 and nthread == 0 and nrow >= 2 * fe.n_sweeps
    assert fe.nsteps == ref.nsteps and list(fe.niter) == list(ref.niter)
    mid = fe._mat_id
    epl = fe._state('epl')
    assert np.max(np.abs(epl[mid == 0])) > 0. and np.max(np.abs(epl[mid == 2])) > 0.         # both bound phases yield
    s = np.max(np.abs(ref.sig))
    w = (np.max(np.abs(fe.u - ref.u)) / np.max(np.abs(ref.u)), np.max(np.abs(fe._state('sig') - ref.sig)) / s,
         np.max(np.abs(epl - ref.epl)) / np.max(np.abs(ref.eps)), np.max(np.abs(fe.sgl - ref.sgl)) / s)
    print('big %d: nsteps %d, u %.2e, sig %.2e, epl %.2e, sgl %.2e' % ((big, fe.nsteps) + w))
    assert max(w) < 2e-6


# ------------------------------------------------------------------------------------------------ (5) model on the anisotropic fit
@pytest.mark.parametrize('dev', [False, True])
def test_model_on_the_anisotropic_fit(z, base, dev):
    p, tex = TC.tables(z, 'GSH_3', dev), TC.textures(z, 'GSH_3')
    par = TB.parent(FE(), base['GSH_3'], p)
    su_y = np.array([0., 1., 0., 0., 0., 0.])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ys = [float(par.yield_scale(su_y, tex=tex[k])) for k in (0, 1)]
    assert np.all(np.isfinite(ys))
    bs = [par.at_texture(tex[k]) for k in (0, 1)]
    fe = FE().Model(dim=2, planestress=True)
    fe.geom([1, 1], LY=2.)
    fe.assign(bs)
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(1.5 * max(ys) / par.E * fe.leny, 'disp')
    fe.mesh(NX=8, NY=6)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve()
    row, thread, nrow, nthread = fe._engine.svc_info()
    assert row == 0b11 and thread == 0 and nthread == 0
    mid, sig, epl = fe._mat_id, fe._state('sig'), fe._state('epl')
    toler = 5e-3 * par.sy
    for k in (0, 1):
        assert np.max(np.abs(epl[mid == k])) > 0.
        yf = par.calc_yf(sig[mid == k], tex=tex[k])
        print('dev %d section %d: ys %.3f, max calc_yf %.3e (toler %.3e), max |epl| %.2e'
              % (dev, k, ys[k], float(np.max(yf)), toler, float(np.max(np.abs(epl[mid == k])))))
        assert np.max(yf) <= toler
    mean = np.mean(sig, axis=0)
    assert np.max(np.abs(fe.sgl[-1] - mean)) <= 1e-9 * np.max(np.abs(mean))
    assert np.all(np.isfinite(fe.field('seq'))) and np.all(np.isfinite(fe.field_range('seq')))


# ------------------------------------------------------------------------------------------------ (6) calc_properties
def test_calc_properties(z, base):
    p, tex = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')[0]
    par = TB.parent(FE(), base['GSH_3'], p)
    b = par.at_texture(tex)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        b.calc_properties(load_cases=['stx', 'sty'], eps=1.5 * float(par.yield_scale(np.array([1., 0., 0., 0., 0., 0.]), tex=tex)) / par.E)
        for case, su in (('stx', [1., 0., 0., 0., 0., 0.]), ('sty', [0., 1., 0., 0., 0., 0.])):
            want = float(b.calc_seq(par.yield_stress(np.array(su), tex=tex)))
            got = float(b.prop[case]['ys'])
            print('%s: ys %.4f, yield_stress(tex=) %.4f, ratio %.4f' % (case, got, want, got / want))
            assert abs(got / want - 1.) <= 0.02


# ------------------------------------------------------------------------------------------------ (7) library conventions
def test_library_conventions(z, base, monkeypatch):
    from pylabfea_amd import _lib
    tex = TC.textures(z, 'GSH_3')[1]
    m, b, CV, sig, epl, deps = bound_case(base, cut64(z, 'GSH_3', False, tex), tex, 20, n=33)
    six = (C.c_double * 6)(*b._bound['scale'])
    ctx = _lib.Context(0)
    try:
        assert ctx.lib.plfx_set_svc_cols(ctx.h, 0, six) == -3                     # before materials
        ctx.set_materials([b._record(CV, ana=True)])
        assert ctx.lib.plfx_set_svc_cols(ctx.h, 0, six) == -4                     # another kind
        rec = b._record(CV)
        arr = (_lib.CMaterial * 1)(rec[0])
        assert ctx.lib.plfx_set_materials(ctx.h, 1, arr) == 0                     # (no column scales sent: all scale_seq)
        assert ctx.svc_info()[:2] == (1, 0)
        equal = ctx.response(sig, epl, deps, maxit=MAXIT)
        for bad in (0., np.nan, -1., np.inf):
            s = np.array(b._bound['scale'])
            s[4] = bad
            assert ctx.lib.plfx_set_svc_cols(ctx.h, 0, (C.c_double * 6)(*s)) == -2
        assert ctx.lib.plfx_set_svc_cols(ctx.h, 1, six) == -2
        assert all(np.array_equal(a, c) for a, c in zip(ctx.response(sig, epl, deps, maxit=MAXIT), equal))
        assert ctx.lib.plfx_set_svc_cols(ctx.h, 0, six) == 0
        cols = ctx.response(sig, epl, deps, maxit=MAXIT)
        assert not np.array_equal(cols[1], equal[1])
        assert all(np.array_equal(a, c) for a, c in zip(cols, row_form(b, CV, sig, epl, deps)))
        assert ctx.lib.plfx_set_materials(ctx.h, 1, arr) == 0                     # the next set_materials: equal scales again
        assert all(np.array_equal(a, c) for a, c in zip(ctx.response(sig, epl, deps, maxit=MAXIT), equal))
        n = len(sig)
        out = np.empty((n, 36))
        st = np.empty(n, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert ctx.lib.plfx_fgrad_batch(ctx.h, 0, n, p(sig), p(out)) == -4
        assert ctx.lib.plfx_hessian_batch(ctx.h, 0, n, p(sig), None, p(out)) == -4
        assert ctx.lib.plfx_yield_scale(ctx.h, 0, n, p(sig), None, None, p(out), p(st)) == -4
        assert ctx.lib.plfx_yf_batch(ctx.h, 0, n, p(sig), p(epl), p(out)) == -4
        ctx.set_materials([rec])                                                   # (sends the column scales)
        assert all(np.array_equal(a, c) for a, c in zip(ctx.response(sig, epl, deps, maxit=MAXIT), cols))
    finally:
        ctx.close()
    monkeypatch.setenv('PLFX_SVC_WAVE', '0')                                      # read at plfx_create
    c2 = _lib.Context(0)
    try:
        c2.set_materials([b._record(CV)])
        assert c2.svc_info()[:2] == (1, 0)
        assert all(np.array_equal(a, c) for a, c in zip(c2.response(sig, epl, deps, maxit=MAXIT), cols))
        f, st = c2.full_yf(0, sig)
        f2, st2 = b._load(CV).full_yf(0, sig)
        assert np.array_equal(f, f2) and np.array_equal(st, st2)
    finally:
        c2.close()

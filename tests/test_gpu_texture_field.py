"""Texture fields on the GPU (Material.at_textures, Model.set_texture_ids): the TEXF instantiations of the
16-lane row kernels, which read the dual coefficient of a point from the coefficient row of its texture.

The yardstick is the material bound to one texture (Material.at_texture), and the bar is equal bits: with the
host fold shared (fold_textures is fold_texture row by row), a point with row t and the same point of at_texture(tex[t])
execute the same operations in the same order on the same numbers -- the coefficient comes from another address, nothing
else differs.  A case that differs is a finding, not a tolerance to widen.  Model fields are held to the 2e-6 of §34's model
check besides, with the measured deviation printed."""
import ctypes as C
import warnings

import numpy as np
import pytest

import texture_bound_cases as TB
import texture_cases as TC
import texture_field_cases as TX
import yield_locus_cases as YC
from test_gpu_model import FE

pytestmark = pytest.mark.gpu

NPTS = 65


@pytest.fixture(scope='module')
def z():
    return TC.load()


@pytest.fixture(scope='module')
def base(z, tmp_path_factory):
    d = tmp_path_factory.mktemp('texture_db')
    return {desc: TC.facade(FE(), z, d, desc)[0] for desc in TC.DESCRIPTORS}


def cut_tables(z, desc, dev, nsv, tex0):
    q = TC.cut(TC.tables(z, desc, dev), nsv=nsv)
    return TC.cut(q, intercept=TC.crossing_intercept(q, tex0))


# ------------------------------------------------------------------------------------------------ (1) points
@pytest.mark.parametrize('dev', [False, True])
@pytest.mark.parametrize('nsv', [1, 63, 64, 65])
@pytest.mark.parametrize('T', [1, 2, 5, 17])
def test_points_against_the_bound_materials(z, base, T, nsv, dev):
    desc = 'GSH_3' if nsv in (1, 64) else 'GSH_7'
    tex = TX.field_textures(TC.textures(z, desc), T, seed=T)
    p = cut_tables(z, desc, dev, nsv, tex[0])
    m, F, CV, sig, epl, deps = TX.field_case(FE(), base[desc], p, tex, 3000 + 100 * T + nsv + dev)
    ids = np.random.default_rng(T + nsv).integers(0, T, NPTS).astype(np.int32)
    ids[:min(T, NPTS)] = np.arange(min(T, NPTS))                                  # every row occurs
    bound = {t: m.at_texture(tex[t]) for t in range(T)}
    for maxit in (5, 50):
        got = TX.field_form(F, CV, sig, epl, deps, ids, maxit)
        want = TX.bound_form(m, tex, CV, sig, epl, deps, ids, maxit, bound)
        assert np.all(want[4] >= 0) and np.all(np.isfinite(want[1]))
        TX.assert_same_bits('T %d nsv %d dev %d maxit %d' % (T, nsv, dev, maxit), got, want)
    # the façade's calls are those launches
    r = F.response_batch(sig, epl, deps, CV, tex_id=ids)
    assert all(np.array_equal(a.reshape(len(sig), -1), b.reshape(len(sig), -1)) for a, b in zip(r, got[:5]))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert np.array_equal(F.ML_full_yf(sig, tex_id=ids), bound_full_yf(bound, sig, ids))
    n = (1, 31, 33, 65)[(T + nsv + dev) % 4]                                      # a batch prefix: the bits of the full batch
    part = TX.field_form(F, CV, sig[:n], epl[:n], deps[:n], ids[:n], 50)
    assert all(np.array_equal(a, b[:n]) for a, b in zip(part, got)), n


def bound_full_yf(bound, sig, ids):
    out = np.full(len(sig), np.nan)
    for t in np.unique(ids):
        out[ids == t] = bound[int(t)].ML_full_yf(sig[ids == t], verb=False)
    return out


def test_placement_and_rows_of_a_wave(z, base):
    """batch prefixes, reversed and shuffled order, the four rows of a wave on four textures and all on one, the default row,
    response at one point, the delegated calls"""
    T = 5
    tex = TX.field_textures(TC.textures(z, 'GSH_3'), T)
    m, F, CV, sig, epl, deps = TX.field_case(FE(), base['GSH_3'], cut_tables(z, 'GSH_3', False, 64, tex[0]), tex, 77)
    bound = {t: m.at_texture(tex[t]) for t in range(T)}
    mixed = (np.arange(NPTS) % T).astype(np.int32)                                 # neighbouring rows of a wave: different textures
    full = TX.field_form(F, CV, sig, epl, deps, mixed, 50)
    TX.assert_same_bits('mixed', full, TX.bound_form(m, tex, CV, sig, epl, deps, mixed, 50, bound))
    assert np.any(full[4] == 0) and np.any(full[4] == 49)                          # elastic / one-step and sub-divided points
    for n in (1, 31, 33, 65):
        part = TX.field_form(F, CV, sig[:n], epl[:n], deps[:n], mixed[:n], 50)
        assert all(np.array_equal(a, b[:n]) for a, b in zip(part, full)), n
    rng = np.random.default_rng(5)
    for perm in (np.arange(NPTS)[::-1], rng.permutation(NPTS), np.arange(5, 38)):
        part = TX.field_form(F, CV, sig[perm], epl[perm], deps[perm], mixed[perm], 50)
        assert all(np.array_equal(a, b[perm]) for a, b in zip(part, full))
    same = np.full(NPTS, 3, dtype=np.int32)                                        # all rows of every wave on one texture
    one = TX.field_form(F, CV, sig, epl, deps, same, 50)
    TX.assert_same_bits('same', one, TX.bound_form(m, tex, CV, sig, epl, deps, same, 50, bound))
    r3 = F.response_batch(sig, epl, deps, CV, tex_id=3)                            # an int is shared by the points
    assert all(np.array_equal(a.reshape(NPTS, -1), b.reshape(NPTS, -1)) for a, b in zip(r3, one[:5]))
    r0 = F.response_batch(sig, epl, deps, CV)                                      # the default is row 0
    b0 = bound[0].response_batch(sig, epl, deps, CV)
    assert all(np.array_equal(a, b) for a, b in zip(r0, b0))
    for i in (0, 13, 64):
        fy, so, dp, ct = F.response(sig[i], epl[i], deps[i], CV, tex_id=int(mixed[i]))
        assert fy == full[0][i] and np.array_equal(so, full[1][i]) and np.array_equal(dp, full[2][i])
        assert np.array_equal(ct.reshape(36), full[3][i]) and F.msg['nsteps'] == full[4][i]
    bad = deps.copy()
    bad[9, 2] = np.nan                                                             # a masked row keeps the others' rows in step
    got = F.response_batch(sig, epl, bad, CV, tex_id=mixed)
    keep = np.arange(NPTS) != 9
    assert got[4][9] == -1 and all(np.array_equal(a.reshape(NPTS, -1)[keep], b.reshape(NPTS, -1)[keep]) for a, b in zip(got, full[:5]))
    # the delegated point functions are the parent's at the rows' textures
    assert np.array_equal(F.calc_yf(sig, tex_id=mixed), m.calc_yf(sig, tex=tex[mixed]))
    assert np.array_equal(F.calc_yf(sig, tex_id=2), m.calc_yf(sig, tex=tex[2]))
    assert np.array_equal(F.calc_yf(sig), bound[0].calc_yf(sig))
    assert np.array_equal(F.calc_fgrad(sig, tex_id=mixed), m.calc_fgrad(sig, tex=tex[mixed]))
    su = sig[:8] / TB.j2(sig[:8])[:, None]
    with warnings.catch_warnings():                                                # (rays without a root are NaN on both sides)
        warnings.simplefilter('ignore')
        x = F.yield_scale(su, tex_id=mixed[:8])
        assert np.any(np.isfinite(x)) and np.array_equal(x, m.yield_scale(su, tex=tex[mixed[:8]]), equal_nan=True)
        assert np.array_equal(F.yield_stress(su, tex_id=1), m.yield_stress(su, tex=tex[1]), equal_nan=True)


def test_tables_past_the_lds(z, base):
    """the GSH_3 fit padded to 2240 rows: the tables are read from device memory (INLDS = false), 16 points"""
    tex = TX.field_textures(TC.textures(z, 'GSH_3'), 3)
    p = TC.cut(TC.tables(z, 'GSH_3'), pad=2240 - 522)
    m, F, CV, sig, epl, deps = TX.field_case(FE(), base['GSH_3'], p, tex, 56, n=16)
    ids = (np.arange(16) % 3).astype(np.int32)
    for maxit in (5, 50):
        got = TX.field_form(F, CV, sig, epl, deps, ids, maxit)
        TX.assert_same_bits('2240 rows maxit %d' % maxit, got, TX.bound_form(m, tex, CV, sig, epl, deps, ids, maxit))
    info = F._load(CV).svc_textures_info(0)
    assert info['rows'] == 3 and info['staged'] is False


# ------------------------------------------------------------------------------------------------ (2) model against the element-map form
def laminate(mats, elmts=None, planestress=False, NX=10, NY=7, top=0.0005):
    """the laminate of §34's model check (4); top strain 5e-4: the load at which the three textures of the map leave some
    elements elastic (59 of 70 yield; at 7e-4 and above all do)"""
    fe = FE().Model(dim=2, planestress=planestress)
    fe.geom([2, 1, 2], LY=4.)
    fe.assign(mats)
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(top * fe.leny, 'disp')
    if elmts is None:
        fe.mesh(NX=NX, NY=NY)
    else:
        fe.mesh(elmts=elmts)
    return fe


def solved(fe, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(**kw)
    return fe


def deviation(fe, ref):
    """the relative measures of §34's model check (4) and whether every array has the bits of the reference model's"""
    a = {k: (fe._state(k), ref._state(k)) for k in ('sig', 'epl')}
    s = np.max(np.abs(a['sig'][1]))
    w = (np.max(np.abs(fe.u - ref.u)) / np.max(np.abs(ref.u)), np.max(np.abs(a['sig'][0] - a['sig'][1])) / s,
         np.max(np.abs(a['epl'][0] - a['epl'][1])) / np.max(np.abs(ref._state('eps'))), np.max(np.abs(fe.sgl - ref.sgl)) / s)
    bits = (np.array_equal(fe.u, ref.u) and np.array_equal(fe.sgl, ref.sgl) and
            all(np.array_equal(x, y) for x, y in a.values()))
    return w, bits


@pytest.mark.parametrize('big', [False, True])
def test_model_against_the_element_map_form(z, base, golden_dir, big):
    """T = 3 on a seeded random map of 10 x 7 elements, plane strain: one field material with set_texture_ids against three
    bound materials placed by mesh(elmts=).  big: the tables padded past the LDS with zero coefficients."""
    import os
    p6 = YC.ml_params('hill')
    q = TB.equal_scale_texture_set(p6, np.random.default_rng(11))
    if big:
        q = TC.cut(q, pad=2240 - len(q['sv']))
    par = TB.parent(FE(), base['GSH_3'], q)
    par.elasticity(CV=np.load(os.path.join(golden_dir, 'svc_hill.npz'))['par_CV'])
    par.sy = par.sy0 = p6['sy']
    tex = np.array([[0.1, -0.1, 0.05], [-0.15, 0.1, 0.1], [0.05, 0.15, -0.1]])
    tmap = np.random.default_rng(21).integers(0, 3, (10, 7))
    assert all(np.any(tmap == t) for t in range(3))
    ref = solved(laminate([par.at_texture(t) for t in tex], elmts=tmap + 1), min_step=6)
    F = par.at_textures(tex)
    fe = laminate([F, F, F])
    fe.set_texture_ids(tmap)
    solved(fe, min_step=6)
    assert fe.nsteps == ref.nsteps and list(fe.niter) == list(ref.niter)
    w, bits = deviation(fe, ref)
    print('big %d: nsteps %d, u %.2e, sig %.2e, epl %.2e, sgl %.2e; equal bits: %s' % ((big, fe.nsteps) + w + (bits,)))
    assert max(w) < 2e-6
    epl = fe._state('epl')
    assert np.any(epl != 0.) and np.any(np.all(epl == 0., axis=1))                  # both phases occur
    row, thread, nrow, nthread = fe._engine.svc_info()
    info = fe._engine.svc_textures_info(0)
    assert row == 0b1 and thread == 0 and nthread == 0 and info['rows'] == 3
    assert info['launches'] >= 2 * fe.n_sweeps and info['launches'] >= nrow          # the sweeps and calc_scf took the field kernels
    assert np.array_equal(fe.texture_ids, tmap.reshape(-1))
    assert np.all(np.isfinite(fe.field('seq'))) and np.array_equal(fe.field('seq'), ref.field('seq'))
    fe.calc_global()
    assert np.all(np.isfinite(fe.glob['sig']))


# ------------------------------------------------------------------------------------------------ (3) more textures than materials
def model24(par, mats, ids=None, elmts=None, top=None):
    fe = FE().Model(dim=2, planestress=True)
    fe.geom([1, 1], LY=2.)
    fe.assign(mats)
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(top * fe.leny, 'disp')
    fe.mesh(NX=12, NY=8)
    if ids is not None:
        fe.set_texture_ids(ids)
    return solved(fe)


@pytest.fixture(scope='module')
def case24(z, base):
    p, tex6 = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    par = TB.parent(FE(), base['GSH_3'], p)
    su_y = np.array([0., 1., 0., 0., 0., 0.])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ys = [float(par.yield_scale(su_y, tex=t)) for t in tex6[:5]]
    assert np.all(np.isfinite(ys))
    ids = np.random.default_rng(24).permutation(96) % 24                          # all 24 rows, four elements each
    return par, tex6, ids.reshape(12, 8), 1.5 * max(ys) / par.E


def test_24_equal_rows_are_the_bound_material(case24):
    par, tex6, ids, top = case24
    b = par.at_texture(tex6[0])
    ref = model24(par, [b, b], top=top)
    fe = model24(par, [par.at_textures(np.tile(tex6[0], (24, 1)))] * 2, ids, top=top)
    assert fe.nsteps == ref.nsteps and list(fe.niter) == list(ref.niter)
    w, bits = deviation(fe, ref)
    assert bits, w
    assert np.any(fe._state('epl') != 0.)
    assert fe._engine.svc_textures_info(0)['rows'] == 24


def test_24_distinct_rows_permuted_and_on_the_locus(case24):
    par, tex6, ids, top = case24
    tex = TX.field_textures(tex6, 24, seed=3)
    assert len(np.unique(np.round(tex, 12), axis=0)) == 24
    fe = model24(par, [par.at_textures(tex)] * 2, ids, top=top)
    perm = np.random.default_rng(8).permutation(24)                                # row perm[t] of the new table is texture t
    inv = np.empty(24, dtype=int)
    inv[perm] = np.arange(24)
    tex2 = tex[inv]
    assert np.array_equal(tex2[perm[ids]], tex[ids])
    fe2 = model24(par, [par.at_textures(tex2)] * 2, perm[ids], top=top)
    assert fe2.nsteps == fe.nsteps and list(fe2.niter) == list(fe.niter)
    w, bits = deviation(fe2, fe)
    assert bits, w
    # check (5) of §34: the plastic elements lie on the locus of their own texture
    sig, epl, flat = fe._state('sig'), fe._state('epl'), ids.reshape(-1)
    plastic = np.any(epl != 0., axis=1)
    assert np.sum(plastic) > 0
    toler = 5e-3 * par.sy
    yf = par.calc_yf(sig[plastic], tex=tex[flat[plastic]])
    print('T = 24: %d of 96 elements plastic on %d textures, max calc_yf %.3e (toler %.3e)'
          % (int(np.sum(plastic)), len(np.unique(flat[plastic])), float(np.max(yf)), toler))
    assert np.max(yf) <= toler
    mean = np.mean(sig, axis=0)
    assert np.max(np.abs(fe.sgl[-1] - mean)) <= 1e-9 * np.max(np.abs(mean))
    assert np.all(np.isfinite(fe.field('seq'))) and np.all(np.isfinite(fe.field_range('seq')))


# ------------------------------------------------------------------------------------------------ (4) lifetime and calls
def test_library_conventions(z, base):
    from pylabfea_amd import _lib
    T = 3
    tex = TX.field_textures(TC.textures(z, 'GSH_3'), T)
    m, F, CV, sig, epl, deps = TX.field_case(FE(), base['GSH_3'], cut_tables(z, 'GSH_3', False, 64, tex[0]), tex, 20, n=33)
    n, nsv = len(sig), 64
    coef = np.ascontiguousarray(F._bound['coef'])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ids = (np.arange(n) % T).astype(np.int32)
    ctx = _lib.Context(0)
    try:
        lib = ctx.lib
        assert lib.plfx_set_svc_textures(ctx.h, 0, T, p(coef)) == -3                # before materials
        ctx.set_materials([F._record(CV, ana=True)])
        assert lib.plfx_set_svc_textures(ctx.h, 0, T, p(coef)) == -4                # another kind
        b0 = m.at_texture(tex[0])
        ctx.set_materials([b0._record(CV)])                                         # the plain COLS material (row 0's coefficients)
        assert ctx.svc_textures_info(0) == dict(rows=0, staged=False, launches=0)
        plain = ctx.response(sig, epl, deps, maxit=5)
        plain_f = ctx.full_yf(0, sig, epl)
        bad = coef.copy()
        bad[1, 7] = np.nan
        assert lib.plfx_set_svc_textures(ctx.h, 0, T, p(bad)) == -2                 # a NaN coefficient
        assert lib.plfx_set_svc_textures(ctx.h, 0, -1, p(coef)) == -2
        assert lib.plfx_set_svc_textures(ctx.h, 1, T, p(coef)) == -2
        assert lib.plfx_set_svc_textures(ctx.h, 0, 2 ** 31 // 64, p(coef)) == -2    # ntex * rowpad beyond INT32_MAX (checked first)
        assert ctx.svc_textures_info(0)['rows'] == 0
        assert all(np.array_equal(a, c) for a, c in zip(ctx.response(sig, epl, deps, maxit=5), plain))
        ctx.set_svc_textures(0, coef)
        assert ctx.svc_textures_info(0) == dict(rows=T, staged=False, launches=0)
        want = TX.bound_form(m, tex, CV, sig, epl, deps, ids, 5)
        got = tuple(ctx.response(sig, epl, deps, maxit=5, tex_id=ids)) + tuple(ctx.full_yf(0, sig, epl, tex_id=ids))
        TX.assert_same_bits('attached', got, want)
        assert ctx.svc_textures_info(0)['launches'] == 2
        assert not np.array_equal(got[1], plain[1])
        # NULL ids and the old entry points: row 0
        assert all(np.array_equal(a, c) for a, c in zip(ctx.response(sig, epl, deps, maxit=5), plain))
        assert all(np.array_equal(a, c) for a, c in zip(ctx.full_yf(0, sig, epl), plain_f))
        # an index outside the table in a _tid call: -2, nothing launched
        nl = ctx.svc_textures_info(0)['launches']
        out = [np.empty(n), np.empty((n, 6)), np.empty((n, 6)), np.empty((n, 36)), np.empty(n, dtype=np.int32)]
        for badid in (T, -1):
            bid = ids.copy()
            bid[17] = badid
            assert lib.plfx_response_batch_tid(ctx.h, n, None, p(sig), p(epl), p(deps), *[p(a) for a in out], p(bid)) == -2
            assert lib.plfx_full_yf_batch_tid(ctx.h, 0, n, p(sig), p(epl), None, p(out[0]), p(out[4]), p(bid)) == -2
        assert ctx.svc_textures_info(0)['launches'] == nl
        # n = 0
        assert lib.plfx_response_batch_tid(ctx.h, 0, None, p(sig), p(epl), p(deps), *[p(a) for a in out], p(ids)) == 0
        assert lib.plfx_full_yf_batch_tid(ctx.h, 0, 0, p(sig), p(epl), None, p(out[0]), p(out[4]), p(ids)) == 0
        # ntex = 0 detaches: the plain material again, and ids are ignored
        ctx.set_svc_textures(0, None)
        assert ctx.svc_textures_info(0) == dict(rows=0, staged=False, launches=0)
        assert all(np.array_equal(a, c) for a, c in zip(ctx.response(sig, epl, deps, maxit=5, tex_id=ids), plain))
        assert all(np.array_equal(a, c) for a, c in zip(ctx.full_yf(0, sig, epl), plain_f))
        # ... and so does the next plfx_set_materials
        ctx.set_svc_textures(0, coef)
        rec = b0._record(CV)
        arr = (_lib.CMaterial * 1)(rec[0])
        assert lib.plfx_set_materials(ctx.h, 1, arr) == 0
        ctx.set_svc_cols(0, b0._bound['scale'])
        assert ctx.svc_textures_info(0)['rows'] == 0
        assert all(np.array_equal(a, c) for a, c in zip(ctx.response(sig, epl, deps, maxit=5), plain))
    finally:
        ctx.close()


def test_element_rows_out_of_range_and_between_two_solves(z, base):
    """a bad element row is PLFX_ERR_ARG when the sweep is set up; set_texture_ids between two chained solves changes the
    second solve only, and re-sends the index array alone"""
    p, tex6 = TC.tables(z, 'GSH_3'), TC.textures(z, 'GSH_3')
    par = TB.parent(FE(), base['GSH_3'], p)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        top = 0.6 * float(par.yield_scale(np.array([0., 1., 0., 0., 0., 0.]), tex=tex6[0])) / par.E
    F = par.at_textures(tex6[:3])
    rng = np.random.default_rng(2)
    idsA, idsB = rng.integers(0, 3, (6, 4)), rng.integers(0, 3, (6, 4))

    def model(ids):
        fe = FE().Model(dim=2, planestress=True)
        fe.geom([1, 1], LY=2.)
        fe.assign([F, F])
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(top * fe.leny, 'disp')
        fe.mesh(NX=6, NY=4)
        if ids is not None:
            fe.set_texture_ids(ids)
        return fe
    one = solved(model(idsA))
    first = (one.u.copy(), one._state('sig').copy(), one._state('epl').copy())
    eng = one._engine
    one.set_texture_ids(idsB)
    one.bctop(2. * top * one.leny, 'disp')
    solved(one)
    assert one._engine is eng                                                      # the engine, its materials and its mesh stay
    assert not np.array_equal(one._state('sig'), first[1])
    # the second solve continues from the state the first left: the same chain with the rows switched by hand
    two = solved(model(idsA))
    assert all(np.array_equal(a, b) for a, b in zip((two.u, two._state('sig'), two._state('epl')), first))
    two._engine.set_element_textures(idsB.reshape(-1))
    two._tex_ids_sent = two._tex_ids
    two.bctop(2. * top * two.leny, 'disp')
    solved(two)
    assert np.array_equal(two.u, one.u) and np.array_equal(two._state('sig'), one._state('sig'))
    assert np.any(one._state('epl') != 0.)
    # a row outside the table, sent past the façade's check: the sweep answers PLFX_ERR_ARG before it launches
    e = two._engine
    bad = idsB.reshape(-1).astype(np.int32)
    bad[5] = 3
    e.set_element_textures(bad)
    nl = e.svc_textures_info(0)['launches']
    ch, cv = C.c_int(), C.c_int()
    assert e.lib.plfx_sweep(e.h, 0, C.byref(ch), C.byref(cv)) == -2
    assert e.svc_textures_info(0)['launches'] == nl
    e.set_element_textures(None)                                                   # NULL clears it: row 0 everywhere
    assert e.lib.plfx_sweep(e.h, 0, C.byref(ch), C.byref(cv)) == 0
    with pytest.raises(ValueError, match='outside 0..2'):                          # the façade's own check
        bad_model = model(np.full((6, 4), 3))
        bad_model.solve()

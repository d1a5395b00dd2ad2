"""Model.field / fields / field_range and plfx_element_fields: the sixteen element fields of the
reference's Model.plot as arrays from one device pass, and their colour-bar ranges reduced on the device.

Bars.  The component selectors and ux / uy repeat one product (or four exact ones and three sums in the reference's order):
np.array_equal.  seq, seqJ2, peeq, etot are about ten roundings of positive terms under a square root: 8 * 2.2e-16 * max|field|
(derived, not measured).  Against the reference's recorded fields the bar is that of a solve against the reference in
tests/test_gpu_sweep_prefetch.py: RTOL = 1e-6 of max(max|reference field|, scale of the underlying state array).
Measured deviations are printed in units of their bars (pytest -s) and quoted in DESIGN section 23."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import model_fields_cases as cases
from test_gpu_sharded import build_strip, collect, free_port
from test_gpu_sweep_prefetch import RTOL, hill, mixed_model

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
DEVICE_FIELDS = ('strain1', 'strain2', 'strain12', 'stress1', 'stress2', 'stress12', 'plastic1', 'plastic2', 'plastic12',
                 'seq', 'seqJ2', 'peeq', 'etot', 'ux', 'uy')
ALL = DEVICE_FIELDS + ('mat',)
GOSS = [0.81766901, -0.36431565, 0.31238124, 0.84321164, -0.01812166, 0.8320893, 0.35952332,
        0.08127502, 1.29314957, 1.0956107, 0.90916744, 0.27655112, 1.090482, 1.18282173,
        -0.01897814, 0.90539357, 1.88256105, 0.0127306]


def FE():
    import pylabfea_amd
    return pylabfea_amd


def laminate(nx, ny, eps, ly, mats):
    fe = FE().Model(dim=2, planestress=False)
    fe.geom([2, 1, 2], LY=ly)
    fe.assign(mats)
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(eps * fe.leny, 'disp')
    fe.mesh(NX=nx, NY=ny)
    return fe


def elastic(num=3):
    el = FE().Material(num=num)
    el.elasticity(E=50.e3, nu=0.25)
    return el


def make(tag):
    """15: fixture case a (Hill-6 | J2 sdim 3 | elastic); 255: 17 x 15, every material plastic (the end of a load step
    exchanges sig and res_sig); 257: one row of 257 square elements (one element in the second block); 1160: 40 x 29"""
    if tag == 15:
        return cases.build(FE(), 'a')
    if tag == 255:
        return laminate(17, 15, 0.01, 5., [hill(1), hill(2, 80.), hill(3, 60.)])
    if tag == 257:
        return laminate(257, 1, 0.01, 5. / 257., [hill(1), elastic(), hill(2, 60.)])
    return mixed_model(40, 29, 0.01)


def solved(tag):
    fe = make(tag)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=2)
    return fe


def expected(fe):
    """the expressions of the issue's table on the model's own state arrays"""
    sig, eps, epl, u = fe._state('sig'), fe._state('eps'), fe._state('epl'), fe.u
    from pylabfea_amd.basic import eps_eq, sig_eq_j2
    x = {'strain1': eps[:, 0] * 100, 'strain2': eps[:, 1] * 100, 'strain12': eps[:, 5] * 100,
         'stress1': sig[:, 0], 'stress2': sig[:, 1], 'stress12': sig[:, 5],
         'plastic1': epl[:, 0] * 100, 'plastic2': epl[:, 1] * 100, 'plastic12': epl[:, 5] * 100,
         'seqJ2': sig_eq_j2(sig), 'peeq': eps_eq(epl) * 100, 'etot': eps_eq(eps) * 100}
    mid = np.asarray(fe._mat_id)
    seq = np.zeros(fe.Nel)
    for k, m in enumerate(fe.mat):
        if np.any(mid == k):
            seq[mid == k] = m.calc_seq(sig[mid == k])
    x['seq'] = seq
    conn = np.asarray(fe._conn, dtype=np.int64)
    for d, name in enumerate(('ux', 'uy')):
        hh = np.zeros(fe.Nel)
        for k in range(4):
            hh += u[2 * conn[:, k] + d] * 0.25
        x[name] = hh
    x['mat'] = np.array([m.num for m in fe.mat], dtype=float)[mid]
    return x


@pytest.mark.parametrize('tag', [15, 255, 257, 1160])
def test_fields_against_own_state_and_no_side_effect(tag):
    fe, twin = solved(tag), solved(tag)
    assert fe.Nel == tag
    # immediately after solve(), before any element getter: on the all-plastic model sig and res_sig are still exchanged.
    # (The stored eps is current here -- solve() ends by reading u, which brings it up to date; the strain formed from u
    # while eps is really behind it is test_strain_from_u_* below.)
    got = fe.fields(ALL)
    x = expected(fe)
    for n in ('strain1', 'strain2', 'strain12', 'stress1', 'stress2', 'stress12', 'plastic1', 'plastic2', 'plastic12',
              'ux', 'uy', 'mat'):
        assert got[n].dtype == np.float64 and got[n].shape == (fe.Nel,)
        assert np.array_equal(got[n], x[n]), n
    assert np.max(np.abs(got['stress2'])) > 0. and np.max(got['peeq']) > 0. and np.max(np.abs(got['uy'])) > 0.
    for n in ('seq', 'seqJ2', 'peeq', 'etot'):
        bar = 8 * EPS * np.max(np.abs(x[n]))
        dev = np.max(np.abs(got[n] - x[n]))
        print('fields vs own state, %d elements, %s: %.3f bars%s' % (tag, n, dev / bar, ' (bit-identical)' if dev == 0. else ''))
        assert dev <= bar, (n, dev, bar)
    # the call changed nothing: state, and the solve that follows, equal those of a twin that never asked for a field
    for q in ('eps', 'sig', 'res_sig', 'epl'):
        assert np.array_equal(fe._state(q), twin._state(q)), q
    for m in (fe, twin):
        m.bctop(0.012 * m.leny, 'disp')
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m.solve(min_step=2)
    assert np.array_equal(fe.u, twin.u) and fe.nsteps == twin.nsteps
    for q in ('sig', 'eps', 'epl'):
        assert np.array_equal(fe._state(q), twin._state(q)), q


def test_exchanged_sig_at_the_moment_of_the_call():
    """on the all-plastic model the end of the load step exchanged sig and res_sig: the fields asked right after solve()
    equal those asked after res_sig has been read out of the exchanged buffer and written apart again"""
    fe = solved(255)
    first = fe.fields(DEVICE_FIELDS)
    fe._state('eps'), fe._state('res_sig')     # res_sig read out of the exchanged buffer
    eng = fe._ensure_engine()
    from pylabfea_amd import _lib
    eng.state_set(_lib.ST_RES_SIG, np.zeros((fe.Nel, 6)))   # two buffers again (split_res_sig), scratch overwritten
    fe._cache = {}
    again = fe.fields(DEVICE_FIELDS)
    for n in DEVICE_FIELDS:
        assert np.array_equal(first[n], again[n]), n


STRAIN = ('strain1', 'strain2', 'strain12', 'etot', 'ux', 'uy', 'stress2', 'peeq')


@pytest.mark.parametrize('tag', [255, 1160])
def test_strain_from_u_inside_the_load_step_loop(tag):
    """The stored eps is really behind u only between the end of a load step and the next read of u or eps.  The step
    hook of Model.solve runs exactly there: the engine is asked for the fields after EVERY load step of a solve that stops
    after four, no getter in between.  The stored eps is then the zero field of the reset (nothing has written it), so a
    kernel that read it, or a call that marked it current without writing it, cannot match: the strain rows of the last
    step must be array_equal to _state('eps') read after the solve, those of the step before must differ from them, and
    state and the continued solve must equal those of a twin without the hook."""
    from pylabfea_amd import _lib
    from pylabfea_amd.basic import eps_eq
    ids = [_lib.FIELD_ID[n] for n in STRAIN]
    fe, twin = make(tag), make(tag)
    seen = {}

    def hook(il):
        rows, rng = fe._engine.element_fields(ids, want_range=True)
        seen[il] = (rows, rng)
    fe._step_hook = hook
    for m in (fe, twin):
        m._max_load_steps = 4
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m.solve(min_step=8)
    assert sorted(seen) == [1, 2, 3, 4] and fe.nsteps == twin.nsteps
    rows, rng = seen[4]
    got = dict(zip(STRAIN, rows))
    eps, u = fe._state('eps'), fe.u
    assert np.max(np.abs(eps)) > 0.
    assert np.array_equal(got['strain1'], eps[:, 0] * 100) and np.array_equal(got['strain2'], eps[:, 1] * 100)
    assert np.array_equal(got['strain12'], eps[:, 5] * 100)
    want = eps_eq(eps) * 100
    assert np.max(np.abs(got['etot'] - want)) <= 8 * EPS * np.max(want)
    x = expected(fe)
    for n in ('ux', 'uy', 'stress2'):
        assert np.array_equal(got[n], x[n]), n
    assert np.max(np.abs(got['peeq'] - x['peeq'])) <= 8 * EPS * max(np.max(x['peeq']), 1e-300)
    for k, n in enumerate(STRAIN):           # the ranges of that same pass
        assert rng[k, 0] == np.amin(got[n]) and rng[k, 1] == np.amax(got[n]), n
    before = dict(zip(STRAIN, seen[3][0]))   # the step before: another u, another strain -- and no stored copy of either
    assert not np.array_equal(before['strain2'], got['strain2']) and np.max(np.abs(before['strain2'])) > 0.
    for q in ('eps', 'sig', 'res_sig', 'epl'):
        assert np.array_equal(fe._state(q), twin._state(q)), q
    assert np.array_equal(u, twin.u)
    fe._step_hook = None
    for m in (fe, twin):
        m._max_load_steps = None
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m.solve(min_step=8)
    assert np.array_equal(fe.u, twin.u) and fe.nsteps == twin.nsteps
    for q in ('sig', 'eps', 'epl'):
        assert np.array_equal(fe._state(q), twin._state(q)), q


def test_strain_from_u_after_update_state():
    """The same through the library alone: plfx_update_state leaves the stored eps behind u.  The strain selectors asked
    right then come from u -- the stored field is still the zero field of the reset -- and equal eps read afterwards."""
    from pylabfea_amd import _lib
    m, el = hill(1), elastic()
    eng = _lib.Context(0)
    eng.set_materials([m._record(np.array(m.CV, dtype=float)), el._record(np.array(el.CV, dtype=float))])
    nx, ny = 19, 14                                   # 266 elements: a partial second block; two classes
    eng.set_mesh_structured(nx, ny, np.full(nx, 0.5), 0.25, 1., False, mat_col=(np.arange(nx) % 2).astype(np.int32))
    eng.set_grid(nx, ny)
    eng.state_reset()
    eng.assemble()
    rng = np.random.default_rng(4)
    eng.state_set(_lib.ST_DU, rng.normal(size=eng.ndof) * 1e-3)
    eng.update_state()                                # u += du; sig, epl updated; eps not stored
    names = ('strain1', 'strain2', 'strain12', 'etot', 'ux', 'stress1')
    rows, r = eng.element_fields([_lib.FIELD_ID[n] for n in names], want_range=True)
    only_range = eng.element_fields([_lib.FIELD_ID['strain12']], want_out=False, want_range=True)[1]
    eps, sig = eng.state_get(_lib.ST_EPS), eng.state_get(_lib.ST_SIG)     # ensure_eps runs here, not before
    assert np.min(np.abs(eps[:, [0, 1, 5]])) > 0.
    assert np.array_equal(rows[0], eps[:, 0] * 100) and np.array_equal(rows[1], eps[:, 1] * 100)
    assert np.array_equal(rows[2], eps[:, 5] * 100) and np.array_equal(rows[5], sig[:, 0])
    from pylabfea_amd.basic import eps_eq
    assert np.max(np.abs(rows[3] - eps_eq(eps) * 100)) <= 8 * EPS * np.max(eps_eq(eps) * 100)
    assert tuple(only_range[0]) == (np.amin(rows[2]), np.amax(rows[2])) == tuple(r[2])
    again, _ = eng.element_fields([_lib.FIELD_ID[n] for n in names])     # now from the stored columns: the same bits
    assert np.array_equal(again, rows)
    eng.close()


def test_fields_equal_single_calls():
    fe = solved(1160)
    single = {}
    for n in ALL:
        fe._cache = {}             # every call a device pass of its own
        single[n] = fe.field(n).copy()
    fe._cache = {}
    both = fe.fields(ALL)
    perm = list(np.random.default_rng(5).permutation(ALL)) + ['seq', 'stress2']
    fe._cache = {}
    mixed = fe.fields(perm)
    for n in ALL:
        assert np.array_equal(both[n], single[n]), n
        assert np.array_equal(mixed[n], single[n]), n
    # the library itself with a repeated selector: both rows
    from pylabfea_amd import _lib
    ids = [_lib.FIELD_ID[n] for n in ('seq', 'uy', 'seq', 'strain12', 'uy')]
    rows, rng = fe._ensure_engine().element_fields(ids, want_range=True)
    for r, n in zip(rows, ('seq', 'uy', 'seq', 'strain12', 'uy')):
        assert np.array_equal(r, single[n]), n
    assert np.array_equal(rng[0], rng[2]) and np.array_equal(rng[1], rng[4])
    assert rng[0, 0] == np.amin(single['seq']) and rng[0, 1] == np.amax(single['seq'])
    with pytest.raises(KeyError):
        fe.field('stress3')
    with pytest.raises(KeyError):
        fe.field_range('nope')
    with pytest.raises(NotImplementedError):
        fe.plot('seq')


def floor_of(z, c, n):
    """scale of the state array under a field, as tests/test_gpu_sweep_prefetch.py compares it against the reference"""
    if n in ('stress1', 'stress2', 'stress12', 'seq', 'seqJ2'):
        return np.max(np.abs(z[c + '_sig']))
    if n in ('ux', 'uy'):
        return np.max(np.abs(z[c + '_u']))
    return 100. * np.max(np.abs(z[c + '_eps']))   # strains in per cent; epl on the scale of eps


@pytest.mark.parametrize('c', ['a', 'b', 'c', 'd'])
def test_reference_parity(golden_dir, c):
    z = np.load(os.path.join(golden_dir, 'model_fields.npz'))
    fe = cases.build(FE(), c)
    if cases.CASES[c]['solve']:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fe.solve()
        assert fe.nsteps == int(z[c + '_nsteps'])
    got = fe.fields(ALL)
    assert np.array_equal(got['mat'], z[c + '_f_mat'])
    worst = 0.
    for n in DEVICE_FIELDS:
        ref = z['%s_f_%s' % (c, n)]
        bar = RTOL * max(np.max(np.abs(ref)), floor_of(z, c, n))
        dev = np.max(np.abs(got[n] - ref))
        worst = max(worst, dev / bar if bar > 0. else (0. if dev == 0. else np.inf))
        assert dev <= bar, (c, n, dev, bar)
    for n in ALL:
        want = z['%s_r_%s' % (c, n)]
        ref = z['%s_f_%s' % (c, n)]
        bar = RTOL * max(np.max(np.abs(ref)), 0. if n == 'mat' else floor_of(z, c, n))
        r = fe.field_range(n)
        dev = max(abs(r[0] - want[0]), abs(r[1] - want[1]))
        # the recorded limits carry the colour bar's own roundings, 4 ulp (tests/test_fields_cpu.py): all an all-zero field allows
        bar = max(bar, 4 * EPS * np.max(np.abs(want)))
        worst = max(worst, dev / bar)
        assert dev <= bar, (c, n, r, want)
        lo, hi = float(np.amin(got[n])), float(np.amax(got[n]))
        assert fe.field_range(n, vmin=-7.5) == (-7.5, hi)         # a given limit is honoured, and switches auto-scale off
        assert fe.field_range(n, vmax=1234.) == (lo, 1234.)
        assert fe.field_range(n, vmin=0.25, vmax=0.26) == (0.25, 0.26)
    print('reference parity, case %s: worst deviation %.3g bars' % (c, worst))


def material_table(golden_dir):
    F = FE()
    tr = F.Material(num=1)
    tr.elasticity(E=200.e3, nu=0.3)
    tr.plasticity(sy=100., tresca=True)
    b0 = F.Material(num=2)
    b0.elasticity(E=151220., nu=0.3)
    b0.plasticity(sy=46.76, barlat=GOSS, barlat_exp=8)
    b1 = F.Material(num=3)
    b1.elasticity(E=151220., nu=0.3)
    b1.plasticity(sy=46.76, barlat=GOSS, barlat_exp=6)
    b1.enable_barlat_normal()
    h3 = F.Material(num=4)
    h3.elasticity(E=200.e3, nu=0.3)
    h3.plasticity(sy=150., hill=[0.7, 1., 1.4], khard=0., sdim=3)
    ml = F.Material(name='loaded', num=5)
    ml.from_MLparam('abq_ML-J2_C15_G25', path=os.path.join(golden_dir, 'mlparam'))
    return [tr, b0, b1, h3, ml]


def test_seq_by_material_kind_without_a_solve(golden_dir):
    """An engine whose table holds Tresca, Barlat without and with the native normal, Hill-3 on principal stresses and a
    6-feature SVC material accepts the table (only a sweep or a response call refuses a material without flow rule), so the
    field is tested: random stresses with out-of-plane shear, seq against every material's calc_seq."""
    from pylabfea_amd import _lib
    mats = material_table(golden_dir)
    eng = _lib.Context(0)
    eng.set_materials([m._record(np.array(m.CV, dtype=float)) for m in mats])
    nx, ny = 10, 7
    mat_col = np.repeat(np.arange(5), 2)
    eng.set_mesh_structured(nx, ny, np.ones(nx), 1., 1., False, mat_col=mat_col)
    rng = np.random.default_rng(11)
    sig = rng.normal(size=(nx * ny, 6)) * 60.
    assert np.all(sig[:, 3] != 0.) and np.all(sig[:, 4] != 0.)
    eng.state_set(_lib.ST_SIG, sig)
    rows, _ = eng.element_fields([_lib.FIELD_ID['seq'], _lib.FIELD_ID['seqJ2']])
    mid = np.repeat(mat_col, ny)
    from pylabfea_amd.basic import sig_eq_j2
    want = np.zeros(nx * ny)
    for k, m in enumerate(mats):
        want[mid == k] = m.calc_seq(sig[mid == k])
    for k, m in enumerate(mats):
        bar = 8 * EPS * np.max(np.abs(want[mid == k]))
        dev = np.max(np.abs(rows[0][mid == k] - want[mid == k]))
        print('seq by kind, material %d (kind %d): %.3f bars' % (k, m._record(np.array(m.CV))[0].kind, dev / bar))
        assert dev <= bar, (k, dev, bar)
    assert np.max(np.abs(rows[1] - sig_eq_j2(sig))) <= 8 * EPS * np.max(sig_eq_j2(sig))
    assert not np.allclose(rows[0], rows[1])     # the kinds differ from J2
    eng.close()


def small_engine(nel_x=257):
    from pylabfea_amd import _lib
    m = hill(1)
    eng = _lib.Context(0)
    eng.set_materials([m._record(np.array(m.CV, dtype=float))])
    eng.set_mesh_structured(nel_x, 1, np.ones(nel_x), 1., 1., False, mat_col=np.zeros(nel_x, dtype=np.int32))
    return eng


def test_range_nan_and_positions():
    from pylabfea_amd import _lib
    ids = [_lib.FIELD_ID[n] for n in ('stress1', 'stress2', 'seqJ2')]
    eng = small_engine(257)
    rng = np.random.default_rng(2)
    sig = rng.normal(size=(257, 6))
    sig[256, 0], sig[0, 0] = 50., -50.          # maximum in the last, partial block; minimum in element 0
    sig[0, 1], sig[256, 1] = 70., -70.          # and the other way round
    eng.state_set(_lib.ST_SIG, sig)
    rows, r = eng.element_fields(ids, want_range=True)
    assert tuple(r[0]) == (-50., 50.) and tuple(r[1]) == (-70., 70.)
    assert r[2, 0] == np.amin(rows[2]) and r[2, 1] == np.amax(rows[2])
    none, r2 = eng.element_fields(ids, want_out=False, want_range=True)     # out = NULL
    assert none is None and np.array_equal(r, r2)
    sig[130, 0] = np.nan                         # a NaN comes out as NaN, as np.amin / np.amax give it
    eng.state_set(_lib.ST_SIG, sig)
    _, r3 = eng.element_fields(ids, want_out=False, want_range=True)
    assert np.all(np.isnan(r3[0])) and tuple(r3[1]) == (-70., 70.) and np.all(np.isnan(r3[2]))
    eng.close()
    # through the façade
    fe = solved(257)
    eng = fe._ensure_engine()
    s = eng.state_get(_lib.ST_SIG)
    s[256, 0] = np.nan
    eng.state_set(_lib.ST_SIG, s)
    fe._cache = {}
    r = fe.field_range('stress1')
    assert np.isnan(r[0]) and np.isnan(r[1])
    lo, hi = fe.field_range('stress2')
    assert np.isfinite(lo) and np.isfinite(hi) and lo <= hi
    f = fe.field('stress2')
    from pylabfea_amd.model import autoscale_range
    assert (lo, hi) == autoscale_range(float(np.amin(f)), float(np.amax(f)))


def test_library_edges():
    from pylabfea_amd import _lib
    lib = _lib.load()
    m = hill(1)
    eng = _lib.Context(0)
    eng.set_materials([m._record(np.array(m.CV, dtype=float))])
    sel = np.array([_lib.FIELD_ID['seq']], dtype=np.int32)
    out = np.zeros(64)

    def call(n, s, o):
        return lib.plfx_element_fields(eng.h, n, s.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), None)
    assert call(1, sel, out) == -3                                   # PLFX_ERR_STATE before set_mesh
    assert 'set_mesh first' in lib.plfx_last_error(eng.h).decode()
    eng.set_mesh_structured(8, 8, np.ones(8), 1., 1., False, mat_col=np.zeros(8, dtype=np.int32))
    out[:] = 7.
    assert call(0, sel, out) == 0 and np.all(out == 7.)              # nsel = 0: PLFX_OK, nothing written
    for bad in (15, -1, 99):
        assert call(2, np.array([_lib.FIELD_ID['ux'], bad], dtype=np.int32), out) == -2      # PLFX_ERR_ARG
        msg = lib.plfx_last_error(eng.h).decode()
        assert 'unknown field selector %d' % bad in msg and 'sel[1]' in msg
    assert np.all(out == 7.)
    with pytest.raises(_lib.PlfxError):
        eng.element_fields([15])
    assert call(1, sel, out) == 0 and np.all(out == 0.)              # the zero state
    eng.close()


def dist_model(mode):
    """(model, min_step, hand-over level): 17 x 15 with replicated operator; 128 x 32 tension as two strips with halos"""
    if mode == 'replicated':
        return make(255), 2, None
    fe, ms = build_strip('tension', None)
    return fe, ms, 3


def _field_worker(rank, world, port, mode, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import pylabfea_amd as F
        fe, ms, level = dist_model(mode)
        fe.distribute(rank, world, None, host_allreduce=F.host_transport(dist, rank, world), mode=mode, coarse_level=level)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fe.solve(min_step=ms)
        assert (fe._strip is not None) == (mode == 'strip')
        f = fe.fields(ALL)
        q.put((rank, dict(e0=fe._e0, e1=fe._e1, fields=f, ranges={n: fe.field_range(n) for n in ALL})))
    except Exception as exc:  # noqa: BLE001
        import traceback
        q.put((rank, 'ERROR: ' + traceback.format_exc()))
        raise exc
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('mode', ['replicated', 'strip'])
def test_two_ranks_on_one_gpu(mode):
    """bars: 1e-8 of the single-rank field's scale for the owned part, the bar of tests/test_gpu_sharded.py for the state of
    a sharded (or strip) solve against the single-rank one; the rest is exactly zero; the ranges are the same numbers on
    both ranks"""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_field_worker, args=(r, world, port, mode, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, 300.)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    fe, ms, _ = dist_model(mode)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=ms)
    one = fe.fields(ALL)
    scale = {n: max(np.max(np.abs(one[n])), 1e-30) for n in ALL}
    scale.update({n: max(scale[n], 100. * np.max(np.abs(fe._state('eps')))) for n in ALL if 'plastic' in n or 'strain' in n})
    scale.update({n: max(scale[n], np.max(np.abs(fe._state('sig')))) for n in ('stress1', 'stress2', 'stress12')})
    scale.update({n: max(scale[n], np.max(np.abs(fe.u))) for n in ('ux', 'uy')})
    spans = sorted((res[r]['e0'], res[r]['e1']) for r in res)
    assert spans[0][0] == 0 and spans[0][1] == spans[1][0] and spans[1][1] == fe.Nel and spans[0][1] % fe._NY == 0
    for r in range(world):
        e0, e1 = res[r]['e0'], res[r]['e1']
        for n in ALL:
            a = res[r]['fields'][n]
            if n == 'mat':
                assert np.array_equal(a, one[n])       # the host's material map: every element
                continue
            assert np.max(np.abs(a[e0:e1] - one[n][e0:e1])) <= 1e-8 * scale[n], (r, n)
            assert not np.any(a[:e0]) and not np.any(a[e1:]), (r, n)
    for n in ALL:
        assert res[0]['ranges'][n] == res[1]['ranges'][n], n
        lo, hi = fe.field_range(n)
        assert abs(res[0]['ranges'][n][0] - lo) <= 1.02 * 1e-8 * scale[n] and abs(res[0]['ranges'][n][1] - hi) <= 1.02 * 1e-8 * scale[n], n

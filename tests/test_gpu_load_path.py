"""Material.load_path on the GPU: K increments of N material points in one launch, strain- and mixed-controlled.

(1) Strain control has the bits of the host loop -- K response_batch calls with epl += depl in NumPy between them -- at every
    step, for every material kind the path kernels run; a difference is a finding, not a tolerance to widen.
(2) Mixed control reaches its stress targets within stol, leaves the strain-controlled components alone, and its result is
    reproduced bit for bit by a strain-controlled replay of the increments it took, which ties it to (1).
(3) From the definition: uniaxial stress of an elastic material, the r-value of a Hill material.
(4) Paths that end early are results: the completed steps are those of the shorter path, the rest is NaN / -1.
(5) The library's argument checks, launch count and refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import flow_curve_cases as FC
import load_path_cases as LP
import texture_cases as TC
import texture_field_cases as TX
import yield_locus_cases as YC
from pylabfea_amd import _lib
from test_gpu_model import FE

pytestmark = pytest.mark.gpu

SVC_CASES = [(nsv, dev) for nsv in (1, 63, 64, 65, None) for dev in (False, True)]
MATERIALS = (['hill', 'j2k0', 'hill3'] + ['svc_%s_%d' % (nsv or 'all', dev) for nsv, dev in SVC_CASES]
             + ['svc_past_lds', 'bound', 'field', 'barlat'])
ALL_EVENTS = ('elastic', 'plastic', 'ns0', 'nspos', 'reyield')
# what must occur on the yardstick of a material (a cut table need not have a closed locus; without hardening the J2 material
# never sub-divides a step)
EVENTS = dict({k: ALL_EVENTS for k in ('hill', 'hill3', 'svc_all_0', 'svc_all_1', 'svc_past_lds', 'bound', 'field', 'barlat')},
              j2k0=('elastic', 'plastic', 'ns0', 'reyield'))


@pytest.fixture(scope='module')
def tex_case(tmp_path_factory):
    """(parent, field on T = 5 textures, CV, textures) of tests/texture_field_cases.py, on the whole GSH_3 fit"""
    z = TC.load()
    base = TC.facade(FE(), z, tmp_path_factory.mktemp('texture_db'), 'GSH_3')[0]
    tex = TX.field_textures(TC.textures(z, 'GSH_3'), 5)
    m, F, CV, _, _, _ = TX.field_case(FE(), base, TC.tables(z, 'GSH_3'), tex, 91)
    return m, F, CV, tex


@pytest.fixture(scope='module')
def cases(tex_case):
    """name -> (material, CV, tex_id or None, dload (12, 65, 6)), built on first use"""
    made = {}

    def get(name):
        if name in made:
            return made[name]
        tid, zero, seed = None, (), MATERIALS.index(name)
        if name == 'hill':
            m = FC.hill_material(FE())
        elif name == 'j2k0':
            m = LP.j2_material(FE(), khard=0.)
        elif name == 'hill3':
            m = LP.hill3_material(FE())
        elif name == 'barlat':
            m = YC.analytic(FE(), 'abarlat').enable_barlat_normal()
        elif name == 'svc_past_lds':   # 2240 rows: beyond the LDS of a CU, the tables are read from device memory
            m, _ = YC.facade_ml('hill', pad=2240 - 1585)
        elif name.startswith('svc_'):
            nsv, dev = SVC_CASES[MATERIALS.index(name) - 3]
            m, p = FC.svc6_material(nsv=nsv, dev_only=dev)
            if nsv is not None:        # a cut table: an intercept from its own tables, with which it has a locus along most rays
                su = FE().load_cases(0, 20)
                b = YC.crossing_intercept(p, su, np.zeros((20, 6)), [np.full(20, p['sy'])])
                m, _ = FC.svc6_material(nsv=nsv, dev_only=dev, intercept=b)
        else:
            par, F, CV, tex = tex_case
            zero = (3, 4)              # (the texture data sets hold no out-of-plane shear)
            if name == 'bound':
                m = par.at_texture(tex[2])
            else:
                m, tid = F, (np.arange(LP.N_PATH) % len(tex)).astype(np.int32)
        CV = np.array(m.CV) if name not in ('bound', 'field') else tex_case[2]
        made[name] = (m, CV, tid, LP.strain_paths(float(m.sy), float(m.E), seed=seed, zero=zero))
        return made[name]
    return get


# ------------------------------------------------------------------------------------------------ (1) strain control
@pytest.mark.parametrize('maxit', [5, 50])
@pytest.mark.parametrize('name', MATERIALS)
def test_strain_control_has_the_bits_of_the_loop(cases, name, maxit):
    m, CV, tid, dload = cases(name)
    Y = LP.yardstick(m, CV, dload, maxit, tex_id=tid)
    ev = LP.events(Y)
    print(name, maxit, ev)
    if name in EVENTS:
        assert np.all(np.isfinite(Y['sig'])) and np.all(Y['nsteps'] >= 0)
        assert all(ev[k] > 0 for k in EVENTS[name]), ev   # elastic, plastic, nsteps = 0 and > 0, a re-yield after unloading
    ctx = m._load(CV)
    n0 = ctx.load_path_info()['launches']
    P = m.load_path(dload, CV=CV, maxit=maxit, tex_id=tid, return_tangent=True)
    assert ctx.load_path_info()['launches'] == n0 + 1                                # one launch per call
    LP.assert_same_bits('%s maxit %d' % (name, maxit), P, Y)
    assert np.array_equal(P['deps'], dload) and np.all(P['newton'] == 0)
    for N in (1, 31, 33):                                                            # prefixes in N and in K
        for K in (1, 2, 12):
            Q = m.load_path(dload[:K, :N], CV=CV, maxit=maxit, tex_id=None if tid is None else tid[:N], return_tangent=True)
            LP.assert_same_bits('%s maxit %d N %d K %d' % (name, maxit, N, K), Q, Y, K=K, N=N)
    for K in (1, 2):
        Q = m.load_path(dload[:K], CV=CV, maxit=maxit, tex_id=tid)
        LP.assert_same_bits('%s maxit %d N 65 K %d' % (name, maxit, K), Q, Y, K=K, ct=False)


@pytest.mark.parametrize('name', ['hill', 'hill3', 'svc_all_0', 'svc_past_lds', 'field'])
def test_placement_shared_path_and_start_states(cases, name):
    m, CV, tid, dload = cases(name)
    Y = LP.yardstick(m, CV, dload, 50, tex_id=tid)
    perm = np.random.default_rng(8).permutation(LP.N_PATH)
    Q = m.load_path(dload[:, perm], CV=CV, tex_id=None if tid is None else tid[perm], return_tangent=True)
    LP.assert_same_bits(name + ' shuffled', Q, Y, cols=perm)
    # the state in the middle of a path starts the rest of it
    Q = m.load_path(dload[6:], sig0=Y['sig'][5], epl0=Y['epl'][5], CV=CV, tex_id=tid, return_tangent=True)
    for what in LP.NAMES:
        assert np.array_equal(Q[what], Y[what][6:]), (name, what)
    assert np.array_equal(Q['ct'], Y['ct']) and np.all(Q['ksteps'] == 6)
    # one path shared by points in different states: the bits of its expansion, and of the loop
    one = np.ascontiguousarray(dload[:, 7])
    S = m.load_path(one, sig0=Y['sig'][3], epl0=Y['epl'][3], CV=CV, tex_id=tid, return_tangent=True)
    X = m.load_path(np.ascontiguousarray(np.broadcast_to(one[:, None, :], dload.shape)), sig0=Y['sig'][3], epl0=Y['epl'][3],
                    CV=CV, tex_id=tid, return_tangent=True)
    for what in LP.NAMES + ('ct', 'deps', 'ksteps', 'status', 'newton'):
        assert np.array_equal(S[what], X[what]), (name, what)
    Y2 = LP.yardstick(m, CV, np.ascontiguousarray(np.broadcast_to(one[:, None, :], dload.shape)), 50, tex_id=tid,
                      sig0=Y['sig'][3], epl0=Y['epl'][3])
    LP.assert_same_bits(name + ' shared', S, Y2)


def test_rows_of_a_field_against_the_bound_materials(cases, tex_case):
    par, F, CV, tex = tex_case
    _, _, tid, dload = cases('field')
    P = F.load_path(dload, CV=CV, tex_id=tid, return_tangent=True)
    for t in range(len(tex)):
        k = np.nonzero(tid == t)[0]
        B = par.at_texture(tex[t]).load_path(np.ascontiguousarray(dload[:, k]), CV=CV, return_tangent=True)
        for what in LP.NAMES + ('ct',):
            assert np.array_equal(B[what], P[what][:, k] if what != 'ct' else P[what][k]), (t, what)
    r0 = F.load_path(dload[:, :8], CV=CV)                                            # the default row is 0, an int is shared
    b0 = par.at_texture(tex[0]).load_path(dload[:, :8], CV=CV)
    r3 = F.load_path(dload[:, :8], CV=CV, tex_id=3)
    b3 = par.at_texture(tex[3]).load_path(dload[:, :8], CV=CV)
    assert np.array_equal(r0['sig'], b0['sig']) and np.array_equal(r3['sig'], b3['sig'])
    assert not np.array_equal(r0['sig'], r3['sig'])


# ------------------------------------------------------------------------------------------------ (2) mixed control
def golden_hill():
    """the Hill material of tests/golden/material_hill6.npz, the one of the CPU record behind the mixed-control cases"""
    z = np.load(os.path.join(FC.GOLD, 'material_hill6.npz'))
    m = FE().Material(name='Hill-golden')
    m.elasticity(E=float(z['par_E']), nu=float(z['par_nu']))
    m.plasticity(sy=float(z['par_sy']), hill=list(z['par_hill']), khard=float(z['par_khard']), sdim=6)
    assert np.array_equal(np.array(m.CV), z['par_CV'])
    return m, z


@pytest.mark.parametrize('name', ['hill_golden', 'hill', 'svc_all_0'])
def test_mixed_control_reaches_its_targets_and_replays(cases, name):
    m = golden_hill()[0] if name == 'hill_golden' else cases(name)[0]
    CV = np.array(m.CV)
    dload, control = LP.mixed_paths(float(m.sy), float(m.E))
    P = LP.assert_mixed(name, m, CV, dload, control, 1.e-9 * float(m.sy))
    assert np.any(np.any(P['epl'][-1] != 0., axis=1))                                # the paths yield
    # a (6,) mask is the (N, 6) mask of equal rows
    A = m.load_path(dload[:, :1], control=control[0], CV=CV)
    assert np.array_equal(A['sig'], P['sig'][:, :1]) and np.array_equal(A['newton'], P['newton'][:, :1])
    # ... and a shared path takes its mask per point
    d0 = np.ascontiguousarray(dload[:, 0])
    B = m.load_path(d0, control=control[[0, 5]], CV=CV)
    assert np.array_equal(B['sig'][:, 0], P['sig'][:, 0]) and np.array_equal(B['sig'][:, 1], P['sig'][:, 5])


def test_mixed_control_on_a_texture_field(tex_case):
    par, F, CV, tex = tex_case
    d6, c6 = LP.mixed_paths(float(F.sy), float(F.E))
    T = len(tex)
    dload = np.ascontiguousarray(np.tile(d6, (1, T, 1)))
    control = np.tile(c6, (T, 1))
    tid = np.repeat(np.arange(T), len(c6)).astype(np.int32)
    LP.assert_mixed('field', F, CV, dload, control, 1.e-9 * float(F.sy), tex_id=tid)


# ------------------------------------------------------------------------------------------------ (3) from the definition
def test_elastic_uniaxial_stress():
    m = LP.elastic_material(FE())
    E, nu, K = 200.e3, 0.3, 12
    stol = 1.e-9 * 100.
    dload = np.zeros((K, 6))
    dload[:, 0] = 1.e-4
    P = m.load_path(dload, control=[False, True, True, True, True, True], stol=stol, return_tangent=True)
    assert np.all(P['status'] == 0) and np.all(P['ksteps'] == K) and P['newton'].max() <= 1
    eps = np.cumsum(P['deps'][:, 0], axis=0)
    assert np.array_equal(P['deps'][:, 0, 0], dload[:, 0])
    print('elastic: sig_xx / (E eps_xx) - 1 = %.3e, lateral / (-nu eps_xx) - 1 = %.3e, other stresses %.3e' % (
        np.max(np.abs(P['sig'][:, 0, 0] / (E * eps[:, 0]) - 1.)), np.max(np.abs(eps[:, 1:3] / (-nu * eps[:, :1]) - 1.)),
        np.max(np.abs(P['sig'][:, 0, 1:]))))
    assert np.all(np.abs(P['sig'][:, 0, 0] - E * eps[:, 0]) <= 1.e-12 * E * eps[:, 0])
    assert np.all(np.abs(eps[:, 1:3] + nu * eps[:, :1]) <= 1.e-12 * nu * eps[:, :1])
    assert np.all(np.abs(P['sig'][:, 0, 1:]) <= stol) and np.all(eps[:, 3:] == 0.) and np.all(P['epl'] == 0.)
    assert np.array_equal(P['ct'][0], np.array(m.CV))


def test_hill_r_value_against_the_oracle_iteration():
    m, z = golden_hill()
    CV, stol = np.array(m.CV), 1.e-9 * float(m.sy)
    dload, control = LP.mixed_paths(float(m.sy), float(m.E))
    d, c = np.ascontiguousarray(dload[:, 0]), control[0]                             # eps_xx driven, the others stress-free
    want = float(m.hill[0] / m.hill[2])
    ref = LP.oracle_load_path(LP.oracle_material(m), CV, d, c, stol)
    assert ref['status'] == 0
    q_ref, k_ref = LP.r_ratio(ref['depl'])
    dev_ref = float(np.max(np.abs(q_ref / want - 1.)))
    P = m.load_path(d, control=c, CV=CV)
    assert P['status'][0] == 0
    depl = np.diff(np.concatenate((np.zeros((1, 6)), P['epl'][:, 0]), axis=0), axis=0)
    q, k0 = LP.r_ratio(depl)
    dev = float(np.max(np.abs(q / want - 1.)))
    print('r-value: depl_yy / depl_zz = %.12f wanted, from step %d; deviation of the oracle iteration %.3e, bar %.3e, device %.3e'
          % (want, k0, dev_ref, 4. * dev_ref, dev))
    assert k0 == k_ref and len(q) >= 10
    assert dev <= 4. * dev_ref


# ------------------------------------------------------------------------------------------------ (4) paths that end early
def test_a_path_that_cannot_go_on_ends_with_a_status():
    m = LP.j2_material(FE(), khard=0.)
    sy, K = float(m.sy), 12
    dload = np.zeros((K, 2, 6))
    dload[:, 0, 0] = 0.12 * sy             # all six stress-controlled: 0.96 sy after eight steps, beyond the locus at the ninth
    dload[:, 1, 0] = 0.05 * sy             # the neighbour stays elastic
    control = np.ones((2, 6), dtype=bool)
    P = m.load_path(dload, control=control, return_tangent=True)
    print('status', P['status'], 'ksteps', P['ksteps'], 'corrections', P['newton'][:, 0])
    assert P['ksteps'][0] == 8 and P['status'][0] in (1, 2, 3)
    assert P['ksteps'][1] == K and P['status'][1] == 0
    Q = m.load_path(dload[:8], control=control, return_tangent=True)
    assert np.all(Q['status'] == 0) and np.all(Q['ksteps'] == 8)
    for what in ('sig', 'epl', 'deps', 'fy', 'nsteps', 'newton'):
        assert np.array_equal(P[what][:8, 0], Q[what][:8, 0]), what
    assert np.array_equal(P['ct'][0], Q['ct'][0])
    for what in ('sig', 'epl', 'deps', 'fy'):
        assert np.all(np.isnan(P[what][8:, 0])), what
    assert np.all(P['nsteps'][8:, 0] == -1) and np.all(P['newton'][8:, 0] == -1)
    alone = m.load_path(np.ascontiguousarray(dload[:, 1:]), control=control[1:], return_tangent=True)
    for what in ('sig', 'epl', 'deps', 'fy', 'nsteps', 'newton', 'ct'):                # the neighbour is unaffected
        assert np.array_equal(P[what][:, 1] if what != 'ct' else P[what][1], alone[what][:, 0] if what != 'ct' else alone[what][0])
    assert np.all(np.abs(P['sig'][:, 1, 0] - np.cumsum(dload[:, 1, 0])) <= 1.e-9 * sy)


# ------------------------------------------------------------------------------------------------ (5) library
def hill_record(z):
    return _lib.pack_material(_lib.HILL6, z['rpe_CV'], E=float(z['par_E']), nu=float(z['par_nu']), sy=float(z['par_sy']),
                              khard=float(z['par_khard']), hill=z['par_hill'], drucker=float(z['par_dp'][0]))


def test_library_argument_checks_and_launch_count():
    z = np.load(os.path.join(FC.GOLD, 'material_hill6.npz'))
    ctx = _lib.Context(0)
    d = np.zeros((3, 2, 6))
    d[:, :, 0] = 1.e-4
    with pytest.raises(_lib.PlfxError, match='error -3'):                            # before set_materials
        ctx.load_path(0, d)
    tresca = _lib.pack_material(_lib.TRESCA, z['rpe_CV'], E=float(z['par_E']), nu=float(z['par_nu']), sy=100.)
    ctx.set_materials([hill_record(z), tresca])
    assert ctx.load_path_info() == dict(launches=0)
    with pytest.raises(_lib.PlfxError, match='error -4'):                            # an unsupported kind
        ctx.load_path(1, d)
    nan, big = d.copy(), d.copy()
    nan[1, 1, 4] = np.nan
    big[2, 0, 3] = 0.06
    bad = [dict(mat=-1), dict(mat=2), dict(maxit=0), dict(newton=-1), dict(stol=0.), dict(stol=np.inf), dict(stol=np.nan),
           dict(eps_cap=0.), dict(eps_cap=-1.), dict(eps_cap=np.inf), dict(dload=nan), dict(dload=big),
           dict(sig0=np.full((2, 6), np.inf)), dict(epl0=np.full((2, 6), np.nan)), dict(control=[64, 0]), dict(control=[0, -1])]
    for kw in bad:
        kw = dict(dict(mat=0, dload=d), **kw)
        with pytest.raises(_lib.PlfxError, match='error -2'):
            ctx.load_path(kw.pop('mat'), kw.pop('dload'), **kw)
    # a component beyond eps_cap is an argument error only where it is a strain
    ok = ctx.load_path(0, big, control=[8, 8])
    assert np.all(ok['ksteps'] >= 0)
    n0 = ctx.load_path_info()['launches']
    assert n0 == 1
    lib = ctx.lib                                                                     # n < 0, K < 0 (no array has such a shape)
    for n, K in ((-1, 3), (2, -1)):
        assert lib.plfx_load_path(ctx.h, 0, n, K, None, 0, None, None, None, None, 50, 30, C.c_double(1.), C.c_double(0.05),
                                  *([None] * 9)) == -2
    e = ctx.load_path(0, np.zeros((0, 2, 6)), return_tangent=True)                    # K = 0, n = 0: no launch
    assert e['sig'].shape == (0, 2, 6) and np.all(e['ksteps'] == 0) and np.all(e['status'] == 0)
    assert np.array_equal(e['ct'][1], z['rpe_CV'].reshape(6, 6))
    e = ctx.load_path(0, np.zeros((3, 0, 6)))
    assert e['sig'].shape == (3, 0, 6) and ctx.load_path_info()['launches'] == n0
    a = ctx.load_path(0, d, return_tangent=True)
    assert ctx.load_path_info()['launches'] == n0 + 1                                # exactly one launch per call
    ctx.set_materials([tresca, hill_record(z)])                                      # other materials between two calls
    with pytest.raises(_lib.PlfxError, match='error -4'):
        ctx.load_path(0, d)
    b = ctx.load_path(1, d, return_tangent=True)
    assert all(np.array_equal(a[k], b[k]) for k in a) and ctx.load_path_info()['launches'] == n0 + 2
    ctx.close()


def test_library_texture_rows_are_checked(tex_case):
    par, F, CV, tex = tex_case
    ctx = F._load(CV)
    d = np.zeros((2, 3, 6))
    n0 = ctx.load_path_info()['launches']
    for tid in ([0, 5, 0], [0, 0, -1]):
        with pytest.raises(_lib.PlfxError, match='error -2'):
            ctx.load_path(0, d, tex_id=tid)
    assert ctx.load_path_info()['launches'] == n0

"""Plane columns.  Every model of this library is a plane model: columns 3 and 4 (the yz / zx shears) of sig,
epl, res_sig and res_depl are zero, and elastic and analytic Hill / J2 materials whose CV does not couple those shears to the
rest keep them zero.  While that holds, the Hill sweep (k_sweep_light_plane) and the state update (k_update_state_plane) neither
load nor store these columns, nor rows 4 and 5 of the tangent factors.  None of that may be seen in a result: every case runs
with PLFX_PLANE_COLS=1 and =0 (the launches as they were) and compares u, f, du, sig, eps, epl, sgl, egl, epgl, niter, the PCG
iterations per solve, res_sig, res_depl, fyn, max_steps and the expanded tangents with np.array_equal (which takes the one
admitted difference, -0.0 for +0.0 in columns 3 and 4 of res_depl, as equal).  The engine reads the variable when it is created
and every Model creates its own, so both runs share a process, as in tests/test_gpu_dead_stores.py, whose models, meshes and
reference-solver run these cases reuse.  plfx_plane_info's counters say which kernels ran.

The premise is asserted on the =0 run of every case: columns 3 and 4 of the four arrays are all zero, and the tangent entries
that couple components 3, 4 to the others (and to each other) are those of the element's CV.

Shapes: the mixed model (Hill | elastic | softer Hill: the elastic branch of the update runs, no exchange) at 15 x 15, 25 x 25
and 40 x 29, partial tiles throughout, the last also against the CPU reference solver at that file's 1e-6; the same with
PLFX_SWEEP_BLOCKS 1 (625 elements), 2 and 3 (1160), where a thread takes several tiles and the carried prefetch registers are
consumed with real data and a partial last tile; the all-plastic 25 x 25 model (load steps end by exchanging sig and res_sig)
with state reads between the load steps and stopped and resumed; the bench tension model at 128 x 128 and 160 x 104 (above the
16 384-node gate of the interpolated start, partial blocks), where the armed first sweep of a step rewrites tangents through the
five-row factor store; and the same with the soft inclusion, where the corrector list is not empty and load steps end at the
iteration limit, so that averaged full-form tangents are written and then met as old tangents by plane-form new ones."""
import os
import warnings

import numpy as np
import pytest

from test_gpu_dead_stores import EPS, arrays as base_arrays, inclusion, mixed_ref, solved
from test_gpu_end_of_step import plastic_model
from test_gpu_pred_start import tension
from test_gpu_sweep_prefetch import close, mixed_model

pytestmark = pytest.mark.gpu

KEYS = ('u', 'f', 'du', 'sig', 'eps', 'epl', 'sgl', 'egl', 'epgl', 'niter', 'its', 'res_sig', 'res_depl', 'fyn', 'max_steps',
        'elstiff')
ON, NEVER, SWITCH, SHARDED, MATERIALS, STATE_SET, TANGENT_SET = range(7)    # PLFX_PLANE_* of include/plfx.h


def arrays(fe):
    out = base_arrays(fe)
    eng = fe._ensure_engine()
    out.update(max_steps=fe._state('max_steps').copy(), elstiff=fe._state('elstiff').copy(), plane=eng.plane_info())
    return out


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def assert_premise(b, fe):
    """on the run with the launches as they were: the columns the plane kernels leave out hold zeros, the tangent rows CV's"""
    for k in ('sig', 'epl', 'res_sig', 'res_depl'):
        assert np.all(b[k].reshape(-1, 6)[:, 3:5] == 0.), k
    D = b['elstiff'].reshape(-1, 6, 6)
    cv = np.stack([fe._element_CV(m) for m in fe.mat])[np.asarray(fe._mat_id)]
    assert np.array_equal(D[:, 3:5, :], cv[:, 3:5, :]) and np.array_equal(D[:, :, 3:5], cv[:, :, 3:5])


def on_off(monkeypatch, make, min_step, steps=None, **env):
    """the model of make() solved with the switch on and off: (arrays on, arrays off, model on)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    runs = []
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_PLANE_COLS', switch)
        fe = solved(make(), min_step, steps)
        runs.append((arrays(fe), fe))
    (a, fe), (b, _) = runs
    assert_premise(b, fe)
    assert_same(a, b)
    on, sweeps, updates, why = a['plane']
    assert on and why == ON and sweeps == a['sweeps'][0] and updates >= int(a['nsteps'])
    assert b['plane'] == (False, 0, 0, SWITCH)
    assert np.array_equal(a['sweeps'], b['sweeps']) and np.array_equal(a['dead'], b['dead'])
    return a, b, fe


def mixed_case(monkeypatch, nx, ny, ref=False, **env):
    a, b, fe = on_off(monkeypatch, lambda: mixed_model(nx, ny, EPS), 2, **env)
    print('%d x %d %s: plane_info on %s off %s, sweeps / tangents rewritten %s, load steps %d, niter %s'
          % (nx, ny, env, a['plane'], b['plane'], tuple(a['sweeps']), int(a['nsteps']), list(a['niter'])))
    assert fe.Nel % 256 != 0 and np.max(a['niter']) >= 2 and np.max(np.abs(a['epl'])) > 0.
    mat = np.asarray(fe._mat_id)
    assert np.sum(mat == 1) > 0 and np.any(a['sig'][mat == 1] != 0.)    # the elastic section: the other branch of the update
    assert not np.array_equal(a['res_sig'], a['sig'])                    # no exchange
    assert np.sum(a['max_steps'].ravel() >= 49) > 0                      # the corrector (six-column stores) ran beside the plane stores
    if ref:
        r = mixed_ref(nx, ny)
        assert int(a['nsteps']) == r.nsteps and list(a['niter']) == list(r.niter)
        assert close(a['u'], r.u) and close(a['sig'], r.sig) and close(a['eps'], r.eps)
        assert close(a['epl'], r.epl, scale=np.max(np.abs(r.eps)))
        assert close(a['sgl'], r.sgl) and close(a['egl'], r.egl)


@pytest.mark.parametrize('nx,ny,ref', [(15, 15, False), (25, 25, False), (40, 29, True)])
def test_mixed_model_edge_tiles(monkeypatch, nx, ny, ref):
    mixed_case(monkeypatch, nx, ny, ref)


@pytest.mark.parametrize('blocks,nx,ny', [(1, 25, 25), (2, 40, 29), (3, 40, 29)])
def test_mixed_model_several_tiles_per_thread(monkeypatch, blocks, nx, ny):
    assert (nx * ny + 255) // 256 > blocks and (nx * ny) % 256 != 0     # a thread takes a second pass; the last tile is partial
    mixed_case(monkeypatch, nx, ny, PLFX_SWEEP_BLOCKS=str(blocks))


def test_all_plastic_exchange_with_reads_between_load_steps(monkeypatch):
    seen = {}

    def make(switch):
        fe = plastic_model()

        def hook(il):
            fe._cache = {}
            seen.setdefault(switch, []).append({k: fe._state(k).copy() for k in ('sig', 'eps', 'epl', 'res_sig', 'res_depl', 'fyn', 'elstiff')})
            fe._cache = {}
        fe._step_hook = hook
        return fe
    runs = {}
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_PLANE_COLS', switch)
        fe = solved(make(switch), 2)
        runs[switch] = arrays(fe)
    a, b = runs['1'], runs['0']
    print('all-plastic 25 x 25: plane_info on %s off %s, load steps %d, niter %s' % (a['plane'], b['plane'], int(a['nsteps']), list(a['niter'])))
    assert_premise(b, fe)
    assert_same(a, b)
    assert a['plane'][0] and a['plane'][1] == a['sweeps'][0] and a['plane'][2] >= int(a['nsteps']) and a['plane'][3] == ON
    assert b['plane'] == (False, 0, 0, SWITCH)
    assert np.max(a['niter']) >= 2
    assert np.array_equal(a['res_sig'], a['sig']) and np.any(a['sig'] != 0.)     # the exchanged buffer is the stress
    assert len(seen['1']) == len(seen['0']) == int(a['nsteps']) >= 2
    for s1, s0 in zip(seen['1'], seen['0']):
        for k in s1:
            assert np.array_equal(s1[k], s0[k]), k
    assert not np.array_equal(seen['1'][0]['sig'], seen['1'][-1]['sig'])


def test_all_plastic_stopped_and_resumed(monkeypatch):
    N, STOP = 40, 12
    runs = []
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_PLANE_COLS', switch)
        fe = solved(plastic_model(), N, STOP)
        assert fe.nsteps == STOP
        mid = arrays(fe)
        first = list(fe.niter)
        solved(fe, N - STOP)
        runs.append((mid, arrays(fe), first + list(fe.niter)))
    (mid_a, a, nit_a), (mid_b, b, nit_b) = runs
    print('stopped after %d load steps and resumed: plane_info on %s, niter %s' % (STOP, a['plane'], nit_a))
    assert nit_a == nit_b and a['plane'][0] and a['plane'][3] == ON and b['plane'] == (False, 0, 0, SWITCH)
    assert_premise(mid_b, fe)
    assert_premise(b, fe)
    assert_same(mid_a, mid_b)
    assert_same(a, b)
    assert not np.array_equal(mid_a['sig'], a['sig'])


def bench_case(monkeypatch, make, steps):
    a, b, fe = on_off(monkeypatch, make, 50, steps)
    print('%d elements: plane_info on %s, dead_store_info %s, sweeps / tangents rewritten %s, niter %s, PCG iterations %s'
          % (fe.Nel, a['plane'], tuple(a['dead']), tuple(a['sweeps']), list(a['niter']), list(a['its'])))
    assert fe.Nnode >= 16384 and fe.Nnode % 256 != 0
    assert int(a['nsteps']) == steps and np.max(np.abs(a['epl'])) > 0.
    assert a['dead'][0] > 0 and a['dead'][1] > 0        # armed sweeps rewrote tangents: the five-row factor store
    return a, fe


@pytest.mark.parametrize('nx,ny', [(128, 128), (160, 104)])
def test_bench_tension_model(monkeypatch, nx, ny):
    a, fe = bench_case(monkeypatch, lambda: tension(nx, ny), 8)
    assert a['dead'][1] >= fe.Nel                        # a sweep that rewrote every tangent
    assert a['dead'][2] > 0                              # the interpolated / test-only starts ran as they do in the headline


@pytest.mark.parametrize('nx,ny', [(128, 128), (160, 104)])
def test_bench_tension_model_with_soft_inclusion(monkeypatch, nx, ny):
    a, fe = bench_case(monkeypatch, lambda: inclusion(nx, ny), 12)
    assert np.sum(a['max_steps'].ravel() >= 49) > 0     # the corrector list was not empty
    at_limit = int(np.sum(a['niter'] == 15))
    assert at_limit >= 2 and a['niter'][-1] == 15       # averaged full-form tangents written, and met again as old tangents


def test_state_set_with_a_shear_leaves_the_mode(monkeypatch):
    """sig with a non-zero column 3 from outside, between two parts of a solve: the mode reports off with the reason, the full
    kernels run from there on (the column is carried into the result), and the results are those of the switched-off run array
    for array"""
    from pylabfea_amd import _lib
    N, STOP = 40, 12
    runs = []
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_PLANE_COLS', switch)
        fe = solved(plastic_model(), N, STOP)
        eng = fe._ensure_engine()
        before = eng.plane_info()
        s = eng.state_get(_lib.ST_SIG)
        assert np.all(s[:, 3] == 0.)
        s[:, 3] = 1. + 0.01 * np.arange(fe.Nel)
        eng.state_set(_lib.ST_SIG, s)
        after = eng.plane_info()
        solved(fe, N - STOP, 8)                          # (eight more load steps: the stress set from outside makes them long)
        runs.append((arrays(fe), before, after))
    (a, before_a, after_a), (b, before_b, after_b) = runs
    print('state_set of sig with a shear: plane_info before %s after %s at the end %s' % (before_a, after_a, a['plane']))
    assert before_a[0] and before_a[1] > 0 and before_a[2] >= STOP and before_a[3] == ON
    assert after_a == (False, before_a[1], before_a[2], STATE_SET) and a['plane'] == after_a     # no plane launch after it
    assert before_b == after_b == b['plane'] == (False, 0, 0, SWITCH)
    assert_same(a, b)
    assert a['sweeps'][0] > before_a[1] and np.array_equal(a['sweeps'], b['sweeps'])
    assert np.all(a['sig'][:, 3] != 0.) and np.max(np.abs(a['epl'])) > 0.


def test_state_set_with_zero_columns_keeps_the_mode(monkeypatch):
    """the four arrays set from outside with columns 3 and 4 zero (a negative zero is a zero): the mode stays on"""
    from pylabfea_amd import _lib
    N, STOP = 40, 12
    runs = []
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_PLANE_COLS', switch)
        fe = solved(plastic_model(), N, STOP)
        eng = fe._ensure_engine()
        before = eng.plane_info()
        for which in (_lib.ST_SIG, _lib.ST_EPL, _lib.ST_RES_SIG, _lib.ST_RES_DEPL):
            s = eng.state_get(which)
            s[:, [0, 1, 5]] *= 0.999
            s[::2, 3] = -0.
            eng.state_set(which, s)
        assert eng.plane_info() == before
        solved(fe, N - STOP)
        runs.append((arrays(fe), before))
    (a, before_a), (b, _) = runs
    print('state_set with zero columns: plane_info before %s at the end %s' % (before_a, a['plane']))
    assert a['plane'][0] and a['plane'][3] == ON and a['plane'][1] > before_a[1] and a['plane'][2] > before_a[2]
    assert a['plane'][1] == a['sweeps'][0]
    assert_premise(b, fe)
    assert_same(a, b)


def test_set_tangents_leaves_the_mode(monkeypatch):
    from pylabfea_amd import _lib
    monkeypatch.setenv('PLFX_PLANE_COLS', '1')
    fe = plastic_model()
    eng = fe._ensure_engine()
    eng.state_set(_lib.ST_ELSTIFF, eng.state_get(_lib.ST_ELSTIFF))
    assert eng.plane_info() == (False, 0, 0, TANGENT_SET)
    eng.state_reset()
    assert eng.plane_info() == (True, 0, 0, ON)          # a reset starts a new history


def test_material_that_couples_the_shears(monkeypatch):
    """elasticity(CV=...) with a non-zero (0, 3) entry: off at set_materials, the full kernels run, same results as switched off"""
    import pylabfea_amd as FE

    def make():
        m = FE.Material(num=1)
        E, nu = 200.e3, 0.3
        hh = E / ((1. + nu) * (1. - 2. * nu))
        CV = np.zeros((6, 6))
        CV[:3, :3] = nu * hh
        CV[np.arange(3), np.arange(3)] = (1. - nu) * hh
        CV[np.arange(3, 6), np.arange(3, 6)] = (0.5 - nu) * hh
        CV[0, 3] = CV[3, 0] = 0.02 * hh
        m.elasticity(CV=CV)
        m.plasticity(sy=100., hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=100., sdim=6)
        fe = FE.Model(dim=2, planestress=False)
        fe.geom([2.], LY=2.)
        fe.assign([m])
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(0.004 * fe.leny, 'disp')
        fe.mesh(NX=15, NY=15)
        return fe
    runs = []
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_PLANE_COLS', switch)
        fe = make()
        first = fe._ensure_engine().plane_info()
        runs.append((arrays(solved(fe, 2)), first))
    (a, first_a), (b, first_b) = runs
    print('coupled CV: plane_info %s, max |sig[:, 3]| %.3g' % (a['plane'], np.max(np.abs(a['sig'][:, 3]))))
    assert first_a == a['plane'] == (False, 0, 0, MATERIALS) and first_b == b['plane'] == (False, 0, 0, SWITCH)
    assert_same(a, b)
    assert np.any(a['sig'][:, 3] != 0.) and np.max(np.abs(a['epl'])) > 0.     # the premise does not hold for this material


def test_svc_material_in_the_table(monkeypatch, golden_dir):
    """an SVC material in the table, used or not, ends the mode at set_materials; it stays off when the table is Hill again"""
    from pylabfea_amd import _lib
    monkeypatch.setenv('PLFX_PLANE_COLS', '1')
    fe = plastic_model()
    eng = fe._ensure_engine()
    assert eng.plane_info() == (True, 0, 0, ON)
    hill = [m._record(fe._element_CV(m)) for m in fe._eng_uniq]
    z = np.load(os.path.join(golden_dir, 'svc_hill.npz'))
    svc = dict(sv=z['par_sv'], dual=z['par_dual'], gamma=float(z['par_gamma']), intercept=float(z['par_intercept']),
               scale_seq=float(z['par_scale_seq']), dev_only=bool(z['par_dev_only']))
    rec = _lib.pack_material(_lib.SVC6, z['rpe_CV'], E=float(z['par_E']), nu=float(z['par_nu']), sy=float(z['par_sy']),
                             khard=float(z['par_khard']), hill=z['par_hill'], svc=svc)
    eng.set_materials(hill + [rec])
    assert eng.plane_info() == (False, 0, 0, MATERIALS)
    eng.set_materials(hill)
    assert eng.plane_info() == (False, 0, 0, MATERIALS)  # never back on in mid-life
    eng.state_reset()
    assert eng.plane_info() == (True, 0, 0, ON)


def test_reuse_off_switches_it_off(monkeypatch):
    monkeypatch.setenv('PLFX_REUSE', '0')
    monkeypatch.setenv('PLFX_PLANE_COLS', '1')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe = solved(plastic_model(), 2)
    assert np.max(np.abs(fe._state('epl'))) > 0.
    assert fe._ensure_engine().plane_info() == (False, 0, 0, SWITCH)

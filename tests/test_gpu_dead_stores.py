"""Stores that nothing reads are left out.  A.  Inside a load step a sweep that changes a tangent is always
followed by another sweep, which rewrites res_sig, res_depl and fyn of every plastic element: the streaming sweep kernel of
such a sweep does not store the three fields of the elements whose tangent it rewrites.  B.  A predictor solve whose first
tolerance test is expected to pass starts with the sums of that test alone (k_cg_start_test: no r, no z, no r.z); if the test
fails, the full start follows.  None of that may be seen in a result: every case runs with PLFX_DEAD_STORES=1 and =0 (the
launches as they were) and compares u, f, du, sig, eps, epl, sgl, egl, epgl, niter, the PCG iterations per solve, and res_sig,
res_depl and fyn read after the solve, bit for bit.  The engine reads the variable when it is created, and every Model creates
its own, so both runs share a process.  plfx_dead_store_info's counters say which path ran.

Shapes.  The mixed model (Hill | elastic | softer Hill) of tests/test_gpu_sweep_prefetch.py at 15 x 15, 25 x 25 and 40 x 29
elements and eps 0.01: partial tiles, elastic elements the sweep never writes, and elements on the 50-sub-step corrector (which
always stores) beside elements with predicated stores in one wave; these runs are also held to the CPU reference solver at that
file's 1e-6 (computed once per mesh, shared with the next group).  The same model with PLFX_SWEEP_BLOCKS (1 block over 625
elements, 2 and 3 over 1160): a thread takes several tiles, so the carried prefetch registers meet left-out and kept stores in
successive passes.  The all-plastic 25 x 25 model of tests/test_gpu_end_of_step.py ends its load steps by exchanging sig and
res_sig: the buffer the earlier sweeps of the step wrote in part becomes the stress; it runs with state reads between the load
steps, and stopped after 12 of 40 load steps and resumed.  The bench tension model at 128 x 128 and 160 x 104 (the smallest
meshes above the 16 384-node gate of the waited first test, neither node count a multiple of the block) reaches the test-only
start; with the soft inclusion of tests/test_gpu_pred_start.py the predictor's plain start fails and the full start follows.

How many retries the hint predicts: the test-only start is launched exactly where the host then waits for the first test, and
plfx_bc_info's du_early counts the waits that found the test passed -- every other one is a retry.

A step that ends at the iteration limit: load steps 11 and 12 of the inclusion runs (niter 15 on both meshes, i.e. sixteen
sweeps).  Their last sweep (nit = 15) is the one sweep of a load step that is not armed, and it changes tangents; res_sig,
res_depl and fyn compared after load step 12 are what that sweep stored."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

from test_gpu_end_of_step import plastic_model
from test_gpu_pred_start import tension
from test_gpu_sweep_prefetch import RTOL, close, mixed_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('u', 'f', 'du', 'sig', 'eps', 'epl', 'sgl', 'egl', 'epgl', 'niter', 'its', 'res_sig', 'res_depl', 'fyn')
EPS = 0.01


def solved(fe, min_step, steps=None):
    fe._max_load_steps = steps
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=min_step)
    return fe


def arrays(fe):
    from pylabfea_amd import _lib
    eng = fe._ensure_engine()
    fe._cache = {}
    out = {k: fe._state(k).copy() for k in ('sig', 'eps', 'epl', 'res_sig', 'res_depl', 'fyn')}
    out.update(u=np.array(fe.u), f=np.array(fe.f), du=eng.state_get(_lib.ST_DU), sgl=np.asarray(fe.sgl), egl=np.asarray(fe.egl),
               epgl=np.asarray(fe.epgl), niter=np.asarray(fe.niter), its=np.array([q[0] for q in fe.solver_stats]),
               nsteps=np.array(fe.nsteps), dead=np.array(eng.dead_store_info()), bc=np.array(eng.bc_info()),
               sweeps=np.array(eng.sweep_info()))
    return out


def on_off(monkeypatch, make, min_step, steps=None, **env):
    """the model of make() solved with the switch on and off: (arrays on, arrays off, model on)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    runs = []
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_DEAD_STORES', switch)
        fe = solved(make(), min_step, steps)
        runs.append((arrays(fe), fe))
    return runs[0][0], runs[1][0], runs[0][1]


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@functools.lru_cache(maxsize=None)
def mixed_ref(nx, ny):
    """the CPU reference solver's run of the mixed model, once per mesh; read only"""
    from oracle.solve_ref import RefSolver
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return RefSolver(mixed_model(nx, ny, EPS)).solve(min_step=2)


def mixed_case(monkeypatch, nx, ny, **env):
    a, b, fe = on_off(monkeypatch, lambda: mixed_model(nx, ny, EPS), 2, **env)
    armed, rewritten, starts, retries = a['dead']
    print('%d x %d %s: dead_store_info on %s off %s, sweeps / tangents rewritten %s, load steps %d, niter %s'
          % (nx, ny, env, tuple(a['dead']), tuple(b['dead']), tuple(a['sweeps']), int(a['nsteps']), list(a['niter'])))
    assert fe.Nel % 256 != 0 and np.max(a['niter']) >= 2 and np.max(np.abs(a['epl'])) > 0.
    assert_same(a, b)
    assert tuple(b['dead']) == (0, 0, 0, 0)
    assert armed > 0 and rewritten > 0
    assert armed == a['sweeps'][0] and np.max(a['niter']) < 15      # no load step reaches the iteration limit: every sweep is armed
    assert starts == 0                                 # below the 16 384-node gate of the waited first test
    assert np.array_equal(a['sweeps'], b['sweeps'])
    mat = np.asarray(fe._mat_id)
    assert np.sum(mat == 1) > 0 and not np.any(a['fyn'][mat == 1])    # the elastic section, which no sweep stores a response for
    assert np.sum(fe._state('max_steps').ravel() >= 49) > 0           # the corrector ran beside the predicated stores
    ref = mixed_ref(nx, ny)
    assert int(a['nsteps']) == ref.nsteps and list(a['niter']) == list(ref.niter)
    assert close(a['u'], ref.u) and close(a['sig'], ref.sig) and close(a['eps'], ref.eps)
    assert close(a['epl'], ref.epl, scale=np.max(np.abs(ref.eps)))
    assert close(a['sgl'], ref.sgl) and close(a['egl'], ref.egl)


@pytest.mark.parametrize('nx,ny', [(15, 15), (25, 25), (40, 29)])
def test_mixed_model_edge_tiles(monkeypatch, nx, ny):
    mixed_case(monkeypatch, nx, ny)


@pytest.mark.parametrize('blocks,nx,ny', [(1, 25, 25), (2, 40, 29), (3, 40, 29)])
def test_mixed_model_several_tiles_per_thread(monkeypatch, blocks, nx, ny):
    assert (nx * ny + 255) // 256 > blocks      # more tiles than blocks: a thread takes a second pass
    mixed_case(monkeypatch, nx, ny, PLFX_SWEEP_BLOCKS=str(blocks))


def test_all_plastic_exchange_with_reads_between_load_steps(monkeypatch):
    seen = {}

    def make(switch):
        fe = plastic_model()

        def hook(il):
            fe._cache = {}
            seen.setdefault(switch, []).append({k: fe._state(k).copy() for k in ('sig', 'eps', 'res_sig', 'res_depl', 'fyn')})
            fe._cache = {}
        fe._step_hook = hook
        return fe
    runs = {}
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_DEAD_STORES', switch)
        runs[switch] = arrays(solved(make(switch), 2))
    a, b = runs['1'], runs['0']
    print('all-plastic 25 x 25: dead_store_info on %s, load steps %d, niter %s' % (tuple(a['dead']), int(a['nsteps']), list(a['niter'])))
    assert_same(a, b)
    assert a['dead'][0] > 0 and a['dead'][1] > 0 and tuple(b['dead']) == (0, 0, 0, 0)
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
        monkeypatch.setenv('PLFX_DEAD_STORES', switch)
        fe = solved(plastic_model(), N, STOP)
        assert fe.nsteps == STOP
        mid = arrays(fe)
        first = list(fe.niter)
        solved(fe, N - STOP)
        runs.append((mid, arrays(fe), first + list(fe.niter)))
    (mid_a, a, nit_a), (mid_b, b, nit_b) = runs
    print('stopped after %d load steps and resumed: dead_store_info on %s, niter %s' % (STOP, tuple(a['dead']), nit_a))
    assert nit_a == nit_b and a['dead'][0] > 0 and tuple(b['dead']) == (0, 0, 0, 0)
    assert_same(mid_a, mid_b)
    assert_same(a, b)
    assert not np.array_equal(mid_a['sig'], a['sig'])


def start_case(monkeypatch, make, steps):
    a, b, fe = on_off(monkeypatch, make, 50, steps)
    armed, rewritten, starts, retries = a['dead']
    print('%d elements: dead_store_info on %s, bc_info on %s off %s, niter %s, PCG iterations %s'
          % (fe.Nel, tuple(a['dead']), tuple(a['bc']), tuple(b['bc']), list(a['niter']), list(a['its'])))
    assert fe.Nnode >= 16384 and fe.Nnode % 256 != 0
    assert int(a['nsteps']) == steps and np.max(np.abs(a['epl'])) > 0.
    assert_same(a, b)
    assert tuple(b['dead']) == (0, 0, 0, 0) and np.array_equal(a['bc'], b['bc'])
    assert starts > 0 and armed > 0
    assert retries == starts - a['bc'][3]       # the waits for the first test that did not find it passed (module docstring)
    return a


@pytest.mark.parametrize('nx,ny', [(128, 128), (160, 104)])
def test_bench_tension_model_test_only_start(monkeypatch, nx, ny):
    a = start_case(monkeypatch, lambda: tension(nx, ny), 8)
    assert a['dead'][2] > a['dead'][3]          # most predictor solves are answered by their first test


def inclusion(nx, ny):
    """tests/test_gpu_pred_start.py's model with the soft inclusion (its child script, as a function)"""
    import pylabfea_amd as FE
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    soft = FE.Material(name='soft inclusion', num=2)
    soft.elasticity(E=1.e3, nu=0.27)
    fe = FE.Model(dim=2, planestress=False)
    fe.geom(sect=2, LX=4., LY=4.)
    fe.assign([bench.hill_material(FE), soft])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.005 * fe.leny, 'disp')
    el = np.ones((nx, ny))
    el[nx // 3:2 * (nx // 3), ny // 3:2 * (ny // 3)] = 2
    fe.mesh(elmts=el, NX=nx, NY=ny)
    return fe


@pytest.mark.parametrize('nx,ny', [(128, 128), (160, 104)])
def test_inclusion_full_start_follows_a_failed_test(monkeypatch, nx, ny):
    a = start_case(monkeypatch, lambda: inclusion(nx, ny), 12)
    assert a['dead'][3] > 0
    # the iteration limit: the sweep with nit = 15 is not armed, and the tangents it rewrites are counted outside the armed ones
    at_limit = int(np.sum(a['niter'] == 15))
    assert at_limit >= 1 and a['niter'][-1] == 15
    assert a['sweeps'][0] - a['dead'][0] == at_limit
    assert a['sweeps'][1] > a['dead'][1]


def test_direct_sweep_stores_every_element(monkeypatch):
    """plfx_sweep from Python, outside a load step: never armed, whatever changes"""
    from pylabfea_amd import _lib
    res = []
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_DEAD_STORES', switch)
        fe = plastic_model()
        eng = fe._ensure_engine()
        eng.state_reset()
        eng.assemble()
        z = np.zeros(2)
        eng.apply_bc(*fe._bc_data(z, z, z, np.array([0., EPS * fe.leny]), None))
        it, rr, ok = eng.solve(1e-10, 20000, False)
        assert ok
        r0 = eng.sweep_info()[1]
        changed, conv = eng.sweep(0)
        res.append(dict(res_sig=eng.state_get(_lib.ST_RES_SIG), res_depl=eng.state_get(_lib.ST_RES_DEPL), fyn=eng.state_get(_lib.ST_FYN),
                        changed=changed, rewritten=eng.sweep_info()[1] - r0, dead=eng.dead_store_info()))
    a, b = res
    print('direct sweep: changed %s, tangents rewritten %d of %d, dead_store_info %s' % (a['changed'], a['rewritten'], fe.Nel, a['dead']))
    assert a['changed'] and a['rewritten'] > 0 and a['rewritten'] == b['rewritten']
    assert a['dead'] == (0, 0, 0, 0) and b['dead'] == (0, 0, 0, 0)
    assert np.all(np.any(a['res_sig'] != 0., axis=1)) and np.all(a['fyn'].ravel() > 0.)      # every element was stored
    for k in ('res_sig', 'res_depl', 'fyn'):
        assert np.array_equal(a[k], b[k]), k


def test_reuse_off_switches_it_off(monkeypatch):
    monkeypatch.setenv('PLFX_REUSE', '0')
    monkeypatch.setenv('PLFX_DEAD_STORES', '1')
    fe = solved(plastic_model(), 2)
    assert np.max(np.abs(fe._state('epl'))) > 0.
    assert fe._ensure_engine().dead_store_info() == (0, 0, 0, 0)

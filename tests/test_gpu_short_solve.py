"""Three passes a solve answered by the interpolated start never needs (PLFX_SHORT_SOLVE, a bit mask read
when the engine is created): (1) the fine level's dinv after a tangent update waits, like the coarse set-up, for the first
reader of its values -- until then only its zero pattern is read; (2) k_pred_finish leaves the d of the next interpolated
start behind and k_pred_diff is left out while nothing else has written x, pred_x or pred_d.  (Bit 4, one launch behind a
sweep's flags instead of two, was taken out again: the library ignores it and spec_merged stays 0.)  None of that may be seen in
a result: every case runs with PLFX_SHORT_SOLVE=7 and =0 (the parent's launches) in child processes and compares u, f, sig,
eps, epl, sgl, egl, niter and the PCG iterations per solve bit for bit; the first case runs each of the two bits alone as
well.  plfx_short_info's counters (dinv_deferred, dinv_formed_late, d_kept, spec_merged) say which path ran.

Shapes (those of tests/test_gpu_bc_rows.py and tests/test_gpu_pred_start.py).  The interpolated start is tried from 16 384
nodes up: 128 x 128 (16 641 nodes) and 160 x 104 (16 905, not square) are the smallest meshes that reach it, neither a
multiple of the 256-thread block.  Eight load steps of min_step=50 reach yielding and ONE accepted start, in load step 8
(measured on both meshes: predict_info (1, 3, 0), short_info (2, 1, 0, 0)): its d is kept, but the run ends before a solve
could use it.  The eight-step runs therefore check everything but d_kept > 0, and the same two meshes run ten load steps as
well, where the starts of steps 9 and 10 find their d written (d_kept == accepted - 1).  With the soft inclusion
every tried start of the first twelve steps is rejected and iterates, so every deferred dinv is formed in front of its
V-cycle.  The 25 x 25 all-plastic and 15 x 15 mixed models stay below the gate and take several stiffness iterations per load
step, each starting with the plain k_cg_start, which reads dinv's values -- but nothing is ever deferred on them (measured:
their apply_bc finds no coarse set-up pending), so the 64 x 64 tension model (4225 nodes: below the gate, with a multigrid
hierarchy) runs the same eight load steps beside them.  The engine cases go on from the state the eight
load steps on 128 x 128 leave -- the last solve answered by an interpolated start, its d kept, the fine dinv still unformed --
with apply_bc / solve / precond_apply of the engine."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('u', 'f', 'sig', 'eps', 'epl', 'sgl', 'egl', 'niter', 'its')
MESHES = [(128, 128), (160, 104)]

CHILD = r'''
import os, sys, warnings
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import pylabfea_amd as FE
from pylabfea_amd import _lib
case, out = sys.argv[1], sys.argv[2]


def model_arrays(fe):
    return dict(u=np.array(fe.u), f=np.array(fe.f), sig=fe._state('sig'), eps=fe._state('eps'), epl=fe._state('epl'),
                sgl=np.asarray(fe.sgl), egl=np.asarray(fe.egl), epgl=np.asarray(fe.epgl), niter=np.asarray(fe.niter),
                its=np.array([q[0] for q in fe.solver_stats]), nsteps=np.array(fe.nsteps))


def run_model(fe, min_step, steps=None):
    fe._max_load_steps = steps
    per_step = []   # after every load step: solves so far, then the four counters
    fe._step_hook = lambda il: per_step.append((len(fe.solver_stats),) + tuple(fe._engine.short_info()))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=min_step)
    eng = fe._engine
    return dict(model_arrays(fe), info=np.array(eng.short_info()), predict=np.array(eng.predict_info()),
                bc=np.array(eng.bc_info()), per_step=np.array(per_step))


def inclusion(nx, ny):
    """the soft inclusion of tests/test_gpu_pred_start.py"""
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


def engine_case(change):
    """eight load steps of the 128 x 128 tension model, then apply_bc / solve of the engine; counters after every solve"""
    from test_gpu_pred_start import tension
    fe = tension(128, 128)
    res = run_model(fe, 50, 8)
    eng = fe._engine
    z = np.zeros(2)
    du, its, info = [], [], [eng.short_info()]

    def solve(dbcr, dbct):
        eng.apply_bc(*fe._bc_data(z, z, np.array(dbcr, dtype=float), np.array(dbct, dtype=float), None))
        it, rr, ok = eng.solve(1e-10, 20000, True)
        assert ok
        du.append(eng.state_get(_lib.ST_DU))
        its.append(it)
        info.append(eng.short_info())
    d = 1.e-4 * fe.leny
    if change == 'force':
        solve([40., 0.], [0., d])          # a force vector on the right edge: the full pass writes dinv
        solve([25., 0.], [0., 2 * d])
        fe.bcright(0., 'force')
        solve([0., 0.], [0., d])           # the force is gone
        solve([0., 0.], [0., 3 * d])       # rows only again
    elif change == 'set':
        fe.bctop(0., 'force')              # top edge free, right edge prescribed; left and bottom kept
        fe.bcright(0.5 * d, 'disp')
        solve([0.5 * d, 0.], [0., 0.])     # another Dirichlet set: the full pass; the kept d has the old mask
        solve([d, 0.], [0., 0.])           # rows only, with the new row list
    elif change == 'same':
        solve([0., 0.], [0., d])           # the same set, other values: the late dinv is formed, the kept d is used
        solve([0., 0.], [0., 2 * d])
    else:   # 'precond': one V-cycle on a host vector while the fine dinv is still unformed
        r = np.random.default_rng(7).standard_normal(eng.ndof)
        du.append(eng.precond_apply(r))
        its.append(0)
        info.append(eng.short_info())
    return dict(du=np.array(du), its=np.array(its), info=np.array(info), predict=res['predict'], u=res['u'])


if case == 'tension':
    from test_gpu_pred_start import tension
    res = run_model(tension(int(sys.argv[3]), int(sys.argv[4])), 50, int(sys.argv[5]))
elif case == 'inclusion':
    res = run_model(inclusion(int(sys.argv[3]), int(sys.argv[4])), 50, 12)
elif case == 'plastic':
    from test_gpu_end_of_step import plastic_model
    res = run_model(plastic_model(), 2)
elif case == 'mixed':
    from test_gpu_sweep_prefetch import mixed_model
    res = run_model(mixed_model(15, 15, 0.01), 2)
else:
    res = engine_case(case)
np.savez(out, **res)
'''


def run(tmp_path, tag, args, **env):
    out = str(tmp_path / (tag + '.npz'))
    e = {k: v for k, v in os.environ.items() if k not in ('PLFX_SHORT_SOLVE', 'PLFX_REUSE', 'PLFX_PREDICT')}
    e.update(env)
    subprocess.run([sys.executable, '-c', CHILD % {'root': ROOT}, args[0], out] + [str(a) for a in args[1:]], check=True, env=e,
                   cwd=ROOT, timeout=120)
    return np.load(out)


def on_off(tmp_path, args):
    return run(tmp_path, 'on', args, PLFX_SHORT_SOLVE='7'), run(tmp_path, 'off', args, PLFX_SHORT_SOLVE='0')


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def iterated_behind_a_deferral(a):
    """Solves that iterated with a deferred dinv in front of them, from the counters after every load step.  A load step is
    the predictor solve and one solve per stiffness iteration; apply_bc defers exactly where the sweep of the iteration before
    changed a tangent, and from the first such sweep every later iteration of the step follows one: the deferrals of a step
    belong to its LAST solves.  NOT independent of the code under test: the count is built on the library's own per-step
    dinv_deferred and on that assumption.  It pins dinv_formed_late to an exact number; what carries the weight is the
    cross-check late == deferred - accepted and, above all, the bit-for-bit comparison against PLFX_SHORT_SOLVE=0."""
    n0, d0, count = 0, 0, 0
    for row in a['per_step']:
        n1, d1 = int(row[0]), int(row[1])
        its = a['its'][n0:n1]
        if d1 > d0:
            count += int(np.sum(its[len(its) - (d1 - d0):] > 0))
        n0, d0 = n1, d1
    return count


@pytest.mark.parametrize('steps', [8, 10])
@pytest.mark.parametrize('nx,ny', MESHES)
def test_bench_tension_model(nx, ny, steps, tmp_path):
    assert (nx + 1) * (ny + 1) >= 16384 and ((nx + 1) * (ny + 1)) % 256 != 0
    a, b = on_off(tmp_path, ('tension', nx, ny, steps))
    deferred, late, kept, merged = a['info']
    print('%d x %d: short_info on %s off %s, predict_info %s, bc_info %s, niter %s, PCG iterations %s'
          % (nx, ny, tuple(a['info']), tuple(b['info']), tuple(a['predict']), tuple(a['bc']), list(a['niter']), list(a['its'])))
    assert int(a['nsteps']) == steps and np.max(np.abs(a['epl'])) > 0.
    assert_same(a, b)
    assert tuple(b['info']) == (0, 0, 0, 0)
    accepted = int(a['predict'][0])
    assert accepted >= 1 and np.array_equal(a['predict'], b['predict'])   # accepted starts
    assert deferred > 0 and merged == 0
    # dinv_formed_late is the number of solves that iterated BEHIND A DEFERRAL: the other solves that iterate -- the cold first
    # one, the first ones after yielding -- run behind a k_bc_finish or k_dinv of apply_bc and have nothing to form
    assert late == iterated_behind_a_deferral(a) and late >= 1
    assert late == deferred - accepted      # ... and every other deferred dinv was answered by an accepted start, unread
    # every accepted start but the first finds the d that the one before it left behind.  The issue's d_kept > 0 cannot hold
    # on its own eight-step case (one accepted start, in step 8: measured); it is asserted on the ten-step run added for it
    assert kept == accepted - 1
    if steps == 10:
        assert kept > 0


@pytest.mark.parametrize('steps', [8, 10])
@pytest.mark.parametrize('bit', [1, 2])
def test_each_bit_alone(bit, steps, tmp_path):
    nx, ny = MESHES[0]
    a = run(tmp_path, 'bit', ('tension', nx, ny, steps), PLFX_SHORT_SOLVE=str(bit))
    b = run(tmp_path, 'off', ('tension', nx, ny, steps), PLFX_SHORT_SOLVE='0')
    print('PLFX_SHORT_SOLVE=%d, %d load steps: short_info %s' % (bit, steps, tuple(a['info'])))
    assert_same(a, b)
    deferred, late, kept, merged = a['info']
    assert (deferred > 0) == (bit == 1) and merged == 0
    assert kept == (int(a['predict'][0]) - 1 if bit == 2 else 0)   # (ten load steps: > 0, see test_bench_tension_model)
    if bit != 1:
        assert late == 0


@pytest.mark.parametrize('nx,ny', MESHES)
def test_rejected_starts_form_dinv_before_the_vcycle(nx, ny, tmp_path):
    a, b = on_off(tmp_path, ('inclusion', nx, ny))
    c = run(tmp_path, 'nopredict', ('inclusion', nx, ny), PLFX_PREDICT='0')
    print('%d x %d with inclusion: short_info %s, predict_info %s, PCG iterations %s'
          % (nx, ny, tuple(a['info']), tuple(a['predict']), list(a['its'])))
    assert int(a['nsteps']) == 12 and np.max(np.abs(a['epl'])) > 0.
    assert a['predict'][2] >= 1 and a['predict'][0] == 0       # starts were tried and rejected, none accepted
    assert_same(a, b)
    assert_same(a, c)
    assert tuple(b['info']) == (0, 0, 0, 0)
    deferred, late, kept, merged = a['info']
    assert deferred > 0 and late == deferred                   # every deferred dinv was formed in front of its V-cycle
    assert late == iterated_behind_a_deferral(a) and merged == 0
    assert kept == 0                                           # no accepted start, so no d was ever left behind
    assert tuple(c['info']) == (0, 0, 0, 0)                   # PLFX_PREDICT=0: the set-up is not lazy, nothing is deferred


@pytest.mark.parametrize('case,ndof', [('plastic', 2 * 26 * 26), ('mixed', 2 * 16 * 16)])
def test_small_models_several_stiffness_iterations(case, ndof, tmp_path):
    a, b = on_off(tmp_path, (case,))
    print('%s: short_info on %s off %s, load steps %d, niter %s' % (case, tuple(a['info']), tuple(b['info']), int(a['nsteps']), list(a['niter'])))
    assert a['u'].size == ndof and ndof < 2 * 16384
    assert np.max(np.abs(a['epl'])) > 0. and np.max(a['niter']) >= 2
    assert_same(a, b)
    assert tuple(b['info']) == (0, 0, 0, 0)
    deferred, late, kept, merged = a['info']
    assert kept == 0                        # below the gate of the interpolated start
    # Every stiffness iteration starts with k_cg_start, so a deferred dinv would be formed in front of it every time -- but none
    # is deferred on these two (measured (0, 0, 0, 0): no coarse set-up is pending when their apply_bc runs, k_dinv is launched
    # there as before), and late == deferred holds with both sides zero.  test_below_the_gate_with_a_hierarchy is the case
    # that exercises ensure_dinv in front of the plain start.
    assert late == deferred and merged == 0


def test_below_the_gate_with_a_hierarchy(tmp_path):
    """64 x 64 tension model, eight load steps: below the 16 384-node gate no interpolated start is tried, every solve behind a
    tangent update starts with the plain k_cg_start (z = dinv r) and forms the deferred dinv in front of it"""
    a, b = on_off(tmp_path, ('tension', 64, 64, 8))
    print('64 x 64: short_info on %s off %s, predict_info %s, niter %s, PCG iterations %s'
          % (tuple(a['info']), tuple(b['info']), tuple(a['predict']), list(a['niter']), list(a['its'])))
    assert 65 * 65 < 16384 and tuple(a['predict']) == (0, 0, 0) and np.max(np.abs(a['epl'])) > 0.
    assert_same(a, b)
    assert tuple(b['info']) == (0, 0, 0, 0)
    deferred, late, kept, merged = a['info']
    assert deferred > 0 and late == deferred and kept == 0 and merged == 0


def engine_counters(a):
    return [tuple(int(v) for v in row) for row in a['info']]


def test_dirichlet_set_changes_after_an_accepted_start(tmp_path):
    a, b = on_off(tmp_path, ('set',))
    info = engine_counters(a)
    print('short_info after the load steps and after each solve:', info, 'PCG iterations', list(a['its']))
    assert_same(a, b, ('du', 'its', 'u'))
    assert not np.any(b['info'])
    assert a['predict'][0] >= 1
    (def0, late0, kept0, _), (def1, late1, kept1, _), (def2, late2, kept2, _) = info
    assert def0 > late0                      # the load steps end with a deferred dinv still unformed (and the d of step 8 kept)
    assert late1 == late0                    # another set: the full pass wrote dinv, the deferred one was dropped, not formed late
    # ... and the kept d (masked with the old set) was not used: k_pred_diff ran.  This does NOT single out the clear of
    # pred_d_kept on a changed set: a changed set also makes the solve rebuild x (k_x0), which drops the kept d by itself, so a
    # build without that clear passes here too -- the clear is defence in depth, and the case checks the outcome only
    assert kept1 == kept0
    assert (def2, late2) == (def0, late0)    # rows only with the new set, diagonal unchanged: nothing deferred
    assert np.any(a['du'][1] != a['du'][0])


def test_force_vector_comes_and_goes_after_an_accepted_start(tmp_path):
    a, b = on_off(tmp_path, ('force',))
    info = engine_counters(a)
    print('short_info after the load steps and after each solve:', info, 'PCG iterations', list(a['its']))
    assert_same(a, b, ('du', 'its', 'u'))
    assert not np.any(b['info'])
    assert info[0][0] > info[0][1]
    for row in info[1:]:
        assert row[:2] == info[0][:2]        # the full pass of the force vector wrote dinv: dropped, never formed late
    assert info[1][2] == info[0][2] + 1      # (same set, x untouched: the kept d is this solve's d whatever the right-hand side)
    assert np.any(a['du'][1] != a['du'][0]) and np.any(a['du'][3] != a['du'][2])


def test_same_set_uses_the_kept_d_and_forms_the_late_dinv(tmp_path):
    a, b = on_off(tmp_path, ('same',))
    info = engine_counters(a)
    print('short_info after the load steps and after each solve:', info, 'PCG iterations', list(a['its']))
    assert_same(a, b, ('du', 'its', 'u'))
    assert not np.any(b['info'])
    (def0, late0, kept0, _), (def1, late1, kept1, _) = info[:2]
    assert late1 == late0 + 1                # plfx_solve starts with the plain k_cg_start: z = dinv r
    assert kept1 == kept0 + 1                # x and pred_x untouched since k_pred_finish: its d is this solve's d


def test_precond_apply_with_a_late_dinv(tmp_path):
    a, b = on_off(tmp_path, ('precond',))
    info = engine_counters(a)
    print('short_info after the load steps and after precond_apply:', info)
    assert_same(a, b, ('du', 'u'))
    assert np.all(np.isfinite(a['du'])) and np.any(a['du'] != 0.)
    assert info[0][0] > info[0][1]           # the load steps end with a deferred dinv still unformed ...
    assert info[1][1] == info[0][1] + 1      # ... and the V-cycle formed it first

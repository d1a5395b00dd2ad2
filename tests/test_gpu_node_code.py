"""The kernels of an interpolated start read the Dirichlet set from one byte per node, and the two start kernels load the
right-hand side on the rows next to prescribed nodes alone while it is zero elsewhere (PLFX_NODE_CODE, a
bit mask read when the engine is created: 1 = the mask from the code, 2 = the sparse rhs, which needs 1; default 1).  None of
that may be seen in a result: every case runs the masks 0 (the parent's launches), 1 and 3 as engines of ONE process -- the
variable is set in front of Model._ensure_engine -- and compares u, f, du, sig, eps, epl, sgl, egl, epgl, niter and the
iterations and relative residual of every solve with np.array_equal.  plfx_code_info's counters (built, start_launches,
b_sparse_launches, vector_launches) say which path ran; plfx_code_get returns the bytes.

Shapes.  The interpolated start is tried from 16 384 nodes up: 128 x 128 elements (16 641 nodes) and 160 x 104 (16 905, not
square) are the smallest meshes that reach it, neither a multiple of the 256-thread block, so the last block of every node
kernel is partial and the padding of the code is read by nobody.  Ten load steps of the bench tension model reach yielding and
accepted starts (tests/test_gpu_short_solve.py: the first in load step 8).  With the soft inclusion every tried start of the
first twelve steps is rejected and the solves iterate.  64 x 64 stays below the gate.  The 5 x 3 mesh (24 nodes) has all
three bits set on most nodes.  A model is solved once per (case, mask) and the result shared among the tests."""
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
KEYS = ('u', 'f', 'du', 'sig', 'eps', 'epl', 'sgl', 'egl', 'epgl', 'niter', 'its', 'relres')
MESHES = [(128, 128), (160, 104)]
_cache = {}


def tension(nx, ny):
    from test_gpu_pred_start import tension as t
    return t(nx, ny)


def inclusion(nx, ny):
    """the soft inclusion of tests/test_gpu_pred_start.py and tests/test_gpu_short_solve.py"""
    import pylabfea_amd as FE
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


def engine_with(fe, **env):
    """the model's engine, created with these variables set (the library reads them in plfx_create)"""
    keep = {k: os.environ.get(k) for k in ('PLFX_NODE_CODE', 'PLFX_PREDICT', 'PLFX_REUSE')}
    for k in keep:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fe._ensure_engine()
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def advance(fe, min_step, steps):
    """`steps` more load steps; code_info after each of them"""
    eng = fe._engine
    per_step = []
    fe._max_load_steps = steps
    fe._step_hook = lambda il: per_step.append(eng.code_info())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=min_step)
    return np.array(per_step)


def arrays(fe):
    eng = fe._engine
    return dict(u=np.array(fe.u), f=np.array(fe.f), du=np.array(fe.du), sig=fe._state('sig'), eps=fe._state('eps'),
                epl=fe._state('epl'), sgl=np.asarray(fe.sgl), egl=np.asarray(fe.egl), epgl=np.asarray(fe.epgl),
                niter=np.asarray(fe.niter), its=np.array([q[0] for q in fe.solver_stats]),
                relres=np.array([q[1] for q in fe.solver_stats]), info=tuple(int(v) for v in eng.code_info()),
                predict=tuple(int(v) for v in eng.predict_info()), code=eng.code_get(), nsteps=int(fe.nsteps))


def solved(case, nx, ny, steps, mask, predict=None):
    key = (case, nx, ny, steps, mask, predict)
    if key not in _cache:
        fe = (inclusion if case == 'inclusion' else tension)(nx, ny)
        env = {} if mask is None else {'PLFX_NODE_CODE': str(mask)}
        if predict is not None:
            env['PLFX_PREDICT'] = str(predict)
        engine_with(fe, **env)
        per_step = advance(fe, 50, steps)
        _cache[key] = dict(arrays(fe), per_step=per_step)
        fe._drop_engine()
    return _cache[key]


def assert_same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def code_from_definition(fe):
    """bit 0 / 1: the x / y DOF of the node is prescribed; bit 2: a node of the 3 x 3 neighbourhood (the node itself included)
    has a prescribed DOF.  Node j * (NY + 1) + k sits in column j, row k."""
    z = np.zeros(2)
    presc = np.asarray(fe._bc_data(z, z, z, z, None)[0])
    ncx, ncy = fe.NnodeX, fe.NnodeY
    code = np.zeros(ncx * ncy, dtype=np.uint8)
    np.bitwise_or.at(code, presc >> 1, (1 << (presc & 1)).astype(np.uint8))
    has = (code != 0).reshape(ncx, ncy)
    near = np.zeros((ncx + 2, ncy + 2), dtype=bool)
    for dj in range(3):
        for dk in range(3):
            near[dj:dj + ncx, dk:dk + ncy] |= has
    code[near[1:-1, 1:-1].ravel()] |= 4
    return code


@pytest.mark.parametrize('nx,ny', MESHES)
def test_bench_tension_model(nx, ny):
    assert (nx + 1) * (ny + 1) >= 16384 and ((nx + 1) * (ny + 1)) % 256 != 0
    r0, r1, r3 = (solved('tension', nx, ny, 10, m) for m in (0, 1, 3))
    print('%d x %d: code_info mask 0 %s, mask 1 %s, mask 3 %s, predict_info %s, niter %s, PCG iterations %s'
          % (nx, ny, tuple(r0['info']), tuple(r1['info']), tuple(r3['info']), tuple(r3['predict']), r3['niter'].tolist(), r3['its'].tolist()))
    assert r3['nsteps'] == 10 and np.max(np.abs(r3['epl'])) > 0.
    assert_same(r1, r0)
    assert_same(r3, r0)
    assert r3['predict'][0] >= 1 and np.array_equal(r3['predict'], r0['predict']) and np.array_equal(r1['predict'], r0['predict'])
    built, start, sparse, vector = r3['info']
    assert built == 1 and start > 0 and vector > 0
    assert sparse == start                      # no force vector in this run: every coded start took rhs as zero off bc_rows
    assert tuple(r1['info']) == (1, start, 0, vector)
    assert tuple(r0['info']) == (1, 0, 0, 0)    # (the code is formed whatever the switch says; nothing reads it)


def test_default_is_mask_1():
    nx, ny = MESHES[0]
    a, b = solved('tension', nx, ny, 10, None), solved('tension', nx, ny, 10, 1)
    assert_same(a, b)
    assert np.array_equal(a['info'], b['info'])


@pytest.mark.parametrize('nx,ny', [(128, 128), (5, 3)])
def test_code_from_its_definition(nx, ny):
    if (nx, ny) == (128, 128):
        fe = tension(nx, ny)
        code = solved('tension', nx, ny, 10, 3)['code']
    else:
        fe = tension(nx, ny)
        engine_with(fe)
        advance(fe, 50, 1)
        code = fe._engine.code_get()
        fe._drop_engine()
    ref = code_from_definition(fe)
    assert code.dtype == np.uint8 and code.shape == ref.shape == ((nx + 1) * (ny + 1),)
    print('%d x %d: nodes per code value %s' % (nx, ny, np.bincount(ref, minlength=8).tolist()))
    assert np.array_equal(code, ref)
    assert set(np.unique(ref)) <= {0, 4, 5, 6, 7}
    if (nx, ny) == (5, 3):
        assert np.sum(ref >= 4) > ref.size // 2 and np.sum(ref == 7) >= 1


def test_rejected_starts_iterate():
    nx, ny = MESHES[0]
    r3, r0 = solved('inclusion', nx, ny, 12, 3), solved('inclusion', nx, ny, 12, 0)
    rp = solved('inclusion', nx, ny, 12, None, predict=0)
    print('%d x %d with inclusion: code_info %s, predict_info %s, PCG iterations %s'
          % (nx, ny, tuple(r3['info']), tuple(r3['predict']), r3['its'].tolist()))
    assert r3['nsteps'] == 12 and np.max(np.abs(r3['epl'])) > 0.
    assert r3['predict'][2] >= 1 and r3['predict'][0] == 0 and np.max(r3['its']) > 0   # tried and rejected, none accepted
    assert_same(r3, r0)
    assert_same(r3, rp)
    assert r3['info'][1] > 0 and r3['info'][2] == r3['info'][1] and r3['info'][3] > 0
    assert tuple(r0['info'][1:]) == (0, 0, 0)
    # PLFX_PREDICT=0: no interpolated start, none of its kernels -- what is left is the one k_compose_du at the end of a solve
    assert tuple(rp['info'][1:3]) == (0, 0) and 0 < rp['info'][3] <= len(rp['its'])


def test_below_the_gate():
    """64 x 64 tension model: no interpolated start, so no coded launch of its kernels (k_compose_du at the end of a solve
    reads the code on every mesh)"""
    r3, r0 = solved('tension', 64, 64, 8, 3), solved('tension', 64, 64, 8, 0)
    print('64 x 64: code_info %s, predict_info %s' % (tuple(r3['info']), tuple(r3['predict'])))
    assert 65 * 65 < 16384 and tuple(r3['predict']) == (0, 0, 0) and np.max(np.abs(r3['epl'])) > 0.
    assert_same(r3, r0)
    built, start, sparse, vector = r3['info']
    assert built == 1 and start == 0 and sparse == 0
    assert vector <= len(r3['its'])             # at most the one k_compose_du of a solve
    assert tuple(r0['info']) == (1, 0, 0, 0)


def continued(change, mask):
    """eight load steps of the 128 x 128 tension model, then load steps with other boundary conditions from that state"""
    key = ('continued', change, mask)
    if key in _cache:
        return _cache[key]
    fe = tension(128, 128)
    engine_with(fe, PLFX_NODE_CODE=str(mask))
    eng = fe._engine
    phases = [advance(fe, 50, 8)]
    codes = [eng.code_get()]
    refs = [code_from_definition(fe)]
    if change == 'set':
        fe.bcright(2.e-4 * fe.lenx, 'disp')        # the right edge prescribed as well: another Dirichlet set
        phases.append(advance(fe, 40, 2))
        codes.append(eng.code_get())
        refs.append(code_from_definition(fe))
    elif change == 'force':
        fe.bcright(40., 'force')                    # a force on the right edge grows: a force vector in every apply_bc
        phases.append(advance(fe, 40, 2))
        fe.bcright(float(fe.bcr_mem[0]), 'force')   # held where it is: no increment, no force vector
        phases.append(advance(fe, 40, 2))
    else:   # 'same': the same set, other values
        fe.bctop(0.003 * fe.leny, 'disp')
        phases.append(advance(fe, 30, 2))
    res = dict(arrays(fe), codes=codes, refs=refs)
    for k, p in enumerate(phases):
        res['phase%d' % k] = p
    fe._drop_engine()
    _cache[key] = res
    return res


def test_another_dirichlet_set_rebuilds_the_code():
    a, b = continued('set', 3), continued('set', 0)
    print('code_info per load step: first set %s, second set %s' % (a['phase0'].tolist(), a['phase1'].tolist()))
    assert_same(a, b)
    assert a['predict'][0] >= 1
    assert a['phase0'][-1][0] == 1 and a['phase1'][0][0] == 2 and a['phase1'][-1][0] == 2   # built once per set
    assert np.array_equal(a['codes'][0], a['refs'][0]) and np.array_equal(a['codes'][1], a['refs'][1])
    assert np.any(a['codes'][1] != a['codes'][0])
    assert np.array_equal(b['codes'][1], a['codes'][1]) and tuple(b['info']) == (2, 0, 0, 0)
    assert a['phase1'][-1][1] > a['phase0'][-1][1]   # coded starts with the new set


def test_force_vector_comes_and_goes():
    a, b = continued('force', 3), continued('force', 0)
    p0, p1, p2 = a['phase0'], a['phase1'], a['phase2']
    print('code_info per load step: no force %s, force grows %s, force held %s' % (p0.tolist(), p1.tolist(), p2.tolist()))
    assert_same(a, b)
    assert tuple(b['info']) == (1, 0, 0, 0)
    assert p2[-1][0] == 1                            # one Dirichlet set throughout
    start0, sparse0 = p0[-1][1], p0[-1][2]
    assert sparse0 == start0 > 0
    # while the force grows every apply_bc carries a force vector: coded starts, none of them with the sparse rhs
    assert p1[-1][1] > start0 and p1[-1][2] == sparse0
    # held: the first apply_bc is a full pass without a force vector, and from the solve behind it on rhs is sparse again
    assert p2[-1][1] > p1[-1][1] and p2[-1][2] - p1[-1][2] == p2[-1][1] - p1[-1][1]


def test_same_set_other_values():
    a, b = continued('same', 3), continued('same', 0)
    print('code_info per load step: %s, then %s' % (a['phase0'].tolist(), a['phase1'].tolist()))
    assert_same(a, b)
    assert a['phase1'][-1][0] == 1                   # the same set: the code stands
    assert a['phase1'][-1][1] > a['phase0'][-1][1] and a['phase1'][-1][2] == a['phase1'][-1][1]
    assert tuple(b['info']) == (1, 0, 0, 0)

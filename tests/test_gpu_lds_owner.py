"""The thread-per-element SVC sweep kernels with tables above 64 KiB of dynamic LDS.

plfx_set_materials raises the dynamic-LDS limit of every kernel that stages SVC tables, and each kernel is compiled, launched and
raised by one translation unit.  A kernel whose limit was raised on another registration than the one that is launched fails at
its first launch with more than 64 KiB.  The row kernels have such launches all over the suite (the list is in DESIGN 39); the
thread-per-element forms k_sweep_light / k_sweep_heavy <3>, <6> and k_scf_elements run only with PLFX_SVC_WAVE=0 or for an SVC
that is not a 6-feature one, and had no model test with the 1585-vector tables (88 760 bytes).  These are those tests: config 4
on the thread kernels to the bar of test_config4_schedule_4x4, and a laminate of the 6-feature and the principal-stress SVC,
whose thread kernels <6> are launched with the LDS of the whole table set."""
import os
import warnings

import numpy as np
import pytest

from test_gpu_model import FE, check_fields, svc_material, tension_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cfg(golden_dir):
    return np.load(os.path.join(golden_dir, 'solve_configs.npz'))


def solved(fe, min_step):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=min_step)
    return fe


def test_config4_on_the_thread_kernels(cfg, golden_dir, monkeypatch):
    """k_sweep_light<3>, k_sweep_heavy<3>, k_scf_elements with the 1585-vector tables in LDS: the reference's 4 x 4 trace, the bar of
    test_config4_schedule_4x4 (2e-6: brentq's xtol in ML_full_yf)"""
    monkeypatch.setenv('PLFX_SVC_WAVE', '0')                  # read at plfx_create
    fe = solved(tension_model(svc_material(golden_dir, 'hill'), 4, 0.001), 10)
    row, thread, nrow, nthread = fe._engine.svc_info()
    assert row == 0 and thread == 1 and nrow == 0 and nthread >= fe.n_sweeps
    check_fields(fe, cfg, 'cfg4_svc_4', rtol=2e-6)


def sdim3_material(golden_dir):
    z = np.load(os.path.join(golden_dir, 'svc_hill3d.npz'))
    m = FE().Material(name='ML-sdim3')
    m.elasticity(E=float(z['par_E']), nu=float(z['par_nu']))
    m.plasticity(sy=float(z['par_sy']), sdim=3)
    m.set_svc(z['par_sv'], z['par_dual'], float(z['par_intercept']), float(z['par_gamma']), float(z['par_scale_seq']))
    return m


def two_svc_kinds(golden_dir):
    fe = FE().Model(dim=2, planestress=False)
    fe.geom([2, 2], LY=4.)
    fe.assign([svc_material(golden_dir, 'hill'), sdim3_material(golden_dir)])
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(0.001 * fe.leny, 'disp')
    fe.mesh(NX=4, NY=4)
    return fe


def test_two_svc_kinds_in_one_model(golden_dir, monkeypatch):
    """a 6-feature SVC (1585 vectors) beside a principal-stress SVC on 4 x 4: the thread kernels <6> of the second are launched with
    the dynamic LDS of the whole table set (> 64 KiB) in both runs, the kernels <3> of the first with PLFX_SVC_WAVE=0.  The two
    runs differ in the form of the first material's kernels alone: the same schedule, fields to the 2e-6 of a row form against a
    thread form (brentq's xtol, as in config 4)"""
    out = []
    for wave in ('1', '0'):
        monkeypatch.setenv('PLFX_SVC_WAVE', wave)
        fe = solved(two_svc_kinds(golden_dir), 10)
        row, thread, nrow, nthread = fe._engine.svc_info()       # (the masks list 6-feature SVC materials only)
        assert (row, thread) == ((0b01, 0) if wave == '1' else (0, 0b01))
        assert (nrow if wave == '1' else nthread) >= fe.n_sweeps
        out.append((fe.nsteps, list(fe.niter), np.array(fe.u), np.array(fe.sgl), fe._state('sig').copy(), fe._state('epl').copy(),
                    fe._state('eps').copy(), fe._mat_id.copy()))
    a, b = out
    assert a[:2] == b[:2] and sum(a[1]) > 0                    # stiffness iterations: an element yielded
    assert np.max(np.abs(a[5][a[7] == 0])) > 0.                # ... of the 6-feature material
    for k in (2, 3, 4):
        assert np.max(np.abs(a[k] - b[k])) <= 2e-6 * np.max(np.abs(b[k])), k
    assert np.max(np.abs(a[5] - b[5])) <= 2e-6 * np.max(np.abs(b[6]))


def test_response_of_a_texture_field_on_the_1585_vector_tables(golden_dir, tmp_path):
    """k_response_row<true, true, true, TexFieldDev> with its tables in LDS above 64 KiB (the point tests of test_gpu_texture_field.py
    cut the tables to 65 vectors at the most): the folded 1585-vector set of its model test with three textures, 48 points with a
    row each, against the material bound to each texture -- equal bits, the bar of test_points_against_the_bound_materials"""
    import texture_bound_cases as TB
    import texture_cases as TC
    import yield_locus_cases as YC
    p6 = YC.ml_params('hill')
    q = TB.equal_scale_texture_set(p6, np.random.default_rng(11))
    par = TB.parent(FE(), TC.facade(FE(), TC.load(), tmp_path, 'GSH_3')[0], q)
    CV = np.load(os.path.join(golden_dir, 'svc_hill.npz'))['par_CV']
    par.elasticity(CV=CV)
    par.sy = par.sy0 = p6['sy']
    tex = np.array([[0.1, -0.1, 0.05], [-0.15, 0.1, 0.1], [0.05, 0.15, -0.1]])
    F, bound = par.at_textures(tex), [par.at_texture(t) for t in tex]
    sig, epl, deps, _ = TB.seeded_points(par.fold_texture(tex[0]), CV, 48, 71)
    ids = (np.arange(48) % 3).astype(np.int32)
    got = F.response_batch(sig, epl, deps, CV, tex_id=ids)
    ctx = F._load(CV)
    assert ctx.svc_info()[:2] == (1, 0)                                   # on the row kernels; 1585 vectors fit the LDS (2176 do)
    assert ctx.svc_textures_info(0)['rows'] == 3 and ctx.svc_textures_info(0)['launches'] >= 1   # the field kernel ran
    assert np.any(got[4] > 0)                                             # plastic points
    for t in range(3):
        want = bound[t].response_batch(sig[ids == t], epl[ids == t], deps[ids == t], CV)
        for a, b in zip(got, want):
            assert np.array_equal(np.asarray(a)[ids == t], np.asarray(b)), t

#!/usr/bin/env python3
"""GPU time of Material.texture_loci (k_tex_yield_scale: T textures x 72 pi-plane rays searched in one launch) beside the same
loci as one yield_scale call per texture -- the loop of the reference's examples/Texture/train_texture.py, which solves one
coupled fsolve over Python calc_yf calls per texture -- and of calc_yf(tex=) (k_tex_yf) at 1 and 100 000 points.
Material: the GSH_3 fit of tests/golden/texture_svc.npz (522 support vectors, 9 features); T = 6, 100 and 7000 textures, the
fixture's six resampled (convex mixtures of two of them, fixed seed).  Kernel time from the library's HIP events on its
stream (timing family 0, plfx_timing_get): one warm-up call, then the median of --reps calls; wall time of the whole call
beside it.  Every step runs in a child process of its own under its own time limit, and nothing more is started after one
that fails.  One JSON line per step.

--flow times the flow rule and the stress update instead: calc_fgrad(tex=) (k_tex_fgrad) at 1 point and
at 100 000 points with a shared texture and with one texture per row -- beside calc_yf(tex=) at the same 100 000 points, whose
pass over the vectors the gradient repeats with six more FMAs per vector -- and response_batch(tex=) (k_tex_response) at 1
and at 10 000 plastic points: stresses on the yield locus of texture 2 with an oblique strain increment of 1.5e-3, which the
update sub-divides.

--bound times a material bound to one texture instead (Material.at_texture): bound.response_batch on
the 16-lane row kernels at 1 and at 10 000 of the plastic points of --flow, beside parent.response_batch(tex=) on the same
points in the same process; then one Model.solve on 256 x 256 elements, three sections bound at three training textures,
plane strain, a top displacement of 1.2 x the largest uniaxial yield strain in min_step = 10 increments (the schedule of
benchmark configuration 4), and for context the 6-feature 'hill' material of that configuration on the same mesh: wall time,
sweeps, and the corrector's kernel time per element update.

--field times a texture field instead (Material.at_textures), every figure the median of --reps runs
after one warm-up: the 256 x 256 model of --bound with its three bound sections (the laminate: three launches per sweep
phase) beside one field material with T = 3 and the rows by section (one launch), then the same mesh with T = 1024 (32 x 32
blocks of 8 x 8 elements) and T = 65 536 (one row per element) on convex mixtures of the fixture textures -- kernel ms per
sweep, us per element update, and the bytes of the coefficient rows a sweep touches beside the element state it streams --
and F.response_batch(tex_id=) at 10 000 plastic points with T = 6 beside parent.response_batch(tex=) with one texture per
row on the same points.

    python tools/texture_bench.py [--flow | --bound | --field] [--reps 11] [--limit 240]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
STEPS = ('loci:6', 'loci:100', 'loci:7000', 'yf:1', 'yf:100000')
FLOW_STEPS = ('fgrad:1', 'fgrad:100000', 'resp:1', 'resp:10000')
BOUND_STEPS = ('bound:1', 'bound:10000', 'model:256', 'model6:256')
FIELD_STEPS = ('lam:256', 'field:3', 'field:1024', 'field:65536', 'fresp:10000')
DESC = 'GSH_3'


def step(name, reps):
    import texture_cases as TC
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    from pylabfea_amd.material import _ctx
    kind, n = name.split(':')
    n = int(n)
    if kind in ('model', 'model6'):
        return model_step(kind, n)
    if kind in ('lam', 'field'):
        return field_model_step(kind, n, reps)
    z = TC.load()
    with tempfile.TemporaryDirectory() as tmp:
        m, _ = TC.facade(FE, z, tmp, DESC)
    TC.install(m, TC.tables(z, DESC))
    tex6 = TC.textures(z, DESC)
    rng = np.random.default_rng(n)
    ctx = _ctx()
    dev, cus, _ = ctx.device_info()
    ctx.timing_enable(True)
    ctx.timing_select([_lib.T_SWEEP])

    def timed(call):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            out = call()                                 # warm-up: code object load, table upload, allocations
            ms, wall, launches = [], [], 0
            for _ in range(reps):
                ctx.timing_reset()
                t0 = time.perf_counter()
                call()
                wall.append(1e3 * (time.perf_counter() - t0))
                t, launches = ctx.timing_get(_lib.T_SWEEP)
                ms.append(t)
        return out, float(np.median(ms)), float(np.median(wall)), int(launches)

    res = dict(device=dev, cus=cus, step=name, nsv=int(len(m.svc['dual'])), features=int(m.Ndof), reps=reps,
               staged=None)
    if kind == 'loci':
        if n == 6:
            tex = tex6
        else:   # resampled: convex mixtures of two of the fixture's textures
            a, b = rng.integers(0, 6, size=n), rng.integers(0, 6, size=n)
            w = rng.uniform(0., 1., size=(n, 1))
            tex = np.ascontiguousarray(w * tex6[a] + (1. - w) * tex6[b])
        _, snorm = TC.snorm()
        (_, seq, st), k_ms, k_wall, k_l = timed(lambda: m.texture_loci(tex, return_status=True))
        assert k_l == 1
        res.update(textures=n, rays=int(st.size), rays_with_root=int(np.sum(st == 0)), one_launch_kernel_ms=k_ms,
                   one_launch_wall_ms=k_wall)

        def per_texture():
            return np.array([m.yield_scale(snorm, tex=t) for t in tex])
        x, p_ms, p_wall, p_l = timed(per_texture)
        assert p_l == n
        res.update(per_texture_kernel_ms=p_ms, per_texture_wall_ms=p_wall, per_texture_launches=p_l,
                   wall_ratio=p_wall / k_wall, kernel_ratio=p_ms / k_ms,
                   same_bits=bool(np.array_equal(FE.sig_eq_j2((snorm[None] * x[:, :, None]).reshape(-1, 6)).reshape(x.shape)[st == 0],
                                                 seq[st == 0]) and np.all(np.isnan(x[st != 0]))))
    elif kind == 'fgrad':
        u = rng.normal(size=(n, 6))
        sig = u / np.linalg.norm(u, axis=1)[:, None] * 100.
        tid = rng.integers(0, 6, size=n)
        a1, s_ms, s_wall, s_l = timed(lambda: m.calc_fgrad(sig, tex=tex6[2]))
        a2, r_ms, r_wall, r_l = timed(lambda: m.calc_fgrad(sig, tex=tex6[tid]))
        y1, y_ms, y_wall, y_l = timed(lambda: m.calc_yf(sig, tex=tex6[2]))
        assert s_l == 1 and r_l == 1 and y_l == 1 and np.all(np.isfinite(a1)) and np.all(np.isfinite(a2))
        res.update(points=n, shared_texture_kernel_ms=s_ms, shared_texture_wall_ms=s_wall, texture_per_row_kernel_ms=r_ms,
                   texture_per_row_wall_ms=r_wall, calc_yf_shared_texture_kernel_ms=y_ms, calc_yf_shared_texture_wall_ms=y_wall,
                   kernel_ratio_to_calc_yf=s_ms / y_ms)
    elif kind in ('resp', 'bound', 'fresp'):
        cand = np.array(z['probe_sig'])
        import yield_locus_cases as YC
        su = cand / YC.j2(cand)[:, None]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            x = m.yield_scale(su, tex=tex6[2])
        on = (x[:, None] * su)[np.isfinite(x)]
        sig = np.ascontiguousarray(on[np.arange(n) % len(on)])
        v = rng.normal(size=(n, 6))
        deps = 1.5e-3 * v / np.linalg.norm(v, axis=1)[:, None]
        epl = np.zeros((n, 6))
        CV = np.array(m.CV)
        tid = rng.integers(0, 6, size=n).astype(np.int32) if kind == 'fresp' else np.full(n, 2, dtype=np.int32)
        out, k_ms, k_wall, k_l = timed(lambda: m.response_batch(sig, epl, deps, CV, tex=tex6[tid] if kind == 'fresp' else tex6[2]))
        assert k_l == 1 and np.all(np.isfinite(out[1]))
        res.update(points=n, sub_divided=int(np.sum(out[4] == 49)), kernel_ms=k_ms, wall_ms=k_wall)
        if kind == 'bound':   # the same points on the row kernels, in the same process
            b = m.at_texture(tex6[2])
            got, b_ms, b_wall, b_l = timed(lambda: b.response_batch(sig, epl, deps, CV))
            assert b_l == 1 and np.all(np.isfinite(got[1]))
            res.update(bound_kernel_ms=b_ms, bound_wall_ms=b_wall, kernel_ratio=k_ms / b_ms, wall_ratio=k_wall / b_wall,
                       bound_sub_divided=int(np.sum(got[4] == 49)), nsteps_equal=int(np.sum(got[4] == out[4])),
                       max_stress_difference_over_sy=float(np.max(np.abs(got[1] - out[1]))) / float(m.sy))
        if kind == 'fresp':   # the same points with one texture row each on the field kernels, in the same process
            F = m.at_textures(tex6)
            got, f_ms, f_wall, f_l = timed(lambda: F.response_batch(sig, epl, deps, CV, tex_id=tid))
            assert f_l == 1 and np.all(np.isfinite(got[1]))
            res.update(textures=6, field_kernel_ms=f_ms, field_wall_ms=f_wall, kernel_ratio=k_ms / f_ms, wall_ratio=k_wall / f_wall,
                       field_sub_divided=int(np.sum(got[4] == 49)), nsteps_equal=int(np.sum(got[4] == out[4])),
                       max_stress_difference_over_sy=float(np.max(np.abs(got[1] - out[1]))) / float(m.sy))
    else:
        u = rng.normal(size=(n, 6))
        sig = u / np.linalg.norm(u, axis=1)[:, None] * 100.
        tid = rng.integers(0, 6, size=n)
        y1, s_ms, s_wall, s_l = timed(lambda: m.calc_yf(sig, tex=tex6[2]))
        y2, r_ms, r_wall, r_l = timed(lambda: m.calc_yf(sig, tex=tex6[tid]))
        assert s_l == 1 and r_l == 1
        res.update(points=n, shared_texture_kernel_ms=s_ms, shared_texture_wall_ms=s_wall, texture_per_row_kernel_ms=r_ms,
                   texture_per_row_wall_ms=r_wall)
    res['staged'] = ctx.tex_svc_info()['staged']
    ctx.timing_enable(False)
    print(json.dumps(res))
    return 0


def model_step(kind, n):
    """one Model.solve on n x n elements: three sections bound at three training textures (model), or the 6-feature 'hill'
    material of benchmark configuration 4 in all three (model6)"""
    import texture_cases as TC
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    if kind == 'model':
        z = TC.load()
        with tempfile.TemporaryDirectory() as tmp:
            m, _ = TC.facade(FE, z, tmp, DESC)
        TC.install(m, TC.tables(z, DESC))
        tex = TC.textures(z, DESC)[:3]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ys = [float(m.yield_scale(np.array([0., 1., 0., 0., 0., 0.]), tex=t)) for t in tex]
        mats = [m.at_texture(t) for t in tex]
        eps, nsv = 1.2 * max(ys) / m.E, len(m.svc['dual'])
    else:
        g = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_hill.npz'))
        m6 = FE.Material(name='ML-Hill-p1')
        m6.elasticity(CV=g['par_CV'])
        m6.plasticity(sy=float(g['par_sy']), sdim=6)
        m6.set_svc(g['par_sv'], g['par_dual'], float(g['par_intercept']), float(g['par_gamma']), float(g['par_scale_seq']))
        mats, eps, nsv = [m6, m6, m6], 0.001, len(g['par_dual'])
    fe = FE.Model(dim=2, planestress=False)
    fe.geom([1, 1, 1], LY=3.)
    fe.assign(mats)
    fe.bcleft(0.)
    fe.bcbot(0.)
    fe.bcright(0., 'force')
    fe.bctop(eps * fe.leny, 'disp')
    fe.mesh(NX=n, NY=n)
    eng = fe._ensure_engine()
    dev, cus, _ = eng.device_info()
    eng.timing_reset()
    eng.timing_select((_lib.T_SWEEP, _lib.T_SWEEP_HEAVY))
    eng.timing_enable(True)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fe.solve(min_step=10)
    eng.sync()
    wall = time.perf_counter() - t0
    eng.timing_enable(False)
    ms_l, n_l = eng.timing_get(_lib.T_SWEEP)
    ms_h, n_h = eng.timing_get(_lib.T_SWEEP_HEAVY)
    row, thread, nrow, nthread = eng.svc_info()
    steps = np.asarray(fe._state('max_steps'))
    res = dict(device=dev, cus=cus, step='%s:%d' % (kind, n), nsv=int(nsv), elements=int(fe.Nel), eps=float(eps), wall_s=wall,
               load_steps=int(fe.nsteps), sweeps=int(fe.n_sweeps), streaming_kernel_ms=ms_l, corrector_kernel_ms=ms_h,
               streaming_launches=int(n_l), corrector_launches=int(n_h), row_materials=int(row), thread_launches=int(nthread),
               plastic_elements=int(np.sum(np.any(fe._state('epl') != 0., axis=1))), sub_divided_elements=int(np.sum(steps > 0)),
               us_per_element_update_wall=1e6 * wall / (fe.Nel * fe.n_sweeps),
               us_per_element_update_kernels=1e3 * (ms_l + ms_h) / (fe.Nel * fe.n_sweeps),
               sgl_yy=float(fe.sgl[-1][1]))
    print(json.dumps(res))
    return 0


def field_model_step(kind, T, reps):
    """Model.solve on 256 x 256 elements, the model of --bound: three sections bound at training textures 0, 1, 2 (lam), or
    one field material with T rows (field) -- T = 3: the rows by section, the laminate's problem; T = 1024: 32 x 32 blocks of
    8 x 8 elements; T = 65 536: one row per element.  One warm-up solve, then the median of reps solves."""
    import texture_cases as TC
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    n = 256
    z = TC.load()
    with tempfile.TemporaryDirectory() as tmp:
        m, _ = TC.facade(FE, z, tmp, DESC)
    TC.install(m, TC.tables(z, DESC))
    tex6 = TC.textures(z, DESC)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ys = [float(m.yield_scale(np.array([0., 1., 0., 0., 0., 0.]), tex=t)) for t in tex6[:3]]
    eps, nsv = 1.2 * max(ys) / m.E, len(m.svc['dual'])
    ids = None
    if kind == 'lam':
        mats = [m.at_texture(t) for t in tex6[:3]]
    else:
        if T == 3:
            tex = tex6[:3]
        else:   # convex mixtures of two of the fixture's textures, as the loci steps resample them
            rng = np.random.default_rng(T)
            a, b = rng.integers(0, 6, size=T), rng.integers(0, 6, size=T)
            w = rng.uniform(0., 1., size=(T, 1))
            tex = np.ascontiguousarray(w * tex6[a] + (1. - w) * tex6[b])
        t0 = time.perf_counter()
        F = m.at_textures(tex)
        fold_s = time.perf_counter() - t0
        mats = [F, F, F]
    rows = []
    for r in range(reps + 1):
        fe = FE.Model(dim=2, planestress=False)
        fe.geom([1, 1, 1], LY=3.)
        fe.assign(mats)
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(eps * fe.leny, 'disp')
        fe.mesh(NX=n, NY=n)
        if kind == 'field':
            j, k = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
            if T == 3:
                ids = np.asarray(fe._mat_id).reshape(n, n)
            elif T == 1024:
                ids = (j // 8) * 32 + (k // 8)
            else:
                ids = j * n + k
            assert ids.max() == T - 1
            fe.set_texture_ids(ids)
        eng = fe._ensure_engine()
        dev, cus, _ = eng.device_info()
        eng.timing_reset()
        eng.timing_select((_lib.T_SWEEP, _lib.T_SWEEP_HEAVY))
        eng.timing_enable(True)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fe.solve(min_step=10)
        eng.sync()
        wall = time.perf_counter() - t0
        eng.timing_enable(False)
        ms_l, n_l = eng.timing_get(_lib.T_SWEEP)
        ms_h, n_h = eng.timing_get(_lib.T_SWEEP_HEAVY)
        rows.append((wall, ms_l, ms_h, n_l, n_h))
        if r == reps:
            row, thread, nrow, nthread = eng.svc_info()
            info = eng.svc_textures_info(0)
            steps = np.asarray(fe._state('max_steps'))
            last = dict(load_steps=int(fe.nsteps), sweeps=int(fe.n_sweeps), row_materials=int(row), thread_launches=int(nthread),
                        field_rows=info['rows'], field_launches=info['launches'], rows_staged=info['staged'],
                        plastic_elements=int(np.sum(np.any(fe._state('epl') != 0., axis=1))),
                        sub_divided_elements=int(np.sum(steps > 0)), sgl_yy=float(fe.sgl[-1][1]))
        fe._drop_engine()
    t = np.array(rows[1:], dtype=float)
    med = np.median(t, axis=0)
    nsw, nel, rowpad = last['sweeps'], n * n, (nsv + 63) // 64 * 64
    res = dict(device=dev, cus=cus, step='%s:%d' % (kind, T), nsv=int(nsv), elements=nel, eps=float(eps), reps=reps,
               wall_s=float(med[0]), streaming_kernel_ms=float(med[1]), corrector_kernel_ms=float(med[2]),
               streaming_kernel_ms_min_max=[float(t[:, 1].min()), float(t[:, 1].max())],
               streaming_launches=int(med[3]), corrector_launches=int(med[4]),
               streaming_kernel_ms_per_sweep=float(med[1]) / nsw,
               us_per_element_update_wall=1e6 * float(med[0]) / (nel * nsw),
               us_per_element_update_kernels=1e3 * float(med[1] + med[2]) / (nel * nsw))
    res.update(last)
    if kind == 'field':
        # every element reads its row of rowpad doubles at least once per sweep (once per pass over the vectors; neighbours
        # with the same row share it in the caches): the distinct bytes, beside the element state a sweep streams -- read sig,
        # epl (96 B), connectivity and class (20 B), written res_sig, res_depl (96 B), fyn, max_steps (12 B), generators (48 B),
        # tangent factors and tag (57 B)
        res.update(textures=int(T), fold_s=fold_s, coefficient_table_bytes=int(T) * rowpad * 8,
                   coefficient_row_bytes=rowpad * 8, coefficient_bytes_per_sweep_at_one_read_per_element=nel * rowpad * 8,
                   element_state_bytes_per_sweep=nel * 329)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--limit', type=int, default=240, help='time limit of one step in seconds')
    ap.add_argument('--flow', action='store_true', help='time calc_fgrad(tex=) and response_batch(tex=) instead')
    ap.add_argument('--bound', action='store_true', help='time a material bound to one texture (at_texture) instead')
    ap.add_argument('--field', action='store_true', help='time a texture field (at_textures) beside the bound laminate instead')
    ap.add_argument('--step', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps)
    if a.reps < 10:
        ap.error('--reps must be at least 10 (median of >= 10 launches)')
    if a.flow + a.bound + a.field > 1:
        ap.error('--flow, --bound and --field are separate runs')
    for name in (FIELD_STEPS if a.field else BOUND_STEPS if a.bound else FLOW_STEPS if a.flow else STEPS):   # a fresh child per step, each under its own limit; stop at the first that fails
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__),
                              '--step', name, '--reps', str(a.reps)])
        if rc != 0:
            print('step %s ended with status %d; nothing more is started' % (name, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python3
"""Two builds of libplfx.so on the same solves, compared BIT FOR BIT (u, sig, epl, sgl, PCG iterations per solve) -- for
changes that must not move a number (a kernel rewritten with the same sums in the same order).

    python tools/probes/lib_ab.py [--more] [--points] pylabfea_amd/libplfx_prev.so pylabfea_amd/libplfx.so

Cases: even mesh with a soft inclusion (fine + coarse generators, the whole V-cycle), odd mesh 201 x 199 (levels with a wider
last column / row: area-scaled diagonal, k_mg_coarsen_M), non-proportional laminate (per-column widths).  --more adds config 4's
6-feature SVC material on 32 x 32 (the row kernels and their 50-sub-step corrector), config 5's J2 + SVC laminate on 128 x 64,
a solve on 64 x 64 with three indefinite element tangents that GMRES completes, and 32 x 32 with PLFX_MG_MAXIT=2, where
the single-GPU Jacobi-PCG fall-back completes the solves.  --points adds the batched point functions of the C-ABI (function
points below), the two of the context's texture set included: every output array of a call digested, inputs from a fixed-seed
generator, n = 67 and 1025 points."""
import hashlib
import os
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def points(out):
    """hessian and yield_scale (tables as trained, cut to the remainders of the 16-lane trip loop, padded past the LDS),
    committee_yf (as trained and with cut members), tex_svc_yf and tex_svc_yield_scale of the context's texture set (every
    padded width, the same cuts and padding) and, once each, seq / fgrad / fgrad_seq / fgrad_wh / yf / full_yf / response / the
    analytic yield_scale on principal stresses:
    name|digest of all outputs|n (yield_scale: n, rays with a root)"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import numpy as np
    import committee_cases as CC
    import pylabfea_amd as FE
    from pylabfea_amd import _lib

    def record(name, nsv=None, pad=0):
        """The trained SVC of tests/golden/svc_<name>.npz: its first nsv vectors, then `pad` more with a zero coefficient.  A
        cut table keeps vectors of the inner class only (negative coefficients); its intercept is set to half of what they
        sum to at zero stress, so that the function still changes sign along a ray and yield_scale returns roots."""
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_%s.npz' % name))
        sv, dual, icpt = z['par_sv'][:nsv], z['par_dual'][:nsv], float(z['par_intercept'])
        if nsv:
            x0 = np.array([-1., 0.]) if sv.shape[1] == 2 else np.zeros(sv.shape[1])
            icpt = 0.5 * abs(float(np.sum(dual * np.exp(-float(z['par_gamma']) * np.sum((sv - x0) ** 2, axis=1)))))
        sv, dual = np.vstack((sv, np.tile(sv[:1], (pad, 1)))), np.concatenate((dual, np.zeros(pad)))
        m = FE.Material(name='ML-' + name)
        m.elasticity(CV=z['par_CV'])
        m.plasticity(sy=float(z['par_sy']), sdim=int(z['par_sdim']))
        m.set_svc(sv, dual, icpt, float(z['par_gamma']), float(z['par_scale_seq']),
                  dev_only=bool(z['par_dev_only']), scale_wh=float(z['par_scale_wh']) if 'par_scale_wh' in z else None)
        return m._record(np.asarray(m.CV)), m.sy, getattr(m, 'scale_wh', 1.)

    def emit(name, n, arrays, *info):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        out.append((name, (h.hexdigest()[:16], [n] + list(info))))

    def emit_ys(name, n, xs):
        emit(name, n, xs, int(np.sum(xs[1] == 0)))

    def inputs(n, sy, scale_wh):
        rng = np.random.default_rng(1000 + n)
        u = rng.normal(size=(n, 6))
        su = u / np.linalg.norm(u, axis=1)[:, None]
        return dict(su=su, sig=su * (sy * rng.uniform(0.3, 2.0, size=n))[:, None], epl=rng.normal(size=(n, 6)) * 0.3 * scale_wh,
                    x0=sy * rng.uniform(0.5, 1.5, size=n), deps=rng.normal(size=(n, 6)) * 1e-3)

    def with_context(records, fn):
        ctx = _lib.Context(0)
        try:
            ctx.set_materials(records)
            for n in (67, 1025):
                fn(ctx, n)
        finally:
            ctx.close()

    # more doubles than the LDS of a CU holds (160 KiB = 20480): the tables of such a material are read from device memory
    past_lds = {'hill': 3200, 'workhard': 1400, 'hill3d': 7000}
    trained = {'hill': 1585, 'workhard': 1018, 'hill3d': 166}
    for name in ('hill', 'workhard', 'hill3d'):
        wh = name == 'workhard'
        for tag, kw in [('', {})] + [(' nsv %d' % k, dict(nsv=k)) for k in (1, 16, 17, 32, 33)] + \
                       [(' padded to %d' % past_lds[name], dict(pad=past_lds[name] - trained[name]))]:
            rec, sy, swh = record(name, **kw)
            assert rec[0].nsv == (kw.get('nsv') or past_lds[name] if kw else trained[name])
            assert 'pad' not in kw or rec[0].nsv * (rec[0].nfeat + 1) > 20480

            def fn(ctx, n):
                q = inputs(n, sy, swh)
                if name != 'hill3d':
                    emit('hessian %s%s' % (name, tag), n, [ctx.hessian(0, q['sig'], q['epl'] if wh else None)])
                emit_ys('yield_scale %s%s' % (name, tag), n, ctx.yield_scale(0, q['su'], q['epl'] if wh else None))
                emit_ys('yield_scale %s%s, x0' % (name, tag), n, ctx.yield_scale(0, q['su'], q['epl'] if wh else None, q['x0']))
            with_context([rec], fn)

    z = CC.load()
    members = [CC.member_params(z, k) for k in range(5)]

    for tag, cuts in (('', [None] * 5), (', members cut to nsv 1, 16, 17, 32, 33', [1, 16, 17, 32, 33])):
        mem = [CC.cut(p, k) for p, k in zip(members, cuts)]

        def fn(ctx, n):
            q = inputs(n, 1., 1.)
            r = ctx.committee_yf(list(range(5)), [0.5 * p['sy'] for p in mem], q['su'], True, True, True, True)
            emit('committee_yf yf, mean, var, best' + tag, n, [r['yf'], r['mean'], r['var'], np.array(r['best'])])
        with_context([CC.facade(p)._record(np.asarray(CC.facade(p).CV)) for p in mem], fn)

    hill, sy, _ = record('hill')
    wh, sy_wh, swh = record('workhard')
    CV = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_hill.npz'))['par_CV']
    hill6 = _lib.pack_material(_lib.HILL6, CV, E=200.e3, nu=0.3, sy=sy, khard=100., hill=[0.7, 1., 1.4, 1., 1.2, 0.8])
    princ3 = _lib.pack_material(_lib.PRINC3, CV, E=200.e3, nu=0.3, sy=sy, khard=100., hill=[0.7, 1., 1.4])

    def fn(ctx, n):
        q = inputs(n, sy, swh)
        ld = np.array([0.3, 1., -0.2, 0.1, 0., 0.4])
        for k, what in ((0, 'hill6'), (1, 'svc6'), (2, 'svc_wh')):
            emit('seq %s' % what, n, [ctx.seq(k, q['sig'])])
            emit('yf %s' % what, n, [ctx.yf(k, q['sig'], q['epl'])])
        emit('fgrad hill6', n, [ctx.fgrad(0, q['sig'])])
        emit('fgrad svc6', n, [ctx.fgrad(1, q['sig'])])
        emit('fgrad_seq hill6', n, [ctx.fgrad_seq(0, q['sig'], ctx.seq(0, q['sig']))])
        emit('fgrad_wh svc_wh', n, ctx.fgrad_wh(2, q['sig'], q['epl']))
        emit('full_yf svc6, ld', n, ctx.full_yf(1, q['sig'], q['epl'], ld))
        emit('full_yf svc_wh, ld', n, ctx.full_yf(2, q['sig'], q['epl'], ld))
        plane = q['su'] * np.array([1., 1., 1., 0., 0., 1.])   # the closed form of the principal stresses on the device
        emit_ys('yield_scale princ3 (analytic), plane and general states', n, ctx.yield_scale(3, np.vstack((plane, q['su']))))
        mid = np.arange(n, dtype=np.int32) % 3
        emit('response hill6 / svc6 / svc_wh', n, ctx.response(q['sig'], np.abs(q['epl']) * 0.01, q['deps'], mid, return_khard=True))
        os.environ['PLFX_RESPONSE_ROW'] = '0'   # (read by every call) the 6-feature SVC points in the thread kernel
        try:
            emit('response, PLFX_RESPONSE_ROW=0', n, ctx.response(q['sig'], np.abs(q['epl']) * 0.01, q['deps'], mid, return_khard=True))
        finally:
            del os.environ['PLFX_RESPONSE_ROW']
    with_context([hill6, hill, wh, princ3], fn)

    # the texture set of the context (tests/golden/texture_svc.npz): both descriptors as trained (NFP 12 and 16), cut to two
    # texture columns (NFP 8) and widened to ten, cut to the remainders of the trip loop, padded past the LDS, dev_only once
    import texture_cases as TC
    tz = TC.load()
    SY = 40.   # about where the fits change sign along a ray

    def tex_case(tag, p, tex):
        def fn(ctx, n):
            q = inputs(n, SY, 1.)
            emit('tex_svc_yf %s, shared texture' % tag, n, [ctx.tex_svc_yf(q['sig'], tex[:1])])
            emit('tex_svc_yf %s, one texture per point' % tag, n, [ctx.tex_svc_yf(q['sig'], tex[np.arange(n) % len(tex)])])
            emit('tex_svc_yf %s, tex_id' % tag, n, [ctx.tex_svc_yf(q['sig'], tex[:3], np.arange(n, dtype=np.int32) % 3)])
            for nt in (1, 3):
                x0 = np.ascontiguousarray(np.tile(q['x0'], (nt, 1)) * (1. + 0.1 * np.arange(nt))[:, None])
                emit_ys('tex_svc_yield_scale %s, ntex %d, x0' % (tag, nt), n, ctx.tex_svc_yield_scale(q['su'], tex[:nt], x0))

        def fn_unit(ctx, n):
            q = inputs(n, 1., 1.)
            for nt in (1, 3):
                emit_ys('tex_svc_yield_scale %s, ntex %d' % (tag, nt), n, ctx.tex_svc_yield_scale(q['su'], tex[:nt]))
        ctx = _lib.Context(0)
        try:
            # without x0 the search starts at a J2 stress of one stress unit: these rays run on the set with its stress columns
            # in units of SY (a second call replaces the set)
            unit = np.concatenate((np.full(6, SY), np.ones(p['tdim'])))
            ctx.tex_svc_set(p['sv'], p['dual'], p['intercept'], p['gamma'], p['mean'] / unit, p['scale'] / unit, dev_only=p['dev_only'])
            for n in (67, 1025):
                fn_unit(ctx, n)
            ctx.tex_svc_set(p['sv'], p['dual'], p['intercept'], p['gamma'], p['mean'], p['scale'], dev_only=p['dev_only'])
            info = ctx.tex_svc_info()
            assert info['nsv'] == len(p['sv']) and info['tdim'] == p['tdim']
            nfp = 8 if p['tdim'] <= 2 else 12 if p['tdim'] <= 6 else 16
            assert info['staged'] == ('padded' not in tag) and (info['staged'] or len(p['sv']) * (nfp + 3) > 20480)
            for n in (67, 1025):
                fn(ctx, n)
        finally:
            ctx.close()

    for desc in TC.DESCRIPTORS:
        full, tex = TC.tables(tz, desc), TC.textures(tz, desc)
        tex_case(desc, full, tex)
        for k in (1, 16, 17, 32, 33):
            p = TC.cut(full, nsv=k)
            tex_case('%s nsv %d' % (desc, k), TC.cut(p, intercept=TC.crossing_intercept(p, tex[0])), tex)
    tex_case('GSH_7 dev_only', TC.tables(tz, 'GSH_7', dev=True), TC.textures(tz, 'GSH_7'))
    p, tex = TC.tables(tz, 'GSH_3'), TC.textures(tz, 'GSH_3')
    tex_case('GSH_3 cut to tdim 2', TC.cut(p, tdim=2), tex[:, :2])
    tex_case('GSH_7 widened to tdim 10', *TC.widen(TC.tables(tz, 'GSH_7'), TC.textures(tz, 'GSH_7'), 10))
    tex_case('GSH_3 padded to 1500', TC.cut(p, pad=1500 - len(p['sv'])), tex)   # 1500 (12 + 3) doubles > 20480: device memory


def child(more, pts=False):
    sys.path.insert(0, ROOT)
    import numpy as np
    import pylabfea_amd as FE

    def digest(fe):
        h = hashlib.sha256()
        for a in (fe.u, fe._state('sig'), fe._state('epl'), np.asarray(fe.sgl), np.asarray(fe.egl)):
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return h.hexdigest()[:16], [q[0] for q in fe.solver_stats]

    def hill(num=1, sy=100.):
        m = FE.Material(num=num)
        m.elasticity(E=200.e3, nu=0.3)
        m.plasticity(sy=sy, hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=100., sdim=6)
        return m

    def finish(fe, nx, ny, steps, min_step):
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(0.004 * fe.leny, 'disp')
        fe.mesh(NX=nx, NY=ny)
        fe._max_load_steps = steps
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fe.solve(min_step=min_step)
        return digest(fe)

    def svc(name, num=1):
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_%s.npz' % name))
        m = FE.Material(name='ML-' + name, num=num)
        m.elasticity(CV=z['par_CV'])
        m.plasticity(sy=float(z['par_sy']), sdim=int(z['par_sdim']))
        m.set_svc(z['par_sv'], z['par_dual'], float(z['par_intercept']), float(z['par_gamma']),
                  float(z['par_scale_seq']), dev_only=bool(z['par_dev_only']))
        return m

    def solve_tension(fe, eps, min_step):
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(eps * fe.leny, 'disp')
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fe.solve(min_step=min_step)
        return digest(fe)

    def gmres_case():
        # three element tangents with negative eigenvalues (one of config 5's, tests/test_gpu_random.py): PCG gives up, GMRES
        # with the V-cycle of the indefinite operator finishes the solve
        from pylabfea_amd import _lib
        t = [3.06119e+05, 2.30987e+05, 2.44365e+05, -7.10713e+02, 8.16221e+02, -3.89722e+01, -5.30574e+05, -2.01886e+05,
             8.08981e+02, -9.29004e+02, 4.43106e+01, 2.03386e+05, -4.23220e+01, 4.86228e+01, -2.33304e+00, 5.81516e+04,
             1.14637e+01, -5.47451e-01, 5.81484e+04, 6.34734e-01, 5.81615e+04]
        nx = ny = 64
        mat = FE.Material()
        mat.elasticity(E=151220., nu=0.3)
        fe = FE.Model(dim=2, planestress=False)
        fe.geom([4.], LY=4.)
        fe.assign([mat])
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(0.002 * fe.leny, 'disp')
        fe.mesh(NX=nx, NY=ny)
        eng = fe._ensure_engine()
        D = np.tile(fe._element_CV(mat), (fe.Nel, 1, 1))
        bad = np.zeros((6, 6))
        bad[np.triu_indices(6)] = t
        bad = bad + bad.T - np.diag(np.diag(bad))
        for cx, cy in ((nx // 3, ny // 2), (2 * nx // 3, ny // 4), (nx // 2, (3 * ny) // 4)):
            D[cx * ny + cy] = bad
        eng.state_set(_lib.ST_ELSTIFF, D.reshape(fe.Nel, 36))
        eng.assemble()
        z, d = np.zeros(2), np.array([0., 0.002 * fe.leny])
        eng.apply_bc(*fe._bc_data(z, z, z, d, None))
        it, rr, ok = eng.solve(1e-10, 20000, False)
        assert ok and eng.indefinite_info()['by_gmres'] == 1
        h = hashlib.sha256(np.ascontiguousarray(eng.state_get(_lib.ST_DU), dtype=np.float64).tobytes()).hexdigest()[:16]
        return h, [it]

    out = []
    fe = FE.Model(dim=2, planestress=False)   # three sections, the middle one soft: heterogeneous tangents
    fe.geom([2, 1, 2], LY=5.)
    fe.assign([hill(1), hill(2, 40.), hill(1)])
    out.append(('sections 320x256', finish(fe, 320, 256, 8, 12)))
    fe = FE.Model(dim=2, planestress=False)
    fe.geom([4.], LY=4. * 199 / 201)
    fe.assign([hill()])
    out.append(('odd 201x199', finish(fe, 201, 199, 5, 6)))
    ma, mb = hill(1, 150.), hill(2, 90.)
    fe = FE.Model(dim=2, planestress=True)
    fe.geom([3, 1, 2, 1, 2], LY=9. * 256 / 320)
    fe.assign([ma, mb, ma, mb, ma])
    out.append(('laminate 320x256', finish(fe, 320, 256, 6, 20)))
    if more:
        fe = FE.Model(dim=2, planestress=False)   # config 4's schedule: the SVC corrector on every element of the last step
        fe.geom([4.], LY=4.)
        fe.assign([svc('hill')])
        fe.mesh(NX=32, NY=32)
        d = solve_tension(fe, 0.001, 10)
        assert fe._engine.svc_info()[0] == 1 and int(np.max(fe._state('max_steps'))) == 49
        out.append(('svc6 32x32', d))
        ma = FE.Material(num=1)
        ma.elasticity(E=200.e3, nu=0.3)
        ma.plasticity(sy=150., khard=500., sdim=6)
        fe = FE.Model(dim=2, planestress=False)   # config 5's laminate: J2 and the SVC trained on Barlat / Goss
        fe.geom([2, 1, 2, 1, 2], LY=8.)
        mb = svc('gossbarlat', 2)
        fe.assign([ma, mb, ma, mb, ma])
        fe.mesh(NX=128, NY=64)
        out.append(('config 5 laminate 128x64', solve_tension(fe, 0.003, 20)))
        out.append(('indefinite K 64x64, GMRES', gmres_case()))
        os.environ['PLFX_MG_MAXIT'] = '2'   # (read by every solve) multigrid-PCG gives up after two iterations: Jacobi-PCG finishes
        fe = FE.Model(dim=2, planestress=False)
        fe.geom([4.], LY=4.)
        fe.assign([hill()])
        try:
            d = finish(fe, 32, 32, 4, 6)
        finally:
            del os.environ['PLFX_MG_MAXIT']
        assert fe._engine.precond_info()[0] == 1 and fe._engine.precond_info()[1] >= 2   # multigrid-PCG is what gave up
        assert fe._engine.solve_fallbacks() > 0 and fe._engine.indefinite_info()['by_gmres'] == 0   # ... Jacobi, not GMRES
        out.append(('32x32, multigrid capped at 2: Jacobi fall-back', d))
    if pts:
        points(out)
    for name, (d, its) in out:
        print('%s|%s|%s' % (name, d, ','.join(map(str, its))))


if __name__ == '__main__':
    flags = [a for a in ('--more', '--points') if a in sys.argv]
    args = [a for a in sys.argv[1:] if a not in flags]
    if args == ['--child']:
        child('--more' in flags, '--points' in flags)
        sys.exit(0)
    res = []
    for lib in args[:2]:
        env = dict(os.environ, PLFX_LIB=os.path.abspath(lib))
        o = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + flags, env=env,
                           capture_output=True, text=True)
        if o.returncode:
            print(o.stdout, o.stderr)
            sys.exit(1)
        res.append([l for l in o.stdout.splitlines() if l.count('|') == 2])
    bad = 0
    for a, b in zip(*res):
        same = a == b
        bad += not same
        print(('identical  ' if same else 'DIFFERENT  ') + a + ('' if same else '\n           ' + b))
    sys.exit(1 if bad or not res[0] or len(res[0]) != len(res[1]) else 0)

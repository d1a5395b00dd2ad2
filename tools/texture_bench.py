#!/usr/bin/env python3
"""GPU time of Material.texture_loci (k_tex_yield_scale: T textures x 72 pi-plane rays searched in one launch) beside the same
loci as one yield_scale call per texture -- the loop of the reference's examples/Texture/train_texture.py, which solves one
coupled fsolve over Python calc_yf calls per texture -- and of calc_yf(tex=) (k_tex_yf) at 1 and 100 000 points.
Material: the GSH_3 fit of tests/golden/texture_svc.npz (522 support vectors, 9 features); T = 6, 100 and 7000 textures, the
fixture's six resampled (convex mixtures of two of them, fixed seed).  Kernel time from the library's HIP events on its
stream (timing family 0, plfx_timing_get): one warm-up call, then the median of --reps calls; wall time of the whole call
beside it.  Every step runs in a child process of its own under its own time limit, and nothing more is started after one
that fails.  One JSON line per step.

    python tools/texture_bench.py [--reps 11] [--limit 240]
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
DESC = 'GSH_3'


def step(name, reps):
    import texture_cases as TC
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    from pylabfea_amd.material import _ctx
    kind, n = name.split(':')
    n = int(n)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--limit', type=int, default=240, help='time limit of one step in seconds')
    ap.add_argument('--step', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps)
    if a.reps < 10:
        ap.error('--reps must be at least 10 (median of >= 10 launches)')
    for name in STEPS:   # a fresh child per step, each under its own limit; stop at the first that fails
        rc = subprocess.call(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__),
                              '--step', name, '--reps', str(a.reps)])
        if rc != 0:
            print('step %s ended with status %d; nothing more is started' % (name, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())

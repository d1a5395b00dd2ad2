#!/usr/bin/env python3
"""GPU time of Material.calc_hessian (k_hessian_row) beside calc_fgrad (k_point_eval) on N points of the config-4 material
(the trained SVC of tests/golden/svc_hill.npz, 1585 support vectors, 6 features): the kernels alone, from the library's HIP
events on its stream (timing family 0, plfx_timing_get), one warm-up call first, then the median of --reps calls.  The FP64
rate counts, per (point, support vector) pair, what the kernels execute: distance 6 sub + 6 FMA, exponent scaling 1, exp2
(11 FMA + 4 single operations; its integer operations are not counted), weight 1, then 33 for the Hessian (6 FMA
d^2 - 1/(2 gamma), 6 products w d_a, 21 FMA into the accumulators) or 6 FMA for the gradient; an FMA counts as two flops.
With --wh the same for the 15-feature work-hardening material of svc_workhard.npz (distance 12 sub + 15 FMA, 12 FMA for
its gradient).  Prints one JSON line.

    timeout -k 10 300 python tools/hessian_bench.py [--n 100000] [--reps 11] [--wh]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--wh', action='store_true')
    a = ap.parse_args()
    if a.reps < 10:
        ap.error('--reps must be at least 10 (median of >= 10 launches)')
    import pylabfea_amd as FE
    from pylabfea_amd import _lib
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'svc_workhard.npz' if a.wh else 'svc_hill.npz'))
    m = FE.Material(name='ML')
    m.elasticity(CV=z['par_CV'])
    m.plasticity(sy=float(z['par_sy']), sdim=6)
    m.set_svc(z['par_sv'], z['par_dual'], float(z['par_intercept']), float(z['par_gamma']), float(z['par_scale_seq']),
              dev_only=bool(z['par_dev_only']), scale_wh=float(z['par_scale_wh']) if a.wh else None)
    rng = np.random.default_rng(0)
    u = rng.normal(size=(a.n, 6))
    sig = u / np.linalg.norm(u, axis=1)[:, None] * (m.sy * rng.uniform(0.3, 2.0, size=a.n))[:, None]
    epl = rng.normal(size=(a.n, 6)) * 0.3 * m.scale_wh if a.wh else None
    ctx = m._load()
    name, cus, _ = ctx.device_info()
    ctx.timing_enable(True)
    ctx.timing_select([_lib.T_SWEEP])

    def timed(call):
        call()                                   # warm-up: code object load, allocations
        ms = []
        for _ in range(a.reps):
            ctx.timing_reset()
            call()
            t, launches = ctx.timing_get(_lib.T_SWEEP)
            assert launches == 1
            ms.append(t)
        return float(np.median(ms)), ms

    t_h, all_h = timed(lambda: ctx.hessian(0, sig, epl))
    t_g, all_g = timed((lambda: ctx.fgrad_wh(0, sig, epl)) if a.wh else (lambda: ctx.fgrad(0, sig)))
    ctx.timing_enable(False)
    nsv, nf = z['par_sv'].shape
    pairs = float(a.n) * nsv
    dist = (12 + 2 * 15) if a.wh else (6 + 2 * 6)
    fl_h = dist + 1 + (2 * 11 + 4) + 1 + (2 * 6 + 6 + 2 * 21)
    fl_g = dist + 1 + (2 * 11 + 4) + 1 + (2 * 12 if a.wh else 2 * 6)
    res = dict(device=name, cus=cus, n=a.n, nsv=int(nsv), nfeat=int(nf), reps=a.reps,
               hessian_us_per_point=1e3 * t_h / a.n, fgrad_us_per_point=1e3 * t_g / a.n, hessian_over_fgrad=t_h / t_g,
               hessian_ms=t_h, fgrad_ms=t_g, hessian_ms_min_max=[min(all_h), max(all_h)], fgrad_ms_min_max=[min(all_g), max(all_g)],
               flops_per_pair=dict(hessian=fl_h, fgrad=fl_g),
               hessian_fp64_tflops=pairs * fl_h / (t_h * 1e-3) / 1e12, fgrad_fp64_tflops=pairs * fl_g / (t_g * 1e-3) / 1e12)
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())

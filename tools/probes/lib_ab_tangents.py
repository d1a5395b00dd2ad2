#!/usr/bin/env python3
"""Two builds of libplfx.so compared BIT FOR BIT on the paths of the element tangent store that the three
cases of lib_ab.py do not reach: elements on the 50-sub-step corrector and the averaged tangent of K-iteration >= 15.

    python tools/probes/lib_ab_tangents.py pylabfea_amd/libplfx_prev.so pylabfea_amd/libplfx.so

Cases: (1) a three-section model with an elastic middle section and two Hill sections loaded in large increments (most plastic
elements go through the corrector on some sweep; at 20 x 20 and eps 0.03 the last load step takes 15 K-iterations on the CPU
oracle, i.e. one sweep at nit = 15); (2) the 160 x 160 model of (1), then engine sweeps at K-iteration 15 and 16 with its
tangents offset by state_set (every plastic element takes the averaged tangent).  Digest of u, sig, epl, sgl, egl and the expanded
tangents; per case the elements whose final tangent is the elastic CV, whose largest sub-step count is 49, and the rest."""
import hashlib
import os
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import pylabfea_amd as FE
    from pylabfea_amd import _lib

    def hill(num=1, sy=100.):
        m = FE.Material(num=num)
        m.elasticity(E=200.e3, nu=0.3)
        m.plasticity(sy=sy, hill=[0.7, 1., 1.4, 1., 1.2, 0.8], khard=100., sdim=6)
        return m

    def model(n, eps):
        el = FE.Material(num=3)
        el.elasticity(E=50.e3, nu=0.25)
        fe = FE.Model(dim=2, planestress=False)
        fe.geom([2, 1, 2], LY=5.)
        fe.assign([hill(1), el, hill(2, 60.)])
        fe.bcleft(0.)
        fe.bcbot(0.)
        fe.bcright(0., 'force')
        fe.bctop(eps * fe.leny, 'disp')
        fe.mesh(NX=n, NY=n)
        return fe

    def forms(eng, fe):
        D = eng.state_get(_lib.ST_ELSTIFF).reshape(-1, 36)
        ms = eng.state_get(_lib.ST_MAXSTEPS)
        cv = np.stack([fe._element_CV(fe.mat[k]).reshape(36) for k in range(len(fe.mat))])
        is_cv = np.all(D == cv[np.asarray(fe._mat_id)], axis=1)
        is_cor = (ms >= 49) & ~is_cv
        n_cv, n_cor = int(is_cv.sum()), int(is_cor.sum())
        return D, 'cv=%d corrector=%d other=%d' % (n_cv, n_cor, len(D) - n_cv - n_cor)

    def digest(fe, extra=()):
        h = hashlib.sha256()
        for a in (fe.u, fe._state('sig'), fe._state('epl'), np.asarray(fe.sgl), np.asarray(fe.egl)) + tuple(extra):
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return h.hexdigest()[:16]

    for n, eps in ((20, 0.03), (160, 0.01)):
        fe = model(n, eps)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fe.solve(min_step=2)
        eng = fe._ensure_engine()
        D, cnt = forms(eng, fe)
        print('corrector %dx%d eps %g|%s|%s' % (n, n, eps, digest(fe, (D,)), ','.join(map(str, fe.niter)) + ' ' + cnt))
    # K-iteration >= 15: every stored tangent offset by 1e-2 in one entry pair, then sweeps at nit = 15 (averaged tangents)
    D2 = D.copy().reshape(-1, 6, 6)
    D2[:, 0, 1] += 1.e-2
    D2[:, 1, 0] += 1.e-2
    eng.state_set(_lib.ST_ELSTIFF, D2.reshape(-1, 36))
    ch = []
    for nit in (15, 16):
        ch.append(int(eng.sweep(nit)[0]))
    D3 = eng.state_get(_lib.ST_ELSTIFF)
    h = hashlib.sha256()
    for k in (_lib.ST_RES_SIG, _lib.ST_RES_DEPL, _lib.ST_FYN):
        h.update(np.ascontiguousarray(eng.state_get(k)).tobytes())
    h.update(np.ascontiguousarray(D3).tobytes())
    print('averaged nit 15|%s|%s' % (h.hexdigest()[:16], ','.join(map(str, ch)) + ' rewritten=%d' % eng.sweep_info()[1]))


if __name__ == '__main__':
    if len(sys.argv) == 2 and sys.argv[1] == '--child':
        child()
        sys.exit(0)
    res = []
    for lib in sys.argv[1:3]:
        env = dict(os.environ, PLFX_LIB=os.path.abspath(lib))
        o = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, capture_output=True, text=True)
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

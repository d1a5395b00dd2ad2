#!/usr/bin/env python3
"""Fixture generator for Model.field / fields / field_range -- TEST INFRASTRUCTURE, not product code.

Runs the unmodified reference (pyLabFEA v4.4.2) on the build box and writes ``tests/golden/model_fields.npz``.  No test
reads the reference; they read this file.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_model_fields.py

Cases (at most 64 elements each; ``tests/model_fields_cases.py`` builds the same models through the façade):
  a  5 x 3 laminate geom([2, 1, 2], LY=3): Hill-6 (sdim 6) | J2 with sdim 3 | elastic, tension bctop(0.004 leny)
  b  7 x 6 model with an ``elmts`` map: a softer Hill inclusion and one Drucker material in a J2 matrix; the top edge is
     displaced in y and in x, so the 12 components and ux / uy vary over the mesh
  c  case a before any solve: all fields zero
  d  a purely elastic two-material laminate (nonlin false: sig is written by the linear path)

Keys per case ``<c>``:
  <c>_u (Ndof,), <c>_sig, <c>_eps, <c>_epl (Nel, 6)   the model's state
  <c>_nsteps                                          load steps of the solve (0: not solved)
  <c>_f_<selector> (Nel,)      the sixteen field vectors, computed with the reference's own Stress, eps_eq and Material objects
                               as the closures of Model.plot do (model.py:1591-1677)
  <c>_r_<selector> (2,)        (vmin, vmax) of the colour bar of fe.plot(selector, showfig=False): get_ylim() of the last axes
  <c>_branch_<selector>        auto-scale branch plot took: 0 none, 1 +-0.05, 2 positive (x 1.02 / 0.98), 3 negative
``selectors``: the sixteen names in the order of the reference's dictionary.
"""
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden', 'model_fields.npz')
os.environ.setdefault('MPLBACKEND', 'Agg')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import matplotlib.pyplot as plt  # noqa: E402

import pylabfea as FE  # noqa: E402  (the reference)
from pylabfea.basic import Stress, eps_eq  # noqa: E402

import model_fields_cases as cases  # noqa: E402  (the model definitions the tests rebuild through the façade)

SELECTORS = ('strain1', 'strain2', 'strain12', 'stress1', 'stress2', 'stress12', 'plastic1', 'plastic2', 'plastic12',
             'seq', 'seqJ2', 'peeq', 'etot', 'ux', 'uy', 'mat')
BRANCH = ('none', '+-0.05', 'positive', 'negative')


def field_values(fe):
    """the closures of Model.plot (model.py:1591-1677), word for word on the reference's objects"""
    el = fe.element
    f = {
        'strain1': [e.eps[0] * 100 for e in el], 'strain2': [e.eps[1] * 100 for e in el], 'strain12': [e.eps[5] * 100 for e in el],
        'stress1': [e.sig[0] for e in el], 'stress2': [e.sig[1] for e in el], 'stress12': [e.sig[5] for e in el],
        'plastic1': [e.epl[0] * 100 for e in el], 'plastic2': [e.epl[1] * 100 for e in el],
        'plastic12': [e.epl[5] * 100 for e in el],
        'seq': [Stress(e.sig).seq(e.Mat) for e in el], 'seqJ2': [Stress(e.sig).seq_j2() for e in el],
        'peeq': [eps_eq(e.epl) * 100 for e in el], 'etot': [eps_eq(e.eps) * 100 for e in el],
        'mat': [e.Mat.num for e in el],
    }
    u = fe.u if fe.u is not None else np.zeros(fe.Ndof)
    for k, name in enumerate(('ux', 'uy')):
        hh = np.zeros(fe.Nel)
        for ie, e in enumerate(el):
            fac = 1.0 / len(e.nodes)
            for nn in e.nodes:
                hh[ie] += u[nn * fe.dim + k] * fac
        f[name] = hh
    return {k: np.asarray(v, dtype=np.float64) for k, v in f.items()}


def branch_of(val):
    """which branch of model.py:1700-1716 an automatic range of these values takes"""
    vmin, vmax = np.amin(val), np.amax(val)
    delta = np.abs(vmax - vmin)
    with np.errstate(divide='ignore', invalid='ignore'):
        if not (delta < 0.1 or delta / vmax < 0.04):
            return 0
    return 1 if np.abs(vmax) < 0.1 else (2 if vmax > 0. else 3)


def colour_bar(fe, fsel):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fig, _ = fe.plot(fsel, showfig=False)
    lim = fig.axes[-1].get_ylim()
    plt.close(fig)
    return np.array(lim, dtype=np.float64)


def main():
    out = {'selectors': np.array(SELECTORS)}
    seen = set()
    for name in cases.CASES:
        t0 = time.time()
        fe = cases.build(FE, name)
        nsteps = 0
        if cases.CASES[name]['solve']:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                fe.solve()
            nsteps = int(fe.nsteps)
        else:
            fe.u = np.zeros(fe.Ndof)   # plot's ux / uy closures index u: the zero state of a model that was not solved
        dt = time.time() - t0
        assert fe.Nel <= 64
        out[name + '_u'] = np.array(fe.u, dtype=np.float64)
        for q in ('sig', 'eps', 'epl'):
            out['%s_%s' % (name, q)] = np.array([getattr(e, q) for e in fe.element], dtype=np.float64)
        out[name + '_nsteps'] = np.int64(nsteps)
        fv = field_values(fe)
        line = []
        for s in SELECTORS:
            out['%s_f_%s' % (name, s)] = fv[s]
            out['%s_r_%s' % (name, s)] = colour_bar(fe, s)
            b = branch_of(fv[s])
            out['%s_branch_%s' % (name, s)] = np.int64(b)
            seen.add(b)
            line.append('%s:%s' % (s, BRANCH[b]))
        print('case %s: %d elements, %d load steps, %.1f s (reference solve)' % (name, fe.Nel, nsteps, dt))
        print('   auto-scale branch per selector: ' + ', '.join(line))
    assert seen == {0, 1, 2, 3}, 'an auto-scale branch does not occur: %s' % sorted(seen)
    print('every auto-scale branch (none, +-0.05, positive, negative) occurs in the fixture')
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()

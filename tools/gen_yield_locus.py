#!/usr/bin/env python3
"""Golden-vector generator for Material.yield_scale / polar_yield_locus / polar_field / yield_slices / ellipsis (TEST
INFRASTRUCTURE, development machine only): runs the unmodified reference and writes tests/golden/yield_locus.npz.

    MPLBACKEND=Agg PYTHONPATH=oracle/_refshim:<reference>/src python tools/gen_yield_locus.py

Materials: the SVC tables of svc_hill.npz (also with dev_only), svc_hill3d.npz and svc_workhard.npz behind a stand-in for the
scikit-learn estimator (support_vectors_, dual_coef_, decision_function, predict), and analytic Hill-6, Hill-3 / J2 principal,
Tresca and Barlat materials with khard > 0 (tests/yield_locus_cases.py).  Everything evaluated is the reference's code.

Rays per material: load_cases(20, 40) (the 20 principal ones for sdim = 3), the polar snorm of polar_plot_yl for Na = 72 (start
value 1, as there), the in-plane rays of two slices; the work-hardening table at three plastic strains, the analytic
materials at two.  Per ray
    x_ref     the marched bracket of ML_full_yf made symmetric (from x0 down by 0.98 while f >= 0 to 0.01 x0, else up by 1.02
              while f < 0 to 5 x0) on the reference's find_yloc_scalar, then brentq(xtol = 1e-15, rtol = 4 eps)
    x_fsolve  the reference's own coupled fsolve (polar_plot_yl :3292) where it is meaningful (not the work-hardening table)
and per case r_ref: the reference's worst |calc_yf - longdouble restatement| at the roots in units of A 2^-53.  No ray may
lack a bracket (asserted).  Also: the curves polar_plot_yl draws (read from the returned axes), the symmetrised slice fields
Z at Nmesh = 21 (read from the image plot_data draws), ellipsis(), and the field of polar_plot_yl(field=True) at Np = 9."""
import os
import sys
import warnings

import numpy as np
from scipy.optimize import brentq, fsolve

import pylabfea as FE  # the reference
from pylabfea.training import load_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import yield_locus_cases as YC  # noqa: E402


class SvmStub(object):
    def __init__(self, sv, dual, intercept, gamma):
        self.support_vectors_, self.dual_coef_, self.b, self.g = sv, dual[None, :], intercept, gamma

    def decision_function(self, x):
        x = np.asarray(x, dtype=float)
        return np.array([np.sum(self.dual_coef_[0] * np.exp(-self.g * np.sum((self.support_vectors_ - r) ** 2, axis=1)))
                         for r in x]) + self.b

    def predict(self, x):
        return np.where(self.decision_function(x) > 0., 1., -1.)


def ref_ml(tag):
    p = YC.ml_params(tag)
    m = FE.Material(name=tag)
    m.elasticity(E=p['E'], nu=p['nu'])
    m.plasticity(sy=p['sy'], hill=list(p['hill']), sdim=p['sdim'])
    m.svm_yf = SvmStub(p['sv'], p['dual'], p['intercept'], p['gamma'])
    m.gam_yf, m.scale_seq, m.dev_only = p['gamma'], p['scale_seq'], p['dev_only']
    m.ML_yf, m.ML_grad, m.Ndof = True, False, p['Ndof']
    if p['Ndof'] == 15:
        m.whdat, m.ind_wh, m.scale_wh = True, p['ind_wh'], p['scale_wh']
    return m, p


def marched_root(m, su, epl, x0):
    """(x_ref, status) of one ray on the reference's find_yloc_scalar"""
    f = lambda x: float(m.find_yloc_scalar(x, su, epl=epl))   # noqa: E731
    x, fx = x0, f(x0)
    if fx >= 0.:
        hi = x
        while fx >= 0.:
            if x < 0.01 * x0:
                return np.nan, 1
            hi = x
            x *= 0.98
            fx = f(x)
        lo = x
    else:
        lo = x
        while fx < 0.:
            if x > 5. * x0:
                return np.nan, 1
            lo = x
            x *= 1.02
            fx = f(x)
        hi = x
    return brentq(f, lo, hi, xtol=1e-15, rtol=4 * np.finfo(float).eps), 0


def slice_stress(c1, c2, xa, ya):
    s = np.zeros((len(xa), 3))
    for k in ((0, 1) if c1 == 3 else (c1,)):
        s[:, k] = xa
    s[:, 2 if c2 == 3 else c2] = ya
    return s


def rays(m, sdim):
    """list of (group, su (N,sdim), x0 or None)"""
    lc = load_cases(20, 40)
    lc = lc[:20, :3] if sdim == 3 else lc
    theta = np.linspace(0., 2. * np.pi, YC.NA_POLAR)
    snorm = FE.sig_cyl2princ(np.array([m.sy * np.ones(YC.NA_POLAR) * np.sqrt(1.5), theta]).T)
    out = [('lc', lc, None), ('polar', snorm, 1.)]
    phi = np.linspace(0., 2. * np.pi, YC.NA_SLICE)
    for j, (c1, c2) in enumerate(YC.SLICES):
        su = slice_stress(c1, c2, np.cos(phi), np.sin(phi)) * m.sy
        ok = YC.j2(su) > 1e-9 * m.sy          # hydrostatic in-plane rays of code 3 have no locus: kept out of the root table
        out.append(('slice%d' % j, su[ok], None))
    return out


def pad6(su):
    return np.c_[su, np.zeros((len(su), 6 - su.shape[1]))]


def main():
    rec = {}
    plt = __import__('matplotlib.pyplot').pyplot
    mats = {}
    for tag in list(YC.ML_CASES) + list(YC.ANA_CASES):
        if tag in YC.ML_CASES:
            m, p = ref_ml(tag)
            epls = YC.WH_EPL if tag == 'wh' else (None,)
        else:
            m, p = YC.analytic(FE, tag), None
            epls = YC.ANA_EPL
        mats[tag] = m
        SU, EP, X0, XR, XF, GR = [], [], [], [], [], []
        for ie, epl in enumerate(epls):
            e6 = np.zeros(6) if epl is None else epl
            for grp, su, x0 in rays(m, m.sdim):
                xr = np.empty(len(su))
                for k in range(len(su)):
                    start = x0 if x0 is not None else float(m.get_sflow(e6)) / YC.j2(su[k:k + 1])[0]
                    xr[k], st = marched_root(m, su[k], None if epl is None else epl[:m.sdim] if m.sdim == 3 else epl, start)
                    assert st == 0, 'fixture ray without a reference bracket: %s %s %d' % (tag, grp, k)
                xf = np.full(len(su), np.nan)
                if tag != 'wh':   # the coupled fsolve diverges on the work-hardening table
                    ee = None if epl is None else (epl[:3] if m.sdim == 3 else epl)
                    x1 = fsolve(lambda x: m.find_yloc(x, su, epl=ee), np.ones(len(su)) if x0 is not None else xr * 1.01,
                                xtol=1.e-5)
                    xf = x1
                SU.append(pad6(su)), EP.append(np.tile(e6, (len(su), 1))), XR.append(xr), XF.append(xf)
                X0.append(np.full(len(su), np.nan if x0 is None else x0))
                GR += ['%s/%d' % (grp, ie)] * len(su)
        su, ep, x0, xr, xf = (np.concatenate(a) for a in (SU, EP, X0, XR, XF))
        rec[tag + '_su'], rec[tag + '_epl'], rec[tag + '_x0'], rec[tag + '_x_ref'], rec[tag + '_x_fsolve'] = su, ep, x0, xr, xf
        rec[tag + '_group'] = np.array(GR)
        rec[tag + '_status'] = np.zeros(len(su), dtype=np.int32)
        if p is not None:
            sd = m.sdim
            fr = np.array([float(m.find_yloc_scalar(xr[k], su[k, :sd], epl=ep[k] if tag == 'wh' else None))
                           for k in range(len(su))])
            fl, dfl, A = YC.restate(p, su, ep, xr)
            r_ref = float(np.max(np.abs(fr.astype(YC.LD) - fl) / (A * YC.EPS53)))
            rec[tag + '_r_ref'] = np.array(r_ref)
            U = 4 * max(r_ref, 1.)
            worst = float(np.max(np.abs(fl) / YC.residual_bar(U, dfl, A, xr)))
            okf = np.isfinite(xf)
            print('%-8s %4d rays, r_ref = %.2f, |f_L(x_ref)| / bar <= %.3f, max |x_fsolve - x_ref| / x = %.2e'
                  % (tag, len(su), r_ref, worst, np.max(np.abs(xf - xr)[okf] / xr[okf]) if np.any(okf) else np.nan))
        else:
            print('%-8s %4d rays (analytic)' % (tag, len(su)))

    # the curves polar_plot_yl draws, read from the returned axes
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tag, cm in (('hill', ['ahill6', 'hilldev']), ('hill3d', ['aj2p']), ('ahill6', ['hill'])):
            ax = mats[tag].polar_plot_yl(Na=YC.NA_POLAR, cmat=[mats[t] for t in cm], show=False)
            lines = ax.get_lines()
            assert len(lines) == 1 + len(cm)
            rec[tag + '_polar_theta'] = np.array(lines[0].get_xdata(), dtype=float)
            rec[tag + '_polar_syld'] = np.array([np.array(l.get_ydata(), dtype=float) for l in lines])
            rec[tag + '_polar_cmat'] = np.array(cm)
            plt.close('all')
            # per curve, along THIS material's snorm: the fsolve the reference ran (reproduced: it gives the drawn curve to
            # the bit) and the marched root from the same start value 1
            m = mats[tag]
            theta = np.linspace(0., 2. * np.pi, YC.NA_POLAR)
            snorm = FE.sig_cyl2princ(np.array([m.sy * np.ones(YC.NA_POLAR) * np.sqrt(1.5), theta]).T)
            xf, xr = [], []
            for c, mt in enumerate([m] + [mats[t] for t in cm]):
                x1 = fsolve(mt.find_yloc, np.ones(YC.NA_POLAR), args=snorm, xtol=1.e-5)
                assert np.array_equal(m.calc_seq(snorm * x1[:, None]), rec[tag + '_polar_syld'][c])
                xf.append(x1)
                rr = [marched_root(mt, s, None, 1.) for s in snorm]
                assert all(st == 0 for _, st in rr)
                xr.append(np.array([r for r, _ in rr]))
            rec[tag + '_polar_snorm'] = snorm
            rec[tag + '_polar_x_fsolve'], rec[tag + '_polar_x_ref'] = np.array(xf), np.array(xr)
            print('%-8s polar curves: max |x_fsolve - x_ref| / x per curve' % tag,
                  ['%.1e' % v for v in np.max(np.abs(np.array(xf) - np.array(xr)) / np.array(xr), axis=1)])
        # the field polar_plot_yl(field=True) draws (2-feature material): the QuadMesh behind the curve
        ax = mats['hill3d'].polar_plot_yl(Na=YC.NA_POLAR, field=True, Np=YC.NP_FIELD, show=False)
        qm = ax.collections[0]
        rec['hill3d_field_Z'] = np.array(qm.get_array(), dtype=float).reshape(YC.NP_FIELD, YC.NP_FIELD)
        plt.close('all')
        ax = mats['hill3d'].polar_plot_yl(Na=YC.NA_POLAR, field=True, predict=True, Np=YC.NP_FIELD, show=False)
        rec['hill3d_field_Zpred'] = np.array(ax.collections[0].get_array(), dtype=float).reshape(YC.NP_FIELD, YC.NP_FIELD)
        plt.close('all')

    # slice fields: calc_yf(pred=True) on the mesh through plot_data's symmetrisation, read from the image it draws
    for tag, peeq in (('hill', 0.), ('hill3d', 0.), ('wh', 0.002), ('ahill6', 0.002), ('abarlat', 0.)):
        m = mats[tag]
        xx, yy = np.meshgrid(np.linspace(-2., 2., YC.NMESH), np.linspace(-2., 2., YC.NMESH))
        for j, (c1, c2) in enumerate(YC.SLICES):
            sig = slice_stress(c1, c2, xx.ravel(), yy.ravel()) * m.sy
            Z = m.calc_yf(sig, epl=float(peeq), pred=True) * (1. / m.sy)
            fig, ax = plt.subplots()
            m.plot_data(np.array(Z, dtype=float), ax, xx, yy, field=True)
            rec['%s_slice%d_Z' % (tag, j)] = np.array(ax.images[0].get_array(), dtype=float)
            plt.close('all')
            if (c1, c2) == (0, 1):   # the same slice as the reference's own plot_yield_locus draws it
                axs = m.plot_yield_locus(axis1=[0], axis2=[1], peeq=float(peeq), Nmesh=YC.NMESH, field=True)
                own = np.array(axs.images[0].get_array(), dtype=float)
                assert np.array_equal(own, rec["%s_slice%d_Z" % (tag, j)]), (tag, np.max(np.abs(own - rec["%s_slice%d_Z" % (tag, j)])))
                plt.close('all')
        rec[tag + '_slice_peeq'] = np.array(peeq)
    x, y = mats['hill'].ellipsis()
    rec['ellipsis_default'] = np.array([x, y])
    x, y = mats['hill'].ellipsis(a=1.3, b=0.4, n=17)
    rec['ellipsis_13_04_17'] = np.array([x, y])

    out = os.path.join(YC.GOLD, 'yield_locus.npz')
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < 300 * 1024


if __name__ == '__main__':
    sys.exit(main())

"""Committee / query by committee, the parts that need no GPU: the spherical-angle helper against the reference's recorded
vectors, the self-consistency of tests/golden/committee.npz (tools/gen_committee.py), the refusals of Committee, and the
package's exports."""
import numpy as np
import pytest

import pylabfea_amd as FE

import committee_cases as CC


@pytest.fixture(scope='module')
def z():
    return CC.load()


def test_helper_matches_reference(z):
    """sig_spherical_to_cartesian reproduces the reference's eight vectors to 2 ulp per component, for (5,) and (N,5)"""
    ang, seq, ref = z['helper_angles'], z['helper_seq'], z['helper_out']
    tol = 2 * CC.ulp(ref)
    for i in range(8):
        out = FE.sig_spherical_to_cartesian(ang[i], seq=seq[i])
        assert out.shape == (6,)
        assert np.all(np.abs(out - ref[i]) <= tol[i]), (i, np.max(np.abs(out - ref[i]) / tol[i]))
    out = FE.sig_spherical_to_cartesian(ang, seq=seq)
    assert out.shape == (8, 6)
    assert np.all(np.abs(out - ref) <= tol)
    one = FE.sig_spherical_to_cartesian(ang[:3])
    assert np.all(np.abs(np.linalg.norm(one, axis=1) - 1.) < 1e-15 * 8)
    assert np.all(np.abs(FE.sig_spherical_to_cartesian(z['cand_angles']) - z['cand_su']) <= 2 * CC.ulp(z['cand_su']))


@pytest.mark.parametrize('bad', [np.zeros(4), np.zeros(6), np.zeros((3, 4)), np.zeros((2, 3, 5))])
def test_helper_wrong_length(bad):
    with pytest.raises(ValueError):
        FE.sig_spherical_to_cartesian(bad)


def test_fixture_self_check(z):
    """np.var of the recorded yf is the recorded variance; the longdouble restatement from the recorded tables is within
    r_ref A 2^-53 of the recorded yf; the recorded argmax is the variance's"""
    yf, var = z['yf_ref'], z['var_ref']
    assert yf.shape == (CC.NMEM, 256) and z['cand_su'].shape == (256, 6)
    assert np.array_equal(np.var(yf[:5], axis=0), var)
    assert int(z['argmax_ref']) == int(np.argmax(var))
    for k in range(CC.NMEM):
        p = CC.member_params(z, k)
        assert p['sv'].shape == (len(p['dual']), 6)
        assert p['dev_only'] == (k == 5)
        f, A, G, xm = CC.restate(p, z['cand_su'], 0.5 * p['sy'])
        r = float(z['r_ref'][k])
        assert np.all(np.abs(yf[k].astype(CC.LD) - f) <= CC.LD(r) * A * CC.EPS53 * (1 + 1e-12)), k
    # the margin the generator guarantees for the argmax test
    delta = np.max([np.asarray(CC.value_bar(z['r_ref'][k], *CC.restate(CC.member_params(z, k), z['cand_su'],
                                                                        0.5 * float(z['m%d_sy' % k]))[1:]), dtype=float)
                    for k in range(5)], axis=0)
    vbar = CC.variance_bar(yf[:5], delta, var)
    o = np.argsort(var)
    assert var[o[-1]] - var[o[-2]] > 2 * max(vbar[o[-1]], vbar[o[-2]])


def _member(z, k=0):
    return CC.facade(CC.member_params(z, k))


def test_committee_refusals(z):
    m = _member(z)
    un = FE.Material(name='untrained')
    un.elasticity(E=2e5, nu=0.3)
    un.plasticity(sy=50., sdim=6)
    with pytest.raises(ValueError, match='no trained SVC'):
        FE.Committee([m, un])
    z3 = np.load(CC.GOLD + '/svc_hill3d.npz')
    m3 = FE.Material(name='sdim3')
    m3.elasticity(E=float(z3['par_E']), nu=float(z3['par_nu']))
    m3.plasticity(sy=float(z3['par_sy']), sdim=3)
    m3.set_svc(z3['par_sv'], z3['par_dual'], float(z3['par_intercept']), float(z3['par_gamma']), float(z3['par_scale_seq']))
    with pytest.raises(ValueError, match='sdim = 3'):
        FE.Committee([m3])
    zw = np.load(CC.GOLD + '/svc_workhard.npz')
    mw = FE.Material(name='wh')
    mw.elasticity(E=float(zw['par_E']), nu=float(zw['par_nu']))
    mw.plasticity(sy=float(zw['par_sy']), sdim=6)
    mw.set_svc(zw['par_sv'], zw['par_dual'], float(zw['par_intercept']), float(zw['par_gamma']), float(zw['par_scale_seq']),
               scale_wh=float(zw['par_scale_wh']))
    with pytest.raises(ValueError, match='work-hardening'):
        FE.Committee([m, mw])
    mg = _member(z, 1)
    mg.ML_grad = True
    with pytest.raises(ValueError, match='ML_grad'):
        FE.Committee([mg])
    with pytest.raises(ValueError, match='0 members'):
        FE.Committee([])
    with pytest.raises(ValueError, match='17 members'):
        FE.Committee([m] * 17)
    with pytest.raises(ValueError, match='scale'):
        FE.Committee([m, m], scale=[1., 2., 3.])
    with pytest.raises(ValueError, match='scale'):
        FE.Committee([m], scale=0.)
    c = FE.Committee([m] * 16)
    assert len(c) == 16 and np.array_equal(c.scale, np.full(16, 0.5 * m.sy))
    assert np.array_equal(FE.Committee([m, m], scale=3.).scale, [3., 3.])


def test_exports():
    for name in ('Committee', 'train_committee', 'active_learning', 'sig_spherical_to_cartesian'):
        assert hasattr(FE, name) and name in FE.__all__, name
    from pylabfea_amd import _lib
    assert 'plfx_committee_yf' in _lib.SYMBOLS and 'plfx_committee_info' in _lib.SYMBOLS

"""The calc_scf statistics and the 18 element sums of calc_global from their definitions, past one workgroup and past the
grid caps.  So far plfx_scf_all was held to plfx_scf_stats + scf_sumsq (the same element and reduce kernels) and
finish_step to global_sums (bit for bit) on 144 elements, and both to whole-solve traces with uniform fields.  Here the state
is set from outside (state_set), seeded and non-uniform, and the references are NumPy / math.fsum around the CPU oracle
(tests/reduction_cases.py; their input conditions: tests/test_reduction_cases_cpu.py)."""
import numpy as np
import pytest

import reduction_cases as RC

pytestmark = pytest.mark.gpu

_models = {}


def model(kind, nel, *args):
    """façade model and engine, built once per module and size (the 262 656-element one takes a moment)"""
    key = (kind, nel) + args
    if key not in _models:
        fe = RC.scf_model(nel, *args) if kind == 'scf' else RC.sums_model(nel)
        _models[key] = (fe, fe._ensure_engine())
    return _models[key]


# ------------------------------------------------------------------------------------------------ calc_scf statistics
def scf_check(nel, laminate, emins):
    from pylabfea_amd import _lib
    fe, eng = model('scf', nel, laminate)
    for emin in emins:
        case = RC.ScfCase(fe, emin=emin)
        eng.state_reset()
        eng.state_set(_lib.ST_SIG, case.sig)
        eng.state_set(_lib.ST_EPL, case.epl)
        eng.state_set(_lib.ST_DU, case.du)
        cnt, mn, s, s2 = case.stats()
        tau = RC.TAU
        a = eng.scf_all(RC.SLD)
        b3 = eng.scf_stats(RC.SLD)
        b = b3 + (eng.scf_sumsq(b3[2] / b3[0]),)
        for tag, (dc, dmn, ds, ds2) in (('scf_all', a), ('scf_stats + scf_sumsq', b)):
            print('%d elements, minimum at %d, %s: count %d (%d), min %.3e, sum %.3e of %.3e, squares %.3e of %.3e'
                  % (nel, emin, tag, dc, cnt, abs(dmn - mn), abs(ds - s), cnt * tau, abs(ds2 - s2), 2 * cnt * tau))
            assert dc == cnt
            assert abs(dmn - mn) <= tau and abs(dmn - case.hh[emin]) <= tau
            assert abs(ds - s) <= cnt * tau
            assert abs(ds2 - s2) <= 2 * cnt * tau


@pytest.mark.parametrize('nel', [255, 256, 257, 784])
def test_scf_statistics_from_the_definition(nel):
    """count exact, min within tau = 1e-9 (the analytic point kernels' bar on hh <= 1), sum within count tau, centred sum of
    squares within 2 count tau, for both entry points, with the unique minimum (0.15 below every other ratio) at element 0, 255,
    256 and the last one in turn.  All three multiplicities occur in every block of 256; a dropped or doubled element moves the
    sum by 0.2 or more."""
    scf_check(nel, False, sorted({e for e in (0, 255, 256, nel - 1) if e < nel}))


def test_scf_statistics_skip_an_elastic_section():
    """[Hill | elastic | Hill]: the elastic elements are skipped (multiplicity 0)"""
    scf_check(784, True, [0, 783])


def test_scf_statistics_past_the_grid_cap():
    """513 x 512 = 262 656 elements: k_scf_reduce runs its 256 blocks (the cap of plfx_scf_all) through the grid-stride loop
    five times; count tau is 3e-4 here, a dropped element 0.2"""
    scf_check(262656, False, [0, 255, 256, 262655])


# ------------------------------------------------------------------------------------------------ the 18 element sums
@pytest.mark.parametrize('nel', [1, 255, 256, 257, 784, 262656, 524800])
def test_global_sums_from_the_definition(nel):
    """global_sums of seeded sig, eps, epl (random signs, magnitudes in [0.5, 1.5], one seed per component) on a laminate whose
    two sections have different element volumes, against math.fsum(x[:, k] * vel):

        |device - fsum| <= D 2^-53 A_k,   A_k = fsum(|x[:, k] * vel|)

    D = the roundings on the longest path of the device's summation, counted from the code (reduction_cases.sums_depth):
    ceil(nel / (256 g)) fma terms per thread of the g = min(ceil(nel / 256), 2048) blocks of k_global_partials, 6 levels of the
    wave sum, 4 wave results; ceil(g / 256) partials per thread of k_reduce_rows, 6 levels, 4 wave results; 2 for the
    reference (its rounded product, fsum's final rounding).  24 up to 65 536 elements, 28 at 262 656 (1026 partials: five
    per thread), 32 at 524 800 = 1025 x 512, the first mesh of this shape past the cap of 2048 blocks, where the grid-stride
    loop starts.  This is the standard bound of a summation tree, not a measurement; a missing element moves a sum by at
    least 0.5 min(vel), about A_k / nel."""
    from pylabfea_amd import _lib
    fe, eng = model('sums', nel)
    sig, eps, epl = fields = RC.sums_state(nel)
    eng.state_reset()
    eng.state_set(_lib.ST_SIG, sig)
    eng.state_set(_lib.ST_EPS, eps)
    eng.state_set(_lib.ST_EPL, epl)
    got = eng.global_sums()
    ref, gauge = RC.sums_reference(fields, RC.element_volumes(fe))
    D = RC.sums_depth(nel)
    worst = np.max(np.abs(got - ref) / gauge) / 2. ** -53
    print('%d elements: worst |device - fsum| = %.2f x 2^-53 A_k (D = %d)' % (nel, worst, D))
    assert np.all(np.abs(got - ref) <= D * 2. ** -53 * gauge)
    assert np.array_equal(eng.state_get(_lib.ST_EPS), eps)                       # (the stored strain field was the one summed)

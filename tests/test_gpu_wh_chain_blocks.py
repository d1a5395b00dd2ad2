"""The sequential hardening carry of ONE sweep across blocks of 256 elements (k_wh_blockmax, k_wh_scan, k_wh_entry driven by
sweep_wh_sequential).  Every other test that runs these kernels has at most 36 elements: one block, bpre = -1, one
turn of the scan loop.  Here: two to four blocks, blocks without a touched element, predecessors one to three blocks back, a
foreign material that fills a whole block, touched elements at 63 | 64, 255 | 256, 511 | 512 and at the last index, two chains
side by side.  The cases, their reference (the oracle's element loop on one mutable object per material) and the conditions
under which they discriminate are in tests/reduction_cases.py and held on the CPU by tests/test_reduction_cases_cpu.py."""
import numpy as np
import pytest

import reduction_cases as RC

pytestmark = pytest.mark.gpu


def run_sweep(case, khard_guess):
    """state_reset, upload the case's state and a guess of the entry moduli, one plfx_sweep; every read-back"""
    from pylabfea_amd import _lib
    fe = case.fe
    eng = fe._ensure_engine()
    eng.state_reset()
    eng.state_set(_lib.ST_SIG, case.sig)
    eng.state_set(_lib.ST_EPL, case.epl)
    eng.state_set(_lib.ST_DU, case.du)
    eng.state_set(_lib.ST_KHARD, khard_guess)
    for key in case.wh_keys:
        eng.wh_carry(case.engine_mat[key], case.start_carry[key])
    seq0, nsw0, np0 = eng.wh_info()
    unres0 = eng.wh_unresolved_sweeps()
    eng.sweep(0)
    seq, nsw, npass = eng.wh_info()
    return dict(khard=eng.state_get(_lib.ST_KHARD), res_sig=eng.state_get(_lib.ST_RES_SIG), res_depl=eng.state_get(_lib.ST_RES_DEPL),
                fyn=eng.state_get(_lib.ST_FYN), carry={key: eng.wh_carry(case.engine_mat[key]) for key in case.wh_keys},
                sequential=seq, sweeps=nsw - nsw0, passes=npass - np0, unresolved=eng.wh_unresolved_sweeps() - unres0)


@pytest.mark.parametrize('name', RC.CHAIN_CASES)
def test_carry_chain_of_one_sweep_across_blocks(name):
    """One plfx_sweep from two different guesses of the entry moduli (zeros; seeded values) against the reference's loop.

    Exact, device against device: a quiet element (du zero on its four nodes: its call evaluates no gradient, so its exit
    modulus, state 11, IS the scan's output) holds, bit for bit, the exit modulus of the last element of its object before
    it that left another value than it entered with, or the object's start carry.  Against the oracle: state 11 and the
    moduli the objects are left with within 1e-6 max(1, max|kpt|), res_sig within 1e-6 sy, res_depl within 1e-9 (the bars of
    test_gpu_response_with_explicit_khard).  The accepted pass is the sequential loop's sweep whatever the guess was, so
    every read-back is bit-identical between the two guesses; one sweep counted, none unresolved."""
    case = RC.chain_case(name)
    ref = case.reference()
    sy = float(RC.golden('svc_workhard_chain.npz')['par_sy'])
    wh = case.obj_of_el >= 0
    outs = []
    for tag, guess in (('zeros', np.zeros(case.nel)), ('seeded', case.seeded_khard)):
        out = run_sweep(case, guess)
        outs.append(out)
        print('%s, first guess %s: %d passes' % (name, tag, out['passes']))
        assert out['sequential'] and out['sweeps'] == 1 and out['unresolved'] == 0 and out['passes'] >= 1
        kh = out['khard']
        nq = []

        def check(e, run):
            nq.append(e)
            assert kh[e].tobytes() == np.float64(run).tobytes(), (e, kh[e], run)

        entry, touched, last = case.chain_walk(kh, check)
        assert len(nq) == int(np.sum(case.quiet & wh)) > 0
        assert np.array_equal(touched, case.chain_walk(ref['kpt'])[1])           # the same calls evaluate a gradient
        bar = 1e-6 * max(1., float(np.max(np.abs(ref['kpt'][wh]))))
        dev = np.abs(kh - ref['kpt'])[wh]
        print('    max |state 11 - kpt| = %.3e at element %d (bar %.3e)' % (dev.max(), np.nonzero(wh)[0][int(np.argmax(dev))], bar))
        assert dev.max() < bar
        for key in case.wh_keys:
            assert out['carry'][key] == last[key]                                # what the object holds IS its last touched exit
            assert abs(out['carry'][key] - ref['kout'][key]) < bar
        pl = case.ref.plastic
        assert np.max(np.abs(out['res_sig'] - ref['res_sig'])[pl]) < 1e-6 * sy
        assert np.max(np.abs(out['res_depl'] - ref['res_depl'])[pl]) < 1e-9
    a, b = outs
    for k in ('khard', 'res_sig', 'res_depl', 'fyn'):
        sel = wh if k == 'khard' else slice(None)
        assert np.array_equal(a[k][sel], b[k][sel]), k
    assert a['carry'] == b['carry']


def test_unresolved_accessor_leaves_wh_info_as_it_was():
    from pylabfea_amd import _lib
    case = RC.chain_case('quiet0_272')
    eng = case.fe._ensure_engine()
    info = eng.wh_info()
    assert len(info) == 3 and isinstance(info[0], bool)
    assert eng.wh_unresolved_sweeps() == eng.wh_unresolved and isinstance(eng.wh_unresolved_sweeps(), int)
    assert eng.wh_info() == info

"""The designed cases of tests/reduction_cases.py, held on the CPU oracle alone: the conditions under which the GPU
tests test_gpu_wh_chain_blocks.py and test_gpu_element_reductions.py discriminate, the block layout the cases claim, and the
two references against independent restatements.  No case is dropped at run time: a case that misses a condition fails here."""
import math
import warnings

import numpy as np
import pytest

import reduction_cases as RC
from oracle import oracle as O


# ------------------------------------------------------------------------------------------------ A: the carry chain
def test_chain_cases_have_the_block_layout_they_claim():
    """which elements fall in which block of 256, which are quiet, where the foreign sections lie"""
    blk = RC.block_of
    c = RC.chain_case('block0_784')
    assert (c.NX, c.NY, c.nel) == (49, 16, 784) and -(-c.nel // RC.BLOCK) == 4
    assert np.all(blk(np.nonzero(~c.quiet)[0]) == 0) and not c.quiet[255] and np.all(c.quiet[256:])
    c = RC.chain_case('block0_272')
    assert c.nel == 272 and np.all(c.quiet[256:]) and np.sum(blk(np.arange(c.nel)) == 1) == 16
    for name, nel in (('quiet0_272', 272), ('quiet0_512', 512)):
        c = RC.chain_case(name)
        touched = c.chain_walk(c.reference()['kpt'])[1]
        assert c.nel == nel and nel % RC.BLOCK == (16 if nel == 272 else 0)
        assert not np.any(touched[:256]) and np.sum(c.quiet[:256]) >= 254 and np.any(touched[256:])
    assert np.all(RC.chain_case('quiet0_512').quiet[:256])
    for name, want in (('edges_512', [63, 64, 255, 256, 511]), ('edges_784', [63, 64, 255, 256, 511, 512, 783])):
        c = RC.chain_case(name)
        touched = c.chain_walk(c.reference()['kpt'])[1]
        assert list(np.nonzero(touched)[0]) == want                          # single elements at the wave, block and mesh edges
        for e in want:
            for nb in (e - 1, e + 1):
                if 0 <= nb < c.nel and nb not in want:
                    assert c.quiet[nb], (e, nb)                              # quiet neighbours on both sides
    for key in ('el', 'j2'):
        c = RC.chain_case('laminate_%s_784' % key)
        foreign = np.nonzero(c.obj_of_el < 0)[0]
        assert foreign[0] == 256 and foreign[-1] == 256 + 17 * 16 - 1        # the whole of block 1 and one column of block 2
        assert len(c.fe.mat) == 3 and c.fe.mat[0] is c.fe.mat[2] and c.engine_mat['A'] == 0
        assert np.all(c.quiet[528:528 + 8 * 16])                             # the third section starts with eight quiet columns
    c = RC.chain_case('two_objects_784')
    assert c.wh_keys == ['A', 'B'] and c.engine_mat == {'A': 0, 'B': 1} and c.start_carry['A'] != c.start_carry['B']
    assert list(np.nonzero(np.diff(c.obj_of_el))[0] + 1) == [160, 384, 576]  # sections of 10 | 14 | 12 | 13 columns
    for i in (0, 1):
        assert len(set(blk(np.nonzero((c.obj_of_el == i) & ~c.quiet)[0]))) >= 2


@pytest.mark.parametrize('name', RC.CHAIN_CASES)
def test_chain_case_meets_the_input_conditions(name):
    """The entry modulus does not show in the stresses, so the chain shows only in the exit moduli of the quiet elements --
    and only if neighbouring touched elements leave different, positive moduli: every touched predecessor of a quiet run has a
    positive exit that differs from the previous touched element's and from the start carry by more than 1e-3 relative; at
    least half of the touched elements have positive, pairwise distinct exits; every quiet run behind a touched element
    differs from the per-point carry (a run before the first touched element holds the start carry under either contract);
    and no element changes sides under a relative change of 1e-6 of the increment."""
    c = RC.chain_case(name)
    out = c.reference()
    kpt = out['kpt']
    entry, touched, last = c.chain_walk(kpt)
    assert last == out['kout']                                               # the walk reproduces what each object is left with
    runs = RC.quiet_runs(c)
    assert any(p is not None for _, p, _ in runs)
    t_idx = {key: [int(e) for e in np.nonzero(touched & (c.obj_of_el == i))[0]] for i, key in enumerate(c.wh_keys)}
    pp = c.per_point()
    for key, p, run in runs:
        if p is None:
            assert np.all(kpt[run] == c.start_carry[key])
            continue
        assert kpt[p] > 0.
        q = t_idx[key].index(p)
        prev = kpt[t_idx[key][q - 1]] if q > 0 else c.start_carry[key]
        assert abs(kpt[p] - prev) > 1e-3 * kpt[p] and abs(kpt[p] - c.start_carry[key]) > 1e-3 * kpt[p]
        assert np.all(kpt[run] == kpt[p]) and np.all(pp[run] != kpt[run])
    kt = kpt[touched]
    pos = kt[kt > 0.]
    assert len(np.unique(pos)) == len(pos) and 2 * len(pos) >= len(kt) > 0
    wh = c.obj_of_el >= 0
    assert np.all(c.seeded_khard[wh] != entry[wh]) and np.mean(entry[wh] != 0.) > 0.5   # both first guesses of the entry moduli are wrong
    for f in (1. - 1e-6, 1. + 1e-6):
        r = c.ref
        o2 = O.response_wh(r.mats, r.CVs, c.sig, c.epl, f * c.deps(), khard_in=c.carry_by_oracle_mat(), mat_id=r.mat_id,
                           sequential=True)
        assert np.array_equal(o2[4], out['nsteps']) and np.array_equal(c.chain_walk(o2[6])[1], touched)
        assert np.max(np.abs(o2[6] - kpt)) < 1e-3 * np.max(kpt)


def test_chain_reference_equals_a_point_by_point_loop():
    """O.response_wh(sequential=True) against the same chain carried by hand through single-point calls"""
    c = RC.chain_case('edges_512')
    kpt, carry = RC.chain_python_loop(c)
    out = c.reference()
    wh = c.obj_of_el >= 0
    assert np.array_equal(kpt[wh], out['kpt'][wh]) and carry[c.oracle_mat['A']] == out['kout']['A']
    c = RC.chain_case('two_objects_784')
    kpt, carry = RC.chain_python_loop(c)
    assert np.array_equal(kpt, c.reference()['kpt'])
    assert {k: carry[c.oracle_mat[k]] for k in c.wh_keys} == c.reference()['kout']


# ------------------------------------------------------------------------------------------------ B: calc_scf statistics
def scf_emins(nel):
    return sorted({e for e in (0, 255, 256, nel - 1) if e < nel})


@pytest.mark.parametrize('nel,laminate', [(255, False), (256, False), (257, False), (784, False), (784, True), (262656, False)])
def test_scf_case_meets_the_input_conditions(nel, laminate):
    fe = RC.scf_model(nel, laminate)
    sy = next(m.sy for m in fe.mat if m.sy is not None)
    for emin in scf_emins(nel) if nel < 100000 else [0, nel - 1]:
        c = RC.ScfCase(fe, emin=emin)
        cm = c.mult > 0
        assert np.min(np.abs(c.sref[c.ref.plastic] - 0.1)) > 1e-3            # nobody near the sref threshold ...
        assert np.min(np.abs(c.yf0[cm] + 0.15)) > 1e-3 * sy                  # ... or the branch threshold
        assert np.array_equal(c.mult, c.branch)                             # every element on the branch it was designed for
        if laminate:
            assert np.all(c.mult[~c.ref.plastic] == 0) and np.sum(~c.ref.plastic) == 12 * 16
        for b in range(-(-nel // RC.BLOCK)):
            m = c.mult[b * RC.BLOCK:(b + 1) * RC.BLOCK]
            assert len(set(m)) == min(3, len(m)), b                          # all three multiplicities in every block
        entries = np.repeat(c.hh[cm], c.mult[cm])
        assert len(entries) == len(c.list) and np.mean(entries < 1.) >= 0.5   # the sum is not a count
        assert np.max(np.abs(np.sort(entries) - np.sort(c.list))) < 1e-13    # the list of RefSolver.scf_list, restated
        o = np.sort(c.hh[cm])
        assert int(np.argmin(np.where(cm, c.hh, 9.))) == emin and o[1] - o[0] >= 0.05
        assert np.any(c.epl[cm] != 0.) and np.any(np.all(c.epl[cm] == 0., axis=1))


def test_scf_statistics_equal_calc_scf_on_12_by_12():
    """count, min, fsum and centred fsum of the list give RefSolver.calc_scf's return value (model.py:1059-1067)"""
    fe = RC.scf_model(144)
    for emin, scale in ((0, 1.), (143, 1.), (77, 0.3)):
        c = RC.ScfCase(fe, emin=emin)
        du = scale * c.du
        c.list = c.ref.scf_list(du, RC.SLD)
        cnt, mn, s, s2 = c.stats()
        sd = math.sqrt(s2 / cnt)
        want = max(mn if sd < 0.1 else max(1.e-3, s / cnt - sd), 1.e-3)
        got = c.ref.calc_scf(du, RC.SLD)
        assert cnt > 100 and abs(got - want) < 1e-13, (got, want)


# ------------------------------------------------------------------------------------------------ C: the 18 element sums
def test_sums_cases():
    for nel, (NX, NY) in RC.SUM_SIZES.items():
        fe = RC.sums_model(nel)
        assert fe.Nel == nel == NX * NY
        vel = RC.element_volumes(fe)
        assert len(np.unique(vel)) == (1 if nel == 1 else 2)                 # the element volume differs by section
        if nel > 300000:
            continue
        fields = RC.sums_state(nel)
        s, g = RC.sums_reference(fields, vel)
        x = np.concatenate(fields, axis=1)
        assert np.all(np.abs(x) >= 0.5) and np.all(np.abs(x) <= 1.5)
        assert nel == 1 or len({tuple(np.sign(x[:, k])) for k in range(18)}) == 18       # no two components alike
        # a missing element moves a sum by at least 0.5 min(vel): orders above the bar D 2^-53 A_k
        D = RC.sums_depth(nel)
        assert 0.5 * np.min(vel) > 1e6 * D * 2. ** -53 * np.max(g)
    # the depth count at the sizes where the device's path changes (reduction_cases.sums_depth)
    assert [RC.sums_depth(n) for n in (1, 256, 257, 65536, 65537, 262656, 524288, 524800)] == [24, 24, 24, 24, 25, 28, 31, 32]
    assert -(-262656 // RC.BLOCK) > RC.SCF_CAP and -(-524800 // RC.BLOCK) > RC.SUM_CAP > -(-262656 // RC.BLOCK)

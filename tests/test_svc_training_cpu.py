"""Host side of SVC training without a GPU (fixture tests/golden/svc_training.npz from tools/gen_svc_training.py):
the reference's load-case directions, the layout of create_sig_data's training stresses, the fold assignment of
StratifiedKFold(5), the candidate order of the grid search, training_score, and the refusals of the unsupported paths."""
import os

import numpy as np
import pytest

import pylabfea_amd as FE
from pylabfea_amd import training as T


@pytest.fixture(scope='module')
def z(golden_dir):
    return np.load(os.path.join(golden_dir, 'svc_training.npz'))


def ref_st(z, c):
    """the reference's training stresses: its yield-locus stresses scaled block by block (bit for bit, see the generator)"""
    sd, seq = z[c + '_sdata'], z[c + '_seq']
    return (seq[:, None, None] * sd[None, :, :]).reshape(-1, sd.shape[1])


def ref_yt(z, c):
    return np.repeat(np.where(np.arange(len(z[c + '_seq'])) < int(z[c + '_Nseq']), -1., 1.), len(z[c + '_sdata']))


def test_load_cases_match_reference(z):
    ref = z['lc_30_60']
    got = FE.load_cases(30, 60)
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))


class _J2Ref(object):
    """stand-in for a J2 reference material: its yield-locus scale is sy / seq_J2 (what Material._yield_scale returns
    for J2 / Hill references, evaluated on the device there)"""

    def __init__(self, sy):
        self.sy = sy

    def _yield_scale(self, su):
        return self.sy / FE.sig_eq_j2(su)


def test_create_sig_data_layout_j2(z):
    c = 'j2train'
    m = FE.Material('ML-J2')
    m.elasticity(E=200000., nu=0.3)
    m.plasticity(sy=float(z[c + '_sy']), sdim=6)
    st, yt = m.create_sig_data(N=int(z[c + '_Nlc']), mat_ref=_J2Ref(float(z[c + '_sy'])), Nseq=int(z[c + '_Nseq']),
                               Fe=float(z[c + '_Fe']), Ce=float(z[c + '_Ce']), extend=bool(z[c + '_extend']))
    ref = ref_st(z, c)
    assert st.shape == ref.shape
    assert np.max(np.abs(st - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert np.array_equal(yt, ref_yt(z, c))


def test_create_sig_data_from_sdata(z):
    """sdata path: the yield stresses are given, the sequence of scalings is the same"""
    c = 'j2train'
    N = int(z[c + '_Nlc'])
    Nseq = int(z[c + '_Nseq'])
    ref = ref_st(z, c)
    Fe, Ce = float(z[c + '_Fe']), float(z[c + '_Ce'])
    sdata = z[c + '_sdata']
    assert len(sdata) == N
    m = FE.Material('ML-J2')
    m.elasticity(E=200000., nu=0.3)
    m.plasticity(sy=60., sdim=6)
    st, yt = m.create_sig_data(sdata=sdata, Nseq=Nseq, Fe=Fe, Ce=Ce)
    assert st.shape == ref.shape
    assert np.array_equal(st, ref)
    assert np.array_equal(yt, ref_yt(z, c))


def test_stratified_folds_exact(z):
    y = ref_yt(z, 'gs')
    folds = T.stratified_folds(y, 5)
    fold_of = np.empty(len(y), dtype=int)
    for k, f in enumerate(folds):
        fold_of[f] = k
    assert np.array_equal(fold_of, z['gs_fold_of'])
    assert sorted(np.concatenate(folds).tolist()) == list(range(len(y)))


def test_candidate_order(z):
    cands = T.param_grid(list(z['gs_cvals']), list(z['gs_gvals']))
    assert len(cands) == len(z['gs_mean_test_score']) == 24
    assert cands[:7] == [(1., .5), (1., 1.), (1., 1.5), (1., 2.), (1., 2.5), (1., 3.), (2., .5)]
    # the default grid of setup_yf_SVM_6D extended by C = 15, gamma = 4: 5 x 7 = 35 candidates, C outer
    c2 = T.param_grid([1, 2, 4, 10, 15], [0.5, 1, 1.5, 2, 2.5, 3, 4])
    assert len(c2) == 35 and c2[6] == (1, 4) and c2[-1] == (15, 4)


def test_training_score_values():
    ref = np.array([1., -1., 0., 2., -3., 0.5, -0.1, 4.])
    ml = np.array([1., 1., -1., 2., -3., -0.5, -0.2, 0.])
    mae, prec, acc, rec, f1, mcc = FE.training_score(ref, ml)
    assert mae == pytest.approx(np.mean(np.abs(ref - ml)))
    # labels (0 -> +1): ref + - + + - + - + ; ml + + - + - - - +  -> TP 3, FN 2, FP 1, TN 2
    assert (prec, acc, rec) == (3 / 4, 5 / 8, 3 / 5)
    assert f1 == pytest.approx(2 * 0.75 * 0.6 / 1.35)
    assert -1. <= mcc <= 1.


def test_unsupported_paths_refused():
    m = FE.Material('ML')
    with pytest.raises(ValueError):
        m.train_SVC(C=2, gamma=1)            # neither mat_ref nor sdata
    m.msparam = [{'Nlc': 1}]
    with pytest.raises(NotImplementedError):
        m.train_SVC(C=2, gamma=1, mat_ref=FE.Material('ref'))
    m2 = FE.Material('ML')
    m2.txdat = True
    with pytest.raises(NotImplementedError):
        m2.setup_yf_SVM_6D(np.zeros((4, 6)), np.array([-1., -1., 1., 1.]))
    with pytest.raises(NotImplementedError):
        FE.Material('ML').train_SVC(C=2, gamma=1, sdata=np.ones((3, 6)), pca=object())

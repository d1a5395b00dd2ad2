"""Data -> Material.from_data -> training rows, on the host (no GPU): the NumPy port of the reference's data module
(pylabfea/data.py) against the reference's own outputs in tests/golden/svc_data_training.npz
(tools/gen_svc_data_training.py), and the refusals of what is not supported."""
import json
import os

import numpy as np
import pytest

COMP = ('11', '22', '33', '23', '13', '12')


@pytest.fixture(scope='module')
def z(golden_dir):
    return np.load(os.path.join(golden_dir, 'svc_data_training.npz'))


def wh_lc_data(z):
    """the load cases of the wh_ case, rebuilt from the stored arrays (the reference's dict order)"""
    out, o = {}, 0
    for key, n in zip(z['wh_keys'], z['wh_lc_len']):
        out[str(key)] = {f: z['wh_lc_' + f][o:o + n] for f in ('Stress', 'Eq_Stress', 'Strain_Plastic',
                                                                'Eq_Strain_Plastic', 'Strain_Total')}
        o += n
    return out


def js_json(z, path, layout, mode='RS'):
    """the CPFEM database rewritten as a JSON file: 'legacy' (Results, S11 ...) or 'new' (stress / strains in GPa)"""
    data, o = {}, 0
    for key, n in zip(z['js_keys'], z['js_len']):
        comp = {pre + c: z['js_%s%s' % (pre, c)][o:o + n] for pre in ('S', 'E', 'Ep') for c in COMP}
        o += n
        if layout == 'legacy':
            res = {k: list(v) for k, v in comp.items()}
            if mode == 'JS':   # the JS order names the 23 shear component 32
                for pre in ('S', 'E', 'Ep'):
                    res[pre + '32'] = res.pop(pre + '23')
            data[str(key)] = {'Results': res}
        else:
            data[str(key)] = {'stress': {'s' + c: list(comp['S' + c] / 1000.) for c in COMP},
                              'total_strain': {'e' + c: list(comp['E' + c]) for c in COMP},
                              'plastic_strain': {'ep' + c: list(comp['Ep' + c]) for c in COMP},
                              'units': {'Stress': 'GPa', 'Strain': 'None'}}
    with open(path, 'w') as fp:
        json.dump(data, fp)
    return path


def check_md(md, z, pre):
    for k in ('lc_indices', 'Nlc', 'Ncyl', 'transition_ind'):
        assert np.array_equal(np.asarray(md[k]), z[pre + k]), k
    for k in ('flow_stress', 'plastic_strain', 'sig_ideal'):   # selected exactly, values to 1e-12
        a, b = np.asarray(md[k]), z[pre + k]
        assert a.shape == b.shape, k
        assert np.max(np.abs(a - b)) <= 1e-12 * max(1., np.max(np.abs(b))), k
    for k in ('epc', 'ep_start', 'ep_max', 'peeq_max', 'sy_av'):
        assert abs(float(md[k]) - float(z[pre + k])) <= 1e-12 * max(1., abs(float(z[pre + k]))), k
    C, Cr = md['elast_const'], z[pre + 'elast_const']
    assert np.max(np.abs(C - Cr)) <= 1e-9 * np.max(np.abs(Cr))


def test_savgol_against_scipy_values():
    """first derivative, polyorder 1, SciPy's 'interp' edges; expected values from the closed form of the least-squares
    slope, edges included, and one literal vector computed with scipy.signal.savgol_filter(x, 5, 1, deriv=1)"""
    from pylabfea_amd.data import savgol_deriv1
    x = np.array([0., 1., 4., 9., 16., 25., 36., 49.])
    # scipy.signal.savgol_filter(x, 5, 1, deriv=1) -> [4, 4, 4, 6, 8, 10, 10, 10] (the edges fit the first / last window)
    assert np.allclose(savgol_deriv1(x, 5), [4., 4., 4., 6., 8., 10., 10., 10.], rtol=0, atol=1e-12)
    # even window: scipy.signal.savgol_filter(x, 4, 1, deriv=1) -> [3, 3, 5, 7, 9, 11, 11, 11]
    assert np.allclose(savgol_deriv1(x, 4), [3., 3., 5., 7., 9., 11., 11., 11.], rtol=0, atol=1e-12)
    lin = 3. * np.arange(30) + 2.
    for w in (2, 3, 5, 6, 11):
        assert np.allclose(savgol_deriv1(lin, w), 3., rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        savgol_deriv1(x, 9)


def test_transition_index_and_elastic_fit(z):
    from pylabfea_amd.data import find_transition_index, get_elastic_coefficients
    lc = wh_lc_data(z)
    its = [find_transition_index(v['Eq_Stress']) for v in lc.values()]
    assert its == [int(t[0]) for t in z['wh_md_transition_ind']]
    CV = z['wh_CV']
    rng = np.random.default_rng(3)
    eps = rng.normal(size=(12, 6)) * 1e-3
    assert np.allclose(get_elastic_coefficients(eps, eps @ CV.T), CV, rtol=1e-10, atol=1e-6)
    with pytest.raises(NotImplementedError):
        get_elastic_coefficients(eps, eps @ CV.T, method='decomposition')


def test_parse_data_work_hardening(z):
    import pylabfea_amd as FE
    dd = FE.Data(wh_lc_data(z), mat_name='ML_Hill_hardening', epl_start=0.0, epl_crit=0.0,
                 epl_max=float(z['wh_epl_max']), depl=float(z['wh_depl']), wh_data=True)
    check_md(dd.mat_data, z, 'wh_md_')


@pytest.mark.parametrize('layout', ['legacy', 'new'])
def test_read_json_database(z, tmp_path, layout):
    import pylabfea_amd as FE
    p = js_json(z, str(tmp_path / 'db.json'), layout)
    db = FE.Data(os.path.basename(p), path_data=str(tmp_path), epl_crit=2.e-3, epl_start=1.e-3, epl_max=0.03,
                 depl=1.e-3, wh_data=True)
    check_md(db.mat_data, z, 'js_leg_md_' if layout == 'legacy' else 'js_new_md_')


def test_read_json_js_mode(z, tmp_path):
    import pylabfea_amd as FE
    kw = dict(epl_crit=2.e-3, epl_start=1.e-3, epl_max=0.03, depl=1.e-3, wh_data=True)
    p = js_json(z, str(tmp_path / 'js.json'), 'legacy', mode='JS')
    k = str(z['js_keys'][0])
    if len(k.split('_')) < 8:   # the RS key layout has no JS fields to parse: read only the components
        db = FE.Data.__new__(FE.Data)
        db.mode, db.mat_data = 'JS', {'tx_data': False}
        lc = db.read_data(p)
        rs = FE.Data.__new__(FE.Data)
        rs.mode, rs.mat_data = 'RS', {'tx_data': False}
        lc2 = rs.read_data(js_json(z, str(tmp_path / 'rs.json'), 'legacy'))
        for key in lc:
            assert np.array_equal(lc[key]['Stress'], lc2[key]['Stress'])
            assert np.array_equal(lc[key]['Strain_Plastic'], lc2[key]['Strain_Plastic'])


def test_plastic_strains_reconstructed_without_ep(tmp_path):
    """no plastic strains in the file: elastic fit at 90 % of the transition index, then ln-strain differences"""
    import pylabfea_amd as FE
    E, nu = 200e3, 0.3
    m = FE.Material()
    m.elasticity(E=E, nu=nu)
    SV = np.linalg.inv(m.CV)
    rng = np.random.default_rng(5)
    data = {}
    for lc in range(8):
        u = rng.normal(size=6)
        u /= FE.sig_eq_j2(u)
        seq = np.concatenate([np.linspace(0., 100., 60), 100. + 2000. * np.linspace(0., 0.02, 120)[1:] ** 1.])
        ep = np.concatenate([np.zeros(60), np.linspace(0., 0.02, 120)[1:]])
        sig = seq[:, None] * u[None, :]
        eps = sig @ SV.T + ep[:, None] * (1.5 * np.r_[u[:3] - u[:3].mean(), 2 * u[3:]] / FE.sig_eq_j2(u))[None, :]
        data['Us_lc%d_x_y_z' % lc] = {'Results': dict(
            **{'S' + c: list(sig[:, k]) for k, c in enumerate(COMP)},
            **{'E' + c: list(eps[:, k]) for k, c in enumerate(COMP)})}
    p = tmp_path / 'noep.json'
    p.write_text(json.dumps(data))
    db = FE.Data.__new__(FE.Data)
    db.mode, db.mat_data = 'RS', {'tx_data': False}
    lc = db.read_data(str(p))
    for key, v in lc.items():
        el = v['Stress'] @ SV.T
        want = np.exp(np.log(1. + v['Strain_Total']) - np.log(1. + el)) - 1.
        assert np.max(np.abs(v['Strain_Plastic'] - want)) < 1e-8


def test_convert_data_and_from_data_goss_barlat(z):
    import pylabfea_amd as FE
    d = FE.Data(z['gb_sig'], mat_name='Goss-Barlat', wh_data=False)
    md = d.mat_data
    assert md['wh_data'] is False and md['elast_const'] is None and md['peeq_max'] == 0.
    assert md['Nlc'] == int(z['gb_Nlc']) and np.array_equal(md['lc_indices'], z['gb_lc_indices'])
    assert abs(md['sy_av'] - float(z['gb_sy_av'])) < 1e-12 * float(z['gb_sy_av'])
    m = FE.Material('ML-Goss-Barlat')
    m.from_data(md)
    assert m.Nset == 1 and m.whdat is False and m.Ndof == 6 and m.sdim == 6 and m.CV is None
    assert m.sy == md['sy_av']
    m.elasticity(C11=float(z['gb_C11']), C12=float(z['gb_C12']), C44=float(z['gb_C44']))
    Nlc, N0, xt, yt = m._create_data_for_ms(Ce=float(z['gb_Ce']), Fe=float(z['gb_Fe']), Nseq=int(z['gb_Nseq']),
                                            extend=False)
    seq = z['gb_seq']
    assert np.array_equal(xt, (seq[:, None, None] * z['gb_sig'][None]).reshape(-1, 6))
    assert np.array_equal(yt, np.repeat(np.where(np.arange(len(seq)) < int(z['gb_Nseq']), -1., 1.), len(z['gb_sig'])))


def test_from_data_and_training_rows_work_hardening(z):
    import pylabfea_amd as FE
    dd = FE.Data(wh_lc_data(z), epl_start=0.0, epl_crit=0.0, epl_max=float(z['wh_epl_max']), depl=float(z['wh_depl']))
    m = FE.Material('ML')
    m.from_data(dd.mat_data)
    assert m.whdat and m.Ndof == 15 and m.ind_wh == 6 and m.Nset == 1 and m.epc == dd.mat_data['epc']
    assert np.array_equal(m.CV, dd.mat_data['elast_const']) and m.sy == dd.mat_data['sy_av']
    Nseq = int(z['wh_Nseq'])
    Nlc, N0, xt, yt = m._create_data_for_ms(Ce=0.99, Fe=0.1, Nseq=Nseq, extend=False)
    fs, ep = dd.mat_data['flow_stress'], dd.mat_data['plastic_strain']
    Nd = len(fs)
    assert xt.shape == (2 * Nseq * Nd, 15) and Nlc == dd.mat_data['Nlc'] and N0 == Nlc * 2 * Nseq
    seq = z['wh_seq']
    for j in (0, Nseq - 1, Nseq, 2 * Nseq - 1):   # row i + j Ndinp: flow stress i scaled by seq[j], its plastic strain
        assert np.array_equal(xt[j * Nd:(j + 1) * Nd, 0:6], fs * seq[j])
        assert np.array_equal(xt[j * Nd:(j + 1) * Nd, 6:12], ep)
    assert not np.any(xt[:, 12:])
    # the scaled features handed to the fit equal the reference's bit for bit (rebuilt from the stored parse outputs)
    m.scale_seq, m.scale_wh = float(z['wh_scale_seq']), float(z['wh_scale_wh'])
    assert abs(m.scale_seq - dd.mat_data['sy_av']) < 1e-12 * m.scale_seq   # J2 stress: Voigt form vs eigen-solve
    assert abs(m.scale_wh - dd.mat_data['peeq_max']) < 1e-12
    X = m.create_scaled_input(xt[:, 0:6], xt[:, 6:12], xt[:, 12], xt[:, 13], xt[:, 14])
    Xr = np.zeros_like(X)
    Xr[:, 0:6] = (seq[:, None, None] * z['wh_md_flow_stress'][None]).reshape(-1, 6) / float(z['wh_scale_seq'])
    Xr[:, 6:12] = np.tile(z['wh_md_plastic_strain'], (2 * Nseq, 1)) / float(z['wh_scale_wh'])
    assert np.array_equal(X, Xr)


def test_refusals(z, tmp_path):
    import pylabfea_amd as FE
    from pylabfea_amd.data import get_elastic_coefficients
    with pytest.raises(NotImplementedError):
        FE.Data(z['gb_sig'], tx_data=True)
    with pytest.raises(NotImplementedError):
        FE.Data(z['gb_sig'], plot=True)
    with pytest.raises(ValueError):
        FE.Data(z['gb_sig'], sdim=4)
    with pytest.raises(ValueError):
        FE.Data(3.)
    with pytest.raises(NotImplementedError):
        get_elastic_coefficients(np.eye(6), np.eye(6), method='decomposition')
    md = FE.Data(z['gb_sig'], wh_data=False).mat_data
    with pytest.raises(NotImplementedError):
        FE.Material().from_data([md, md])                       # several data sets (textures)
    with pytest.raises(NotImplementedError):
        FE.Material().from_data(dict(md, tx_data=True))
    with pytest.raises(NotImplementedError):
        FE.Material().from_data(dict(md, sdim=3, wh_data=True))  # 8 work-hardening features: no kernel
    m = FE.Material()
    m.msparam = [dict(md)]                                      # not installed by from_data
    with pytest.raises(NotImplementedError, match='msparam'):
        m.train_SVC(C=2, gamma=1)
    m = FE.Material()
    m.from_data(dict(md))
    m.msparam[0].pop('sy_av')                                   # fields missing
    with pytest.raises(NotImplementedError, match='msparam'):
        m.train_SVC(C=2, gamma=1)
    m = FE.Material()
    m.from_data(md)
    for kw in (dict(pca=object()), dict(scaler=object()), dict(train_index=[0]), dict(test_index=[0])):
        with pytest.raises(NotImplementedError):
            m.train_SVC(C=2, gamma=1, **kw)
    m.txdat = True
    with pytest.raises(NotImplementedError):
        m.train_SVC(C=2, gamma=1)

"""Stress-strain data for training SVC yield functions with work hardening or texture (pylabfea/data.py of the reference;
of its texture descriptors the GSH coefficients, not the PCA-reduced address vectors), in NumPy only: no SciPy, no
scikit-learn.

``Data`` reads a JSON database of virtual or physical mechanical tests (both record layouts of the reference), takes
load-case dictionaries as ``examples/train_hardening.py`` builds them, or yield stresses alone, and leaves in
``mat_data`` what ``Material.from_data`` needs: flow stresses with their plastic strains, the averaged yield strength,
elastic constants and the strain bounds of the data.  The training itself runs on the GPU (``Material.train_SVC``).
"""
import json
import os
import warnings

import numpy as np

from .basic import eps_eq, sig_eq_j2, sig_princ

_COMP = ('11', '22', '33', '23', '13', '12')


def ln_strain(eng_strain):
    """logarithmic strain of an engineering strain, with 1 + e clipped at 1e-10 (data.py:29-34)"""
    h2 = np.ones_like(eng_strain) + eng_strain
    h2[np.nonzero(h2 < 1.e-10)] = 1.e-10
    return np.log(h2)


def eng_strain(ln_strain):
    """engineering strain of a logarithmic strain (data.py:37-38)"""
    return np.exp(ln_strain) - np.ones_like(ln_strain)


def interpolate_stress(s0, s1, e0, e1, et):
    """linear interpolation of the stress at strain et between (e0, s0) and (e1, s1)"""
    return s0 + (et - e0) * (s1 - s0) / (e1 - e0)


def savgol_deriv1(x, window_length):
    """First derivative by a Savitzky-Golay filter of polynomial order 1 (unit sample spacing), with the edge treatment
    of SciPy's ``savgol_filter(x, window_length, 1, deriv=1)`` in its default mode 'interp': interior points by the
    least-squares slope of the window around them (for an even window the one SciPy's correlation picks), the first and
    last ``window_length // 2`` points by the slope of a straight line fitted to the first or last window."""
    x = np.asarray(x, dtype=float)
    n, w = len(x), int(window_length)
    if w < 2 or w > n:
        raise ValueError('savgol_deriv1: window_length must lie in [2, len(x)] (got %d for %d values)' % (w, n))
    h = w // 2
    pos = h - 0.5 if w % 2 == 0 else float(h)
    t = np.arange(w) - pos
    c = t / np.sum(t * t)        # y[i] = sum_k c[k] x[i - lo + k] (zero outside: edges replaced below)
    lo = h if w % 2 else h - 1   # an even window reaches one further right than left, as SciPy's convolution places it
    xp = np.concatenate([np.zeros(lo), x, np.zeros(w)])
    y = np.zeros(n)
    for k in range(w):
        y += c[k] * xp[k:k + n]
    u = np.arange(w) - (w - 1) / 2.
    su = np.sum(u * u)
    y[:h] = np.sum(u * x[:w]) / su
    y[n - h:] = np.sum(u * x[n - w:]) / su
    return y


def find_transition_index(stress):
    """Index at which the equivalent stress along a load path leaves the linear regime (data.py:45-81): the second
    derivative, from two Savitzky-Golay passes, departs from its mean in the elastic regime by more than 20 %."""
    nst = len(stress)
    wl1 = max(5, int(nst / 10))
    wl2 = max(2, int(nst / 50))
    sig_d2 = savgol_deriv1(savgol_deriv1(stress, wl1), wl2)
    i0 = int(nst / 10)
    tol = np.mean(sig_d2[i0:i0 + wl2]) * 1.2
    idx = -1
    iend = int((nst - i0) / wl2) - 1
    for i in range(1, iend):
        mav = np.mean(sig_d2[i0 + i * wl2:i0 + (i + 1) * wl2])
        if np.abs(mav) > tol:
            idx = i0 + i * wl2
            break
    if idx < 0:
        print('Warning: Transition not determined properly')
        idx = i0
    return idx


def get_elastic_coefficients(eps, sig, method='least_square', initial_guess=None):
    """Symmetric 6 x 6 stiffness matrix fitted to pairs of elastic strain and stress (data.py:84-348, method
    'least_square'): the 21 independent coefficients by linear least squares over all pairs.  The reference passes the
    pairs through ``random.sample``, an unseeded permutation of the rows; they are taken in their natural order here,
    which changes the result by rounding only.  Method 'decomposition' (a penalised L-BFGS-B fit) is not supported."""
    if method == 'decomposition':
        raise NotImplementedError("get_elastic_coefficients: method 'decomposition' is not supported; "
                                  "use 'least_square'")
    if method != 'least_square':
        raise ValueError("Invalid method selected. Choose 'least_square' or 'decomposition'.")
    eps = np.asarray(eps, dtype=float).reshape(-1, 6)
    sig = np.asarray(sig, dtype=float).reshape(-1, 6)
    iu = np.triu_indices(6)
    col = np.zeros((6, 6), dtype=int)    # column of coefficient C_rc in the 21 unknowns (row-major upper triangle)
    col[iu] = np.arange(21)
    col[(iu[1], iu[0])] = np.arange(21)
    npair = len(eps)
    A = np.zeros((6 * npair, 21))
    for r in range(6):
        A[r::6][:, col[r]] = eps
    b = sig.reshape(-1)
    C_flat = np.linalg.lstsq(A, b, rcond=None)[0]
    C = np.zeros((6, 6))
    C[iu] = C_flat
    C[(iu[1], iu[0])] = C_flat
    return C


class Data(object):
    """Data of mechanical tests for training ML flow rules (data.py:351-925 of the reference).

    ``source`` is the name of a JSON database (read from ``path_data``), a dictionary of load cases (key -> dict with
    'Stress', 'Eq_Stress', 'Strain_Plastic', 'Eq_Strain_Plastic', 'Strain_Total'), or an (N, sdim) array of yield
    stresses.  ``mat_data`` then holds, among others, ``flow_stress`` / ``plastic_strain`` (the training data of
    work hardening), ``sig_ideal`` (stresses at yield onset), ``sy_av``, ``elast_const``, ``epc``, ``peeq_max`` and
    ``Nlc``.  With ``tx_data=True`` and ``tx_descriptor='GSH_n'`` (n = 3, 7, 12 or 37) a JSON database's ``Texture`` entry
    gives ``texture`` (its ``gsh_coeff_reconstructed_random[1:1 + n]``) and ``tdim = n`` (data.py:522-545); the address-vector
    descriptors ``ADV_*`` (reduced by a PCA in training) and ``VF`` (not implemented in the reference either) are refused,
    and so is plotting."""

    def __init__(self, source, path_data='./', name='Dataset', mat_name="Simulanium", sdim=6, epl_crit=None,
                 epl_start=None, epl_max=None, depl=0., plot=False, wh_data=True, tx_data=False,
                 texture_name='Random', tx_descriptor='GSH_3', mode='RS'):
        if sdim != 3 and sdim != 6:
            raise ValueError('Value of sdim must be either 3 or 6')
        self._gsh_dim = None
        if tx_data:
            self._gsh_dim = self._descriptor_dim(tx_descriptor)
            if not isinstance(source, str):
                raise NotImplementedError('Data: tx_data=True needs a JSON database with a "Texture" entry; stress arrays '
                                          'and load-case dictionaries carry no texture descriptor')
        if plot:
            raise NotImplementedError('Data: plotting is not supported')
        self.lc_data = None
        self.mat_data = dict(epc=epl_crit, ep_start=epl_start, ep_max=epl_max, delta_ep=depl, sdim=sdim, tdim=0,
                             Name=mat_name, Dataset=name, wh_data=wh_data, tx_data=tx_data, Ntext=1,
                             tx_name=texture_name, tx_index=0, texture=np.zeros(1), tx_descriptor=tx_descriptor,
                             tx_key=None)
        self.mode = mode
        if isinstance(source, str):
            self.lc_data = self.read_data(os.path.join(path_data, source))
            self.parse_data(epl_crit, epl_start, epl_max, depl)
        elif isinstance(source, dict):
            self.lc_data = source
            self.parse_data(epl_crit, epl_start, epl_max, depl)
        elif isinstance(source, (list, np.ndarray)):
            print('WARNING: This data type will be no longer supported.')
            self.convert_data(np.array(source))
        else:
            raise ValueError('Only sources of type "str" or "dict" are supported.')

    @staticmethod
    def _descriptor_dim(tx_descriptor):
        """number of GSH coefficients of a descriptor name 'GSH_n' (data.py:531-537); other descriptors are refused"""
        tx_descriptor = str(tx_descriptor)
        if 'GSH' in tx_descriptor:
            gsh_dim = int(tx_descriptor.split('_')[-1])
            if gsh_dim not in (3, 7, 12, 37):
                raise ValueError(f"GSH with {gsh_dim} not valid. Must be 3, 7, 12, ")
            return gsh_dim
        if 'ADV' in tx_descriptor:
            raise NotImplementedError('Data: address-vector descriptors (%s) are reduced by a PCA in the reference\'s '
                                      'training, which is not supported; use GSH_3, GSH_7, GSH_12 or GSH_37' % tx_descriptor)
        if tx_descriptor == 'VF':
            raise NotImplementedError('Data: the volume-fraction descriptor VF is not implemented (nor is it in the reference)')
        raise ValueError('Data: unknown texture descriptor %r; GSH_3, GSH_7, GSH_12 or GSH_37 expected' % tx_descriptor)

    def _seq(self, sig):
        """J2 equivalent stress of Voigt stresses.  Data sets with texture descriptors are stacked by train_SVC into rows
        that are held to the reference's bit for bit, so for them the reference's own form is taken: through the principal
        stresses of ``sig_princ`` (the same LAPACK call), which rounds differently from the direct Voigt form in the last
        place."""
        if self.mat_data['tx_data']:
            sig = np.asarray(sig, dtype=float)
            sp = sig_princ(sig)[0]
            return sig_eq_j2(sp)
        return sig_eq_j2(sig)

    def key_parser(self, key):
        parameters = key.split('_')
        if self.mode == 'RS':
            return {"Stress_Type": parameters[0], "Load_Type": parameters[1], "Hash_Load": parameters[2],
                    "Hash_Orientation": parameters[3], "Texture_Type": parameters[4]}
        if self.mode == 'JS':
            return {"Stress_Type": parameters[0], "Load_Type": parameters[1], "Hash_Load": parameters[2],
                    "Hash_Orientation": parameters[5], "Texture_Type": parameters[7], "N_Grains": parameters[3],
                    "Elements_Grain": parameters[4]}
        raise KeyError(f"Mode is: {self.mode}. Must be RS or JS")

    def add_data(self, data_file, path_data='./'):
        self.lc_data.update(self.read_data(os.path.join(path_data, data_file)))
        self.parse_data(self.mat_data['epc'], self.mat_data['ep_start'], self.mat_data['ep_max'],
                        self.mat_data['delta_ep'])

    def add2mat_data(self, data_dict, key):
        """add one load case and parse the data again with the stored strain bounds"""
        self.lc_data[key] = data_dict
        self.parse_data(self.mat_data['epc'], self.mat_data['ep_start'], self.mat_data['ep_max'],
                        self.mat_data['delta_ep'])

    def _legacy(self, res, pre):
        shear = ('32', '13', '12') if self.mode == 'JS' else ('23', '13', '12')
        return np.array([res[pre + c] for c in ('11', '22', '33') + shear]).T

    @staticmethod
    def _layout(block, prev):
        # component arrays of the newer layout by the index in their name; components that are missing keep the value
        # of the previous tensor read for this record (the reference reuses its list)
        tens = list(prev)
        for ind, vals in block.items():
            for k, c in enumerate(_COMP):
                if c in ind:
                    tens[k] = vals
                    break
        return tens

    def read_data(self, data_file):
        """JSON database -> dict of load cases with stress, plastic and total strain (data.py:500-705).  Both record
        layouts: the legacy 'Results' (S11 ..., E11 ..., optional Ep11 ...; component order of ``mode``) and the newer
        'stress' / 'total_strain' / 'plastic_strain' with 'units' (MPa or GPa).  Without plastic strains in the data
        they are reconstructed from an elastic fit to the linear part of every curve (logarithmic strains)."""
        print("Reading data from", data_file)
        with open(data_file) as fp:
            data = json.load(fp)
        final = dict()
        elstrain, elstress = [], []
        e_plastic = False
        for num, (key, val) in enumerate(data.items()):
            if key == 'Texture':
                self.mat_data['tx_name'] = val['name']
                self.mat_data['tx_index'] = val.get('texture_index', 0)
                if not self.mat_data['tx_data']:
                    warnings.warn("WARNING: tx_data was set to false. I will just include qualitative texture info.")
                else:
                    self.mat_data['texture'] = np.array(val['gsh_coeff_reconstructed_random'],
                                                        dtype=float)[1:1 + self._gsh_dim]
                    self.mat_data['tdim'] = len(self.mat_data['texture'])
                continue
            if 'Results' in val.keys():
                res = val['Results']
                if 'cyl' in key:
                    final[key] = {"Stress": res}
                    continue
                stress = self._legacy(res, 'S')
                strain_t = self._legacy(res, 'E')
                strain_p = self._legacy(res, 'Ep') if "Ep11" in res.keys() else None
            else:
                tens = self._layout(val['stress'], [1] * 6)
                stress = np.array(tens).T
                if "units" in val.keys():
                    unit = val['units']['Stress']
                    if unit == 'MPa':
                        sfct = 1.
                    elif unit == 'GPa':
                        sfct = 1000.
                    else:
                        raise ValueError(f"Cannot convert stress unit {unit}. "
                                         f"Data must be provided either im MPa or in GPa.")
                else:
                    sfct = 1.
                    print('Warning: No units for stresses are given. Assuming MPa.')
                stress = stress * sfct
                tens = self._layout(val['total_strain'], [1] * 6)
                strain_t = np.array(tens).T
                strain_p = np.array(self._layout(val['plastic_strain'], tens)).T if "plastic_strain" in val.keys() \
                    else None
            seq_full = self._seq(stress)
            if strain_p is not None:
                peeq_plastic = eps_eq(strain_p)
                e_plastic = True
            else:
                it = find_transition_index(seq_full)
                if it < 10:
                    continue
                it = int(it * 0.9)   # safety margin: strains purely elastic
                elstrain.append(strain_t[it, :])
                elstress.append(stress[it, :])
                peeq_plastic = None
            final[key] = {"Stress": stress, "Eq_Stress": seq_full, "Strain_Plastic": strain_p,
                          "Eq_Strain_Plastic": peeq_plastic, "Strain_Total": strain_t, "Eq_Strain_Total": eps_eq(strain_t),
                          "Index": num}
            if "identifier" in val.keys():
                final[key]["identifier"] = val["identifier"]
                if "input_path" in val.keys():
                    final[key]["input_path"] = val["input_path"]
                if "load_case" in val.keys():
                    final[key]["load_case"] = val["load_case"]
                elif "load_case" in val["mechanical_BC"][0].keys():
                    final[key]["load_case"] = val["mechanical_BC"][0]["load_case"]
        if not e_plastic:
            SV = np.linalg.inv(get_elastic_coefficients(elstrain, elstress, method='least_square'))
            for key, val in final.items():
                stress, strain_t = val['Stress'], val['Strain_Total']
                E_pl = eng_strain(ln_strain(strain_t) - ln_strain(stress @ SV.T))
                val["Strain_Plastic"] = E_pl
                val["Eq_Strain_Plastic"] = eps_eq(E_pl)
            print('Plastic strains are reconstructed from linear part of stress strain data.')
        return final

    def parse_data(self, epl_crit, epl_start, epl_max, depl):
        """Load cases -> mat_data (data.py:706-888): per load case the transition index, yield onset at epl_crit, the
        flow stresses with plastic strains between epl_start and epl_max (at least depl apart, strains scaled by
        max(0, 1 - epc / peeq)); elastic constants fitted over all load cases; averages of the strain bounds."""
        Nlc = len(self.lc_data.keys())
        Ncyl = 0
        peeq_max = 0.
        ct = 0
        ep_c = ep_s = ep_m = 0.0
        sig, epl, sig_ideal = [], [], []
        lc_ind_list = np.zeros(Nlc + 1, dtype=int)
        elstrain, elstress, it_list = [], [], []
        for key, val in self.lc_data.items():
            if 'cyl' in key:
                Ncyl += 1
                ct += 1
                sig_ideal.append(val['Stress'])
                continue
            it = find_transition_index(val["Eq_Stress"])
            elstrain.append(val['Strain_Total'][it] - val['Strain_Plastic'][it])
            elstress.append(val['Stress'][it])
            peeq = val['Eq_Strain_Plastic']
            if epl_crit is None:
                epc_lc = max(peeq[it] * 1.1, 0.002)
                print(f'Critical value for plastic strain at start of plastic regime set to epl_crit={epc_lc * 100}%')
                if epl_start is not None:
                    print('WARNING: Value for "epl_start" has been given, but not for "epl_crit".')
                    if epl_start > epc_lc:
                        raise ValueError(f'Value of epl_start={epl_start} is larger than epl_crit={epc_lc}.')
            else:
                epc_lc = epl_crit
            if epl_start is None:
                eps_lc = peeq[it]
                print(f'Critical value for plastic strain at end of elastic regime set to epl_crit={eps_lc * 100}%')
            else:
                eps_lc = epl_start
                if epl_start > epc_lc:
                    raise ValueError(f'Value of epl_start={epl_start} is larger than epl_crit={epc_lc}.')
            epm_lc = max(peeq) if epl_max is None else epl_max
            i_ideal = np.nonzero(peeq <= epc_lc)[0]
            if len(i_ideal) < 2:
                print(f'Skipping data set {key} (No {ct}): No elastic range before yield onset.')
                Nlc -= 1
                continue
            if len(i_ideal) >= len(peeq) - 2:
                print(f'Skipping data set {key} (No {ct}): Plastic range after yield onset not sufficient.')
                Nlc -= 1
                continue
            iel = np.nonzero(peeq <= eps_lc)[0]
            ipl = np.nonzero(np.logical_and(peeq > eps_lc, peeq <= epm_lc))[0]
            if len(iel) < 2:
                print(f'Skipping data set {key} (No {ct}): No elastic range: IEL: {iel}, vals: {len(peeq)}')
                Nlc -= 1
                continue
            if len(ipl) < 2:
                print(f'Skipping data set {key} (No {ct}): No plastic range: IPL: {ipl}, vals: {len(peeq)}; '
                      f'{eps_lc}, {epm_lc}')
                Nlc -= 1
                continue
            it_list.append([it, int(i_ideal[-1]), int(iel[-1]), int(ipl[0])])
            ep_c += epc_lc
            ep_s += eps_lc
            ep_m += epm_lc
            idx = i_ideal[-1]
            s_crit = interpolate_stress(s0=val['Eq_Stress'][idx], s1=val['Eq_Stress'][idx + 1], e0=peeq[idx],
                                        e1=peeq[idx + 1], et=epc_lc)
            sig_ideal.append(val['Stress'][idx] * s_crit / self._seq(val['Stress'][idx]))
            if peeq[ipl[-1]] > peeq_max:
                peeq_max = peeq[ipl[-1]]
            eps = -depl
            nv = 0
            for i in ipl:
                hh = peeq[i]
                if hh >= eps + depl:
                    sig.append(val['Stress'][i])
                    epl.append(val['Strain_Plastic'][i] * max(0., 1. - epc_lc / hh))
                    eps = hh
                    nv += 1
            nz = np.nonzero(lc_ind_list)[0]
            lc_ind_list[ct] = nv + (lc_ind_list[nz[-1]] if nz.size > 0 else 0)
            if self.mode == 'JS':
                self.mat_data['tx_key'] = self.key_parser(key)["Hash_Orientation"]
            else:
                self.mat_data['ms_type'] = 'unknown'
                self.mat_data['tx_key'] = 'unknown'
            ct += 1
        C = get_elastic_coefficients(elstrain, elstress, method='least_square')
        sy_av = np.mean(self._seq(np.array(sig_ideal)))
        nreal = Nlc - Ncyl
        md = self.mat_data
        md['flow_stress'] = np.array(sig)
        md['plastic_strain'] = np.array(epl)
        md['lc_indices'] = lc_ind_list
        md['epc'] = ep_c / nreal
        md['ep_start'] = ep_s / nreal
        md['ep_max'] = ep_m / nreal
        md['peeq_max'] = peeq_max - ep_c / nreal
        md['elast_const'] = C
        md['sy_av'] = sy_av
        md['Nlc'] = Nlc
        md['Ncyl'] = Ncyl
        md['sig_ideal'] = np.array(sig_ideal)
        md['elstress'] = elstress
        md['elstrain'] = elstrain
        md['transition_ind'] = it_list
        print(f'\n###   Data set: {md["Name"]}  ###')
        print(f'Estimated elastic constants (in GPa): C={C * 1.E-3}')
        print(f'Estimated yield strength: {sy_av:5.2f} MPa at PEEQ = {(ep_s / Nlc):5.3f}')

    def convert_data(self, sig):
        """yield stresses only -> mat_data (data.py:890-914): no work-hardening data, no elastic constants"""
        Nlc = len(sig)
        if len(sig[0, :]) != self.mat_data['sdim']:
            warnings.warn('Warning: dimension of stress in data does not agree with parameter sdim. Use value from data.')
        md = self.mat_data
        md['sig_ideal'] = sig
        md['wh_data'] = False
        md['lc_indices'] = np.append(np.linspace(0, Nlc), 0.)
        md['elast_const'] = None
        md['sy_av'] = np.mean(sig_eq_j2(sig))
        md['peeq_max'] = 0.0
        md['Nlc'] = Nlc
        print(f'\n###   Data set: {md["Name"]}  ###')
        print(f'Converted data for {Nlc} stress tensors at yield onset into material data.')
        print('WARNING: Elastic parameters cannot be derived from data. Please set them manually.')

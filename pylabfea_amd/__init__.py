"""pylabfea_amd — MI355X-native engine for pyLabFEA's elastic-plastic hot path.

Drop-in for the path ``Model.solve() -> Element -> Material.response()`` of pyLabFEA v4.4.2:
the per-element return mapping, the B^T D B assembly and the linear solve run as hand-written
HIP kernels (gfx950) in ``libplfx.so`` behind the reference's own ``Model`` / ``Material`` API.
See DESIGN.md for the scope table and INTEGRATION.md for the C-ABI.
"""
from .basic import (Strain, Stress, eps_eq, sig_cyl2princ, sig_dev, sig_eq_j2, sig_polar_ang, sig_princ, sig_princ2cyl,
                    sig_spherical_to_cartesian,
                    yf_tolerance)
from .basic import polar_ang, s_cyl, sdev, seq_J2, sp_cart, sprinc
from .committee import Committee, active_learning, train_committee
from .data import Data
from .material import Material
from .model import Model
from .training import create_test_sig, load_cases, training_score
from ._dist import host_transport

__version__ = '0.1.0'
__all__ = ['Data', 'Material', 'Model', 'host_transport', 'Stress', 'Strain', 'eps_eq', 'sig_dev', 'sig_eq_j2', 'sig_polar_ang', 'sig_princ',
           'yf_tolerance', 'sig_cyl2princ', 'load_cases', 'training_score', 'Committee', 'train_committee', 'active_learning',
           'sig_spherical_to_cartesian', 'sig_princ2cyl', 'create_test_sig', 'seq_J2', 'sprinc', 'sp_cart', 's_cyl', 'sdev',
           'polar_ang']

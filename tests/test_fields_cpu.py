"""Model.field / field_range without a GPU: the fixture tests/golden/model_fields.npz (tools/gen_model_fields.py, the
unmodified reference) against the façade's pure-Python auto-scale helper, and the three lists of selector names."""
import os
import re

import numpy as np
import pytest

from pylabfea_amd import _lib
from pylabfea_amd.model import FIELD_SELECTORS, autoscale_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('a', 'b', 'c', 'd')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'model_fields.npz'))


def branch_of(lo, hi):
    """the branch of model.py:1700-1716 by its effect on the limits: 0 none, 1 +-0.05, 2 positive, 3 negative"""
    a, b = autoscale_range(lo, hi)
    if (a, b) == (lo, hi):
        return 0
    if (a, b) == (lo - 0.05, hi + 0.05):
        return 1
    return 2 if (a, b) == (lo * 0.98, hi * 1.02) else 3


def test_recorded_ranges_follow_from_recorded_fields(gold):
    """the colour-bar limits the reference's plot showed are the auto-scale helper applied to np.amin / np.amax of the
    recorded field.  The helper repeats plot's own operations; the recorded limits have in addition passed through
    matplotlib's Normalize and its inverse on the way to the colour bar's axis (vmin + t (vmax - vmin): a subtraction, a
    product and a sum, one rounding each of numbers no larger than the limits), hence 4 ulp of the larger limit."""
    for c in CASES:
        for s in FIELD_SELECTORS:
            f = gold['%s_f_%s' % (c, s)]
            assert f.shape == gold[c + '_sig'].shape[:1] and f.size <= 64
            got = autoscale_range(float(np.amin(f)), float(np.amax(f)))
            want = tuple(float(x) for x in gold['%s_r_%s' % (c, s)])
            bar = 4 * 2.2e-16 * max(abs(want[0]), abs(want[1]))
            assert abs(got[0] - want[0]) <= bar and abs(got[1] - want[1]) <= bar, (c, s, got, want)
            assert branch_of(float(np.amin(f)), float(np.amax(f))) == int(gold['%s_branch_%s' % (c, s)]), (c, s)


def test_every_autoscale_branch_occurs(gold):
    seen = {int(gold['%s_branch_%s' % (c, s)]) for c in CASES for s in FIELD_SELECTORS}
    assert seen == {0, 1, 2, 3}
    # the negative branch: x 0.98 on the maximum, x 1.02 on the minimum
    assert autoscale_range(-0.4, -0.2) == (-0.4 * 1.02, -0.2 * 0.98)
    assert autoscale_range(-0.4, -0.2, auto_scale=False) == (-0.4, -0.2)
    assert all(np.isnan(x) for x in autoscale_range(np.nan, np.nan))


def test_selector_lists_agree(gold):
    """the façade's selectors = the header's PLFX_FIELD_* constants in the order of their values, plus the host-side
    'mat' = the keys of the fixture"""
    txt = open(os.path.join(ROOT, 'include', 'plfx.h')).read()
    hdr = sorted(((int(v), n) for n, v in re.findall(r'\bPLFX_FIELD_([A-Z0-9]+)\s*=\s*(\d+)', txt)))
    assert [v for v, _ in hdr] == list(range(len(hdr))) and len(hdr) == 15
    assert [n.lower() for _, n in hdr] == [n.lower() for n in _lib.FIELD_NAMES]
    assert FIELD_SELECTORS == _lib.FIELD_NAMES + ('mat',)
    assert [_lib.FIELD_ID[n] for n in _lib.FIELD_NAMES] == list(range(15))
    assert tuple(str(s) for s in gold['selectors']) == FIELD_SELECTORS
    for c in CASES:
        keys = sorted(k[len(c) + 3:] for k in gold.files if k.startswith(c + '_f_'))
        assert keys == sorted(FIELD_SELECTORS)

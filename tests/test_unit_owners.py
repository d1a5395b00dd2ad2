"""One owning translation unit per kernel (DESIGN sections 39 and 42), checked on the objects the build leaves behind.

A kernel that is no template and is compiled in two units fails the link of libplfx.so: its host stub is a strong symbol in both.
A kernel TEMPLATE instantiated in two units links silently -- the stubs are weak -- and the library then carries the device
code twice, with a dynamic-LDS limit that one unit raises and the other launches under.  This test names kernels only (the
host stubs of the objects); it does not look into device code."""
import collections
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pylabfea_amd', 'csrc')


def makefile_units():
    m = re.search(r'^UNITS\s*:=\s*(.+)$', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M)
    assert m, 'no UNITS line in pylabfea_amd/csrc/Makefile'
    return m.group(1).split()


def kernel_stubs(obj):
    """global and weak __device_stub__ symbols of an object, by type letter"""
    out = subprocess.run(['nm', '--defined-only', obj], check=True, capture_output=True, text=True).stdout
    stubs = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) == 3 and '__device_stub__' in f[2] and f[1] in 'TW':
            stubs[f[2]] = f[1]
    return stubs


def test_every_kernel_has_one_owning_unit():
    units = makefile_units()
    assert len(units) >= 2 and 'plfx' in units, units
    owners = collections.defaultdict(list)
    for u in units:
        obj = os.path.join(CSRC, 'build', u + '.o')
        assert os.path.exists(obj), '%s is missing: run make -C pylabfea_amd/csrc' % os.path.relpath(obj, ROOT)
        stubs = kernel_stubs(obj)
        assert stubs, 'no kernel stubs in %s' % obj
        for s in stubs:
            owners[s].append(u)
    double = {s: us for s, us in owners.items() if len(us) > 1}
    assert not double, 'kernels compiled in two units (export a launcher from the owner through plfx_host.hpp):\n' + \
        '\n'.join('  %s: %s' % (s, ' '.join(us)) for s, us in sorted(double.items()))

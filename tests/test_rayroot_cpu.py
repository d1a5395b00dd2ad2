"""ray_root (pylabfea_amd/csrc/plfx_rayroot.hpp), the root search of yield_scale (k_yield_scale calls it; k_tex_yield_scale
holds the same statements written out and is held to the fixture by tests/test_gpu_texture.py), driven directly: the header
compiled into tests/rayroot_host.cpp by the host compiler, against a line-by-line Python transcription of the search, on
scalar functions whose values are single IEEE operations -- so root (all bits), status and the number of evaluations must be
EQUAL.  The kernels reach the search only through a full SVC table; here its limits and caps are aimed at.

What the cases establish beyond equality is asserted from reasoning written at each of them.  One finding: the refinement cap
cannot be reached.  A bracket comes from one march step, so it spans 2 % of x, at most 0.02 * 2^53 < 2^47.2 doubles; every
refinement puts x strictly inside (lo, hi) and replaces one end by it whatever f returns, so after at most 48 of them lo and
hi are neighbours: YS_CAP_BISECT = 80 is never counted out and status 2 is a guard, not a reachable result.  The function
that answers +1, -1, +1, ... once the bracket stands -- the worst an f can do -- ends with status 0 like any other."""
import math
import os
import shutil
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'pylabfea_amd', 'csrc')
YS_CAP_DOWN, YS_CAP_UP, YS_CAP_BISECT = 240, 90, 80
NAN = float('nan')


def ray_root(x0, f):
    """the search of plfx_rayroot.hpp, statement by statement; returns (root, status)"""
    st, phase, cnt = 0, 0, 0
    x, lo, hi, flo, fhi = x0, 0., 0., 0., 0.
    root = NAN
    while True:
        fx = f(x)
        if fx != fx:
            st = 1
            break
        if phase == 0:
            phase = 1 if fx >= 0. else 2
        if phase == 1:
            if fx < 0.:
                lo, flo, phase = x, fx, 3
            else:
                hi, fhi = x, fx
                if x < 0.01 * x0:
                    st = 1
                    break
                cnt += 1
                if cnt > YS_CAP_DOWN:
                    st = 1
                    break
                x *= 0.98
                continue
        elif phase == 2:
            if fx >= 0.:
                hi, fhi, phase = x, fx, 3
            else:
                lo, flo = x, fx
                if x > 5. * x0:
                    st = 1
                    break
                cnt += 1
                if cnt > YS_CAP_UP:
                    st = 1
                    break
                x *= 1.02
                continue
        elif fx < 0.:
            lo, flo = x, fx
        else:
            hi, fhi = x, fx
        if phase == 3:
            phase, cnt = 4, 0
        mid = lo + 0.5 * (hi - lo)
        if not (mid > lo and mid < hi):   # lo and hi are neighbours
            root = lo if -flo < fhi else hi
            break
        cnt += 1
        if cnt > YS_CAP_BISECT:
            st = 2
            break
        x = mid
    return root, st


def scalar_fn(fid, a, b, c, xs):
    """the functions of rayroot_host.cpp; every evaluation point is appended to xs"""
    seen = {'neg': False, 'pos': False, 'up': False}

    def f(x):
        xs.append(x)
        if fid == 0:
            return x - a
        if fid == 1:
            return a - x
        if fid == 2:
            return b if x >= a else -b
        if fid == 3:
            return a
        if fid == 4:
            return NAN if (b > 0. and x > a) or (b < 0. and x < a) else x - c
        if seen['neg'] and seen['pos']:
            seen['up'] = not seen['up']
            return 1. if seen['up'] else -1.
        seen['neg' if x - a < 0. else 'pos'] = True
        return x - a
    return f


def replay(case):
    """(root, status, evaluation points) of the transcription on a case (fid, a, b, c, x0)"""
    xs = []
    root, st = ray_root(case[4], scalar_fn(*case[:4], xs))
    return root, st, xs


X0 = 1.5
DOWN = replay((3, 1., 0., 0., X0))[2]    # f = +1: the whole march down, its last point the first below 0.01 x0
UP = replay((3, -1., 0., 0., X0))[2]     # f = -1: the whole march up, its last point the first above 5 x0
CASES = {
    # f = x - r, r a double inside [0.01 x0, 5 x0]: below, at and above x0, and on the first step either way
    'linear, inside': [(0, r, 0., 0., X0) for r in (0.02, 0.3, 1.2, 1.4999, X0, 1.5001, 1.7, 7.4)],
    # r outside: no bracket
    'linear, outside': [(0, r, 0., 0., X0) for r in (1e-3, 0.014, 7.7, 100.)],
    # the march ends exactly on its last allowed step: r between the last two points of the march (found on that step), and
    # just beyond the last point (not found); which step that is, the transcription says (DOWN, UP)
    'linear, last step': [(0, 0.5 * (DOWN[-1] + DOWN[-2]), 0., 0., X0), (0, DOWN[-1] * 0.999, 0., 0., X0),
                          (0, 0.5 * (UP[-1] + UP[-2]), 0., 0., X0), (0, UP[-1] * 1.001, 0., 0., X0)],
    # f = r - x: >= 0 below r, so the march down from above r never sees f < 0, and from below r it leaves downwards too
    'reversed': [(1, r, 0., 0., X0) for r in (0.3, 1.2, 1.7, 7.4)],
    # a jump from -b to +b between the double below a and a
    'step': [(2, a, b, 0., X0) for a in (1.2, 1.7, math.nextafter(1.2, 2.)) for b in (1., 0.25)],
    'constant': [(3, v, 0., 0., X0) for v in (0., -0., 1., -1., NAN)],
    # NaN beyond a point on the way up / down, the root x = c behind it; and with the root in front of it
    'nan beyond': [(4, 2., 1., 3., X0), (4, 1., -1., 0.5, X0), (4, 4., 1., 3., X0), (4, 0.2, -1., 0.5, X0)],
    # the function that stops following x once the bracket stands
    # (x0 = 2^52: as many doubles in a bracket as there can be; 2^-1044: subnormal x, the fewest)
    'alternating': [(5, r * x0, 0., 0., x0) for x0 in (X0, 2. ** 52, 2. ** -1044) for r in (0.8, 0.99, 1.3)],
}


def _compiler():
    for n in (os.environ.get('CXX') or 'c++', 'g++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++'):
        p = n if os.path.isabs(n) and os.path.exists(n) else shutil.which(n)
        if p:
            return p
    pytest.skip('no host C++ compiler found')   # a box without the toolchain skips, it does not fail


@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def program(request, tmp_path_factory):
    """tests/rayroot_host.cpp built by the host compiler; `sanitized`: under AddressSanitizer and UBSan, a stand-alone binary"""
    cxx = _compiler()
    exe = str(tmp_path_factory.mktemp('rayroot') / ('rayroot_host_' + request.param))
    cmd = [cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-I', CSRC, '-o', exe, os.path.join(HERE, 'rayroot_host.cpp')]
    if request.param == 'sanitized':
        cmd[3:3] = ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode and request.param == 'sanitized':
        pytest.skip('the compiler has no sanitizer runtime here: ' + r.stderr[-300:])
    assert r.returncode == 0, r.stderr
    return exe


def run(program, cases):
    text = ''.join('%d %s %s %s %s\n' % ((c[0],) + tuple(float(v).hex() if v == v else 'nan' for v in c[1:])) for c in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        root, st, ev = line.split()
        out.append((NAN if root == 'nan' else float.fromhex(root), int(st), int(ev)))
    assert len(out) == len(cases)
    return out


def bits(x):
    return struct.pack('<d', x) if x == x else b'nan'


@pytest.mark.parametrize('group', sorted(CASES))
def test_host_equals_transcription(program, group):
    """root bit for bit, status and number of evaluations"""
    got = run(program, CASES[group])
    for case, (root, st, ev) in zip(CASES[group], got):
        r_ref, st_ref, xs = replay(case)
        print(group, case, 'host', root, st, ev, 'transcription', r_ref, st_ref, len(xs))
        assert (bits(root), st, ev) == (bits(r_ref), st_ref, len(xs)), case


def test_what_the_cases_mean():
    """the transcription's answers, from reasoning about the search rather than from the search"""
    for case in CASES['linear, inside'] + CASES['linear, last step'][0::2]:
        root, st, xs = replay(case)
        # near r the difference x - r is exact (Sterbenz), so f vanishes at r alone and r is one end of the last bracket
        assert st == 0 and root == case[1]
        assert 0.01 * X0 * 0.98 <= min(xs) and max(xs) <= 5. * X0 * 1.02
    for case in CASES['linear, outside'] + CASES['linear, last step'][1::2] + CASES['reversed']:
        root, st, xs = replay(case)
        assert st == 1 and root != root
    # the march: down while x >= 0.01 x0 (229 points), up while x <= 5 x0 (81); both inside their caps
    assert DOWN[-2] >= 0.01 * X0 > DOWN[-1] and len(DOWN) - 1 <= YS_CAP_DOWN
    assert UP[-2] <= 5. * X0 < UP[-1] and len(UP) - 1 <= YS_CAP_UP
    for k in (0, 2):   # found on the last allowed step: no evaluation of the march is left out
        xs = replay(CASES['linear, last step'][k])[2]
        assert xs[:len(DOWN if k == 0 else UP)] == (DOWN if k == 0 else UP)
    for case in CASES['step']:
        # the bracket closes on (the double below a, a) with f = -b, +b: equal magnitudes, so the upper end is returned
        assert replay(case)[:2] == (case[1], 0)
    for case in CASES['constant']:
        root, st, xs = replay(case)
        v = case[1]
        assert st == 1 and root != root and len(xs) == (1 if v != v else len(DOWN) if v >= 0. else len(UP))
    for case, st_want in zip(CASES['nan beyond'], (1, 1, 0, 0)):
        root, st, xs = replay(case)
        assert st == st_want and (root == case[3] if st == 0 else root != root)
    for case in CASES['alternating']:
        # status 2 cannot be reached (module docstring): at most 48 refinements, then the ends are neighbours
        root, st, xs = replay(case)
        below = [x - case[1] < 0. for x in xs]
        march = below.index(not below[0]) + 1   # evaluations up to the one that closes the bracket
        assert st == 0 and len(xs) - march <= 48 < YS_CAP_BISECT

#!/usr/bin/env python3
"""Device assembly of one build of libplfx.so against another, kernel by kernel (DESIGN sections 39 and 42; the method of
profiles/r16a_kernel_resources.txt, r39_kernel_resources.txt and r42_kernel_resources.txt).  For a change that must not move
device code -- a unit cut off, functions reordered in plfx_step.hip, where the order in which the row kernels are first named
decides their registers.  One .s file per translation unit on either side:

    hipcc --offload-arch=gfx950 --cuda-device-only -O3 -std=c++17 -S -o <unit>.s pylabfea_amd/csrc/<unit>.hip
    python tools/kernel_resources_ab.py --before old/plfx.s old/plfx_step.s \\
        --after plfx.s plfx_step.s plfx_material.s plfx_solve.s [--removed k_scatter ...]

Reports whether the kernel sets are equal, kernels that occur in two units of one side (a duplicate the parent already had is
told from a new one), and every kernel whose text differs with its VGPR / SGPR / scratch / LDS figures on both sides.
--removed names kernels (plain names, as in the source) that the change deletes on purpose: they must be in the "before" set
and gone from the "after" set.  Exit status 1 if a kernel is missing, extra, double in the "after" units, or has other figures,
or if a kernel named as removed is still there or never was."""
import argparse
import collections
import os
import re
import sys

def parse(path):
    funcs, meta = {}, {}
    cur = None; kern = None
    isfunc = set()   # (data symbols such as __hip_cuid_* have labels too)
    for l in open(path, errors='replace'):
        l = l.rstrip('\n')
        m = re.match(r'^\s*\.type\s+([^,\s]+),@function', l)
        if m: isfunc.add(m.group(1))
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', l)
        if m: kern = m.group(1); meta[kern] = {}
        if kern:
            m = re.match(r'^\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size|group_segment_fixed_size|accum_offset)\s+(\S+)', l)
            if m: meta[kern][m.group(1)] = m.group(2)
            if '.end_amdhsa_kernel' in l: kern = None
        m = re.match(r'^([A-Za-z_$][\w$.]*):', l)
        if m and m.group(1) in isfunc and cur is None and not l.startswith('\t'):
            cur = m.group(1); funcs[cur] = []; continue
        if cur is not None:
            if re.match(r'^\.Lfunc_end\d+:', l):
                cur = None; continue
            s = l.split(';')[0].rstrip()
            if not s.strip(): continue
            t = s.strip()
            if t.startswith('.') and not re.match(r'^\.LBB\d+_\d+:', t): continue
            t = re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', t)
            t = re.sub(r'\.L(func_end|tmp|_unnamed)\d*_?\d*', r'.L\1', t)
            funcs[cur].append(t)
    return funcs, meta

def side(paths):
    """units, per-unit functions and kernel metadata, and the units every kernel occurs in"""
    units = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    uf, um = {}, {}
    for u, p in zip(units, paths): uf[u], um[u] = parse(p)
    where = collections.defaultdict(list)
    for u in units:
        for k in um[u]: where[k].append(u)
    return units, uf, um, where

def plain_name(mangled):
    """k_name of _ZN4plfx6k_nameE... (the source name of a kernel in namespace plfx; templates: the name before the arguments)"""
    m = re.match(r'^_ZN4plfx(\d+)', mangled)
    if not m: return mangled
    n = int(m.group(1))
    return mangled[m.end():m.end() + n]

ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
ap.add_argument('--before', nargs='+', required=True, metavar='UNIT.s')
ap.add_argument('--after', nargs='+', required=True, metavar='UNIT.s')
ap.add_argument('--removed', nargs='*', default=[], metavar='KERNEL')
a = ap.parse_args()
punits, pf, pm, pwhere = side(a.before)
units, uf, um, where = side(a.after)
out = []
for tag, us, fs, ms in (('before', punits, pf, pm), ('after', units, uf, um)):
    for u in us: out.append(f'{tag}: unit {u}: {len(ms[u])} kernels, {len(fs[u])} functions with text')
gone = {k for k in pwhere if plain_name(k) in a.removed}
bad = False
for n in a.removed:
    was = [k for k in pwhere if plain_name(k) == n]
    still = [k for k in where if plain_name(k) == n]
    out.append(f'removed on purpose: {n}: {len(was)} before, {len(still)} after')
    if not was or still: bad = True; out.append(f'  NOT REMOVED or never there: {n}')
want = set(pwhere) - gone
newk = set(where)
out.append(f'kernel names: {len(pwhere)} before, {len(newk)} after; after equals before minus the removed ones: {newk == want}')
for k in sorted(want - newk): out.append(f'  MISSING after: {k}')
for k in sorted(newk - want): out.append(f'  EXTRA after: {k}')
pdups = {k: v for k, v in pwhere.items() if len(v) > 1}
dups = {k: v for k, v in where.items() if len(v) > 1}
out.append(f'kernel names that occur in two units: {len(pdups)} before, {len(dups)} after')
for k, v in sorted(pdups.items()): out.append(f'  duplicate before {k}: {" ".join(v)}')
for k, v in sorted(dups.items()): out.append(f'  DUPLICATE after{"" if k in pdups else " (new)"} {k}: {" ".join(v)}')
keys = [('next_free_vgpr', 'vgpr'), ('next_free_sgpr', 'sgpr'), ('private_segment_fixed_size', 'scratch'), ('group_segment_fixed_size', 'lds')]
same = diff = 0
moved = collections.Counter()
for k in sorted(want & newk):
    pu = pwhere[k][0]
    for u in where[k]:
        moved[(pu, u)] += 1
        ta, tb, ma, mb = pf[pu].get(k), uf[u].get(k), pm[pu][k], um[u][k]
        if ta == tb and ma == mb: same += 1
        else:
            diff += 1
            figs = ' '.join(f"{n} {ma.get(q)}->{mb.get(q)}" for q, n in keys)
            eq = all(ma.get(q) == mb.get(q) for q, n in keys)
            out.append(f'OTHER TEXT ({pu} -> {u}) {k}')
            out.append(f'   insts {len(ta or [])} -> {len(tb or [])}, same opcode multiset: {sorted(x.split()[0] for x in ta or []) == sorted(x.split()[0] for x in tb or [])}, {figs}: {"figures equal" if eq else "FIGURES DIFFER"}')
for (pu, u), n in sorted(moved.items()): out.append(f'kernels of {pu} now in {u}: {n}')
out.append(f'kernels with identical text and identical vgpr / sgpr / scratch / LDS metadata: {same}, others: {diff}')
# non-kernel device functions (not inlined): each copy against one of the parent's
pnk = {}
for u in punits:
    for f, t in pf[u].items():
        if f not in pm[u]: pnk.setdefault(f, []).append(t)
nk_same = nk_diff = 0
for u in units:
    for f, t in uf[u].items():
        if f in um[u]: continue
        if t in pnk.get(f, []): nk_same += 1
        else:
            nk_diff += 1; out.append(f'NON-KERNEL function differs or is new: {f} ({u})')
out.append(f'non-kernel device functions in the units (a copy per unit that calls one): {nk_same} identical to a parent copy, {nk_diff} others')
print('\n'.join(out))
bad = bad or newk != want or bool(dups) or any('FIGURES DIFFER' in l for l in out)
sys.exit(1 if bad else 0)

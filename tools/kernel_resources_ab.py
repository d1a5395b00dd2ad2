#!/usr/bin/env python3
"""Device assembly of one build of libplfx.so against another, kernel by kernel (the method of
profiles/r16a_kernel_resources.txt and r39_kernel_resources.txt).  For a change that must not move device code -- a unit cut
off, functions reordered in plfx_step.hip, where the order in which the row kernels are first named decides their registers:

    hipcc --offload-arch=gfx950 --cuda-device-only -O3 -std=c++17 -S -o before.s <the unit(s) before>
    hipcc ... -S -o plfx.s pylabfea_amd/csrc/plfx.hip ; hipcc ... -S -o plfx_step.s pylabfea_amd/csrc/plfx_step.hip
    python tools/kernel_resources_ab.py before.s plfx.s plfx_step.s

Reports whether the kernel sets are equal, kernels that occur in two units, and every kernel whose text differs with its VGPR /
SGPR / scratch / LDS figures on both sides.  Exit status 1 if a kernel is missing, extra, double, or has other figures."""
import collections
import os
import re
import sys

def parse(path):
    funcs, meta = {}, {}
    cur = None; kern = None
    for l in open(path, errors='replace'):
        l = l.rstrip('\n')
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', l)
        if m: kern = m.group(1); meta[kern] = {}
        if kern:
            m = re.match(r'^\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size|group_segment_fixed_size|accum_offset)\s+(\S+)', l)
            if m: meta[kern][m.group(1)] = m.group(2)
            if '.end_amdhsa_kernel' in l: kern = None
        m = re.match(r'^([A-Za-z_$][\w$.]*):', l)
        if m and not m.group(1).startswith('.L') and cur is None and not l.startswith('\t'):
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
pf, pm = parse(sys.argv[1])
units = [os.path.splitext(os.path.basename(p))[0] for p in sys.argv[2:]]
uf, um = {}, {}
for u, p in zip(units, sys.argv[2:]): uf[u], um[u] = parse(p)
out = []
out.append(f'parent: {len(pm)} kernels, {len(pf)} functions with text')
where = collections.defaultdict(list)
for u in units:
    for k in um[u]: where[k].append(u)
    out.append(f'unit {u}: {len(um[u])} kernels, {len(uf[u])} functions')
newk = set(where)
out.append(f'union of kernel names over the units: {len(newk)}; equals the parent set: {newk == set(pm)}')
for k in sorted(set(pm) - newk): out.append(f'  MISSING in units: {k}')
for k in sorted(newk - set(pm)): out.append(f'  EXTRA in units: {k}')
dups = {k: v for k, v in where.items() if len(v) > 1}
out.append(f'kernel names that occur in two units: {len(dups)}')
for k, v in sorted(dups.items()): out.append(f'  DUPLICATE {k}: {" ".join(v)}')
same = diff = 0
for k in sorted(pm):
    for u in where.get(k, []):
        a, b = pf.get(k), uf[u].get(k)
        if a == b and pm[k] == um[u][k]: same += 1
        else:
            diff += 1
            keys = [('next_free_vgpr', 'vgpr'), ('next_free_sgpr', 'sgpr'), ('private_segment_fixed_size', 'scratch'), ('group_segment_fixed_size', 'lds')]
            figs = ' '.join(f"{n} {pm[k].get(q)}->{um[u][k].get(q)}" for q, n in keys)
            eq = all(pm[k].get(q) == um[u][k].get(q) for q, n in keys)
            out.append(f'OTHER TEXT ({u}) {k}')
            out.append(f'   insts {len(a or [])} -> {len(b or [])}, same opcode multiset: {sorted(x.split()[0] for x in a) == sorted(x.split()[0] for x in b)}, {figs}: {"figures equal" if eq else "FIGURES DIFFER"}')
out.append(f'kernels with identical text and identical vgpr / sgpr / scratch / LDS metadata: {same}, others: {diff}')
# non-kernel device functions (not inlined): each copy against the parent's
nk_same = nk_diff = 0
for u in units:
    for f, t in uf[u].items():
        if f in um[u]: continue
        if f in pf and pf[f] == t: nk_same += 1
        else:
            nk_diff += 1; out.append(f'NON-KERNEL function differs or is new: {f} ({u})')
out.append(f'non-kernel device functions in the units (a copy per unit that calls one): {nk_same} identical to the parent\'s, {nk_diff} others')
print('\n'.join(out))
bad = newk != set(pm) or dups or any('FIGURES DIFFER' in l for l in out)
sys.exit(1 if bad else 0)

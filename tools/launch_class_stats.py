#!/usr/bin/env python3
"""Medians over the last N load steps of a rocprofv3 kernel trace of bench.py (a step = the launches up to and including a
k_update_state launch): k_sweep_light<1> by its position in the step (in the headline workload the first sweep of a step
rewrites every tangent -- launch class "all" -- and the second none) and the start kernels of a solve (k_cg_start<1>,
k_cg_start_test<1>, k_cg_start_pred).  With the two PMC passes (FETCH_SIZE / WRITE_SIZE, runs of their own) also the counters
of the same launches: the command is deterministic, so launch i of a kernel is the same launch in every pass.

    python tools/launch_class_stats.py <bench_kernel_trace.csv> <N> [<fetch counter_collection.csv> <write counter_collection.csv>]"""
import csv
import re
import sys


def short(name):
    m = re.search(r'plfx::(k_[a-zA-Z_0-9]+(<[0-9, ]+>)?)', name)
    return m.group(1).replace(' ', '') if m else name[:40]


# the analytic Hill sweep under either of its names (k_sweep_light_plane: the plane-column form)
SWEEP = ('k_sweep_light<1>', 'k_sweep_light_plane')


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def steps_of(rows, n):
    ends = [i for i, r in enumerate(rows) if r[2].startswith('k_update_state')]
    return [rows[ends[k - 1] + 1:ends[k] + 1] for k in range(len(ends) - n, len(ends))]


def main(argv):
    n = int(argv[2])
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])) for r in csv.DictReader(open(argv[1])))
    steps = steps_of(rows, n)
    print('%d load steps; kernels per step median %g; span median %.1f us; busy median %.1f us'
          % (len(steps), median([len(s) for s in steps]), median([(s[-1][1] - s[0][0]) / 1e3 for s in steps]),
             median([sum(e - a for a, e, _ in s) / 1e3 for s in steps])))
    sw = [[(e - a) / 1e3 for a, e, k in s if k in SWEEP] for s in steps]
    print('k_sweep_light<1> / k_sweep_light_plane launches per step: median %g' % median([len(x) for x in sw]))
    for pos in range(int(max(len(x) for x in sw))):
        v = [x[pos] for x in sw if len(x) > pos]
        print('  sweep %d of the step: n=%d median %.2f us (min %.2f max %.2f)' % (pos + 1, len(v), median(v), min(v), max(v)))
    for k in ('k_cg_start<1>', 'k_cg_start_test<1>', 'k_cg_start_pred'):
        per = [sum((e - a) / 1e3 for a, e, kk in s if kk == k) for s in steps]
        cnt = [sum(1 for _, _, kk in s if kk == k) for s in steps]
        each = [(e - a) / 1e3 for s in steps for a, e, kk in s if kk == k]
        if each:
            print('%-20s %.2f launches per step; median of a launch %.2f us; mean per step %.2f us' % (k, sum(cnt) / len(cnt), median(each), sum(per) / len(per)))
    if len(argv) > 4:
        # position of every sweep launch in its step, from the trace; the PMC passes run the same launches in the same order
        idx = {}
        order = [i for i, r in enumerate(rows) if r[2] in SWEEP]
        ends = [i for i, r in enumerate(rows) if r[2].startswith('k_update_state')]
        pos_of = []
        e = 0
        cnt = 0
        for i in order:
            while e < len(ends) and ends[e] < i:
                e += 1
                cnt = 0
            pos_of.append(cnt)
            cnt += 1
        for path, cname in ((argv[3], 'FETCH_SIZE'), (argv[4], 'WRITE_SIZE')):
            for kern in (SWEEP, ('k_cg_start<1>',), ('k_cg_start_test<1>',)):
                r = sorted((int(x['Start_Timestamp']), float(x['Counter_Value']) * 1024 / 1e6) for x in csv.DictReader(open(path))
                           if x['Counter_Name'] == cname and short(x['Kernel_Name']) in kern)
                v = [b for _, b in r]
                if not v:
                    continue
                if kern is SWEEP and len(v) == len(pos_of):
                    tail = 2 * n
                    for pos in sorted(set(pos_of[-tail:])):
                        w = [v[i] for i in range(len(v) - tail, len(v)) if pos_of[i] == pos]
                        print('%s %s, sweep %d of the step (last %d launches): n=%d median %.2f MB (min %.2f max %.2f)'
                              % (cname, ' / '.join(kern), pos + 1, tail, len(w), median(w), min(w), max(w)))
                else:
                    w = v[-n:]
                    print('%s %s (last %d dispatches of %d): median %.2f MB (min %.2f max %.2f)' % (cname, kern[0], len(w), len(v), median(w), min(w), max(w)))


if __name__ == '__main__':
    main(sys.argv)

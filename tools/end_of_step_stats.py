#!/usr/bin/env python3
"""Medians over the last N load steps of a rocprofv3 kernel trace of bench.py (a step = the launches up to and including a
k_update_state launch): kernels per step, span and busy time of a step, duration of k_update_state<1> and of the launches that
hand the step's results over (k_gather2 + k_reduce_rows, or k_finish_out), and the launches of k_sweep_heavy per step.  With
the two PMC passes (FETCH_SIZE / WRITE_SIZE, runs of their own) also the counter traffic 2 x FETCH_SIZE + WRITE_SIZE of
k_update_state<1> over its last N dispatches.

    python tools/end_of_step_stats.py <bench_kernel_trace.csv> [N] [<fetch counter_collection.csv> <write counter_collection.csv>]"""
import csv
import re
import sys


def short(name):
    m = re.search(r'plfx::(k_[a-zA-Z_0-9]+(<[0-9, ]+>)?)', name)
    return m.group(1).replace(' ', '') if m else name[:40]


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main(argv):
    n = int(argv[2]) if len(argv) > 2 else 20
    rows = [(int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])) for r in csv.DictReader(open(argv[1]))]
    rows.sort()
    ends = [i for i, r in enumerate(rows) if r[2].startswith('k_update_state')]
    steps = [rows[ends[k - 1] + 1:ends[k] + 1] for k in range(len(ends) - n, len(ends))]
    print('%d load steps (the last %d k_update_state launches of the run)' % (len(steps), n))
    print('kernels per step       median %g   (min %d, max %d)' % (median([len(s) for s in steps]), min(len(s) for s in steps), max(len(s) for s in steps)))
    print('span of a step         median %.1f us' % median([(s[-1][1] - s[0][0]) / 1e3 for s in steps]))
    print('busy time of a step    median %.1f us' % median([sum(e - a for a, e, _ in s) / 1e3 for s in steps]))

    def per_step(names):
        return [sum(e - a for a, e, k in s if k in names) / 1e3 for s in steps]
    for label, names in (('k_update_state<1> / _plane<1>', ('k_update_state<1>', 'k_update_state_plane<1>')), ('k_gather2 + k_reduce_rows', ('k_gather2', 'k_reduce_rows')),
                         ('k_finish_out', ('k_finish_out',)), ('k_sweep_heavy<1>', ('k_sweep_heavy<1>',)), ('k_sweep_flags', ('k_sweep_flags',))):
        v = per_step(names)
        cnt = [sum(1 for _, _, k in s if k in names) for s in steps]
        if any(cnt):
            print('%-26s median %6.1f us per step   (min %.1f, max %.1f; %g launches per step)' % (label, median(v), min(v), max(v), median(cnt)))
    if len(argv) > 4:
        per = []
        for path, cname in ((argv[3], 'FETCH_SIZE'), (argv[4], 'WRITE_SIZE')):
            r = [(int(x['Start_Timestamp']), float(x['Counter_Value']) * 1024 / 1e6) for x in csv.DictReader(open(path))
                 if x['Counter_Name'] == cname and short(x['Kernel_Name']) in ('k_update_state<1>', 'k_update_state_plane<1>')]
            r.sort()
            per.append([v for _, v in r][-n:])
        f, w = median(per[0]), median(per[1])
        print('k_update_state<1> counters over its last %d dispatches: FETCH_SIZE median %.1f MB, WRITE_SIZE median %.1f MB, '
              '2 x FETCH_SIZE + WRITE_SIZE = %.1f MB' % (n, f, w, 2 * f + w))


if __name__ == '__main__':
    main(sys.argv)

#!/usr/bin/env python3
"""Per-launch time of the shade and scatter kernels of a rocprofv3 kernel trace (CSV).

usage: tools/rocprof_per_launch.py kernel_trace.csv[.gz] [bench.json]
A propagate starts at its init_queue_kernel; the k-th shade_kernel and
scatter_queue_kernel dispatch after it belong to its slot k.  Dispatches of a
slot that runs nothing (idle, or the tail's) return at once: slots are
listed while their shade takes >= 5 us in the median.  Per slot: the median
over the propagates of the dispatch's duration, and with a bench.py --full
result line the rays of that launch in the first propagate and the time per
ray."""
import csv
import gzip
import json
import statistics
import sys


def main():
    path = sys.argv[1]
    rows = list(csv.DictReader(gzip.open(path, 'rt') if path.endswith('.gz') else open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    rays = []
    if len(sys.argv) > 2:
        for line in open(sys.argv[2]):
            line = line.strip()
            if line.startswith('{'):
                d = json.loads(line)
                tl = (d.get('detail') or d).get('first_propagate_trace_launches')
                if tl:
                    rays = [x['rays'] for x in tl]
    per = {'shade_kernel': [], 'scatter_queue_kernel': []}
    idx = {}
    nprop = 0
    for r in rows:
        name = r['Kernel_Name']
        if 'init_queue_kernel' in name:
            nprop += 1
            idx = {k: 0 for k in per}
            continue
        for k in per:
            if k in name and nprop:
                i = idx[k]
                idx[k] += 1
                while len(per[k]) <= i:
                    per[k].append([])
                per[k][i].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    out = {'propagates': nprop, 'launches': []}
    for i, sh in enumerate(per['shade_kernel']):
        us = statistics.median(sh)
        if us < 5.0:
            break
        sc = per['scatter_queue_kernel'][i] if i < len(per['scatter_queue_kernel']) else [0.0]
        e = {'slot': i, 'shade_us': round(us, 1), 'scatter_us': round(statistics.median(sc), 1)}
        if i < len(rays):
            e['rays'] = rays[i]
            e['alive_fraction'] = round(rays[i] / rays[0], 4)
            e['shade_ns_per_ray'] = round(1e3 * us / rays[i], 2)
            e['scatter_ns_per_ray'] = round(1e3 * e['scatter_us'] / rays[i], 2)
        out['launches'].append(e)
    out['shade_ms_per_propagate'] = round(sum(e['shade_us'] for e in out['launches']) / 1e3, 3)
    out['scatter_ms_per_propagate'] = round(sum(e['scatter_us'] for e in out['launches']) / 1e3, 3)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()

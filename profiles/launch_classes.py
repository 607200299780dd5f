"""Launch classes of conv1d_wino4_f32 from two rocprofv3 --kernel-trace CSVs (parent, tree): per (instantiation, blocks) the calls and the
mean duration of each build, and MfmaUtil from two pmc_summarize.py tables if given.  The residual launches (EPI 3) pair with each other,
the plain ones (EPI 0 before round 23, EPI 4 since, EPI 0 for strips and C-in slices) with each other.
usage: python profiles/launch_classes.py <parent_trace.csv> <tree_trace.csv> [<parent_pmc.txt> <tree_pmc.txt>]"""
import csv
import re
import sys
from collections import defaultdict


def classes(path):
    d = defaultdict(lambda: [0, 0])
    other = 0
    with open(path) as f:
        for r in csv.DictReader(f):
            dur = int(r['End_Timestamp']) - int(r['Start_Timestamp'])
            m = re.search(r'conv1d_wino4_f32<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>', r['Kernel_Name'])
            if not m:
                other += dur
                continue
            k, noct, nst, epi, lp, pt = map(int, m.groups())
            key = (pt, k, lp, 'residual' if epi == 3 else 'plain', int(r['Grid_Size_X']) // int(r['Workgroup_Size_X']))
            d[key][0] += 1
            d[key][1] += dur
    return d, other


a, oa = classes(sys.argv[1])
b, ob = classes(sys.argv[2])
print(f'{"groups":>6} {"k":>3} {"window":>7} {"epilogue":>9} {"blocks":>7} {"calls":>6} {"us parent":>10} {"us tree":>9} {"ratio":>6}')
ta = tb = 0
for key in sorted(set(a) | set(b), key=lambda t: (-t[0], t[1], t[2], t[3], t[4])):
    ca, da = a.get(key, (0, 0))
    cb, db = b.get(key, (0, 0))
    ta += da
    tb += db
    ua, ub = (da / ca / 1e3 if ca else float('nan')), (db / cb / 1e3 if cb else float('nan'))
    print(f'{"seven" if key[0] == 7 else "six":>6} {key[1]:3d} {"vector" if key[2] == 1 else "strip":>7} {key[3]:>9} {key[4]:7d} {max(ca, cb):6d} '
          f'{ua:10.1f} {ub:9.1f} {ub / ua:6.3f}')
print(f'sum over the conv1d_wino4_f32 launches: {ta / 1e6:.2f} -> {tb / 1e6:.2f} ms; every other kernel: {oa / 1e6:.2f} -> {ob / 1e6:.2f} ms (whole trace)')

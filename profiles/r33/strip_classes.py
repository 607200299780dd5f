"""The strip launches (dilation 3 / 5) of conv1d_wino4_f32 from two rocprofv3 --kernel-trace CSVs (parent, tree), paired by SHAPE AND ORDER:
the i-th strip launch of one trace is the i-th of the other (same workload, one stream), whatever its instantiation and block count
(profiles/launch_classes.py pairs by instantiation and block count, and the packed strip form changes both).  Per class (groups, k,
parent blocks, tree blocks): calls, blocks and us per launch of each build; the dilation-1 launches as the control, by launch_classes.py's key.
usage: python profiles/r33/strip_classes.py <parent_trace.csv> <tree_trace.csv> [<parent_pmc_trace.csv> <tree_pmc_trace.csv> <parent_counters.csv> <tree_counters.csv>]"""
import csv
import re
import sys
from collections import defaultdict

PAT = re.compile(r'conv1d_wino4_f32<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>')


def launches(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            m = PAT.search(r['Kernel_Name'])
            if not m:
                continue
            k, noct, nst, epi, lp, pt = map(int, m.groups())
            rows.append((int(r['Start_Timestamp']), k, epi, lp, pt, int(r['Grid_Size_X']) // int(r['Workgroup_Size_X']),
                         int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
    rows.sort()
    return rows


a, b = launches(sys.argv[1]), launches(sys.argv[2])
sa, sb = [r for r in a if r[3] == 2], [r for r in b if r[3] == 2]
assert len(sa) == len(sb), (len(sa), len(sb))
cls = defaultdict(lambda: [0, 0, 0, set(), set()])
for x, y in zip(sa, sb):
    assert x[1] == y[1] and x[4] == y[4], (x, y)
    c = cls[(x[4], x[1], x[5], x[2], y[5])]
    c[0] += 1
    c[1] += x[6]
    c[2] += y[6]
    c[3].add(y[5])
    c[4].add(y[2])
print(f'{"groups":>6} {"k":>3} {"EPI p":>5} {"EPI t":>5} {"blocks p":>8} {"blocks t":>8} {"calls":>6} {"us parent":>10} {"us tree":>9} {"ratio":>6} {"diff us":>8}')
ta = tb = 0
per_epi = defaultdict(lambda: [0, 0])
for key in sorted(cls, key=lambda t: (-t[0], t[1], t[2], t[4])):
    n, da, db, bt, et = cls[key]
    ta += da
    tb += db
    for e in et:
        per_epi[e][0] += da
        per_epi[e][1] += db
    print(f'{"seven" if key[0] == 7 else "six":>6} {key[1]:3d} {key[3]:5d} {"/".join(map(str, sorted(et))):>5} {key[2]:8d} {"/".join(map(str, sorted(bt))):>8} {n:6d} '
          f'{da / n / 1e3:10.1f} {db / n / 1e3:9.1f} {db / da:6.3f} {(db - da) / n / 1e3:8.1f}')
print(f'strip launches, whole trace: {ta / 1e6:.3f} -> {tb / 1e6:.3f} ms ({(tb - ta) / 1e6:+.3f})')
for e, (da, db) in sorted(per_epi.items()):
    print(f'  of them on EPI {e} in the tree: {da / 1e6:.3f} -> {db / 1e6:.3f} ms ({(db - da) / 1e6:+.3f})')
ctl = defaultdict(lambda: [0, 0, 0])
for rows, i in ((a, 1), (b, 2)):
    for r in rows:
        if r[3] == 1:
            key = (r[4], r[1], 'residual' if r[2] == 3 else ('convt' if r[2] >= 5 else 'plain'), r[5])
            ctl[key][0] += 1 if i == 1 else 0
            ctl[key][i] += r[6]
ra = [(v[2] / v[1], k) for k, v in ctl.items() if v[1] and v[2]]
sa_, sb_ = sum(v[1] for v in ctl.values()), sum(v[2] for v in ctl.values())
print(f'control, {len(ctl)} dilation-1 classes: {sa_ / 1e6:.3f} -> {sb_ / 1e6:.3f} ms ({sb_ / sa_:.4f}x); per class {min(ra)[0]:.3f} .. {max(ra)[0]:.3f}x')
for r, k in sorted(ra):
    if r < 0.99 or r > 1.01:
        print(f'  outside +-1 %: {k} {ctl[k][0]} calls {r:.3f}x')

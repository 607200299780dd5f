"""Writes tests/golden/hifigan_launches.json: the launches of hifigan_forward, line by line as TTSAMD_CONV_LOG records them, for the grid
of tests/test_gpu_hifigan_launches.py (three batch sizes x every option set that moves a ResBlock between kernels).

    python tools/gen_golden_hifigan_launches.py          (on an MI355X, with the library of the PARENT commit built in the tree)

The golden in the repository was made this way from the commit before hifigan_forward was split into one stage schedule and
csrc/conv_route.hip's pair_route, so that tests/test_gpu_hifigan_launches.py and tests/test_pair_route_cpu.py hold the new code to the
launches of the code it replaced.  It is never run against the code under test: regenerate it only from a build whose launch sequence is
the intended one.  Each distinct sequence is stored once, zlib-compressed."""
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
from test_gpu_hifigan_launches import GOLDEN_PATH, SHAPES, pack_lines, run_child  # noqa: E402  (the one enumeration of the grid)


def main():
    with tempfile.TemporaryDirectory() as d:
        all_cases, runs = run_child(os.path.join(d, 'conv_log.csv'))
    sequences, index, out = [], {}, []
    for (gen, prec, options, si), lines in zip(all_cases, runs):
        key = '\n'.join(lines)
        if key not in index:
            index[key] = len(sequences)
            sequences.append(pack_lines(lines))
        out.append({'generator': gen, 'precision': prec, 'options': options, 'shape': si, 'sequence': index[key]})
        print(gen, prec, options, SHAPES[si][:2], len(lines), 'launches ->', sorted({ln.split(',')[0] for ln in lines}))
    with open(GOLDEN_PATH, 'w') as f:
        json.dump({'shapes': SHAPES, 'cases': out, 'sequences': sequences}, f, indent=0)
        f.write('\n')
    print(len(out), 'cases,', len(sequences), 'distinct sequences,', os.path.getsize(GOLDEN_PATH), 'bytes')


if __name__ == '__main__':
    main()

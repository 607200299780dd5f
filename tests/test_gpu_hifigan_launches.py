"""The launch sequence of hifigan_forward, line by line as TTSAMD_CONV_LOG records it, against tests/golden/hifigan_launches.json:
what the commit before the stage schedule and csrc/conv_route.hip's pair_route launched (tools/gen_golden_hifigan_launches.py), for
three batch sizes under every option set that moves a ResBlock from one kernel to another."""
import base64
import json
import os
import subprocess
import sys
import zlib

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(REPO, 'tests', 'golden', 'hifigan_launches.json')

# (B, T, lens): by the small-problem rule of pair_route (B T >= 504 at C = 32, >= 1008 at C = 64) no stage, the C = 32 stage alone, and
# the C = 32 and C = 64 stages lie above the bound; the forced masks reach C = 128
SHAPES = [(1, 40, None), (4, 160, [160, 151, 97, 133]), (8, 160, [160, 151, 97, 133, 160, 120, 88, 144])]
ALL = {'FUSED2_MASK': '1ff'}
OPTION_SETS = {
    ('v1', 'f32'): [{}, {'FUSED_PAIR': 0}, {'FUSED2': 0}, {'FUSED2_MASK': 0}, ALL, dict(ALL, FUSED2_MASK_N1='1ff'), dict(ALL, FUSED2_WB=0),
                    dict(ALL, FUSED2_WB=1), {'PAIR4': 0}, {'PAIR4': 2}, {'HIFIGAN_STREAMS': 0}, {'HIFIGAN_STREAMS': 1}, {'WINO': 0}],
    ('v1', 'bf16'): [{}, {'BFO_CHAIN': 0}, {'BFO': 0}, {'BFO': 0, 'BF16_PACKED_T': 0}],
    ('v1', 'bf16x3'): [{}, {'BFO_CHAIN': 0}],
    ('v3', 'f32'): [{}, {'RESBLOCK2_PAIR': '3f'}],
}


def cases():
    """(generator, precision, options, shape index), in the order the child runs them"""
    for (gen, prec), sets in OPTION_SETS.items():
        for options in sets:
            for si in range(len(SHAPES)):
                yield gen, prec, options, si


_CHILD = r'''
import json, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from ttsamd import lib, synth
from ttsamd.config import HIFIGAN_V3_CONFIG
from ttsamd.engine import HifiGanEngine, set_precision
log, shapes, cases = sys.argv[1], json.loads(sys.argv[2]), json.loads(sys.argv[3])
dev = torch.device('cuda:0')
engines = {'v1': HifiGanEngine(synth.hifigan_state_dict(), device=dev),
           'v3': HifiGanEngine(synth.hifigan_state_dict(HIFIGAN_V3_CONFIG), HIFIGAN_V3_CONFIG, device=dev)}
rng = np.random.default_rng(12)
inputs = []
for B, T, lens in shapes:
    mel = torch.from_numpy((rng.standard_normal((B, 80, T)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    inputs.append((mel, None if lens is None else torch.tensor(lens).to(dev)))
for i, (gen, prec, options, si) in enumerate(cases):
    set_precision(prec)
    for name, value in options.items():
        lib.set_option(name, value)
    with open(log, 'a') as f:
        f.write('# case %%d\n' %% i)
    engines[gen].forward(*inputs[si])
    torch.cuda.synchronize()
    for name in options:
        lib.set_option(name, None)
set_precision('f32')
print('LAUNCHES OK')
'''


def run_child(log, env=None):
    """One child process with TTSAMD_CONV_LOG set (the log is opened once per process) runs every case, a marker line before each
    forward; returns the logged lines per case, in order."""
    all_cases = list(cases())
    code = _CHILD % (os.path.join(REPO, 'tts-arabic-pytorch_amd'), os.path.join(REPO, 'oracle'))
    p = subprocess.run([sys.executable, '-c', code, str(log), json.dumps(SHAPES), json.dumps(all_cases)], capture_output=True, timeout=600,
                       env=dict(os.environ if env is None else env, TTSAMD_CONV_LOG=str(log)))
    assert p.returncode == 0 and b'LAUNCHES OK' in p.stdout, p.stderr.decode()[-3000:]
    runs, cur = [], None
    with open(log) as f:
        for ln in f.read().splitlines():
            if ln.startswith('# case '):
                assert int(ln[len('# case '):]) == len(runs)
                cur = []
                runs.append(cur)
            elif cur is not None:
                cur.append(ln)
    assert len(runs) == len(all_cases)
    return all_cases, runs


def pack_lines(lines):
    return base64.b64encode(zlib.compress('\n'.join(lines).encode(), 9)).decode()


def load_golden():
    """-> [(generator, precision, options, shape index, [log lines])]"""
    with open(GOLDEN_PATH) as f:
        g = json.load(f)
    assert g['shapes'] == [list(s) for s in SHAPES]
    seqs = [zlib.decompress(base64.b64decode(s)).decode().split('\n') for s in g['sequences']]
    return [(c['generator'], c['precision'], c['options'], c['shape'], seqs[c['sequence']]) for c in g['cases']]


@pytest.mark.gpu
def test_launch_sequences_equal_the_golden(tmp_path):
    """every forward of the grid logs exactly the lines, in exactly the order, of the golden"""
    golden = load_golden()
    all_cases, runs = run_child(tmp_path / 'conv_log.csv')
    assert [list(c[:4]) for c in golden] == [list(c) for c in all_cases], 'the golden was made for another grid'
    wrong = []
    for (gen, prec, options, si, want), got in zip(golden, runs):
        if got != want:
            first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            wrong.append(f'{gen} {prec} {options} shape {SHAPES[si][:2]}: {len(got)} lines for {len(want)}, first difference at line {first}: '
                         f'{got[first] if first < len(got) else None!r} for {want[first] if first < len(want) else None!r}')
    assert not wrong, '\n'.join(wrong)


def test_golden_names_every_launch_kind():
    """the golden holds every log name a forward can produce: the fused pairs in all their forms, an un-fused fp32 pair, ResBlock2 as
    convs and as a pair, and the octet engine's chain, pair and conv launches in both modes"""
    names = set()
    unfused_pair = False
    for gen, prec, options, si, lines in load_golden():
        kinds = [ln.split(',')[0] for ln in lines]
        names.update(kinds)
        if prec == 'f32' and options.get('FUSED_PAIR') == 0:
            unfused_pair = unfused_pair or not any(k.startswith('fused_pair') for k in kinds)
    want = {'fused_pair', 'fused_pair2', 'fused_pair2n', 'fused_pair2w', 'fused_pair2ww', 'fused_pair4', 'fused_pair44', 'rb2_conv', 'rb2_pair',
            'bfo_chain', 'bfo_pair', 'bfo', 'bfo3_chain', 'bfo3_pair', 'bfo3', 'f32', 'f32_wino4', 'bf16'}
    assert want <= names, sorted(want - names)
    assert unfused_pair

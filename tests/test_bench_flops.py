"""The numerator of bench.py's roofline: algorithmic FLOPs per unit must equal SURVEY §8(d)'s figures
(HiFi-GAN 614.1 MFLOP per mel frame incl. 0.11 of conv_post; FastPitch 22.88 GFLOP per 64-token / 448-frame
utterance incl. the 0.26 GFLOP of attention scores that do not run in conv launches)."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(REPO, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_hifigan_flops_per_frame():
    from ttsamd.config import HIFIGAN_CONFIG
    f = _bench().hifigan_flops_per_frame(HIFIGAN_CONFIG)
    conv_post = 2.0 * 32 * 7 * 256
    assert abs((f + conv_post) / 1e6 - 614.11) < 0.05
    assert abs(f / 256 / 1e6 - 2.3984) < 0.001            # MFLOP per output sample


def test_fastpitch_flops_per_utterance():
    from ttsamd.config import NET_CONFIG
    dec, enc = _bench().fastpitch_conv_flops_per_pos(NET_CONFIG)
    conv = dec * 448 + enc * 64                              # conv launches only
    attn = 6 * (2 * 2 * 64 * 448) * 448 + 6 * (2 * 2 * 64 * 64) * 64   # QK^T and PV, 1 head of 64, both stacks
    assert abs((conv + attn) / 1e9 - 22.88) < 0.05
    assert abs(dec / 1e6 - 43.71) < 0.02 and abs(enc / 1e6 - 46.60) < 0.02


def test_bf16_roofline_bound_follows_the_algorithmic_intensity():
    """`roofline.bound` of a bf16 launch sequence is whichever roof the algorithmic FLOP / HBM-byte ratio puts first (ridge =
    2.5 PFLOP/s / 8 TB/s = 312.5): the fused-pair step (562 FLOP/B) is MFMA-bound and `frac` is the MFMA fraction; a layer-wise
    step (137 FLOP/B) is HBM-bound and `frac` is the HBM fraction.  Both sides always ride along."""
    b = _bench()
    r = b.bf16_roofline(9.53e12, 16.95e9, 10e-3)
    assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s' and abs(r['frac'] - 953.0 / 2500.0) < 1e-6
    assert abs(r['hbm_frac'] - 1695.0 / 8000.0) < 1e-6 and abs(r['algorithmic_flop_per_byte'] - 562.2) < 0.5
    r = b.bf16_roofline(9.53e12, 9.53e12 / 137.0, 10e-3)
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and abs(r['frac'] - r['hbm_frac']) < 1e-12
    assert abs(r['mfma_frac'] - 953.0 / 2500.0) < 1e-6


def test_median_and_gpu_count_helpers(tmp_path, monkeypatch):
    b = _bench()
    assert b._median([3.0, 1.0, 2.0]) == 2.0 and b._median([4.0, 1.0, 2.0, 3.0]) == 2.5 and b._median([]) is None
    # the launcher parents count GPUs without the HIP runtime: the visibility variables win over the topology
    monkeypatch.setenv('HIP_VISIBLE_DEVICES', '0,3')
    assert b._count_gpus() == 2
    monkeypatch.setenv('HIP_VISIBLE_DEVICES', '')
    assert b._count_gpus() == 0


def test_dump_outputs_cut_zeroed_and_capped(tmp_path):
    """--dump-outputs: the step's outputs cut to max(dec_lens) and zeroed past each utterance's end (independent of the engines'
    row padding), float32 / float64 files; above the cap the same seeded utterances of every array, listed in rows.npy."""
    import numpy as np
    import torch
    b = _bench()
    hop = 4
    lens = torch.tensor([3, 5, 2], dtype=torch.int64)
    mel = torch.randn(3, 2, 8)
    wave = torch.randn(3, 8 * hop)
    got = b.step_outputs(mel, lens, wave, hop)
    assert got['mel'].shape == (3, 2, 5) and got['wave'].shape == (3, 5 * hop)
    for i, n in enumerate(lens.tolist()):
        assert np.array_equal(got['mel'][i, :, :n], mel[i, :, :n].numpy()) and not got['mel'][i, :, n:].any()
        assert np.array_equal(got['wave'][i, :n * hop], wave[i, :n * hop].numpy()) and not got['wave'][i, n * hop:].any()
    files = b.dump_outputs(str(tmp_path / 'all'), got)
    assert files == ['dec_lens.npy', 'mel.npy', 'wave.npy']
    lo = np.load(tmp_path / 'all' / 'dec_lens.npy')
    assert lo.dtype == np.float64 and lo.tolist() == [3.0, 5.0, 2.0]
    assert np.load(tmp_path / 'all' / 'wave.npy').dtype == np.float32
    big = {'wave': np.arange(100 * 1000, dtype=np.float32).reshape(100, 1000), 'dec_lens': np.arange(100)}
    cap = 30 * (4000 + 8) + 800
    files = b.dump_outputs(str(tmp_path / 'cap'), big, cap=cap)
    assert 'rows.npy' in files and sum(os.path.getsize(tmp_path / 'cap' / f) for f in files) <= cap + 128 * len(files)
    rows = np.load(tmp_path / 'cap' / 'rows.npy').astype(np.int64)
    assert len(rows) == 30 and np.array_equal(rows, np.sort(rows))
    assert np.array_equal(np.load(tmp_path / 'cap' / 'dec_lens.npy'), rows.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / 'cap' / 'wave.npy'), big['wave'][rows])
    assert b.dump_outputs(str(tmp_path / 'cap2'), big, cap=cap) == files
    assert np.array_equal(np.load(tmp_path / 'cap2' / 'rows.npy'), np.load(tmp_path / 'cap' / 'rows.npy'))   # seeded
    b.dump_outputs(str(tmp_path / 'cap'), {'dec_lens': np.arange(3)}, cap=cap)
    assert not os.path.exists(tmp_path / 'cap' / 'rows.npy')            # no stale sample list beside a full dump


def test_bench_rejects_zero_steps():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '0'], capture_output=True, text=True)
    assert r.returncode == 2 and '--steps' in r.stderr


def test_bench_full_option_listed():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and '--full' in r.stdout


def _bench_line(*extra):
    import json
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                        '--batch', '16', '--tokens', '16', *extra], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_line_is_the_headline_and_full_adds_the_sub_results():
    """A plain run prints the headline of its timed steps and runs nothing else; --full adds the sub-results after them (here
    batch 1 / 8 only: --no-extra and --no-cpu-baseline keep the test short)."""
    plain = _bench_line()
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'roofline'):
        assert k in plain, k
    assert plain['value'] > 0 and plain['ms_per_step'] > 0 and plain['dtype'] == 'f32'
    for k in ('configs', 'd2h', 'cpu_baseline', 'bench_sections_s'):
        assert k not in plain, k
    full = _bench_line('--full', '--no-extra', '--no-cpu-baseline')
    assert [c['batch'] for c in full['configs']] == [1, 8] and 'batch 1 / 8' in full['bench_sections_s']
    assert 'd2h' not in full and 'cpu_baseline' not in full
    assert full['config']['frames_per_step_rank0'] == plain['config']['frames_per_step_rank0']

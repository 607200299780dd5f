"""Output levelling next to the vocoder step it follows (profiles/r19/NOTES.md is written from its output).

Workload: 32 rows of 5 s at 22 050 Hz (110 250 samples each; the wave of the same batch's HiFi-GAN step: 32 mels of 430 frames through
the synthetic V1 generator), LoudnessEngine.measure + ttsamd_wave_level on the current stream: the five launches `normalize='lufs'`
adds behind the denoiser.  Reported: the median time of measure + level, of measure alone and of the HiFi-GAN step of that batch, by
device events around --iters back-to-back calls (so that a timed window is long against the event resolution), every shape warmed up
first, the three alternating inside one process; and the share of the vocoder step the levelling takes.

    python profiles/loudness_bench.py [--reps 15] [--warmup 3] [--iters 20] [--rows 32] [--seconds 5] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rows', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=5.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG
    from ttsamd.engine import HifiGanEngine, leveller

    assert torch.cuda.is_available(), 'loudness_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    hg = HifiGanEngine(synth.hifigan_state_dict(), dict(HIFIGAN_CONFIG), device=dev)
    frames = int(round(args.seconds * 22050 / hg.hop))
    B = args.rows
    rng = np.random.default_rng(0)
    mel = torch.from_numpy(rng.standard_normal((B, HIFIGAN_CONFIG['num_mels'], frames)).astype(np.float32)).to(dev)
    lens = torch.full((B,), frames, dtype=torch.int64, device=dev)
    n = lens * hg.hop
    wave0 = hg.forward(mel, lens).clone()
    eng = leveller(22050, dev)
    mode = [2] * B
    target = [-23.0] * B

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    wave = wave0.clone()
    cases = {
        'hifigan_step_ms': (lambda: hg.forward(mel, lens), max(1, args.iters // 10)),
        'measure_ms': (lambda: eng.measure(wave, n), args.iters),
        # the gain of a levelled row is ~1 from the second call on: the same launches and traffic
        'measure_level_ms': (lambda: eng.level(wave, n, mode, target), args.iters),
    }
    for fn, _ in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, (fn, iters) in cases.items():
            times[k].append(timed(fn, iters))
    loud, peak = eng.measure(wave0, n)
    row = dict(bench='loudness', rows=B, samples_per_row=int(n[0]), sample_rate=22050, reps=args.reps, iters=args.iters,
               loudness_of_row0_lufs=round(float(loud[0]), 4), peak_of_row0=round(float(peak[0]), 6))
    for k, v in times.items():
        row[k] = round(statistics.median(v), 5)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 5)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 5)
    row['level_share_of_vocoder_step'] = round(row['measure_level_ms'] / row['hifigan_step_ms'], 6)
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

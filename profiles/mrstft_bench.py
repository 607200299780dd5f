"""Multi-resolution STFT distance next to the log-spectral distance of the same pairs (profiles/r38/NOTES.md is written from its output).

Workload: 32 pairs of 5 s at 22 050 Hz (110 080 samples = 430 mel frames each): a speech-like row (harmonics under a syllable envelope,
a different pitch per row) against its copy synthesis through the synthetic V1 generator.  Reported: the median time of
ttsamd.engine.mr_stft at the default resolutions (what utils.objective.multi_resolution_stft runs: 3 + 1 launches), of each of its
resolutions alone, and, in the same run, of ttsamd.engine.log_spectral_distance (ttsamd_log_spectral_distance: one block per row) on
the same pairs, by device events around --iters back-to-back calls, every case warmed up first, the cases alternating inside one
process.  Then the per-resolution values of plain-bf16 and split-bf16 copy synthesis against the fp32 copy synthesis (synthetic
weights: they say nothing about a trained model's values).

    python profiles/mrstft_bench.py [--reps 15] [--warmup 3] [--iters 20] [--rows 32] [--seconds 5] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))


def speech_like(rows, n, fs=22050):
    import numpy as np
    rng = np.random.default_rng(0)
    t = np.arange(n) / fs
    out = np.empty((rows, n), dtype=np.float32)
    for b in range(rows):
        phase = 2 * np.pi * (100.0 + 5.0 * b) * t + 3.0 * np.sin(2 * np.pi * 5.0 * t)
        s = sum(np.sin(h * phase + 0.7 * h) / h for h in range(1, 9))
        env = np.maximum(np.sin(2 * np.pi * 2.3 * t + 0.2 * b), 0.0) ** 2
        out[b] = 0.3 * env * s + 1e-4 * rng.standard_normal(n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rows', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=5.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from ttsamd import engine as E
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG

    assert torch.cuda.is_available(), 'mrstft_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    hg = E.HifiGanEngine(synth.hifigan_state_dict(), dict(HIFIGAN_CONFIG), device=dev)
    frames = int(round(args.seconds * 22050 / hg.hop))
    B, n = args.rows, frames * hg.hop
    ref = torch.from_numpy(speech_like(B, n)).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    mel, mel_frames = E.ObjectiveEngine(device=dev).melspec.forward(ref, lens)

    def resynth(precision):
        E.set_precision(precision)
        try:
            return hg.forward(mel, mel_frames).clone()
        finally:
            E.set_precision('f32')

    est = resynth('f32')

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    res = E.MR_STFT_RESOLUTIONS
    cases = {
        'mr_stft_ms': lambda: E.mr_stft(ref, est, lens, res),
        'lsd_ms': lambda: E.log_spectral_distance(ref, est, lens),
    }
    for N, H, W in res:
        cases[f'mr_stft_{N}_{H}_{W}_ms'] = lambda r=(N, H, W): E.mr_stft(ref, est, lens, [r])
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            times[k].append(timed(fn, args.iters))

    def mean_values(a, b):
        per, _ = E.mr_stft(a, b, lens, res)
        m = per.mean(dim=0)                                             # over the rows
        out = {f'{N}_{H}_{W}': [round(float(m[r, 0]), 6), round(float(m[r, 1]), 6)] for r, (N, H, W) in enumerate(res)}
        out['mr_stft'] = round(float(m.mean(dim=0).sum()), 6)
        return out

    _, fr = E.mr_stft(ref, est, lens, res)
    row = dict(bench='mrstft', rows=B, samples_per_row=n, sample_rate=22050, reps=args.reps, iters=args.iters,
               resolutions=[list(r) for r in res], frames_row0=fr[0].tolist(), kernel_launches=len(res) + 1,
               lsd_frames_row0=int(E.log_spectral_distance(ref, est, lens)[0, 1]),
               copy_synthesis_fp32_vs_input=mean_values(ref, est),
               bf16_vs_fp32_copy_synthesis=mean_values(est, resynth('bf16')),
               bf16x3_vs_fp32_copy_synthesis=mean_values(est, resynth('bf16x3')))
    for k, v in times.items():
        row[k] = round(statistics.median(v), 5)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 5)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 5)
    row['mr_stft_over_lsd'] = round(row['mr_stft_ms'] / row['lsd_ms'], 4)
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

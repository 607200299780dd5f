"""Wave-against-wave scores next to the vocoder step of the same batch (profiles/r29/NOTES.md is written from its output).

Workload: 32 pairs of 5 s at 22 050 Hz (110 080 samples = 430 mel frames each): a speech-like row (harmonics under a syllable envelope,
a different pitch per row) against its copy synthesis through the synthetic V1 generator.  Reported: the median time of
WaveScoreEngine.metrics (what utils.objective.wave_metrics runs) and of its parts -- the two resampler calls to 10 kHz, STOI, ESTOI,
SI-SDR / SNR, the log-spectral distance -- and of the HiFi-GAN step of that batch, by device events around --iters back-to-back calls,
every case warmed up first, the cases alternating inside one process.  Then the scores of plain-bf16 and split-bf16 copy synthesis
against the fp32 copy synthesis (synthetic weights: they say nothing about a trained model's scores).

    python profiles/wavescore_bench.py [--reps 15] [--warmup 3] [--iters 20] [--rows 32] [--seconds 5] [--out FILE.jsonl]"""
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

    assert torch.cuda.is_available(), 'wavescore_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    hg = E.HifiGanEngine(synth.hifigan_state_dict(), dict(HIFIGAN_CONFIG), device=dev)
    frames = int(round(args.seconds * 22050 / hg.hop))
    B, n = args.rows, frames * hg.hop
    ref = torch.from_numpy(speech_like(B, n)).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    mel, mel_frames = E.ObjectiveEngine(device=dev).melspec.forward(ref, lens)
    scorer = E.wave_scorer(22050, dev)

    def resynth(precision):
        E.set_precision(precision)
        try:
            return hg.forward(mel, mel_frames).clone()
        finally:
            E.set_precision('f32')

    est = resynth('f32')
    r10, n10 = scorer.to_10k(ref, lens)
    e10, _ = scorer.to_10k(est, lens)

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    cases = {
        'hifigan_step_ms': (lambda: hg.forward(mel, mel_frames), max(1, args.iters // 10)),
        'wave_metrics_ms': (lambda: scorer.metrics(ref, est, lens), args.iters),
        'resample_pair_ms': (lambda: (scorer.to_10k(ref, lens), scorer.to_10k(est, lens)), args.iters),
        'stoi_ms': (lambda: E.stoi_10k(r10, e10, n10), args.iters),
        'estoi_ms': (lambda: E.stoi_10k(r10, e10, n10, extended=True), args.iters),
        'sdr_ms': (lambda: E.wave_sdr(ref, est, lens), args.iters),
        'lsd_ms': (lambda: E.log_spectral_distance(ref, est, lens), args.iters),
    }
    for fn, _ in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, (fn, iters) in cases.items():
            times[k].append(timed(fn, iters))

    def mean_scores(a, b):
        m = scorer.metrics(a, b, lens)
        return {k: round(float(m[k].double().mean()), 6) for k in ('stoi', 'estoi', 'si_sdr', 'snr', 'lsd')}

    m = scorer.metrics(ref, est, lens)
    row = dict(bench='wavescore', rows=B, samples_per_row=n, sample_rate=22050, reps=args.reps, iters=args.iters,
               stoi_frames_row0=[int(m['frames'][0]), int(m['frames_kept'][0])],
               # launches of one wave_metrics call: 2 resampler + 2 x 3 STOI / ESTOI + 1 SI-SDR / SNR + 1 LSD, plus the length clamps
               kernel_launches_of_the_scoring=10,
               copy_synthesis_fp32_vs_input=mean_scores(ref, est),
               bf16_vs_fp32_copy_synthesis=mean_scores(est, resynth('bf16')),
               bf16x3_vs_fp32_copy_synthesis=mean_scores(est, resynth('bf16x3')))
    for k, v in times.items():
        row[k] = round(statistics.median(v), 5)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 5)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 5)
    row['wave_metrics_share_of_vocoder_step'] = round(row['wave_metrics_ms'] / row['hifigan_step_ms'], 6)
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

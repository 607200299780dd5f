"""True peak: what it costs and whether the project's waves need it (profiles/r34/NOTES.md is written from its output).

Two parts, one JSON line each:
  clipping   the bench's batch (FastPitch + HiFi-GAN, synthetic weights, 32 lines of 64 tokens with forced durations) through
             LoudnessEngine.limit towards --lufs at ceiling 0.99, utils.audio.resample to 48 kHz, PCM16: the share of rows with at least one
             sample that the PCM16 conversion has to clip (|rint(32767 x)| beyond the int16 range), with true_peak=False and True; the
             same for a sine at fs / 4 with 45 degrees of phase.  And max TP(y) / c of the limited rows, TP by the float64 restatement
             tests/true_peak_ref.py (not by the kernel under test).
  time       32 rows of 5 s of that generator's output: ttsamd_true_peak against what a caller could do before it,
             utils.audio.resample(x, fs, 4 fs, lowpass_filter_width=12, rolloff=1.0).abs().amax(-1); ttsamd_wave_limit_true_peak against
             ttsamd_wave_limit.  Medians over --reps of device events around --iters back-to-back calls, every shape warmed up, the cases
             alternating inside one process.

    python profiles/true_peak_bench.py [--reps 15] [--warmup 3] [--iters 20] [--lufs -16] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--lufs', type=float, default=-16.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import true_peak_ref as T
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG
    from ttsamd.engine import LIMITER_NO_MAX_GAIN, FastPitchEngine, HifiGanEngine, leveller
    from utils import audio

    assert torch.cuda.is_available(), 'true_peak_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    fp, hg = FastPitchEngine(synth.fastpitch_state_dict()), HifiGanEngine(synth.hifigan_state_dict(), dict(HIFIGAN_CONFIG), device=dev)
    eng = leveller(22050, dev)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    # ---- does the problem exist here? ----
    ids, dur = synth.synth_ids(32, 64), synth.synth_durations(32, 64)
    mel, dec_lens, *_ = fp.infer(ids, dur_tgt=dur)
    wave = hg.forward(mel, dec_lens).contiguous()
    n = (dec_lens * hg.hop).to(torch.int64)
    sine = (0.5 * torch.sin(2 * np.pi * torch.arange(2 * 22050, dtype=torch.float64) / 4 + np.pi / 4)).float().to(dev)[None]

    def clipped_rows(x, lens):
        y, m = audio.resample(x, 22050, 48000, lens=lens)
        v = torch.round(y * 32767.0)
        keep = torch.arange(y.shape[1], device=dev)[None, :] < m[:, None]
        return ((v > 32767) | (v < -32768)) & keep

    row = dict(bench='true_peak_clipping', rows=32, target_lufs=args.lufs, ceiling=0.99, samples=int(n.sum()))
    for name, tp in (('sample_peak', False), ('true_peak', True)):
        y, gain, red = eng.limit(wave.clone(), n, 2, args.lufs, true_peak=tp)
        bad = clipped_rows(y, n)
        yh, nh = y.cpu().numpy(), n.cpu().tolist()
        over = max(T.true_peak64(yh[b, :nh[b]]) for b in range(32)) / float(np.float32(0.99))
        row[name] = dict(rows_clipped=int(bad.any(1).sum()), samples_clipped=int(bad.sum()), rows_limited=int((red < (1 << 30)).sum()),
                         max_true_peak_over_ceiling=round(over, 6), loudness_min_max=[round(float(v), 3) for v in
                                                                                      (eng.measure(y, n)[0].min(), eng.measure(y, n)[0].max())])
        ys, _ = audio.limit(sine, gain_db=12.0, true_peak=tp)
        sb = clipped_rows(ys, torch.tensor([ys.shape[1]], device=dev))
        row[name]['quarter_rate_sine'] = dict(samples_clipped=int(sb.sum()), sample_peak=round(float(ys.abs().max()), 6),
                                              true_peak=round(T.true_peak64(ys[0].cpu().numpy()), 6))
    emit(row)

    # ---- time ----
    frames = int(round(5.0 * 22050 / hg.hop))
    rng = np.random.default_rng(0)
    mel5 = torch.from_numpy(rng.standard_normal((32, HIFIGAN_CONFIG['num_mels'], frames)).astype(np.float32)).to(dev)
    lens5 = torch.full((32,), frames, dtype=torch.int64, device=dev)
    w5 = hg.forward(mel5, lens5).clone()
    n5 = lens5 * hg.hop
    mode = torch.full((32,), 3, dtype=torch.int32, device=dev)
    gain_db = float(20 * np.log10(0.99 / float(w5.abs().amax(1).median()) * 2.0))     # the median row's peak to twice the ceiling
    target = torch.full((32,), gain_db, dtype=torch.float32, device=dev)
    A, R = 33, 331
    scratch = torch.empty_like(w5)

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    def limit(tp):
        scratch.copy_(w5)                   # the limiter works in place: every call gets the same input (the copy is timed on its own)
        eng.limit_samples(scratch, n5, mode, target, 0.99, LIMITER_NO_MAX_GAIN, A, R, true_peak=tp)

    cases = {
        'true_peak_ms': lambda: eng.true_peak(w5, n5),
        'resample_4x_amax_ms': lambda: audio.resample(w5, 22050, 88200, lowpass_filter_width=12, rolloff=1.0).abs().amax(-1),
        'sample_peak_amax_ms': lambda: w5.abs().amax(-1),
        'copy_ms': lambda: scratch.copy_(w5),
        'copy_limit_ms': lambda: limit(False),
        'copy_limit_true_peak_ms': lambda: limit(True),
    }
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            times[k].append(timed(fn, args.iters))
    row = dict(bench='true_peak_time', rows=32, samples_per_row=int(n5[0]), reps=args.reps, iters=args.iters, limiter_gain_db=round(gain_db, 3))
    for k, v in times.items():
        row[k] = round(statistics.median(v), 5)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 5)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 5)
    row['resample_route_over_true_peak'] = round(row['resample_4x_amax_ms'] / row['true_peak_ms'], 3)
    row['limit_true_peak_over_limit'] = round((row['copy_limit_true_peak_ms'] - row['copy_ms']) / (row['copy_limit_ms'] - row['copy_ms']), 3)
    # the two routes read the same peak up to the resampler's fp32 fma chain
    a = eng.true_peak(w5, n5).double()
    b = torch.maximum(audio.resample(w5, 22050, 88200, lowpass_filter_width=12, rolloff=1.0).abs().amax(-1), w5.abs().amax(-1)).double()
    row['max_rel_difference_of_the_two_routes'] = float(((a - b).abs() / a).max())
    emit(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""The look-ahead limiter next to the vocoder step it follows (the next profiles/rNN/NOTES.md is written from its output).

Workload: 32 rows of 5 s at 22 050 Hz (the wave of the same batch's HiFi-GAN step: 32 mels of 431 frames through the synthetic V1
generator), LoudnessEngine.limit in mode 2 towards --target LUFS on the current stream: the four launches of `measure` and the two of
ttsamd_wave_limit that `normalize=<LUFS>, limiter=True` adds behind the denoiser.  Reported: the median time of measure + limit, of the
two limiter launches alone (mode 3: no measurement) and of the HiFi-GAN step of that batch, by device events around --iters
back-to-back calls, every shape warmed up first, the cases alternating inside one process; the share of the vocoder step; and, on the
un-levelled batch, how many rows the cap of ttsamd_wave_level would have hit at the target (peak g > ceiling) and how many the limiter
reduces.  The limiter's launches do the same work whatever the samples are (the curve is computed for every tile), so the calls after
the first, which find the rows already at the target, cost what the first costs.

    python tools/limiter_bench.py [--reps 15] [--warmup 3] [--iters 20] [--rows 32] [--seconds 5] [--target -16] [--out FILE.jsonl]"""
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
    ap.add_argument('--target', type=float, default=-16.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG
    from ttsamd.engine import LIMITER_Q, HifiGanEngine, leveller

    assert torch.cuda.is_available(), 'limiter_bench needs an MI355X: a CPU run says nothing about time'
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
    ceiling = 0.99

    # the un-levelled batch: what the cap would have done, what the limiter does
    loud, peak = eng.measure(wave0, n)
    want = 10.0 ** ((args.target - loud) / 20.0)
    finite = torch.isfinite(loud)
    capped = int((finite & (peak.double() * want > ceiling)).sum())
    lev, _ = eng.level(wave0.clone(), n, 2, args.target, ceiling)
    lim, gain, red = eng.limit(wave0.clone(), n, 2, args.target, ceiling=ceiling)
    l_lev, l_lim = eng.measure(lev, n)[0], eng.measure(lim, n)[0]
    miss = lambda l: float((l[finite] - args.target).abs().max()) if bool(finite.any()) else float('nan')      # noqa: E731

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    wave, wave3 = wave0.clone(), wave0.clone()
    cases = {
        'hifigan_step_ms': (lambda: hg.forward(mel, lens), max(1, args.iters // 10)),
        'measure_ms': (lambda: eng.measure(wave, n), args.iters),
        'measure_limit_ms': (lambda: eng.limit(wave, n, 2, args.target, ceiling=ceiling), args.iters),
        'limit_only_ms': (lambda: eng.limit(wave3, n, 3, 0.0, ceiling=ceiling), args.iters),
    }
    for fn, _ in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, (fn, iters) in cases.items():
            times[k].append(timed(fn, iters))
    row = dict(bench='limiter', rows=B, samples_per_row=int(n[0]), sample_rate=22050, reps=args.reps, iters=args.iters,
               target_lufs=args.target, ceiling=ceiling, loudness_min_lufs=round(float(loud.min()), 3),
               loudness_max_lufs=round(float(loud.max()), 3), peak_max=round(float(peak.max()), 5),
               rows_the_cap_hits=capped, rows_the_limiter_reduces=int((red < LIMITER_Q).sum()),
               deepest_reduction_db=round(float(20 * torch.log10(red.min().double() / LIMITER_Q)), 3),
               worst_miss_capped_lu=round(miss(l_lev), 4), worst_miss_limited_lu=round(miss(l_lim), 4),
               peak_after_limit=round(float(lim.abs().max()), 6))
    for k, v in times.items():
        row[k] = round(statistics.median(v), 5)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 5)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 5)
    row['limit_share_of_vocoder_step'] = round(row['measure_limit_ms'] / row['hifigan_step_ms'], 6)
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

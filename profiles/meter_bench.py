"""The loudness meter next to the plain measurement (profiles/r35/NOTES.md is written from its output).

Workload: 32 rows of 5 s of noise at 22 050 Hz (110 250 samples each).  Timed: LoudnessEngine.measure (ttsamd_loudness_measure: three
filter launches and the gate launch) and LoudnessEngine.meter (ttsamd_loudness_meter: the same three filter launches and the meter
launch), and one push of the whole batch into a LoudnessMeter followed by its reset (the stream path on the same samples).  Median of
--reps windows of --iters back-to-back calls between device events, every case warmed up first, the cases alternating inside one process.

    python profiles/meter_bench.py [--reps 15] [--warmup 3] [--iters 20] [--rows 32] [--seconds 5] [--out FILE.jsonl]"""
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
    from ttsamd.engine import LoudnessMeter, leveller

    assert torch.cuda.is_available(), 'meter_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    B, n = args.rows, int(round(args.seconds * 22050))
    wave = torch.from_numpy((np.random.default_rng(0).standard_normal((B, n)) * 0.1).astype(np.float32)).to(dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    eng = leveller(22050, dev)
    lm = LoudnessMeter(22050, max_streams=B, max_seconds=args.seconds + 1.0, device=dev)
    slots = list(range(B))

    def push():
        lm.push(wave, lens, slots)
        lm.reset(slots)

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    cases = {'measure_ms': lambda: eng.measure(wave, lens), 'meter_ms': lambda: eng.meter(wave, lens),
             'meter_series_ms': lambda: eng.meter(wave, lens, series=True), 'stream_push_reset_ms': push}
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            times[k].append(timed(fn, args.iters))
    m = eng.meter(wave, lens)
    row = dict(bench='meter', rows=B, samples_per_row=n, sample_rate=22050, reps=args.reps, iters=args.iters,
               integrated_of_row0_lufs=round(float(m['integrated'][0]), 4), short_term_values=int(m['counts'][0, 1]))
    for k, v in times.items():
        row[k] = round(statistics.median(v), 5)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 5)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 5)
    row['meter_over_measure'] = round(row['meter_ms'] / row['measure_ms'], 4)
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

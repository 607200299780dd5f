"""pYIN pitch tracking (csrc/pyin.hip): milliseconds per call through ttsamd.engine.PyinEngine with the reference's settings (C2..C7,
frames of 1024 every 256 samples, 22 050 Hz) on rows of 10 s of speech-like signal (glides, silences, noise), B = 1 and B = 32, and one
row of 90 s.  Per measurement: warm-up, then >= 15 calls timed with device events, median; three rounds, the per-round medians kept.
The two kernels are not timed apart here (their launches are back to back on one stream): the kernel trace does that.
One JSON line per measurement on stdout.
    python tools/pyin_bench.py [--calls 20] [--rounds 3] > profiles/r11/pyin_bench.jsonl
    python tools/pyin_bench.py --kernel-only       (five calls per shape, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))
SR, HOP = 22050, 256


def speech_like(seed, n):
    rng = np.random.default_rng(seed)
    y, pos, phase = np.zeros(n), 0, 0.0
    while pos < n:
        end = min(n, pos + int(rng.integers(8, 30)) * HOP)
        kind, m = rng.choice(3, p=[0.6, 0.2, 0.2]), end - pos
        if kind == 0:
            f_a = rng.uniform(80, 400)
            f = np.linspace(f_a, float(np.clip(f_a * rng.uniform(0.75, 1.25), 80, 400)), m)
            ph = phase + 2 * np.pi * np.cumsum(f) / SR
            y[pos:end] = 0.3 * sum(a * np.sin((i + 1) * ph) for i, a in enumerate((1.0, 0.5, 0.3, 0.2)))
            phase = ph[-1] % (2 * np.pi)
        elif kind == 2:
            y[pos:end] = rng.normal(0, 0.05, m)
        pos = end
    return (y + rng.normal(0, 1e-3, n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    import torch
    from ttsamd.engine import PyinEngine
    eng = PyinEngine(65.40639132514966, 2093.004522404789, frame_length=1024, hop_length=256)

    def timed(fn, calls):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    for name, B, secs in (('10 s b1', 1, 10), ('10 s b32', 32, 10), ('90 s b1', 1, 90)):
        n = secs * SR
        x = torch.from_numpy(np.stack([speech_like(100 + b, n) for b in range(B)])).to('cuda:0')
        T = eng.frames(n)
        if a.kernel_only:
            for _ in range(5):
                eng.forward(x)
            torch.cuda.synchronize()
            continue
        f0, flag, prob, frames = eng.forward(x)
        r = [timed(lambda: eng.forward(x), max(a.calls, 15)) for _ in range(a.rounds)]
        med = float(np.median(r))
        print(json.dumps({'what': f'pyin {name}', 'batch': B, 'samples': n, 'frames': T, 'call_ms': round(med, 3),
                          'call_ms_per_round': [round(v, 3) for v in r], 'call_us_per_frame_step': round(med * 1e3 / T, 3),
                          'voiced_share': round(float(flag.float().mean()), 3),
                          'workspace_mb': round(eng.workspace_bytes(B, T) / 1e6, 1)}), flush=True)


if __name__ == '__main__':
    main()

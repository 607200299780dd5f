"""Polyphase resampler (csrc/resample.hip): milliseconds per call through ttsamd.engine.ResampleEngine for rows of 10 s at 48 kHz ->
22 050 Hz, B = 1 and B = 32, lowpass_filter_width 64 and 1024, on the general kernel, on the MFMA kernel and on the automatic route, and the
same polyphase table through torch-ROCm's F.conv1d(stride=o) -- what torchaudio.functional.resample executes.  Per measurement: warm-up, then >= 15 calls timed with device events, median; three rounds, the
per-round medians kept.  One JSON line per measurement on stdout; `tf` = 2 n J frames B / time in TFLOP/s (useful FLOPs: phases not
padded), `peak_share` = that over the 157.3 TFLOP/s fp32 matrix peak.
    python tools/resample_bench.py [--calls 20] [--rounds 3] > profiles/r12/resample_bench.jsonl
    python tools/resample_bench.py --sweep > profiles/r12/resample_sweep.jsonl      (B = 1 .. 16 rows of 1 s / 10 s, the kernels only)
    python tools/resample_bench.py --kernel-only       (five calls per shape and route, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))
ORIG, NEW, PEAK_TF = 48000, 22050, 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--sweep', action='store_true', help='small batches, the two kernels only: where the automatic route should switch')
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ttsamd.engine import ResampleEngine
    from ttsamd.resample import resample_taps

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

    rng = np.random.default_rng(0)
    for lfw in (64, 1024):
        eng = ResampleEngine(ORIG, NEW, lowpass_filter_width=lfw)
        taps, width, o, n = resample_taps(ORIG, NEW, lfw)
        w_t = torch.from_numpy(np.array(taps)).to('cuda:0')[:, None]
        for B, secs in (((1, 1), (4, 1), (1, 10), (2, 10), (3, 10), (4, 10), (6, 10), (8, 10), (12, 10), (16, 10)) if a.sweep else ((1, 10), (32, 10))):
            L = secs * ORIG
            x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(B, L)).astype(np.float32)).to('cuda:0')
            flop = 2.0 * n * taps.shape[1] * (L // o) * B

            def conv():
                return F.conv1d(F.pad(x[:, None], (width, width + o)), w_t, stride=o).transpose(1, 2).reshape(B, -1)

            routes = [('general', lambda: eng.forward(x, route='general')), ('mfma', lambda: eng.forward(x, route='mfma')),
                      ('auto', lambda: eng.forward(x)), ('torch conv1d', conv)][:2 if a.sweep else 4]
            for name, fn in routes:
                if a.kernel_only:
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    continue
                r = [timed(fn, max(a.calls, 15)) for _ in range(a.rounds)]
                med = float(np.median(r))
                print(json.dumps({'what': f'resample {ORIG} -> {NEW} lfw {lfw} b{B} x {secs} s {name}', 'batch': B, 'samples': L, 'o': o, 'n': n,
                                  'taps_per_phase': int(taps.shape[1]), 'call_ms': round(med, 4),
                                  'call_ms_per_round': [round(v, 4) for v in r], 'tf': round(flop / med / 1e9, 2),
                                  'peak_share': round(flop / med / 1e9 / PEAK_TF, 3)}), flush=True)


if __name__ == '__main__':
    main()

"""Oversmoothing kernels (csrc/oversmooth.hip): microseconds per call and cells per second of the DTW at the bench's utterance
(449 x 430 frames) and config 1's longest line (2 291 x 2 100), M = 1 and M = 80, one pair and 32 pairs; the series and summary kernels at
32 x 449 frames; the whole scoring call (ttsamd.engine.oversmoothing_score: 32 pairs = 128 alignments).  Per measurement: warm-up, then
>= 15 calls timed with device events, median; three rounds, the per-round medians kept.  One JSON line per measurement.
There is no baseline to divide by: the reference's DTW is numba code, numba is no dependency, and its text run as plain Python takes
seconds per alignment (about 1.5 s for 180 x 160 x 80), which is not what its users run.
    python tools/oversmoothing_bench.py [--calls 20] [--rounds 3]
    python tools/oversmoothing_bench.py --kernel-only      (the HIP calls alone, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    import torch
    from ttsamd import engine as E
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(11)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(a.calls, 15)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def rounds(fn):
        return [timed(fn) for _ in range(a.rounds)]

    def walk(B, M, T):                                             # smooth random walks: a realistic, wandering path
        return torch.cumsum(torch.randn(B, M, T, generator=g), dim=2).mul_(0.3).to(dev)

    base = {}
    for ta, tb in ((449, 430), (2291, 2100)):
        for M in (1, 80):
            for B in (1, 32):
                if M == 80 and B == 32 and ta > 1000:
                    continue                                       # 32 x 4.8 M cells x 80 channels: minutes of calls, nothing new
                x, y = walk(B, M, ta), walk(B, M, tb)
                if a.kernel_only:
                    for _ in range(5):
                        E.dtw(x, y)
                    torch.cuda.synchronize()
                    continue
                r = rounds(lambda: E.dtw(x, y))
                med = float(np.median(r))
                base[(ta, M, B)] = med
                rec = {'what': 'dtw', 'ta': ta, 'tb': tb, 'channels': M, 'pairs': B, 'us': round(med * 1e3, 1),
                       'us_per_round': [round(v * 1e3, 1) for v in r], 'cells_per_s': round(B * ta * tb / med * 1e3),
                       'workspace_bytes': int(E.L.load().ttsamd_dtw_workspace_bytes(B, ta, tb, M))}
                if B == 32:
                    rec['b32_over_b1'] = round(med / base[(ta, M, 1)], 2)
                print(json.dumps(rec), flush=True)
    mel = (torch.randn(32, 80, 449, generator=g) * 2.0 - 4.0).to(dev)
    ref = (mel[:, :, :430] + 0.05 * torch.randn(32, 80, 430, generator=g).to(dev)).contiguous()
    series = E.cepstral_series(mel)
    if a.kernel_only:
        for _ in range(20):
            E.cepstral_series(mel)
            E.series_summary(series)
            E.oversmoothing_score(mel, None, ref, None)
        torch.cuda.synchronize()
        return
    for what, fn in (('cepstral_series 32 x 449 x 80', lambda: E.cepstral_series(mel)), ('series_summary 128 x 449', lambda: E.series_summary(series)),
                     ('oversmoothing_score 32 pairs 449 x 430 x 80', lambda: E.oversmoothing_score(mel, None, ref, None))):
        r = rounds(fn)
        print(json.dumps({'what': what, 'us': round(float(np.median(r)) * 1e3, 1), 'us_per_round': [round(v * 1e3, 1) for v in r]}), flush=True)


if __name__ == '__main__':
    main()

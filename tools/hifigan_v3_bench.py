"""HiFi-GAN V3 (ResBlock2) vocoder alone on the bench's synthetic shapes: batch 1 / 8 / 32 of the bench's utterance lengths
(64 tokens, synth.synth_durations: 2..12 frames per token) with seeded mel values, V3 weights from synth.hifigan_state_dict.
Per shape: warm-up, then >= 10 calls timed with device events, median.  Prints ms per call, audio samples/s and the share of the
fp32 MFMA peak on the algorithmic work computed from the config, for every ResBlock2 pair fused (TTSAMD_RESBLOCK2_PAIR=3f) and
none (=0, the default), alternated in the same run, and V1 (the shipped config) on the same mels for scale.  One JSON line per measurement.
    python tools/hifigan_v3_bench.py [--calls 20] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tts-arabic-pytorch_amd'))

PEAK_F32_TFLOPS = 157.3     # v_mfma_f32_32x32x2f32, MI355X (256 CUs at 2.4 GHz)


def flops_per_frame(h):
    """Algorithmic FLOPs of one mel frame through the generator (multiply-adds x 2), from the config alone."""
    mels = h.get('num_mels', 80)
    c = h['upsample_initial_channel']
    f = 2.0 * c * mels * 7                                   # conv_pre
    mul = 1
    n_convs = 2 if str(h.get('resblock', '1')) == '2' else 2 * len(h['resblock_dilation_sizes'][0])
    for u, k in zip(h['upsample_rates'], h['upsample_kernel_sizes']):
        cout = c // 2
        mul *= u
        f += 2.0 * c * cout * k / u * mul                     # ConvTranspose1d: k / u taps per output sample
        c = cout
        f += sum(n_convs * 2.0 * c * c * kk * mul for kk in h['resblock_kernel_sizes'])
    f += 2.0 * c * 7 * mul                                   # conv_post
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3, help='alternations of RESBLOCK2_PAIR=3f and =0')
    a = ap.parse_args()
    import torch
    from ttsamd import lib, synth
    from ttsamd.config import HIFIGAN_CONFIG, HIFIGAN_V3_CONFIG
    from ttsamd.engine import HifiGanEngine
    dev = torch.device('cuda:0')
    engines = {'v3': HifiGanEngine(synth.hifigan_state_dict(HIFIGAN_V3_CONFIG), HIFIGAN_V3_CONFIG, device=dev),
               'v1': HifiGanEngine(synth.hifigan_state_dict(), HIFIGAN_CONFIG, device=dev)}
    fpf = {'v3': flops_per_frame(HIFIGAN_V3_CONFIG), 'v1': flops_per_frame(HIFIGAN_CONFIG)}
    print(json.dumps({'mflop_per_frame': {k: round(v / 1e6, 3) for k, v in fpf.items()}}))
    lens_all = synth.synth_durations(32, 64).sum(axis=1).astype(np.int64)

    def timed(eng, mel, lens):
        for _ in range(3):
            eng.forward(mel, lens)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.forward(mel, lens)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    for B in (1, 8, 32):
        lens_h = lens_all[:B]
        T = int(lens_h.max())
        rng = np.random.default_rng(B)
        mel = torch.from_numpy((rng.standard_normal((B, 80, T)) * 1.5 - 4.0).astype(np.float32)).to(dev)
        lens = torch.from_numpy(lens_h).to(dev)
        frames = int(lens_h.sum())
        runs = {}
        for r in range(a.rounds):
            for name, mask in (('v3_fused', '3f'), ('v3_unfused', 0)):
                with lib.options(TTSAMD_RESBLOCK2_PAIR=mask):
                    runs.setdefault(name, []).append(timed(engines['v3'], mel, lens))
        runs['v1'] = [timed(engines['v1'], mel, lens)]
        for name, ms_l in runs.items():
            ms = float(np.median(ms_l))
            work = fpf['v1' if name == 'v1' else 'v3'] * frames
            print(json.dumps({'batch': B, 'frames': frames, 'route': name, 'ms': round(ms, 4), 'ms_per_round': [round(m, 4) for m in ms_l],
                              'samples_per_s': round(256 * frames / ms * 1e3), 'tflops': round(work / ms / 1e9, 2),
                              'frac_f32_peak': round(work / ms / 1e9 / PEAK_F32_TFLOPS, 4)}))


if __name__ == '__main__':
    main()

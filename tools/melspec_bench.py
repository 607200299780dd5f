"""Mel analysis kernel (csrc/melspec.hip) against the reference's own module with its tensors on the GPU, and MelVocos('24k') beside
'22k'.  Shapes: the bench's B = 32 batch (64 tokens of synth.synth_durations frames, 256 samples per frame, every row padded to the
longest as the reference's module takes it) and its first utterance alone.  Per measurement: warm-up, then >= 15 calls timed with device
events, median; the routes alternate in three rounds in the same process, the per-round medians are kept so that the run-to-run
spread is visible next to every difference.  One JSON line per measurement.
    python tools/melspec_bench.py [--calls 20] [--rounds 3]
    python tools/melspec_bench.py --kernel-only      (the HIP calls alone, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29      # MI355X: HBM3E spec, and what a float4 copy measures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ttsamd import melfb, synth
    from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG
    from ttsamd.engine import MelSpecEngine, VocosEngine
    dev = torch.device('cuda:0')
    lens_f = synth.synth_durations(32, 64).sum(axis=1).astype(np.int64)
    g = torch.Generator().manual_seed(7)

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

    configs = {
        'audio (same, sqrt(|X|^2+1e-9), linear, 80 slaney bands)':
            (melfb.mel_filterbank(22050, 1024, 80, 0, 8000.0, 'slaney', 'slaney'), 'same', 'eps', None),
        'vocos 24k (center, |X|, log, 100 htk bands)': (melfb.mel_filterbank(24000, 1024, 100), 'center', 'abs', 1e-5),
    }
    win = torch.hann_window(1024, device=dev)
    for cname, (fb, framing, mag, clip) in configs.items():
        eng = MelSpecEngine(fb, framing, mag, clip, device=dev)
        fbd = torch.from_numpy(fb).to(dev)

        def ref(x):                                   # utils/audio.py:35-46 / feature_extractors.py:58-64 with the tensors on the GPU
            if framing == 'same':
                x = F.pad(x[:, None], (384, 384), mode='reflect')[:, 0]
            s = torch.stft(x, 1024, 256, 1024, win, center=framing == 'center', pad_mode='reflect', return_complex=True)
            m = s.abs().pow_(2).add_(1e-9).sqrt_() if mag == 'eps' else s.abs()
            m = torch.matmul(fbd, m)
            return torch.log(torch.clip(m, min=clip)) if clip else m

        for B in (32, 1):
            n = int(lens_f[:B].max()) * 256
            x = (torch.randn(B, n, generator=g) * 0.1).to(dev)
            ns = torch.from_numpy(lens_f[:B] * 256).to(dev)
            if a.kernel_only:
                for _ in range(20):
                    eng.forward(x)
                torch.cuda.synchronize()
                continue
            out, want = eng.forward(x)[0], ref(x)
            err = float((out - want).abs().max())
            runs = {}
            for _ in range(a.rounds):
                runs.setdefault('hip', []).append(timed(lambda: eng.forward(x)))
                runs.setdefault('torch_reference_module', []).append(timed(lambda: ref(x)))
                runs.setdefault('hip_ragged', []).append(timed(lambda: eng.forward(x, ns)))
            med = {k: float(np.median(v)) for k, v in runs.items()}
            nbytes = B * (4 * n + 4 * fb.shape[0] * (n // 256))
            rag_bytes = int((4 * lens_f[:B] * 256 + 4 * fb.shape[0] * lens_f[:B]).sum())
            print(json.dumps({'what': 'melspec', 'config': cname, 'batch': B, 'samples_per_row': n, 'max_abs_diff_vs_torch': err,
                              'ms': {k: round(v, 4) for k, v in med.items()}, 'ms_per_round': {k: [round(m, 4) for m in v] for k, v in runs.items()},
                              'torch_over_hip': round(med['torch_reference_module'] / med['hip'], 2),
                              'algorithmic_bytes': nbytes, 'hip_call_GBs': round(nbytes / med['hip'] / 1e6, 1),
                              'hip_call_frac_hbm_peak': round(nbytes / med['hip'] / 1e9 / HBM_PEAK_TBS, 4),
                              'hip_call_frac_hbm_copy': round(nbytes / med['hip'] / 1e9 / HBM_COPY_TBS, 4),
                              'hip_ragged_GBs': round(rag_bytes / med['hip_ragged'] / 1e6, 1)}), flush=True)
    if a.kernel_only:
        return
    # MelVocos('24k') beside '22k' on the same frame counts: the same backbone but for the embed conv (100 -> 104 against 80 input channels,
    # one channel-padding launch) and the overlap-add's trimming
    T = int(lens_f.max())
    lens = torch.from_numpy(lens_f).to(dev)
    engines = {'22k': VocosEngine(synth.vocos_state_dict(VOCOS_22K_CONFIG), VOCOS_22K_CONFIG, device=dev),
               '24k': VocosEngine(synth.vocos_state_dict(VOCOS_24K_CONFIG), VOCOS_24K_CONFIG, device=dev)}
    mels = {k: (torch.randn(32, e.n_mels, T, generator=g) * 1.5 - 4.0).to(dev) for k, e in engines.items()}
    runs = {}
    for _ in range(a.rounds):
        for k, e in engines.items():
            runs.setdefault(k, []).append(timed(lambda: e.forward(mels[k], lens)))
    print(json.dumps({'what': 'vocos_forward', 'batch': 32, 'frames': int(lens_f.sum()), 't_max': T,
                      'ms': {k: round(float(np.median(v)), 4) for k, v in runs.items()},
                      'ms_per_round': {k: [round(m, 4) for m in v] for k, v in runs.items()}}), flush=True)


if __name__ == '__main__':
    main()

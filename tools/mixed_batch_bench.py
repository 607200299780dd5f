"""Mixed requests in one batch against one call per distinct option tuple.  Workload: 32 requests of the bench's 64-token utterances
(synth.synth_ids) over 4 speakers x 4 speeds = 16 distinct (speaker_id, speed) tuples, two requests each, on the four-speaker synthetic
FastPitch + HiFi-GAN through the drop-in `FastPitch2Wave.tts` (tokens in, CPU waves out, denoise 0.005):
    mixed      ONE tts(32 lines, batch_size=32, speaker_id=[...], speed=[...]) call
    per_tuple  the same requests as a caller without per-line lists has to run them: 16 tts(2 lines, speaker_id=k, speed=s) calls
    uniform    for scale: ONE tts(32 lines, batch_size=32, speaker_id=0, speed=1.0) call, all scalars (padded-batch arithmetic)
The two legs are NOT like for like in FastPitch: `mixed` computes its 32 rows as if alone (what per-line lists select), `per_tuple` runs
the reference's padded-batch arithmetic on each pair, so predicted durations and with them a wave's length can differ between the legs
(`same_lengths`, `frames` / `frames_per_tuple` in the result line); the ratio compares what the two callers actually run.
Per measurement: warm-up, then >= 15 calls timed with device events, median; the two alternate in three rounds in the same process and the
per-round medians are kept.  One JSON line.
    python tools/mixed_batch_bench.py [--calls 15] [--rounds 3]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    import torch
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    dev = torch.device('cuda:0')
    cfg4 = dict(NET_CONFIG, n_speakers=4)
    with tempfile.TemporaryDirectory() as d:
        torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in synth.fastpitch_state_dict(cfg4).items()}, 'config': cfg4,
                    'symbols': list(text.symbols)}, os.path.join(d, 'fp4.pth'))
        torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth.hifigan_state_dict().items()}}, os.path.join(d, 'hg.pth'))
        with open(os.path.join(d, 'config.json'), 'w') as f:
            json.dump(HIFIGAN_CONFIG, f)
        model = FastPitch2Wave(os.path.join(d, 'fp4.pth'), vocoder_sd=os.path.join(d, 'hg.pth'), vocoder_config=os.path.join(d, 'config.json')).to(dev)
    # the bench's utterances are token ids, not text: line 'u<i>' tokenises to row i of synth_ids
    ids = synth.synth_ids(32, 64)
    tokens = {f'u{i}': [text.symbols[j] for j in row] for i, row in enumerate(ids.tolist())}
    model.model._tokenize = lambda line, vowelizer=None: tokens[line]
    lines = list(tokens)
    speeds = [0.8, 1.0, 1.25, 1.5]
    speaker_id = [i % 4 for i in range(32)]
    speed = [speeds[(i // 4) % 4] for i in range(32)]
    tuples = sorted(set(zip(speaker_id, speed)))
    assert len(tuples) == 16

    def mixed():
        return model.tts(lines, batch_size=32, speaker_id=speaker_id, speed=speed)

    def per_tuple():
        out = [None] * 32
        for k, s in tuples:
            idx = [i for i in range(32) if (speaker_id[i], speed[i]) == (k, s)]
            for i, w in zip(idx, model.tts([lines[i] for i in idx], batch_size=32, speaker_id=k, speed=s)):
                out[i] = w
        return out

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

    wa, wb = mixed(), per_tuple()
    same_len = all(x.shape == y.shape for x, y in zip(wa, wb))
    err = max(float((x - y).abs().max()) for x, y in zip(wa, wb)) if same_len else None
    def uniform():
        return model.tts(lines, batch_size=32, speaker_id=0, speed=1.0)

    runs = {'mixed': [], 'per_tuple': [], 'uniform': []}
    for _ in range(a.rounds):
        runs['mixed'].append(timed(mixed))
        runs['per_tuple'].append(timed(per_tuple))
        runs['uniform'].append(timed(uniform))
    med = {k: float(np.median(v)) for k, v in runs.items()}
    print(json.dumps({'what': 'mixed_batch', 'requests': 32, 'n_tokens': 64, 'distinct_tuples': len(tuples),
                      'frames': int(sum(w.numel() for w in wa) // 256), 'frames_per_tuple': int(sum(w.numel() for w in wb) // 256),
                      'frames_uniform': int(sum(w.numel() for w in uniform()) // 256), 'same_lengths': same_len, 'max_abs_diff_mixed_vs_per_tuple': err,
                      'ms': {k: round(v, 3) for k, v in med.items()}, 'ms_per_round': {k: [round(m, 3) for m in v] for k, v in runs.items()},
                      'per_tuple_over_mixed': round(med['per_tuple'] / med['mixed'], 2)}), flush=True)


if __name__ == '__main__':
    main()

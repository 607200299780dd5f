"""Forced alignment (csrc/aligner.hip): milliseconds per FastPitch-aligner call -- encoders, attention, MAS -- through ttsamd.engine.AlignerEngine
at the bench's 64-token inputs (B = 1 and B = 32, each utterance with the mel FastPitch itself gives it, so with its own length) and one long
utterance (300 tokens, about 2 300 frames); MAS alone on the same attention maps; and beside each the reference's route restated with torch
on the same GPU: the ConvAttention in torch (F.conv1d, broadcast difference, softmax), torch.log, a copy to the host, mas_width1 row by row
in NumPy per utterance, and a copy back (model.py:246-257).  The reference runs its MAS under numba, which is no dependency here; the NumPy
rows are the nearest thing that runs, and the route's device part and its host part are reported apart so that each can be judged alone.
Per measurement: warm-up, then >= 15 calls timed with device events around work that ends in a synchronise, median; three rounds, the
per-round medians kept.  One JSON line per measurement, written to stdout.
    python tools/aligner_bench.py [--calls 20] [--rounds 3] > profiles/r10/aligner_bench.jsonl
    python tools/aligner_bench.py --kernel-only      (the library's calls alone, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))
GAIN = 8.0                                                       # as tests/golden/aligner.npz: a peaked attention, a real path


def torch_route(sd, ids, in_lens, mel, mel_lens):
    """-> (dur [B, L] on the device, seconds spent on the host side of MAS).  The reference's aligner path with its tensors on the GPU."""
    import torch
    import torch.nn.functional as F
    k = sd['encoder.word_emb.weight'][ids].permute(0, 2, 1)
    k = F.conv1d(F.relu(F.conv1d(k, sd['attention.key_proj.0.conv.weight'], sd['attention.key_proj.0.conv.bias'], padding=1)),
                 sd['attention.key_proj.2.conv.weight'], sd['attention.key_proj.2.conv.bias'])
    q = F.relu(F.conv1d(mel, sd['attention.query_proj.0.conv.weight'], sd['attention.query_proj.0.conv.bias'], padding=1))
    q = F.relu(F.conv1d(q, sd['attention.query_proj.2.conv.weight'], sd['attention.query_proj.2.conv.bias']))
    q = F.conv1d(q, sd['attention.query_proj.4.conv.weight'], sd['attention.query_proj.4.conv.bias'])
    attn = -0.0005 * ((q[:, :, :, None] - k[:, :, None]) ** 2).sum(1, keepdim=True)
    mask = torch.arange(ids.shape[1], device=ids.device)[None, None, None, :] >= in_lens[:, None, None, None]
    soft = torch.softmax(attn.masked_fill(mask, -float('inf')), dim=3)
    log_attn = torch.log(soft).to(device='cpu', dtype=torch.float32).numpy()
    t0 = time.perf_counter()
    il, ol = in_lens.cpu().numpy(), mel_lens.cpu().numpy()
    hard = np.zeros(log_attn.shape, np.float32)
    for b in range(log_attn.shape[0]):
        log_p = log_attn[b, 0, :ol[b], :il[b]].copy()
        log_p[0, 1:] = -np.inf
        for i in range(1, log_p.shape[0]):
            prev = log_p[i - 1]
            left = np.concatenate([[np.float32(-np.inf)], prev[:-1]])
            log_p[i] += np.maximum(left, prev)
        j = log_p.shape[1] - 1
        for i in range(log_p.shape[0] - 1, 0, -1):
            hard[b, 0, i, j] = 1
            if j > 0 and log_p[i - 1, j - 1] >= log_p[i - 1, j]:
                j -= 1
        hard[b, 0, 0, j] = 1
    host = time.perf_counter() - t0
    return torch.from_numpy(hard).to(ids.device).sum(2)[:, 0, :], host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    import torch
    from ttsamd import engine as E
    from ttsamd import synth
    dev = torch.device('cuda:0')
    sd = synth.fastpitch_state_dict()
    sd.update(synth.fastpitch_aligner_state_dict(gain=GAIN))
    fp, al = E.FastPitchEngine(sd), E.AlignerEngine(sd)
    sd_t = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if k in E.ALIGNER_KEYS}

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

    def rounds(fn, calls=None):
        return [timed(fn, max(a.calls, 15) if calls is None else calls) for _ in range(a.rounds)]

    for name, B, Lt in (('bench b1', 1, 64), ('bench b32', 32, 64), ('long', 1, 300)):
        ids = torch.from_numpy(synth.synth_ids(B, Lt)).to(dev)
        dur0 = torch.from_numpy(synth.synth_durations(B, Lt)).to(dev)
        mel, mel_lens, *_ = fp.infer(ids, dur_tgt=dur0)          # the utterances' own mels and lengths
        mel = mel.contiguous()
        T = mel.shape[2]
        in_lens = (ids != 0).sum(1)
        soft, _, _ = al.attention(ids, mel)
        soft = soft.clone()
        if a.kernel_only:
            for _ in range(5):
                al.align(ids, mel, mel_lens)
            torch.cuda.synchronize()
            continue
        dur = al.align(ids, mel, mel_lens)
        dur_ref, _ = torch_route(sd_t, ids, in_lens, mel, mel_lens)
        same = bool(torch.equal(dur, dur_ref))
        r_align = rounds(lambda: al.align(ids, mel, mel_lens))
        r_mas = rounds(lambda: E.mas(soft, in_lens, mel_lens, is_log=False, return_hard=False))
        r_mas_hard = rounds(lambda: E.mas(soft, in_lens, mel_lens, is_log=False))
        host = []
        r_ref = rounds(lambda: host.append(torch_route(sd_t, ids, in_lens, mel, mel_lens)[1]), calls=5 if B * T > 4000 else 15)
        med = lambda r: float(np.median(r))  # noqa: E731
        print(json.dumps({
            'what': f'align {name}', 'batch': B, 'tokens': Lt, 'frames': T, 'frames_min': int(mel_lens.min()),
            'align_us': round(med(r_align) * 1e3, 1), 'align_us_per_round': [round(v * 1e3, 1) for v in r_align],
            'mas_us': round(med(r_mas) * 1e3, 1), 'mas_us_per_round': [round(v * 1e3, 1) for v in r_mas],
            'mas_with_attn_hard_us': round(med(r_mas_hard) * 1e3, 1),
            'mas_us_per_frame_row': round(med(r_mas) * 1e3 / T, 3),
            'mas_workspace_bytes': int(E.L.load().ttsamd_mas_workspace_bytes(B, T, Lt)),
            'torch_route_us': round(med(r_ref) * 1e3, 1), 'torch_route_us_per_round': [round(v * 1e3, 1) for v in r_ref],
            'torch_route_host_mas_us': round(float(np.median(host)) * 1e6, 1),
            'torch_route_over_align': round(med(r_ref) / med(r_align), 1),
            'durations_equal_torch_route': same}), flush=True)


if __name__ == '__main__':
    main()

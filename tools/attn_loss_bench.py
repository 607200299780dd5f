"""Alignment prior and alignment scores (csrc/attn_loss.hip): microseconds per call at B = 32, T = 860 frames, L = 200 tokens (ragged: the
rows' lengths run from 60 % to 100 % of the padded size) of
  prior_exact / prior_interpolated   ttsamd_attn_prior, one launch, [B, T, L] fp32 out
  forward_sum                        ttsamd_attn_ctc_loss, two launches (per-frame normalisers, then the chain: one block per row)
  binarization                       ttsamd_attn_bin_loss, one launch
and for orientation, on the same shape and lengths,
  mas                                ttsamd_mas (durations only) on the same log-attention: the existing chain of the same shape
  torch_ctc_loss                     torch.nn.functional.ctc_loss (float64, reduction='none') on the device with the inputs AttentionCTCLoss
                                     builds (blank column, mask, log_softmax; their cost is reported apart as torch_ctc_prepare), if it runs
                                     on this torch build; its rows are compared with forward_sum's.
Per measurement: warm-up, then >= 15 calls timed with device events around work that ends in a synchronise, median; three rounds, the
per-round medians kept.  One JSON line per measurement, written to stdout.
    python tools/attn_loss_bench.py [--calls 20] [--rounds 3] > profiles/r16/attn_loss_bench.jsonl
    python tools/attn_loss_bench.py --kernel-only      (the library's calls alone, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
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
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=860)
    ap.add_argument('--tokens', type=int, default=200)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from ttsamd import engine as E
    dev = torch.device('cuda:0')
    B, T, Lt = a.batch, a.frames, a.tokens
    rng = np.random.default_rng(0)
    frac = np.linspace(1.0, 0.6, B)
    in_lens = torch.from_numpy(np.maximum(1, np.round(frac * Lt)).astype(np.int64)).to(dev)
    out_lens = torch.from_numpy(np.maximum(1, np.round(frac * T)).astype(np.int64)).to(dev)
    # a log-attention with a diagonal ridge, as an aligner gives: log_softmax over the tokens
    t, l = np.arange(T)[None, :, None] / T, np.arange(Lt)[None, None, :] / Lt
    raw = rng.normal(0, 1.5, (B, T, Lt)) - 3.0 * np.abs(t - l) * np.sqrt(Lt)
    logprob = torch.log_softmax(torch.from_numpy(raw.astype(np.float32)).to(dev), dim=2).contiguous()
    soft = torch.softmax(logprob.masked_fill(torch.arange(Lt, device=dev)[None, None, :] >= in_lens[:, None, None], -float('inf')), dim=2)
    _, hard = E.mas(soft, in_lens, out_lens, is_log=False)

    calls = {
        'prior_exact': lambda: E.attention_prior(in_lens, out_lens, n_tokens=Lt, n_frames=T, mode='exact'),
        'prior_interpolated': lambda: E.attention_prior(in_lens, out_lens, n_tokens=Lt, n_frames=T, mode='interpolated'),
        'forward_sum': lambda: E.forward_sum_loss(logprob, in_lens, out_lens),
        'binarization': lambda: E.binarization_loss(hard, soft),
        'mas': lambda: E.mas(logprob, in_lens, out_lens, is_log=True, return_hard=False),
    }
    if a.kernel_only:
        for fn in calls.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return

    def timed(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def report(name, fn, **extra):
        r = [timed(fn, max(a.calls, 15)) for _ in range(a.rounds)]
        print(json.dumps({'what': name, 'batch': B, 'frames': T, 'tokens': Lt, 'us': round(float(np.median(r)) * 1e3, 1),
                          'us_per_round': [round(v * 1e3, 1) for v in r], **extra}), flush=True)

    for name, fn in calls.items():
        extra = {}
        if name.startswith('prior'):
            extra['out_bytes'] = B * T * Lt * 4
        if name == 'forward_sum':
            extra['workspace_bytes'] = int(E.L.load().ttsamd_attn_ctc_loss_workspace_bytes(B, T, Lt))
            extra['us_per_frame'] = round(timed(fn, 15) * 1e3 / T, 3)
        report(name, fn, **extra)

    # torch's own CTC on the device, with the inputs the reference's AttentionCTCLoss builds
    def prepare():
        x = F.pad(logprob.double().permute(1, 0, 2), (1, 0, 0, 0, 0, 0), value=-1.0)
        x = x.masked_fill(torch.arange(Lt + 1, device=dev).view(1, 1, -1) > in_lens.view(1, -1, 1), -float('inf'))
        return torch.log_softmax(x, dim=-1)
    try:
        targets = torch.arange(1, Lt + 1, device=dev).unsqueeze(0).repeat(B, 1)
        x = prepare()
        ctc = lambda: F.ctc_loss(x, targets, out_lens, in_lens, blank=0, reduction='none')   # noqa: E731
        rows = ctc()
        torch.cuda.synchronize()
        mine = E.forward_sum_loss(logprob, in_lens, out_lens)
        rel = float(((rows - mine).abs() / mine.abs()).max())
        report('torch_ctc_loss', ctc, dtype='float64', largest_relative_difference_from_forward_sum=rel)
        report('torch_ctc_prepare', prepare)
    except Exception as e:                                       # this torch build may not carry the kernel
        print(json.dumps({'what': 'torch_ctc_loss', 'error': f'{type(e).__name__}: {e}'[:300]}), flush=True)


if __name__ == '__main__':
    main()

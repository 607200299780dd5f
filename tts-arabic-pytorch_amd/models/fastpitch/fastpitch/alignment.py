"""Drop-in for the reference's models/fastpitch/fastpitch/alignment.py: `mas_width1` and `b_mas` with the reference's signatures, run by
ttsamd_mas (csrc/aligner.hip), which reproduces mas_width1 decision for decision in fp32.  NumPy in gives NumPy out, as in the reference
(one copy to the device and one back); tensors on the device are accepted and stay there.  The general-width `mas` is not built: the
reference itself only ever calls width 1 (model.py:253,269).  One token (`in_lens[b] == 1`): the reference indexes out of bounds there;
every frame goes to token 0.  No CPU fallback: without a gfx950 device every call raises."""
import numpy as np
import torch

from ttsamd import engine as _engine
from ttsamd.lib import TtsAmdError


def _to_device(x):
    if isinstance(x, torch.Tensor):
        if x.device.type != 'cuda':
            raise TtsAmdError('alignment: a tensor must live on the ROCm device (NumPy arrays are copied there)')
        return x, False
    _engine._require_gpu()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to('cuda:0'), True


def mas_width1(log_attn_map):
    """log_attn_map [T, L] (mel x text) -> the 0 / 1 path of the same shape and float32"""
    x, host = _to_device(log_attn_map)
    if x.dim() != 2:
        raise ValueError(f'mas_width1: expected [T, L], got {tuple(x.shape)}')
    T, Lt = x.shape
    lens = torch.tensor([Lt, T], dtype=torch.int64, device=x.device)
    _, hard = _engine.mas(x[None], lens[:1], lens[1:], is_log=True)
    return hard[0].cpu().numpy() if host else hard[0]


def b_mas(b_log_attn_map, in_lens, out_lens, width=1):
    """b_log_attn_map [B, 1, T, L] -> attn_out of the same shape: mas_width1 on every row's [:out_lens[b], :in_lens[b]] corner, zero
    outside it"""
    assert width == 1
    x, host = _to_device(b_log_attn_map)
    if x.dim() != 4 or x.shape[1] != 1:
        raise ValueError(f'b_mas: expected [B, 1, T, L], got {tuple(x.shape)}')
    as_lens = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v).astype(np.int64)))  # noqa: E731
    _, hard = _engine.mas(x, as_lens(in_lens), as_lens(out_lens), is_log=True)
    return hard.cpu().numpy() if host else hard

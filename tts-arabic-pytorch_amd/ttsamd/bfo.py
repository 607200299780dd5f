"""Kernel-level access to the bf16 octet engine (csrc/bfo*.hip, include/ttsamd.h ttsamd_bfo_* / ttsamd_bfo3_*): layout converters,
weight packing and single layers.  Used by the parity tests and tools/bfo_bench.py; the model forwards reach the
same kernels through ttsamd_hifigan_forward under set_precision('bf16') / set_precision('bf16x3').

Every layer is written once, in _Mode, for the engine's two modes: plain bf16 (pack, conv1d, ...: tensors stored as int16
[B, C/8, L, 8]) and split bf16, "x3" (pack3, conv1d3, ...: every value = hi + lo, int16 [B, C/8, L, 16] -- 32 bytes per octet and
position, two halves of hi 4 | lo 4 bf16)."""
import ctypes as C

import numpy as np
import torch

from . import lib as L


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Mode:
    def __init__(self, prefix, last):
        self.prefix, self.last = prefix, last           # symbol prefix, int16 elements per (octet, position)

    def _call(self, name, *args):
        L.check(getattr(L.load(), f'ttsamd_{self.prefix}_{name}')(*args), f'{self.prefix}_{name}')

    def pack(self, x, slope=1.0):
        """fp32 [B, C, L] (device) -> the mode's tensor [B, C/8, L, 8 or 16] (int16), activated with leaky_relu(slope)."""
        x = x.contiguous().float()
        B, Cn, Ln = x.shape
        out = torch.empty(B, Cn // 8, Ln, self.last, dtype=torch.int16, device=x.device)
        self._call('pack', _ptr(x), B, Cn, Ln, float(slope), _ptr(out), _stream())
        return out

    def unpack(self, t, slope=1.0):
        """The mode's tensor [B, C/8, L, 8 or 16] -> fp32 [B, C, L]; slope != 1 undoes the activation the tensor was stored with."""
        B, no, Ln, _ = t.shape
        out = torch.empty(B, no * 8, Ln, dtype=torch.float32, device=t.device)
        self._call('unpack', _ptr(t), B, no * 8, Ln, float(slope), _ptr(out), _stream())
        return out

    def pack_weight(self, w, up=1, device='cuda'):
        """torch Conv1d weight [Cout, Cin, K] (up = 1) or ConvTranspose1d weight [Cin, Cout, 2*up] -> packed weights on `device`."""
        w = np.ascontiguousarray(w.detach().cpu().float().numpy() if hasattr(w, 'detach') else w, dtype=np.float32)
        if up > 1:
            cin, cout, k = w.shape
        else:
            cout, cin, k = w.shape
        n = getattr(L.load(), f'ttsamd_{self.prefix}_weight_elems')(cout, cin, k, up)
        out = np.empty(n, dtype=np.uint16)
        self._call('pack_weight', w.ctypes.data_as(C.c_void_p), cout, cin, k, up, out.ctypes.data_as(C.c_void_p))
        return torch.from_numpy(out.view(np.int16)).to(device)

    def conv1d(self, x, wp, bias, cout, k, dilation=1, up=1, lens=None, len_mul=1, res=None, res_slope=1.0, sum_in=None, mode=0,
               div=1.0, out_slope=1.0, y=None, f32_out=False, res_f32=None):
        """f32_out: the result is an fp32 channel-first [B, cout, L] tensor (+ the fp32 channel-first residual res_f32)."""
        B, no, Ln, _ = x.shape
        if f32_out:
            yf = torch.zeros(B, cout, Ln, dtype=torch.float32, device=x.device) if y is None else y
            self._call('conv1d', _ptr(x), _ptr(wp), _ptr(bias), None, None, _ptr(lens), len_mul, B, no * 8, cout, k, dilation, up, Ln,
                       0, 1.0, 1.0, float(out_slope), None, _ptr(yf), _ptr(res_f32), _stream())
            return yf
        if y is None:
            y = torch.zeros(B, cout // 8, Ln * up, self.last, dtype=torch.int16, device=x.device)
        self._call('conv1d', _ptr(x), _ptr(wp), _ptr(bias), _ptr(res), _ptr(sum_in), _ptr(lens), len_mul, B, no * 8, cout, k, dilation,
                   up, Ln, mode, float(div), float(res_slope), float(out_slope), _ptr(y), None, None, _stream())
        return y

    def resblock_pair(self, x, w1p, b1, w2p, b2, k, dilation, lens=None, len_mul=1, sum_in=None, mode=0, div=1.0, in_slope=0.1,
                      mid_slope=0.1, out_slope=0.1, y=None):
        B, no, Ln, _ = x.shape
        if y is None:
            y = torch.zeros_like(x)
        self._call('resblock_pair', _ptr(x), _ptr(w1p), _ptr(b1), _ptr(w2p), _ptr(b2), _ptr(sum_in), _ptr(lens), len_mul, B, no * 8, k,
                   dilation, Ln, mode, float(div), float(in_slope), float(mid_slope), float(out_slope), _ptr(y), _stream())
        return y

    def _chain(self, x, w1p, b1, w2p, b2, dilations, lens, len_mul, sum_in, mode, div, in_slope, mid_slope, out_slope, y, *k):
        """*k: the trailing kernel-size argument of ttsamd_bfo_resblock_chain; the x3 entry has none (k = 3)."""
        B, no, Ln, _ = x.shape
        if y is None:
            y = torch.zeros_like(x)
        arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
        dl = (C.c_int32 * 3)(*[int(d) for d in dilations])
        self._call('resblock_chain', _ptr(x), arr(w1p), arr(b1), arr(w2p), arr(b2), dl, _ptr(sum_in), _ptr(lens), len_mul, B, no * 8, Ln,
                   mode, float(div), float(in_slope), float(mid_slope), float(out_slope), _ptr(y), _stream(), *k)
        return y

    def conv_post(self, x, w, bias, lens=None, len_mul=1):
        B, no, Ln, _ = x.shape
        wave = torch.zeros(B, Ln, dtype=torch.float32, device=x.device)
        self._call('conv_post', _ptr(x), _ptr(w), _ptr(bias), _ptr(lens), len_mul, B, no * 8, Ln, _ptr(wave), Ln, _stream())
        return wave


_BF16, _X3 = _Mode('bfo', 8), _Mode('bfo3', 16)

pack, unpack, pack_weight, conv1d = _BF16.pack, _BF16.unpack, _BF16.pack_weight, _BF16.conv1d
resblock_pair, conv_post = _BF16.resblock_pair, _BF16.conv_post
pack3, unpack3, pack_weight3, conv1d3 = _X3.pack, _X3.unpack, _X3.pack_weight, _X3.conv1d
resblock_pair3, conv_post3 = _X3.resblock_pair, _X3.conv_post


def resblock_chain(x, w1p, b1, w2p, b2, dilations, lens=None, len_mul=1, sum_in=None, mode=0, div=1.0, in_slope=0.1, mid_slope=0.1,
                   out_slope=0.1, y=None, k=3):
    """A whole ResBlock (three pairs) in one launch, k = 3 or (C <= 64) k = 7; w1p / b1 / w2p / b2: lists of three device tensors."""
    return _BF16._chain(x, w1p, b1, w2p, b2, dilations, lens, len_mul, sum_in, mode, div, in_slope, mid_slope, out_slope, y, int(k))


def resblock_chain3(x, w1p, b1, w2p, b2, dilations, lens=None, len_mul=1, sum_in=None, mode=0, div=1.0, in_slope=0.1, mid_slope=0.1,
                    out_slope=0.1, y=None):
    """A whole k = 3 ResBlock (three pairs) in one launch of the split-bf16 engine; w1p / b1 / w2p / b2: lists of three device tensors."""
    return _X3._chain(x, w1p, b1, w2p, b2, dilations, lens, len_mul, sum_in, mode, div, in_slope, mid_slope, out_slope, y)

"""Drop-in for the reference's utils/oversmoothing.py: the cepstral-domain oversmoothing measures of a mel-spectrogram (HQER, CSlope,
CCentroid, CRoll95: an rFFT across the mel bands of every frame) and their DTW-aligned comparison between a prediction and a ground
truth, with the reference's names, signatures and defaults.  All arithmetic runs in libttsamd.so (csrc/oversmooth.hip) through
ttsamd.engine; there is no CPU fallback: without a gfx950 device every call raises ttsamd.lib.TtsAmdError.

Conventions: numpy arrays in give numpy arrays and floats out, as in the reference; tensors in give tensors on the device out.  A batch is
this project's addition: one more leading dimension ([B, n_mels, T] mels, [B, T] series) plus `lens` (int64 [B], None = full rows);
batched results carry the leading dimension, frames past a row's length are zero.  DTW is all-fp32 and bit-reproducible
(include/ttsamd.h: ttsamd_dtw); at most ttsamd.engine.OVERSMOOTH_MAX_FRAMES frames per side."""
import numpy as np
import torch

from ttsamd import engine as E
from ttsamd.lib import TtsAmdError

KEYS = E.OVERSMOOTH_KEYS


# ---- plumbing: numpy / tensor in, the same kind out ------------------------------------------------------------------------------------
def _prep(x, nd, what):
    """-> (float32 device tensor with a leading batch dimension, came as numpy, came batched)"""
    E._require_gpu()
    was_np = not isinstance(x, torch.Tensor)
    t = torch.as_tensor(np.asarray(x)) if was_np else x
    if t.dim() not in (nd, nd + 1):
        raise TtsAmdError(f'{what}: expected {nd} dimensions (or {nd + 1} with a batch), got shape {tuple(t.shape)}')
    batched = t.dim() == nd + 1
    t = t.to(device='cuda:0' if t.device.type != 'cuda' else t.device, dtype=torch.float32)
    return (t if batched else t[None]).contiguous(), was_np, batched


def _lens(lens, t, batched):
    if lens is not None and not batched:
        raise TtsAmdError('lens goes with a batched input')
    return E._dev_lens(lens, t.shape[0], t.shape[-1], t.device)


def _out(t, was_np, batched, dtype=None):
    t = t if batched else t[0]
    if not was_np:
        return t if dtype is None else t.to(dtype)
    a = t.cpu().numpy()
    if dtype is not None:
        a = a.astype({torch.int64: np.int64}[dtype])
    return a if a.ndim else a.item()


def _reduced(series, lens, k, reduction, was_np, batched, dtype=None):
    """series [B, 4, T]: key k as the reference's _reduce_series gives it ('none': the series, else the mean / median of its finite values)"""
    if reduction not in ('mean', 'median'):
        return _out(series[:, k], was_np, batched, dtype)
    stats, _ = E.series_summary(series[:, k:k + 1].contiguous(), lens)
    return _out(stats[:, 0, 1 if reduction == 'mean' else 2], was_np, batched)


def _from_power(P_qT, lens, k, reduction, dtype=None, **kw):
    P, was_np, batched = _prep(P_qT, 2, 'power')
    lens = _lens(lens, P, batched)
    return _reduced(E.cepstral_series_from_power(P, lens, **kw), lens, k, reduction, was_np, batched, dtype)


# ---- the four measures ---------------------------------------------------------------------------------------------------------------
def framewise_rfft_power(mel_BxT, center=True, hann=True, lens=None):
    """mel [n_mels, T] -> P [Q, T], Q = n_mels // 2 + 1: |rFFT across the bands|^2 per frame, the frame's mean over the bands removed
    (`center`) and np.hanning(n_mels) applied (`hann`) first."""
    mel, was_np, batched = _prep(mel_BxT, 2, 'framewise_rfft_power')
    _, P = E.cepstral_series(mel, _lens(lens, mel, batched), center, hann, return_power=True)
    return _out(P, was_np, batched)


def hqer_from_power(P_qT, q_c=None, reduction='none', lens=None):
    """High-quefrency energy ratio: sum P[q_c:] / (sum P[1:] + 1e-12) per frame; q_c defaults to clamp(floor(0.25 Q), 1, Q - 1)."""
    return _from_power(P_qT, lens, 0, reduction, q_c=q_c)


def slope_from_power(P_qT, q1=1, q2=None, eps=1e-8, reduction='none', lens=None):
    """Least-squares slope of 10 log10(P + eps) over q = q1 .. q2 (default Q - 1) per frame; NaN for fewer than two points."""
    E._require_gpu()
    Q = P_qT.shape[-2]
    if (Q - 1 if q2 is None else q2) - q1 + 1 < 2:
        return float('nan')
    return _from_power(P_qT, lens, 1, reduction, q1=q1, q2=q2, eps=eps)


def centroid_from_power(P_qT, reduction='none', lens=None):
    """Energy-weighted mean quefrency over q >= 1 per frame."""
    return _from_power(P_qT, lens, 2, reduction)


def rolloff_from_power(P_qT, p=0.95, reduction='none', lens=None):
    """First q whose cumulative power from q = 1 reaches p (total + 1e-12) per frame, 1 if none does (an integer series)."""
    return _from_power(P_qT, lens, 3, reduction, dtype=torch.int64, roll_p=p)


def compute_mel_oversmoothing_metrics(mel, center=True, hann=True, q_c=None, reduction='none', lens=None):
    """mel [n_mels, T] -> {HQER (x 100), CSlope, CCentroid, CRoll95, Q}: per-frame series, or their mean / median over the finite frames."""
    m, was_np, batched = _prep(mel, 2, 'compute_mel_oversmoothing_metrics')
    lens = _lens(lens, m, batched)
    series = E.cepstral_series(m, lens, center, hann, q_c)
    out = {name: _reduced(series, lens, k, reduction, was_np, batched, torch.int64 if name == 'CRoll95' else None)
           for k, name in enumerate(KEYS)}
    out['Q'] = int(m.shape[1] // 2 + 1)
    return out


# ---- alignment -----------------------------------------------------------------------------------------------------------------------
def _align(A, B, lens_a, lens_b, metric, window, return_aligned, was_np, batched):
    """A [B, M, Ta], B [B, M, Tb] on the device -> the reference's tuple"""
    cost, path, plen = E.dtw(A, B, lens_a, lens_b, 'l2' if str(metric).lower() == 'l2' else 'cosine', window)
    if batched:
        res = (cost, path, plen)
        if return_aligned:
            M = A.shape[1]
            res += tuple(torch.gather(X.transpose(1, 2), 1, path[:, :, c].long()[:, :, None].expand(-1, -1, M)) for c, X in ((0, A), (1, B)))
        return tuple(r.cpu().numpy() for r in res) if was_np else res
    L = int(plen[0])                                               # the one host read: the path's length sizes what is returned
    p = path[0, :L]
    res = (cost[0], p)
    if return_aligned:
        res += (A[0].t()[p[:, 0].long()], B[0].t()[p[:, 1].long()])
    if was_np:
        return (float(res[0]),) + tuple(r.cpu().numpy() for r in res[1:])
    return res


def dtw_align_mels(mel_a, mel_b, metric='cosine', window=None, return_aligned=True, lens_a=None, lens_b=None):
    """DTW of two mels [n_mels, T] (frame distance 'cosine' | 'l2', `window` = Sakoe-Chiba radius or None) -> (cost, path [L, 2]) and, with
    return_aligned, the two sequences sampled along the path ([L, n_mels] each).  A batch gives (cost [B], path [B, Ta + Tb, 2],
    path_len [B]) and the aligned sequences at full path length."""
    A, np_a, batched = _prep(mel_a, 2, 'dtw_align_mels: mel_a')
    B, np_b, batched_b = _prep(mel_b, 2, 'dtw_align_mels: mel_b')
    if batched != batched_b or A.shape[:2] != B.shape[:2]:
        raise TtsAmdError(f'dtw_align_mels: mel_a {tuple(mel_a.shape)} and mel_b {tuple(mel_b.shape)} differ in batch or band count')
    return _align(A, B.to(A.device), _lens(lens_a, A, batched), _lens(lens_b, B, batched), metric, window, return_aligned, np_a and np_b,
                  batched)


def aligned_mae_distance(series_pred, series_ref, lens_pred=None, lens_ref=None):
    """Mean |pred - ref| of two series [T] along the DTW path of their NaN-interpolated, z-scored copies (L2, no band)."""
    a, np_a, batched = _prep(series_pred, 1, 'aligned_mae_distance: series_pred')
    b, np_b, batched_b = _prep(series_ref, 1, 'aligned_mae_distance: series_ref')
    if batched != batched_b or a.shape[0] != b.shape[0]:
        raise TtsAmdError('aligned_mae_distance: the two series differ in batch')
    b = b.to(a.device)
    la, lb = _lens(lens_pred, a, batched), _lens(lens_ref, b, batched)
    _, fa = E.series_summary(a[:, None], la)
    _, fb = E.series_summary(b[:, None], lb)
    _, path, plen = E.dtw(fa, fb, la, lb)
    return _out(E.dtw_aligned_mae(a, b, path, plen), np_a and np_b, batched)


def oversmoothing_metrics_aligned(mel_spec_pred, mel_spec_ref, center=True, hann=True, lens_pred=None, lens_ref=None):
    """{mae_<k>, delta_u_<k>} for the four measures: the frame-wise error after DTW alignment and the difference of the medians between a
    predicted and a reference mel [n_mels, T] (ttsamd.engine.oversmoothing_score: nothing is read back before the final dict)."""
    p, np_p, batched = _prep(mel_spec_pred, 2, 'oversmoothing_metrics_aligned: mel_spec_pred')
    r, np_r, batched_r = _prep(mel_spec_ref, 2, 'oversmoothing_metrics_aligned: mel_spec_ref')
    if batched != batched_r:
        raise TtsAmdError('oversmoothing_metrics_aligned: one mel is batched, the other is not')
    _, _, score = E.oversmoothing_score(p, _lens(lens_pred, p, batched), r.to(p.device), _lens(lens_ref, r, batched), center, hann)
    out = {}
    for k in KEYS:                                                 # the reference's order: mae, delta_u per key
        for name in (f'mae_{k}', f'delta_u_{k}'):
            out[name] = _out(score[name], np_p and np_r, batched)
    return out

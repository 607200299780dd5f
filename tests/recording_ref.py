"""Shared by tests/test_recording_cpu.py and tests/test_gpu_recording.py (not a test module): float64 restatements of the recording
preparation -- the polyphase sinc resampler (torchaudio's 'sinc_interp_hann' arithmetic), librosa.effects.trim with ref = max, the
reference's remove_silence -- and the test signals."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from melspec_ref import voiced

# (orig, new, lowpass_filter_width) -> (o, n, J): the rate pairs every resampler test walks
RATE_CASES = {
    (48000, 22050, 1024): (320, 147, 4824),
    (48000, 22050, 64): (320, 147, 602),
    (44100, 22050, 64): (2, 1, 262),
    (16000, 22050, 64): (320, 441, 450),
    (22050, 24000, 6): (147, 160, 161),
    (8000, 22050, 16): (160, 441, 194),
}


def taps_ref(orig, new, lfw=6, rolloff=0.99):
    """-> (taps float32 [n, J], width, o, n), phase by phase in float64, rounded once."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = int(math.ceil(lfw * o / base))
    J = 2 * width + o
    taps = np.empty((n, J), dtype=np.float32)
    j = np.arange(J, dtype=np.float64)
    for p in range(n):
        t = np.clip(((j - width) / o - p / n) * base, -lfw, lfw)
        win = np.cos(t * np.pi / lfw / 2) ** 2
        tp = t * np.pi
        safe = np.where(tp == 0.0, 1.0, tp)
        taps[p] = (np.where(tp == 0.0, 1.0, np.sin(safe) / safe) * win * (base / o)).astype(np.float32)
    return taps, width, o, n


def out_len(L, o, n):
    return (n * L + o - 1) // o if L > 0 else 0


def resample_ref(x, orig, new, lfw=6, rolloff=0.99, dtype=torch.float64, taps=None):
    """One row [L] -> [ceil(n L / o)] in `dtype`: F.conv1d at stride o over the zero-padded row, phases interleaved, truncated."""
    tp, width, o, n = taps if taps is not None else taps_ref(orig, new, lfw, rolloff)
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    L = x.numel()
    xp = F.pad(x[None, None], (width, width + o))
    y = F.conv1d(xp, torch.from_numpy(np.asarray(tp)).to(dtype)[:, None], stride=o)      # [1, n, frames]
    return y[0].t().reshape(-1)[:out_len(L, o, n)]


def resample_direct(x, orig, new, lfw=6, rolloff=0.99, taps=None):
    """The same sum, sample by sample, as a plain loop in Python floats (= float64)."""
    tp, width, o, n = taps if taps is not None else taps_ref(orig, new, lfw, rolloff)
    x = [float(v) for v in np.asarray(x)]
    L, J = len(x), tp.shape[1]
    rows = [[float(v) for v in tp[p]] for p in range(n)]
    out = []
    for m in range(out_len(L, o, n)):
        f, p = divmod(m, n)
        acc, row = 0.0, rows[p]
        lo, hi = max(0, width - f * o), min(J, L + width - f * o)
        for j in range(lo, hi):
            acc += row[j] * x[f * o + j - width]
        out.append(acc)
    return np.array(out)


def frame_power(x, frame_length, hop):
    """Mean of the squares of the T = 1 + L // hop centred frames (zero padding of frame_length // 2 per side), float64."""
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    T = 1 + L // hop
    xp = np.concatenate([np.zeros(frame_length // 2), x, np.zeros(frame_length + hop)])
    c = np.concatenate([[0.0], np.cumsum(xp * xp)])
    s = np.arange(T) * hop
    return (c[s + frame_length] - c[s]) / frame_length


def trim_ref(x, top_db=60, frame_length=2048, hop=512):
    """-> ((start, end), margin): librosa.effects.trim's bounds by its arithmetic, and the smallest distance in dB of any frame from the
    threshold."""
    L = int(np.asarray(x).size)
    r2 = np.maximum(np.sqrt(frame_power(x, frame_length, hop)), 1e-5) ** 2
    db = 10.0 * np.log10(r2 / r2.max())
    loud = np.nonzero(db > -top_db)[0]
    margin = float(np.abs(db + top_db).min())
    if loud.size == 0:
        return (0, 0), margin
    return (int(loud[0]) * hop, min(L, (int(loud[-1]) + 1) * hop)), margin


def remove_silence_ref(e, thresh=-10.0):
    """Bool mask: frames above the threshold, everything behind the last of them; none above: all but frame 0."""
    e = np.asarray(e)
    keep = e > thresh
    idx = np.nonzero(keep)[0]
    keep[(idx[-1] + 1 if idx.size else 1):] = True
    return keep


def trim_rows():
    """The trim cases: noise of sigma 1e-3, a voiced stretch, noise; + an all-zero row and a row shorter than one hop.
    -> list of float32 arrays."""
    rng = np.random.default_rng(0)
    rows = []
    for i, (a, b, c) in enumerate([(3000, 5000, 2100), (0, 4097, 1500), (1234, 2560, 0), (700, 9001, 333)]):
        rows.append(np.concatenate([1e-3 * rng.standard_normal(a), voiced(b, 40 + i).astype(np.float64),
                                    1e-3 * rng.standard_normal(c)]).astype(np.float32))
    rows.append(np.zeros(3000, dtype=np.float32))
    rows.append(voiced(200, 44))
    return rows


TRIM_BOUNDS = [(2560, 8704), (0, 4608), (768, 3794), (256, 10034)]


def pack_rows(rows, width=None, poison=7.0):
    """Ragged rows -> (float32 [B, width] with `poison` behind each row's end, int64 lens)."""
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    W = int(width or lens.max() + 5)
    buf = np.full((len(rows), W), poison, dtype=np.float32)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = r
    return buf, lens

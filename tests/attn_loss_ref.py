"""NumPy float64 restatement of the alignment prior and the two alignment losses of the reference: beta_binomial_prior_distribution and
BetaBinomialInterpolator.__call__ (models/fastpitch/fastpitch/data_function.py:45-78), AttentionCTCLoss and AttentionBinarizationLoss
(attn_loss_function.py).  Our own text: the CPU tests check it against the golden file (tools/gen_golden_attn_loss.py wrote that with scipy
and the reference's loss module), the GPU tests use it for the shapes that are too big to commit."""
import functools
import math

import numpy as np


@functools.lru_cache(maxsize=None)
def _lf_cached(n):
    return np.array([math.lgamma(k + 1.0) for k in range(n)], np.float64)


def log_factorials(n):
    """lf[k] = log k! for k < n"""
    size = 1024
    while size < n:
        size *= 2
    return _lf_cached(size)[:n]


def betabinom_pmf(n, a, b, k):
    """betabinom(n, a, b).pmf(k) for integer arrays a, b >= 1 and 0 <= k < n (broadcast)"""
    n, a, b, k = np.broadcast_arrays(*(np.asarray(v, np.int64) for v in (n, a, b, k)))
    lf = log_factorials(int((n + a + b).max()) + 1)
    return np.exp((lf[n] - lf[k] - lf[n - k]) + (lf[k + a - 1] + lf[n - k + b - 1] - lf[n + a + b - 1]) - (lf[a - 1] + lf[b - 1] - lf[a + b - 1]))


def exact_prior(phoneme_count, mel_count):
    """beta_binomial_prior_distribution(P, M) -> [M, P]: row i - 1 is betabinom(n = P, a = i, b = M + 1 - i).pmf(0 .. P - 1)"""
    P, M = int(phoneme_count), int(mel_count)
    i = np.arange(1, M + 1)[:, None]
    return betabinom_pmf(P, i, M + 1 - i, np.arange(P)[None, :])


def round_to(val, to):
    """BetaBinomialInterpolator.round: halves go to the even multiple, as np.round takes them"""
    return max(1, int(np.round((val + 1) / to))) * to


def interpolated_prior(w, h):
    """BetaBinomialInterpolator()(w = mel length, h = text length) -> [w, h]: the exact prior of the rounded sizes (the rounded MEL length
    as the phoneme count, as the reference passes it) transposed, sampled as scipy.ndimage.zoom(order=1) does"""
    w, h = int(w), int(h)
    bw, bh = round_to(w, 100), round_to(h, 20)
    x = np.arange(w) * ((bw - 1) / (w - 1)) if w > 1 else np.zeros(w)
    y = np.arange(h) * ((bh - 1) / (h - 1)) if h > 1 else np.zeros(h)
    x0, y0 = np.minimum(np.floor(x).astype(np.int64), bw - 1), np.minimum(np.floor(y).astype(np.int64), bh - 1)
    x1, y1 = np.minimum(x0 + 1, bw - 1), np.minimum(y0 + 1, bh - 1)
    fx, fy = (x - x0)[:, None], (y - y0)[None, :]
    bank = lambda xi, yi: betabinom_pmf(bw, yi[None, :] + 1, bh - yi[None, :], xi[:, None])   # noqa: E731  (bank.T[x][y])
    return (1.0 - fx) * ((1.0 - fy) * bank(x0, y0) + fy * bank(x0, y1)) + fx * ((1.0 - fy) * bank(x1, y0) + fy * bank(x1, y1))


def batch_prior(in_lens, mel_lens, n_tokens, n_frames, mode):
    """[B, n_frames, n_tokens]: every row's corner, zero outside it"""
    out = np.zeros((len(in_lens), n_frames, n_tokens), np.float64)
    for b, (p, m) in enumerate(zip(in_lens, mel_lens)):
        p, m = min(int(p), n_tokens), min(int(m), n_frames)
        if p > 0 and m > 0:
            out[b, :m, :p] = exact_prior(p, m) if mode == 'exact' else interpolated_prior(m, p)
    return out


def _lse(*xs):
    m = np.maximum.reduce(xs)
    ms = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide='ignore'):
        return m + np.log(sum(np.exp(x - ms) for x in xs))


def forward_sum(logprob, n_in, n_out, blank_logprob=-1.0):
    """The CTC negative log-likelihood of the targets 0 .. n_in - 1 over the frames t < n_out, frame t's distribution being
    [blank_logprob, logprob[t, :n_in]] log-softmaxed; logprob [T, L].  +inf when no path exists, 0 without tokens."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in == 0:
        return 0.0
    if n_out < n_in:
        return np.inf
    x = np.concatenate([np.full((n_out, 1), float(blank_logprob)), np.asarray(logprob, np.float64)[:n_out, :n_in]], axis=1)
    m = x.max(axis=1, keepdims=True)
    x = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    tok, blk = np.full(n_in, -np.inf), np.full(n_in + 1, -np.inf)         # blk[l]: the blank before token l; blk[n_in] trails
    blk[0], tok[0] = x[0, 0], x[0, 1]
    neg = np.array([-np.inf])
    for t in range(1, n_out):
        left = np.concatenate([neg, tok[:-1]])
        tok_new = x[t, 1:] + _lse(tok, blk[:-1], left)
        blk = x[t, 0] + _lse(blk, np.concatenate([neg, tok]))
        tok = tok_new
    return float(-_lse(tok[-1:], blk[-1:])[0])


def batch_forward_sum(logprob, in_lens, out_lens, blank_logprob=-1.0):
    """logprob [B, T, L] or [B, 1, T, L] -> nll [B]"""
    logprob = np.asarray(logprob)
    logprob = logprob[:, 0] if logprob.ndim == 4 else logprob
    T, L = logprob.shape[1:]
    return np.array([forward_sum(logprob[b], min(int(in_lens[b]), L), min(int(out_lens[b]), T), blank_logprob) for b in range(len(logprob))])


def ctc_mean(nll, in_lens):
    """nn.CTCLoss(zero_infinity=True) with the default mean reduction: infinite rows count 0, every row is divided by its target length"""
    nll = np.asarray(nll, np.float64)
    return float((np.where(np.isinf(nll), 0.0, nll) / np.maximum(np.asarray(in_lens, np.float64), 1.0)).mean())


def binarization(hard, soft, eps=1e-12):
    """-> (sum_log [B], count [B]): the sum of log(max(soft, eps)) over the cells with hard == 1, and how many there are"""
    hard, soft = np.asarray(hard), np.asarray(soft, np.float64)
    B = hard.shape[0]
    on = hard.reshape(B, -1) == 1
    logs = np.where(on, np.log(np.maximum(soft.reshape(B, -1), eps)), 0.0)
    return np.array([math.fsum(r) for r in logs]), on.sum(axis=1).astype(np.float64)

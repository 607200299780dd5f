"""NumPy restatement of the aligner path of the reference's FastPitch.forward (models/fastpitch/fastpitch/model.py:298-318): ConvAttention.forward
(attention.py:174-223), mas_width1 (alignment.py:46-72) and average_pitch (model.py:93-111).  Our own text, used by the CPU tests to check the
golden file (tools/gen_golden_aligner.py wrote it with the reference's modules) and by the GPU tests as the float64 / fp32 yardstick.

Everything takes a dtype: float64 is the yardstick of the soft values; float32 MAS is the decision-for-decision yardstick of the hard path
(one max and one add per cell, both exact in IEEE arithmetic whatever the library, so NumPy's fp32 equals the reference's)."""
import numpy as np

KEY_CONVS = (('attention.key_proj.0.conv', True), ('attention.key_proj.2.conv', False))
QUERY_CONVS = (('attention.query_proj.0.conv', True), ('attention.query_proj.2.conv', True), ('attention.query_proj.4.conv', False))


def conv1d(x, w, b, dtype=np.float64):
    """x [B, Ci, S], w [Co, Ci, K] (K odd, 'same' zero padding), b [Co] -> [B, Co, S]"""
    x, w, b = x.astype(dtype), w.astype(dtype), b.astype(dtype)
    K, S = w.shape[2], x.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (K // 2, K // 2)))
    y = np.zeros((x.shape[0], w.shape[0], S), dtype)
    for k in range(K):
        y += np.einsum('oc,bcs->bos', w[:, :, k], xp[:, :, k:k + S])
    return y + b[None, :, None]


def _encode(sd, x, convs, dtype):
    for name, relu in convs:
        x = conv1d(x, sd[name + '.weight'], sd[name + '.bias'], dtype)
        if relu:
            x = np.maximum(x, 0)
    return x


def attention(sd, ids, mel, in_lens, prior=None, dtype=np.float64):
    """ConvAttention.forward on the padded batch: ids [B, L], mel [B, n_mel, T], prior [B, T, L] or None ->
    (attn_soft, attn_logprob), both [B, 1, T, L] in `dtype`.  Columns l >= in_lens[b] are masked after attn_logprob is taken."""
    keys = _encode(sd, sd['encoder.word_emb.weight'][ids].transpose(0, 2, 1), KEY_CONVS, dtype)        # [B, C, L]
    queries = _encode(sd, mel, QUERY_CONVS, dtype)                                                       # [B, C, T]
    d = queries[:, :, :, None] - keys[:, :, None, :]
    a = dtype(-0.0005) * (d * d).sum(axis=1)                                                             # [B, T, L]
    if prior is not None:
        m = a.max(axis=2, keepdims=True)
        a = (a - m) - np.log(np.exp(a - m).sum(axis=2, keepdims=True)) + np.log(prior.astype(dtype) + dtype(1e-8))
    logprob = a.copy()
    L = a.shape[2]
    masked = np.where(np.arange(L)[None, None, :] < np.asarray(in_lens)[:, None, None], a, -np.inf)
    m = masked.max(axis=2, keepdims=True)
    e = np.exp(masked - m)
    return (e / e.sum(axis=2, keepdims=True))[:, None], logprob[:, None]


def mas_forward(log_attn):
    """The table of mas_width1 in the dtype of `log_attn` [T, L]: log_p[0, 1:] = -inf, log_p[i, j] += max(log_p[i-1, j-1], log_p[i-1, j])."""
    log_p = np.array(log_attn, copy=True)
    neg = log_p.dtype.type(-np.inf)
    log_p[0, 1:] = neg
    for i in range(1, log_p.shape[0]):
        prev = log_p[i - 1]
        left = np.concatenate([[neg], prev[:-1]])
        log_p[i] = log_p[i] + np.where(prev > left, prev, left)
    return log_p


def mas_backtrack(log_p):
    """-> (opt [T, L] of 0 / 1 in log_p's dtype, the |log_p[i-1, j-1] - log_p[i-1, j]| met on the way; NaN where both are -inf).
    One token: every frame goes to token 0 (the reference indexes out of bounds there; the library defines it so)."""
    T, L = log_p.shape
    opt = np.zeros_like(log_p)
    margins = []
    j = L - 1
    for i in range(T - 1, 0, -1):
        opt[i, j] = 1
        if j == 0:
            continue
        a, b = log_p[i - 1, j - 1], log_p[i - 1, j]
        with np.errstate(invalid='ignore'):
            margins.append(abs(a - b))
        if a >= b:
            j -= 1
    opt[0, j] = 1
    return opt, np.array(margins, np.float64)


def mas_width1(log_attn):
    return mas_backtrack(mas_forward(log_attn))[0]


def b_mas(log_attn, in_lens, out_lens):
    """log_attn [B, 1, T, L] -> attn_hard of the same shape and dtype, zero outside each row's [:out_len, :in_len]"""
    out = np.zeros_like(log_attn)
    for b in range(log_attn.shape[0]):
        t, l = int(out_lens[b]), int(in_lens[b])
        if t > 0 and l > 0:
            out[b, 0, :t, :l] = mas_width1(log_attn[b, 0, :t, :l])
    return out


def average_pitch(pitch, durs):
    """pitch [B, F, T], durs [B, L] -> [B, F, L] float64: the mean of the non-zero values of each token's frames, 0 where there is none.
    Bounds as the reference takes them: the running fp32 sum of durs, truncated."""
    pitch = np.asarray(pitch, np.float64)
    B, F, T = pitch.shape
    ends = np.cumsum(np.asarray(durs, np.float32), axis=1, dtype=np.float32).astype(np.int64)
    out = np.zeros((B, F, ends.shape[1]), np.float64)
    for b in range(B):
        start = 0
        for l in range(ends.shape[1]):
            end = min(max(int(ends[b, l]), 0), T)
            start = min(start, end)
            seg = pitch[b, :, start:end]
            nz = (seg != 0).sum(axis=1)
            out[b, :, l] = np.where(nz > 0, seg.sum(axis=1) / np.maximum(nz, 1), 0.0)
            start = end
    return out

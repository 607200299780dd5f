"""numpy statement of ttsamd_token_spans (include/ttsamd.h): integer arithmetic, the products in Python ints, so nothing can wrap."""
import numpy as np

INT64_MAX = (1 << 63) - 1
MAX_RATIO = 1 << 20


def span_pos(p, hop, m):
    """m(p) = off + ceil((min(max(p hop, lo), hi) - lo) num / den) for one row's map m = (lo, hi, off, num, den)"""
    lo, hi, off, num, den = (int(v) for v in m)
    x = min(max(int(p) * int(hop), lo), hi)
    return off + -((-(x - lo) * num) // den)


def token_spans(reps, n_tokens=None, groups=None, n_groups=None, hop=256, maps=None):
    """reps [B, L] (+ n_tokens [B], groups [B, G, 2], n_groups [B], maps [B, 5]) -> (tok int64 [B, L, 2], grp int64 [B, G, 2] or None)"""
    reps = np.asarray(reps)
    B, L = reps.shape
    tok = np.zeros((B, L, 2), dtype=np.int64)
    G = 0 if groups is None else np.asarray(groups).shape[1]
    grp = np.zeros((B, G, 2), dtype=np.int64) if groups is not None else None
    for b in range(B):
        n = L if n_tokens is None else min(max(int(n_tokens[b]), 0), L)
        m = (0, INT64_MAX, 0, 1, 1) if maps is None else tuple(int(v) for v in maps[b])
        if not (1 <= m[3] <= MAX_RATIO and 1 <= m[4] <= MAX_RATIO) or m[1] < m[0]:
            tok[b] = -1
            if grp is not None:
                grp[b] = -1
            continue
        c = [0]
        for i in range(n):
            c.append(c[-1] + max(int(reps[b, i]), 0))
        pos = [span_pos(v, hop, m) for v in c]
        for i in range(L):
            tok[b, i] = (pos[min(i, n)], pos[min(i + 1, n)])
        if grp is None:
            continue
        ng = G if n_groups is None else min(max(int(n_groups[b]), 0), G)
        for g in range(G):
            t0 = t1 = n
            if g < ng:
                t0 = min(max(int(groups[b][g][0]), 0), n)
                t1 = max(min(max(int(groups[b][g][1]), 0), n), t0)
            grp[b, g] = (pos[t0], pos[t1])
    return tok, grp

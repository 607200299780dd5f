"""pYIN restated in numpy float64 from its arithmetic (steps 1-9 of the specification in DESIGN.md section 4), written from that text
and not from the kernel: the yardstick of tests/test_pyin_cpu.py and tests/test_gpu_pyin.py.  librosa is not needed.

`viterbi_dense` is the reference's dense recurrence (every one of the 2P x 2P transitions, out-of-band ones at log(tiny)) in a chosen
dtype; `viterbi_kernel_form` restates the device's own fp32 recurrence: 2 x w in-band candidates per state in state order plus ONE
candidate max_k value[k] + log(tiny), single fp32 additions, ties to the lowest index."""
import math

import numpy as np

TINY = np.finfo(np.float64).tiny


class Params:
    def __init__(self, fmin, fmax, sr=22050, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100,
                 beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01,
                 no_trough_prob=0.01, pad_mode='constant'):
        self.fmin, self.fmax, self.sr, self.N = float(fmin), float(fmax), int(sr), int(frame_length)
        self.W = self.N // 2 if win_length is None else int(win_length)
        self.hop = self.N // 4 if hop_length is None else int(hop_length)
        self.K, (self.a, self.b), self.lam = int(n_thresholds), beta_parameters, float(boltzmann_parameter)
        self.switch, self.ntp, self.pad_mode = float(switch_prob), float(no_trough_prob), pad_mode
        self.pmin = max(int(math.floor(self.sr / self.fmax)), 1)
        self.pmax = min(int(math.ceil(self.sr / self.fmin)), self.N - self.W - 1)
        self.nb = int(math.ceil(1.0 / resolution))
        self.P = int(math.floor(12 * self.nb * np.log2(self.fmax / self.fmin))) + 1
        self.w = int(round(max_transition_rate * 12 * self.hop / self.sr)) * self.nb + 1


def beta_cdf(a, b, x):
    n = a + b - 1
    return sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1))


def beta_weights(p):
    cdf = np.array([beta_cdf(p.a, p.b, k / p.K) for k in range(p.K + 1)])
    return np.diff(cdf)


def boltzmann_prior(lam, pos, n):
    return (1.0 - math.exp(-lam)) * np.exp(-lam * np.asarray(pos, dtype=np.float64)) / (1.0 - math.exp(-lam * n))


def frames_of(y, p):
    y = np.asarray(y, dtype=np.float32)
    pad = p.N // 2
    if p.pad_mode == 'reflect':
        yp = np.pad(y, pad, mode='reflect')
    else:
        yp = np.pad(y, pad, mode='constant')
    T = 1 + len(y) // p.hop
    return np.stack([yp[t * p.hop: t * p.hop + p.N] for t in range(T)]).astype(np.float64)


def normalised_difference(frame, p):
    """d'(tau) for tau = pmin..pmax.  The sum over j runs along axis 0 of a [W][pmax] array: numpy adds the rows one after the other, a
    sequential float64 sum per lag."""
    x = frame
    taus = np.arange(1, p.pmax + 1)
    diff = x[:p.W, None] - x[np.arange(p.W)[:, None] + taus[None, :]]
    d = np.add.reduce(diff * diff, axis=0)
    dn = d / (np.cumsum(d) / taus + TINY)
    return dn[p.pmin - 1:]


def frame_observation(frame, p, beta):
    """-> (obs [P] probabilities of the voiced bins, voiced_prob, debug dict)"""
    dn = normalised_difference(frame, p)
    L = len(dn)
    tr = np.zeros(L, dtype=bool)
    tr[1:-1] = (dn[1:-1] < dn[:-2]) & (dn[1:-1] <= dn[2:])
    tr[0] = dn[0] < dn[1]
    tr[-1] = dn[-1] < dn[-2]
    idx = np.flatnonzero(tr)
    obs = np.zeros(p.P)
    if len(idx) == 0:
        return obs, 0.0, {'heights': np.zeros(0), 'index': idx}
    shift = np.zeros(len(idx))
    for n, i in enumerate(idx):
        if 0 < i < L - 1:
            a = dn[i + 1] + dn[i - 1] - 2 * dn[i]
            b = (dn[i + 1] - dn[i - 1]) / 2
            if abs(b) < abs(a):
                shift[n] = -b / a
    h = dn[idx]
    prob = np.zeros(len(idx))
    lowest = int(np.argmin(h))
    for k in range(p.K):
        theta = (k + 1) / p.K
        under = h < theta
        nk = int(under.sum())
        if nk:
            prob[under] += boltzmann_prior(p.lam, np.arange(nk), nk) * beta[k]
        if not under[lowest]:
            prob[lowest] += p.ntp * beta[k]
    f = p.sr / (p.pmin + idx + shift)
    bins = np.clip(np.round(12 * p.nb * np.log2(f / p.fmin)), 0, p.P).astype(int)
    for n in range(len(idx)):                                   # lag order: the larger lag is assigned last and wins
        if bins[n] < p.P:
            obs[bins[n]] = prob[n]
    return obs, float(np.clip(obs.sum(), 0.0, 1.0)), {'heights': h, 'index': idx, 'bins': bins, 'prob': prob}


def observations(y, p):
    """-> obs [T][2P] probabilities, voiced_prob [T]"""
    beta = beta_weights(p)
    fr = frames_of(y, p)
    obs = np.zeros((len(fr), 2 * p.P))
    vp = np.zeros(len(fr))
    for t, f in enumerate(fr):
        o, v, _ = frame_observation(f, p, beta)
        obs[t, :p.P] = o
        obs[t, p.P:] = (1.0 - v) / p.P
        vp[t] = v
    return obs, vp


def triangle(w):
    h = w // 2
    return np.array([(h + 1 - abs(d - h)) / (h + 1) for d in range(w)])


def transition_local(p):
    tri, h = triangle(p.w), p.w // 2
    B = np.zeros((p.P, p.P))
    for k in range(p.P):
        lo, hi = max(0, k - h), min(p.P - 1, k + h)
        B[k, lo:hi + 1] = tri[lo - k + h: hi - k + h + 1]
        B[k] /= B[k].sum()
    return B


def transition(p):
    S = np.array([[1 - p.switch, p.switch], [p.switch, 1 - p.switch]])
    return np.kron(S, transition_local(p))


def viterbi_dense(logobs, logtrans, loginit, dtype=np.float64):
    lo, lt = logobs.astype(dtype), logtrans.astype(dtype)
    T, S = lo.shape
    value = lo[0] + loginit.astype(dtype)
    ptr = np.zeros((T, S), dtype=np.int64)
    for t in range(1, T):
        cand = value[:, None] + lt                              # [source][destination]
        ptr[t] = np.argmax(cand, axis=0)                        # the lowest source attaining the max
        value = lo[t] + cand[ptr[t], np.arange(S)]
    states = np.zeros(T, dtype=np.int64)
    states[-1] = int(np.argmax(value))
    for t in range(T - 1, 0, -1):
        states[t - 1] = ptr[t, states[t]]
    return states


def band_tables(p):
    """-> (src [2P][2w] source state of each in-band candidate in state order, -1 where cut off; lt32 [2P][2w] its fp32 log transition)"""
    lt = np.log(transition(p) + TINY).astype(np.float32)
    h, P = p.w // 2, p.P
    src = -np.ones((2 * P, 2 * p.w), dtype=np.int64)
    val = np.zeros((2 * P, 2 * p.w), dtype=np.float32)
    for b in range(2):
        for j in range(P):
            ks = np.arange(max(0, j - h), min(P - 1, j + h) + 1)
            for a in range(2):
                src[b * P + j, a * p.w: a * p.w + len(ks)] = a * P + ks
                val[b * P + j, a * p.w: a * p.w + len(ks)] = lt[a * P + ks, b * P + j]
    return src, val


def viterbi_kernel_form(logobs32, p, tables=None):
    """The device recurrence: logobs32 fp32 [T][2P].  -> states [T]"""
    src, val = tables if tables is not None else band_tables(p)
    T, S = logobs32.shape
    LT = np.float32(np.log(TINY))
    linit = np.float32(np.log(1.0 / S + TINY))
    value = (logobs32[0] + linit).astype(np.float32)
    ptr = np.zeros((T, S), dtype=np.int64)
    ok = src >= 0
    big = np.iinfo(np.int64).max
    for t in range(1, T):
        cand = np.where(ok, value[np.where(ok, src, 0)] + val, np.float32(-np.inf)).astype(np.float32)
        g = int(np.argmax(value))                               # lowest index of the global max
        cg = np.float32(value[g] + LT)
        best = cand.max(axis=1)
        # lowest source index among the in-band candidates attaining the max (they are listed in ascending state order)
        arg = np.where(ok & (cand == best[:, None]), src, big).min(axis=1)
        take = (cg > best) | ((cg == best) & (g < arg))
        best = np.where(take, cg, best).astype(np.float32)
        arg = np.where(take, g, arg)
        ptr[t] = arg
        value = (logobs32[t] + best).astype(np.float32)
    states = np.zeros(T, dtype=np.int64)
    states[-1] = int(np.argmax(value))
    for t in range(T - 1, 0, -1):
        states[t - 1] = ptr[t, states[t]]
    return states


def decode(states, p, fill_na=np.nan):
    f0 = p.fmin * 2.0 ** ((states % p.P) / (12.0 * p.nb))
    flag = states < p.P
    if fill_na is not None:
        f0 = np.where(flag, f0, fill_na)
    return f0, flag


def pyin(y, p, dtype=np.float64, fill_na=np.nan):
    """-> (f0, voiced_flag, voiced_prob, states) with the dense Viterbi in `dtype`"""
    obs, vp = observations(y, p)
    S = 2 * p.P
    states = viterbi_dense(np.log(obs + TINY), np.log(transition(p) + TINY), np.log(np.full(S, 1.0 / S) + TINY), dtype)
    f0, flag = decode(states, p, fill_na)
    return f0, flag, vp, states


# ---- signals ---------------------------------------------------------------------------------------------------------------------------
def harmonic_tone(f0, n, sr=22050, noise=0.0, seed=0):
    t = np.arange(n) / sr
    y = sum(a * np.sin(2 * np.pi * f0 * (i + 1) * t) for i, a in enumerate((1.0, 0.5, 0.3, 0.2)))
    y = 0.3 * y
    if noise:
        y = y + np.random.default_rng(seed).normal(0, noise, n)
    return y.astype(np.float32)


def speech_like(seed, n_frames, hop=256, sr=22050, noise=0.0):
    """Piecewise f0 glides 80-400 Hz with +-25 % drift, in voiced / silent / noisy segments."""
    rng = np.random.default_rng(seed)
    n = n_frames * hop - 1 - int(rng.integers(0, hop - 1))
    n = max(n, (n_frames - 1) * hop)
    y = np.zeros(n)
    pos, phase = 0, 0.0
    while pos < n:
        seg = int(rng.integers(8, 30)) * hop
        end = min(n, pos + seg)
        kind = rng.choice(3, p=[0.6, 0.2, 0.2])
        m = end - pos
        if kind == 0:
            f_a = rng.uniform(80, 400)
            f_b = float(np.clip(f_a * rng.uniform(0.75, 1.25), 80, 400))
            f = np.linspace(f_a, f_b, m)
            ph = phase + 2 * np.pi * np.cumsum(f) / sr
            y[pos:end] = 0.3 * sum(a * np.sin((i + 1) * ph) for i, a in enumerate((1.0, 0.5, 0.3, 0.2)))
            phase = ph[-1] % (2 * np.pi)
        elif kind == 2:
            y[pos:end] = rng.normal(0, 0.05, m)
        pos = end
    if noise:
        y = y + rng.normal(0, noise, n)
    return y.astype(np.float32)


def cents(f, f_true):
    return 1200.0 * np.abs(np.log2(np.asarray(f, dtype=np.float64) / f_true))

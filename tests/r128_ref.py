"""float64 restatement of the loudness meter (include/ttsamd.h, "loudness meter"): step energies, momentary and short-term loudness,
their maxima and the loudness range of EBU Tech 3342 on a hop of one step, on top of tests/loudness_ref.py (K-weighting, blocks,
gates); and a chunked meter that filters sequentially with carried lfilter state, so that "a stream measures what the whole wave
measures" is a CPU fact."""
import numpy as np
from scipy.signal import lfilter

import loudness_ref as R

ST_STEPS = 30                               # a short-term window: 30 steps of 100 ms


def _lu(e):
    with np.errstate(divide='ignore'):
        return -0.691 + 10.0 * np.log10(np.asarray(e, dtype=np.float64))


def percentile_indices(k):
    """(low, high): the indices of the 10th and 95th percentile among k sorted survivors, round((k - 1) p) in integers"""
    return ((k - 1) * 10 + 50) // 100, ((k - 1) * 95 + 50) // 100


def step_energies(y, fs):
    """u[i] = the sum of y^2 over step i, for the n // step whole steps"""
    step, _ = R.step_block(fs)
    y2 = np.asarray(y, dtype=np.float64) ** 2
    return np.array([y2[i * step:(i + 1) * step].sum() for i in range(len(y2) // step)])


def windows(u, fs, z_short=None):
    """u (+ the one block energy of a short row) -> dict(z, M, s, S, max_momentary, max_short_term, lra, gamma_s, k): the series and
    what is taken from them"""
    step, block = R.step_block(fs)
    u = np.asarray(u, dtype=np.float64)
    U = len(u)
    if z_short is not None:
        z = np.array([z_short])
    else:
        z = np.array([u[j:j + 4].sum() / block for j in range(max(U - 3, 0))])
    s = np.array([u[j:j + ST_STEPS].sum() / (ST_STEPS * step) for j in range(max(U - ST_STEPS + 1, 0))])
    M, S = _lu(z), _lu(s)
    out = dict(z=z, M=M, s=s, S=S, max_momentary=M.max() if len(M) else -np.inf, max_short_term=S.max() if len(S) else -np.inf,
               lra=0.0, gamma_s=-np.inf, k=0)
    a = S > -70.0
    if a.any():
        gamma = float(_lu(s[a].mean())) - 20.0
        v = np.sort(S[a & (S > gamma)])
        out.update(gamma_s=gamma, k=len(v))
        if len(v):
            lo, hi = percentile_indices(len(v))
            out['lra'] = float(v[hi] - v[lo])
    return out


def meter(x, fs):
    """the whole-wave meter of one row x (float32 samples): loudness_ref.measure's dict (L, gamma, l, z, peak) plus windows()'s"""
    x = np.asarray(x, dtype=np.float32)
    m = R.measure(x, fs)
    _, block = R.step_block(fs)
    y = R.kweight(x, fs)
    w = windows(step_energies(y, fs), fs, z_short=m['z'][0] if 0 < len(x) < block else None)
    if len(x) >= block:
        assert np.allclose(w['z'], m['z'], rtol=1e-12, atol=0)      # the momentary blocks are the gating blocks
    w.pop('z')
    m.update(w)
    return m


def lra_margin(m):
    """smallest distance in LU of any finite short-term value of meter()'s result from -70 and from the range's relative gate (inf
    when there is none)"""
    S = m['S'][np.isfinite(m['S'])]
    if not len(S):
        return np.inf
    d = np.abs(S + 70.0).min()
    if np.isfinite(m['gamma_s']):
        d = min(d, np.abs(S - m['gamma_s']).min())
    return float(d)


class ChunkedMeter:
    """The stream meter: samples arrive in chunks of any length, the two biquads run sequentially with carried lfilter state, whole
    steps are closed as they fill.  reading(): what a push reports; result(): what the whole-wave meter reports on the samples so far."""

    def __init__(self, fs):
        self.fs = fs
        self.c = R.coefficients(fs)
        self.step, self.block = R.step_block(fs)
        self.z1, self.z2 = np.zeros(2), np.zeros(2)
        self.y2 = np.zeros(0)                       # y^2 of the unfinished step
        self.u = []
        self.n = 0
        self.peak = np.float32(0)

    def push(self, x):
        x = np.asarray(x, dtype=np.float32)
        if len(x):
            b1, a1, b2, a2 = self.c
            y, self.z1 = lfilter(b1, a1, x.astype(np.float64), zi=self.z1)
            y, self.z2 = lfilter(b2, a2, y, zi=self.z2)
            self.y2 = np.concatenate([self.y2, y * y])
            self.n += len(x)
            self.peak = max(self.peak, np.float32(np.abs(x).max()))
            while len(self.y2) >= self.step:
                self.u.append(self.y2[:self.step].sum())
                self.y2 = self.y2[self.step:]
        return self.reading()

    def reading(self):
        """dict(momentary, short_term, integrated): the latest M and S (-inf before the first) and both gates over the blocks so far"""
        w = windows(self.u, self.fs)
        return dict(momentary=w['M'][-1] if len(w['M']) else -np.inf, short_term=w['S'][-1] if len(w['S']) else -np.inf,
                    integrated=R.gate(w['z'])['L'] if len(w['z']) else -np.inf)

    def result(self):
        short = (sum(self.u) + self.y2.sum()) / self.n if 0 < self.n < self.block else None
        w = windows(self.u, self.fs, z_short=short)
        w.update(R.gate(w['z']) if len(w['z']) else dict(L=-np.inf, gamma=-np.inf, l=np.zeros(0)))
        w['peak'] = self.peak
        return w


def chunked(x, fs, chunk):
    """the ChunkedMeter after x in chunks of `chunk` samples (or of the lengths of a list)"""
    m = ChunkedMeter(fs)
    x = np.asarray(x, dtype=np.float32)
    sizes = chunk if isinstance(chunk, (list, tuple)) else [chunk] * (-(-len(x) // chunk))
    pos = 0
    for c in sizes:
        m.push(x[pos:pos + c])
        pos += c
    assert pos >= len(x)
    return m


# ---- the rows of the GPU tests ----
def program_row():
    """19 s of noise at 22 050 Hz in five parts: 4 s at sigma 0.1, 3 s at 0.03, 4 s at 0.0002, 4 s of zeros, 4 s at 0.06"""
    rng = np.random.default_rng(7)
    parts = [(4, 0.1), (3, 0.03), (4, 0.0002), (4, 0.0), (4, 0.06)]
    return np.concatenate([(rng.standard_normal(d * 22050) * sg).astype(np.float32) for d, sg in parts])


EDGE_LENGTHS = [0, 3000, 8820, 8821, 66149, 66150, 68355]


def edge_row(n):
    return (np.random.default_rng(7).standard_normal(n) * 0.1).astype(np.float32)


def long_row(fs=8000, seconds=113):
    """noise under the envelope 0.02 * 10^(0.6 sin(2 pi t / 37) + 0.3 sin(2 pi t / 5.3))"""
    t = np.arange(seconds * fs) / fs
    env = 0.02 * 10.0 ** (0.6 * np.sin(2 * np.pi * t / 37.0) + 0.3 * np.sin(2 * np.pi * t / 5.3))
    return (np.random.default_rng(7).standard_normal(len(t)) * env).astype(np.float32)


def binding_row():
    """4 s of noise at sigma 0.1, then 20 s at 0.03 (the issue's 0.003 falls under the relative gate, so L stays at the opening's level and
    the cap does not bind; at 0.03 the quiet part counts and L lies 6 LU under the maximum short-term loudness): a loud opening in a
    quieter programme, where the short-term cap of R 128 s1 binds"""
    rng = np.random.default_rng(7)
    return np.concatenate([(rng.standard_normal(4 * 22050) * 0.1).astype(np.float32), (rng.standard_normal(20 * 22050) * 0.03).astype(np.float32)])

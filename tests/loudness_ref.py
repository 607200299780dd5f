"""float64 restatement of the output levelling (include/ttsamd.h, "output levelling"): the K-weighting coefficients by the bilinear
transform, the filter (scipy.signal.lfilter: transposed direct form II, zero state), the 400 ms blocks with the short-row rule, the
two gates of ITU-R BS.1770-4, the peak and the three gain modes -- and the segment scan the kernels run (zero-state responses of
segments stitched with the 4 x 4 transition matrix of one segment), so that its agreement with the sequential filter is a CPU fact."""
import numpy as np
from scipy.signal import lfilter

FS_MIN, FS_MAX = 8000, 192000
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz), as printed
TABLE_48K = dict(b1=[1.53512485958697, -2.69169618940638, 1.19839281085285], a1=[1.0, -1.69065929318241, 0.73248077421585],
                 b2=[1.0, -2.0, 1.0], a2=[1.0, -1.99004745483398, 0.99007225036621])


def coefficients(fs):
    """-> (b1, a1, b2, a2), float64 arrays of three: the shelf and the high-pass at sample rate fs"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return b1, a1, b2, a2


def coefficient_vector(fs):
    """the ten numbers ttsamd_loudness_coefficients writes: b1[0..2], a1[1..2], b2[0..2], a2[1..2]"""
    b1, a1, b2, a2 = coefficients(fs)
    return np.concatenate([b1, a1[1:], b2, a2[1:]])


def step_block(fs):
    step = (int(fs) + 5) // 10               # fs / 10 rounded, a half upwards
    return step, 4 * step


def kweight(x, fs):
    """stage 2 of stage 1 of x from a zero state, float64"""
    b1, a1, b2, a2 = coefficients(fs)
    return lfilter(b2, a2, lfilter(b1, a1, np.asarray(x, dtype=np.float64)))


def block_energies(y, fs):
    """z_j: the mean of y^2 over [j step, j step + block); one block over all n samples when 0 < n < block; none for n = 0"""
    step, block = step_block(fs)
    n = len(y)
    if n == 0:
        return np.zeros(0)
    y2 = np.asarray(y, dtype=np.float64) ** 2
    if n < block:
        return np.array([y2.sum() / n])
    J = (n - block) // step + 1
    return np.array([y2[j * step:j * step + block].sum() / block for j in range(J)])


def gate(z):
    """-> dict(L, gamma, l): integrated loudness, the relative threshold and the block loudnesses of the energies z"""
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(divide='ignore'):
        l = -0.691 + 10.0 * np.log10(z)
    a = l > -70.0
    if not a.any():
        return dict(L=-np.inf, gamma=-np.inf, l=l)
    gamma = -0.691 + 10.0 * np.log10(z[a].mean()) - 10.0
    r = a & (l > gamma)
    L = -0.691 + 10.0 * np.log10(z[r].mean()) if r.any() else -np.inf
    return dict(L=L, gamma=gamma, l=l)


def measure(x, fs, chunked=False):
    """-> dict(L, gamma, l, z, peak) of one row x (float32 samples)"""
    x = np.asarray(x, dtype=np.float32)
    y = kweight_chunked(x, fs) if chunked else kweight(x, fs)
    z = block_energies(y, fs)
    out = gate(z)
    out.update(z=z, peak=np.float32(np.abs(x).max()) if len(x) else np.float32(0))
    return out


def loudness(x, fs):
    return measure(x, fs)['L']


def gate_margin(m):
    """smallest distance in LU of any block loudness of measure()'s result from either gate (inf when there is no block)"""
    l = m['l'][np.isfinite(m['l'])]
    if not len(l):
        return np.inf
    d = np.abs(l + 70.0).min()
    if np.isfinite(m['gamma']):
        d = min(d, np.abs(l - m['gamma']).min())
    return float(d)


def gating_case():
    """3 s of noise at sigma 0.1 whose middle second is scaled by 1e-3, at 22 050 Hz: 27 blocks, L = -17.81, Gamma = -27.81"""
    x = (np.random.default_rng(0).standard_normal(3 * 22050) * 0.1).astype(np.float32)
    x[22050:44100] *= np.float32(1e-3)
    return x


# ---- the scan ----
def segment_length(step, longest=64):
    """the largest divisor of step that is <= longest"""
    return next(d for d in range(longest, 0, -1) if step % d == 0)


def _segment(b1, a1, b2, a2, x, state):
    """one segment from the state (s1, s2 of stage 1, s1, s2 of stage 2) -> (y, the state behind it)"""
    y1, z1 = lfilter(b1, a1, x, zi=state[:2])
    y2, z2 = lfilter(b2, a2, y1, zi=state[2:])
    return y2, np.concatenate([z1, z2])


def transition_matrix(fs, S):
    """M [4, 4]: the state behind S samples of zero input = M @ the state in front of them"""
    c = coefficients(fs)
    return np.stack([_segment(*c, np.zeros(S), e)[1] for e in np.eye(4)], axis=1)


def kweight_chunked(x, fs, S=None):
    """kweight as the kernels run it: every segment of S samples from a zero state, the final states carried along the row with M,
    every segment again from its true state"""
    x = np.asarray(x, dtype=np.float64)
    c = coefficients(fs)
    S = S or segment_length(step_block(fs)[0])
    M = transition_matrix(fs, S)
    segs = [x[k:k + S] for k in range(0, len(x), S)]
    zero = [_segment(*c, np.concatenate([s, np.zeros(S - len(s))]), np.zeros(4))[1] for s in segs]
    state, out = np.zeros(4), []
    for s, z in zip(segs, zero):
        out.append(_segment(*c, s, state)[0])
        state = M @ state + z
    return np.concatenate(out) if out else np.zeros(0)


# ---- the gain ----
MODES = {'off': 0, 'peak': 1, 'lufs': 2}


def gain(L, peak, mode, target, ceiling=0.99):
    """the float32 gain of a row (what the kernel writes to gain_out)"""
    peak = np.float32(peak)
    if mode == 1 and peak > 0:
        return np.float32(target) / peak
    if mode == 2 and peak > 0 and np.isfinite(L):
        g = 10.0 ** ((float(np.float32(target)) - L) / 20.0)
        if float(peak) * g > float(np.float32(ceiling)):
            g = float(np.float32(ceiling)) / float(peak)
        g = np.float32(g)
        if peak * g > np.float32(ceiling):             # float32 product: the rounding of g or of the product may pass the ceiling by one ulp
            g = np.nextafter(g, np.float32(0))
        return g
    return np.float32(1.0)


def apply(x, mode, target, peak, g, L=0.0):
    """numpy's float32 arithmetic on the row: mode 1 x / peak * target, mode 2 x * g; anything else, peak == 0 or L not finite: x"""
    x = np.asarray(x, dtype=np.float32)
    if mode == 1 and np.float32(peak) > 0:
        return x / np.float32(peak) * np.float32(target)
    if mode == 2 and np.float32(peak) > 0 and np.isfinite(L):
        return x * np.float32(g)
    return x.copy()

"""float64 numpy restatement of the wave-against-wave scores of include/ttsamd.h (csrc/wavescore.hip): STOI / ESTOI at 10 kHz, SI-SDR /
SNR and the log-spectral distance.  Written from the specification; it shares no code with the kernels.  tests/test_wavescore_cpu.py
pins it on the CPU, tests/test_gpu_wavescore.py uses it as the GPU yardstick."""
import numpy as np

EPS = 2.0 ** -52
WIN, HOP, NFFT, SEG, BANDS = 256, 128, 512, 30, 15
W = np.hanning(WIN + 2)[1:-1]
LO = np.array([7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174])
HI = np.array([9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219])
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
TOO_SHORT = 1e-5


def band_edges(fs=10000, nfft=NFFT, bands=BANDS, f0=150.0):
    """(lo, hi): the bins nearest to f0 * 2^((2 j -/+ 1) / 6) Hz on the grid k fs / nfft"""
    grid = np.arange(nfft // 2 + 1) * fs / nfft
    j = np.arange(bands)
    lo = np.array([np.argmin((grid - f0 * 2.0 ** ((2 * k - 1) / 6.0)) ** 2) for k in j])
    hi = np.array([np.argmin((grid - f0 * 2.0 ** ((2 * k + 1) / 6.0)) ** 2) for k in j])
    return lo, hi


def frames(x, win=WIN, hop=HOP):
    """x [n] -> [F, win] UNwindowed frames at hop; F = (n - win) // hop + 1, or 0 below win samples"""
    x = np.asarray(x, dtype=np.float64)
    F = (len(x) - win) // hop + 1 if len(x) >= win else 0
    if F == 0:
        return np.zeros((0, win))
    return np.stack([x[hop * f: hop * f + win] for f in range(F)])


def frame_energies_db(x):
    """e[f] = 20 log10(sqrt(sum (w x_f)^2) + EPS) of the frames of x"""
    xf = frames(x) * W
    return 20.0 * np.log10(np.sqrt(np.sum(xf * xf, axis=1)) + EPS)


def kept_frames(x):
    """indices of the frames of the clean signal x that survive the 40 dB silent-frame removal"""
    e = frame_energies_db(x)
    if e.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero(np.max(e) - 40.0 - e < 0)[0]


def threshold_margin_db(x):
    """the smallest |max e - 40 - e[f]| over the frames: how far the nearest frame lies from the silence threshold (inf without frames)"""
    e = frame_energies_db(x)
    return float(np.min(np.abs(np.max(e) - 40.0 - e))) if e.size else np.inf


def overlap_add(fr, hop=HOP):
    """[K, win] frames -> their overlap-add at hop, length hop (K - 1) + win, frames added in order"""
    K, win = fr.shape
    out = np.zeros(hop * (K - 1) + win)
    for k in range(K):
        out[hop * k: hop * k + win] += fr[k]
    return out


def remove_silent_frames(x, y):
    """-> (x', y', F, K): both rebuilt from the windowed frames the clean signal x keeps"""
    keep = kept_frames(x)
    xf, yf = frames(x) * W, frames(y) * W
    F, K = xf.shape[0], len(keep)
    if K == 0:
        return np.zeros(0), np.zeros(0), F, 0
    return overlap_add(xf[keep]), overlap_add(yf[keep]), F, K


def spectra(sig, win=WIN, hop=HOP, nfft=NFFT, window=W):
    """windowed frames of sig, zero-padded to nfft -> |X|^2 [F, nfft // 2 + 1]"""
    fr = frames(sig, win, hop) * window
    X = np.fft.rfft(fr, n=nfft, axis=1)
    return X.real ** 2 + X.imag ** 2


def third_octave(sig):
    """-> tob [15, K] and the total power of every frame (sum of |X|^2 over the 512 bins = 512 sum of the windowed frame squared)"""
    fr = frames(sig) * W
    P = spectra(sig)
    tob = np.stack([np.sqrt(np.sum(P[:, LO[j]:HI[j]], axis=1)) for j in range(BANDS)]) if P.shape[0] else np.zeros((BANDS, 0))
    return tob, NFFT * np.sum(fr * fr, axis=1)


def _row_norm(A):
    A = A - np.mean(A, axis=-1, keepdims=True)
    return A / (np.sqrt(np.sum(A * A, axis=-1, keepdims=True)) + EPS)


def stoi_segments(tx, ty, extended):
    """tob of both signals [15, K], K >= 30 -> the per-segment sums d[m] (before the division) and the smallest ratio of a centred
    row norm to its uncentred norm (the conditioning of the normalisation; inf where a row is all zero)"""
    K = tx.shape[1]
    d, cond = [], np.inf
    for m in range(SEG, K + 1):
        X, Y = tx[:, m - SEG: m], ty[:, m - SEG: m]
        if not extended:
            c = np.sqrt(np.sum(X * X, axis=1, keepdims=True)) / (np.sqrt(np.sum(Y * Y, axis=1, keepdims=True)) + EPS)
            Y = np.minimum(c * Y, X * CLIP)
        for A in (X, Y):
            un = np.sqrt(np.sum(A * A, axis=1))
            ce = np.sqrt(np.sum((A - A.mean(axis=1, keepdims=True)) ** 2, axis=1))
            if np.any(un > 0):
                cond = min(cond, float(np.min(ce[un > 0] / un[un > 0])))
        Xn, Yn = _row_norm(X), _row_norm(Y)
        if extended:
            Xn, Yn = _row_norm(Xn.T).T, _row_norm(Yn.T).T
        d.append(np.sum(Xn * Yn))
    return np.array(d), cond


def stoi_10k(x, y, extended=False, details=False):
    """x (clean), y (degraded): float arrays of one length at 10 kHz -> score; details: dict(score, frames=(F, K), tob_x, tob_y,
    power_x, power_y, margin_db, cond)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 1
    xs, ys, F, K = remove_silent_frames(x, y)
    if K:
        tx, px = third_octave(xs)
        ty, py = third_octave(ys)
    else:
        tx = ty = np.zeros((BANDS, 0))
        px = py = np.zeros(0)
    cond = np.inf
    if K < SEG:
        score = TOO_SHORT
    else:
        d, cond = stoi_segments(tx, ty, extended)
        M = K - SEG + 1
        score = float(np.sum(d) / SEG / M) if extended else float(np.sum(d) / (BANDS * M))
    if not details:
        return score
    return dict(score=score, frames=(F, K), tob_x=tx, tob_y=ty, power_x=px, power_y=py, margin_db=threshold_margin_db(x), cond=cond)


def sdr(ref, est, zero_mean=True):
    """-> (SI-SDR, SNR) in dB of est against ref; IEEE results as they fall"""
    r, e = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    with np.errstate(all='ignore'):
        if zero_mean:
            r = r - np.sum(r) / np.float64(len(r))
            e = e - np.sum(e) / np.float64(len(e))
        rr = np.float64(np.sum(r * r))
        alpha = np.float64(np.sum(e * r)) / rr
        t = alpha * r
        si = 10.0 * np.log10(np.float64(np.sum(t * t)) / np.float64(np.sum((t - e) ** 2)))
        sn = 10.0 * np.log10(rr / np.float64(np.sum((r - e) ** 2)))
    return float(si), float(sn)


def hann_periodic(n=1024):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def lsd(ref, est):
    """-> (log-spectral distance in dB, frames): frames of 1024 every 256 without padding; NaN without a frame"""
    w = hann_periodic(1024)
    Pr, Pe = spectra(ref, 1024, 256, 1024, w), spectra(est, 1024, 256, 1024, w)
    F = Pr.shape[0]
    if F == 0:
        return float('nan'), 0
    Lr, Le = 10.0 * np.log10(np.maximum(Pr, 1e-10)), 10.0 * np.log10(np.maximum(Pe, 1e-10))
    return float(np.mean(np.sqrt(np.mean((Lr - Le) ** 2, axis=1)))), F


def speech_like(n=20000, fs=10000, seed=0):
    """the deterministic test row: eight slowly vibrato'd harmonics of 120 Hz under a max(sin(2 pi 2.3 t), 0)^2 envelope, plus 1e-4 noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    phase = 2 * np.pi * 120.0 * t + 3.0 * np.sin(2 * np.pi * 5.0 * t)
    s = sum(np.sin(h * phase + 0.7 * h) / h for h in range(1, 9))
    env = np.maximum(np.sin(2 * np.pi * 2.3 * t), 0.0) ** 2
    return (0.3 * env * s + 1e-4 * rng.standard_normal(n)).astype(np.float32)


def add_noise(x, snr_db, seed=1):
    """x + white noise at snr_db (over the whole row), as float32"""
    rng = np.random.default_rng(seed)
    x64 = np.asarray(x, dtype=np.float64)
    noise = rng.standard_normal(len(x64))
    noise *= np.sqrt(np.sum(x64 * x64) / (np.sum(noise * noise) * 10.0 ** (snr_db / 10.0)))
    return (x64 + noise).astype(np.float32)

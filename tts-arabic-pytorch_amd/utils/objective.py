"""Objective evaluation of synthesised speech against a recording, on the device: mel-cepstral distortion (MCD) along a DTW path, the
mel error along it, F0 RMSE in cents and in Hz, F0 correlation and the voiced/unvoiced error.  The reference has no such module; the
arithmetic is this project's own, stated in DESIGN.md section 4 and include/ttsamd.h (ttsamd_mel_cepstrum, ttsamd_dtw_aligned_eval) and
restated in float64 by tests/objective_ref.py.  Parity with a particular MCD package is not pinned: the cepstrum here is the orthonormal
DCT-II of the natural-log mel, MCD = 10 sqrt(2) / ln 10 x the mean Euclidean distance of coefficients 1 .. n_coef - 1 along the path.
All arithmetic runs in libttsamd.so (csrc/objective.hip, csrc/oversmooth.hip) through ttsamd.engine; there is no CPU fallback: without a
gfx950 device every call raises ttsamd.lib.TtsAmdError.

Conventions (those of utils/oversmoothing.py): numpy arrays in give numpy arrays and floats out, tensors in give tensors on the device
out.  A batch is one more leading dimension ([B, n_mels, T] mels, [B, T] tracks) plus `lens_*` (int64 [B], None = full rows); batched
results carry the leading dimension.  Mels are natural-log mels (log(max(mel, 1e-5)) in the reference); an f0 track is in Hz, a frame is
voiced when its value is finite and > 0 (pyin's NaN fill and FastPitch.pitch_track(normalize=False)'s 0 both mean unvoiced).  At most
ttsamd.engine.OVERSMOOTH_MAX_FRAMES frames per side."""
import numpy as np
import torch

from ttsamd import engine as E
from ttsamd.lib import TtsAmdError
from utils.oversmoothing import _lens, _out, _prep

KEYS = E.OBJECTIVE_KEYS
MCD_SCALE = E.MCD_SCALE
_F0_KEYS = ('n', 'n_vv', 'f0_rmse_cents', 'f0_rmse_hz', 'f0_corr', 'vuv_error')
_engines = {}


def _pair(a, b, nd, what):
    """two inputs of the same kind -> (device tensors with a batch dimension, both came as numpy, came batched)"""
    x, np_x, batched = _prep(a, nd, f'{what}: prediction')
    y, np_y, batched_y = _prep(b, nd, f'{what}: reference')
    if batched != batched_y or x.shape[0] != y.shape[0]:
        raise TtsAmdError(f'{what}: prediction {tuple(x.shape)} and reference {tuple(y.shape)} differ in batch')
    return x, y.to(x.device), np_x and np_y, batched


def _scores(score, keys, was_np, batched):
    return {k: _out(score[k], was_np, batched) for k in keys}


def mel_cepstrum(logmel, n_coef=13, lens=None):
    """logmel [n_mels, T] -> [n_coef, T]: the orthonormal DCT-II across the bands of every frame
    (scipy.fft.dct(logmel, type=2, norm='ortho', axis=0)[:n_coef]), float64 inside, rounded once to float32."""
    m, was_np, batched = _prep(logmel, 2, 'mel_cepstrum')
    return _out(E.mel_cepstrum(m, _lens(lens, m, batched), n_coef), was_np, batched)


def objective_metrics(mel_pred, mel_ref, f0_pred=None, f0_ref=None, n_coef=13, align='dtw', window=None, lens_pred=None, lens_ref=None):
    """{n, mcd, mel_mae, n_vv, f0_rmse_cents, f0_rmse_hz, f0_corr, vuv_error} of a predicted log-mel [n_mels, Tp] against a reference
    [n_mels, Tr], with their f0 tracks [Tp] / [Tr] in Hz if given (NaN in the f0 scores otherwise).  align 'dtw': along the DTW path of
    the cepstra 1 .. n_coef - 1 (L2; `window` = Sakoe-Chiba radius or None); 'frames': frame by frame over the shorter side."""
    p, r, was_np, batched = _pair(mel_pred, mel_ref, 2, 'objective_metrics')
    if (f0_pred is None) != (f0_ref is None):
        raise TtsAmdError('objective_metrics: f0_pred and f0_ref come as a pair or not at all')
    fp = fr = None
    if f0_pred is not None:
        fp, fr, _, fb = _pair(f0_pred, f0_ref, 1, 'objective_metrics: f0')
        if fb != batched or fp.shape != (p.shape[0], p.shape[2]) or fr.shape != (r.shape[0], r.shape[2]):
            raise TtsAmdError(f'objective_metrics: f0 tracks {tuple(fp.shape)} / {tuple(fr.shape)} do not match the mels '
                              f'{tuple(p.shape)} / {tuple(r.shape)} frame for frame')
    score = E.objective_score(p, _lens(lens_pred, p, batched), r, _lens(lens_ref, r, batched), fp, fr, n_coef=n_coef, align=align,
                              window=window)
    return _scores(score, KEYS, was_np, batched)


def mel_cepstral_distortion(mel_pred, mel_ref, n_coef=13, align='dtw', window=None, lens_pred=None, lens_ref=None):
    """MCD in dB between two log-mels [n_mels, T]: 10 sqrt(2) / ln 10 x the mean over the path of the Euclidean distance between the
    cepstral coefficients 1 .. n_coef - 1 (c0, the level, is left out)."""
    return objective_metrics(mel_pred, mel_ref, None, None, n_coef, align, window, lens_pred, lens_ref)['mcd']


def f0_metrics(f0_pred, f0_ref, path=None, path_len=None, lens_pred=None, lens_ref=None):
    """{n, n_vv, f0_rmse_cents, f0_rmse_hz, f0_corr, vuv_error} of two f0 tracks [T] in Hz.  path None: frame by frame over the shorter
    side; else the (i, j) steps to compare, [L, 2] for one pair (as dtw_align_mels returns them), or [B, Tp + Tr, 2] with path_len [B]
    for a batch (as ttsamd.engine.dtw does)."""
    a, b, was_np, batched = _pair(f0_pred, f0_ref, 1, 'f0_metrics')
    B, Ta = a.shape
    Tb = b.shape[1]
    if path is None:
        path, path_len = E.identity_path(_lens(lens_pred, a, batched), _lens(lens_ref, b, batched), Ta, Tb)
    else:
        path = torch.as_tensor(np.asarray(path) if not isinstance(path, torch.Tensor) else path).to(device=a.device, dtype=torch.int32)
        if not batched:
            if path.dim() != 2 or path.shape[1] != 2 or path.shape[0] > Ta + Tb:
                raise TtsAmdError(f'f0_metrics: path of shape {tuple(path.shape)} for tracks of {Ta} and {Tb} frames ([L, 2] is expected)')
            path_len = torch.full((1,), path.shape[0], dtype=torch.int32, device=a.device)
            path = torch.nn.functional.pad(path, (0, 0, 0, Ta + Tb - path.shape[0]))[None]
        elif path_len is None:
            raise TtsAmdError('f0_metrics: a batched path goes with path_len')
        path_len = torch.as_tensor(path_len).to(device=a.device, dtype=torch.int32)
    zero = torch.zeros(B, 1, 1, dtype=torch.float32, device=a.device)
    stats = E.dtw_aligned_eval(zero.expand(B, 1, Ta), zero.expand(B, 1, Tb), path.contiguous(), path_len, f0_a=a, f0_b=b, first_coef=0)
    return {k: _out(stats[:, KEYS.index(k)], was_np, batched) for k in _F0_KEYS}


def evaluate_waves(wave_pred, wave_ref, n_coef=13, align='dtw', window=None, lens_pred=None, lens_ref=None):
    """The eight scores of a synthesised wave [n] against a recording [n'], both at 22 050 Hz: the reference's log-mel analysis and pYIN
    settings on both (ttsamd.engine.ObjectiveEngine), then objective_metrics.  `lens_*`: samples per row of a batch."""
    x, y, was_np, batched = _pair(wave_pred, wave_ref, 1, 'evaluate_waves')
    if str(x.device) not in _engines:
        _engines[str(x.device)] = E.ObjectiveEngine(device=x.device)
    score = _engines[str(x.device)].score_waves(x, _lens(lens_pred, x, batched), y, _lens(lens_ref, y, batched), n_coef=n_coef, align=align,
                                                window=window)
    return _scores(score, KEYS, was_np, batched)


# ---- wave against wave, sample for sample (csrc/wavescore.hip) -------------------------------------------------------------------------
# STOI / ESTOI, SI-SDR / SNR and a log-spectral distance between two SAMPLE-ALIGNED waves: copy synthesis (a recording against its own
# analysis and resynthesis), one precision mode against another, a delivery format against the float wave.  Free-running synthesis is
# not sample-aligned with a recording, so a wave-level score of it would be meaningless: evaluate_waves and FastPitch2Wave.evaluate stay
# on the DTW-aligned feature scores above and do not call these.  Specified by their arithmetic (include/ttsamd.h, restated in float64
# by tests/wavescore_ref.py); parity with a release of pystoi is not pinned, and the 10 kHz resampling is the project's own resampler
# (lowpass_filter_width = 64), not pystoi's.  float64 throughout.  The multi-resolution STFT distance (csrc/mrstft.hip, restated by
# tests/mrstft_ref.py) is specified by its arithmetic; the framing is `torch.stft`'s, parity with `auraloss` or Parallel WaveGAN's
# batch-wide sums unpinned.  Out of scope: PESQ, VISQOL, use as training losses, time alignment of unaligned waves.
WAVE_KEYS = ('stoi', 'estoi', 'si_sdr', 'snr', 'lsd', 'frames', 'frames_kept')
MR_STFT_KEYS = ('mr_stft', 'spectral_convergence', 'log_stft_magnitude', 'per_resolution', 'frames')


def _wave_pair(wave_a, wave_b, lens, what):
    """-> (a, b [B, n] on the device, lens int64 [B], both numpy, batched).  The two waves of a pair share one length per row; rows of
    different padded width are compared over the min of the two."""
    a, np_a, batched = _prep(wave_a, 1, f'{what}: first wave')
    b, np_b, batched_b = _prep(wave_b, 1, f'{what}: second wave')
    if batched != batched_b or a.shape[0] != b.shape[0]:
        raise TtsAmdError(f'{what}: waves of shape {tuple(a.shape)} and {tuple(b.shape)} differ in batch')
    b = b.to(a.device)
    W = min(a.shape[1], b.shape[1])
    a, b = a[:, :W].contiguous(), b[:, :W].contiguous()
    return a, b, _lens(lens, a, batched), np_a and np_b, batched


def stoi(wave_ref, wave_deg, fs=22050, extended=False, lens=None):
    """Short-time objective intelligibility (extended: ESTOI) of wave_deg [n] against the clean wave_ref [n], both at `fs` Hz: resampled
    to 10 kHz on the device, silent frames removed on the clean signal, fifteen third-octave bands, segments of 30 frames.  1e-5 for a
    row with fewer than 30 kept frames.  The two waves share `lens`; rows of different padded width are compared over the min of the two."""
    r, d, n, was_np, batched = _wave_pair(wave_ref, wave_deg, lens, 'stoi')
    return _out(E.wave_scorer(fs, r.device).stoi(r, d, n, extended=extended)[0], was_np, batched)


def si_sdr(wave_est, wave_ref, zero_mean=True, lens=None):
    """Scale-invariant signal-to-distortion ratio in dB of wave_est [n] against wave_ref [n] (zero_mean: both centred first); +inf for
    identical rows.  The two waves share `lens`; rows of different padded width are compared over the min of the two."""
    e, r, n, was_np, batched = _wave_pair(wave_est, wave_ref, lens, 'si_sdr')
    return _out(E.wave_sdr(r, e, n, zero_mean=zero_mean)[:, 0], was_np, batched)


def snr(wave_est, wave_ref, zero_mean=True, lens=None):
    """Signal-to-noise ratio in dB, 10 log10(sum ref^2 / sum (ref - est)^2), with si_sdr's conventions (it is NOT invariant to the
    scale of wave_est)."""
    e, r, n, was_np, batched = _wave_pair(wave_est, wave_ref, lens, 'snr')
    return _out(E.wave_sdr(r, e, n, zero_mean=zero_mean)[:, 1], was_np, batched)


def log_spectral_distance(wave_est, wave_ref, lens=None):
    """Log-spectral distance in dB of wave_est [n] against wave_ref [n]: frames of 1024 every 256 samples (no padding), periodic Hann,
    the mean over frames of the rms over bins 0 .. 512 of the difference of 10 log10 max(|X|^2, 1e-10); NaN under 1024 samples.  The two
    waves share `lens`; rows of different padded width are compared over the min of the two."""
    e, r, n, was_np, batched = _wave_pair(wave_est, wave_ref, lens, 'log_spectral_distance')
    return _out(E.log_spectral_distance(r, e, n)[:, 0], was_np, batched)


def _resolutions(fft_sizes, hop_sizes, win_lengths, what):
    try:
        res = tuple(zip(*(tuple(int(v) for v in a) for a in (fft_sizes, hop_sizes, win_lengths)), strict=True))
    except (TypeError, ValueError):
        raise TtsAmdError(f'{what}: fft_sizes {fft_sizes!r}, hop_sizes {hop_sizes!r} and win_lengths {win_lengths!r} are not three '
                          f'sequences of integers of one length') from None
    return res


def _mr_scores(per, frames):
    """per [B, R, 2], frames [B, R] -> the MR_STFT_KEYS dict of device tensors; NaN where any resolution is NaN (the mean over them)"""
    sc, mag = per[:, :, 0].mean(dim=1), per[:, :, 1].mean(dim=1)
    return dict(mr_stft=sc + mag, spectral_convergence=sc, log_stft_magnitude=mag, per_resolution=per, frames=frames)


def multi_resolution_stft(wave_est, wave_ref, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), lens=None):
    """Multi-resolution STFT distance of wave_est [n] against the sample-aligned wave_ref [n] (Parallel WaveGAN's three resolutions by
    default; n_fft in 512 / 1024 / 2048, up to eight).  Per resolution, on torch.stft's framing (center=True, reflect padding, periodic
    Hann of win_length centred in the frame) with S = sqrt(max(|X|^2, 1e-7)): the spectral convergence ||S_ref - S_est|| / ||S_ref|| and
    the log-magnitude distance mean |ln S_ref - ln S_est|, over the row's own frames.  -> {mr_stft, spectral_convergence,
    log_stft_magnitude, per_resolution [R, 2], frames [R]}: the two means over the resolutions, their sum first; NaN where any resolution
    is NaN (a row of n_fft / 2 samples or fewer).  The two waves share `lens`; rows of different padded width are compared over the min
    of the two."""
    res = _resolutions(fft_sizes, hop_sizes, win_lengths, 'multi_resolution_stft')
    e, r, n, was_np, batched = _wave_pair(wave_est, wave_ref, lens, 'multi_resolution_stft')
    return _scores(_mr_scores(*E.mr_stft(r, e, n, res)), MR_STFT_KEYS, was_np, batched)


def stft_distance(wave_est, wave_ref, n_fft=1024, hop_length=256, win_length=None, lens=None):
    """-> (spectral convergence, log-magnitude distance) of wave_est [n] against wave_ref [n] at ONE resolution (win_length None: n_fft):
    the bits of that resolution's row of multi_resolution_stft's per_resolution."""
    res = _resolutions((n_fft,), (hop_length,), (n_fft if win_length is None else win_length,), 'stft_distance')
    e, r, n, was_np, batched = _wave_pair(wave_est, wave_ref, lens, 'stft_distance')
    per, _ = E.mr_stft(r, e, n, res)
    return _out(per[:, 0, 0], was_np, batched), _out(per[:, 0, 1], was_np, batched)


def _wave_scores(ref, est, n, fs, mr_stft, was_np, batched):
    score = E.wave_scorer(fs, ref.device).metrics(ref, est, n)
    keys = WAVE_KEYS
    if mr_stft:
        score.update({k: v for k, v in _mr_scores(*E.mr_stft(ref, est, n)).items() if k in MR_STFT_KEYS[:3]})
        keys = WAVE_KEYS + MR_STFT_KEYS[:3]
    return _scores(score, keys, was_np, batched)


def wave_metrics(wave_est, wave_ref, fs=22050, lens=None, mr_stft=False):
    """{stoi, estoi, si_sdr (zero-mean), snr, lsd, frames, frames_kept} of wave_est [n] against the sample-aligned wave_ref [n] at `fs`
    Hz; frames / frames_kept are the STOI frames at 10 kHz before and after the silent-frame removal.  mr_stft: + {mr_stft,
    spectral_convergence, log_stft_magnitude} of multi_resolution_stft at its default resolutions.  The two waves share `lens`; rows
    of different padded width are compared over the min of the two."""
    e, r, n, was_np, batched = _wave_pair(wave_est, wave_ref, lens, 'wave_metrics')
    return _wave_scores(r, e, n, fs, mr_stft, was_np, batched)


def copy_synthesis(vocoder, wave, lens=None, mr_stft=False):
    """Copy synthesis, the standard way to judge a vocoder: `wave` [n] at 22 050 Hz is analysed with ObjectiveEngine's log-mel analysis,
    the HiFi-GAN `Generator` resynthesises it (vocoder.engine().forward(mel, frames)) under the current ttsamd.engine.set_precision
    mode, and the result is scored against the input over 256 * frames samples.  -> (wave_metrics dict (mr_stft: with its three
    multi-resolution STFT entries), the resynthesised wave [256 * frames] on the device, or numpy for numpy input).  Vocos and Tacotron2
    are out of scope for this helper."""
    x, was_np, batched = _prep(wave, 1, 'copy_synthesis')
    n = _lens(lens, x, batched)
    if str(x.device) not in _engines:
        _engines[str(x.device)] = E.ObjectiveEngine(device=x.device)
    if x.shape[1] < E.MelSpecEngine.MIN_SAMPLES['same']:
        raise TtsAmdError(f'copy_synthesis: rows of {x.shape[1]} samples; the mel analysis needs at least '
                          f'{E.MelSpecEngine.MIN_SAMPLES["same"]}')
    mel, frames = _engines[str(x.device)].melspec.forward(x, n)
    out = vocoder.engine().forward(mel, frames)
    W = min(out.shape[1], x.shape[1])
    return (_wave_scores(x[:, :W].contiguous(), out[:, :W].contiguous(), 256 * frames, 22050, mr_stft, was_np, batched),
            _out(out, was_np, batched))

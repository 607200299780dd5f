"""Drop-in for the reference's utils/metrics.py, the older twin of utils/oversmoothing.py: the same measures and the same DTW under the
older names, over the same engine (csrc/oversmooth.hip through ttsamd.engine), so that code written against either module runs.
What differs from utils.oversmoothing: dtw_align_mels accepts [T, M] or [M, T] and guesses the layout (`_ensure_time_major`),
compute_mel_over_smoothing_metrics takes `assume_BxT`, and the aligned comparison always applies the hann window.  (The reference's
commented-out parselmouth code and pYIN f0 are not part of this project.)  No CPU fallback: without a gfx950 device every call raises."""
from ttsamd.lib import TtsAmdError
from utils import oversmoothing as _ov
from utils.oversmoothing import (hqer_from_power, slope_from_power, centroid_from_power, rolloff_from_power,  # noqa: F401
                                 framewise_rfft_power as _framewise_rfft_power)


def _ensure_time_major(x):
    """[T, M] or [M, T] -> [T, M]: the axis with fewer entries is taken for the mel bands (frames usually outnumber bands); a square
    input is taken as time-major already."""
    if x.ndim != 2:
        raise ValueError(f'Expected 2D array, got {tuple(x.shape)}')
    return x.T if x.shape[0] < x.shape[1] else x


def dtw_align_mels(mel_a, mel_b, metric='cosine', window=None, return_aligned=True):
    """DTW of two mels given as [T, M] or [M, T] -> (cost, path [L, 2]) and, with return_aligned, the sequences along the path [L, M]."""
    return _ov.dtw_align_mels(_ensure_time_major(mel_a).T, _ensure_time_major(mel_b).T, metric=metric, window=window,
                              return_aligned=return_aligned)


def compute_mel_over_smoothing_metrics(mel, assume_BxT=True, center=True, hann=True, q_c=None, reduction='none'):
    """{HQER (x 100), CSlope, CCentroid, CRoll95, Q} of one utterance; assume_BxT True: mel is [bands, T], False: [T, bands]."""
    if assume_BxT is True:
        mel_BxT = mel
    elif assume_BxT is False:
        mel_BxT = mel.T
    else:
        raise TtsAmdError('compute_mel_over_smoothing_metrics: assume_BxT must be True or False (the reference has no auto-detection either)')
    return _ov.compute_mel_oversmoothing_metrics(mel_BxT, center=center, hann=hann, q_c=q_c, reduction=reduction)


def aligned_distance(series_pred, series_ref):
    return _ov.aligned_mae_distance(series_pred, series_ref)


def over_smoothing_metric_aligned(mel_spec_pred, mel_spec_ref, center=True):
    return _ov.oversmoothing_metrics_aligned(mel_spec_pred, mel_spec_ref, center=center, hann=True)

"""Drop-in for the reference's models/fastpitch/fastpitch/data_function.py: the alignment prior (:45-78), `BetaBinomialInterpolator` and
`beta_binomial_prior_distribution`, computed by ttsamd_attn_prior (csrc/attn_loss.hip) in float64 on the device and copied back, float64 on
the CPU as the reference returns them (a batch of priors that stays on the device: ttsamd.engine.attention_prior); and the pitch part
(:81-122), `estimate_pitch` and `normalize_pitch`, with the reference's signatures.  The track comes from utils.pitch.pyin (csrc/pyin.hip) with the reference's
settings: C2..C7, frame_length 1024, hop 256, 22 050 Hz.  The reference loads the file with librosa.load, which resamples to 22 050 Hz;
there is no resampler here, so a file at another rate raises.  No CPU fallback."""
import numpy as np
import torch
import torch.nn.functional as F

from ttsamd.lib import TtsAmdError
from utils.audio import load_wav
from utils.pitch import note_to_hz, pyin

SAMPLE_RATE = 22050


def _prior(in_len, mel_len, mode, scaling=1.0):
    from ttsamd.engine import attention_prior
    return attention_prior([int(in_len)], [int(mel_len)], n_tokens=int(in_len), n_frames=int(mel_len), mode=mode, scaling=scaling,
                           dtype=torch.float64)[0].cpu()


def beta_binomial_prior_distribution(phoneme_count, mel_count, scaling=1.0):
    """-> float64 tensor [mel_count, phoneme_count] on the CPU: row i - 1 is betabinom(n = phoneme_count, a = scaling i, b = scaling
    (mel_count + 1 - i)).pmf(0 .. phoneme_count - 1).  n is phoneme_count, not phoneme_count - 1, so a row does not add up to 1: the
    reference's behaviour.  Only scaling = 1 is built."""
    return _prior(phoneme_count, mel_count, 'exact', scaling)


class BetaBinomialInterpolator:
    """The reference's prior bank: the exact prior of sizes rounded to 100 frames / 20 tokens, resized to the sizes asked for with
    scipy.ndimage.zoom(order=1).  Here nothing is cached or resized: every cell is computed where it is asked for, with the same
    arithmetic (the four bank values around it, interpolated in float64)."""

    def __init__(self, round_mel_len_to=100, round_text_len_to=20):
        if (round_mel_len_to, round_text_len_to) != (100, 20):
            raise TtsAmdError(f'BetaBinomialInterpolator: rounding to {round_mel_len_to} frames / {round_text_len_to} tokens; 100 / 20, '
                              'the values every caller of the reference uses, are built')
        self.round_mel_len_to = round_mel_len_to
        self.round_text_len_to = round_text_len_to

    def round(self, val, to):
        return max(1, int(np.round((val + 1) / to))) * to

    def __call__(self, w, h):
        """w = mel length, h = text length -> float64 numpy [w, h]"""
        ret = _prior(h, w, 'interpolated').numpy()
        assert ret.shape == (w, h), ret.shape
        return ret


def normalize_pitch(pitch, mean, std):
    """(pitch - mean[:, None]) / std[:, None] in place with the zeros (unvoiced frames) kept at zero; pitch [n_formants, T]."""
    zeros = (pitch == 0.0)
    pitch -= mean[:, None]
    pitch /= std[:, None]
    pitch[zeros] = 0.0
    return pitch


def fit_to_mel_len(track, mel_len):
    """[1, T] -> [1, mel_len]: trimmed at the end or zero-padded, as F.pad with a possibly negative amount does."""
    return F.pad(track, (0, int(mel_len) - track.size(1)))


def estimate_pitch(wav, mel_len, method='pyin', normalize_mean=None, normalize_std=None, n_formants=1):
    """wav: path of a 22 050 Hz .wav file, or a 1-D tensor / array of samples at that rate -> float32 [1, mel_len] on the CPU (the data
    loader's side, as in the reference): f0 in Hz, 0 where unvoiced, normalised when a mean and a std are given."""
    if type(normalize_mean) is float or type(normalize_mean) is list:
        normalize_mean = torch.tensor(normalize_mean)
    if type(normalize_std) is float or type(normalize_std) is list:
        normalize_std = torch.tensor(normalize_std)
    if method != 'pyin':
        raise ValueError(f'estimate_pitch: method {method!r} (only pyin, as in the reference)')
    if isinstance(wav, torch.Tensor):
        snd = wav.reshape(-1)
    elif isinstance(wav, np.ndarray):
        snd = np.ascontiguousarray(wav, dtype=np.float32).reshape(-1)
    else:
        snd, sr = load_wav(wav)
        if sr != SAMPLE_RATE:
            raise TtsAmdError(f'estimate_pitch: {wav} is sampled at {sr} Hz; only {SAMPLE_RATE} Hz is built (there is no resampler)')
    pitch_mel, _, _ = pyin(snd, fmin=note_to_hz('C2'), fmax=note_to_hz('C7'), frame_length=1024)
    if isinstance(pitch_mel, torch.Tensor):
        pitch_mel = pitch_mel.cpu().numpy()
    assert np.abs(mel_len - pitch_mel.shape[0]) <= 1.0
    pitch_mel = np.where(np.isnan(pitch_mel), 0.0, pitch_mel)
    pitch_mel = fit_to_mel_len(torch.from_numpy(pitch_mel).unsqueeze(0), mel_len)
    if n_formants > 1:
        raise NotImplementedError
    pitch_mel = pitch_mel.float()
    if normalize_mean is not None:
        assert normalize_std is not None
        pitch_mel = normalize_pitch(pitch_mel, normalize_mean.reshape(-1), normalize_std.reshape(-1))
    return pitch_mel

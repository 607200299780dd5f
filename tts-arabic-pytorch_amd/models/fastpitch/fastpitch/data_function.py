"""Drop-in for the pitch part of the reference's models/fastpitch/fastpitch/data_function.py (:81-122): `estimate_pitch` and
`normalize_pitch` with the reference's signatures.  The track comes from utils.pitch.pyin (csrc/pyin.hip) with the reference's
settings: C2..C7, frame_length 1024, hop 256, 22 050 Hz.  The reference loads the file with librosa.load, which resamples to 22 050 Hz;
there is no resampler here, so a file at another rate raises.  No CPU fallback."""
import numpy as np
import torch
import torch.nn.functional as F

from ttsamd.lib import TtsAmdError
from utils.audio import load_wav
from utils.pitch import note_to_hz, pyin

SAMPLE_RATE = 22050


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

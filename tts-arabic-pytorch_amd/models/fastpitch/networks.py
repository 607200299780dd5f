"""Drop-in for the reference's models/fastpitch/networks.py: same classes, signatures,
defaults and return conventions, with the arithmetic routed to the HIP engines.

  FastPitch       (reference :45-253)  checkpoint -> .infer/.ttmel/.ttmel_single/.ttmel_batch
  FastPitch2Wave  (reference :256-435) + vocoder + denoiser -> .tts/.tts_single/.tts_batch
  text_collate_fn (:16-35), pitch_trf (:38-42)

Differences, all host-side: the vocoder runs ONCE on the ragged batch instead of in a
per-utterance loop (:340-345) — results are identical because every layer pads at the true
utterance edge — `vowelizer=` runs the Shakkelha / Shakkala taggers of models/diacritizers on the HIP tagger engine.
"""
from collections import namedtuple
from typing import List, Optional, Union

import numpy as np
import os
import torch
import torch.nn as nn

import text
from ttsamd.engine import ALIGNER_KEYS, OBJECTIVE_KEYS, AlignerEngine, FastPitchEngine, ObjectiveEngine
from ttsamd.engine import average_pitch as _average_pitch
from ttsamd.engine import binarization_loss as _binarization_loss
from ttsamd.engine import forward_sum_loss as _forward_sum_loss
from ttsamd.engine import mas as _mas
from ttsamd.engine import check_finite, check_limiter, check_normalize, check_speakers, check_true_peak, level_waves, limiter_spec, per_row, \
    row_values
from ttsamd.lib import TtsAmdError
from utils import get_basic_config
from models.diacritizers import load_vowelizer
from vocoder import load_hifigan
from vocoder.hifigan.denoiser import Denoiser
from vocoder.hifigan.models import _HipModule


def text_collate_fn(batch: List[torch.Tensor]):
    """Sort by length (descending), zero-pad; returns (ids_pad, lens_sorted, reverse_ids)."""
    lens_sorted, sort_ids = torch.sort(torch.LongTensor([len(x) for x in batch]), descending=True)
    ids_pad = torch.zeros(len(batch), int(lens_sorted[0]), dtype=torch.long)
    for i, j in enumerate(sort_ids):
        ids_pad[i, :batch[j].size(0)] = batch[j]
    return ids_pad, lens_sorted, sort_ids.argsort()


# ---- mixed requests: `speed`, `speaker_id`, `pitch_mul`, `pitch_add` (and `denoise` and `normalize` on the wave side) are one scalar for all lines or a
# list with one value per line.  A list follows its lines through every reordering (the collate sort, the chunks, the length-sorted
# groups) by being indexed with the same positions as the lines: _take.
def _take(value, idx):
    """The control for the lines at positions `idx`: a scalar as it is, a per-line list picked in that order."""
    return [value[i] for i in idx] if per_row(value) else value


def _at(value, i):
    return value[i] if per_row(value) else value


def _lim(limiter, normalize, true_peak=False):
    """the `limiter` and `true_peak` keywords for a call that gets `normalize` (one option or a list): only where they are asked for and
    a line of that call asks for a level -- every other call gets exactly the arguments it got before"""
    if not any(v is not None for v in (normalize if per_row(normalize) else [normalize])):
        return {}
    return dict({'limiter': limiter} if limiter else {}, **({'true_peak': True} if true_peak else {}))


def check_line_controls(n_lines, n_speakers, speed=1., speaker_id=0, pitch_mul=1., pitch_add=0., denoise=0., normalize=None, true_peak=False):
    """Host-side validation of per-line controls before any work: a list must have one value per line (ValueError), speakers lie in
    [0, n_speakers) (IndexError), speeds are finite and > 0, pitch values and denoise strengths finite (ValueError).  Scalars pass
    through to the checks of the calls that take them.  `normalize` (the level of the wave: None, 'peak', 'lufs' or a finite target in
    LUFS, one for all lines or one per line) is checked in both forms: nothing below looks at it before the vocoder has run.
    `true_peak` (False or True: the peaks of `normalize` and of its limiter are true peaks) with no line that asks for a level is a
    ValueError."""
    check_normalize(normalize, n_lines)
    check_true_peak(true_peak, normalize, None)
    for what, v in (('speed', speed), ('speaker_id', speaker_id), ('pitch_mul', pitch_mul), ('pitch_add', pitch_add), ('denoise', denoise)):
        if not per_row(v):
            continue
        vals = row_values(v, n_lines, what)
        if what == 'speaker_id':
            check_speakers(vals, n_speakers, what)
        else:
            check_finite(vals, what, positive=(what == 'speed'))


# what FastPitch.align returns: dur_tgt [B, L], pitch_tgt / energy_tgt [B, 1, L] or None, the attention maps [B, 1, T, L] or None
Alignment = namedtuple('Alignment', ['dur_tgt', 'pitch_tgt', 'energy_tgt', 'attn_soft', 'attn_hard', 'attn_logprob'])
# what FastPitch.alignment_score returns: per row the forward-sum cost per token and the binarization cost per frame [B] float64, the
# durations [B, L], and the two batch scalars as the reference's AttentionCTCLoss / AttentionBinarizationLoss report them
AlignmentScore = namedtuple('AlignmentScore', ['forward_sum', 'binarization', 'dur_tgt', 'ctc_loss', 'bin_loss'])


def _attention_tensors(model_sd):
    """the aligner's tensors of a checkpoint (`attention.*`, reference model.py:234), kept apart from the inference weights"""
    return {k: v.detach().cpu().float().numpy() for k, v in model_sd.items()
            if torch.is_tensor(v) and v.is_floating_point() and k.startswith('attention.')}


def pitch_trf(mul: float = 1, add: float = 0):
    """Affine transform of the *normalised* pitch prediction; mean/std are ignored, as in the
    reference (:38-42).  Tagged so `infer` can run it inside the HIP predictor head."""
    def _pitch_trf(pitch_pred, enc_mask_sum, mean, std):
        return mul * pitch_pred + add
    _pitch_trf.affine = (float(mul), float(add))
    return _pitch_trf


class FastPitch(_HipModule):
    def __init__(self, checkpoint: str, arabic_in: bool = True, vowelizer: Optional[str] = None, **kwargs):
        super().__init__()
        from models.fastpitch import net_config
        state_dicts = torch.load(checkpoint, map_location='cpu')
        self.net_config = dict(state_dicts['config']) if 'config' in state_dicts else dict(net_config)
        self.arabic_in = arabic_in
        self._sd = {k: v.detach().cpu().float().numpy() for k, v in state_dicts['model'].items()
                    if torch.is_tensor(v) and v.is_floating_point() and not k.startswith('attention.')}
        self._attn_sd = _attention_tensors(state_dicts['model'])      # host copies; nothing goes to the GPU before the first align()
        self._aligners = {}
        self.config = get_basic_config()
        self.vowelizers = {}
        if vowelizer is not None:
            self.vowelizers[vowelizer] = load_vowelizer(vowelizer, self.config)
        self.default_vowelizer = vowelizer
        self.phon_to_id = None
        if 'symbols' in state_dicts:
            self.phon_to_id = {phon: i for i, phon in enumerate(state_dicts['symbols'])}
        self.pitch_mean = float(self._sd.get('pitch_mean', np.zeros(1))[0])
        self.pitch_std = float(self._sd.get('pitch_std', np.zeros(1))[0])
        self.eval()

    def engine(self):
        return self._engine(lambda dev: FastPitchEngine(self._sd, self.net_config, device=dev))

    def load_state_dict(self, state_dict, strict=True):
        self._sd = {k: v.detach().cpu().float().numpy() for k, v in state_dict.items()
                    if torch.is_tensor(v) and v.is_floating_point() and not k.startswith('attention.')}
        self._engines.clear()
        self._attn_sd = _attention_tensors(state_dict)
        self._aligners.clear()

    def state_dict(self, *a, **k):
        return {k_: torch.from_numpy(v) for k_, v in self._sd.items()}

    def release_device_memory(self):
        super().release_device_memory()
        self._aligners.clear()

    # ---- forced alignment: the aligner path of FastPitch.forward (models/fastpitch/fastpitch/model.py:298-318,331-332) ----
    def aligner(self):
        """The AlignerEngine of the device the module is on, created on first use from the checkpoint's `attention.*` tensors."""
        dev = self.device
        if dev.type != 'cuda':
            raise TtsAmdError(f'FastPitch is on {dev}: the MI355X path has no CPU fallback; move the module with .to("cuda")')
        missing = [k for k in ALIGNER_KEYS if k != 'encoder.word_emb.weight' and k not in self._attn_sd]
        if missing:
            raise TtsAmdError(f'this checkpoint carries no aligner: missing {", ".join(missing)}')
        if str(dev) not in self._aligners:
            sd = dict(self._attn_sd)
            sd['encoder.word_emb.weight'] = self._sd['encoder.word_emb.weight']
            self._aligners[str(dev)] = AlignerEngine(sd, self.net_config, device=dev)
        return self._aligners[str(dev)]

    def _align_ids(self, ids_or_text):
        """ids int64 [B, L] as they are; one utterance or a list of utterances as text: tokenised like ttmel and zero-padded at the end"""
        if isinstance(ids_or_text, str):
            ids_or_text = [ids_or_text]
        if isinstance(ids_or_text, (list, tuple)) and len(ids_or_text) and isinstance(ids_or_text[0], str):
            rows = [text.tokens_to_ids(self._tokenize(line), self.phon_to_id) for line in ids_or_text]
            ids = torch.full((len(rows), max(len(r) for r in rows)), self.net_config['padding_idx'], dtype=torch.int64)
            for b, r in enumerate(rows):
                ids[b, :len(r)] = torch.as_tensor(r, dtype=torch.int64)
            return ids
        return torch.as_tensor(ids_or_text).long()

    @torch.inference_mode()
    def align(self, ids_or_text, mel, mel_lens=None, attn_prior=None, pitch=None, energy=None, return_attn=False):
        """Forced alignment of a recording with its text, as the reference's training forward does it (model.py:298-318,331-332): the
        checkpoint's ConvAttention scores every (frame, token) pair, monotonic alignment search picks the best monotonic path, and a token's
        duration is the number of frames the path gives it.  ids_or_text: int64 ids [B, L] zero-padded at the end, or one utterance / a
        list of utterances as text (tokenised like ttmel; rows keep the order given).  mel [B, n_mel, T] (+ mel_lens [B], None: T frames
        each); attn_prior [B, T, L], None, or 'interpolated' / 'exact': the beta-binomial prior of the rows' own lengths, built on the device
        ('interpolated' is what the reference's data loader hands the model in training); pitch [B, 1, T] / [B, T] and energy [B, T], frame-level tracks to average per token.
        -> Alignment(dur_tgt [B, L], pitch_tgt [B, 1, L] | None, energy_tgt [B, 1, L] = log(1 + mean) | None, attn_soft, attn_hard,
        attn_logprob [B, 1, T, L] with return_attn, else None); dur_tgt, pitch_tgt and energy_tgt feed infer() as they are."""
        ids = self._align_ids(ids_or_text)
        eng = self.aligner()
        out = eng.align(ids, mel, mel_lens, attn_prior=attn_prior, return_attn=return_attn)
        dur, soft, hard, logprob = out if return_attn else (out, None, None, None)
        pitch_tgt = energy_tgt = None
        if pitch is not None:
            pitch = torch.as_tensor(pitch).to(dur.device)
            pitch_tgt = _average_pitch(pitch[:, None] if pitch.dim() == 2 else pitch, dur)
        if energy is not None:
            energy = torch.as_tensor(energy).to(dur.device)
            energy_tgt = torch.log(1.0 + _average_pitch(energy[:, None] if energy.dim() == 2 else energy, dur))
        return Alignment(dur, pitch_tgt, energy_tgt, soft, hard, logprob)

    @torch.inference_mode()
    def timestamps(self, ids_or_text, mel, mel_lens=None, attn_prior=None):
        """Word and token timings of a RECORDING from the checkpoint's own aligner: align()'s durations (whole frames per token) through
        the kernel the synthesis timestamps use (ttsamd.timing), at 256 samples a frame.  ids_or_text and mel as align() takes them ->
        one timing dict per row (one dict for a single string): positions in samples of the recording the mel was made of.  Given ids
        instead of text, a word is named by its tokens."""
        single = isinstance(ids_or_text, str)
        if single:
            ids_or_text = [ids_or_text]
        if isinstance(ids_or_text, (list, tuple)) and len(ids_or_text) and isinstance(ids_or_text[0], str):
            toks = [self._tokenize_words(line) for line in ids_or_text]
            token_rows, word_rows = [t for t, _ in toks], [w for _, w in toks]
            rows = [text.tokens_to_ids(t, self.phon_to_id) for t in token_rows]
            ids = torch.full((len(rows), max(len(r) for r in rows)), self.net_config['padding_idx'], dtype=torch.int64)
            for b, r in enumerate(rows):
                ids[b, :len(r)] = torch.as_tensor(r, dtype=torch.int64)
        else:
            ids = torch.as_tensor(ids_or_text).long().cpu()
            names = {i: p for p, i in self.phon_to_id.items()} if self.phon_to_id else dict(enumerate(text.symbols))
            token_rows = [[names[int(i)] for i in row[:n]] for row, n in zip(ids.tolist(), self._ends_padded(ids).tolist())]
            word_rows = [[' '.join(t[t0:t1]) for t0, t1 in text.word_ranges(t)] for t in token_rows]
        dur = self.align(ids, mel, mel_lens, attn_prior=attn_prior).dur_tgt
        res = self._pending_timings(token_rows, word_rows, dur.round().to(torch.int64)).resolve()
        return res[0] if single else res

    @torch.inference_mode()
    def alignment_score(self, ids_or_text, mel, mel_lens=None, attn_prior='interpolated'):
        """How far a forced alignment can be trusted: align() as above (the prior defaults to the one the checkpoint was trained with), then
        the reference's two alignment losses, forward only (csrc/attn_loss.hip).  -> AlignmentScore(forward_sum [B] float64: the
        forward-sum negative log-likelihood of the row's text given its frames, per token (+inf where the row has fewer frames than
        tokens) -- a recording whose transcript is wrong or truncated lies far from the corpus' bulk; binarization [B] float64: minus the
        mean log of attn_soft along the MAS path; dur_tgt [B, L]; ctc_loss, bin_loss: the batch scalars as AttentionCTCLoss() and
        AttentionBinarizationLoss() report them).  Nothing is read back to the host."""
        ids = self._align_ids(ids_or_text)
        eng = self.aligner()
        soft, logprob, in_lens = eng.attention(ids, mel, attn_prior, mel_lens=mel_lens)
        B, _, T, Lt = soft.shape
        out_lens = torch.full((B,), T, dtype=torch.int64, device=soft.device) if mel_lens is None else \
            torch.as_tensor(mel_lens).to(device=soft.device, dtype=torch.int64)
        dur, hard = _mas(soft, in_lens, out_lens, is_log=False, return_hard=True)
        nll = _forward_sum_loss(logprob, in_lens, out_lens)
        sum_log, count = _binarization_loss(hard, soft)
        forward_sum = nll / in_lens.clamp(min=1).double()
        ctc = (torch.where(torch.isinf(nll), torch.zeros_like(nll), nll) / in_lens.clamp(min=1).double()).mean()
        return AlignmentScore(forward_sum, -sum_log / count, dur, ctc, -sum_log.sum() / count.sum())

    @torch.inference_mode()
    def pitch_track(self, wave, wave_lens=None, mel_len=None, normalize=True):
        """Frame-level pitch of recordings at 22 050 Hz, ready for align(pitch=...): pYIN with the reference's settings (C2..C7, frames of
        1024 every 256 samples; scripts/extract_f0.py:34-39) on the device (csrc/pyin.hip).  wave [B, n] or [n] (+ wave_lens [B], None: n
        samples each) -> [B, 1, T], T = mel_len or 1 + n // 256 (trimmed at the end or zero-padded, as the reference fits the track to its
        mel): f0 in Hz, or with normalize (f0 - pitch_mean) / pitch_std by the checkpoint's statistics (218.14 / 67.24 when it carries
        none, as infer does); unvoiced frames are 0 either way."""
        from utils.pitch import note_to_hz, pyin
        dev = self.device
        if dev.type != 'cuda':
            raise TtsAmdError(f'FastPitch is on {dev}: the MI355X path has no CPU fallback; move the module with .to("cuda")')
        x = torch.as_tensor(wave).to(device=dev, dtype=torch.float32)
        x = x[None] if x.dim() == 1 else x
        f0, flag, _ = pyin(x, fmin=note_to_hz('C2'), fmax=note_to_hz('C7'), frame_length=1024, hop_length=256, fill_na=0.0, lens=wave_lens)
        if normalize:
            mean, std = (218.14, 67.24) if self.pitch_std == 0.0 else (self.pitch_mean, self.pitch_std)
            f0 = torch.where(flag, (f0 - mean) / std, torch.zeros_like(f0))
        if mel_len is not None:
            f0 = torch.nn.functional.pad(f0, (0, int(mel_len) - f0.shape[1]))
        return f0[:, None]

    # ---- FastPitch.infer (models/fastpitch/fastpitch/model.py:351-353) -------------------
    @torch.inference_mode()
    def infer(self, inputs, pace=1.0, dur_tgt=None, pitch_tgt=None, energy_tgt=None, pitch_transform=None,
              max_duration=75, speaker=0, alone=False, pitch_mul=None, pitch_add=None, return_reps=False):
        """`return_reps` (not in the reference): the tuple ends with reps int64 [B, L] on the device, the frames every token got.
        `alone=True` (not in the reference): every row of the batch as if it were the only utterance of the call, i.e. row b ==
        infer(inputs[b:b+1, :len_b]) within fp32 summation order (FastPitchEngine.infer) -- the batch_size = 1 loop as one ragged call.
        Mixed requests (not in the reference): `pace` and `speaker` take a scalar or one value per row; `pitch_mul` / `pitch_add` (scalars
        or per row) are pitch_trf's two numbers given directly -- together with a `pitch_transform` they are refused, since a callable
        cannot be applied per row inside the predictor head."""
        ids = torch.as_tensor(inputs).long()
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.net_config['n_symbols']):
            raise IndexError(f'token id out of range [0, {self.net_config["n_symbols"]}) (nn.Embedding raises here too)')
        if (pitch_mul is not None or pitch_add is not None) and pitch_transform is not None:
            raise ValueError('infer: pitch_mul / pitch_add are given together with a pitch_transform; pass one or the other '
                             '(per-row pitch values cannot go through a callable)')
        mul, add = (1.0 if pitch_mul is None else pitch_mul), (0.0 if pitch_add is None else pitch_add)
        check_line_controls(ids.shape[0], self.net_config['n_speakers'], speed=pace, speaker_id=speaker, pitch_mul=mul, pitch_add=add)
        if not per_row(speaker) and self.net_config['n_speakers'] > 1 and not 0 <= int(speaker) < self.net_config['n_speakers']:
            raise IndexError(f'speaker {speaker} out of range [0, {self.net_config["n_speakers"]})')
        lens = self._ends_padded(ids)
        eng = self.engine()
        if pitch_transform is not None:
            if hasattr(pitch_transform, 'affine'):
                mul, add = pitch_transform.affine
            else:
                # arbitrary callable: run the predictor, transform on the host side, feed back
                _, _, _, pp, _ = eng.infer(ids, pace=pace, dur_tgt=dur_tgt, max_duration=max_duration, speaker=speaker, alone=alone)
                mean, std = (218.14, 67.24) if self.pitch_std == 0.0 else (self.pitch_mean, self.pitch_std)
                pp = pitch_transform(pp, lens.to(pp.device), mean, std)
                out = eng.infer(ids, pace=pace, dur_tgt=dur_tgt, pitch_tgt=pp if pitch_tgt is None else pitch_tgt,
                                energy_tgt=energy_tgt, max_duration=max_duration, speaker=speaker, alone=alone,
                                **({'return_reps': True} if return_reps else {}))
                return (out[0], out[1], out[2], pp, out[4]) + tuple(out[5:])
        return eng.infer(ids, pace=pace, dur_tgt=dur_tgt, pitch_tgt=pitch_tgt, energy_tgt=energy_tgt,
                         pitch_mul=mul, pitch_add=add, max_duration=max_duration, speaker=speaker, alone=alone,
                         **({'return_reps': True} if return_reps else {}))

    def _ends_padded(self, ids):
        """token counts per row; ValueError unless every row is zero-padded at its end"""
        nz = (ids != self.net_config['padding_idx'])
        lens = nz.sum(1)
        if not bool((nz == (torch.arange(ids.shape[1], device=ids.device)[None] < lens[:, None])).all()):
            raise ValueError('ids must be zero-padded at the end of each row (text_collate_fn layout)')
        return lens

    # ---- text -> mel (reference :77-253) -----------------------------------------------
    def _vowelize(self, utterance: str, vowelizer=None):
        """Optional diacritization pre-step (reference :77-87): Buckwalter -> Arabic -> tagger.predict."""
        vowelizer = self.default_vowelizer if vowelizer is None else vowelizer
        if vowelizer is None:
            return utterance
        if vowelizer not in self.vowelizers:
            self.vowelizers[vowelizer] = load_vowelizer(vowelizer, self.config)
        tagger = self.vowelizers[vowelizer]
        if tagger.device != self.device:          # the dict is not a registered submodule, .to() does not reach it
            tagger.to(self.device)
        return tagger.predict(text.buckwalter_to_arabic(utterance))

    def _tokenize_words(self, utterance: str, vowelizer=None):
        """(the line's tokens, its words as text.line_words groups them -- of the line the tokeniser saw, behind the vowelizer)"""
        utterance = self._vowelize(utterance, vowelizer)
        return text.tokens_and_words(utterance, self.arabic_in, append_space=False)          # one pass of the phonetiser for both

    def _tokenize(self, utterance: str, vowelizer=None):
        utterance = self._vowelize(utterance, vowelizer)
        if self.arabic_in:
            return text.arabic_to_tokens(utterance, append_space=False)
        return text.buckwalter_to_tokens(utterance, append_space=False)

    sample_rate, hop = 22050, 256           # of the mel: one frame is `hop` samples of the vocoder's wave

    def _pending_timings(self, token_rows, word_rows, reps, launch=True):
        """the spans of the rows of one infer call, launched behind it (ttsamd.timing.PendingTimings: resolve() is the one copy);
        launch=False: held back until the rows' maps are known (tts_long: the join table)"""
        from ttsamd.timing import PendingTimings
        return PendingTimings(token_rows, word_rows, reps, self.hop, self.sample_rate, launch=launch)

    @staticmethod
    def _ptrf(pitch_mul, pitch_add, pitch_transform):
        if (pitch_mul != 1. or pitch_add != 0.) and pitch_transform is None:
            return pitch_trf(pitch_mul, pitch_add)
        return pitch_transform

    @classmethod
    def _pitch_kw(cls, pitch_mul, pitch_add, pitch_transform):
        """infer()'s pitch arguments: the tagged affine transform for scalars (as before), the two numbers themselves when either is given
        per line -- a custom `pitch_transform` cannot be applied per row and is refused then."""
        if per_row(pitch_mul) or per_row(pitch_add):
            if pitch_transform is not None:
                raise ValueError('per-line pitch_mul / pitch_add cannot be combined with a pitch_transform callable')
            return dict(pitch_mul=pitch_mul, pitch_add=pitch_add)
        return dict(pitch_transform=cls._ptrf(pitch_mul, pitch_add, pitch_transform))

    @torch.inference_mode()
    def ttmel_single(self, utterance: str, speed: float = 1, speaker_id: int = 0, vowelizer=None,
                     pitch_mul: float = 1., pitch_add: float = 0., dur_tgt=None, pitch_tgt=None,
                     energy_tgt=None, pitch_transform=None, max_duration=75, return_timestamps=False):
        """return_timestamps (not in the reference): -> (mel, PendingTimings of the one row)"""
        if return_timestamps:
            tokens, words = self._tokenize_words(utterance, vowelizer=vowelizer)
        else:
            tokens = self._tokenize(utterance, vowelizer=vowelizer)
        ids = torch.LongTensor(text.tokens_to_ids(tokens, self.phon_to_id)).unsqueeze(0)
        mel, *rest = self.infer(ids, pace=speed, speaker=speaker_id, dur_tgt=dur_tgt, pitch_tgt=pitch_tgt,
                                energy_tgt=energy_tgt, pitch_transform=self._ptrf(pitch_mul, pitch_add, pitch_transform),
                                max_duration=max_duration, **({'return_reps': True} if return_timestamps else {}))
        if return_timestamps:
            return mel[0], self._pending_timings([tokens], [words], rest[-1])
        return mel[0]                                                   # [80, T]

    @torch.inference_mode()
    def _ttmel_batch_padded(self, batch, speed, speaker_id, vowelizer, pitch_mul, pitch_add, dur_tgt=None,
                            pitch_tgt=None, energy_tgt=None, pitch_transform=None, max_duration=75, alone=None,
                            return_timestamps=False):
        """alone None: rows as if alone exactly when a control is given per line -- mixed requests are independent requests, and one's
        mel must not depend on which others shared its batch (it equals ttmel_single with its options within fp32 summation order); all
        scalars: the reference's padded-batch arithmetic, as before.  return_timestamps: a fourth result, the PendingTimings of the rows
        in the order of the padded batch (row i is line sort_ids[i])."""
        toks = [self._tokenize_words(line, vowelizer) if return_timestamps else (self._tokenize(line, vowelizer), None) for line in batch]
        batch_ids = [torch.LongTensor(text.tokens_to_ids(t, self.phon_to_id)) for t, _ in toks]
        check_line_controls(len(batch), self.net_config['n_speakers'], speed, speaker_id, pitch_mul, pitch_add)
        ids_pad, lens_sorted, reverse_ids = text_collate_fn(batch_ids)
        # row i of the padded batch is line sort_ids[i]: per-line controls go through the same sort (a scalar stays a scalar)
        sort_ids = reverse_ids.argsort().tolist()
        if alone is None:
            alone = any(per_row(v) for v in (speed, speaker_id, pitch_mul, pitch_add))
        mel, dec_lens, *rest = self.infer(ids_pad, alone=alone, pace=_take(speed, sort_ids), speaker=_take(speaker_id, sort_ids), dur_tgt=dur_tgt,
                                          pitch_tgt=pitch_tgt, energy_tgt=energy_tgt, max_duration=max_duration,
                                          **self._pitch_kw(_take(pitch_mul, sort_ids), _take(pitch_add, sort_ids), pitch_transform),
                                          **({'return_reps': True} if return_timestamps else {}))
        if return_timestamps:
            return mel, dec_lens, reverse_ids, self._pending_timings([toks[j][0] for j in sort_ids], [toks[j][1] for j in sort_ids], rest[-1])
        return mel, dec_lens, reverse_ids

    @torch.inference_mode()
    def ttmel_lines_alone(self, lines: List[str], speed: float = 1, speaker_id: int = 0, vowelizer=None,
                          pitch_mul: float = 1., pitch_add: float = 0., max_duration=75, return_timestamps=False, _launch_spans=True):
        """`[ttmel_single(l) for l in lines]` as ONE ragged FastPitch call (infer(..., alone=True)): (mel [B, 80, T_max], dec_lens int64
        [B]) in HBM, rows in the order of `lines`; mel[b, :, :dec_lens[b]] equals ttmel_single(lines[b]) within fp32 summation order
        (frames past dec_lens[b] are undefined).  What `FastPitch2Wave.tts(list, batch_size=1)` runs per group of lines.  speed,
        speaker_id, pitch_mul and pitch_add: scalars or one value per line (the rows keep the order of `lines`).  return_timestamps: a
        third result, the PendingTimings of the rows (_launch_spans=False: not launched yet, for tts_long, whose maps come with the join)."""
        check_line_controls(len(lines), self.net_config['n_speakers'], speed, speaker_id, pitch_mul, pitch_add)
        toks = [self._tokenize_words(line, vowelizer) if return_timestamps else (self._tokenize(line, vowelizer), None) for line in lines]
        batch_ids = [text.tokens_to_ids(t, self.phon_to_id) for t, _ in toks]
        ids = torch.zeros(len(batch_ids), max(len(i) for i in batch_ids), dtype=torch.int64)
        for b, i in enumerate(batch_ids):
            ids[b, :len(i)] = torch.as_tensor(i, dtype=torch.int64)
        mel, dec_lens, *rest = self.infer(ids, pace=speed, speaker=speaker_id, max_duration=max_duration, alone=True,
                                          **self._pitch_kw(pitch_mul, pitch_add, None), **({'return_reps': True} if return_timestamps else {}))
        if return_timestamps:
            return mel, dec_lens, self._pending_timings([t for t, _ in toks], [w for _, w in toks], rest[-1], launch=_launch_spans)
        return mel, dec_lens

    @torch.inference_mode()
    def ttmel_batch(self, batch: List[str], speed: float = 1, speaker_id: int = 0, vowelizer=None,
                    pitch_mul: float = 1., pitch_add: float = 0., dur_tgt=None, pitch_tgt=None, energy_tgt=None,
                    pitch_transform=None, max_duration=75):
        mel, dec_lens, reverse_ids = self._ttmel_batch_padded(batch, speed, speaker_id, vowelizer, pitch_mul,
                                                              pitch_add, dur_tgt, pitch_tgt, energy_tgt,
                                                              pitch_transform, max_duration)
        lens = dec_lens.tolist()
        return [mel[j, :, :lens[j]] for j in reverse_ids.tolist()]      # original order

    def ttmel(self, text_input: Union[str, List[str]], speed: float = 1, speaker_id: int = 0, batch_size: int = 1,
              vowelizer=None, pitch_mul: float = 1., pitch_add: float = 0.):
        """speed, speaker_id, pitch_mul and pitch_add: scalars, or for a list of lines one value per line (each follows its line)."""
        kw = dict(speed=speed, speaker_id=speaker_id, pitch_mul=pitch_mul, pitch_add=pitch_add)
        if isinstance(text_input, str):
            return self.ttmel_single(text_input, vowelizer=vowelizer, **kw)
        assert isinstance(text_input, list)
        check_line_controls(len(text_input), self.net_config['n_speakers'], **kw)
        if batch_size == 1:
            return [self.ttmel_single(sample, vowelizer=vowelizer, **{k: _at(v, i) for k, v in kw.items()})
                    for i, sample in enumerate(text_input)]
        mel_list = []
        for k in range(0, len(text_input), batch_size):
            idx = range(k, min(k + batch_size, len(text_input)))
            mel_list += self.ttmel_batch(text_input[k:k + batch_size], vowelizer=vowelizer, **{n: _take(v, idx) for n, v in kw.items()})
        return mel_list


class FastPitch2Wave(nn.Module):
    def __init__(self, model_sd_path: str, vocoder_sd: Optional[str] = None, vocoder_config: Optional[str] = None,
                 vowelizer: Optional[str] = None, arabic_in: bool = True, vocoder: Optional[str] = None):
        """vocoder=None: the HiFi-GAN checkpoint (vocoder_sd / vocoder_config, or the basic config's).  vocoder='griffin_lim' (not in the
        reference): no vocoder checkpoint is read; the mel goes through the pseudo-inverse of the filterbank and 32 Griffin-Lim
        iterations on the device (vocoder.griffinlim.GriffinLimVocoder), and tts / tts_single / tts_batch / tts_requests return those
        waves.  `denoise` is then taken as 0 -- the bias denoiser removes HiFi-GAN's own artefact, which these waves do not have --
        while normalize= and limiter= act on the wave as they always do; tts_stream raises ValueError (streaming is out of scope)."""
        super().__init__()
        self.model = FastPitch(model_sd_path, arabic_in=arabic_in, vowelizer=vowelizer)
        if vocoder is not None:
            if vocoder != 'griffin_lim':
                raise ValueError(f"FastPitch2Wave: vocoder={vocoder!r}: None (the HiFi-GAN checkpoint) or 'griffin_lim'")
            from vocoder.griffinlim import NoDenoiser, GriffinLimVocoder
            self.vocoder, self.denoiser = GriffinLimVocoder().eval(), NoDenoiser()
            self.eval()
            return
        if vocoder_sd is None or vocoder_config is None:
            config = get_basic_config()
            vocoder_sd, vocoder_config = config.vocoder_state_path, config.vocoder_config_path
        self.vocoder = load_hifigan(vocoder_sd, vocoder_config)
        self.denoiser = Denoiser(self.vocoder)
        self.eval()

    @property
    def device(self):
        return next(self.parameters()).device

    def forward(self, x):
        return x

    sample_rate = 22050         # of the vocoder's wave: what `normalize` measures the loudness at

    @torch.inference_mode()
    def tts_single(self, text_buckw: str, speed: float = 1, speaker_id: int = 0, denoise: float = 0,
                   vowelizer=None, pitch_mul: float = 1., pitch_add: float = 0., return_mel: bool = False, normalize=None,
                   limiter=False, true_peak=False, return_timestamps=False):
        """return_timestamps (not in the reference): the result ends with the line's timing (ttsamd.timing: words and tokens in samples of
        the returned wave) -- (wave, timing), or (wave, mel, timing) with return_mel."""
        check_normalize(normalize, 1)
        limiter = check_limiter(limiter, normalize)
        check_true_peak(true_peak, normalize, limiter)
        mel_spec = self.model.ttmel_single(text_buckw, speed, speaker_id, vowelizer, pitch_mul=pitch_mul,
                                           pitch_add=pitch_add, **({'return_timestamps': True} if return_timestamps else {}))
        if return_timestamps:
            mel_spec, spans = mel_spec
        wave = self.vocoder(mel_spec)
        if denoise > 0:
            wave = self.denoiser(wave, denoise)
        if normalize is not None:
            wave = level_waves(wave, None, normalize, self.sample_rate, **_lim(limiter, normalize, true_peak))
        out = (wave[0].cpu(), mel_spec) if return_mel else (wave[0].cpu(),)
        if return_timestamps:
            out += (spans.resolve()[0],)              # the one small copy, behind the wave's own
        return out[0] if len(out) == 1 else out

    def _tts_batch_sorted(self, batch, speed, speaker_id, denoise, vowelizer, pitch_mul, pitch_add, normalize=None, limiter=False,
                          true_peak=False, return_timestamps=False):
        """What tts_batch and tts_batch_device share: (wave [B, n_max], n_samples int64 [B], reverse_ids), rows in the collate order (longest
        first; with return_timestamps a fourth result, the PendingTimings of those rows).  Every control is a scalar or one value per line of `batch`; a per-line denoise strength goes through the same sort as
        the lines, and a line whose strength is not > 0 keeps its vocoder output bit for bit.  `normalize` takes the same sort; the
        rows are levelled on the device after the denoiser (ttsamd.engine.level_waves)."""
        check_line_controls(len(batch), self.model.net_config['n_speakers'], denoise=denoise, normalize=normalize, true_peak=true_peak)
        limiter = check_limiter(limiter, normalize)
        mel, dec_lens, reverse_ids, *spans = self.model._ttmel_batch_padded(batch, speed, speaker_id, vowelizer, pitch_mul, pitch_add,
                                                                            **({'return_timestamps': True} if return_timestamps else {}))
        wave = self.vocoder.engine().forward(mel, dec_lens)             # one ragged batched launch sequence
        n = (dec_lens * self.vocoder.engine().hop)
        denoise = _take(denoise, reverse_ids.argsort().tolist())
        if any(d > 0 for d in denoise) if per_row(denoise) else denoise > 0:
            wave = self.denoiser.forward_batch(wave, n, denoise)
        if normalize is not None:
            wave = level_waves(wave, n, _take(normalize, reverse_ids.argsort().tolist()), self.sample_rate,
                               **_lim(limiter, normalize, true_peak))
        return (wave, n, reverse_ids, *spans)

    @torch.inference_mode()
    def tts_batch_device(self, batch: List[str], speed: float = 1, speaker_id: int = 0, denoise: float = 0,
                         vowelizer=None, pitch_mul: float = 1., pitch_add: float = 0., return_mel: bool = False, normalize=None,
                         limiter=False, true_peak=False):
        """`tts_batch` without the device->host copy: (wave [B, n_max] float32, n_samples int64 [B]), both in HBM,
        rows in the order of `batch` (zeros past n_samples[b]).  What the data-parallel gather (ttsamd.dp) and
        any GPU-side consumer take; `tts_batch` is this plus one D2H."""
        wave, n, reverse_ids = self._tts_batch_sorted(batch, speed, speaker_id, denoise, vowelizer, pitch_mul, pitch_add, normalize, limiter,
                                                      true_peak)
        rev = reverse_ids.to(wave.device)
        return wave.index_select(0, rev), n.index_select(0, rev)

    @torch.inference_mode()
    def tts_batch(self, batch: List[str], speed: float = 1, speaker_id: int = 0, denoise: float = 0, vowelizer=None,
                  pitch_mul: float = 1., pitch_add: float = 0., return_mel: bool = False, normalize=None, limiter=False, true_peak=False,
                  return_timestamps=False):
        """return_timestamps (not in the reference): -> (waves, timings), timing i of line i (one more small copy for the batch)"""
        wave, n, reverse_ids, *spans = self._tts_batch_sorted(batch, speed, speaker_id, denoise, vowelizer, pitch_mul, pitch_add, normalize,
                                                              limiter, true_peak, **({'return_timestamps': True} if return_timestamps else {}))
        n = n.tolist()
        # one exact-size D2H per utterance (a padded [B, n_max] copy + per-row clones touches every host page twice)
        # NB the reference silently ignores return_mel here (:347-350); so do we
        waves = [wave[j, :n[j]].cpu() for j in reverse_ids.tolist()]
        if return_timestamps:
            rows = spans[0].resolve()
            return waves, [rows[j] for j in reverse_ids.tolist()]
        return waves

    def tts(self, text_input: Union[str, List[str]], speed: float = 1., denoise: float = 0.005, speaker_id: int = 0,
            batch_size: int = 2, vowelizer=None, pitch_mul: float = 1., pitch_add: float = 0.,
            return_mel: bool = False, normalize=None, limiter=False, true_peak=False,
            return_timestamps: bool = False) -> Union[torch.Tensor, List[torch.Tensor]]:
        """Same contract as the reference (:352-435): str -> Tensor[n_samples] (CPU);
        list -> list of tensors, chunked by `batch_size`.
        Mixed requests (not in the reference): for a list of lines, speed, denoise, speaker_id, pitch_mul and pitch_add each take a scalar
        or a list with one value per line; every value follows its line through the chunking, the collate sort and the length-sorted
        groups of the batch_size = 1 pipeline, and wave i answers line i with its own options.  With a list for speed, speaker_id, pitch_mul or pitch_add the rows of every batch
        are computed as if alone (FastPitch.infer(alone=True)): requests are independent, so wave i equals tts_single(line i, its options)
        within fp32 summation order at every batch_size; all scalars keep the reference's padded-batch arithmetic (a `denoise` list
        on its own does too: the strength has no bearing on FastPitch).
        normalize (not in the reference, whose server ends with wave / max|wave| * 0.99 on the host): the level of every wave, set on
        the device after the denoiser and before the copy to the host -- None (as it comes from the vocoder), 'peak' (x / max|x| * 0.99:
        the bits of utils.audio.peak_normalise on that wave), 'lufs' (ITU-R BS.1770-4 integrated loudness -23 LUFS) or a target in LUFS
        (one gain per wave, capped so that the peak stays <= 0.99), or for a list of lines one such value per line.  It changes
        nothing in front of it: a wave is its un-normalised wave, levelled.
        limiter (False, True or a dict with any of ceiling, attack_ms, hold_ms, max_gain_db; needs a normalize): the lines with 'lufs' or
        a target get the full gain towards it (at most max_gain_db) and the look-ahead limiter holds their peaks at the ceiling
        (utils.audio.limit; include/ttsamd.h states the arithmetic), so the target is reached where the cap would have stopped short of
        it; 'peak' and None lines keep their path.  One setting for the call, not per line.
        true_peak (False or True; needs a normalize): every peak above is the true peak (utils.audio.true_peak: 4x oversampled), so
        0.99 and the limiter's ceiling are true-peak ceilings; one setting for the call.  With no line to level it is a ValueError.
        return_timestamps (not in the reference): where every word and token lies in the wave -- (wave, timing) for a string, (waves,
        timings) for a list, timing i of line i whatever the chunking and sorting did (ttsamd.timing: a dict of sample_rate, words =
        dicts of word, start, end in samples of the returned wave, t0, t1 in seconds, tokens = the word's token range, and tokens =
        dicts of token, start, end; the last token ends where the wave does).  The spans are made on the device from the frames every
        token got (csrc/timing.hip) and cost one small copy per FastPitch call; the denoiser and the level move no sample, so no mark.
        For a string with return_mel: (wave, mel, timing)."""
        kw = dict(speaker_id=speaker_id, speed=speed, denoise=denoise, pitch_mul=pitch_mul, pitch_add=pitch_add)
        if normalize is not None and not (per_row(normalize) and all(v is None for v in normalize)):
            kw['normalize'] = normalize         # (None, or only None: the calls below get exactly the arguments they got before)
        ts = {'return_timestamps': True} if return_timestamps else {}
        if isinstance(text_input, str):
            return self.tts_single(text_input, vowelizer=vowelizer, return_mel=return_mel, **kw, **({'limiter': limiter} if limiter else {}),
                                   **({'true_peak': true_peak} if true_peak else {}), **ts)
        assert isinstance(text_input, list)
        check_line_controls(len(text_input), self.model.net_config['n_speakers'], **dict(kw, normalize=normalize, true_peak=true_peak))
        limiter = check_limiter(limiter, normalize)
        if (len(text_input) > batch_size and not return_mel and self.device.type == 'cuda'
                and os.environ.get('TTSAMD_TTS_PIPELINE', '1') != '0'):
            return self._tts_list_pipelined(text_input, batch_size, vowelizer=vowelizer, return_mel=return_mel, **kw,
                                            **_lim(limiter, normalize, true_peak), **ts)
        if batch_size == 1:
            res = [self.tts_single(sample, vowelizer=vowelizer, return_mel=return_mel, **{k: _at(v, i) for k, v in kw.items()},
                                   **_lim(limiter, _at(normalize, i), true_peak), **ts)
                   for i, sample in enumerate(text_input)]
            if return_timestamps:                   # (wave, [mel,] timing) per line -> (the list as without the flag, the timings)
                return [r[0] if len(r) == 2 else r[:-1] for r in res], [r[-1] for r in res]
            return res
        wav_list, timings = [], []
        for k in range(0, len(text_input), batch_size):
            idx = range(k, min(k + batch_size, len(text_input)))
            got = self.tts_batch(text_input[k:k + batch_size], vowelizer=vowelizer, return_mel=return_mel,
                                 **{n: _take(v, idx) for n, v in kw.items()}, **_lim(limiter, _take(normalize, idx), true_peak), **ts)
            if return_timestamps:
                got, more = got
                timings += more
            wav_list += got
        return (wav_list, timings) if return_timestamps else wav_list

    # the options of one request of tts_requests and what a request that leaves one out gets: tts()'s own defaults
    REQUEST_DEFAULTS = dict(speed=1., denoise=0.005, speaker_id=0, pitch_mul=1., pitch_add=0.)

    def tts_requests(self, requests, batch_size: int = 32, vowelizer=None, limiter=False, true_peak=False, return_timestamps=False):
        """A server's queue in one go: `requests` is a list of dicts with `text` and any of speed, denoise, speaker_id, pitch_mul, pitch_add, normalize
        (the per-request options of the reference's app); returns one wave per request, in request order, from ONE `tts` call with the
        options as per-line lists -- requests with different options share batches instead of one call per distinct option tuple."""
        requests = list(requests)
        for i, r in enumerate(requests):
            extra = set(r) - set(self.REQUEST_DEFAULTS) - {'text', 'normalize'}
            if 'text' not in r or not isinstance(r['text'], str) or extra:
                raise ValueError(f'request {i}: needs a `text` string and takes {sorted(self.REQUEST_DEFAULTS) + ["normalize"]}'
                                 + (f' (got {sorted(extra)})' if extra else ''))
        if not requests:
            return ([], []) if return_timestamps else []
        lists = {k: [r.get(k, d) for r in requests] for k, d in self.REQUEST_DEFAULTS.items()}
        if return_timestamps:                     # -> (waves, timings), as tts does for a list
            lists['return_timestamps'] = True
        if any(r.get('normalize') is not None for r in requests):
            lists['normalize'] = [r.get('normalize') for r in requests]
        if limiter:                               # one setting for the call (a request has no limiter of its own); tts checks it
            lists['limiter'] = limiter
        if true_peak:                             # likewise one setting for the call
            lists['true_peak'] = true_peak
        return self.tts([r['text'] for r in requests], batch_size=batch_size, vowelizer=vowelizer, **lists)

    # ---- paragraph synthesis (not in the reference; text.split_text, ttsamd.join, csrc/join.hip) ----
    @torch.inference_mode()
    def tts_long(self, text_input: Union[str, List[str]], speed: float = 1., denoise: float = 0.005, speaker_id: int = 0, batch_size: int = 32,
                 vowelizer=None, pitch_mul: float = 1., pitch_add: float = 0., pauses=None, max_chars: int = 200, trim_db=40.0,
                 keep_ms: float = 10.0, fade_ms: float = 5.0, normalize=None, limiter=False, true_peak=False, return_segments: bool = False,
                 return_timestamps: bool = False):
        """A paragraph -> ONE wave (CPU tensor [n_samples]).  text_input: a string, or a list of strings taken as paragraphs.  The text is
        cut into segments by text.split_text (sentences; pieces longer than max_chars at clause marks, commas, and last at a space);
        the segments go through FastPitch, the vocoder and the denoiser in groups of batch_size, every row computed as if alone
        (FastPitch.infer(alone=True)), so that a sentence's audio is `tts(sentence)`'s within fp32 summation order whichever others
        shared its group.  A segment is said without the marks that close it (text.spoken_text: a free-standing . , ? ! is a token the
        symbol table does not hold, and `tts` raises KeyError on it as the reference does).  On the device each row is then cut to its speech bounds (librosa.effects.trim's at trim_db, frame 1024 /
        hop 256, widened by keep_ms; trim_db=None: not cut), faded over fade_ms at both edges and joined with the pause of its
        boundary: `pauses`, a dict in ms over the defaults paragraph 700, sentence 350, clause 250, comma 150, forced -fade_ms (an
        overlap-added seam), end 0 -- choices, not measurements.  normalize / limiter / true_peak (as `tts` takes them, one option)
        act on the JOINED wave as one row: one gain for the paragraph.  One copy to the host at the end.  speed, speaker_id,
        pitch_mul, pitch_add, denoise: one value for the whole text.  return_segments: also a list of dicts, one per segment: text,
        boundary, start, end (samples in the returned wave), src_start, src_end (samples in the segment's own wave).  Empty text: ValueError.
        return_timestamps: the result ends with the paragraph's timing (as `tts` describes it), positions in the JOINED wave: every
        segment's tokens are clamped to what the trim kept of it and moved to the segment's place, on the device beside the join
        table, so a token the trim cut away is an empty span at the segment's edge; words carry segment=k, and the pauses are the
        gaps between the segments.  -> (wave, timing), or (wave, segments, timing) with return_segments."""
        from ttsamd.join import join_paragraph, paragraph_pieces, pause_table
        from utils.audio import _trimmer
        pieces, lines = paragraph_pieces(text_input, max_chars)
        table = pause_table(pauses, fade_ms)
        if any(per_row(v) for v in (speed, denoise, speaker_id, pitch_mul, pitch_add, normalize)):
            raise ValueError('tts_long: speed, denoise, speaker_id, pitch_mul, pitch_add and normalize take one value for the whole text')
        check_line_controls(1, self.model.net_config['n_speakers'], [speed], [speaker_id], [pitch_mul], [pitch_add], [denoise], normalize, true_peak)
        limiter = check_limiter(limiter, normalize)
        dev = self.device
        if dev.type != 'cuda':
            raise TtsAmdError(f'FastPitch2Wave is on {dev}: the MI355X path has no CPU fallback; move the module with .to("cuda")')
        eng, groups, spans = self.vocoder.engine(), [], []
        batch_size = max(int(batch_size), 1)
        for k in range(0, len(lines), batch_size):
            mel, dec_lens, *sp = self.model.ttmel_lines_alone(lines[k:k + batch_size], speed, speaker_id, vowelizer, pitch_mul=pitch_mul,
                                                              pitch_add=pitch_add, **({'return_timestamps': True, '_launch_spans': False} if return_timestamps else {}))
            spans += sp
            wave, n = eng.forward(mel, dec_lens), dec_lens * eng.hop
            if denoise > 0:
                wave = self.denoiser.forward_batch(wave, n, denoise)
            groups.append((wave, n))
        wave, rows, *timing = join_paragraph(groups, pieces, table, trim_db, keep_ms, fade_ms, self.sample_rate, _trimmer(dev), normalize, limiter,
                                             true_peak, **({'spans': spans} if return_timestamps else {}))
        out = ((wave, rows) if return_segments else (wave,)) + tuple(timing)
        return out[0] if len(out) == 1 else out

    # ---- streaming synthesis (not in the reference; ttsamd.stream, csrc/stream.hip) ----
    def _streamer(self, chunk_frames, first_chunk_frames, pcm16, max_streams, max_frames, sample_rate=None, encoding=None, limiter=None,
                  true_peak=False):
        """the StreamingVocoder of this model for these settings (its pool and buffers are allocated once and kept)"""
        from ttsamd.stream import StreamingVocoder
        key = (str(self.device), int(chunk_frames), int(first_chunk_frames), bool(pcm16), int(max_streams), int(max_frames),
               None if sample_rate is None else int(sample_rate), encoding, None if limiter is None else tuple(sorted(limiter.items())),
               bool(true_peak))
        if getattr(self, '_stream_key', None) != key:
            self._stream_voc = StreamingVocoder(self.vocoder, self.denoiser, max_streams=max_streams, max_frames=max_frames,
                                                chunk_frames=chunk_frames, first_chunk_frames=first_chunk_frames, pcm16=pcm16,
                                                sample_rate=sample_rate, encoding=encoding, limiter=limiter,
                                                **({'true_peak': True} if true_peak else {}))
            self._stream_key = key
        for sid in self._stream_voc.open_streams:           # a generator that was abandoned half-way
            self._stream_voc.close(sid)
        return self._stream_voc

    def tts_stream(self, text_input: Union[str, List[str]], chunk_frames: int = 64, first_chunk_frames: int = 32, pcm16: bool = False,
                   max_streams: int = 32, max_frames: int = 4096, speed: float = 1., denoise: float = 0.005, speaker_id: int = 0,
                   vowelizer=None, pitch_mul: float = 1., pitch_add: float = 0., sample_rate=None, encoding=None, gain_db=0.0,
                   limiter=False, true_peak=False, meter=False, marks=False):
        """`tts` that hands out audio while it is being made (a generator; one at a time per model).  FastPitch is not autoregressive, so
        the whole mel exists at once; the vocoder then runs over windows of it (ttsamd.stream.StreamingVocoder), the first of
        first_chunk_frames frames, the following of chunk_frames.
        str -> CPU chunks (float32, or int16 PCM with pcm16) whose concatenation has tts_single's 256 T samples and equals it within
        fp32 summation order.
        list of lines (the options as scalars or per-line lists, as in `tts`) -> (i, chunk, last) as the steps produce them: every line
        is a request of its own (the mels come from the rows-as-if-alone path of the mixed requests, so line i's audio is
        tts_single(line i, its options)); at most max_streams lines are open at a time, each step vocodes the next window of all of
        them in one call, a line that ends frees its slot and the next line joins mid-flight.  Line i's chunks arrive in order and
        `last` once.  No peak normalisation: that needs the whole wave.
        sample_rate / encoding ('float32' | 'pcm16' | 'mulaw' | 'alaw'): the chunks leave at that rate and in that encoding (8 000 Hz
        'mulaw' is telephony's G.711: uint8 chunks); put together they are utils.audio.resample of the line's 22 050 Hz samples,
        encoded, bit for bit -- no seam at a chunk border.
        limiter (False, True or a dict with any of ceiling, attack_ms, hold_ms, max_gain_db) and gain_db (a scalar, or one value per
        line): levelling inside the stream.  A stream has no whole-utterance loudness to level by, so it is levelled the way a live chain is: a fixed
        gain, then the look-ahead limiter, at 22 050 Hz in front of the resampler.  The chunks put together are utils.audio.limit of
        the stream's samples in front of the limiter (StreamingVocoder.bypass), bit for bit; against the stream without a limiter
        those differ within fp32 summation order, as its windows are narrower.  gain_db other than 0 without a limiter is a ValueError.
        true_peak (needs a limiter; ValueError without one): the limiter's detector is the true-peak one, and the chunks are the bits
        of utils.audio.limit(true_peak=True).
        meter=True: every chunk that leaves the stream is pushed into a utils.audio.LoudnessMeter at the stream's output rate, on the
        device, so the meter measures what is delivered; the generator then yields (chunk, reading) for a str and (i, chunk, last,
        reading) for a list.  reading: a dict of Python floats, momentary, short_term (-inf before the first 400 ms / 3 s) and
        integrated (of the line so far); on a line's last chunk also loudness_range, max_momentary and max_short_term.  Float chunks
        only: with pcm16 or an encoding other than None / 'float32' it is a ValueError.
        marks=True: every item gets one more element at its end, the list of the word marks (the word dicts of `tts(...,
        return_timestamps=True)`, at the DELIVERED rate: a position s of the 22 050 Hz wave is ceil(n s / o) of the resampler's ratio,
        the rule of the chunk borders) whose start lies in the delivered range of that chunk; a mark at the very end goes with the
        last chunk.  Put together they are the line's timing at that rate.  The spans are made once, when the line's mel is opened;
        nothing runs per chunk on the device.  Works with every encoding, the meter and the limiter."""
        if not hasattr(self.vocoder, 'h'):
            raise ValueError("tts_stream: vocoder='griffin_lim' does not stream (every iteration needs the whole utterance)")
        kw = dict(speed=speed, speaker_id=speaker_id, pitch_mul=pitch_mul, pitch_add=pitch_add)
        limiter = limiter_spec(limiter)
        check_true_peak(true_peak, None, limiter)
        if meter and (pcm16 or encoding not in (None, 'float32')):
            raise ValueError('tts_stream: meter=True measures float chunks: not with pcm16 or an encoding')
        n_lines = 1 if isinstance(text_input, str) else len(text_input)
        gains = row_values(gain_db, n_lines, 'gain_db') if per_row(gain_db) else [gain_db]
        check_finite(gains, 'gain_db')
        if limiter is None and any(float(g) != 0.0 for g in gains):
            raise ValueError('tts_stream: gain_db needs limiter=True (or its settings): a gain alone could clip')
        ts = {'return_timestamps': True} if marks else {}
        if marks:
            from ttsamd.timing import MarkFeeder, delivered_timing
        if isinstance(text_input, str):
            mel = self.model.ttmel_single(text_input, vowelizer=vowelizer, **kw, **ts)
            sv = self._streamer(chunk_frames, first_chunk_frames, pcm16, max_streams, max_frames, sample_rate, encoding, limiter, true_peak)
            if marks:                               # the spans once, when the mel is opened; from here on the marks are host work
                mel, sp = mel
                feed = MarkFeeder(delivered_timing(sp.resolve()[0], sv.sample_rate, self.sample_rate))
            sv.open(mel, denoise, float(gains[0]))
            lm = self._stream_meter(sv, max_streams) if meter else None
            while sv.open_streams:
                for sid, chunk, last in sv.step():
                    item = (chunk.cpu(),) + ((self._meter_reading(lm, sid, chunk, last),) if meter else ())
                    item += (feed.take(chunk.numel(), last),) if marks else ()
                    yield item[0] if len(item) == 1 else item
            return
        lines = list(text_input)
        check_line_controls(len(lines), self.model.net_config['n_speakers'], denoise=denoise, **kw)
        sv = self._streamer(chunk_frames, first_chunk_frames, pcm16, max_streams, max_frames, sample_rate, encoding, limiter, true_peak)
        # FastPitch over the lines in input order, in ragged calls of up to _ALONE_GROUP rows computed as if alone; a group is made when
        # a slot is free and no mel is waiting
        groups, fill, longest = [], [], 0
        for i, line in enumerate(lines):
            if fill and (len(fill) >= self._ALONE_GROUP or (len(fill) + 1) * max(longest, len(line)) > self._ALONE_CHARS):
                groups.append(fill)
                fill, longest = [], 0
            fill.append(i)
            longest = max(longest, len(line))
        if fill:
            groups.append(fill)
        waiting, line_of, feeds = [], {}, {}
        lm = self._stream_meter(sv, max_streams) if meter else None
        while True:
            while sv.free_slots and (waiting or groups):
                if not waiting:
                    pos = groups.pop(0)
                    mel_b, lens_d, *sp = self.model.ttmel_lines_alone([lines[p] for p in pos], _take(speed, pos), _take(speaker_id, pos),
                                                                      vowelizer, pitch_mul=_take(pitch_mul, pos), pitch_add=_take(pitch_add, pos),
                                                                      **ts)
                    waiting = [(p, mel_b[b, :, :t]) for b, (p, t) in enumerate(zip(pos, lens_d.cpu().tolist()))]
                    if marks:                       # this FastPitch call's spans in one copy, beside the lengths'
                        feeds.update({p: MarkFeeder(delivered_timing(t, sv.sample_rate, self.sample_rate)) for p, t in zip(pos, sp[0].resolve())})
                p, mel = waiting.pop(0)
                line_of[sv.open(mel, _at(denoise, p), float(_at(gain_db, p)))] = p
            if not line_of:
                return
            for sid, chunk, last in sv.step():
                i = line_of.pop(sid) if last else line_of[sid]
                item = (i, chunk.cpu(), last) + ((self._meter_reading(lm, sid, chunk, last),) if meter else ())
                yield item + ((feeds.pop(i) if last else feeds[i]).take(chunk.numel(), last),) if marks else item

    def _stream_meter(self, sv, max_streams):
        """the LoudnessMeter of this model's streams at the stream's output rate (made once per rate and pool size), every slot reset"""
        from utils.audio import LoudnessMeter
        key = (str(self.device), int(sv.sample_rate), int(max_streams))
        if getattr(self, '_meter_key', None) != key:
            self._meter = LoudnessMeter(sv.sample_rate, max_streams=max_streams, device=self.device)
            self._meter_key = key
        self._meter.reset(range(max_streams))
        self._meter_free, self._meter_slot = list(range(max_streams)), {}
        return self._meter

    def _meter_reading(self, lm, sid, chunk, last):
        """push the chunk of stream `sid` into its slot of the meter -> the reading as Python floats; behind `last` the slot is free again"""
        if sid not in self._meter_slot:
            self._meter_slot[sid] = self._meter_free.pop(0)
        slot = self._meter_slot[sid]
        reading = {k: float(v[0]) for k, v in lm.push(chunk, slots=[slot]).items()}
        if last:
            res = lm.result([slot])
            reading.update({k: float(res[k][0]) for k in ('integrated', 'loudness_range', 'max_momentary', 'max_short_term')})
            lm.reset([slot])
            self._meter_free.append(self._meter_slot.pop(sid))
        return reading

    # ---- objective evaluation against recordings (not in the reference; ttsamd.engine.ObjectiveEngine, csrc/objective.hip) ----
    @staticmethod
    def _pad_waves(waves, device):
        """list of 1-D waves (tensors / arrays) -> (float32 [B, n_max] on the device, zero-padded; samples int64 [B] on the device)"""
        rows = [torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w).reshape(-1).float() for w in waves]
        n = [int(r.numel()) for r in rows]
        out = torch.zeros(len(rows), max(n), dtype=torch.float32, device=device)
        for b, r in enumerate(rows):
            out[b, :n[b]] = r.to(device)
        return out, torch.tensor(n, dtype=torch.int64).to(device)

    @torch.inference_mode()
    def evaluate(self, text_input: Union[str, List[str]], recordings, teacher_forced: bool = False, align: str = 'dtw', n_coef: int = 13,
                 window=None, **tts_options):
        """Synthesise the lines and score every wave against its recording (a 22 050 Hz wave, already prepared: utils.audio.prepare_recording):
        one dict of Python floats per line with the keys of ttsamd.engine.OBJECTIVE_KEYS (n, mcd, mel_mae, n_vv, f0_rmse_cents, f0_rmse_hz,
        f0_corr, vuv_error) plus frames_pred / frames_ref.  Default: `tts(lines, **tts_options)`, then ObjectiveEngine.score_waves with
        `align` ('dtw' | 'frames'), `n_coef`, `window`.  teacher_forced: the recording's log-mel, its pitch_track and its energy (the L2 norm
        over the bands, as the reference's data_function takes it) go through FastPitch.align, the resulting dur / pitch / energy targets
        go to infer, so the prediction has the recording's durations, and every dict also carries align_forward_sum and align_binarization,
        the two scores of that alignment (FastPitch.alignment_score, with the prior align used: none); tts_options are then speaker_id, denoise (default 0.005) and
        vowelizer."""
        dev = self.device
        if dev.type != 'cuda':
            raise TtsAmdError(f'FastPitch2Wave is on {dev}: the MI355X path has no CPU fallback; move the module with .to("cuda")')
        lines = [text_input] if isinstance(text_input, str) else list(text_input)
        if isinstance(text_input, str) and not (isinstance(recordings, (list, tuple)) and len(recordings) == 1):
            recordings = [recordings]
        if len(recordings) != len(lines) or not lines:
            raise TtsAmdError(f'evaluate: {len(lines)} lines against {len(recordings)} recordings')
        if getattr(self, '_objective', None) is None or self._objective.device != dev:
            self._objective = ObjectiveEngine(device=dev)
        obj = self._objective
        rec, n_rec = self._pad_waves(recordings, dev)
        if not teacher_forced:
            waves = self.tts(lines, **tts_options)
            wave, n = self._pad_waves(waves, dev)
        else:
            extra = set(tts_options) - {'speaker_id', 'denoise', 'vowelizer'}
            if extra:
                raise TtsAmdError(f'evaluate(teacher_forced=True): {sorted(extra)} do not apply (durations, pitch and energy come from the '
                                  'recording); speaker_id, denoise and vowelizer are taken')
            speaker, denoise = tts_options.get('speaker_id', 0), tts_options.get('denoise', 0.005)
            model = self.model
            rows = [text.tokens_to_ids(model._tokenize(line, tts_options.get('vowelizer')), model.phon_to_id) for line in lines]
            ids = torch.full((len(rows), max(len(r) for r in rows)), model.net_config['padding_idx'], dtype=torch.int64)
            for b, r in enumerate(rows):
                ids[b, :len(r)] = torch.as_tensor(r, dtype=torch.int64)
            mel_rec, frames = obj.melspec.forward(rec, n_rec)
            pitch = model.pitch_track(rec, n_rec, mel_len=mel_rec.shape[2])
            tgt = model.align(ids, mel_rec, frames, pitch=pitch, energy=torch.linalg.vector_norm(mel_rec, dim=1), return_attn=True)
            in_lens = (ids != model.net_config['padding_idx']).sum(1).to(dev)
            nll = _forward_sum_loss(tgt.attn_logprob, in_lens, frames)
            sum_log, count = _binarization_loss(tgt.attn_hard, tgt.attn_soft)
            extra_scores = {'align_forward_sum': (nll / in_lens.clamp(min=1).double()).cpu().tolist(), 'align_binarization': (-sum_log / count).cpu().tolist()}
            mel, dec_lens, *_ = model.infer(ids, dur_tgt=tgt.dur_tgt, pitch_tgt=tgt.pitch_tgt, energy_tgt=tgt.energy_tgt, speaker=speaker)
            eng = self.vocoder.engine()
            wave, n = eng.forward(mel, dec_lens), dec_lens * eng.hop
            if denoise > 0:
                wave = self.denoiser.forward_batch(wave, n, denoise)
        score = obj.score_waves(wave, n, rec, n_rec, n_coef=n_coef, align=align, window=window)
        table = torch.stack([score[k] for k in OBJECTIVE_KEYS] + [score['lens_pred'].double(), score['lens_ref'].double()], dim=1).cpu().tolist()
        out = [dict(zip(OBJECTIVE_KEYS + ('frames_pred', 'frames_ref'), row)) for row in table]
        if teacher_forced:
            for b, row in enumerate(out):
                row.update({k: v[b] for k, v in extra_scores.items()})
        return out

    # utterances per vocoder call of the list pipeline: chunks of `batch_size` lines go through FastPitch one by one (a chunk is the
    # reference's padded batch: its results depend on the chunk's composition), their mels are vocoded together
    _VOCODER_GROUP = 16
    # lines per ragged FastPitch + vocoder call of the batch_size = 1 list path (rows computed as if alone: FastPitch.infer(alone=True))
    _ALONE_GROUP = 32
    _ALONE_CHARS = 12288         # ... and at most this many characters x lines per call (lines x the longest line: bounds the padded batch)

    @staticmethod
    def _alone_groups(lengths, group, budget):
        """Index groups over lines SORTED by length (ascending `lengths`): a group is filled until it has `group` lines or
        lines x longest line would pass `budget` -- a list of very long lines must not become one 32-row batch padded to the longest."""
        groups, fill = [], []
        for i, n in enumerate(lengths):
            if fill and (len(fill) >= group or (len(fill) + 1) * n > budget):
                groups.append(fill)
                fill = []
            fill.append(i)
        if fill:
            groups.append(fill)
        return groups

    @torch.inference_mode()
    def _tts_list_pipelined(self, text_input, batch_size, speed, denoise, speaker_id, vowelizer, pitch_mul, pitch_add,
                            return_mel=False, normalize=None, limiter=False, true_peak=False, return_timestamps=False):
        """The list path of `tts` over several chunks, as a three-stage pipeline on three HIP streams: tokenisation + FastPitch
        of the next chunks (host work and ~150 short launches that leave most CUs idle) run under the vocoder + denoiser of the
        previous ones, whose audio is copied to the host on a third stream.  FastPitch sees exactly the chunks of the one-stream
        loop (`ttmel_single` per line for batch_size 1, the padded batch otherwise).  The vocoder is batch-independent -- every
        layer pads each utterance at its own true edge, so a ragged batch equals the per-utterance loop of the reference
        (networks.py:340-345; tests: test_hifigan_ragged_batch_matches_unbatched, test_full_size_bench_workload_properties) -- and
        therefore takes the mels of up to _VOCODER_GROUP utterances in ONE ragged call: at batch_size 1 its launches fill the chip
        like a batch-16 call instead of 100 batch-1 calls (C1, 100 lines: 861 -> see DESIGN.md).  Waves equal the one-stream loop's
        within the vocoder's fp32 summation-order noise (1e-6; a larger batch picks other tiles), lengths exactly.
        batch_size 1 (TTSAMD_TTS_ALONE=0 restores the line-by-line FastPitch calls): FastPitch too is made batch-independent -- batch mode 1
        of the engine computes every row of a ragged batch as if it were alone (ttsamd_fastpitch_set_batch_mode; tests/test_gpu_alone.py) --
        so the lines are sorted by length and go through FastPitch AND the vocoder in balanced groups of up to _ALONE_GROUP similar
        lengths (little padding), waves handed back in input order: 100 launch-bound batch-1 calls of ~1.7 ms become 4 chip-filling ones
        (C1, 100 lines: 500 -> see DESIGN.md); each wave equals its line-by-line result within fp32 summation order, lengths exactly.
        return_timestamps: every FastPitch call also launches its spans on the FastPitch stream (ttsamd.timing.PendingTimings, kept with
        the positions of its rows); they are copied to the host behind the last group's audio -> (waves, timings)."""
        dev = self.device
        if getattr(self, '_pipe_streams', None) is None or self._pipe_streams[0].device != dev:
            self._pipe_streams = tuple(torch.cuda.Stream(dev) for _ in range(3))
        s_fp, s_hg, s_cp = self._pipe_streams
        cur = torch.cuda.current_stream(dev)
        for st in (s_fp, s_hg, s_cp):
            st.wait_stream(cur)
        eng = self.vocoder.engine()
        hop = eng.hop
        out, pending = [], None
        ts, spans = ({'return_timestamps': True} if return_timestamps else {}), []      # spans: (PendingTimings, the positions of its rows)
        group = max(1, self._VOCODER_GROUP // batch_size)           # chunks per vocoder call
        n_in = len(text_input)
        order = list(range(n_in))
        alone_ok = batch_size == 1 and n_in > 1 and os.environ.get('TTSAMD_TTS_ALONE', '1') != '0'
        if alone_ok:
            order.sort(key=lambda i: len(text_input[i]))
            n_groups = (n_in + self._ALONE_GROUP - 1) // self._ALONE_GROUP
            group = (n_in + n_groups - 1) // n_groups
            text_input = [text_input[i] for i in order]
            # per-line controls take the sort of their lines; from here on position p of every list belongs to text_input[p]
            speed, denoise, speaker_id, pitch_mul, pitch_add, normalize = (_take(v, order) for v in (speed, denoise, speaker_id, pitch_mul,
                                                                                                     pitch_add, normalize))

        def flush(item):
            wave, n, done = item
            s_cp.wait_event(done)
            with torch.cuda.stream(s_cp):
                wave.record_stream(s_cp)
                out.extend(wave[j, :n[j]].cpu() for j in range(len(n)))      # blocks the host on THIS group's audio only

        # chunks and groups as POSITIONS into text_input, so that the per-line controls are picked with the lines
        # a per-line FastPitch control: every chunk's rows as if alone (a denoise list alone has no bearing on FastPitch and changes no mel)
        mixed = any(per_row(v) for v in (speed, speaker_id, pitch_mul, pitch_add))
        chunks = [list(range(k, min(k + batch_size, len(text_input)))) for k in range(0, len(text_input), batch_size)]
        groups = [chunks[g0:g0 + group] for g0 in range(0, len(chunks), group)]
        if alone_ok:
            groups = [[chunks[i] for i in g] for g in self._alone_groups([len(text_input[ch[0]]) for ch in chunks], group, self._ALONE_CHARS)]
        for grp in groups:
            mels, lens = [], []                                     # this group's utterances in input order
            pos = [p for ch in grp for p in ch]                     # ... = these positions, in this order
            with torch.cuda.stream(s_fp):
                alone = alone_ok and len(grp) > 1
                if alone:
                    # the batch_size = 1 loop of this group's lines as ONE ragged FastPitch call whose rows are computed as if alone
                    # (ttsamd_fastpitch_set_batch_mode 1); the mel batch and its lengths go to the vocoder as they are
                    mel_b, lens_d, *sp = self.model.ttmel_lines_alone([text_input[p] for p in pos], _take(speed, pos), _take(speaker_id, pos),
                                                                      vowelizer, pitch_mul=_take(pitch_mul, pos), pitch_add=_take(pitch_add, pos),
                                                                      **ts)
                    spans += [(sp[0], pos)] if sp else []
                    lens = lens_d.cpu().tolist()
                for ch in ([] if alone else grp):
                    chunk = [text_input[p] for p in ch]
                    if batch_size == 1:
                        mel = self.model.ttmel_single(chunk[0], _at(speed, ch[0]), _at(speaker_id, ch[0]), vowelizer,
                                                      pitch_mul=_at(pitch_mul, ch[0]), pitch_add=_at(pitch_add, ch[0]), **ts)
                        if return_timestamps:
                            mel, sp = mel
                            spans.append((sp, [ch[0]]))
                        mels.append(mel)
                        lens.append(int(mel.shape[-1]))
                    else:
                        mel, dec_lens, rev, *sp = self.model._ttmel_batch_padded(chunk, _take(speed, ch), _take(speaker_id, ch), vowelizer,
                                                                                 _take(pitch_mul, ch), _take(pitch_add, ch), alone=mixed, **ts)
                        spans += [(sp[0], [ch[j] for j in rev.argsort().tolist()])] if sp else []      # row i of the padded batch is line sort_ids[i]
                        dl = dec_lens.cpu().tolist()                # (FastPitch has synchronised on these lengths already)
                        for j in rev.tolist():
                            mels.append(mel[j, :, :dl[j]])
                            lens.append(int(dl[j]))
                if alone:
                    pass
                elif len(mels) == 1:
                    mel_b = mels[0][None]
                else:
                    mel_b = torch.zeros(len(mels), mels[0].shape[0], max(lens), dtype=mels[0].dtype, device=dev)
                    for i, m in enumerate(mels):
                        mel_b[i, :, :lens[i]] = m
                if not alone:
                    lens_d = torch.tensor(lens, dtype=torch.int64).to(dev, non_blocking=True)
            s_hg.wait_stream(s_fp)
            with torch.cuda.stream(s_hg):
                mel_b.record_stream(s_hg)
                lens_d.record_stream(s_hg)
                wave = eng.forward(mel_b, lens_d)
                n_host = [t * hop for t in lens]
                dn = _take(denoise, pos)                            # rows of `wave` are the positions `pos`, in that order
                if per_row(dn):
                    n_dn = [n for n, d in zip(n_host, dn) if d > 0]
                    if n_dn:
                        wave = self.denoiser.forward_batch(wave, lens_d * hop, dn, nsamples_min=min(n_dn))
                elif dn > 0:
                    wave = self.denoiser.forward_batch(wave, lens_d * hop, dn, nsamples_min=min(n_host))
                if normalize is not None:
                    wave = level_waves(wave, lens_d * hop, _take(normalize, pos), self.sample_rate,
                                       **_lim(limiter, _take(normalize, pos), true_peak))
                done = torch.cuda.Event()
                done.record(s_hg)
            if pending is not None:
                flush(pending)
            pending = (wave, n_host, done)
        if pending is not None:
            flush(pending)
        cur.wait_stream(s_hg)
        cur.wait_stream(s_cp)
        timings = [None] * n_in
        for sp, rows in spans:                                      # s_hg has waited for every FastPitch call, and `cur` for s_hg
            for p, t in zip(rows, sp.resolve()):
                timings[order[p]] = t
        if alone_ok:                                                # back to the order of the input
            res = [None] * n_in
            for pos, w in enumerate(out):
                res[order[pos]] = w
            out = res
        return (out, timings) if return_timestamps else out

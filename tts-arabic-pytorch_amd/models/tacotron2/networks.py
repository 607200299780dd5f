"""Drop-in for the reference's models/tacotron2/networks.py: same classes, signatures, defaults and
return conventions, with the arithmetic routed to the HIP engines.

  Tacotron2      (reference :71-253)  checkpoint -> .infer/.ttmel/.ttmel_single/.ttmel_batch
  Tacotron2Wave  (reference :256-426) + HiFi-GAN + denoiser -> .tts/.tts_single/.tts_batch
  text_collate_fn (:16-35), needs_postprocessing (:38-40), truncate_mel (:43-48), resize_mel (:51-66)

Differences, host-side only: `tts_batch` vocodes the (truncated / resized, hence ragged) mels in ONE
ragged HiFi-GAN call instead of a per-mel loop (:340-346) — identical results, every layer pads at the
true utterance edge — `vowelizer=` runs the Shakkelha / Shakkala taggers of models/diacritizers on the HIP tagger engine.
Not in the reference: `Tacotron2Wave.tts_stream` (audio in chunks while the decoder is still running) with `cut_bound`, truncate_mel's
cut in causal form.
"""
from typing import List, Optional, Union

import torch
import torch.nn as nn

import text
from text.symbols import EOS_TOKENS, SEPARATOR_TOKEN
from utils import get_basic_config
from models.diacritizers import load_vowelizer
from vocoder import load_hifigan
from ttsamd.engine import check_limiter, check_normalize, check_true_peak, level_waves, per_row
from vocoder.hifigan.denoiser import Denoiser

from .tacotron2_ms import Tacotron2MS


def text_collate_fn(batch: List[torch.Tensor]):
    """Sort by length (descending), zero-pad; returns (ids_pad, lens_sorted, reverse_ids)."""
    lens_sorted, sort_ids = torch.sort(torch.LongTensor([len(x) for x in batch]), descending=True)
    ids_pad = torch.zeros(len(batch), int(lens_sorted[0]), dtype=torch.long)
    for i, j in enumerate(sort_ids):
        ids_pad[i, :batch[j].size(0)] = batch[j]
    return ids_pad, lens_sorted, sort_ids.argsort()


_OPEN_ENDINGS = frozenset(['a', 'i', 'u', 'aa', 'ii', 'uu', 'n', 'm', 'h'])


def needs_postprocessing(token: str):
    """True when the utterance ends in a phoneme the model tends to drag out (everything but
    short/long vowels and n, m, h): a separator is inserted and the mel cut at its attention peak."""
    return token not in _OPEN_ENDINGS


def truncate_mel(mel_spec: torch.Tensor, ps_end):
    """Cut [F, T] at the first frame whose attention on the inserted separator reaches 80 % of its
    maximum, then repeat the last kept frame 3 times (reference :43-48)."""
    hit = (ps_end >= 0.8 * ps_end.max()).nonzero()
    n_end = int(hit[0])
    mel_cut = mel_spec[:, :n_end]
    return torch.nn.functional.pad(mel_cut, (0, 3), mode='replicate')


def cut_bound(ps_seen, state=None):
    """truncate_mel's cut in causal form.  The cut n_end = first t with ps[t] >= 0.8 * max(ps) needs the whole column; with
    m_s = max(ps[:s]) and c_s = the first t < s with ps[t] >= 0.8 * m_s: c_s never decreases (the threshold only rises, so a frame
    that failed it keeps failing), c_s <= n_end (no frame before c_s reaches 0.8 * m_s, let alone 0.8 * max(ps)) and c_T = n_end.
    Frames below c_s can therefore leave before the utterance is over.  ps_seen: the NEW values of the separator column
    (1-D float32 tensor), state: what the previous call returned (None at the start) -> (c_s, state).  The device twin is
    taco_cut_kernel (csrc/tacotron2.hip).  How far c_s runs behind s depends on the checkpoint: one tiny early value of the column
    holds it at that frame until the attention reaches the separator, i.e. until the end.  On a trained checkpoint the lag has not
    been measured; the synthetic test checkpoint shows both cases (profiles/r36/NOTES.md: one line's bound is final 8 steps behind its
    cut, another's sits at frame 1 until the cut at frame 35 has been decoded)."""
    ps_seen = torch.as_tensor(ps_seen, dtype=torch.float32).reshape(-1).cpu()
    m, c, ps = state if state is not None else (None, 0, ps_seen[:0])
    ps = torch.cat([ps, ps_seen])
    if ps.numel() == 0:
        return 0, (m, c, ps)
    m = ps_seen.max() if m is None else (torch.maximum(m, ps_seen.max()) if ps_seen.numel() else m)
    thr = 0.8 * m
    while c < ps.numel() and not bool(ps[c] >= thr):
        c += 1
    return c, (m, c, ps)


def stream_truncate_mel(mel_spec: torch.Tensor, ps_end, halo: int = 0, block: int = 8):
    """Host model of what Tacotron2Wave.tts_stream puts into the vocoder stream for one row with a cut: the frames arrive in blocks of
    `block`; after each, the frames below min(c_s, s - halo) are appended; at the end what remains up to n_end, then frame n_end - 1
    three more times.  -> (the mel put together, [appended-so-far after each block]): the mel is truncate_mel's, frame for frame."""
    T = int(mel_spec.shape[-1])
    out, sent, state, trace = [], 0, None, []
    for s0 in range(0, T, block):
        s1 = min(s0 + block, T)
        c, state = cut_bound(ps_end[s0:s1], state)
        final = min(c, s1 if s1 == T else max(s1 - halo, 0))
        if final > sent:
            out.append(mel_spec[:, sent:final])
            sent = final
        trace.append(sent)
    n_end = state[1] if state is not None else 0
    assert sent == n_end, (sent, n_end)
    if n_end == 0:
        return truncate_mel(mel_spec, ps_end), trace            # (what the one-shot path does with an empty cut)
    out += [mel_spec[:, n_end - 1:n_end]] * 3
    return torch.cat(out, dim=-1), trace


def resize_mel(mel: torch.Tensor, rate: Union[int, float] = 1.0, mode: str = 'bicubic'):
    """[F, T] -> [F, int(T / rate)] by image interpolation (reference :51-66)."""
    n_f, n_t = mel.shape[-2:]
    n_t_new = int(1 / rate * n_t)
    if n_t == n_t_new:
        return mel
    return torch.nn.functional.interpolate(mel[None, None, ...], (n_f, n_t_new), mode=mode)[0, 0]


class Tacotron2(Tacotron2MS):
    def __init__(self, checkpoint: str = None, n_symbol: int = 40, decoder_max_step: int = 3000,
                 arabic_in: bool = True, vowelizer: Optional[str] = None, **kwargs):
        super().__init__(n_symbol=n_symbol, decoder_max_step=decoder_max_step, **kwargs)
        self.n_eos = len(EOS_TOKENS)
        self.arabic_in = arabic_in
        state_dicts = None
        if checkpoint is not None:
            state_dicts = torch.load(checkpoint, map_location='cpu')
            self.load_state_dict(state_dicts['model'])
        self.config = get_basic_config()
        self.vowelizers = {}
        if vowelizer is not None:
            self.vowelizers[vowelizer] = load_vowelizer(vowelizer, self.config)
        self.default_vowelizer = vowelizer
        self.phon_to_id = None
        if state_dicts is not None and 'symbols' in state_dicts:
            self.phon_to_id = {phon: i for i, phon in enumerate(state_dicts['symbols'])}
        self.eval()

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

    def _tokenize(self, utterance: str, vowelizer=None):
        utterance = self._vowelize(utterance, vowelizer)
        if self.arabic_in:
            return text.arabic_to_tokens(utterance)
        return text.buckwalter_to_tokens(utterance)

    def _tokens_for(self, utterance, vowelizer, postprocess_mel, with_words=False):
        """tokens (+ the extra separator before the EOS tokens when the ending needs the cut); with_words: a third result, the line's
        words as text.line_words groups them (of the line the tokeniser saw)"""
        if with_words:                                                   # _tokenize's two steps, one pass of the phonetiser for tokens and words
            tokens, words = text.tokens_and_words(self._vowelize(utterance, vowelizer), self.arabic_in)
        else:
            tokens = self._tokenize(utterance, vowelizer=vowelizer)
        process_mel = False
        if postprocess_mel and needs_postprocessing(tokens[-self.n_eos - 1]):
            tokens.insert(-self.n_eos, SEPARATOR_TOKEN)
            process_mel = True
        return (tokens, process_mel, words) if with_words else (tokens, process_mel)

    # ---- timestamps (not in the reference; ttsamd.timing, csrc/timing.hip) ----
    sample_rate, hop = 22050, 256           # of the mel: one frame is `hop` samples of the vocoder's wave

    @staticmethod
    def attention_durations(alignments, in_lens, out_lens):
        """The frames every token got: the monotonic path through the decoder's attention, ttsamd.engine.mas on log(max(alignments, tiny))
        -- the clamp and the log taken on the device, so that an exact zero puts no -inf into the search.  alignments [B, T, L] on the
        device -> (dur fp32 [B, L], the log-attention tensor the search ran on)."""
        from ttsamd.engine import mas
        log_attn = torch.log(torch.clamp(alignments.float(), min=torch.finfo(torch.float32).tiny)).contiguous()
        dur, _ = mas(log_attn, in_lens, out_lens, is_log=True, return_hard=False)
        return dur, log_attn

    def _pending_timings(self, token_rows, word_rows, alignments, in_lens, out_lens, shapes, launch=True):
        """the spans of the rows of one infer call (ttsamd.timing.PendingTimings: resolve() is the one copy).  shapes: per row (n_end or
        None, n_t, n_t_new): where truncate_mel cut the mel, and the frame counts in front of and behind resize_mel.  A position is
        clamped to n_end hop (the three replicated closing frames belong to no token) and counted at n_t_new / n_t of the rate: the
        sampling grid of the resize, without bicubic's half-pixel offset -- a choice."""
        from ttsamd.timing import PendingTimings
        dev = alignments.device
        dur, _ = self.attention_durations(alignments, torch.as_tensor(in_lens), torch.as_tensor(out_lens))
        maps = torch.tensor([(0, (1 << 63) - 1 if n_end is None else n_end * self.hop, 0, max(n_new, 1), max(n_t, 1))
                             for n_end, n_t, n_new in shapes], dtype=torch.int64).to(dev)
        # launch=False (tts_long): held back until the join's map is known; it then comes on top of these in a second launch
        return PendingTimings(token_rows, word_rows, dur.round().to(torch.int64), self.hop, self.sample_rate, row_maps=maps, launch=launch)

    @torch.inference_mode()
    def ttmel_single(self, utterance: str, speaker_id: int = 0, speed: Union[int, float, None] = None,
                     vowelizer=None, postprocess_mel: bool = True, return_timestamps=False):
        """return_timestamps (not in the reference): -> (mel, PendingTimings of the one row)"""
        tokens, process_mel, *words = self._tokens_for(utterance, vowelizer, postprocess_mel, **({'with_words': True} if return_timestamps else {}))
        ids_batch = torch.LongTensor(text.tokens_to_ids(tokens, self.phon_to_id)).unsqueeze(0)
        sid = torch.LongTensor([speaker_id])
        mel_spec, _, alignments = self.infer(ids_batch, sid)
        mel_spec = mel_spec[0]
        n_end = None
        if process_mel:
            mel_spec = truncate_mel(mel_spec, alignments[0, :, -self.n_eos - 1])
            n_end = int(mel_spec.shape[-1]) - 3
        n_t = int(mel_spec.shape[-1])
        if speed is not None:
            mel_spec = resize_mel(mel_spec, rate=speed)
        if return_timestamps:
            return mel_spec, self._pending_timings([tokens], words, alignments, [len(tokens)], [alignments.shape[1]],
                                                   [(n_end, n_t, int(mel_spec.shape[-1]))])
        return mel_spec                                                  # [80, T]

    @torch.inference_mode()
    def ttmel_batch(self, batch: List[str], speaker_id: int = 0, speed: Union[int, float, None] = None,
                    vowelizer=None, postprocess_mel: bool = True, return_timestamps=False, _launch_spans=True):
        """return_timestamps (not in the reference): -> (mels, PendingTimings of the rows in the order of `batch`; _launch_spans=False: not
        launched yet, for tts_long, whose maps come with the join)"""
        prepared = [self._tokens_for(line, vowelizer, postprocess_mel, **({'with_words': True} if return_timestamps else {})) for line in batch]
        batch_ids = [torch.LongTensor(text.tokens_to_ids(p[0], self.phon_to_id)) for p in prepared]
        ids_pad, lens_sorted, reverse_ids = text_collate_fn(batch_ids)
        sids = lens_sorted * 0 + speaker_id
        mel_post, mel_lens, alignments = self.infer(ids_pad, sids, lens_sorted)
        mel_lens, in_lens = mel_lens.tolist(), lens_sorted.tolist()
        mel_list, shapes = [], []
        for i, j in enumerate(reverse_ids.tolist()):
            mel = mel_post[j, :, :mel_lens[j]]
            n_end = None
            if prepared[i][1]:
                mel = truncate_mel(mel, alignments[j, :mel_lens[j], in_lens[j] - self.n_eos - 1])
                n_end = int(mel.shape[-1]) - 3
            n_t = int(mel.shape[-1])
            if speed is not None:
                mel = resize_mel(mel, rate=speed)
            shapes.append((n_end, n_t, int(mel.shape[-1])))
            mel_list.append(mel)
        if return_timestamps:
            rows = reverse_ids.tolist()                                  # line i is row rows[i] of the padded batch
            return mel_list, self._pending_timings([p[0] for p in prepared], [p[2] for p in prepared], alignments.index_select(
                0, reverse_ids.to(alignments.device)), [in_lens[j] for j in rows], [mel_lens[j] for j in rows], shapes,
                launch=_launch_spans)
        return mel_list

    def ttmel(self, text_input: Union[str, List[str]], speaker_id: int = 0, speed: Union[int, float, None] = None,
              batch_size: int = 8, vowelizer=None, postprocess_mel: bool = True):
        args = (speaker_id, speed, vowelizer, postprocess_mel)
        if isinstance(text_input, str):
            return self.ttmel_single(text_input, *args)
        assert isinstance(text_input, list)
        if batch_size == 1:
            return [self.ttmel_single(sample, *args) for sample in text_input]
        mel_list = []
        for k in range(0, len(text_input), batch_size):
            mel_list += self.ttmel_batch(text_input[k:k + batch_size], *args)
        return mel_list


def _lim(limiter, normalize, true_peak=False):
    """the `limiter` and `true_peak` keywords for a call that gets `normalize`: only where they are asked for and a line of that call asks
    for a level"""
    if not any(v is not None for v in (normalize if per_row(normalize) else [normalize])):
        return {}
    return dict({'limiter': limiter} if limiter else {}, **({'true_peak': True} if true_peak else {}))


class Tacotron2Wave(nn.Module):
    def __init__(self, model_sd_path: str, vocoder_sd: Optional[str] = None, vocoder_config: Optional[str] = None,
                 vowelizer: Optional[str] = None, arabic_in: bool = True, n_symbol: int = 40, vocoder: Optional[str] = None):
        """vocoder=None: the HiFi-GAN checkpoint.  vocoder='griffin_lim' (not in the reference): no vocoder checkpoint is read, the
        waves of tts / tts_single / tts_batch come from vocoder.griffinlim.GriffinLimVocoder (pseudo-inverse of the filterbank, 32
        Griffin-Lim iterations on the device); `denoise` is then taken as 0 (the bias denoiser removes HiFi-GAN's own artefact),
        normalize= / limiter= act on the wave as always, and tts_stream raises ValueError (streaming is out of scope)."""
        super().__init__()
        self.model = Tacotron2(model_sd_path, n_symbol=n_symbol, arabic_in=arabic_in, vowelizer=vowelizer)
        if vocoder is not None:
            if vocoder != 'griffin_lim':
                raise ValueError(f"Tacotron2Wave: vocoder={vocoder!r}: None (the HiFi-GAN checkpoint) or 'griffin_lim'")
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
    def tts_single(self, text_input: str, speed: Union[int, float, None] = None, speaker_id: int = 0,
                   denoise: float = 0, vowelizer=None, postprocess_mel: bool = True, return_mel: bool = False, normalize=None,
                   limiter=False, true_peak=False, return_timestamps=False):
        """return_timestamps (not in the reference): the result ends with the line's timing (ttsamd.timing), as FastPitch2Wave.tts
        describes it; the durations are the monotonic path through the decoder's attention (Tacotron2.attention_durations), cut where
        truncate_mel cut and scaled where resize_mel stretched."""
        check_normalize(normalize, 1)
        limiter = check_limiter(limiter, normalize)
        check_true_peak(true_peak, normalize, limiter)
        mel_spec = self.model.ttmel_single(text_input, speaker_id, speed, vowelizer, postprocess_mel,
                                           **({'return_timestamps': True} if return_timestamps else {}))
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

    @torch.inference_mode()
    def tts_batch(self, batch: List[str], speed: Union[int, float, None] = None, denoise: float = 0,
                  speaker_id: int = 0, vowelizer=None, postprocess_mel: bool = True, return_mel: bool = False, normalize=None,
                  limiter=False, true_peak=False, return_timestamps=False):
        """return_timestamps (not in the reference): -> (waves, timings), timing i of line i (one more small copy for the batch)"""
        check_normalize(normalize, len(batch))
        limiter = check_limiter(limiter, normalize)
        check_true_peak(true_peak, normalize, limiter)
        mel_list = self.model.ttmel_batch(batch, speaker_id, speed, vowelizer, postprocess_mel,
                                          **({'return_timestamps': True} if return_timestamps else {}))
        if return_timestamps:
            mel_list, spans = mel_list
        eng = self.vocoder.engine()
        lens_host = [m.shape[-1] for m in mel_list]
        lens = torch.tensor(lens_host, dtype=torch.int64, device=mel_list[0].device)
        mel = torch.zeros(len(mel_list), mel_list[0].shape[0], max(lens_host), device=lens.device)
        for i, m in enumerate(mel_list):
            mel[i, :, :m.shape[-1]] = m
        wave = eng.forward(mel, lens)                                    # one ragged batched launch sequence
        n = [t * eng.hop for t in lens_host]
        if denoise > 0:
            wave = self.denoiser.forward_batch(wave, lens * eng.hop, denoise, nsamples_min=min(n))
        if normalize is not None:
            wave = level_waves(wave, lens * eng.hop, normalize, self.sample_rate, **_lim(limiter, normalize, true_peak))    # on the device, after the denoiser
        # one exact-size D2H per utterance (a padded [B, n_max] copy + per-row clones touches every host page twice)
        # NB the reference silently ignores return_mel here (:348-351); so do we
        waves = [wave[i, :n[i]].cpu() for i in range(len(mel_list))]
        return (waves, spans.resolve()) if return_timestamps else waves

    def _tts_batch_device(self, batch, speed, denoise, speaker_id, vowelizer, postprocess_mel, spans=None):
        """tts_batch up to the denoiser, without the copies to the host: (wave [B, n_max] fp32, samples int64 [B]), both on the device,
        rows in the order of `batch`.  What tts_long joins.  spans: a list that gets the rows' PendingTimings, not launched yet."""
        mel_list = self.model.ttmel_batch(batch, speaker_id, speed, vowelizer, postprocess_mel,
                                          **({'return_timestamps': True, '_launch_spans': False} if spans is not None else {}))
        if spans is not None:
            mel_list, sp = mel_list
            spans.append(sp)
        eng = self.vocoder.engine()
        lens_host = [m.shape[-1] for m in mel_list]
        lens = torch.tensor(lens_host, dtype=torch.int64, device=mel_list[0].device)
        mel = torch.zeros(len(mel_list), mel_list[0].shape[0], max(lens_host), device=lens.device)
        for i, m in enumerate(mel_list):
            mel[i, :, :m.shape[-1]] = m
        wave = eng.forward(mel, lens)
        if denoise > 0:
            wave = self.denoiser.forward_batch(wave, lens * eng.hop, denoise, nsamples_min=min(lens_host) * eng.hop)
        return wave, lens * eng.hop

    @torch.inference_mode()
    def tts_long(self, text_input: Union[str, List[str]], speed: Union[int, float, None] = None, denoise: float = 0.005, speaker_id: int = 0,
                 batch_size: int = 32, vowelizer=None, postprocess_mel: bool = True, pauses=None, max_chars: int = 200, trim_db=40.0,
                 keep_ms: float = 10.0, fade_ms: float = 5.0, normalize=None, limiter=False, true_peak=False, return_segments: bool = False,
                 return_timestamps: bool = False):
        """return_timestamps: the result ends with the paragraph's timing, positions in the JOINED wave, as FastPitch2Wave.tts_long hands
        it out: a segment's marks are first put into its own wave (the end-of-utterance cut, the ratio of a `speed`), then clamped to
        what the trim kept and moved to its place -- two launches per group, because the two maps do not compose into one.
        A paragraph -> ONE wave (CPU tensor [n_samples]), as FastPitch2Wave.tts_long: the text (a string, or a list of strings taken as
        paragraphs) is cut by text.split_text, the segments -- each said without the marks that close it, text.spoken_text -- go through
        the batch path in groups of batch_size (the rows of a group are decoded together, as tts_batch decodes them), and on the device every row is cut to its speech bounds (trim_db, keep_ms),
        faded over fade_ms and joined with the pause of its boundary (`pauses` in ms over paragraph 700, sentence 350, clause 250,
        comma 150, forced -fade_ms, end 0).  speed: tts's own (None, or the rate resize_mel stretches every mel by).  normalize /
        limiter / true_peak act on the JOINED wave as one row; one copy to the host.  return_segments: also one dict per segment
        (text, boundary, start, end, src_start, src_end).  Empty text: ValueError."""
        from ttsamd.join import join_paragraph, paragraph_pieces, pause_table
        from utils.audio import _trimmer
        pieces, lines = paragraph_pieces(text_input, max_chars)
        table = pause_table(pauses, fade_ms)
        if per_row(normalize):
            raise ValueError('tts_long: normalize takes one option for the whole text')
        check_normalize(normalize, 1)
        limiter = check_limiter(limiter, normalize)
        check_true_peak(true_peak, normalize, limiter)
        batch_size = max(int(batch_size), 1)
        spans = [] if return_timestamps else None
        groups = [self._tts_batch_device(lines[k:k + batch_size], speed, denoise, speaker_id, vowelizer, postprocess_mel,
                                         **({'spans': spans} if return_timestamps else {}))
                  for k in range(0, len(lines), batch_size)]
        wave, rows, *timing = join_paragraph(groups, pieces, table, trim_db, keep_ms, fade_ms, self.sample_rate, _trimmer(groups[0][0].device),
                                             normalize, limiter, true_peak, **({'spans': spans} if return_timestamps else {}))
        out = ((wave, rows) if return_segments else (wave,)) + tuple(timing)
        return out[0] if len(out) == 1 else out

    def _streamer(self, chunk_frames, first_chunk_frames, pcm16, max_streams, max_frames, sample_rate, encoding, limiter, true_peak):
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
                   denoise: float = 0.005, speaker_id: int = 0, batch_size: int = 8, vowelizer=None, postprocess_mel: bool = True,
                   sample_rate=None, encoding=None, gain_db=0.0, limiter=False, true_peak=False, max_frames: int = 4096,
                   speed: Union[int, float, None] = None, meter=False, marks=False):
        """`tts` that hands out audio while the decoder is still running (a generator; one at a time per model).  Tacotron2 makes its
        mel frame by frame: the decoder runs in advances (Tacotron2Engine.stream), the postnet over windows of the frames that are
        final, and every row of the batch is a growing stream of the chunked vocoder (StreamingVocoder.open_growing).
        str -> CPU chunks whose concatenation has tts_single's samples and equals them within fp32 summation order (the vocoder's
        windows); list -> (i, chunk, last) as the steps produce them: the lines go through Tacotron2 in batches of batch_size, sorted
        by text_collate_fn, line i's audio is tts(list, batch_size)[i]'s, its chunks arrive in order and `last` once; the rows of a
        finished batch drain while the next batch decodes.  Each turn of the loop runs one advance, one postnet window, the appends and
        finishes, and one vocoder step.  The first advance is first_chunk_frames + the look-ahead the chunk planner asks for
        (max(chunk_frames // 2, the right halo of vocoder, denoiser, resampler and limiter)) + the postnet's halo, rounded up to 8
        steps; later ones are chunk_frames rounded up to 8.  The cooperative decoder holds every CU while it runs, so decoder and
        vocoder alternate; they do not overlap.
        postprocess_mel: the end-of-utterance cut in causal form (cut_bound): frames below the bound -- and at least the postnet's
        halo behind the decoder -- enter the vocoder while the row is still being decoded; at the row's end follow the rest up to the
        cut and the three repeated frames, so the streamed mel is truncate_mel's frame for frame.  How early audio leaves a row with
        a cut depends on how far the bound runs behind the decoder on the checkpoint (cut_bound).
        pcm16, sample_rate, encoding, gain_db (a scalar, or one value per line), limiter, true_peak: as FastPitch2Wave.tts_stream.
        speed other than None / 1 (resize_mel needs the total length), meter and marks are ValueErrors; there is no peak normalisation (it
        needs the whole wave).  Tacotron2.dropout_seed applies per batch as in `infer`.  `stream_sessions` maps each line to the
        decoder session of its batch (its steps_done / ended at the time of a yield)."""
        from ttsamd.engine import check_finite, check_true_peak, limiter_spec, row_values
        if not hasattr(self.vocoder, 'h'):
            raise ValueError("tts_stream: vocoder='griffin_lim' does not stream (every iteration needs the whole utterance)")
        if speed is not None and float(speed) != 1.0:
            raise ValueError('tts_stream: speed is not supported in the stream (resize_mel needs the total length): use tts')
        if meter:
            raise ValueError('tts_stream: meter is not supported for Tacotron2 streams')
        if marks:
            raise ValueError('tts_stream: marks are not supported for Tacotron2 streams (the attention path is known only at the end '
                             'of the utterance): use tts(..., return_timestamps=True)')
        limiter = limiter_spec(limiter)
        check_true_peak(true_peak, None, limiter)
        single = isinstance(text_input, str)
        lines = [text_input] if single else list(text_input)
        gains = row_values(gain_db, len(lines), 'gain_db') if per_row(gain_db) else [gain_db] * len(lines)
        check_finite(gains, 'gain_db')
        if limiter is None and any(float(g) != 0.0 for g in gains):
            raise ValueError('tts_stream: gain_db needs limiter=True (or its settings): a gain alone could clip')
        batch_size = max(int(batch_size), 1)
        gen = self._tts_stream(lines, [float(g) for g in gains], single, int(chunk_frames), int(first_chunk_frames), pcm16, float(denoise),
                               speaker_id, batch_size, vowelizer, postprocess_mel, sample_rate, encoding, limiter, true_peak, int(max_frames))
        return gen

    @torch.inference_mode()
    def _tts_stream(self, lines, gains, single, chunk_frames, first_chunk_frames, pcm16, denoise, speaker_id, batch_size, vowelizer,
                    postprocess_mel, sample_rate, encoding, limiter, true_peak, max_frames):
        model = self.model
        sv = self._streamer(chunk_frames, first_chunk_frames, pcm16, 2 * batch_size, max_frames, sample_rate, encoding, limiter, true_peak)
        eng = model.engine()
        up8 = lambda n: -(-int(n) // 8) * 8                                                              # noqa: E731
        first_steps = up8(sv.first_release_frames(denoise) + eng.postnet_halo)
        later_steps = up8(chunk_frames)
        whole_rows = single or batch_size == 1          # tts_single's rule: the row is as long as the decode
        self.stream_sessions = {}
        todo = list(range(len(lines)))
        sess, rows, line_of = None, [], {}              # rows of the session: [line, batch row, sid, frames sent, cut?]
        while True:
            if sess is None and todo and sv.free_slots >= min(batch_size, len(todo)):
                idx, todo = todo[:batch_size], todo[batch_size:]
                prepared = [model._tokens_for(lines[i], vowelizer, postprocess_mel) for i in idx]
                ids = [torch.LongTensor(text.tokens_to_ids(tokens, model.phon_to_id)) for tokens, _ in prepared]
                ids_pad, lens_sorted, reverse_ids = text_collate_fn(ids)
                in_lens = lens_sorted.tolist()
                cols = [-1] * len(idx)
                for k, j in enumerate(reverse_ids.tolist()):
                    if prepared[k][1]:
                        cols[j] = in_lens[j] - model.n_eos - 1
                sess = eng.stream(ids_pad, lens_sorted * 0 + speaker_id, lens_sorted, max_step=model.decoder_max_step,
                                  dropout_seed=model.dropout_seed, max_chunk_steps=max(first_steps, later_steps), cut_columns=cols,
                                  rows_to_batch_end=whole_rows)
                rows = []
                for k, j in enumerate(reverse_ids.tolist()):
                    sid = sv.open_growing(denoise, gains[idx[k]])
                    line_of[sid] = idx[k]
                    self.stream_sessions[idx[k]] = sess
                    rows.append([idx[k], j, sid, 0, cols[j] >= 0])
                post_pos = 0
            if sess is not None:
                sess.advance(first_steps if sess.n_advances == 0 else later_steps)
                if sess.final_frames > post_pos:
                    sess.postnet(post_pos, sess.final_frames)
                    post_pos = sess.final_frames
                mel_post = sess.mel_post
                for row in rows:
                    i, j, sid, sent, cut = row
                    if sid is None:
                        continue
                    final, row_ended, n_end, row_len = sess.rows[j]
                    if final > sent:
                        sv.append(sid, mel_post[j, :, sent:final])
                        row[3] = sent = final
                    if row_ended and sent == n_end:             # (n_end is the row's length where it has no cut)
                        if cut:
                            if n_end == 0:                       # an empty cut: what tts_single does with it
                                truncate_mel(mel_post[j, :, :row_len], sess.alignments[j, :row_len, int(sess._keep[3][j])])
                            sv.append(sid, mel_post[j, :, n_end - 1:n_end].expand(-1, 3))
                        sv.finish(sid)
                        row[2] = None
                if sess.ended:
                    assert all(row[2] is None for row in rows)
                    sess, rows = None, []
            chunks = sv.step()
            for sid, chunk, last in chunks:
                i = line_of.pop(sid) if last else line_of[sid]
                yield chunk.cpu() if single else (i, chunk.cpu(), last)
            if sess is None and not todo and not line_of:
                return

    def tts(self, text_buckw: Union[str, List[str]], speed: Union[int, float, None] = None, denoise: float = 0.005,
            speaker_id: int = 0, batch_size: int = 8, vowelizer=None, postprocess_mel: bool = True,
            return_mel: bool = False, normalize=None, limiter=False, true_peak=False,
            return_timestamps: bool = False) -> Union[torch.Tensor, List[torch.Tensor]]:
        """Same contract as the reference (:353-426): str -> Tensor[n_samples] (CPU); list -> list of
        tensors, chunked by `batch_size`.
        normalize (not in the reference): the level of every wave, set on the device after the denoiser -- None, 'peak' (x / max|x| *
        0.99), 'lufs' (-23 LUFS, ITU-R BS.1770-4) or a target in LUFS, or for a list of lines one such value per line (as
        FastPitch2Wave.tts takes it).
        limiter (False, True or a dict with any of ceiling, attack_ms, hold_ms, max_gain_db; needs a normalize): the lines with 'lufs' or
        a target get the full gain towards it and the look-ahead limiter holds their peaks at the ceiling (as FastPitch2Wave.tts).
        true_peak (False or True; needs a normalize): the peaks of both are true peaks (utils.audio.true_peak), as FastPitch2Wave.tts.
        return_timestamps (not in the reference): (wave, timing) for a string, (waves, timings) for a list, as FastPitch2Wave.tts
        hands them out; Tacotron2 has no durations of its own, so they are the monotonic path through its attention (tts_single)."""
        kw = dict(speaker_id=speaker_id, speed=speed, denoise=denoise, vowelizer=vowelizer,
                  postprocess_mel=postprocess_mel, return_mel=return_mel, **({'return_timestamps': True} if return_timestamps else {}))
        if isinstance(text_buckw, str):
            return self.tts_single(text_buckw, normalize=normalize, **kw, **({'limiter': limiter} if limiter else {}),
                                   **({'true_peak': true_peak} if true_peak else {}))
        assert isinstance(text_buckw, list)
        check_normalize(normalize, len(text_buckw))
        limiter = check_limiter(limiter, normalize)
        check_true_peak(true_peak, normalize, limiter)
        at = (lambda i: normalize[i]) if per_row(normalize) else (lambda i: normalize)
        if batch_size == 1:
            res = [self.tts_single(sample, normalize=at(i), **kw, **_lim(limiter, at(i), true_peak)) for i, sample in enumerate(text_buckw)]
            if return_timestamps:                   # (wave, [mel,] timing) per line -> (the list as without the flag, the timings)
                return [r[0] if len(r) == 2 else r[:-1] for r in res], [r[-1] for r in res]
            return res
        wav_list, timings = [], []
        for k in range(0, len(text_buckw), batch_size):
            idx = range(k, min(k + batch_size, len(text_buckw)))
            chunk_norm = [at(i) for i in idx] if per_row(normalize) else normalize
            got = self.tts_batch(text_buckw[k:k + batch_size], normalize=chunk_norm, **kw, **_lim(limiter, chunk_norm, true_peak))
            if return_timestamps:
                got, more = got
                timings += more
            wav_list += got
        return (wav_list, timings) if return_timestamps else wav_list

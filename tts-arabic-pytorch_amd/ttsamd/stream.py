"""Streaming synthesis: chunked HiFi-GAN or Vocos with continuous batching of windows (csrc/stream.hip, csrc/vocos.hip).

HiFi-GAN is a stack of zero-padded convolutions, so a window of mel frames with `halo` extra frames on each side gives, on its core, the
samples of the whole-utterance call; a window that touches an utterance edge starts or ends exactly there, which keeps the per-layer
zero padding (and the denoiser's reflect padding) what the whole-utterance call sees.  `plan_chunks` cuts an utterance into such
windows; `StreamingVocoder` keeps the mels of the open utterances in a pool and, per `step()`, takes the next window of every one of
them through ONE gather -> ttsamd_hifigan_forward -> ttsamd_denoise_rows -> emit sequence: utterances at different points of their
lengths share one chip-filling vocoder call, and audio leaves while the rest is still being made.

Vocos (MelVocos '22k' / '24k') goes the same way with its own receptive field (`vocos_halo_frames`): its backbone is zero-padded
convolutions with a per-frame LayerNorm, its head an ISTFT whose frames overlap by three hops.  A step is gather ->
ttsamd_vocos_forward_windows -> emit; the bias denoise is a per-frame spectral subtraction inside that call (no Denoiser, no halo of its
own).  The "center" framing of '24k' gives an utterance of T frames 256 (T - 1) samples: `plan_chunks_center` cuts those.

A stream may grow (Tacotron2 makes its mel frame by frame: `open_growing` / `append` / `finish`).  `next_growing_chunk` releases a core
as soon as enough frames are known behind it that it is a core of `plan_chunks` of the final length with a complete window, so the
chunks -- and with them the denoiser halo, the resampler, the limiter's carried samples -- are those of open() on the whole mel.

Levelling inside a stream: with `limiter=` a step runs vocoder -> denoise -> ttsamd_wave_limit (mode 3: the stream's fixed gain in dB and
the look-ahead limiter, in place on the window rows) -> emit.  A limited sample depends on the input over [i - A - R, i + 2A] only, so
the windows widen by that reach in frames (`limiter_halo_frames`), as they widen by the resampler's, and the curve is integer
arithmetic: the chunks put together are the bits of utils.audio.limit on the whole wave.  With `true_peak=True` the call is
ttsamd_wave_limit_true_peak, whose detector reads 13 more samples on each side: the reach, the windows and the carried history grow by
that, and the chunks are the bits of utils.audio.limit(true_peak=True)."""
import ctypes as C

import numpy as np

from . import lib as L

MAX_WINDOWS = 64            # TTSAMD_STREAM_MAX_WINDOWS of include/ttsamd.h
DENOISER_HALO = 3           # ttsamd_denoiser_halo_frames(): 768 samples of the 1024 / 256 STFT -> ISTFT round trip
ENCODINGS = {'float32': 0, 'pcm16': 1, 'mulaw': 2, 'alaw': 3}       # the format codes of ttsamd_stream_emit_resampled


def hifigan_halo_frames(config):
    """(left, right): the receptive field of a HiFi-GAN generator in mel frames per side, from its config dict -- the derivation of
    ttsamd_hifigan_halo_frames (include/ttsamd.h) restated on the host.  The samples [0, hop - 1] of one frame are walked back to the
    mel frames they depend on: conv_post widens the interval by 3, every stage by its longest ResBlock branch, every transposed conv
    (kernel kt, stride u, padding (kt - u) / 2) maps [lo, hi] to [ceil((lo + p - kt + 1) / u), floor((hi + p) / u)], conv_pre widens by 3."""
    rates, kts = list(config['upsample_rates']), list(config['upsample_kernel_sizes'])
    rb2 = str(config.get('resblock', '1')) == '2'
    reach = 0
    for k, ds in zip(config['resblock_kernel_sizes'], config['resblock_dilation_sizes']):
        half = (k - 1) // 2
        reach = max(reach, half * (ds[0] + ds[1]) if rb2 else sum(half * (d + 1) for d in ds))
    lo, hi = -3, int(np.prod(rates)) - 1 + 3
    for u, kt in zip(reversed(rates), reversed(kts)):
        p = (kt - u) // 2
        lo, hi = lo - reach, hi + reach
        lo, hi = -((-(lo + p - kt + 1)) // u), (hi + p) // u
    return 3 - lo, hi + 3


def vocos_halo_frames(config):
    """(left, right): the receptive field of a Vocos vocoder in mel frames per side, from its config dict -- the derivation of
    ttsamd_vocos_halo_frames (include/ttsamd.h) restated on the host.  The backbone (embed k = 7, then num_layers depthwise k = 7; the
    rest is per frame) reaches 3 + 3 num_layers frames; sample 256 c + j sums the ISTFT frames t with 0 <= 256 (c - t) + j + pad < 1024:
    c - 2 ... c + 2 with "same" (pad 384), c - 1 ... c + 2 with "center" (pad 512).  (29, 29) for '22k', (28, 29) for '24k'."""
    reach = 3 + 3 * int(config['num_layers'])
    padding = config.get('padding', 'same')
    if padding not in ('same', 'center'):
        raise ValueError(f'vocos_halo_frames: padding {padding!r}')
    return reach + (1 if padding == 'center' else 2), reach + 2


def pcm16(x):
    """float samples -> int16 PCM with save_wav's arithmetic (utils/audio.py): clip(rint(x * 32767), -32768, 32767) on the fp32 product,
    round-half-even, NaN -> 0.  What ttsamd_stream_emit(format = 1) writes."""
    a = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        v = np.clip(np.rint(a * np.float32(32767.0)), -32768, 32767)
    return np.where(np.isnan(a), np.float32(0), v).astype('<i2')


def resample_reach(o, width):
    """the samples before S0 and after S1 - 1 that the resampler's outputs of a core [S0, S1) can read: width + o - 1.  With
    K0 = ceil(n S0 / o), K1 = ceil(n S1 / o), f0 = K0 // n and f1 = (K1 - 1) // n: K0 o / n >= S0 gives f0 o >= S0 - o + 1, and
    (K1 - 1) o / n < S1 gives f1 o <= S1 - 1; frame f reads the samples f o - width ... f o + width + o - 1."""
    return int(width) + int(o) - 1


def resample_halo_frames(o, n, width, hop):
    """resample_reach in frames of hop samples, rounded up: 2 for 22 050 -> 8 000, 16 000 or 32 000 Hz, 1 for 11 025, 24 000, 44 100, 48 000"""
    return -(-resample_reach(o, width) // int(hop))


def limiter_halo_frames(attack, hold, hop, true_peak=False):
    """the limiter's reach (A + R samples back, 2A ahead, each 13 more with the true-peak detector: include/ttsamd.h) in frames of hop
    samples, rounded up"""
    extra = 13 if true_peak else 0
    return -(-(max(int(attack) + int(hold), 2 * int(attack)) + extra) // int(hop))


def chunk_outputs(core_start, core_end, o, n):
    """(K0, K1): the resampler's outputs that belong to the core [core_start, core_end) (samples): ceil(n S / o) at both ends, in
    exact integers.  The cores of an utterance partition [0, L), so these ranges partition [0, out_len(L))."""
    return -(-n * int(core_start) // o), -(-n * int(core_end) // o)


def delivery(source_rate, sample_rate=None, encoding=None, pcm16=False, lowpass_filter_width=6, rolloff=0.99):
    """The delivery arguments of StreamingVocoder, checked on the host -> (encoding, sample_rate, (o, n, width) or None when the rate
    stays).  ValueError: an unknown encoding, pcm16=True next to another encoding, a rate the resampler refuses."""
    from . import resample as R
    if encoding is not None and encoding not in ENCODINGS:
        raise ValueError(f'StreamingVocoder: encoding {encoding!r}: one of {sorted(ENCODINGS)}')
    if pcm16 and encoding not in (None, 'pcm16'):
        raise ValueError(f"StreamingVocoder: pcm16=True means encoding='pcm16', got encoding={encoding!r}")
    encoding = 'pcm16' if pcm16 else (encoding or 'float32')
    source_rate = int(source_rate)
    if sample_rate is None or sample_rate == source_rate:
        return encoding, source_rate, None
    return encoding, int(sample_rate), R.geometry(source_rate, sample_rate, lowpass_filter_width, rolloff)


def plan_chunks(T, first_chunk_frames, chunk_frames, halo_left, halo_right):
    """[(core_start, core_len, win_start, win_len)] for an utterance of T frames.  The cores partition [0, T) in order: the first is
    min(first_chunk_frames, T) frames (a short one: time to first audio), the following ones chunk_frames; a remainder shorter than
    chunk_frames // 2 is folded into the core before it.  A window is its core plus min(halo, distance to the utterance edge) frames
    on each side."""
    T, first, chunk, hl, hr = int(T), int(first_chunk_frames), int(chunk_frames), int(halo_left), int(halo_right)
    if T < 1 or first < 1 or chunk < 1 or hl < 0 or hr < 0:
        raise ValueError(f'plan_chunks: T {T}, first_chunk_frames {first}, chunk_frames {chunk}, halos {hl} / {hr}')
    cores, pos = [], 0
    while pos < T:
        n = min(first if not cores else chunk, T - pos)
        cores.append([pos, n])
        pos += n
    if len(cores) > 1 and cores[-1][1] < chunk // 2:
        cores[-2][1] += cores.pop()[1]
    plan = []
    for s, n in cores:
        ws, we = s - min(hl, s), s + n + min(hr, T - s - n)
        plan.append((s, n, ws, we - ws))
    return plan


def growing_lookahead(chunk_frames, halo_right):
    """the frames a growing stream must know behind a core before it may release it while the end is unknown:
    max(chunk_frames // 2, halo_right, 1).  The first term: the rest of the utterance is then at least chunk_frames // 2 frames, so
    plan_chunks would not fold it into this core; the second: the core's window is complete and does not touch the utterance's end;
    the 1 (it only matters with chunk_frames = 1 and no halo): the last core is never released before the end is known, so every
    stream has a chunk left to carry `last`."""
    return max(int(chunk_frames) // 2, int(halo_right), 1)


def next_growing_chunk(pos, known_frames, ended, first_chunk_frames, chunk_frames, halo_left, halo_right):
    """The planner of a stream whose length is not known when it opens: the next (core_start, core_len, win_start, win_len) of an
    utterance whose released cores cover [0, pos), of which `known_frames` frames have arrived and whose end is known (`ended`: the
    utterance has known_frames frames) or not -- or None while that chunk may not be released yet (and when nothing is left).
    Whatever the arrival schedule, the chunks released are plan_chunks(T, ...) of the final T, in order: with the end known, the core
    at `pos` of that plan; without, the nominal core [pos, pos + n) once known_frames >= pos + n + growing_lookahead(...)."""
    pos, known, first, chunk, hl, hr = int(pos), int(known_frames), int(first_chunk_frames), int(chunk_frames), int(halo_left), int(halo_right)
    if pos < 0 or known < pos or first < 1 or chunk < 1 or hl < 0 or hr < 0:
        raise ValueError(f'next_growing_chunk: pos {pos}, known_frames {known}, first_chunk_frames {first}, chunk_frames {chunk}, halos {hl} / {hr}')
    if ended:
        if pos >= known:
            return None
        for c in plan_chunks(known, first, chunk, hl, hr):
            if c[0] == pos:
                return c
        raise ValueError(f'next_growing_chunk: no core of plan_chunks({known}, ...) starts at {pos}')
    n = first if pos == 0 else chunk
    if known < pos + n + growing_lookahead(chunk, hr):
        return None
    ws = pos - min(hl, pos)
    return (pos, n, ws, pos + n + hr - ws)


def plan_chunks_center(T, first_chunk_frames, chunk_frames, halo_left, halo_right):
    """plan_chunks for the "center" framing (MelVocos '24k'), where an utterance of T >= 2 mel frames has hop * (T - 1) samples:
    [(core_start, core_len, win_start, win_len)] with the cores in frames of hop SAMPLES, partitioning [0, T - 1) by plan_chunks' rule
    (none is empty), and the windows in MEL frames: the frames the core's samples depend on, [core_start - halo_left, core_start +
    core_len + halo_right) clipped to [0, T) -- up to T, one frame past the last core's end, which that core's samples read."""
    T, hl, hr = int(T), int(halo_left), int(halo_right)
    if T < 2:
        raise ValueError(f'plan_chunks_center: {T} frame(s): the centred ISTFT needs at least 2')
    plan = []
    for s, n, _, _ in plan_chunks(T - 1, first_chunk_frames, chunk_frames, hl, hr):
        ws = max(s - hl, 0)
        plan.append((s, n, ws, min(s + n + hr, T) - ws))
    return plan


def max_core_frames(first_chunk_frames, chunk_frames):
    """the longest core plan_chunks can return: a core that took a folded remainder"""
    return max(int(first_chunk_frames), int(chunk_frames)) + max(int(chunk_frames) // 2 - 1, 0)


class _Open:
    __slots__ = ('sid', 'slot', 'plan', 'next', 'denoise', 'frames', 'gain_db', 'lim_end', 'growing', 'ended', 'pos', 'halos')

    def __init__(self, sid, slot, plan, denoise, frames, gain_db=0.0):
        self.sid, self.slot, self.plan, self.next, self.denoise, self.frames, self.gain_db = sid, slot, plan, 0, denoise, frames, gain_db
        self.lim_end = 0                # samples of the utterance whose value in front of the limiter is settled (see _carry)
        # a growing stream (open_growing): `plan` is None, `frames` the frames that have arrived, `pos` the end of the released cores
        self.growing, self.ended, self.pos, self.halos = False, True, 0, None


class StreamingVocoder:
    """Chunked vocoding of up to `max_streams` open utterances of up to `max_frames` frames each.

    vocoder: a vocoder.hifigan.models.Generator (V1 or V3) on the GPU; denoiser: the vocoder.hifigan.denoiser.Denoiser of that
    generator, needed only for open(denoise > 0).  Or a vocoder.vocos.MelVocos ('22k' / '24k'): its bias denoise is part of the vocoder
    call, so denoiser must stay None and open() takes any strength >= 0; with '24k' an utterance of T frames has 256 (T - 1) samples
    and needs T >= 2.  Every buffer is allocated here, once.  open(mel, denoise) -> sid copies a mel into a
    free slot; step() returns the next chunk of every open utterance; an utterance closes itself after its last chunk.  Precision is
    the library's (ttsamd.engine.set_precision): the step calls the forward entry the one-shot path calls.

    sample_rate: the rate the chunks leave at (None: the vocoder's own, vocoder.sampling_rate or 22 050 Hz), through the polyphase
    resampler of utils.audio.resample with lowpass_filter_width and rolloff; encoding: 'float32' (default) | 'pcm16' | 'mulaw' |
    'alaw' (G.711, one byte per sample); pcm16=True means encoding='pcm16'.  Put together, the chunks of a stream are the bits of
    utils.audio.resample on the samples the stream has at the vocoder's rate, encoded.  The vocoder's rate as float32 or PCM16 is the
    path without a resampler, ttsamd_stream_emit.

    limiter (None / False, True or a dict with any of ceiling, attack_ms, hold_ms, max_gain_db: ttsamd.engine.limiter_spec): every
    window goes through the look-ahead limiter at the vocoder's rate, after the denoiser and before the resampler, with the gain
    open(gain_db=) gave its utterance (at most max_gain_db); the chunks of a stream are then the bits of utils.audio.limit on the
    stream's unlimited samples (resampled and encoded as above).  `reduction` holds the last step's smallest curve value per row.
    `bypass = True` skips the limiter's launch (and with it the gain) and leaves everything else as it is: the same windows, the same
    vocoder launches, the same samples carried from step to step (`_carry`), so these are, bit for bit, the samples the limiter works
    on -- for an A / B comparison.
    true_peak (needs a limiter; ValueError without one): the limiter's detector is the true-peak one (ttsamd_wave_limit_true_peak),
    and the chunks are the bits of utils.audio.limit(true_peak=True)."""

    def __init__(self, vocoder, denoiser=None, max_streams=32, max_frames=4096, chunk_frames=64, first_chunk_frames=32, pcm16=False,
                 sample_rate=None, encoding=None, lowpass_filter_width=6, rolloff=0.99, limiter=None, true_peak=False):
        import torch
        from .engine import DenoiserEngine, _Workspace, limiter_reach, limiter_samples, limiter_spec
        if min(int(max_streams), int(max_frames), int(chunk_frames), int(first_chunk_frames)) < 1:
            raise ValueError('StreamingVocoder: max_streams, max_frames, chunk_frames and first_chunk_frames must be >= 1')
        source_rate = int(getattr(vocoder, 'sampling_rate', None) or (getattr(vocoder, 'h', None) or {}).get('sampling_rate') or 22050)
        self._encoding, self._sample_rate, self._rs = delivery(source_rate, sample_rate, encoding, pcm16, lowpass_filter_width, rolloff)
        pcm16 = self._encoding == 'pcm16'
        from vocoder.vocos import MelVocos
        self._vocos = isinstance(vocoder, MelVocos)
        if self._vocos and denoiser is not None:
            raise ValueError('StreamingVocoder: a Vocos vocoder subtracts its bias inside the vocoder call: denoiser must be None')
        self.eng = vocoder.engine()
        self.lib, self.device = self.eng.lib, self.eng.device
        self.hop, self.num_mels = self.eng.hop, self.eng.n_mels if self._vocos else self.eng.num_mels
        self._center = bool(self._vocos and self.eng.center)          # utterance samples: hop * (T - 1)
        left, right = C.c_int32(), C.c_int32()
        if self._vocos:
            L.check(self.lib.ttsamd_vocos_halo_frames(self.eng.handle, C.byref(left), C.byref(right)), 'vocos_halo_frames')
        else:
            L.check(self.lib.ttsamd_hifigan_halo_frames(self.eng.handle, C.byref(left), C.byref(right)), 'hifigan_halo_frames')
        self._halo = (left.value, right.value)
        self.max_streams, self.max_frames = int(max_streams), int(max_frames)
        self.chunk_frames, self.first_chunk_frames, self.pcm16 = int(chunk_frames), int(first_chunk_frames), bool(pcm16)
        self.denoiser = denoiser
        self._dn_eng = self._bias = None
        dn_halo = 0
        if denoiser is not None:
            dn_halo = int(self.lib.ttsamd_denoiser_halo_frames())
            if denoiser.device != self.device:
                denoiser.to(self.device)
            self._dn_eng = denoiser._engine(lambda d: DenoiserEngine(device=d))
            self._bias = denoiser._bias_spec(self.device).reshape(-1).contiguous()
        self._dn_halo = dn_halo
        if self._vocos:
            self._bias = self.eng.bias_vec().reshape(-1)
        dev = self.device
        # the resampled / G.711 path (ttsamd_stream_emit_resampled); None: ttsamd_stream_emit, as before there was one
        self._resampled = self._rs is not None or self._encoding in ('mulaw', 'alaw')
        self._rs_eng, self._rs_halo = None, 0
        if self._rs is not None:
            from utils.audio import _resampler
            self._rs_eng = _resampler(source_rate, self._sample_rate, lowpass_filter_width, rolloff, 'sinc_interp_hann', dev)
            assert (self._rs_eng.o, self._rs_eng.n, self._rs_eng.width) == self._rs
            self._rs_halo = resample_halo_frames(*self._rs, self.hop)
        # the limiter (ttsamd_wave_limit, mode 3) between the denoiser and the emit: its reach widens the windows as the resampler's does
        self._lim = limiter_spec(limiter)
        self._lim_tp = bool(true_peak)
        if self._lim_tp and self._lim is None:
            raise ValueError('StreamingVocoder: true_peak needs the limiter (StreamingVocoder(..., limiter=True))')
        self._lim_halo = 0
        self.bypass = False
        self.reduction = None           # int32 [rows] on the device after a step with a limiter: min of the curve per window (Q30)
        if self._lim is not None:
            self._lim_ar = limiter_samples(self._lim['attack_ms'], self._lim['hold_ms'], source_rate)
            self._lim_halo = limiter_halo_frames(*self._lim_ar, self.hop, self._lim_tp)
            self._lim_ws = _Workspace()
        self._rs_halo += self._lim_halo         # everything below plans with the sum: the emit reads limited samples
        self._core_cap = max_core_frames(first_chunk_frames, chunk_frames)
        self._w_cap = (self._core_cap + left.value + right.value + 2 * dn_halo + 2 * self._rs_halo + 3) & ~3
        self._rows = min(MAX_WINDOWS, self.max_streams)
        self._pool = torch.zeros(self.max_streams, self.num_mels, self.max_frames, dtype=torch.float32, device=dev)
        self._batch = torch.empty(self._rows * self.num_mels * self._w_cap, dtype=torch.float32, device=dev)
        self._lens = torch.empty(self._rows, dtype=torch.int64, device=dev)
        self._wave = torch.empty(self._rows * self.hop * self._w_cap, dtype=torch.float32, device=dev)
        out_dtype = {'float32': torch.float32, 'pcm16': torch.int16}.get(self._encoding, torch.uint8)
        o, n = self._rs[:2] if self._rs else (1, 1)
        self._c_cap = self.hop * self._core_cap if not self._resampled else -(-n * self.hop * self._core_cap // o) + 1
        self._out = [torch.empty(self._rows * self._c_cap, dtype=out_dtype, device=dev) for _ in range(2)]
        if self._lim is not None:
            self._lim_gain = torch.empty(self._rows, dtype=torch.float32, device=dev)
            self._lim_red = [torch.empty(self._rows, dtype=torch.int32, device=dev) for _ in range(2)]
            self._lim_mode = torch.full((self._rows,), 3, dtype=torch.int32, device=dev)
            # samples behind / ahead of a core that its chunk depends on through the limiter (and the resampler behind it)
            rs_reach = resample_reach(self._rs[0], self._rs[2]) if self._rs else 0
            back, ahead = limiter_reach(*self._lim_ar, true_peak=self._lim_tp)
            self._lim_lb, self._lim_la = rs_reach + back, rs_reach + ahead
            self._hist = torch.zeros(self.max_streams, max(self._lim_lb + self._lim_la, 1), dtype=torch.float32, device=dev)
        self._flip = 0
        self._free = list(range(self.max_streams))
        self._open = {}                 # sid -> _Open, in opening order (oldest first)
        self._next_sid = 0

    @property
    def halo(self):
        """(left, right) receptive field of the vocoder in mel frames: ttsamd_hifigan_halo_frames / ttsamd_vocos_halo_frames of its handle"""
        return self._halo

    @property
    def sample_rate(self):
        """the rate the chunks leave at, Hz"""
        return self._sample_rate

    @property
    def encoding(self):
        """'float32' | 'pcm16' | 'mulaw' | 'alaw'"""
        return self._encoding

    @property
    def free_slots(self):
        return len(self._free)

    @property
    def open_streams(self):
        return list(self._open)

    def open(self, mel, denoise=0.0, gain_db=0.0):
        """mel [num_mels, T] (a device tensor: copied device to device) -> sid.  ValueError: T > max_frames, no free slot, a denoise
        strength that is not finite, denoise > 0 without a denoiser or on an utterance of at most 512 samples (as the one-shot Denoiser).
        A Vocos vocoder takes any denoise >= 0 on any length; '24k' refuses one frame, as MelVocos.forward does.
        gain_db: the utterance's fixed gain in front of the limiter; a value other than 0 without a limiter is a ValueError."""
        import torch
        mel = torch.as_tensor(mel)
        if mel.dim() != 2 or mel.shape[0] != self.num_mels or mel.shape[1] < 1:
            raise ValueError(f'StreamingVocoder.open: mel must be [{self.num_mels}, T >= 1], got {tuple(mel.shape)}')
        T = int(mel.shape[1])
        denoise = float(denoise)
        if not np.isfinite(denoise):
            raise ValueError(f'StreamingVocoder.open: denoise {denoise!r} is not finite')
        gain_db = float(gain_db)
        if not np.isfinite(gain_db):
            raise ValueError(f'StreamingVocoder.open: gain_db {gain_db!r} is not finite')
        if gain_db != 0.0 and self._lim is None:
            raise ValueError('StreamingVocoder.open: gain_db needs the limiter (StreamingVocoder(..., limiter=True)): a gain alone could clip')
        if T > self.max_frames:
            raise ValueError(f'StreamingVocoder.open: {T} frames, the pool holds utterances of up to max_frames = {self.max_frames}')
        if self._vocos:
            if denoise < 0:
                raise ValueError(f'StreamingVocoder.open: denoise {denoise!r} is negative')
            if self._center and T < 2:
                raise ValueError("MelVocos('24k'): the centred ISTFT needs at least 2 frames (got %d)" % T)
        elif denoise > 0:
            if self._dn_eng is None:
                raise ValueError('StreamingVocoder.open: denoise > 0 needs the denoiser (StreamingVocoder(vocoder, denoiser=...))')
            if self.hop * T <= 512:
                raise ValueError('Denoiser: every utterance needs more than 512 samples (reflect padding of n_fft/2); '
                                 f'shortest has {self.hop * T}')
        if not self._free:
            raise ValueError(f'StreamingVocoder.open: all {self.max_streams} slots are taken (max_streams)')
        halo = (self._dn_halo if denoise > 0 and not self._vocos else 0) + self._rs_halo
        plan = (plan_chunks_center if self._center else plan_chunks)(T, self.first_chunk_frames, self.chunk_frames, self._halo[0] + halo,
                                                                     self._halo[1] + halo)
        slot = self._free.pop(0)
        self._pool[slot, :, :T].copy_(mel.to(dtype=torch.float32), non_blocking=True)
        sid = self._next_sid
        self._next_sid += 1
        self._open[sid] = _Open(sid, slot, plan, denoise, T - 1 if self._center else T, gain_db)        # frames of hop samples
        return sid

    def first_release_frames(self, denoise=0.0):
        """the frames a growing stream opened with this denoise strength needs before step() releases its first chunk while its end is
        unknown: first_chunk_frames + growing_lookahead over the right halo in total (vocoder, denoiser, resampler, limiter)"""
        halo = (self._dn_halo if float(denoise) > 0 and not self._vocos else 0) + self._rs_halo
        return self.first_chunk_frames + growing_lookahead(self.chunk_frames, self._halo[1] + halo)

    def open_growing(self, denoise=0.0, gain_db=0.0):
        """A stream whose length is not known when it opens -> sid: `append` its frames as they come, `finish` it at its end.  step()
        returns its next chunk as soon as the planner may release it (`next_growing_chunk`) and skips it otherwise; the chunks are those
        of open() on the whole mel, bit for bit, because the cores and windows are the same.  denoise / gain_db and their ValueErrors
        as open(); the short-utterance check of the denoiser falls at finish(), where the length is known.  The centred framing
        (MelVocos '24k') is refused: its last core reads one frame past its end."""
        if self._center:
            raise ValueError("StreamingVocoder.open_growing: the centred framing (MelVocos '24k') is not supported for growing streams")
        denoise, gain_db = float(denoise), float(gain_db)
        if not np.isfinite(denoise):
            raise ValueError(f'StreamingVocoder.open_growing: denoise {denoise!r} is not finite')
        if not np.isfinite(gain_db):
            raise ValueError(f'StreamingVocoder.open_growing: gain_db {gain_db!r} is not finite')
        if gain_db != 0.0 and self._lim is None:
            raise ValueError('StreamingVocoder.open_growing: gain_db needs the limiter (StreamingVocoder(..., limiter=True)): a gain alone could clip')
        if self._vocos and denoise < 0:
            raise ValueError(f'StreamingVocoder.open_growing: denoise {denoise!r} is negative')
        if not self._vocos and denoise > 0 and self._dn_eng is None:
            raise ValueError('StreamingVocoder.open_growing: denoise > 0 needs the denoiser (StreamingVocoder(vocoder, denoiser=...))')
        if not self._free:
            raise ValueError(f'StreamingVocoder.open_growing: all {self.max_streams} slots are taken (max_streams)')
        halo = (self._dn_halo if denoise > 0 and not self._vocos else 0) + self._rs_halo
        sid = self._next_sid
        self._next_sid += 1
        st = _Open(sid, self._free.pop(0), None, denoise, 0, gain_db)
        st.growing, st.ended, st.halos = True, False, (self._halo[0] + halo, self._halo[1] + halo)
        self._open[sid] = st
        return sid

    def append(self, sid, frames):
        """frames [num_mels, n] (a device tensor: copied device to device behind the stream's frames so far); n = 0 is allowed.
        KeyError: sid is not open; ValueError: not a growing stream, already finished, a wrong shape, more than max_frames in all."""
        import torch
        st = self._open[sid]
        if not st.growing or st.ended:
            raise ValueError(f'StreamingVocoder.append: stream {sid} is not a growing stream that is still open for frames')
        frames = torch.as_tensor(frames)
        if frames.dim() != 2 or frames.shape[0] != self.num_mels:
            raise ValueError(f'StreamingVocoder.append: frames must be [{self.num_mels}, n], got {tuple(frames.shape)}')
        n = int(frames.shape[1])
        if st.frames + n > self.max_frames:
            raise ValueError(f'StreamingVocoder.append: {st.frames + n} frames, the pool holds utterances of up to max_frames = {self.max_frames}')
        if n:
            self._pool[st.slot, :, st.frames:st.frames + n].copy_(frames.to(dtype=torch.float32), non_blocking=True)
            st.frames += n

    def finish(self, sid):
        """The stream has all its frames: its remaining chunks follow, the last one marked.  ValueError: no frame at all, or denoise > 0
        on an utterance of at most 512 samples (as open() and the one-shot Denoiser)."""
        st = self._open[sid]
        if not st.growing or st.ended:
            raise ValueError(f'StreamingVocoder.finish: stream {sid} is not a growing stream that is still open for frames')
        if st.frames < 1:
            raise ValueError(f'StreamingVocoder.finish: stream {sid} has no frames')
        if not self._vocos and st.denoise > 0 and self.hop * st.frames <= 512:
            raise ValueError('Denoiser: every utterance needs more than 512 samples (reflect padding of n_fft/2); '
                             f'shortest has {self.hop * st.frames}')
        st.ended = True

    def _next_chunk(self, st):
        """the chunk step() takes next from an open stream, or None (a growing stream that has to wait for frames)"""
        if not st.growing:
            return st.plan[st.next]
        return next_growing_chunk(st.pos, st.frames, st.ended, self.first_chunk_frames, self.chunk_frames, *st.halos)

    def _carry(self, rows, chunks, w_max):
        """The vocoder's fp32 sums for one sample differ in their last bits from window to window, and the limiter's curve at a chunk's
        edge depends on samples of the neighbouring cores.  So that the chunks are the limiter's bits on ONE wave, a sample's value in
        front of the limiter is settled by the first window that has to provide it: step k settles [end of step k - 1, core end + la)
        from its window and takes what lies before from the utterance's history (the last lb + la settled samples, kept per slot),
        copied over the window row; then the history moves on.  Two index copies per step; the cores read behind this (with `bypass`,
        as they are) are that one wave."""
        import torch
        H, hop = self._lim_lb + self._lim_la, self.hop
        if H == 0:
            return
        stride = hop * w_max
        put_w, put_h, get_w, get_h = [], [], [], []
        for w, (st, c) in enumerate(zip(rows, chunks)):
            w0, end, prev = hop * c[2], min(hop * (c[0] + c[1]) + self._lim_la, hop * st.frames), st.lim_end
            lo = max(prev - H, w0, 0)
            if prev > lo:                   # history -> window row
                pos = np.arange(lo, prev, dtype=np.int64)
                put_w.append(w * stride + pos - w0)
                put_h.append(st.slot * H + pos - (prev - H))
            lo = max(end - H, w0, 0)
            if end > lo:                    # window row -> history, right-aligned at `end`
                pos = np.arange(lo, end, dtype=np.int64)
                get_w.append(w * stride + pos - w0)
                get_h.append(st.slot * H + pos - (end - H))
            st.lim_end = end
        up = lambda parts: torch.from_numpy(np.concatenate(parts)).pin_memory().to(self.device, non_blocking=True)      # noqa: E731
        hist = self._hist.view(-1)
        if put_w:
            self._wave[up(put_w)] = hist[up(put_h)]
        if get_w:
            hist[up(get_h)] = self._wave[up(get_w)]

    def close(self, sid):
        """Drop an open utterance (its remaining chunks are not made) and free its slot.  KeyError for a sid that is not open."""
        self._free.append(self._open.pop(sid).slot)

    def step(self):
        """The next chunk of every open utterance whose next window is ready (a growing stream that waits for frames is skipped and stays
        open), oldest first, at most 64 -> [(sid, chunk, last)]: chunk is a device tensor of
        hop * core_len samples (float32, or int16 with pcm16) -- at another sample_rate, of the resampler's outputs that belong to the
        core (`chunk_outputs`: float32, int16, or uint8 for G.711) --, valid until the step after next; `last` marks an utterance's
        final chunk, after which it is closed.  One gather, one vocoder forward, one denoise (when a row asks for it) and one emit on
        the current stream; the host waits for none of them (the chunk lengths are host arithmetic).  Vocos: one gather, one
        ttsamd_vocos_forward_windows (whose head runs only on the core, widened by the resampler's reach), one emit."""
        import torch
        from .engine import _ptr, _stream
        ready = [(st, c) for st, c in ((st, self._next_chunk(st)) for st in self._open.values()) if c is not None][:self._rows]
        if not ready:
            return []               # nothing open, or only growing streams that wait for frames: they stay open
        rows, chunks = [st for st, _ in ready], [c for _, c in ready]
        W = len(rows)
        i32 = C.c_int32 * W
        w_max = (max(c[3] for c in chunks) + 3) & ~3
        if self._resampled:
            o, n = self._rs[:2] if self._rs else (1, 1)
            k = [chunk_outputs(self.hop * c[0], self.hop * (c[0] + c[1]), o, n) for c in chunks]
            counts = [k1 - k0 for k0, k1 in k]
        else:
            counts = [self.hop * c[1] for c in chunks]
        c_max = max(max(counts), 1)
        slot, start, length = i32(*[st.slot for st in rows]), i32(*[c[2] for c in chunks]), i32(*[c[3] for c in chunks])
        off, n = i32(*[self.hop * (c[0] - c[2]) for c in chunks]), i32(*[self.hop * c[1] for c in chunks])
        out = self._out[self._flip]
        self._flip ^= 1
        lib, eng = self.lib, self.eng
        with torch.cuda.device(self.device):
            L.check(lib.ttsamd_stream_gather(_ptr(self._pool), self.max_streams, self.num_mels, self.max_frames, slot, start, length, W,
                                             w_max, _ptr(self._batch), _ptr(self._lens), _stream()), 'stream_gather')
            if self._vocos:
                # the samples the emit reads: the core, with another rate the resampler's reach around it, inside the utterance
                need = [(max(c[0] - self._rs_halo, 0) - c[2], min(c[0] + c[1] + self._rs_halo, st.frames) - c[2]) for st, c in zip(rows, chunks)]
                strength = None
                if any(st.denoise > 0 for st in rows):
                    strength = torch.tensor([st.denoise for st in rows], dtype=torch.float32).pin_memory().to(self.device, non_blocking=True)
                nbytes = lib.ttsamd_vocos_workspace_bytes(eng.handle, W, w_max)
                ws = eng.ws.get(nbytes, self.device)
                L.check(lib.ttsamd_vocos_forward_windows(eng.handle, _ptr(self._batch), _ptr(self._lens), W, w_max, i32(*[a for a, _ in need]),
                                                         i32(*[b - a for a, b in need]), _ptr(strength), _ptr(self._bias), _ptr(self._wave),
                                                         _ptr(ws), nbytes, _stream()), 'vocos_forward_windows')
            else:
                nbytes = lib.ttsamd_hifigan_workspace_bytes(eng.handle, W, w_max)
                ws = eng.ws.get(nbytes, self.device)
                L.check(lib.ttsamd_hifigan_forward(eng.handle, _ptr(self._batch), _ptr(self._lens), W, w_max, _ptr(self._wave), _ptr(ws), nbytes,
                                                   _stream()), 'hifigan_forward')
                if any(st.denoise > 0 for st in rows):
                    # the strengths go up from pinned memory, asynchronously; a row at 0 is left untouched by ttsamd_denoise_rows
                    strength = torch.tensor([st.denoise for st in rows], dtype=torch.float32).pin_memory().to(self.device, non_blocking=True)
                    nsamples = self._lens[:W] * self.hop
                    n_max = self.hop * w_max
                    nb = lib.ttsamd_denoiser_workspace_bytes(W, n_max)
                    dws = self._dn_eng.ws.get(nb, self.device)
                    L.check(lib.ttsamd_denoise_rows(self._dn_eng.handle, _ptr(self._wave), n_max, _ptr(nsamples), W, n_max, _ptr(self._bias),
                                                    _ptr(strength), _ptr(dws), nb, _stream()), 'denoise_rows')
            if self._lim is not None:
                self._carry(rows, chunks, w_max)
            if self._lim is not None and not self.bypass:
                # mode 3 in place on the window rows, over the samples the vocoder made: a HiFi-GAN window whole, a Vocos window up to
                # the end of what its head ran on (what lies in front of that range is outside the reach of every sample the emit reads)
                ends = [self.hop * (nd[1] if self._vocos else c[3]) for nd, c in zip(need if self._vocos else chunks, chunks)]
                ends_d = torch.tensor(ends, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
                gains_d = torch.tensor([st.gain_db for st in rows], dtype=torch.float32).pin_memory().to(self.device, non_blocking=True)
                n_max = self.hop * w_max
                nb = lib.ttsamd_wave_limit_workspace_bytes(W, n_max)
                lws = self._lim_ws.get(max(nb, 1), self.device)
                self.reduction = self._lim_red[self._flip][:W]
                call, what = (lib.ttsamd_wave_limit_true_peak, 'wave_limit_true_peak') if self._lim_tp else (lib.ttsamd_wave_limit, 'wave_limit')
                L.check(call(_ptr(self._wave), n_max, _ptr(ends_d), W, _ptr(self._lim_mode), _ptr(gains_d), float(self._lim['ceiling']),
                             10.0 ** (self._lim['max_gain_db'] / 20.0), self._lim_ar[0], self._lim_ar[1], None, _ptr(self._lim_gain),
                             _ptr(self.reduction), _ptr(lws), nb, _stream()), what)
            if self._resampled:
                hop = self.hop
                L.check(lib.ttsamd_stream_emit_resampled(self._rs_eng.handle if self._rs_eng else None, _ptr(self._wave), W, w_max, hop,
                                                         i32(*[hop * c[2] for c in chunks]), i32(*[hop * (c[3] - self._center) for c in chunks]),
                                                         i32(*[hop * st.frames for st in rows]), i32(*[hop * c[0] for c in chunks]),
                                                         i32(*[hop * (c[0] + c[1]) for c in chunks]), c_max, ENCODINGS[self._encoding],
                                                         _ptr(out), None, _stream()), 'stream_emit_resampled')
            else:
                L.check(lib.ttsamd_stream_emit(_ptr(self._wave), W, w_max, self.hop, off, n, c_max, 1 if self.pcm16 else 0, _ptr(out),
                                               _stream()), 'stream_emit')
        view = out[:W * c_max].view(W, c_max)
        res = []
        for w, (st, c) in enumerate(zip(rows, chunks)):
            st.next += 1
            st.pos = c[0] + c[1]
            last = st.ended and st.pos == st.frames if st.growing else st.next == len(st.plan)
            res.append((st.sid, view[w, :counts[w]], last))
            if last:
                self.close(st.sid)
        return res

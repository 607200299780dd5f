"""Engines = C-ABI handles + workspaces.  PyTorch here is plumbing only (device memory,
current stream); every FLOP of the path runs in libttsamd.so."""
import ctypes as C

import numpy as np
import torch

from . import lib as L
from .config import NET_CONFIG, HIFIGAN_CONFIG, VOCOS_22K_CONFIG, TACOTRON2_CONFIG


def _require_gpu():
    if not torch.cuda.is_available():
        raise L.TtsAmdError('no ROCm device visible: the ttsamd engines run only on an MI355X (gfx950); '
                            'there is no CPU fallback')
    lib = L.load()
    if not lib.ttsamd_device_ok():
        raise L.TtsAmdError('device 0 is not gfx950')
    return lib


PRECISIONS = {'f32': 0, 'bf16': 1, 'bf16x3': 2}


def set_precision(name):
    """MFMA operand precision of all conv/linear GEMMs: 'f32' (default, exact), 'bf16' (config 3),
    'bf16x3' (split bf16: fp32-class accuracy at bf16 MFMA rate)."""
    lib = L.load()
    L.check(lib.ttsamd_set_precision(PRECISIONS[name]), 'set_precision')


def get_precision():
    code = L.load().ttsamd_get_precision()
    return {v: k for k, v in PRECISIONS.items()}[code]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, device):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _check_ids(t, n, what):
    """nn.Embedding raises IndexError on an out-of-range index; the HIP gathers only clamp.  Checked where it is free:
    on tensors that still live on the host (the drop-in wrappers tokenise on the CPU)."""
    if isinstance(t, torch.Tensor) and t.device.type == 'cpu' and t.numel():
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= n:
            raise IndexError(f'{what}: index out of range [0, {n}) (got min {lo}, max {hi})')


# ---- mixed requests in one batch: a control (speaker, pace, pitch_mul, pitch_add, denoise strength) is one scalar for the call or one
# value per row.  The library trusts device values (it only clamps), so everything is checked here, on the host, before the upload.
def per_row(value):
    """True when a control is given per row (list / tuple / array / tensor with a dimension) rather than as one scalar."""
    if isinstance(value, (torch.Tensor, np.ndarray)):
        return value.ndim > 0
    return isinstance(value, (list, tuple))


def row_values(value, n, what):
    """A per-row control as a host list of n Python numbers; ValueError when its length is not n."""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu()
    vals = np.asarray(value).reshape(-1).tolist() if isinstance(value, (torch.Tensor, np.ndarray)) else list(value)
    if len(vals) != n:
        raise ValueError(f'{what}: {len(vals)} values for {n} rows')
    return vals


def check_speakers(vals, n_speakers, what='speaker'):
    """IndexError (as nn.Embedding raises) for a speaker outside [0, n_speakers); a single-speaker model ignores the index."""
    for v in vals:
        if isinstance(v, float) and not v.is_integer():
            raise ValueError(f'{what}: {v!r} is not an integer')
        if n_speakers > 1 and not 0 <= int(v) < n_speakers:
            raise IndexError(f'{what} {int(v)} out of range [0, {n_speakers})')


def check_finite(vals, what, positive=False):
    """ValueError for a value that is not finite or, with `positive`, not > 0 (a pace)."""
    for v in vals:
        v = float(v)
        if not np.isfinite(v) or (positive and not v > 0.0):
            raise ValueError(f'{what}: {v!r} is not ' + ('finite and > 0' if positive else 'finite'))


def _rows_f32(vals, device):
    return None if vals is None else torch.tensor([float(v) for v in vals], dtype=torch.float32).to(device)


class _Workspace:
    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf


class HifiGanEngine:
    """Handle over ttsamd_hifigan_* (replaces vocoder.load_hifigan + Generator.forward)."""

    def __init__(self, state_dict, config=None, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        h = dict(HIFIGAN_CONFIG if config is None else config)
        rb = str(h.get('resblock', '1'))
        if rb not in ('1', '2'):
            raise L.TtsAmdError(f'resblock {h.get("resblock")!r}: only "1" (ResBlock1) and "2" (ResBlock2) generators exist')
        cfg = L.HifiGanCfg()
        cfg.resblock = int(rb)
        cfg.num_mels = h.get('num_mels', 80)
        cfg.upsample_initial_channel = h['upsample_initial_channel']
        cfg.n_ups = len(h['upsample_rates'])
        for i, (u, k) in enumerate(zip(h['upsample_rates'], h['upsample_kernel_sizes'])):
            cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
        cfg.n_kernels = len(h['resblock_kernel_sizes'])
        # ResBlock1: every dilation of the list; ResBlock2: the first two (models.py:62-70; the library refuses fewer)
        n_dil = min(len(ds) for ds in h['resblock_dilation_sizes'])
        cfg.n_dilations = min(n_dil, 2) if rb == '2' else len(h['resblock_dilation_sizes'][0])
        for j, (k, ds) in enumerate(zip(h['resblock_kernel_sizes'], h['resblock_dilation_sizes'])):
            cfg.resblock_kernel_sizes[j] = k
            for m, d in enumerate(ds[:cfg.n_dilations] if rb == '2' else ds):
                cfg.resblock_dilations[j][m] = d
        self.hop = int(np.prod(h['upsample_rates']))
        self.num_mels = cfg.num_mels
        arr, keep = L.make_tensors(state_dict)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_hifigan_create(arr, len(arr), C.byref(cfg), C.byref(handle)), 'hifigan_create')
        self.handle = handle
        self.ws = _Workspace()

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_hifigan_destroy(self.handle)
            self.handle = None

    def forward(self, mel, lens=None):
        """mel [B,80,T] float32 on the GPU, lens int64 [B] (device) or None -> wave [B, hop*T].
        Samples past hop*lens[b] are zero."""
        mel = _f32(mel, self.device)
        B, M, T = mel.shape
        assert M == self.num_mels
        if lens is not None:
            lens = lens.to(device=self.device, dtype=torch.int64).contiguous()
        wave = torch.zeros(B, self.hop * T, dtype=torch.float32, device=self.device)
        if T == 0:
            return wave
        with torch.cuda.device(self.device):
            nbytes = self.lib.ttsamd_hifigan_workspace_bytes(self.handle, B, T)
            ws = self.ws.get(nbytes, self.device)
            L.check(self.lib.ttsamd_hifigan_forward(self.handle, _ptr(mel), _ptr(lens), B, T, _ptr(wave), _ptr(ws),
                                                    nbytes, _stream()), 'hifigan_forward')
        return wave


class FastPitchEngine:
    """Handle over ttsamd_fastpitch_* (replaces FastPitch.infer, model.py:351-409)."""

    def __init__(self, state_dict, config=None, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        c = dict(NET_CONFIG if config is None else config)
        self.config = c
        cfg = L.FastPitchCfg()
        cfg.n_mel_channels, cfg.n_symbols, cfg.padding_idx = c['n_mel_channels'], c['n_symbols'], c['padding_idx']
        cfg.d_model = c['symbols_embedding_dim']
        cfg.in_fft_n_layers, cfg.in_fft_n_heads, cfg.in_fft_d_head = c['in_fft_n_layers'], c['in_fft_n_heads'], c['in_fft_d_head']
        cfg.in_fft_kernel, cfg.in_fft_filter = c['in_fft_conv1d_kernel_size'], c['in_fft_conv1d_filter_size']
        cfg.out_fft_n_layers, cfg.out_fft_n_heads, cfg.out_fft_d_head = c['out_fft_n_layers'], c['out_fft_n_heads'], c['out_fft_d_head']
        cfg.out_fft_kernel, cfg.out_fft_filter = c['out_fft_conv1d_kernel_size'], c['out_fft_conv1d_filter_size']
        cfg.dur_kernel, cfg.dur_filter, cfg.dur_n_layers = c['dur_predictor_kernel_size'], c['dur_predictor_filter_size'], c['dur_predictor_n_layers']
        cfg.pitch_kernel, cfg.pitch_filter, cfg.pitch_n_layers = c['pitch_predictor_kernel_size'], c['pitch_predictor_filter_size'], c['pitch_predictor_n_layers']
        cfg.pitch_emb_kernel = c['pitch_embedding_kernel_size']
        cfg.energy_conditioning = int(bool(c['energy_conditioning']))
        cfg.energy_kernel, cfg.energy_filter, cfg.energy_n_layers = c['energy_predictor_kernel_size'], c['energy_predictor_filter_size'], c['energy_predictor_n_layers']
        cfg.energy_emb_kernel = c['energy_embedding_kernel_size']
        cfg.n_speakers, cfg.speaker_emb_weight = c['n_speakers'], float(c['speaker_emb_weight'])
        assert c.get('pitch_conditioning_formants', 1) == 1
        self.d_model, self.n_mel = cfg.d_model, cfg.n_mel_channels
        arr, keep = L.make_tensors(state_dict)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_fastpitch_create(arr, len(arr), C.byref(cfg), C.byref(handle)), 'fastpitch_create')
        self.handle = handle
        self.ws = _Workspace()
        self._alone = False
        # rows padded to 16 bytes (see infer): the library's ragged schedule handles the reference's kernel size 3 only
        self._pad_ok = all(int(c[k]) == 3 for k in ('in_fft_conv1d_kernel_size', 'out_fft_conv1d_kernel_size', 'dur_predictor_kernel_size',
                                                    'pitch_predictor_kernel_size')) and \
            (not c['energy_conditioning'] or int(c['energy_predictor_kernel_size']) == 3)

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_fastpitch_destroy(self.handle)
            self.handle = None

    def set_batch_mode(self, alone):
        """ttsamd_fastpitch_set_batch_mode: how the calls WITHOUT per-row controls treat a batch from now on (False: the reference's padded
        batch; True: every row as if alone).  encode / decode / infer set it from their `alone` argument."""
        if bool(alone) != self._alone:
            L.check(self.lib.ttsamd_fastpitch_set_batch_mode(self.handle, int(bool(alone))), 'fastpitch_set_batch_mode')
            self._alone = bool(alone)

    def encode(self, ids, pace=1.0, dur_tgt=None, pitch_tgt=None, energy_tgt=None, pitch_mul=1.0, pitch_add=0.0, max_duration=75,
               speaker=0, alone=False):
        """Phase A of `infer` (ttsamd_fastpitch_encode / _encode_rows; model.py:355-399 and the integer half of regulate_len), arguments as
        there.  Returns (enc_cond [B,d_model,L] channel-first -- the input of length_regulate --, dur_pred [B,L], pitch_pred [B,1,L],
        energy_pred [B,L] or None, reps int64 [B,L], dec_lens int64 [B]), all on the device; nothing is read back to the host."""
        dev = self.device
        ids = torch.as_tensor(ids).to(device=dev, dtype=torch.int64).contiguous()
        B, Lt = ids.shape
        rows = {k: row_values(v, B, k) if per_row(v) else None
                for k, v in (('pace', pace), ('speaker', speaker), ('pitch_mul', pitch_mul), ('pitch_add', pitch_add))}
        mixed = any(v is not None for v in rows.values())
        if mixed:
            if rows['speaker'] is not None:
                check_speakers(rows['speaker'], int(self.config['n_speakers']))
            if rows['pace'] is not None:
                check_finite(rows['pace'], 'pace', positive=True)
            for k in ('pitch_mul', 'pitch_add'):
                if rows[k] is not None:
                    check_finite(rows[k], k)
            spk_rows = None if rows['speaker'] is None else torch.tensor([int(v) for v in rows['speaker']], dtype=torch.int32).to(dev)
            pace_rows, mul_rows, add_rows = (_rows_f32(rows[k], dev) for k in ('pace', 'pitch_mul', 'pitch_add'))
            speaker, pace = (0 if spk_rows is not None else speaker), (1.0 if pace_rows is not None else pace)
            pitch_mul, pitch_add = (1.0 if mul_rows is not None else pitch_mul), (0.0 if add_rows is not None else pitch_add)
            flags = int(bool(alone))
        else:
            self.set_batch_mode(alone)
        d = self.d_model
        dur_tgt, pitch_tgt, energy_tgt = _f32(dur_tgt, dev), _f32(pitch_tgt, dev), _f32(energy_tgt, dev)
        enc = torch.empty(B, d, Lt, dtype=torch.float32, device=dev)
        dur_pred = torch.empty(B, Lt, dtype=torch.float32, device=dev)
        pitch_pred = torch.empty(B, 1, Lt, dtype=torch.float32, device=dev)
        energy_pred = torch.empty(B, Lt, dtype=torch.float32, device=dev) if self.config['energy_conditioning'] else None
        reps = torch.empty(B, Lt, dtype=torch.int64, device=dev)
        dec_lens = torch.empty(B, dtype=torch.int64, device=dev)
        lib = self.lib
        with torch.cuda.device(dev):
            nb = lib.ttsamd_fastpitch_encode_workspace_bytes(self.handle, B, Lt)
            ws = self.ws.get(nb, dev)
            args = (self.handle, _ptr(ids), B, Lt, int(speaker), float(pace), _ptr(dur_tgt), _ptr(pitch_tgt), _ptr(energy_tgt),
                    float(pitch_mul), float(pitch_add), float(max_duration), _ptr(enc), _ptr(dur_pred), _ptr(pitch_pred),
                    _ptr(energy_pred), _ptr(reps), _ptr(dec_lens), _ptr(ws), nb)
            if mixed:
                L.check(lib.ttsamd_fastpitch_encode_rows(*args, _ptr(spk_rows), _ptr(pace_rows), _ptr(mul_rows), _ptr(add_rows), flags,
                                                         _stream()), 'fastpitch_encode_rows')
            else:
                L.check(lib.ttsamd_fastpitch_encode(*args, _stream()), 'fastpitch_encode')
        return enc, dur_pred, pitch_pred, energy_pred, reps, dec_lens

    def decode(self, x, dec_lens, alone=False, rows=False):
        """Phase B of `infer` (ttsamd_fastpitch_decode; model.py:405-408): x [B,d_model,T] float32 channel-first on the device (the output
        of length_regulate: zero past a row's length; used as scratch and CLOBBERED), dec_lens int64 [B] -> mel [B,80,T], rows exactly as
        wide as x's.  `rows=True`: ttsamd_fastpitch_decode_rows with `alone` as the per-call flag (the phase B of a call with per-row
        controls: the handle's mode is left alone)."""
        dev = self.device
        B, d, T = x.shape
        assert d == self.d_model and x.dtype == torch.float32 and x.is_contiguous() and x.device == dev
        dec_lens = torch.as_tensor(dec_lens).to(device=dev, dtype=torch.int64).contiguous()
        if not rows:
            self.set_batch_mode(alone)
        mel = torch.empty(B, self.n_mel, T, dtype=torch.float32, device=dev)
        if T > 0:
            lib = self.lib
            with torch.cuda.device(dev):
                nb = lib.ttsamd_fastpitch_decode_workspace_bytes(self.handle, B, T)
                ws = self.ws.get(nb, dev)
                args = (self.handle, _ptr(x), _ptr(dec_lens), B, T, _ptr(mel), _ptr(ws), nb)
                if rows:
                    L.check(lib.ttsamd_fastpitch_decode_rows(*args, int(bool(alone)), _stream()), 'fastpitch_decode_rows')
                else:
                    L.check(lib.ttsamd_fastpitch_decode(*args, _stream()), 'fastpitch_decode')
        return mel

    def infer(self, ids, pace=1.0, dur_tgt=None, pitch_tgt=None, energy_tgt=None, pitch_mul=1.0, pitch_add=0.0,
              max_duration=75, speaker=0, return_idx=False, lens_hook=None, alone=False, return_reps=False):
        """Same contract as FastPitch.infer (model.py:351-353) with pitch_transform restricted to
        the affine pitch_trf the reference wrappers install (networks.py:38-42,121-122).
        ids int64 [B,L] zero-padded at the end.  Returns (mel [B,80,T_max], dec_lens int64 [B],
        dur_pred [B,L], pitch_pred [B,1,L], energy_pred [B,L] or None).
        `lens_hook(dec_lens_device) -> host ints [B]` replaces the one device->host read of the call (the
        data-parallel path all-gathers every rank's lengths in that same synchronisation, ttsamd.dp).
        `alone=True`: every row as if it were the only utterance of the call (ttsamd_fastpitch_set_batch_mode 1) -- row b equals
        infer(ids[b:b+1, :len_b]) within fp32 summation order: the reference's batch_size = 1 loop as one ragged call.
        Mixed requests: `pace`, `speaker`, `pitch_mul` and `pitch_add` each take a scalar or B values (list / array / tensor), checked
        on the host (length B, speaker in range, pace finite and > 0: ValueError / IndexError) before they are uploaded.  With any
        per-row control the call runs ttsamd_fastpitch_encode_rows / _decode_rows -- row b's bits are those of the scalar call with row
        b's values -- and `alone` goes down as the per-call flag: the handle's mode is left alone.  All scalars: the route above.
        The two phases are `encode` and `decode`; between them the one host read and the length regulator.
        `return_reps`: the tuple ends with reps int64 [B, L] in HBM, the frames every token got (no launch, no copy more)."""
        dev = self.device
        ids = torch.as_tensor(ids).to(device=dev, dtype=torch.int64).contiguous()
        B, Lt = ids.shape
        mixed = any(per_row(v) for v in (pace, speaker, pitch_mul, pitch_add))
        enc, dur_pred, pitch_pred, energy_pred, reps, dec_lens = self.encode(
            ids, pace=pace, dur_tgt=dur_tgt, pitch_tgt=pitch_tgt, energy_tgt=energy_tgt, pitch_mul=pitch_mul, pitch_add=pitch_add,
            max_duration=max_duration, speaker=speaker, alone=alone)
        d = self.d_model
        # Batches: the DECODER's frame rows padded to a multiple of 4 (16 bytes).  The conv engine's fast paths -- the Winograd F(4,3) kernel,
        # the float4 row epilogue -- need 16-byte-aligned rows, and a real batch's longest utterance is a multiple of 4 one time in four (config
        # 1: three of the four FastPitch calls ran the decoder conv-FF on the direct kernel's per-lane epilogue, 2x the time).  The decoder
        # takes the batch's length from dec_lens, not from the row width (lens_plus1_kernel), so the extra columns are plain padding; mel is
        # returned as a view of the un-padded shape.  (Batch 1 keeps its exact shape: one launch more would cost what alignment gains; the
        # bf16 octet path has no ragged schedule; the encoder's rows stay as given -- the caller's ids tensor IS the reference's padded batch.)
        pad = B >= 2 and self._pad_ok and get_precision() != 'bf16'
        with torch.cuda.device(dev):
            if lens_hook is None:
                t_max0 = int(dec_lens.max().item())     # the reference syncs here too (model.py:76)
            else:
                t_max0 = int(max(lens_hook(dec_lens), default=0))
            t_max = (t_max0 + 3) & ~3 if pad else t_max0
            x = torch.empty(B, d, t_max, dtype=torch.float32, device=dev)
            idx = torch.empty(B, t_max, dtype=torch.int32, device=dev) if return_idx else None
            if t_max > 0:
                L.check(self.lib.ttsamd_length_regulate(_ptr(enc), _ptr(reps), B, Lt, d, t_max, _ptr(x), _ptr(idx), _stream()),
                        'length_regulate')
        mel = self.decode(x, dec_lens, alone=alone, rows=mixed)
        if t_max != t_max0:
            mel = mel[:, :, :t_max0]
            idx = None if idx is None else idx[:, :t_max0]
        out = (mel, dec_lens, dur_pred, pitch_pred, energy_pred)
        out = out + (idx,) if return_idx else out
        return out + (reps,) if return_reps else out        # reps int64 [B, L]: what ttsamd.timing turns into timestamps; last in the tuple


class DenoiserEngine:
    """Handle over ttsamd_denoiser_* (replaces vocoder.hifigan.denoiser.Denoiser)."""

    def __init__(self, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_denoiser_create(C.byref(handle)), 'denoiser_create')
        self.handle = handle
        self.ws = _Workspace()

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_denoiser_destroy(self.handle)
            self.handle = None

    def bias_spec(self, audio):
        """audio [n] (vocoder output for a zero mel) -> |STFT| of frame 0, shape [1, 513, 1]."""
        audio = _f32(audio, self.device).reshape(-1)
        n = audio.numel()
        out = torch.empty(513, dtype=torch.float32, device=self.device)
        n_dev = torch.tensor([n], dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            nb = self.lib.ttsamd_denoiser_workspace_bytes(1, n)
            ws = self.ws.get(nb, self.device)
            L.check(self.lib.ttsamd_denoiser_bias_spec(self.handle, _ptr(audio), _ptr(n_dev), n, _ptr(out), _ptr(ws), nb,
                                                       _stream()), 'denoiser_bias_spec')
        return out.reshape(1, 513, 1)

    def denoise(self, wave, nsamples, bias_spec, strength):
        """wave [B, n_max] (modified in place and returned), nsamples int64 [B] on the device.  `strength`: a scalar, or B values -- then
        a row whose strength is > 0 gets the bits of the scalar call with that value and any other row is left untouched."""
        assert wave.is_contiguous() and wave.dtype == torch.float32
        B, n_max = wave.shape
        rows = None
        if per_row(strength):
            vals = row_values(strength, B, 'denoise strength')
            check_finite(vals, 'denoise strength')
            rows = _rows_f32(vals, self.device)
        nsamples = nsamples.to(device=self.device, dtype=torch.int64).contiguous()
        bias = _f32(bias_spec, self.device).reshape(-1)
        with torch.cuda.device(self.device):
            nb = self.lib.ttsamd_denoiser_workspace_bytes(B, n_max)
            ws = self.ws.get(nb, self.device)
            if rows is not None:
                L.check(self.lib.ttsamd_denoise_rows(self.handle, _ptr(wave), n_max, _ptr(nsamples), B, n_max, _ptr(bias),
                                                     _ptr(rows), _ptr(ws), nb, _stream()), 'denoise_rows')
            else:
                L.check(self.lib.ttsamd_denoise(self.handle, _ptr(wave), n_max, _ptr(nsamples), B, n_max, _ptr(bias),
                                                float(strength), _ptr(ws), nb, _stream()), 'denoise')
        return wave


class MelSpecEngine:
    """Handle over ttsamd_melspec_* (csrc/melspec.hip): wave -> (log-)mel in one launch.  `fbank` [n_mels, 513] (numpy / tensor, copied);
    framing 'same' (reflect pad 384, n // 256 frames) or 'center' (reflect pad 512, n // 256 + 1); mag 'abs' = |X| or 'eps' = sqrt(|X|^2 + 1e-9);
    log_clip > 0: log(max(mel, log_clip)), None / 0: linear."""

    MIN_SAMPLES = {'same': 385, 'center': 513}                 # reflect padding needs more samples than it adds per side

    def __init__(self, fbank, framing='same', mag='abs', log_clip=None, n_fft=1024, hop_length=256, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        if framing not in ('same', 'center') or mag not in ('abs', 'eps'):
            raise L.TtsAmdError(f'MelSpecEngine: framing {framing!r} / mag {mag!r} (same | center, abs | eps)')
        fb = fbank.detach().cpu().numpy() if hasattr(fbank, 'detach') else np.asarray(fbank)
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        if fb.ndim != 2 or fb.shape[1] != n_fft // 2 + 1:
            raise L.TtsAmdError(f'MelSpecEngine: filterbank of shape {fb.shape}, expected [n_mels, {n_fft // 2 + 1}]')
        self.n_mels, self.framing, self.hop = fb.shape[0], framing, int(hop_length)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_melspec_create(fb.ctypes.data_as(C.c_void_p), fb.shape[0], int(n_fft), int(hop_length),
                                                   int(framing == 'center'), int(mag == 'eps'), float(log_clip or 0.0),
                                                   C.byref(handle)), 'melspec_create')
        self.handle = handle

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_melspec_destroy(self.handle)
            self.handle = None

    def frames(self, n):
        return n // self.hop + (self.framing == 'center')

    def forward(self, wave, nsamples=None):
        """wave [B, n_max] float32, nsamples int64 [B] on the device or None (every row n_max long) ->
        (mel [B, n_mels, frames(n_max)], frames int64 [B] on the device).  Row b is the call on wave[b, :nsamples[b]] alone; frames at
        or past a row's own count are zero.  Nothing is read back to the host."""
        wave = _f32(wave, self.device)
        B, n_max = wave.shape
        if nsamples is None:
            nsamples = torch.full((B,), n_max, dtype=torch.int64, device=self.device)
        nsamples = nsamples.to(device=self.device, dtype=torch.int64).contiguous()
        T = self.frames(n_max)
        mel = torch.empty(B, self.n_mels, T, dtype=torch.float32, device=self.device)
        frames = torch.empty(B, dtype=torch.int64, device=self.device)
        if B:
            with torch.cuda.device(self.device):
                L.check(self.lib.ttsamd_melspec_forward(self.handle, _ptr(wave), n_max, _ptr(nsamples), B, T, _ptr(mel), _ptr(frames),
                                                        _stream()), 'melspec_forward')
        return mel, frames


class GriffinLimEngine:
    """ttsamd_griffinlim / ttsamd_mel_to_linear (csrc/griffinlim.hip) with a workspace cache: a linear magnitude -> wave without a
    vocoder.  Only n_fft = win = 1024, hop 256, periodic hann is built; framing 'same' (T frames <-> 256 T samples, T >= 2: the HiFi-GAN
    mel's) or 'center' (T frames <-> 256 (T - 1) samples, T >= 4: torch.stft's).  Specified by its arithmetic (include/ttsamd.h); the
    `center` framing is pinned against torch.stft / torch.istft, parity with a torchaudio release is not (own random init)."""

    MIN_FRAMES = {'same': 2, 'center': 4}                      # the reflect padding (384 / 512 per side) needs more samples than it adds
    INIT = {'zeros': 0, 'hash': 1, 'phase': 2}
    FLOOR = 1e-10

    def __init__(self, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        self.ws = _Workspace()
        self._pinv = {}

    @classmethod
    def samples(cls, frames, framing):
        return 256 * (frames - 1) if framing == 'center' else 256 * frames

    def _frames(self, frames, B, T, framing, what):
        """int32 [B] on the device; counts that still live on the host are checked there (a row below the minimum is refused by name),
        device counts are only clamped by the kernel (such a row is an empty row)"""
        if framing not in self.MIN_FRAMES:
            raise L.TtsAmdError(f"{what}: framing {framing!r}: only 'same' and 'center' are built")
        need = self.MIN_FRAMES[framing]
        if T < need:
            raise L.TtsAmdError(f'{what}: {T} frames, the {framing!r} framing needs at least {need} (reflect padding)')
        if frames is None:
            return torch.full((B,), T, dtype=torch.int32, device=self.device)
        if not (isinstance(frames, torch.Tensor) and frames.device.type != 'cpu'):
            host = np.asarray(frames.numpy() if isinstance(frames, torch.Tensor) else frames).reshape(-1)
            if host.size != B:
                raise L.TtsAmdError(f'{what}: {host.size} frame counts for {B} rows')
            if host.size and (int(host.min()) < need or int(host.max()) > T):
                raise L.TtsAmdError(f'{what}: frame counts {host.tolist()} outside [{need}, {T}]: the {framing!r} framing needs at '
                                    f'least {need} frames (reflect padding)')
            frames = torch.as_tensor(host.astype(np.int32))
        if frames.numel() != B:
            raise L.TtsAmdError(f'{what}: {frames.numel()} frame counts for {B} rows')
        return frames.to(device=self.device, dtype=torch.int32).contiguous()

    def forward(self, mag, frames=None, n_iter=32, momentum=0.99, framing='same', init='hash', seed=0, phase=None, return_phase=False,
                return_inconsistency=False):
        """mag [B, 513, T] float32 (the project's channel-first layout), frames int [B] or None (every row T) -> wave [B, n(T)], zeros
        at and past a row's own length; row b is the call on row b alone, bit for bit.  init 'zeros' | 'hash' | 'phase'; seed: one int
        for every row or one per row (64 bits); phase: complex64 [B, T, 513], the initial angles of init='phase'.  return_phase: also
        the final angles [B, T, 513] complex64 (rows / frames past a row's count are zero); return_inconsistency: also float64 [B],
        || |rebuilt| - mag || / || mag || of the last iteration (NaN for n_iter = 0).  -> wave, or (wave[, phase][, inconsistency])."""
        what = 'GriffinLimEngine.forward'
        mag = _f32(mag, self.device)
        if mag.dim() != 3 or mag.shape[1] != 513:
            raise L.TtsAmdError(f'{what}: mag of shape {tuple(mag.shape)}, expected [B, 513, T] (only n_fft = 1024 is built)')
        B, _, T = mag.shape
        if init not in self.INIT:
            raise L.TtsAmdError(f"{what}: init {init!r} ('zeros' | 'hash' | 'phase')")
        if int(n_iter) != n_iter or n_iter < 0:
            raise L.TtsAmdError(f'{what}: n_iter = {n_iter!r} is not an integer >= 0')
        if not 0.0 <= float(momentum) < 1.0:
            raise L.TtsAmdError(f'{what}: momentum = {momentum!r} outside [0, 1)')
        frames = self._frames(frames, B, T, framing, what)
        if (init == 'phase') != (phase is not None):
            raise L.TtsAmdError(f"{what}: init='phase' and phase= go together (init {init!r}, phase {'given' if phase is not None else 'None'})")
        ph = None
        if phase is not None:
            if tuple(phase.shape) != (B, T, 513) or not torch.is_complex(phase):
                raise L.TtsAmdError(f'{what}: phase of shape {tuple(phase.shape)} / {phase.dtype}, expected complex [B, T, 513] = {(B, T, 513)}')
            ph = torch.view_as_real(phase.to(device=self.device, dtype=torch.complex64)).contiguous().clone()
        elif return_phase:
            ph = torch.zeros(B, T, 513, 2, dtype=torch.float32, device=self.device)
        seed_rows = None
        if per_row(seed):
            vals = [int(v) & 0xFFFFFFFFFFFFFFFF for v in row_values(seed, B, 'seed')]
            seed_rows = torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).to(self.device)
            seed = 0
        n = self.samples(T, framing)
        wave = torch.empty(B, n, dtype=torch.float32, device=self.device)
        inc = torch.empty(B, dtype=torch.float64, device=self.device) if return_inconsistency else None
        if B:
            with torch.cuda.device(self.device):
                nbytes = int(self.lib.ttsamd_griffinlim_workspace_bytes(B, T, float(momentum)))
                if nbytes < 0:
                    raise L.TtsAmdError(f'{what}: a batch of {B} rows of {T} frames is refused (1 .. 65535 rows, 1 .. 2^22 frames)')
                ws = self.ws.get(nbytes, self.device)
                L.check(self.lib.ttsamd_griffinlim(_ptr(mag), _ptr(frames), B, T, int(framing == 'center'), int(n_iter), float(momentum),
                                                   self.INIT[init], _ptr(seed_rows), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(ph), _ptr(wave), n,
                                                   _ptr(inc), _ptr(ws), nbytes, _stream()), 'griffinlim')
        out = (wave,)
        if return_phase:
            out += (torch.view_as_complex(ph),)
        if return_inconsistency:
            out += (inc,)
        return out[0] if len(out) == 1 else out

    def pinv(self, fbank):
        """The pseudo-inverse [513, n_mels] of a filterbank [n_mels, 513], float64 on the host, rounded once to fp32; cached per matrix"""
        fb = fbank.detach().cpu().numpy() if hasattr(fbank, 'detach') else np.asarray(fbank)
        if fb.ndim != 2 or fb.shape[1] != 513 or not 1 <= fb.shape[0] <= 128:
            raise L.TtsAmdError(f'GriffinLimEngine: filterbank of shape {fb.shape}, expected [n_mels <= 128, 513]')
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        key = fb.tobytes()
        if key not in self._pinv:
            self._pinv = {key: torch.from_numpy(np.linalg.pinv(fb.astype(np.float64)).astype(np.float32)).to(self.device).contiguous()}
        return self._pinv[key]

    def mel_to_linear(self, mel, frames=None, log=True, fbank=None):
        """mel [B, n_mels, T] (log=True: the natural log of a clamped mel, as the HiFi-GAN analysis writes it) -> mag [B, 513, T] =
        max(pinv(fbank) exp(mel), 1e-10), zero at and past a row's frame count.  fbank [n_mels, 513]: None = the 80-band mel of
        utils.audio.MelSpectrogram (ttsamd.melfb).  The plain pseudo-inverse: no NNLS refinement."""
        what = 'GriffinLimEngine.mel_to_linear'
        mel = _f32(mel, self.device)
        if mel.dim() != 3:
            raise L.TtsAmdError(f'{what}: mel of shape {tuple(mel.shape)}, expected [B, n_mels, T]')
        B, n_mels, T = mel.shape
        if fbank is None:
            from . import melfb
            fbank = melfb.mel_filterbank(22050, 1024, 80, 0.0, 8000.0, 'slaney', 'slaney')
        P = self.pinv(fbank)
        if P.shape[1] != n_mels:
            raise L.TtsAmdError(f'{what}: mel of {n_mels} bands, filterbank of {P.shape[1]}')
        if frames is None:
            frames = torch.full((B,), T, dtype=torch.int32, device=self.device)
        frames = frames.to(device=self.device, dtype=torch.int32).contiguous() if isinstance(frames, torch.Tensor) else \
            torch.as_tensor(np.asarray(frames, dtype=np.int32)).to(self.device)
        if frames.numel() != B:
            raise L.TtsAmdError(f'{what}: {frames.numel()} frame counts for {B} rows')
        mag = torch.empty(B, 513, T, dtype=torch.float32, device=self.device)
        if B and T:
            with torch.cuda.device(self.device):
                L.check(self.lib.ttsamd_mel_to_linear(_ptr(mel), _ptr(frames), B, n_mels, T, _ptr(P), int(bool(log)), self.FLOOR, _ptr(mag),
                                                      _stream()), 'mel_to_linear')
        return mag


class VocosEngine:
    """Handle over ttsamd_vocos_* (replaces vocoder.vocos.pretrained.MelVocos: '22k' = "same" head, 80 bands; '24k' = "center" head, 100)."""

    def __init__(self, state_dict, config=None, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        c = dict(VOCOS_22K_CONFIG if config is None else config)
        assert c['n_fft'] == 1024 and c['hop_length'] == 256 and c['padding'] in ('same', 'center')
        self.hop, self.n_mels, self.center = c['hop_length'], c['input_channels'], c['padding'] == 'center'
        arr, keep = L.make_tensors(state_dict)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_vocos_create(arr, len(arr), c['input_channels'], c['dim'], c['intermediate_dim'],
                                                 c['num_layers'], C.byref(handle)), 'vocos_create')
            if self.center:
                L.check(self.lib.ttsamd_vocos_set_padding(handle, 1), 'vocos_set_padding')
        self.handle = handle
        self.ws = _Workspace()
        self._bias = None

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_vocos_destroy(self.handle)
            self.handle = None

    def bias_vec(self):
        if self._bias is None:
            out = torch.empty(513, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                nb = self.lib.ttsamd_vocos_workspace_bytes(self.handle, 1, 88)
                ws = self.ws.get(nb, self.device)
                L.check(self.lib.ttsamd_vocos_bias_vec(self.handle, _ptr(out), _ptr(ws), nb, _stream()), 'vocos_bias_vec')
            self._bias = out.reshape(1, 513, 1)
        return self._bias

    def forward(self, mel, lens=None, denoise=0.0):
        """mel [B,n_mels,T] on the GPU, lens int64 [B] or None -> wave [B, 256*T] (zeros past 256*lens[b]); with the "center" head ('24k':
        torch.istft(center=True)) [B, 256*(T-1)], zeros past 256*(lens[b]-1).  `denoise`: a scalar or B values, one per row (row b then
        has the bits of the scalar call with its value)."""
        mel = _f32(mel, self.device)
        B, M, T0 = mel.shape
        assert M == self.n_mels
        rows = None
        if per_row(denoise):
            vals = row_values(denoise, B, 'denoise')
            check_finite(vals, 'denoise')
            rows = _rows_f32(vals, self.device)
        if lens is None:
            lens = torch.full((B,), T0, dtype=torch.int64, device=self.device)
        lens = lens.to(device=self.device, dtype=torch.int64).contiguous()
        n0 = self.hop * (T0 - 1) if self.center else self.hop * T0
        if T0 == 0 or n0 == 0:
            return torch.zeros(B, 0, dtype=torch.float32, device=self.device)
        # frame rows padded to a multiple of 4 (16 bytes): the conv engine's fast paths (the k = 1 GEMM route, float4 row epilogues) need aligned
        # rows and a real T is a multiple of 4 one time in four; every layer reads frames >= lens[b] as zero, so the extra columns change nothing
        T = (T0 + 3) & ~3
        if T != T0:
            mel = torch.nn.functional.pad(mel, (0, T - T0))
        wave = torch.zeros(B, self.hop * T, dtype=torch.float32, device=self.device)
        bias = self.bias_vec().reshape(-1) if rows is not None or denoise != 0 else None
        with torch.cuda.device(self.device):
            nb = self.lib.ttsamd_vocos_workspace_bytes(self.handle, B, T)
            ws = self.ws.get(nb, self.device)
            if rows is not None:
                L.check(self.lib.ttsamd_vocos_forward_rows(self.handle, _ptr(mel), _ptr(lens), B, T, _ptr(rows), _ptr(bias),
                                                           _ptr(wave), _ptr(ws), nb, _stream()), 'vocos_forward_rows')
            else:
                L.check(self.lib.ttsamd_vocos_forward(self.handle, _ptr(mel), _ptr(lens), B, T, float(denoise), _ptr(bias),
                                                      _ptr(wave), _ptr(ws), nb, _stream()), 'vocos_forward')
        return wave if wave.shape[1] == n0 else wave[:, :n0]

    def features(self, mel, lens=None):
        """mel [B, n_mels, T] with T a multiple of 4 (what forward() pads to), lens int64 [B] or None -> head.out's output [B, 1026, T]
        (log-magnitude | phase): the backbone of forward() alone, the same launches and bits."""
        mel = _f32(mel, self.device)
        B, M, T = mel.shape
        assert M == self.n_mels and B >= 1 and T >= 1 and T % 4 == 0
        if lens is None:
            lens = torch.full((B,), T, dtype=torch.int64, device=self.device)
        lens = lens.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty(B, 1026, T, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nb = self.lib.ttsamd_vocos_workspace_bytes(self.handle, B, T)
            ws = self.ws.get(nb, self.device)
            L.check(self.lib.ttsamd_vocos_features(self.handle, _ptr(mel), _ptr(lens), B, T, _ptr(out), _ptr(ws), nb, _stream()),
                    'vocos_features')
        return out

    def head(self, feats, lens=None, denoise=0.0, bias_vec=None):
        """feats [B, 1026, T] (log-magnitude | phase), lens int64 [B] or None -> wave [B, 256 T] ("same") or [B, 256 (T - 1)] ("center"),
        zeros past a row's end: the ISTFT head of forward() alone.  `denoise`: a scalar or B values; `bias_vec` [513]: the engine's own
        when None."""
        feats = _f32(feats, self.device)
        B, C2, T = feats.shape
        assert C2 == 1026 and B >= 1
        rows = None
        if per_row(denoise):
            vals = row_values(denoise, B, 'denoise')
            check_finite(vals, 'denoise')
            rows = _rows_f32(vals, self.device)
        elif denoise != 0:
            check_finite([float(denoise)], 'denoise')
            rows = _rows_f32([float(denoise)] * B, self.device)
        if lens is None:
            lens = torch.full((B,), T, dtype=torch.int64, device=self.device)
        lens = lens.to(device=self.device, dtype=torch.int64).contiguous()
        n0 = self.hop * (T - 1) if self.center else self.hop * T
        if T == 0 or n0 == 0:
            return torch.zeros(B, 0, dtype=torch.float32, device=self.device)
        wave = torch.zeros(B, self.hop * T, dtype=torch.float32, device=self.device)
        bias = None
        if rows is not None:
            bias = (self.bias_vec() if bias_vec is None else _f32(bias_vec, self.device)).reshape(-1)
            assert bias.numel() == 513
        with torch.cuda.device(self.device):
            nb = self.lib.ttsamd_vocos_workspace_bytes(self.handle, B, T)
            ws = self.ws.get(nb, self.device)
            L.check(self.lib.ttsamd_vocos_head(self.handle, _ptr(feats), _ptr(lens), B, T, _ptr(rows), _ptr(bias), _ptr(wave), _ptr(ws),
                                               nb, _stream()), 'vocos_head')
        return wave if wave.shape[1] == n0 else wave[:, :n0]


class Tacotron2Engine:
    """Handle over ttsamd_tacotron2_* (replaces Tacotron2MS.infer, models/tacotron2/tacotron2_ms.py:279-332)."""

    def __init__(self, state_dict, config=None, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        c = dict(TACOTRON2_CONFIG if config is None else config)
        self.config = c
        cfg = L.Tacotron2Cfg()
        for name, _ in L.Tacotron2Cfg._fields_:
            setattr(cfg, name, int(bool(c.get(name, True))) if name == 'decoder_early_stopping' else c[name])
        arr, keep = L.make_tensors(state_dict)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_tacotron2_create(arr, len(arr), C.byref(cfg), C.byref(handle)), 'tacotron2_create')
        self.handle = handle
        self.ws = _Workspace()
        self.n_mels = c['n_mels']
        self.max_decoder_steps = c.get('decoder_max_step', 2000)

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_tacotron2_destroy(self.handle)
            self.handle = None

    def infer(self, tokens, speaker_ids=None, lengths=None, max_step=None, dropout_seed=-1, return_raw=False):
        """tokens int64 [B,L] -> (mel_postnet [B,80,T], mel_lens int32 [B], alignments [B,T,L]);
        dropout_seed None draws a fresh seed per call (the reference's always-on prenet dropout);
        return_raw=True appends the decoder's frames before the postnet, mel_raw [B,80,T]."""
        _check_ids(tokens, self.config['n_symbol'], 'Tacotron2 tokens')
        if speaker_ids is not None and self.config['num_speakers'] > 1:
            _check_ids(speaker_ids, self.config['num_speakers'], 'Tacotron2 speaker_ids')
        tokens = tokens.to(device=self.device, dtype=torch.int64).contiguous()
        B, Ltok = tokens.shape
        if lengths is None:
            lengths = torch.full((B,), Ltok, dtype=torch.int64)
        lengths = lengths.to(device=self.device, dtype=torch.int64).contiguous()
        if self.config['num_speakers'] > 1:
            if speaker_ids is None:
                speaker_ids = torch.zeros(B, dtype=torch.int64)
            speaker_ids = speaker_ids.to(device=self.device, dtype=torch.int64).contiguous()
        else:
            speaker_ids = None
        max_step = int(self.max_decoder_steps if max_step is None else max_step)
        if dropout_seed is None:
            dropout_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        mel_post = torch.zeros(B, self.n_mels, max_step, dtype=torch.float32, device=self.device)
        mel_raw = torch.zeros(B, self.n_mels, max_step, dtype=torch.float32, device=self.device)
        mel_lens = torch.zeros(B, dtype=torch.int32, device=self.device)
        align = torch.zeros(B, max_step, Ltok, dtype=torch.float32, device=self.device)
        n_steps = C.c_int32(0)
        with torch.cuda.device(self.device):
            nb = self.lib.ttsamd_tacotron2_workspace_bytes(self.handle, B, Ltok, max_step)
            ws = self.ws.get(nb, self.device)
            L.check(self.lib.ttsamd_tacotron2_infer(self.handle, _ptr(tokens), _ptr(lengths), _ptr(speaker_ids), B, Ltok,
                                                    max_step, int(dropout_seed), _ptr(mel_post), _ptr(mel_lens),
                                                    _ptr(align), _ptr(mel_raw), C.byref(n_steps), _ptr(ws), nb,
                                                    _stream()), 'tacotron2_infer')
        T = n_steps.value
        if return_raw:
            return mel_post[:, :, :T], mel_lens, align[:, :T], mel_raw[:, :, :T]
        return mel_post[:, :, :T], mel_lens, align[:, :T]

    @property
    def postnet_halo(self):
        """frames an output frame of the postnet reads on each side: ttsamd_tacotron2_postnet_halo_frames (10)"""
        halo = C.c_int32(0)
        L.check(self.lib.ttsamd_tacotron2_postnet_halo_frames(self.handle, C.byref(halo)), 'tacotron2_postnet_halo_frames')
        return halo.value

    def stream(self, tokens, speaker_ids=None, lengths=None, max_step=None, dropout_seed=-1, max_chunk_steps=64, cut_columns=None,
               rows_to_batch_end=False):
        """The decode of infer() as a session of advances -> Tacotron2Stream (advance(n), postnet(t0, t1), mel_raw, alignments,
        mel_lens, steps_done, ended).  Arguments as infer(); max_chunk_steps: the longest advance (a multiple of 8) -- the workspace
        is sized by it, not by max_step; cut_columns (a list or tensor of B ints, < 0 = none): per row the token column of the
        wrapper's end-of-utterance cut, whose causal bound every advance reports (Tacotron2Stream.rows); rows_to_batch_end: rows end
        with the batch (ttmel_single's rule) instead of at their own mel_lens."""
        return Tacotron2Stream(self, tokens, speaker_ids, lengths, max_step, dropout_seed, max_chunk_steps, cut_columns, rows_to_batch_end)


class Tacotron2Stream:
    """One streaming decode (ttsamd_tacotron2_stream_*): `advance(n)` runs n more decoder steps of the loop infer() runs -- the frames
    in mel_raw[:, :, :steps_done], alignments[:, :steps_done] and mel_lens are infer()'s bit for bit --, `postnet(t0, t1)` the postnet
    over a window of final frames.  After every advance: `steps_done`, `ended`, and `rows`, per row (final_frames, row_ended, n_end,
    row_length) as include/ttsamd.h describes them.  The session owns its buffers; close() (or the garbage collector) ends it."""

    def __init__(self, eng, tokens, speaker_ids, lengths, max_step, dropout_seed, max_chunk_steps, cut_columns, rows_to_batch_end):
        _check_ids(tokens, eng.config['n_symbol'], 'Tacotron2 tokens')
        if speaker_ids is not None and eng.config['num_speakers'] > 1:
            _check_ids(speaker_ids, eng.config['num_speakers'], 'Tacotron2 speaker_ids')
        self.eng, self.lib, dev = eng, eng.lib, eng.device
        self._session = None
        tokens = tokens.to(device=dev, dtype=torch.int64).contiguous()
        B, Ltok = tokens.shape
        if lengths is None:
            lengths = torch.full((B,), Ltok, dtype=torch.int64)
        lengths = lengths.to(device=dev, dtype=torch.int64).contiguous()
        if eng.config['num_speakers'] > 1:
            if speaker_ids is None:
                speaker_ids = torch.zeros(B, dtype=torch.int64)
            speaker_ids = speaker_ids.to(device=dev, dtype=torch.int64).contiguous()
        else:
            speaker_ids = None
        max_step = int(eng.max_decoder_steps if max_step is None else max_step)
        max_chunk_steps = int(max_chunk_steps)
        if max_chunk_steps < 8 or max_chunk_steps % 8:
            raise ValueError(f'Tacotron2Engine.stream: max_chunk_steps {max_chunk_steps} must be a positive multiple of 8')
        if dropout_seed is None:
            dropout_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        cols = None
        if cut_columns is not None:
            cols = torch.as_tensor(cut_columns).to(dtype=torch.int32).reshape(-1)
            if cols.numel() != B:
                raise ValueError(f'Tacotron2Engine.stream: cut_columns has {cols.numel()} entries for {B} rows')
            if int(cols.max()) >= Ltok:
                raise ValueError(f'Tacotron2Engine.stream: cut column {int(cols.max())} outside the {Ltok} tokens')
            cols = cols.to(dev).contiguous()
        self.B, self.n_tokens, self.max_step, self.max_chunk_steps = B, Ltok, max_step, max_chunk_steps
        self.halo = eng.postnet_halo
        self._keep = (tokens, lengths, speaker_ids, cols)        # the session reads `lengths` at every advance
        self._mel_raw = torch.zeros(B, eng.n_mels, max_step, dtype=torch.float32, device=dev)
        self._mel_post = torch.zeros(B, eng.n_mels, max_step, dtype=torch.float32, device=dev)
        self.mel_lens = torch.zeros(B, dtype=torch.int32, device=dev)
        self._align = torch.zeros(B, max_step, Ltok, dtype=torch.float32, device=dev)
        self.steps_done, self.ended, self.n_advances = 0, False, 0
        self.rows = [(0, 0, 0, 0)] * B
        self._post_ws = _Workspace()
        session = C.c_void_p()
        with torch.cuda.device(dev):
            nb = self.lib.ttsamd_tacotron2_stream_bytes(eng.handle, B, Ltok, max_step, max_chunk_steps)
            self._ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)       # the session's own: it lives across calls
            L.check(self.lib.ttsamd_tacotron2_stream_begin(eng.handle, _ptr(tokens), _ptr(lengths), _ptr(speaker_ids), B, Ltok, max_step,
                                                           max_chunk_steps, int(dropout_seed), _ptr(cols), int(bool(rows_to_batch_end)),
                                                           _ptr(self._mel_raw), _ptr(self.mel_lens), _ptr(self._align), _ptr(self._ws), nb,
                                                           C.byref(session), _stream()), 'tacotron2_stream_begin')
        self._session = session

    def close(self):
        if getattr(self, '_session', None):
            self.lib.ttsamd_tacotron2_stream_end(self._session)
            self._session = None

    __del__ = close

    @property
    def mel_raw(self):
        """[B, n_mels, steps_done]: the decoder's frames so far, before the postnet"""
        return self._mel_raw[:, :, :self.steps_done]

    @property
    def alignments(self):
        """[B, steps_done, n_tokens]"""
        return self._align[:, :self.steps_done]

    @property
    def mel_post(self):
        """[B, n_mels, steps_done]: valid where postnet() windows have written"""
        return self._mel_post[:, :, :self.steps_done]

    def advance(self, n_steps):
        """n_steps more decoder steps (a multiple of 8, at most max_chunk_steps; clipped to max_step) -> (steps_done, ended).  The
        call waits for them.  ValueError after the session has ended."""
        if self._session is None or self.ended:
            raise ValueError('Tacotron2Stream.advance: the session has ended')
        done, ended = C.c_int32(0), C.c_int32(0)
        rows = (C.c_int32 * (4 * self.B))()
        with torch.cuda.device(self.eng.device):
            L.check(self.lib.ttsamd_tacotron2_stream_advance(self._session, int(n_steps), C.byref(done), C.byref(ended), rows, _stream()),
                    'tacotron2_stream_advance')
        self.steps_done, self.ended = done.value, bool(ended.value)
        self.n_advances += 1
        self.rows = [tuple(rows[4 * b:4 * b + 4]) for b in range(self.B)]
        return self.steps_done, self.ended

    @property
    def final_frames(self):
        """frames [0, n) whose postnet output cannot change any more, for the whole batch: steps_done - halo, or steps_done once ended"""
        return self.steps_done if self.ended else max(self.steps_done - self.halo, 0)

    def postnet(self, t0, t1):
        """mel_post[:, :, t0:t1] -> that view, from the raw frames [t0 - halo, t1 + halo) inside [0, steps_done); the frames must be
        final (t1 <= final_frames), otherwise the library refuses the call."""
        t0, t1 = int(t0), int(t1)
        with torch.cuda.device(self.eng.device):
            nb = self.lib.ttsamd_tacotron2_postnet_window_bytes(self.eng.handle, self.B, max(t1 - t0, 1))
            ws = self._post_ws.get(nb, self.eng.device)
            L.check(self.lib.ttsamd_tacotron2_postnet_window(self.eng.handle, _ptr(self._mel_raw), _ptr(self._mel_post), self.B, self.max_step,
                                                             self.steps_done, t0, t1, int(self.ended), _ptr(ws), nb, _stream()),
                    'tacotron2_postnet_window')
        return self._mel_post[:, :, t0:t1]


class TaggerEngine:
    """Handle over ttsamd_tagger_* (replaces Shakkelha.forward / Shakkala.forward of models/diacritizers)."""

    RENAME = {'emb0.weight': 'emb.weight', 'emb_input.weight': 'emb.weight'}

    def __init__(self, state_dict, config, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        c = dict(config)
        cfg = L.TaggerCfg()
        cfg.n_vocab, cfg.emb_dim = c['n_vocab'], c['emb_dim']
        cfg.n_lstm, cfg.n_dense = len(c['lstm_hidden']), len(c['dense_dim'])
        for i, v in enumerate(c['lstm_hidden']):
            cfg.lstm_hidden[i] = v
        for i, v in enumerate(c['dense_dim']):
            cfg.dense_dim[i] = v
        cfg.hard_sigmoid, cfg.bn_after_lstm0, cfg.bn_eps = c['hard_sigmoid'], c['bn_after_lstm0'], c['bn_eps']
        self.n_classes = c['dense_dim'][-1]
        self.n_vocab = c['n_vocab']
        arr, keep = L.make_tensors({self.RENAME.get(k, k): v for k, v in state_dict.items()})
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_tagger_create(arr, len(arr), C.byref(cfg), C.byref(handle)), 'tagger_create')
        self.handle = handle
        self.ws = _Workspace()

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_tagger_destroy(self.handle)
            self.handle = None

    def forward(self, ids):
        """ids int64 [B, T] -> probs [B, T, n_classes] on the device"""
        ids = torch.as_tensor(ids)
        _check_ids(ids, self.n_vocab, 'tagger ids')
        ids = ids.to(device=self.device, dtype=torch.int64).contiguous()
        B, T = ids.shape
        probs = torch.empty(B, T, self.n_classes, dtype=torch.float32, device=self.device)
        if T == 0:
            return probs
        with torch.cuda.device(self.device):
            nb = self.lib.ttsamd_tagger_workspace_bytes(self.handle, B, T)
            ws = self.ws.get(nb, self.device)
            L.check(self.lib.ttsamd_tagger_forward(self.handle, _ptr(ids), B, T, _ptr(probs), _ptr(ws), nb, _stream()),
                    'tagger_forward')
        return probs


def conv1d(x, w, bias=None, lens=None, dilation=1, in_slope=1.0, relu_out=False, res=None, mode=0, div=1.0, y=None, splitk_floats=None):
    """Kernel-level entry (parity tests / roofline bench): y = act(conv1d(lrelu(x), w) + b [+ res]), 'same' padding;
    mode 1 / 2: y <- y + that / (y + that) / div (the ResBlock sum of HiFi-GAN); res may be y itself (in place).
    `splitk_floats`: the call carries a split-K workspace of that many floats, as the models' convs do (ttsamd_conv1d_splitk; the models
    pass 4 << 20), allocated here for every call and filled with NaN: a reduce that reads a partial sum nobody wrote shows in y.
    last_conv_launch() then tells which kernel ran and in how many slices."""
    lib = _require_gpu()
    x = x.contiguous().float()
    w = w.contiguous().float()
    B, cin, lin = x.shape
    cout, cin2, k = w.shape
    assert cin == cin2
    if y is None:
        y = torch.zeros(B, cout, lin, dtype=torch.float32, device=x.device)
    packed = torch.empty(lib.ttsamd_conv1d_packed_floats(cout, cin, k), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        if splitk_floats is None:
            L.check(lib.ttsamd_conv1d_ex(_ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(lens), B, cin, cout, k, dilation, lin,
                                         float(in_slope), int(relu_out), int(mode), float(div), _ptr(y), _ptr(packed), _stream()), 'conv1d')
        else:
            ws = torch.full((max(int(splitk_floats), 1),), float('nan'), dtype=torch.float32, device=x.device)
            L.check(lib.ttsamd_conv1d_splitk(_ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(lens), B, cin, cout, k, dilation, lin,
                                             float(in_slope), int(relu_out), int(mode), float(div), _ptr(y), _ptr(packed), _ptr(ws),
                                             int(splitk_floats), _stream()), 'conv1d_splitk')
    return y


def last_conv_launch():
    """(route, ksplit) of this thread's last fp32 conv launch (ttsamd_conv_last_launch): route 0 direct kernel, 1 / 2 Winograd F(2,3),
    3 / 4 Winograd F(4,3) on six- / seven-point groups, 5 the all-phase transposed conv, 6 the transposed conv on Winograd F(4,2),
    7 / 8 Winograd F(4,3) on six- / seven-point groups in the packed strip form (dilation 3 / 5; TTSAMD_WINO4 bit 7);
    ksplit = input-channel slices (1: not split)."""
    route, ksplit = C.c_int32(-1), C.c_int32(0)
    L.check(L.load().ttsamd_conv_last_launch(C.byref(route), C.byref(ksplit)), 'conv_last_launch')
    return route.value, ksplit.value


def conv_route(batch, cin, cout, k, lin, dilation=1, in_slope=1.0, relu_out=False, has_res=False, mode=0, splitk_floats=None):
    """(route, ksplit) that last_conv_launch() would report after conv1d() with these shapes and arguments under the current options
    (ttsamd_conv1d_route): asked on the host, nothing is launched and no GPU is needed."""
    route, ksplit = C.c_int32(-1), C.c_int32(0)
    L.check(L.load().ttsamd_conv1d_route(batch, cin, cout, k, dilation, lin, float(in_slope), int(relu_out), int(bool(has_res)), mode,
                                         int(splitk_floats or 0), C.byref(route), C.byref(ksplit)), 'conv1d_route')
    return route.value, ksplit.value


def pair_route(batch, channels, k, lin, dilation=1):
    """What HifiGanEngine.forward launches for the c1 -> c2 pair of a ResBlock1 at a stage of `lin` positions per row under the current
    options (ttsamd_resblock_pair_route; host only, no GPU): {'kernel': 0 two convs | 1 resblock_pair | 2 resblock_pair2 | 3 resblock_pair4,
    'ntw', 'wino_phases' (kernel 2), 'points' (kernel 3), 'name': the TTSAMD_CONV_LOG kind}."""
    kernel, ntw, wm, points, name = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_char_p()
    L.check(L.load().ttsamd_resblock_pair_route(batch, channels, k, dilation, lin, C.byref(kernel), C.byref(ntw), C.byref(wm), C.byref(points),
                                                C.byref(name)), 'resblock_pair_route')
    return {'kernel': kernel.value, 'ntw': ntw.value, 'wino_phases': wm.value, 'points': points.value, 'name': name.value.decode()}


def conv_transpose1d(x, w, bias=None, lens=None, in_slope=1.0, y=None):
    """Kernel-level entry (parity tests): one HiFi-GAN upsampler as the generator launches it (ttsamd_conv_transpose1d),
    y = conv_transpose1d(lrelu(x), w, stride=u, padding=u // 2) + b for w [Cin][Cout][2u] (torch layout); x [B][Cin][L] -> y [B][Cout][L * u];
    row b reads lens[b] inputs and writes lens[b] * u outputs, the rest of `y` stays as given."""
    lib = _require_gpu()
    x = x.contiguous().float()
    w = w.contiguous().float()
    B, cin, lin = x.shape
    cin2, cout, kt = w.shape
    assert cin == cin2 and kt % 2 == 0
    u = kt // 2
    if y is None:
        y = torch.zeros(B, cout, lin * u, dtype=torch.float32, device=x.device)
    assert tuple(y.shape) == (B, cout, lin * u) and y.is_contiguous() and y.dtype == torch.float32
    if lens is not None:
        lens = lens.to(device=x.device, dtype=torch.int64).contiguous()
    packed = torch.empty(max(int(lib.ttsamd_convt_packed_floats(cin, cout, u)), 1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(lib.ttsamd_conv_transpose1d(_ptr(x), _ptr(w), _ptr(bias), _ptr(lens), B, cin, cout, u, lin, float(in_slope), _ptr(y),
                                            _ptr(packed), _stream()), 'conv_transpose1d')
    return y


def resblock_pair(x, w1, b1, w2, b2, dil, lens=None, len_mul=1, y=None, mode=0, div=1.0, slope=0.1, variant=2):
    """Kernel-level entry (parity tests / roofline bench): one fused c1 -> c2 pair of a ResBlock1 in exact fp32,
    v = x + conv1d(lrelu(conv1d(lrelu(x), w1, dilation=dil) + b1), w2) + b2; y = v | y + v | (y + v) / div (mode 0 | 1 | 2)."""
    lib = _require_gpu()
    x = x.contiguous().float()
    w1, w2, b1, b2 = (t.contiguous().float() for t in (w1, w2, b1, b2))
    B, Cc, Lx = x.shape
    k = w1.shape[2]
    assert tuple(w1.shape) == tuple(w2.shape) == (Cc, Cc, k)
    if y is None:
        assert mode == 0
        y = torch.zeros_like(x)
    if lens is not None:
        lens = lens.to(device=x.device, dtype=torch.int64).contiguous()
    n_packed = int(lib.ttsamd_resblock_pair_packed_floats(Cc, k, int(variant)))      # variants 4 / 5: + the convs' Winograd groups
    packed = torch.empty(max(n_packed, 1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(lib.ttsamd_resblock_pair(_ptr(x), _ptr(y), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), Cc, k, int(dil), _ptr(lens),
                                         int(len_mul), Lx, B, int(mode), float(div), float(slope), int(variant), _ptr(packed),
                                         n_packed, _stream()), 'resblock_pair')
    return y


def resblock2(x, w1, b1, w2, b2, dil1, dil2, lens=None, len_mul=1, y=None, mode=0, div=1.0, slope=0.1, variant=2):
    """Kernel-level entry (parity tests / roofline bench): one ResBlock2 in exact fp32,
    x1 = x + conv1d(lrelu(x), w1, dilation=dil1) + b1, v = x1 + conv1d(lrelu(x1), w2, dilation=dil2) + b2;
    y = v | y + v | (y + v) / div (mode 0 | 1 | 2).  variant 1: two single-conv launches, 2: one fused launch."""
    lib = _require_gpu()
    x = x.contiguous().float()
    w1, w2, b1, b2 = (t.contiguous().float() for t in (w1, w2, b1, b2))
    B, Cc, Lx = x.shape
    k = w1.shape[2]
    assert tuple(w1.shape) == tuple(w2.shape) == (Cc, Cc, k)
    if y is None:
        assert mode == 0
        y = torch.zeros_like(x)
    if lens is not None:
        lens = lens.to(device=x.device, dtype=torch.int64).contiguous()
    n_packed = int(lib.ttsamd_resblock2_packed_floats(Cc, k, int(variant)))
    packed = torch.empty(max(n_packed, 1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(lib.ttsamd_resblock2(_ptr(x), _ptr(y), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), Cc, k, int(dil1), int(dil2), _ptr(lens),
                                     int(len_mul), Lx, B, int(mode), float(div), float(slope), int(variant), _ptr(packed), n_packed,
                                     _stream()), 'resblock2')
    return y


def length_regulate(enc, reps, t_max):
    lib = _require_gpu()
    enc = enc.contiguous().float()
    reps = reps.contiguous().to(torch.int64)
    B, Cc, Lt = enc.shape
    out = torch.empty(B, Cc, t_max, dtype=torch.float32, device=enc.device)
    idx = torch.empty(B, t_max, dtype=torch.int32, device=enc.device)
    with torch.cuda.device(enc.device):
        L.check(lib.ttsamd_length_regulate(_ptr(enc), _ptr(reps), B, Lt, Cc, t_max, _ptr(out), _ptr(idx), _stream()),
                'length_regulate')
    return out, idx


# ---- oversmoothing analysis (csrc/oversmooth.hip): plain functions, there is nothing to create ---------------------------------------
OVERSMOOTH_KEYS = ('HQER', 'CSlope', 'CCentroid', 'CRoll95')
OVERSMOOTH_MAX_FRAMES = 4096                                     # TTSAMD_OVERSMOOTH_MAX_FRAMES of include/ttsamd.h
_dtw_ws = _Workspace()


def _dev_f32(t, ndim, what):
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise L.TtsAmdError(f'{what}: expected a tensor on the ROCm device (there is no CPU fallback)')
    if t.dim() != ndim:
        raise L.TtsAmdError(f'{what}: expected {ndim} dimensions, got shape {tuple(t.shape)}')
    return t.to(torch.float32).contiguous()


def _dev_lens(lens, B, T, device):
    if lens is None:
        return torch.full((B,), T, dtype=torch.int64, device=device)
    lens = torch.as_tensor(lens).to(device=device, dtype=torch.int64).contiguous()
    if lens.shape != (B,):
        raise L.TtsAmdError(f'lens of shape {tuple(lens.shape)} for a batch of {B}')
    return lens


def cepstral_series(mel, lens=None, center=True, hann=True, q_c=None, hqer_scale=100.0, return_power=False):
    """mel [B, n_mels, T] on the device (+ lens int64 [B]) -> series [B, 4, T] fp32 in the order OVERSMOOTH_KEYS, one launch
    (ttsamd_cepstral_series).  HQER is scaled by 100 as compute_mel_oversmoothing_metrics reports it; frames past a row's end are zero."""
    lib = _require_gpu()
    mel = _dev_f32(mel, 3, 'cepstral_series: mel')
    B, M, T = mel.shape
    lens = _dev_lens(lens, B, T, mel.device)
    out = torch.empty(B, 4, T, dtype=torch.float32, device=mel.device)
    power = torch.empty(B, M // 2 + 1, T, dtype=torch.float32, device=mel.device) if return_power else None
    if B:
        with torch.cuda.device(mel.device):
            L.check(lib.ttsamd_cepstral_series(_ptr(mel), _ptr(lens), B, M, T, int(bool(center)), int(bool(hann)),
                                               -1 if q_c is None else int(q_c), float(hqer_scale), _ptr(power), _ptr(out), _stream()),
                    'cepstral_series')
    return (out, power) if return_power else out


def cepstral_series_from_power(power, lens=None, q_c=None, q1=1, q2=None, eps=1e-8, roll_p=0.95, hqer_scale=1.0):
    """power [B, Q, T] on the device -> series [B, 4, T] (ttsamd_cepstral_series_from_power): the four measures with the parameters the
    reference's *_from_power functions take."""
    lib = _require_gpu()
    power = _dev_f32(power, 3, 'cepstral_series_from_power: power')
    B, Q, T = power.shape
    lens = _dev_lens(lens, B, T, power.device)
    out = torch.empty(B, 4, T, dtype=torch.float32, device=power.device)
    if B:
        with torch.cuda.device(power.device):
            L.check(lib.ttsamd_cepstral_series_from_power(_ptr(power), _ptr(lens), B, Q, T, -1 if q_c is None else int(q_c), int(q1),
                                                          Q - 1 if q2 is None else int(q2), float(eps), float(roll_p), float(hqer_scale),
                                                          _ptr(out), _stream()), 'cepstral_series_from_power')
    return out


def series_summary(series, lens=None):
    """series [B, K, T] (+ lens [B]) -> (stats [B, K, 3] = count / mean / median of the finite values, feat [B, K, T] = the NaN-interpolated,
    z-scored copy the alignment uses).  One launch (ttsamd_series_summary)."""
    lib = _require_gpu()
    series = _dev_f32(series, 3, 'series_summary: series')
    B, K, T = series.shape
    lens = _dev_lens(lens, B, T, series.device)
    stats = torch.empty(B, K, 3, dtype=torch.float32, device=series.device)
    feat = torch.empty(B, K, T, dtype=torch.float32, device=series.device)
    if B and K:
        with torch.cuda.device(series.device):
            L.check(lib.ttsamd_series_summary(_ptr(series), _ptr(lens), B, K, T, _ptr(stats), _ptr(feat), _stream()), 'series_summary')
    return stats, feat


def dtw(a, b, lens_a=None, lens_b=None, metric='l2', window=None, workspace=None):
    """a [B, M, Ta], b [B, M, Tb] on the device -> (cost [B] fp32, path int32 [B, Ta + Tb, 2] in ascending time, path_len int32 [B]).
    metric 'l2' | 'cosine', window None or the Sakoe-Chiba radius; all fp32, bit-reproducible (ttsamd_dtw).  `workspace`: a uint8 tensor
    to use instead of the module's own (it must hold ttsamd_dtw_workspace_bytes)."""
    lib = _require_gpu()
    a, b = _dev_f32(a, 3, 'dtw: a'), _dev_f32(b, 3, 'dtw: b')
    if a.shape[0] != b.shape[0] or a.shape[1] != b.shape[1]:
        raise L.TtsAmdError(f'dtw: a {tuple(a.shape)} and b {tuple(b.shape)} differ in batch or channels')
    m = str(metric).lower()
    if m not in ('l2', 'cosine'):
        raise L.TtsAmdError(f'dtw: metric {metric!r} (l2 | cosine)')
    B, M, Ta = a.shape
    Tb = b.shape[2]
    lens_a, lens_b = _dev_lens(lens_a, B, Ta, a.device), _dev_lens(lens_b, B, Tb, a.device)
    cost = torch.empty(B, dtype=torch.float32, device=a.device)
    path = torch.empty(B, Ta + Tb, 2, dtype=torch.int32, device=a.device)
    plen = torch.empty(B, dtype=torch.int32, device=a.device)
    if not B:
        return cost, path, plen
    if M < 1:
        raise L.TtsAmdError('dtw: no channels')
    nb = int(lib.ttsamd_dtw_workspace_bytes(B, Ta, Tb, M))
    if nb < 0:
        raise L.TtsAmdError(f'dtw: {Ta} x {Tb} frames, at most {OVERSMOOTH_MAX_FRAMES} per side are built')
    ws = _dtw_ws.get(max(nb, 8), a.device) if workspace is None else workspace
    with torch.cuda.device(a.device):
        L.check(lib.ttsamd_dtw(_ptr(a), _ptr(lens_a), _ptr(b), _ptr(lens_b), B, M, Ta, Tb, int(m == 'cosine'),
                               -1 if window is None else int(window), _ptr(cost), _ptr(path), _ptr(plen), _ptr(ws),
                               nb if workspace is None else int(ws.numel() * ws.element_size()), _stream()), 'dtw')
    return cost, path, plen


def dtw_aligned_mae(pred, ref, path, path_len):
    """pred [B, Ta], ref [B, Tb], path / path_len of dtw() -> mae [B] = mean |pred[i] - ref[j]| along the path (ttsamd_dtw_aligned_mae)."""
    lib = _require_gpu()
    pred, ref = _dev_f32(pred, 2, 'dtw_aligned_mae: pred'), _dev_f32(ref, 2, 'dtw_aligned_mae: ref')
    B, Ta = pred.shape
    Tb = ref.shape[1]
    if ref.shape[0] != B or tuple(path.shape) != (B, Ta + Tb, 2) or path.dtype != torch.int32 or path_len.dtype != torch.int32:
        raise L.TtsAmdError(f'dtw_aligned_mae: pred {tuple(pred.shape)}, ref {tuple(ref.shape)}, path {tuple(path.shape)} do not belong together')
    mae = torch.empty(B, dtype=torch.float32, device=pred.device)
    if B:
        with torch.cuda.device(pred.device):
            L.check(lib.ttsamd_dtw_aligned_mae(_ptr(pred), _ptr(ref), B, Ta, Tb, _ptr(path.contiguous()), _ptr(path_len.contiguous()),
                                               _ptr(mae), _stream()), 'dtw_aligned_mae')
    return mae


def oversmoothing_score(mel_pred, lens_pred, mel_ref, lens_ref, center=True, hann=True, q_c=None):
    """The paper's comparison of a batch on the device: mel_pred [B, n_mels, Tp], mel_ref [B, n_mels, Tr] (+ lens, None = full rows) ->
    (series_pred [B, 4, Tp], series_ref [B, 4, Tr], {mae_<k>, delta_u_<k>: [B] tensors for k in OVERSMOOTH_KEYS}).
    mae_<k>: the two series of key k aligned by DTW on their NaN-interpolated z-scores (L2, no band), mean |difference| of the ORIGINAL
    series along the path; delta_u_<k>: median(pred) - median(ref) over the finite frames.  Seven launches (2 series, 2 summaries, DTW of
    the 4 B series pairs, the aligned error, one subtraction), nothing is read back to the host in between."""
    mel_pred, mel_ref = _dev_f32(mel_pred, 3, 'oversmoothing_score: mel_pred'), _dev_f32(mel_ref, 3, 'oversmoothing_score: mel_ref')
    if mel_pred.shape[:2] != mel_ref.shape[:2]:
        raise L.TtsAmdError(f'oversmoothing_score: prediction {tuple(mel_pred.shape)} and reference {tuple(mel_ref.shape)} differ in batch '
                            'or band count')
    B, _, Tp = mel_pred.shape
    Tr = mel_ref.shape[2]
    lens_pred, lens_ref = _dev_lens(lens_pred, B, Tp, mel_pred.device), _dev_lens(lens_ref, B, Tr, mel_pred.device)
    sp = cepstral_series(mel_pred, lens_pred, center, hann, q_c)
    sr = cepstral_series(mel_ref, lens_ref, center, hann, q_c)
    stp, fp = series_summary(sp, lens_pred)
    st_r, fr = series_summary(sr, lens_ref)
    _, path, plen = dtw(fp.view(B * 4, 1, Tp), fr.view(B * 4, 1, Tr), lens_pred.repeat_interleave(4), lens_ref.repeat_interleave(4))
    mae = dtw_aligned_mae(sp.view(B * 4, Tp), sr.view(B * 4, Tr), path, plen).view(B, 4)
    delta = stp[:, :, 2] - st_r[:, :, 2]
    out = {}
    for k, name in enumerate(OVERSMOOTH_KEYS):
        out[f'mae_{name}'] = mae[:, k]
        out[f'delta_u_{name}'] = delta[:, k]
    return sp, sr, out


# ---- objective evaluation (csrc/objective.hip): MCD, mel error, F0 and voicing errors along a DTW path ---------------------------------
OBJECTIVE_KEYS = ('n', 'mcd', 'mel_mae', 'n_vv', 'f0_rmse_cents', 'f0_rmse_hz', 'f0_corr', 'vuv_error')   # TTSAMD_EVAL_STATS = 8
MCD_SCALE = 10.0 * np.sqrt(2.0) / np.log(10.0)                   # cepstral distance of natural-log mels -> dB
MEL_CEPSTRUM_MAX_MELS, MEL_CEPSTRUM_MAX_COEF = 128, 64


def mel_cepstrum(logmel, lens=None, n_coef=13):
    """logmel [B, n_mels, T] on the device (+ lens int64 [B]) -> cep [B, n_coef, T] fp32: the orthonormal DCT-II across the bands of
    every frame (scipy.fft.dct(type=2, norm='ortho')[:n_coef]), float64 inside, rounded once; frames past a row's end are zero.  One
    launch (ttsamd_mel_cepstrum)."""
    lib = _require_gpu()
    logmel = _dev_f32(logmel, 3, 'mel_cepstrum: logmel')
    B, M, T = logmel.shape
    if not 1 <= M <= MEL_CEPSTRUM_MAX_MELS:
        raise L.TtsAmdError(f'mel_cepstrum: {M} bands; 1 to {MEL_CEPSTRUM_MAX_MELS} are built')
    if int(n_coef) != n_coef or not 1 <= n_coef <= min(M, MEL_CEPSTRUM_MAX_COEF):
        raise L.TtsAmdError(f'mel_cepstrum: n_coef = {n_coef!r}; 1 to min(n_mels = {M}, {MEL_CEPSTRUM_MAX_COEF}) coefficients are built')
    lens = _dev_lens(lens, B, T, logmel.device)
    cep = torch.empty(B, int(n_coef), T, dtype=torch.float32, device=logmel.device)
    if B:
        with torch.cuda.device(logmel.device):
            L.check(lib.ttsamd_mel_cepstrum(_ptr(logmel), _ptr(lens), B, M, T, int(n_coef), _ptr(cep), _stream()), 'mel_cepstrum')
    return cep


def identity_path(lens_a, lens_b, ta_max, tb_max):
    """The frame-by-frame comparison in ttsamd_dtw's layout: (path int32 [B, ta_max + tb_max, 2], path_len int32 [B]) with
    min(lens_a[b], lens_b[b]) steps (p, p) and zeros past them (lengths clamped to the padded sizes).  torch ops on the device, no host
    read."""
    if not isinstance(lens_a, torch.Tensor) or lens_a.device.type != 'cuda':
        raise L.TtsAmdError('identity_path: lens_a must be a tensor on the ROCm device')
    la = lens_a.to(torch.int64).clamp(0, int(ta_max))
    lb = torch.as_tensor(lens_b).to(device=la.device, dtype=torch.int64).clamp(0, int(tb_max))
    if la.dim() != 1 or la.shape != lb.shape:
        raise L.TtsAmdError(f'identity_path: lens of shapes {tuple(la.shape)} and {tuple(lb.shape)}')
    n = torch.minimum(la, lb)
    p = torch.arange(int(ta_max) + int(tb_max), dtype=torch.int64, device=la.device)[None]
    path = torch.where(p < n[:, None], p, torch.zeros_like(p)).to(torch.int32)
    return path[:, :, None].expand(-1, -1, 2).contiguous(), n.to(torch.int32)


def dtw_aligned_eval(cep_a, cep_b, path, path_len, mel_a=None, mel_b=None, f0_a=None, f0_b=None, first_coef=1, scale=MCD_SCALE):
    """cep_a [B, C, Ta], cep_b [B, C, Tb], path / path_len of dtw() (or identity_path) -> stats float64 [B, 8] in the order
    OBJECTIVE_KEYS: along the path, scale x the mean Euclidean distance over coefficients first_coef .. C - 1 (mcd), the mean |difference|
    of mel_a [B, M, Ta] / mel_b [B, M, Tb] (NaN without them) and, from f0_a [B, Ta] / f0_b [B, Tb] in Hz (voiced = finite and > 0; NaN
    without them), the count of steps voiced on both sides, the RMSE in cents and in Hz and the Pearson correlation over those steps, and
    the share of steps that differ in voicing.  One launch (ttsamd_dtw_aligned_eval); a row equals the call on its pair alone."""
    lib = _require_gpu()
    cep_a, cep_b = _dev_f32(cep_a, 3, 'dtw_aligned_eval: cep_a'), _dev_f32(cep_b, 3, 'dtw_aligned_eval: cep_b')
    B, Cc, Ta = cep_a.shape
    Tb = cep_b.shape[2]
    if cep_b.shape[0] != B or cep_b.shape[1] != Cc:
        raise L.TtsAmdError(f'dtw_aligned_eval: cep_a {tuple(cep_a.shape)} and cep_b {tuple(cep_b.shape)} differ in batch or coefficients')
    if (not isinstance(path, torch.Tensor) or tuple(path.shape) != (B, Ta + Tb, 2) or path.dtype != torch.int32
            or tuple(path_len.shape) != (B,) or path_len.dtype != torch.int32):
        raise L.TtsAmdError(f'dtw_aligned_eval: cep_a {tuple(cep_a.shape)}, cep_b {tuple(cep_b.shape)} and the path do not belong together '
                            f'(int32 [{B}, {Ta + Tb}, 2] and int32 [{B}] are what dtw() returns)')
    if int(first_coef) != first_coef or not 0 <= first_coef < max(Cc, 1):
        raise L.TtsAmdError(f'dtw_aligned_eval: first_coef = {first_coef!r} outside [0, {Cc})')
    if (mel_a is None) != (mel_b is None) or (f0_a is None) != (f0_b is None):
        raise L.TtsAmdError('dtw_aligned_eval: mel_a / mel_b (and f0_a / f0_b) come as a pair or not at all')
    M = 0
    if mel_a is not None:
        mel_a, mel_b = _dev_f32(mel_a, 3, 'dtw_aligned_eval: mel_a'), _dev_f32(mel_b, 3, 'dtw_aligned_eval: mel_b')
        M = mel_a.shape[1]
        if tuple(mel_a.shape) != (B, M, Ta) or tuple(mel_b.shape) != (B, M, Tb):
            raise L.TtsAmdError(f'dtw_aligned_eval: mel_a {tuple(mel_a.shape)} / mel_b {tuple(mel_b.shape)} for cepstra of {Ta} / {Tb} '
                                f'frames in a batch of {B}')
    if f0_a is not None:
        f0_a, f0_b = _dev_f32(f0_a, 2, 'dtw_aligned_eval: f0_a'), _dev_f32(f0_b, 2, 'dtw_aligned_eval: f0_b')
        if tuple(f0_a.shape) != (B, Ta) or tuple(f0_b.shape) != (B, Tb):
            raise L.TtsAmdError(f'dtw_aligned_eval: f0_a {tuple(f0_a.shape)} / f0_b {tuple(f0_b.shape)} for cepstra of {Ta} / {Tb} frames '
                                f'in a batch of {B}')
    stats = torch.empty(B, len(OBJECTIVE_KEYS), dtype=torch.float64, device=cep_a.device)
    if B:
        with torch.cuda.device(cep_a.device):
            L.check(lib.ttsamd_dtw_aligned_eval(_ptr(cep_a), _ptr(cep_b), Cc, int(first_coef), _ptr(mel_a), _ptr(mel_b), M, _ptr(f0_a),
                                                _ptr(f0_b), B, Ta, Tb, _ptr(path.contiguous()), _ptr(path_len.contiguous()), float(scale),
                                                _ptr(stats), _stream()), 'dtw_aligned_eval')
    return stats


def objective_score(mel_pred, lens_pred, mel_ref, lens_ref, f0_pred=None, f0_ref=None, n_coef=13, align='dtw', window=None):
    """The objective scores of a batch on the device: log-mels mel_pred [B, n_mels, Tp], mel_ref [B, n_mels, Tr] (+ lens, None = full
    rows), f0 tracks [B, Tp] / [B, Tr] in Hz or None -> {key: float64 [B] for key in OBJECTIVE_KEYS, 'path', 'path_len'[, 'dtw_cost']}.
    align 'dtw': the two sides' cepstra 1 .. n_coef - 1 aligned by dtw() (L2; `window` = Sakoe-Chiba radius or None); 'frames': frame p
    against frame p over the shorter side.  Four launches with 'dtw' (two cepstra, DTW, the evaluation); nothing is read back to the
    host."""
    mel_pred, mel_ref = _dev_f32(mel_pred, 3, 'objective_score: mel_pred'), _dev_f32(mel_ref, 3, 'objective_score: mel_ref')
    if mel_pred.shape[:2] != mel_ref.shape[:2]:
        raise L.TtsAmdError(f'objective_score: prediction {tuple(mel_pred.shape)} and reference {tuple(mel_ref.shape)} differ in batch '
                            'or band count')
    if align not in ('dtw', 'frames'):
        raise L.TtsAmdError(f"objective_score: align {align!r} ('dtw' | 'frames')")
    B, M, Tp = mel_pred.shape
    Tr = mel_ref.shape[2]
    if max(Tp, Tr) > OVERSMOOTH_MAX_FRAMES:
        raise L.TtsAmdError(f'objective_score: {Tp} x {Tr} frames, at most {OVERSMOOTH_MAX_FRAMES} per side are built')
    if int(n_coef) != n_coef or not 1 <= n_coef <= min(M, MEL_CEPSTRUM_MAX_COEF):
        raise L.TtsAmdError(f'objective_score: n_coef = {n_coef!r}; 1 to min(n_mels = {M}, {MEL_CEPSTRUM_MAX_COEF}) coefficients are built')
    if align == 'dtw' and n_coef < 2:
        raise L.TtsAmdError("objective_score: align='dtw' aligns the coefficients 1 .. n_coef - 1 and needs n_coef >= 2")
    lens_pred, lens_ref = _dev_lens(lens_pred, B, Tp, mel_pred.device), _dev_lens(lens_ref, B, Tr, mel_pred.device)
    cp, cr = mel_cepstrum(mel_pred, lens_pred, n_coef), mel_cepstrum(mel_ref, lens_ref, n_coef)
    out = {}
    if align == 'dtw':
        out['dtw_cost'], path, plen = dtw(cp[:, 1:], cr[:, 1:], lens_pred, lens_ref, 'l2', window)
    else:
        path, plen = identity_path(lens_pred, lens_ref, Tp, Tr)
    stats = dtw_aligned_eval(cp, cr, path, plen, mel_pred, mel_ref, f0_pred, f0_ref, first_coef=min(1, n_coef - 1))
    for k, name in enumerate(OBJECTIVE_KEYS):
        out[name] = stats[:, k]
    out['path'], out['path_len'] = path, plen
    return out


def _fit_width(x, width):
    """[B, T] -> [B, width]: trimmed at the end or zero-padded, as FastPitch.pitch_track(mel_len=) fits a track to its mel"""
    return torch.nn.functional.pad(x, (0, int(width) - x.shape[1]))


class ObjectiveEngine:
    """Wave against wave at 22 050 Hz: owns the reference's log-mel analysis (80-band slaney filterbank, 'same' framing, sqrt(|X|^2 +
    1e-9), log(max(., 1e-5)): utils/audio.py of the reference with its safe log) and its pYIN settings (C2 .. C7, frames of 1024 every
    256 samples: scripts/extract_f0.py), and scores with objective_score."""

    def __init__(self, device='cuda'):
        from . import melfb
        _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        fb = melfb.mel_filterbank(22050, 1024, 80, 0, 8000.0, 'slaney', 'slaney')
        self.melspec = MelSpecEngine(fb, 'same', 'eps', 1e-5, device=self.device)
        c2, c7 = 440.0 * 2.0 ** ((36 - 69) / 12.0), 440.0 * 2.0 ** ((96 - 69) / 12.0)
        self.pyin = PyinEngine(c2, c7, device=self.device, sr=22050, frame_length=1024, hop_length=256)

    def features(self, wave, nsamples=None):
        """wave [B, n] (+ nsamples int64 [B]) -> (logmel [B, 80, n // 256], frames int64 [B], f0 [B, n // 256] in Hz, 0 where unvoiced):
        the track (1 + n // 256 frames) is fitted to the mel's width, trimmed at the end; no score reads a frame at or past `frames`."""
        wave = _f32(wave, self.device)
        if wave.dim() != 2:
            raise L.TtsAmdError(f'ObjectiveEngine: wave of shape {tuple(wave.shape)}, expected [B, n]')
        if wave.shape[1] < MelSpecEngine.MIN_SAMPLES['same']:
            raise L.TtsAmdError(f'ObjectiveEngine: rows of {wave.shape[1]} samples; the mel analysis needs at least '
                                f'{MelSpecEngine.MIN_SAMPLES["same"]} (reflect padding)')
        mel, frames = self.melspec.forward(wave, nsamples)
        f0, _, _, _ = self.pyin.forward(wave, nsamples)
        return mel, frames, _fit_width(f0, mel.shape[2])

    def score_waves(self, wave_pred, n_pred, wave_ref, n_ref, **kw):
        """wave_pred [B, n], wave_ref [B, n'] (+ samples per row, int64 [B] or None) -> objective_score(...) of their log-mels and pYIN
        tracks plus 'lens_pred' / 'lens_ref' (mel frames per row); **kw: n_coef, align, window.  Nothing is read back to the host."""
        mp, lp, fp = self.features(wave_pred, n_pred)
        mr, lr, fr = self.features(wave_ref, n_ref)
        if mp.shape[0] != mr.shape[0]:
            raise L.TtsAmdError(f'ObjectiveEngine.score_waves: {mp.shape[0]} predictions against {mr.shape[0]} recordings')
        out = objective_score(mp, lp, mr, lr, fp, fr, **kw)
        out['lens_pred'], out['lens_ref'] = lp, lr
        return out


# ---- FastPitch forced alignment (csrc/aligner.hip) ------------------------------------------------------------------------------------
MAS_MAX_TOKENS = 1024                                            # TTSAMD_MAS_MAX_TOKENS of include/ttsamd.h
ALIGNER_KEYS = ('encoder.word_emb.weight',) + tuple(
    f'attention.{proj}.{i}.conv.{p}' for proj, idx in (('key_proj', (0, 2)), ('query_proj', (0, 2, 4))) for i in idx for p in ('weight', 'bias'))
_mas_ws = _Workspace()


def mas(log_attn, in_lens, out_lens, is_log=True, return_hard=True, workspace=None):
    """Monotonic alignment search on the device (ttsamd_mas; the reference's mas_width1 bit for bit, one block per utterance).
    log_attn [B, T, L] or [B, 1, T, L] fp32 on the device (is_log=False: probabilities, their fp32 log is taken first), in_lens / out_lens
    [B] -> (dur [B, L] fp32, attn_hard in the shape of log_attn, or None with return_hard=False).  in_lens[b] == 1 assigns every frame to
    token 0 (the reference indexes out of bounds there)."""
    lib = _require_gpu()
    if not isinstance(log_attn, torch.Tensor) or log_attn.device.type != 'cuda':
        raise L.TtsAmdError('mas: expected a tensor on the ROCm device (there is no CPU fallback)')
    shape = tuple(log_attn.shape)
    if log_attn.dim() == 4 and shape[1] == 1:
        a = log_attn[:, 0]
    elif log_attn.dim() == 3:
        a = log_attn
    else:
        raise L.TtsAmdError(f'mas: expected [B, T, L] or [B, 1, T, L], got shape {shape}')
    a = a.to(torch.float32).contiguous()
    B, T, Lt = a.shape
    if Lt > MAS_MAX_TOKENS:
        raise L.TtsAmdError(f'mas: {Lt} tokens, at most {MAS_MAX_TOKENS} are built (TTSAMD_MAS_MAX_TOKENS)')
    in_lens, out_lens = _dev_lens(in_lens, B, Lt, a.device), _dev_lens(out_lens, B, T, a.device)
    dur = torch.empty(B, Lt, dtype=torch.float32, device=a.device)
    hard = torch.empty(B, T, Lt, dtype=torch.float32, device=a.device) if return_hard else None
    if B and Lt:
        nb = int(lib.ttsamd_mas_workspace_bytes(B, T, Lt))
        ws = _mas_ws.get(max(nb, 8), a.device) if workspace is None else workspace
        with torch.cuda.device(a.device):
            L.check(lib.ttsamd_mas(_ptr(a), int(bool(is_log)), _ptr(in_lens), _ptr(out_lens), B, T, Lt, _ptr(dur), _ptr(hard), _ptr(ws),
                                   nb if workspace is None else int(ws.numel() * ws.element_size()), _stream()), 'mas')
    return dur, (hard.view(shape) if return_hard else None)


def average_pitch(pitch, durs):
    """The reference's average_pitch (model.py:93-111) on the device: pitch [B, F, T], durs [B, L] -> [B, F, L] fp32, per token the mean of
    the non-zero values of its frames, 0 where there is none (ttsamd_average_pitch)."""
    lib = _require_gpu()
    pitch = _dev_f32(pitch, 3, 'average_pitch: pitch')
    durs = _dev_f32(durs, 2, 'average_pitch: durs')
    B, F, T = pitch.shape
    if durs.shape[0] != B:
        raise L.TtsAmdError(f'average_pitch: pitch {tuple(pitch.shape)} and durs {tuple(durs.shape)} differ in batch')
    Lt = durs.shape[1]
    out = torch.empty(B, F, Lt, dtype=torch.float32, device=pitch.device)
    if B and F and Lt:
        with torch.cuda.device(pitch.device):
            L.check(lib.ttsamd_average_pitch(_ptr(pitch), _ptr(durs), B, F, T, Lt, _ptr(out), _stream()), 'average_pitch')
    return out


class AlignerEngine:
    """Handle over ttsamd_aligner_* (replaces the aligner path of FastPitch.forward, model.py:298-318): `state_dict` holds
    encoder.word_emb.weight and the attention.key_proj.* / attention.query_proj.* tensors under their reference names."""

    def __init__(self, state_dict, config=None, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        c = dict(NET_CONFIG if config is None else config)
        missing = [k for k in ALIGNER_KEYS if k not in state_dict]
        if missing:
            raise L.TtsAmdError(f'the checkpoint holds no aligner: missing {", ".join(missing)}')
        cfg = L.AlignerCfg()
        cfg.n_mel, cfg.d_text = c['n_mel_channels'], c['symbols_embedding_dim']
        cfg.n_att = int(np.asarray(state_dict['attention.key_proj.2.conv.bias']).shape[0])
        cfg.n_symbols, cfg.padding_idx = c['n_symbols'], c['padding_idx']
        self.n_mel, self.n_symbols, self.padding_idx = cfg.n_mel, cfg.n_symbols, cfg.padding_idx
        arr, keep = L.make_tensors({k: state_dict[k] for k in ALIGNER_KEYS})
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_aligner_create(arr, len(arr), C.byref(cfg), C.byref(handle)), 'aligner_create')
        self.handle = handle
        self.ws = _Workspace()

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_aligner_destroy(self.handle)
            self.handle = None

    def attention(self, ids, mel, attn_prior=None, in_lens=None, mel_lens=None):
        """ConvAttention.forward on the padded batch: ids int64 [B, L], mel [B, n_mel, T], attn_prior [B, T, L] or None ->
        (attn_soft, attn_logprob), both [B, 1, T, L]; in_lens None = the count of non-padding ids per row.  attn_prior 'interpolated' /
        'exact': the beta-binomial prior of the rows' own lengths (in_lens, mel_lens; None: T frames each), built on the device by
        attention_prior."""
        dev = self.device
        ids = torch.as_tensor(ids)
        _check_ids(ids, self.n_symbols, 'aligner ids')
        ids = ids.to(device=dev, dtype=torch.int64).contiguous()
        mel = _f32(mel, dev)
        B, Lt = ids.shape
        if mel.dim() != 3 or mel.shape[0] != B or mel.shape[1] != self.n_mel:
            raise L.TtsAmdError(f'aligner: mel of shape {tuple(mel.shape)} for {B} rows of {self.n_mel} bands')
        T = mel.shape[2]
        if Lt > MAS_MAX_TOKENS:
            raise L.TtsAmdError(f'aligner: {Lt} tokens, at most {MAS_MAX_TOKENS} are built (TTSAMD_MAS_MAX_TOKENS)')
        in_lens = (ids != self.padding_idx).sum(1) if in_lens is None else _dev_lens(in_lens, B, Lt, dev)
        if isinstance(attn_prior, str):
            attn_prior = attention_prior(in_lens, _dev_lens(mel_lens, B, T, dev), n_tokens=Lt, n_frames=T, mode=attn_prior, device=dev)
        prior = _f32(attn_prior, dev)
        if prior is not None and tuple(prior.shape) != (B, T, Lt):
            raise L.TtsAmdError(f'aligner: attn_prior of shape {tuple(prior.shape)}, expected {(B, T, Lt)}')
        soft = torch.empty(B, 1, T, Lt, dtype=torch.float32, device=dev)
        logprob = torch.empty(B, 1, T, Lt, dtype=torch.float32, device=dev)
        if B and T and Lt:
            with torch.cuda.device(dev):
                nb = self.lib.ttsamd_aligner_workspace_bytes(self.handle, B, Lt, T)
                ws = self.ws.get(nb, dev)
                L.check(self.lib.ttsamd_aligner_forward(self.handle, _ptr(ids), _ptr(in_lens), _ptr(mel), None, _ptr(prior), B, Lt, T,
                                                        _ptr(soft), _ptr(logprob), _ptr(ws), nb, _stream()), 'aligner_forward')
        return soft, logprob, in_lens

    def align(self, ids, mel, mel_lens=None, attn_prior=None, return_attn=False):
        """ids int64 [B, L] zero-padded at the end, mel [B, n_mel, T], mel_lens [B] (None: every row T frames) -> dur [B, L] fp32, the
        frames MAS gives each token (model.py:306-314); with return_attn also attn_soft, attn_hard, attn_logprob, each [B, 1, T, L].
        Two launches of this file's own plus the encoders' six; nothing is read back to the host."""
        soft, logprob, in_lens = self.attention(ids, mel, attn_prior, mel_lens=mel_lens)
        B, _, T, Lt = soft.shape
        mel_lens = _dev_lens(mel_lens, B, T, self.device)
        dur, hard = mas(soft, in_lens, mel_lens, is_log=False, return_hard=return_attn)
        return (dur, soft, hard, logprob) if return_attn else dur


# ---- the alignment prior and the alignment scores (csrc/attn_loss.hip) ----------------------------------------------------------------
PRIOR_MODES = {'exact': 0, 'interpolated': 1}
_PRIOR_F64 = 2                                                   # TTSAMD_ATTN_PRIOR_F64 of include/ttsamd.h
_ctc_ws = _Workspace()


def attn_prior_tables(n):
    """lf[k] = log k! for k < n, float64: the table csrc/attn_loss.hip builds on the host (std::lgamma) and uploads for the prior
    (ttsamd_attn_prior_tables; no GPU is needed)."""
    lf = np.zeros(int(n), dtype=np.float64)
    L.check(L.load().ttsamd_attn_prior_tables(int(n), lf.ctypes.data_as(C.c_void_p)), 'attn_prior_tables')
    return lf


def _host_max(lens):
    return int(torch.as_tensor(lens).max()) if torch.as_tensor(lens).numel() else 0


def attention_prior(in_lens, mel_lens, n_tokens=None, n_frames=None, mode='interpolated', scaling=1.0, dtype=torch.float32, device='cuda'):
    """The aligner's beta-binomial prior on the device (ttsamd_attn_prior, one launch): in_lens / mel_lens [B] -> [B, n_frames, n_tokens]
    (None: the longest row; given sizes save the read-back of the lengths), row b's [mel_lens[b], in_lens[b]] corner filled and zero
    outside it, as TTSCollate pads.  mode 'interpolated': what the reference's BetaBinomialInterpolator()(mel_len, in_len) returns, the
    prior the checkpoints were trained with; 'exact': beta_binomial_prior_distribution(in_len, mel_len).  float64 arithmetic, rounded
    once to `dtype` (torch.float32, or torch.float64 for the values before that rounding).  Only scaling = 1 is built."""
    lib = _require_gpu()
    if mode not in PRIOR_MODES:
        raise L.TtsAmdError(f"attention_prior: mode {mode!r}: 'interpolated' and 'exact' are built")
    if dtype not in (torch.float32, torch.float64):
        raise L.TtsAmdError(f'attention_prior: dtype {dtype}: torch.float32 and torch.float64 are built')
    dev = torch.device(device if device != 'cuda' else 'cuda:0')
    Lt = _host_max(in_lens) if n_tokens is None else int(n_tokens)
    T = _host_max(mel_lens) if n_frames is None else int(n_frames)
    in_lens = torch.as_tensor(in_lens).to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
    B = in_lens.numel()
    mel_lens = _dev_lens(torch.as_tensor(mel_lens).reshape(-1), B, T, dev)
    out = torch.empty(B, T, Lt, dtype=dtype, device=dev)
    if B:
        with torch.cuda.device(dev):
            L.check(lib.ttsamd_attn_prior(_ptr(in_lens), _ptr(mel_lens), B, Lt, T, PRIOR_MODES[mode] | (_PRIOR_F64 if dtype == torch.float64 else 0),
                                          float(scaling), _ptr(out), _stream()), 'attn_prior')
    return out


def _attn_map(t, what):
    """[B, T, L] or [B, 1, T, L] on the device -> contiguous fp32 [B, T, L]"""
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise L.TtsAmdError(f'{what}: expected a tensor on the ROCm device (there is no CPU fallback)')
    if t.requires_grad:
        raise L.TtsAmdError(f'{what}: the input requires grad, and the backward of this loss is not built (forward only: detach it)')
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    elif t.dim() != 3:
        raise L.TtsAmdError(f'{what}: expected [B, T, L] or [B, 1, T, L], got shape {tuple(t.shape)}')
    return t.to(torch.float32).contiguous()


def forward_sum_loss(attn_logprob, in_lens, out_lens, blank_logprob=-1):
    """The forward-sum (CTC) negative log-likelihood of every row's text given its frames, as the reference's AttentionCTCLoss takes it
    (ttsamd_attn_ctc_loss, two launches): attn_logprob [B, T, L] or [B, 1, T, L] fp32 on the device, in_lens / out_lens [B] -> nll [B]
    float64; +inf where out_lens[b] < in_lens[b] (no path), 0 where in_lens[b] == 0.  Forward only: no grad history."""
    lib = _require_gpu()
    a = _attn_map(attn_logprob, 'forward_sum_loss')
    B, T, Lt = a.shape
    if Lt > MAS_MAX_TOKENS:
        raise L.TtsAmdError(f'forward_sum_loss: {Lt} tokens, at most {MAS_MAX_TOKENS} are built (TTSAMD_MAS_MAX_TOKENS)')
    in_lens, out_lens = _dev_lens(in_lens, B, Lt, a.device), _dev_lens(out_lens, B, T, a.device)
    nll = torch.empty(B, dtype=torch.float64, device=a.device)
    if B:
        nb = int(lib.ttsamd_attn_ctc_loss_workspace_bytes(B, T, Lt))
        ws = _ctc_ws.get(max(nb, 8), a.device)
        with torch.cuda.device(a.device):
            L.check(lib.ttsamd_attn_ctc_loss(_ptr(a), _ptr(in_lens), _ptr(out_lens), B, T, Lt, float(blank_logprob), _ptr(nll), _ptr(ws), nb,
                                             _stream()), 'attn_ctc_loss')
    return nll


def binarization_loss(hard, soft, eps=1e-12):
    """Per row the sum of log(max(soft, eps)) over the cells where hard == 1, and their count (ttsamd_attn_bin_loss, one launch): hard, soft
    [B, T, L] or [B, 1, T, L] on the device -> (sum_log [B], count [B]) float64, summed in a fixed order (the same bits run to run).  The
    reference's AttentionBinarizationLoss is -sum_log.sum() / count.sum().  Forward only: no grad history."""
    lib = _require_gpu()
    h, s = _attn_map(hard, 'binarization_loss: hard'), _attn_map(soft, 'binarization_loss: soft')
    if h.shape != s.shape:
        raise L.TtsAmdError(f'binarization_loss: hard {tuple(h.shape)} and soft {tuple(s.shape)} differ')
    B, T, Lt = h.shape
    sum_log = torch.empty(B, dtype=torch.float64, device=h.device)
    count = torch.empty(B, dtype=torch.float64, device=h.device)
    if B:
        with torch.cuda.device(h.device):
            L.check(lib.ttsamd_attn_bin_loss(_ptr(h), _ptr(s), B, T, Lt, float(eps), _ptr(sum_log), _ptr(count), _stream()), 'attn_bin_loss')
    return sum_log, count


# ---- pYIN pitch tracking (csrc/pyin.hip) ------------------------------------------------------------------------------------------------
PYIN_MAX_FRAMES = 8192                                          # TTSAMD_PYIN_MAX_FRAMES of include/ttsamd.h


def _pyin_cfg(fmin, fmax, sr=22050, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100, beta_parameters=(2, 18),
              boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01,
              pad_mode='constant'):
    """librosa.pyin's names and defaults -> ttsamd_pyin_cfg.  What the struct cannot hold is refused here, naming what is built."""
    a, b = beta_parameters
    for name, v in (('sr', sr), ('frame_length', frame_length), ('n_thresholds', n_thresholds), ('beta_parameters[0]', a),
                    ('beta_parameters[1]', b)):
        if int(v) != v:
            raise L.TtsAmdError(f'pyin: {name} = {v!r}: integers are built (the Beta CDF in closed form needs integer parameters)')
    if pad_mode not in ('constant', 'reflect'):
        raise L.TtsAmdError(f"pyin: pad_mode {pad_mode!r}: 'constant' and 'reflect' are built")
    frame_length = int(frame_length)
    cfg = L.PyinCfg()
    cfg.sample_rate, cfg.frame_length = int(sr), frame_length
    cfg.win_length = frame_length // 2 if win_length is None else int(win_length)
    cfg.hop_length = frame_length // 4 if hop_length is None else int(hop_length)
    cfg.fmin, cfg.fmax = float(fmin), float(fmax)
    cfg.n_thresholds, cfg.beta_a, cfg.beta_b = int(n_thresholds), int(a), int(b)
    cfg.boltzmann, cfg.resolution = float(boltzmann_parameter), float(resolution)
    cfg.max_transition_rate, cfg.switch_prob, cfg.no_trough_prob = float(max_transition_rate), float(switch_prob), float(no_trough_prob)
    cfg.pad_mode = int(pad_mode == 'reflect')
    return cfg


def pyin_tables(fmin, fmax, **kw):
    """The tables csrc/pyin.hip builds on the host in float64 and uploads at create (ttsamd_pyin_tables; no GPU is needed):
    dict(pmin, pmax, n_bins, bins_per_semitone, width, max_obs, n_kinds, beta [K], expn / norm [max_obs + 1], trans [n_kinds, width, 2]
    float64, logtrans [n_kinds, width, 2] float32, f0 [n_bins] float32)."""
    lib, cfg = L.load(), _pyin_cfg(fmin, fmax, **kw)
    dims = (C.c_int32 * 8)()
    none = C.c_void_p(0)
    L.check(lib.ttsamd_pyin_tables(C.byref(cfg), dims, none, none, none, none, none, none), 'pyin_tables')
    pmin, pmax, P, nb, w, E, kinds = list(dims)[:7]
    beta, expn, norm = np.zeros(cfg.n_thresholds), np.zeros(E + 1), np.zeros(E + 1)
    trans, logtrans, f0 = np.zeros((kinds, w, 2)), np.zeros((kinds, w, 2), dtype=np.float32), np.zeros(P, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(lib.ttsamd_pyin_tables(C.byref(cfg), dims, p(beta), p(expn), p(norm), p(trans), p(logtrans), p(f0)), 'pyin_tables')
    return dict(pmin=pmin, pmax=pmax, n_bins=P, bins_per_semitone=nb, width=w, max_obs=E, n_kinds=kinds, beta=beta, expn=expn, norm=norm,
                trans=trans, logtrans=logtrans, f0=f0)


class PyinEngine:
    """Handle over ttsamd_pyin_* (csrc/pyin.hip): wave -> (f0, voiced_flag, voiced_prob) per frame in two launches.  The keyword
    arguments are librosa.pyin's (the reference's two calls: fmin = C2, fmax = C7, frame_length = 1024, hop_length 256, sr 22050)."""

    def __init__(self, fmin, fmax, device='cuda', **kw):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        cfg = _pyin_cfg(fmin, fmax, **kw)
        dims = (C.c_int32 * 8)()
        none = C.c_void_p(0)
        L.check(self.lib.ttsamd_pyin_tables(C.byref(cfg), dims, none, none, none, none, none, none), 'pyin: configuration')
        self.n_bins, self.max_obs, self.hop, self.fmin = int(dims[2]), int(dims[5]), int(cfg.hop_length), float(fmin)
        self.bins_per_semitone = int(dims[3])
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_pyin_create(C.byref(cfg), C.byref(handle)), 'pyin_create')
        self.handle = handle
        self.ws = _Workspace()

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_pyin_destroy(self.handle)
            self.handle = None

    def frames(self, n):
        return 1 + n // self.hop

    def workspace_bytes(self, batch, n_frames):
        return int(self.lib.ttsamd_pyin_workspace_bytes(self.handle, int(batch), int(n_frames)))

    def forward(self, wave, nsamples=None, return_states=False, return_obs=False):
        """wave [B, n_max] float32, nsamples int64 [B] on the device or None (every row n_max long) ->
        (f0 [B, T] fp32, 0 where unvoiced; voiced_flag [B, T] bool; voiced_prob [B, T] float64; frames int64 [B]), T = frames(n_max),
        all on the device.  Row b is the call on wave[b, :nsamples[b]] alone; frames at or past a row's own count are zero.  Nothing is
        read back to the host.  return_states: + the Viterbi states int32 [B, T] (< n_bins voiced, -1 past the row);
        return_obs: + the sparse observations the Viterbi kernel read, dict(count int32 [B, T], unvoiced fp32 [B, T],
        logprob fp32 [B, T, max_obs], bin int16-as-int32 [B, T, max_obs]) copied out of the workspace."""
        wave = _f32(wave, self.device)
        if wave.dim() != 2:
            raise L.TtsAmdError(f'PyinEngine.forward: wave of shape {tuple(wave.shape)}, expected [B, n]')
        B, n_max = wave.shape
        T = self.frames(n_max)
        if T > PYIN_MAX_FRAMES:
            raise L.TtsAmdError(f'PyinEngine.forward: {T} frames; at most {PYIN_MAX_FRAMES} per row are built')
        if nsamples is None:
            nsamples = torch.full((B,), n_max, dtype=torch.int64, device=self.device)
        nsamples = nsamples.to(device=self.device, dtype=torch.int64).contiguous()
        f0 = torch.empty(B, T, dtype=torch.float32, device=self.device)
        flag = torch.empty(B, T, dtype=torch.uint8, device=self.device)
        prob = torch.empty(B, T, dtype=torch.float64, device=self.device)
        frames = torch.empty(B, dtype=torch.int64, device=self.device)
        states = torch.empty(B, T, dtype=torch.int32, device=self.device) if return_states else None
        out = [f0, flag.view(torch.bool), prob, frames]
        if return_states:
            out.append(states)
        if B == 0:
            return tuple(out) + (({},) if return_obs else ())
        nbytes = self.workspace_bytes(B, T)
        if nbytes < 0:
            raise L.TtsAmdError(f'PyinEngine.forward: batch {B} x {T} frames is refused')
        ws = self.ws.get(nbytes, self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_pyin_forward(self.handle, _ptr(wave), n_max, _ptr(nsamples), B, T, _ptr(f0), _ptr(flag), _ptr(prob),
                                                 _ptr(states), _ptr(frames), _ptr(ws), nbytes, _stream()), 'pyin_forward')
        if return_obs:
            off = (C.c_int64 * 4)()
            L.check(self.lib.ttsamd_pyin_obs_offsets(self.handle, B, T, off), 'pyin_obs_offsets')
            E, n = self.max_obs, B * T
            obs = dict(count=ws[off[0]: off[0] + 4 * n].view(torch.int32).view(B, T).clone(),
                       unvoiced=ws[off[1]: off[1] + 4 * n].view(torch.float32).view(B, T).clone(),
                       logprob=ws[off[2]: off[2] + 4 * n * E].view(torch.float32).view(B, T, E).clone(),
                       bin=ws[off[3]: off[3] + 2 * n * E].view(torch.int16).view(B, T, E).to(torch.int32))
            out.append(obs)
        return tuple(out)


RESAMPLE_ROUTES = {'auto': 0, 'general': 1, 'mfma': 2}


class ResampleEngine:
    """Handle over ttsamd_resample_* (csrc/resample.hip): polyphase sinc resampling orig_freq -> new_freq with the table of
    ttsamd.resample.resample_taps (Hann-windowed sinc: torchaudio's 'sinc_interp_hann').  route 'auto' | 'general' (VALU kernel) |
    'mfma' (fp32 MFMA kernel; raises when the shape is not eligible: `mfma_eligible`)."""

    def __init__(self, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, device='cuda'):
        from . import resample as R
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        try:
            taps, self.width, self.o, self.n = R.resample_taps(orig_freq, new_freq, lowpass_filter_width, rolloff)
        except ValueError as e:
            raise L.TtsAmdError(str(e)) from None
        self.taps_per_phase = taps.shape[1]
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ttsamd_resample_create(taps.ctypes.data_as(C.c_void_p), self.o, self.n, self.width, C.byref(handle)),
                    'resample_create')
        self.handle = handle
        self.mfma_eligible = bool(self.lib.ttsamd_resample_mfma_eligible(handle))

    def __del__(self):
        if getattr(self, 'handle', None):
            self.lib.ttsamd_resample_destroy(self.handle)
            self.handle = None

    def out_len(self, n):
        return int(self.lib.ttsamd_resample_out_len(self.handle, int(n)))

    def forward(self, wave, nsamples=None, route='auto', out_width=None):
        """wave [B, n_max] float32, nsamples int64 [B] on the device or None (every row n_max long) ->
        (out [B, out_len(n_max)] (or out_width columns, if wider), nout int64 [B] on the device).  Row b is the call on
        wave[b, :nsamples[b]] alone, bit for bit; samples at or past a row's own count are zero.  Nothing is read back to the host."""
        wave = _f32(wave, self.device)
        if wave.dim() != 2:
            raise L.TtsAmdError(f'ResampleEngine.forward: wave of shape {tuple(wave.shape)}, expected [B, n]')
        B, n_max = wave.shape
        if nsamples is None:
            nsamples = torch.full((B,), n_max, dtype=torch.int64, device=self.device)
        nsamples = nsamples.to(device=self.device, dtype=torch.int64).contiguous()
        W = max(self.out_len(n_max), int(out_width or 0))
        out = torch.empty(B, W, dtype=torch.float32, device=self.device)
        nout = torch.empty(B, dtype=torch.int64, device=self.device)
        if B:
            with torch.cuda.device(self.device):
                L.check(self.lib.ttsamd_resample_forward(self.handle, _ptr(wave), n_max, _ptr(nsamples), B, _ptr(out), W, _ptr(nout),
                                                         RESAMPLE_ROUTES[route], _stream()), 'resample_forward')
        return out, nout


class TrimEngine:
    """ttsamd_trim_bounds / ttsamd_trim_apply / ttsamd_frames_compact (csrc/trim.hip) with their workspace: librosa.effects.trim's
    bounds with ref = max, the peak normalisation x / max|x| * gain over the kept span, and the removal of silent mel frames."""

    def __init__(self, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        self.ws = _Workspace()

    def _wave(self, wave, nsamples):
        wave = _f32(wave, self.device)
        if wave.dim() != 2:
            raise L.TtsAmdError(f'TrimEngine: wave of shape {tuple(wave.shape)}, expected [B, n]')
        return wave, _dev_lens(nsamples, wave.shape[0], wave.shape[1], self.device)

    def bounds(self, wave, nsamples=None, top_db=60.0, frame_length=2048, hop_length=512, gain=0.0):
        """wave [B, n_max], nsamples int64 [B] or None -> (bounds int64 [B, 2] = (start, end), peak fp32 [B] = max |x| per row), on the
        device.  gain > 0: the bounds of the row scaled to that peak (what `apply` writes)."""
        wave, nsamples = self._wave(wave, nsamples)
        B, n_max = wave.shape
        frame_length, hop_length = int(frame_length), int(hop_length)
        if not 1 <= frame_length <= 8192 or not 1 <= hop_length <= frame_length:
            raise L.TtsAmdError(f'trim: frame_length {frame_length} / hop_length {hop_length}: frame_length <= 8192 and '
                                '1 <= hop_length <= frame_length are built')
        bounds = torch.zeros(B, 2, dtype=torch.int64, device=self.device)
        peak = torch.zeros(B, dtype=torch.float32, device=self.device)
        if B:
            nbytes = int(self.lib.ttsamd_trim_workspace_bytes(B, n_max, hop_length))
            ws = self.ws.get(nbytes, self.device)
            with torch.cuda.device(self.device):
                L.check(self.lib.ttsamd_trim_bounds(_ptr(wave), n_max, _ptr(nsamples), B, float(top_db), frame_length, hop_length,
                                                    float(gain), _ptr(bounds), _ptr(peak), _ptr(ws), nbytes, _stream()), 'trim_bounds')
        return bounds, peak

    def apply(self, wave, bounds, peak=None, gain=1.0, tail=0, out_width=None):
        """-> (out [B, out_width or n_max + tail]: fl32(fl32(x / peak) * gain) over [start, end), zeros behind; lens int64 [B] =
        end - start + tail)."""
        wave = _f32(wave, self.device)
        B, n_max = wave.shape
        W = int(out_width) if out_width is not None else n_max + int(tail)
        out = torch.empty(B, W, dtype=torch.float32, device=self.device)
        lens = torch.empty(B, dtype=torch.int64, device=self.device)
        bounds = bounds.to(device=self.device, dtype=torch.int64).contiguous()
        if peak is not None:
            peak = _f32(peak, self.device)
        if B:
            with torch.cuda.device(self.device):
                L.check(self.lib.ttsamd_trim_apply(_ptr(wave), n_max, _ptr(bounds), _ptr(peak), float(gain), int(tail), B, _ptr(out), W,
                                                   _ptr(lens), _stream()), 'trim_apply')
        return out, lens

    def compact(self, mel, lens=None, thresh=-10.0, extra=None):
        """mel [B, C, T] (+ extra [B, C2, T]) on the device -> (mel', extra' or None, lens'): the columns whose channel mean is above
        `thresh`, plus everything behind the last such column (the reference's remove_silence), moved to the front; zeros behind."""
        mel = _dev_f32(mel, 3, 'drop_silent_frames: mel')
        B, Cn, T = mel.shape
        lens = _dev_lens(lens, B, T, mel.device)
        C2 = 0
        if extra is not None:
            extra = _dev_f32(extra, 3, 'drop_silent_frames: extra')
            if extra.shape[0] != B or extra.shape[2] != T:
                raise L.TtsAmdError(f'drop_silent_frames: extra of shape {tuple(extra.shape)} next to mel {tuple(mel.shape)}')
            C2 = extra.shape[1]
        mel_out = torch.empty_like(mel)
        extra_out = torch.empty_like(extra) if extra is not None else None
        lens_out = torch.empty(B, dtype=torch.int64, device=mel.device)
        if B and Cn:
            with torch.cuda.device(mel.device):
                L.check(self.lib.ttsamd_frames_compact(_ptr(mel), _ptr(extra), _ptr(lens), B, Cn, C2, T, float(thresh), _ptr(mel_out),
                                                       _ptr(extra_out), _ptr(lens_out), _stream()), 'frames_compact')
        return mel_out, extra_out, lens_out


LEVEL_MODES = {'off': 0, 'peak': 1, 'lufs': 2}


class LoudnessEngine:
    """ttsamd_loudness_measure / ttsamd_wave_level (csrc/loudness.hip) with their workspace: ITU-R BS.1770-4 integrated loudness and the
    peak per row of a ragged mono batch at `sample_rate`, and one gain per row towards a target.  Nothing is read back to the host."""

    def __init__(self, sample_rate=22050, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        self.sample_rate = int(sample_rate)
        coef = (C.c_double * 10)()
        L.check(self.lib.ttsamd_loudness_coefficients(self.sample_rate, coef), 'loudness_coefficients')
        self.coefficients = np.array(coef)      # b1[0..2], a1[1..2], b2[0..2], a2[1..2]
        self.ws = _Workspace()
        self.limit_ws = _Workspace()

    def _wave(self, wave, lens):
        wave = _dev_f32(wave, 2, 'LoudnessEngine: wave')
        return wave, _dev_lens(lens, wave.shape[0], wave.shape[1], wave.device)

    def measure(self, wave, lens=None):
        """wave [B, n_max], lens int64 [B] or None -> (loudness float64 [B] in LUFS, -inf for a silent or empty row; peak fp32 [B] =
        max |x| per row), on the device."""
        wave, lens = self._wave(wave, lens)
        B, n_max = wave.shape
        loud = torch.full((B,), float('-inf'), dtype=torch.float64, device=wave.device)
        peak = torch.zeros(B, dtype=torch.float32, device=wave.device)
        if B:
            nbytes = int(self.lib.ttsamd_loudness_workspace_bytes(B, n_max, self.sample_rate))
            if nbytes < 0:
                raise L.TtsAmdError(f'loudness: a batch of {B} rows of {n_max} samples at {self.sample_rate} Hz is refused')
            ws = self.ws.get(max(nbytes, 1), wave.device)
            with torch.cuda.device(wave.device):
                L.check(self.lib.ttsamd_loudness_measure(_ptr(wave), n_max, _ptr(lens), B, self.sample_rate, _ptr(loud), _ptr(peak),
                                                         _ptr(ws), nbytes, _stream()), 'loudness_measure')
        return loud, peak

    def meter(self, wave, lens=None, series=False):
        """The whole-wave loudness meter (ttsamd_loudness_meter; include/ttsamd.h states the arithmetic): wave [B, n_max], lens int64
        [B] or None -> dict of device tensors [B]: integrated (float64 LUFS; the bits of `measure`), peak (fp32), loudness_range
        (float64 LU), max_momentary, max_short_term (float64, -inf when there is no value), counts (int64 [B, 2]: momentary and
        short-term values).  series: also momentary [B, J] and short_term [B, JS] (float64), NaN at and past a row's own count."""
        wave, lens = self._wave(wave, lens)
        B, n_max = wave.shape
        dev = wave.device
        step = (self.sample_rate + 5) // 10
        J = (n_max - 4 * step) // step + 1 if n_max >= 4 * step else 1
        JS = max(n_max // step - 29, 0)
        out = dict(integrated=torch.full((B,), float('-inf'), dtype=torch.float64, device=dev),
                   peak=torch.zeros(B, dtype=torch.float32, device=dev), loudness_range=torch.zeros(B, dtype=torch.float64, device=dev),
                   max_momentary=torch.full((B,), float('-inf'), dtype=torch.float64, device=dev),
                   max_short_term=torch.full((B,), float('-inf'), dtype=torch.float64, device=dev),
                   counts=torch.zeros(B, 2, dtype=torch.int64, device=dev))
        if series:
            out['momentary'] = torch.full((B, J), float('nan'), dtype=torch.float64, device=dev)
            out['short_term'] = torch.full((B, JS), float('nan'), dtype=torch.float64, device=dev)
        if B:
            nbytes = int(self.lib.ttsamd_loudness_meter_workspace_bytes(B, n_max, self.sample_rate))
            if nbytes < 0:
                raise L.TtsAmdError(f'loudness meter: a batch of {B} rows of {n_max} samples at {self.sample_rate} Hz is refused')
            ws = self.ws.get(max(nbytes, 1), dev)
            with torch.cuda.device(dev):
                L.check(self.lib.ttsamd_loudness_meter(_ptr(wave), n_max, _ptr(lens), B, self.sample_rate, _ptr(out['integrated']),
                                                       _ptr(out['peak']), _ptr(out['loudness_range']), _ptr(out['max_momentary']),
                                                       _ptr(out['max_short_term']), _ptr(out['counts']), _ptr(out.get('momentary')), J,
                                                       _ptr(out.get('short_term')), JS, _ptr(ws), nbytes, _stream()), 'loudness_meter')
        return out

    def true_peak(self, wave, lens=None):
        """wave [B, n_max], lens int64 [B] or None -> fp32 [B] on the device: the peak of the 4x oversampled row (ttsamd_true_peak;
        include/ttsamd.h states the interpolator), rounded upward to fp32; 0 for an empty row.  Two launches, no workspace."""
        wave, lens = self._wave(wave, lens)
        B, n_max = wave.shape
        tp = torch.zeros(B, dtype=torch.float32, device=wave.device)
        if B:
            with torch.cuda.device(wave.device):
                L.check(self.lib.ttsamd_true_peak(_ptr(wave), n_max, _ptr(lens), B, _ptr(tp), _stream()), 'true_peak')
        return tp

    def level(self, wave, lens, mode, target, ceiling=0.99, true_peak=False):
        """wave [B, n_max] fp32 contiguous on the device, scaled IN PLACE up to lens[b] and returned with the gains fp32 [B].
        mode: 0 / 'off', 1 / 'peak' (x / max|x| * target), 2 / 'lufs' (towards `target` LUFS, the gain capped so that the peak stays
        <= ceiling); mode and target are scalars or one value per row, checked here on the host before they go to the device.
        true_peak: the peak of both modes is the row's true peak (`true_peak`) instead of max |x|."""
        if not isinstance(wave, torch.Tensor) or wave.device.type != 'cuda' or wave.dtype != torch.float32 or not wave.is_contiguous() \
                or wave.dim() != 2:
            raise L.TtsAmdError('LoudnessEngine.level: expected a contiguous float32 tensor [B, n] on the ROCm device (it is scaled in place)')
        B, n_max = wave.shape
        lens = _dev_lens(lens, B, n_max, wave.device)
        modes = row_values(mode, B, 'level mode') if per_row(mode) else [mode] * B
        modes = [LEVEL_MODES.get(m, m) if isinstance(m, str) else m for m in modes]
        for m in modes:
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= int(m) <= 2:
                raise L.TtsAmdError(f"level: mode {m!r}: one of 0 / 'off', 1 / 'peak', 2 / 'lufs'")
        targets = row_values(target, B, 'level target') if per_row(target) else [target] * B
        check_finite(targets, 'level target')
        if not 0.0 < float(ceiling) <= 1.0:
            raise L.TtsAmdError(f'level: ceiling {ceiling!r} is not in (0, 1]')
        gain = torch.ones(B, dtype=torch.float32, device=wave.device)
        if B:
            loud, peak = self.measure(wave, lens)
            if true_peak:
                peak = self.true_peak(wave, lens)
            mode_d = torch.tensor([int(m) for m in modes], dtype=torch.int32).to(wave.device)
            with torch.cuda.device(wave.device):
                L.check(self.lib.ttsamd_wave_level(_ptr(wave), n_max, _ptr(lens), B, _ptr(mode_d), _ptr(_rows_f32(targets, wave.device)),
                                                   float(ceiling), _ptr(loud), _ptr(peak), _ptr(gain), _stream()), 'wave_level')
        return wave, gain

    def limit_samples(self, wave, lens, mode, target, ceiling, max_gain, attack, hold, loudness=None, true_peak=False):
        """ttsamd_wave_limit as it is: attack and hold in samples, max_gain linear, mode int32 [B] and target fp32 [B] ON THE DEVICE
        (already checked), loudness float64 [B] on the device or None (no mode 2 row) -> (wave, gain fp32 [B], reduction int32 [B]).
        true_peak: ttsamd_wave_limit_true_peak, the same call with the true-peak detector."""
        call, what = (self.lib.ttsamd_wave_limit_true_peak, 'wave_limit_true_peak') if true_peak else (self.lib.ttsamd_wave_limit, 'wave_limit')
        B, n_max = wave.shape
        gain = torch.ones(B, dtype=torch.float32, device=wave.device)
        red = torch.full((B,), LIMITER_Q, dtype=torch.int32, device=wave.device)
        if B:
            nbytes = int(self.lib.ttsamd_wave_limit_workspace_bytes(B, n_max))
            if nbytes < 0:
                raise L.TtsAmdError(f'limit: a batch of {B} rows of {n_max} samples is refused')
            ws = self.limit_ws.get(max(nbytes, 1), wave.device)
            with torch.cuda.device(wave.device):
                L.check(call(_ptr(wave), n_max, _ptr(lens), B, _ptr(mode), _ptr(target), float(ceiling), float(max_gain), int(attack), int(hold),
                             _ptr(loudness), _ptr(gain), _ptr(red), _ptr(ws), nbytes, _stream()), what)
        return wave, gain, red

    def limit(self, wave, lens, mode, target, ceiling=0.99, max_gain_db=30.0, attack_ms=1.5, hold_ms=15.0, true_peak=False):
        """The look-ahead limiter (csrc/limiter.hip; include/ttsamd.h states its arithmetic): wave [B, n_max] fp32 contiguous on the
        device, IN PLACE up to lens[b]: row b times its gain, then a gain-reduction curve that keeps |y| <= ceiling exactly and leaves a
        row that stays under the ceiling as fl32(x g).  mode: 0 / 'off', 2 / 'lufs' (towards `target` LUFS, measured here, with no cap
        from the peak), 3 / 'gain' (`target` is a gain in dB); mode and target are scalars or one value per row, checked here on the host.
        The gain is at most max_gain_db.  attack_ms: the look-ahead and the length of both ramps, hold_ms: how long the reduction stays
        after a peak; A = round(attack_ms fs / 1000) <= 1024 samples, R = max(round(hold_ms fs / 1000), A) <= 4096.
        true_peak: the detector also sees the 4x interpolator's values to either side of a sample (ttsamd_wave_limit_true_peak): the
        sample peak still stays <= ceiling exactly, the true peak close to it (no exact bound: include/ttsamd.h).
        -> (wave, gain fp32 [B], reduction int32 [B] = the smallest curve value in Q30, LIMITER_Q where nothing was limited)."""
        if not isinstance(wave, torch.Tensor) or wave.device.type != 'cuda' or wave.dtype != torch.float32 or not wave.is_contiguous() \
                or wave.dim() != 2:
            raise L.TtsAmdError('LoudnessEngine.limit: expected a contiguous float32 tensor [B, n] on the ROCm device (it is limited in place)')
        B, n_max = wave.shape
        lens = _dev_lens(lens, B, n_max, wave.device)
        modes = row_values(mode, B, 'limit mode') if per_row(mode) else [mode] * B
        modes = [LIMIT_MODES.get(m, m) if isinstance(m, str) else m for m in modes]
        for m in modes:
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in (0, 2, 3):
                raise L.TtsAmdError(f"limit: mode {m!r}: one of 0 / 'off', 2 / 'lufs', 3 / 'gain'")
        targets = row_values(target, B, 'limit target') if per_row(target) else [target] * B
        check_finite(targets, 'limit target')
        if not 0.0 < float(ceiling) <= 1.0:
            raise L.TtsAmdError(f'limit: ceiling {ceiling!r} is not in (0, 1]')
        check_finite([max_gain_db], 'limit max_gain_db')
        attack, hold = limiter_samples(attack_ms, hold_ms, self.sample_rate)
        if not B:
            return wave, torch.ones(0, dtype=torch.float32, device=wave.device), torch.zeros(0, dtype=torch.int32, device=wave.device)
        loud = self.measure(wave, lens)[0] if any(int(m) == 2 for m in modes) else None
        mode_d = torch.tensor([int(m) for m in modes], dtype=torch.int32).to(wave.device)
        return self.limit_samples(wave, lens, mode_d, _rows_f32(targets, wave.device), ceiling, 10.0 ** (float(max_gain_db) / 20.0), attack,
                                  hold, loud, true_peak=bool(true_peak))


class LoudnessMeter:
    """The stream meter (ttsamd_meter_*; include/ttsamd.h states the arithmetic): `max_streams` slots on the device, each a stream of at
    most `max_seconds` at `sample_rate` that is measured while it arrives, in chunks of any length.  Nothing is read back to the host.
    METER_DROPPED in a result's status: a push went beyond max_seconds and was left out."""
    METER_DROPPED = 1

    def __init__(self, sample_rate=22050, max_streams=32, max_seconds=600.0, device='cuda'):
        self.lib = _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        self.sample_rate, self.max_streams = int(sample_rate), int(max_streams)
        self.max_samples = int(float(max_seconds) * self.sample_rate)
        nbytes = int(self.lib.ttsamd_meter_state_bytes(self.max_streams, self.max_samples, self.sample_rate))
        if nbytes < 0:
            raise L.TtsAmdError(f'LoudnessMeter: {max_streams} streams of {max_seconds} s at {sample_rate} Hz are refused')
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.ws = _Workspace()
        self.reset(range(self.max_streams))

    def _slots(self, slots, rows=None):
        slots = [int(s) for s in slots]
        if len(set(slots)) != len(slots) or any(not 0 <= s < self.max_streams for s in slots) or (rows is not None and len(slots) != rows):
            raise ValueError(f'LoudnessMeter: slots {slots}: one slot of 0 .. {self.max_streams - 1} per row, none twice')
        return torch.tensor(slots, dtype=torch.int32).to(self.device)

    def _call(self, fn, what, *args):
        with torch.cuda.device(self.device):
            L.check(fn(_ptr(self.state), self.state.numel(), self.max_streams, self.max_samples, self.sample_rate, *args, _stream()), what)

    def reset(self, slots):
        """the slots start again at zero samples"""
        slots_d = self._slots(slots)
        if slots_d.numel():
            self._call(self.lib.ttsamd_meter_reset, 'meter_reset', _ptr(slots_d), slots_d.numel())

    def push(self, chunks, lens=None, slots=None):
        """chunks [rows, n_max] fp32 on the device (or one chunk [n]), lens int64 [rows] or None, slots: one slot per row (default
        0 .. rows - 1) -> dict of float64 device tensors [rows]: momentary and short_term (the latest value, -inf before the first)
        and integrated (both gates over the blocks so far)."""
        chunks = _dev_f32(chunks if chunks.dim() != 1 else chunks[None], 2, 'LoudnessMeter.push: chunks')
        rows, n_max = chunks.shape
        lens = _dev_lens(lens, rows, n_max, chunks.device)
        slots_d = self._slots(range(rows) if slots is None else slots, rows)
        out = {k: torch.full((rows,), float('-inf'), dtype=torch.float64, device=self.device) for k in ('momentary', 'short_term', 'integrated')}
        if rows:
            nbytes = int(self.lib.ttsamd_meter_push_workspace_bytes(rows, n_max, self.sample_rate))
            if nbytes < 0:
                raise L.TtsAmdError(f'LoudnessMeter.push: {rows} rows of {n_max} samples are refused')
            ws = self.ws.get(max(nbytes, 1), self.device)
            self._call(self.lib.ttsamd_meter_push, 'meter_push', _ptr(chunks), n_max, _ptr(lens), _ptr(slots_d), rows,
                       _ptr(out['momentary']), _ptr(out['short_term']), _ptr(out['integrated']), _ptr(ws), nbytes)
        return out

    def result(self, slots):
        """-> dict of device tensors [rows] over each slot's samples so far: integrated, loudness_range, max_momentary, max_short_term
        (float64), peak (fp32), counts (int64 [rows, 2]: momentary and short-term values), status (int32; METER_DROPPED)"""
        slots_d = self._slots(slots)
        rows = slots_d.numel()
        f64 = lambda: torch.zeros(rows, dtype=torch.float64, device=self.device)
        out = dict(integrated=f64(), loudness_range=f64(), max_momentary=f64(), max_short_term=f64(),
                   peak=torch.zeros(rows, dtype=torch.float32, device=self.device),
                   counts=torch.zeros(rows, 2, dtype=torch.int64, device=self.device),
                   status=torch.zeros(rows, dtype=torch.int32, device=self.device))
        if rows:
            self._call(self.lib.ttsamd_meter_result, 'meter_result', _ptr(slots_d), rows, *(_ptr(out[k]) for k in (
                'integrated', 'loudness_range', 'max_momentary', 'max_short_term', 'peak', 'counts', 'status')))
        return out


LIMIT_MODES = {'off': 0, 'lufs': 2, 'gain': 3}
LIMITER_TILE = 2048                     # samples per block of the limiter's second launch (csrc/limiter.hip: LM_T)
LIMITER_Q = 1 << 30                     # the gain-reduction curve's one: reduction == LIMITER_Q means nothing was limited
LIMITER_MAX_ATTACK, LIMITER_MAX_HOLD = 1024, 4096
LIMITER_NO_MAX_GAIN = 3.0e38            # a max_gain that clamps no fp32 gain (utils.audio.limit: the gain is the caller's own)
LIMITER_DEFAULTS = dict(ceiling=0.99, attack_ms=1.5, hold_ms=15.0, max_gain_db=30.0)


def limiter_samples(attack_ms, hold_ms, sample_rate):
    """(attack, hold) in samples: A = round(attack_ms fs / 1000), R = max(round(hold_ms fs / 1000), A); ValueError outside the kernel's
    limits (A <= 1024, R <= 4096) or for a negative or non-finite time"""
    for name, v in (('attack_ms', attack_ms), ('hold_ms', hold_ms)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)) or float(v) < 0:
            raise ValueError(f'limiter: {name} {v!r}: a finite time in milliseconds, 0 or more')
    A = int(round(float(attack_ms) * sample_rate / 1000.0))
    R = max(int(round(float(hold_ms) * sample_rate / 1000.0)), A)
    if A > LIMITER_MAX_ATTACK or R > LIMITER_MAX_HOLD:
        raise ValueError(f'limiter: attack of {A} and hold of {R} samples at {sample_rate} Hz: at most {LIMITER_MAX_ATTACK} and {LIMITER_MAX_HOLD}')
    return A, R


TRUE_PEAK_REACH = 13                    # the true-peak detector widens the limiter's reach by W + 1 samples on each side (include/ttsamd.h)


def limiter_reach(attack, hold, true_peak=False):
    """samples of input before and after a sample that its limited value depends on: (A + R, 2A), each 13 more with the true-peak
    detector"""
    extra = TRUE_PEAK_REACH if true_peak else 0
    return attack + hold + extra, 2 * attack + extra


def true_peak_taps():
    """-> float64 [3, 25]: the interpolator's phases 1 .. 3 as the kernels take them (ttsamd_true_peak_taps; needs no GPU)"""
    out = (C.c_double * 75)()
    L.check(L.load().ttsamd_true_peak_taps(out), 'true_peak_taps')
    return np.array(out).reshape(3, 25)


def check_true_peak(true_peak, normalize, limiter):
    """Host-side validation of `true_peak` next to `normalize` and `limiter` (both already checked): it has effect only where one of
    them is set, so True with neither is a ValueError."""
    if not isinstance(true_peak, (bool, np.bool_)):
        raise ValueError(f'true_peak: {true_peak!r}: False or True')
    if true_peak and limiter_spec(limiter) is None and not any(v is not None for v in (normalize if per_row(normalize) else [normalize])):
        raise ValueError('true_peak: needs normalize or a limiter to work in')
    return bool(true_peak)


def limiter_spec(limiter):
    """The `limiter` option of the tts wrappers and the streams -> None (off: None or False) or a dict(ceiling, attack_ms, hold_ms,
    max_gain_db) with the defaults filled in (True: all defaults).  ValueError for anything else, an unknown key or a bad value."""
    if limiter is None or limiter is False:
        return None
    if limiter is True:
        return dict(LIMITER_DEFAULTS)
    if not isinstance(limiter, dict):
        raise ValueError(f'limiter: {limiter!r}: False, True or a dict with {sorted(LIMITER_DEFAULTS)}')
    unknown = sorted(set(limiter) - set(LIMITER_DEFAULTS))
    if unknown:
        raise ValueError(f'limiter: unknown keys {unknown}: {sorted(LIMITER_DEFAULTS)}')
    spec = dict(LIMITER_DEFAULTS, **limiter)
    for name, v in spec.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)):
            raise ValueError(f'limiter: {name} {v!r} is not a finite number')
        spec[name] = float(v)
    if not 0.0 < spec['ceiling'] <= 1.0:
        raise ValueError(f"limiter: ceiling {spec['ceiling']!r} is not in (0, 1]")
    if spec['attack_ms'] < 0 or spec['hold_ms'] < 0:
        raise ValueError('limiter: attack_ms and hold_ms are 0 or more')
    return spec


def check_limiter(limiter, normalize):
    """Host-side validation of `limiter` next to `normalize` (already checked): the spec of limiter_spec, or None.  A limiter with no
    line that asks for a level is a ValueError: it has nothing to work on."""
    spec = limiter_spec(limiter)
    if spec is not None and not any(v is not None for v in (normalize if per_row(normalize) else [normalize])):
        raise ValueError("limiter: needs normalize ('lufs' or a target in LUFS on the lines it is to work on)")
    return spec


STOI_BANDS, STOI_SEGMENT = 15, 30                              # third-octave bands, frames per segment (include/ttsamd.h)
_wavescore_ws = _Workspace()


def _wave_pair(ref, other, lens, what):
    """two sample-aligned batches [B, n], [B, n'] on the device -> (ref, other, lens int64 [B], B, width): rows of different padded width
    are compared over the narrower one, so the lengths are clamped to it (on the device)."""
    ref, other = _dev_f32(ref, 2, f'{what}: reference wave'), _dev_f32(other, 2, f'{what}: second wave')
    if ref.shape[0] != other.shape[0]:
        raise L.TtsAmdError(f'{what}: waves of shape {tuple(ref.shape)} and {tuple(other.shape)} differ in batch')
    other = other.to(ref.device)
    W = min(ref.shape[1], other.shape[1])
    if ref.shape[1] != W:
        ref = ref[:, :W].contiguous()
    if other.shape[1] != W:
        other = other[:, :W].contiguous()
    lens = _dev_lens(lens, ref.shape[0], W, ref.device).clamp(max=W)
    return ref, other, lens, ref.shape[0], W


def stoi_10k(wave_ref, wave_deg, lens=None, extended=False, return_bands=False):
    """STOI (extended: ESTOI) of wave_deg against the clean wave_ref, both [B, n] fp32 on the device and ALREADY at 10 000 Hz, lens int64
    [B] or None -> (score float64 [B], frames int32 [B, 2] = (all, kept after the silent-frame removal)); return_bands: + the third-octave
    magnitudes of both, float64 [B, 15, F], zero from a row's kept count on.  Three launches (ttsamd_stoi), float64 throughout; a row
    with fewer than 30 kept frames scores 1e-5.  Specified by the arithmetic in include/ttsamd.h; parity with pystoi is not pinned."""
    lib = _require_gpu()
    ref, deg, lens, B, W = _wave_pair(wave_ref, wave_deg, lens, 'stoi_10k')
    score = torch.empty(B, dtype=torch.float64, device=ref.device)
    frames = torch.zeros(B, 2, dtype=torch.int32, device=ref.device)
    f_max = max((W - 256) // 128 + 1, 0) if W >= 256 else 0
    tob_r = torch.zeros(B, STOI_BANDS, f_max, dtype=torch.float64, device=ref.device) if return_bands else None
    tob_d = torch.zeros_like(tob_r) if return_bands else None
    if B:
        nbytes = int(lib.ttsamd_stoi_workspace_bytes(B, W))
        if nbytes < 0:
            raise L.TtsAmdError(f'stoi_10k: a batch of {B} rows of {W} samples is refused')
        ws = _wavescore_ws.get(max(nbytes, 1), ref.device)
        with torch.cuda.device(ref.device):
            L.check(lib.ttsamd_stoi(_ptr(ref), _ptr(deg), W, _ptr(lens), B, int(bool(extended)), _ptr(score), _ptr(frames),
                                    _ptr(tob_r) if f_max else None, _ptr(tob_d) if f_max else None, f_max, _ptr(ws), nbytes, _stream()), 'stoi')
    return (score, frames, tob_r, tob_d) if return_bands else (score, frames)


def wave_sdr(wave_ref, wave_est, lens=None, zero_mean=True):
    """wave_ref, wave_est [B, n] on the device, lens int64 [B] or None -> float64 [B, 2] = (SI-SDR, SNR) in dB of wave_est against
    wave_ref, one launch (ttsamd_wave_sdr).  zero_mean: both rows are centred first.  +inf for identical rows, NaN for an empty row."""
    lib = _require_gpu()
    ref, est, lens, B, W = _wave_pair(wave_ref, wave_est, lens, 'wave_sdr')
    out = torch.empty(B, 2, dtype=torch.float64, device=ref.device)
    if B:
        with torch.cuda.device(ref.device):
            L.check(lib.ttsamd_wave_sdr(_ptr(ref), _ptr(est), W, _ptr(lens), B, int(bool(zero_mean)), _ptr(out), _stream()), 'wave_sdr')
    return out


def log_spectral_distance(wave_ref, wave_est, lens=None):
    """wave_ref, wave_est [B, n] on the device, lens int64 [B] or None -> float64 [B, 2] = (log-spectral distance in dB, frames): frames
    of 1024 samples every 256 without padding, periodic Hann, 10 log10 max(|X|^2, 1e-10) over bins 0 .. 512, the mean over the frames of
    the rms difference over the bins; NaN for a row under 1024 samples.  One launch (ttsamd_log_spectral_distance)."""
    lib = _require_gpu()
    ref, est, lens, B, W = _wave_pair(wave_ref, wave_est, lens, 'log_spectral_distance')
    out = torch.empty(B, 2, dtype=torch.float64, device=ref.device)
    if B:
        with torch.cuda.device(ref.device):
            L.check(lib.ttsamd_log_spectral_distance(_ptr(ref), _ptr(est), W, _ptr(lens), B, _ptr(out), _stream()), 'log_spectral_distance')
    return out


MR_STFT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))   # (n_fft, hop, win_length): Parallel WaveGAN's three


def mr_stft(wave_ref, wave_est, lens=None, resolutions=MR_STFT_RESOLUTIONS):
    """wave_ref, wave_est [B, n] on the device, lens int64 [B] or None, resolutions: 1 .. 8 triples (n_fft in 512 / 1024 / 2048, hop,
    win_length <= n_fft) -> (float64 [B, R, 2] = (spectral convergence, log-magnitude distance) per resolution, frames int32 [B, R]):
    torch.stft's framing (periodic Hann centred in the frame, reflect padding by n_fft / 2, 1 + n // hop frames), S = sqrt(max(|X|^2,
    1e-7)), sc = ||S_ref - S_est|| / ||S_ref||, mag = mean |ln S_ref - ln S_est| over the row's own frames.  NaN and 0 frames for a row
    of n_fft / 2 samples or fewer.  R + 1 launches (ttsamd_mr_stft), float64 throughout; specified by the arithmetic in include/ttsamd.h."""
    lib = _require_gpu()
    ref, est, lens, B, W = _wave_pair(wave_ref, wave_est, lens, 'mr_stft')
    try:
        res = [tuple(int(v) for v in r) for r in resolutions]
    except (TypeError, ValueError):
        raise L.TtsAmdError(f'mr_stft: resolutions {resolutions!r} are not (n_fft, hop, win_length) triples') from None
    if any(len(r) != 3 for r in res):
        raise L.TtsAmdError(f'mr_stft: resolutions {resolutions!r} are not (n_fft, hop, win_length) triples')
    R = len(res)
    arr = [(C.c_int32 * max(R, 1))(*(r[q] for r in res)) for q in range(3)]
    out = torch.empty(B, R, 2, dtype=torch.float64, device=ref.device)
    frames = torch.zeros(B, R, dtype=torch.int32, device=ref.device)
    if B:
        nbytes = int(lib.ttsamd_mr_stft_workspace_bytes(B, W, arr[0], arr[1], arr[2], R))
        if nbytes < 0:
            raise L.TtsAmdError(f'mr_stft: a batch of {B} rows of {W} samples at the resolutions {res} is refused (1 .. 8 of n_fft 512 / '
                                f'1024 / 2048, 1 <= win_length <= n_fft, hop >= 1)')
        ws = _wavescore_ws.get(max(nbytes, 1), ref.device)
        with torch.cuda.device(ref.device):
            L.check(lib.ttsamd_mr_stft(_ptr(ref), _ptr(est), W, _ptr(lens), B, arr[0], arr[1], arr[2], R, _ptr(out), _ptr(frames), _ptr(ws),
                                       nbytes, _stream()), 'mr_stft')
    return out, frames


class WaveScoreEngine:
    """Wave against wave at `sample_rate`, sample for sample (csrc/wavescore.hip): STOI / ESTOI (after the engine's own
    ResampleEngine(sample_rate, 10000, lowpass_filter_width=64, rolloff=0.99): the project's resampler, not pystoi's), SI-SDR / SNR and
    the log-spectral distance at the waves' own rate.  float64 throughout; nothing is read back to the host.  The two waves must be
    sample-aligned (copy synthesis, one precision mode against another, a delivery format against the float wave): free-running
    synthesis is not aligned with a recording, and a wave-level score of it means nothing."""

    def __init__(self, sample_rate=22050, device='cuda'):
        _require_gpu()
        self.device = torch.device(device if device != 'cuda' else 'cuda:0')
        self.sample_rate = int(sample_rate)
        self.resampler = ResampleEngine(self.sample_rate, 10000, lowpass_filter_width=64, rolloff=0.99, device=self.device) \
            if self.sample_rate != 10000 else None

    def to_10k(self, wave, lens=None):
        """wave [B, n] (+ lens) -> (wave at 10 kHz, its lengths int64 [B] on the device)"""
        wave = _dev_f32(wave, 2, 'WaveScoreEngine: wave')
        lens = _dev_lens(lens, wave.shape[0], wave.shape[1], wave.device)
        if self.resampler is None:
            return wave, lens
        return self.resampler.forward(wave, lens)

    def stoi(self, wave_ref, wave_deg, lens=None, extended=False):
        """-> (score float64 [B], frames int32 [B, 2]) of stoi_10k on both waves resampled to 10 kHz with the shared lengths"""
        ref, deg, lens, _, _ = _wave_pair(wave_ref, wave_deg, lens, 'WaveScoreEngine.stoi')
        r10, n10 = self.to_10k(ref, lens)
        d10, _ = self.to_10k(deg, lens)
        return stoi_10k(r10, d10, n10, extended=extended)

    def metrics(self, wave_ref, wave_est, lens=None):
        """-> dict(stoi, estoi, si_sdr, snr, lsd float64 [B]; frames, frames_kept int32 [B]: the STOI frames at 10 kHz before and
        after the silent-frame removal) of wave_est against wave_ref; the waves are resampled once for both STOI variants."""
        ref, est, lens, _, _ = _wave_pair(wave_ref, wave_est, lens, 'WaveScoreEngine.metrics')
        r10, n10 = self.to_10k(ref, lens)
        e10, _ = self.to_10k(est, lens)
        st, fr = stoi_10k(r10, e10, n10, extended=False)
        es, _ = stoi_10k(r10, e10, n10, extended=True)
        sdr = wave_sdr(ref, est, lens)
        lsd = log_spectral_distance(ref, est, lens)
        return dict(stoi=st, estoi=es, si_sdr=sdr[:, 0], snr=sdr[:, 1], lsd=lsd[:, 0], frames=fr[:, 0], frames_kept=fr[:, 1])

    def mr_stft(self, wave_ref, wave_est, lens=None, resolutions=MR_STFT_RESOLUTIONS):
        """-> (float64 [B, R, 2] = (spectral convergence, log-magnitude distance) per resolution, frames int32 [B, R]) of the
        module-level mr_stft at the waves' own rate"""
        return mr_stft(wave_ref, wave_est, lens, resolutions)


_wave_scorers = {}


def wave_scorer(sample_rate, device):
    """the WaveScoreEngine of (sample rate, device), made once"""
    key = (int(sample_rate), str(device))
    if key not in _wave_scorers:
        _wave_scorers[key] = WaveScoreEngine(int(sample_rate), device=device)
    return _wave_scorers[key]


_levellers = {}


def leveller(sample_rate, device):
    """the LoudnessEngine of (sample rate, device), made once"""
    key = (int(sample_rate), str(device))
    if key not in _levellers:
        _levellers[key] = LoudnessEngine(int(sample_rate), device=device)
    return _levellers[key]


def level_spec(normalize):
    """One line's `normalize` option of the tts wrappers -> None (off) or (mode, target): 'peak' -> (1, 0.99), 'lufs' -> (2, -23.0), a
    number -> (2, that many LUFS).  ValueError for anything else."""
    if normalize is None:
        return None
    if isinstance(normalize, str):
        if normalize == 'peak':
            return 1, 0.99
        if normalize == 'lufs':
            return 2, -23.0
        raise ValueError(f"normalize: {normalize!r}: None, 'peak', 'lufs' or a target in LUFS")
    if isinstance(normalize, bool) or not isinstance(normalize, (int, float, np.integer, np.floating)) or not np.isfinite(float(normalize)):
        raise ValueError(f"normalize: {normalize!r}: None, 'peak', 'lufs' or a finite target in LUFS")
    return 2, float(normalize)


def check_normalize(normalize, n_lines):
    """Host-side validation of `normalize`: one option, or a list with one option per line (ValueError otherwise)."""
    if per_row(normalize):
        vals = row_values(normalize, n_lines, 'normalize')
        for v in vals:
            level_spec(v)
    else:
        level_spec(normalize)


def level_waves(wave, nsamples, normalize, sample_rate=22050, ceiling=0.99, limiter=None, true_peak=False):
    """The levelling step of the tts wrappers, after the denoiser and before the copy to the host: wave [B, n_max] on the device, row b
    levelled by its option (`normalize`: one option or one per row) over its nsamples[b] samples.  Only None: the wave as it is.
    limiter (None / False, True or a dict: limiter_spec): the rows with 'lufs' or a target go through the look-ahead limiter
    (LoudnessEngine.limit in mode 2: the full gain towards the target, the peaks held at the limiter's ceiling) instead of the capped
    gain; 'peak' and None rows keep their path.  true_peak: every peak above is the true peak (LoudnessEngine.level / limit with
    true_peak=True); with no row to level it is a ValueError, as a limiter is."""
    rows = list(normalize) if per_row(normalize) else [normalize] * wave.shape[0]
    specs = [level_spec(v) for v in rows]
    lim = limiter_spec(limiter)
    if not any(s is not None for s in specs):
        if lim is not None:
            raise ValueError("limiter: needs normalize ('lufs' or a target in LUFS on the rows it is to work on)")
        if true_peak:
            raise ValueError('true_peak: needs normalize or a limiter to work in')
        return wave
    if len(specs) != wave.shape[0]:
        raise ValueError(f'normalize: {len(specs)} values for {wave.shape[0]} rows')
    shape = wave.shape
    wave = wave.to(torch.float32).reshape(-1, shape[-1]).contiguous()
    eng = leveller(sample_rate, wave.device)
    tp = dict(true_peak=True) if true_peak else {}         # without it: the calls as they were
    if lim is None:
        eng.level(wave, nsamples, [s[0] if s else 0 for s in specs], [s[1] if s else 0.0 for s in specs], ceiling, **tp)
        return wave.reshape(shape)
    if any(s and s[0] == 1 for s in specs):
        eng.level(wave, nsamples, [1 if s and s[0] == 1 else 0 for s in specs], [s[1] if s else 0.0 for s in specs], ceiling, **tp)
    if any(s and s[0] == 2 for s in specs):
        eng.limit(wave, nsamples, [2 if s and s[0] == 2 else 0 for s in specs], [s[1] if s else 0.0 for s in specs], **lim, **tp)
    return wave.reshape(shape)

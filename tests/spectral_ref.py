"""Reference, data, cases and checker for the spectral back end: Vocos' backbone (dwconv7_kernel, LayerNorm at eps 1e-6, the GELU and
layer-scale epilogues of the conv engine, vocos_pad_channels_kernel) through ttsamd_vocos_features, its ISTFT head (vocos_spec_t_kernel,
vocos_istft_kernel, vocos_bias_kernel, the frame-major overlap_add_kernel in both trims) through ttsamd_vocos_head, and the denoiser
(denoise_fft_kernel, overlap_add_kernel, bias_frame0_kernel).  Plain module: tests/test_spectral_ref_cpu.py shows what
the checker rejects, tests/test_gpu_spectral.py holds the library to it.

Reference = the oracle's own pieces (oracle/tts_oracle.py: _vocos_backbone, vocos_forward, vocos_bias_vec, denoise; tests/melspec_ref.py:
vocos24_ref) at a `dtype`: float64 is the reference, float32 on the same data "the reference's own rounding".  Every bound is a multiple
R of that rounding error on the same data (fft_block_ref.check), never an absolute number.

What is restated here rather than taken from the oracle, each with switches for the mutants of the CPU test and each the oracle's own
function bit for bit when no switch is set (the CPU test asserts it):
  - `backbone`: O._vocos_backbone; with `lens` the padded batch whose convs read positions >= lens[b] as zero;
  - `head`: the part of O.vocos_forward / melspec_ref.vocos24_ref behind head.out, so that it can start from a given float32
    [1026, T] (log-magnitude | phase): both references then take exp, cos and sin of the exact same arguments;
  - `denoise`: O.denoise's torch.stft -> gain -> torch.istft.

Layout: every tensor handed to `check` has time (frames or samples) last; `lens[b]` positions of row b are valid."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import melspec_ref
import tts_oracle as O
from fft_block_ref import check                                               # noqa: F401  (the checker, shared)
from ttsamd import synth
from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG

N_FFT, HOP, N_BIN = 1024, 256, 513


# ---------------------------------------------------------------------------------------------------------------------------------
# geometries and weights
# ---------------------------------------------------------------------------------------------------------------------------------

# name -> (input channels, dim, intermediate dim, layers, padding)
GEOMS = {
    'L1': (80, 512, 1536, 1, 'same'),
    'L8': (80, 512, 1536, 8, 'same'),                                         # MelVocos('22k')
    '24k': (100, 512, 1536, 1, 'center'),                                     # one layer of MelVocos('24k'): vocos_pad_channels_kernel
    'W128': (80, 128, 1152, 1, 'same'),
    'W256': (80, 256, 1280, 1, 'same'),
    'W384': (80, 384, 1536, 1, 'same'),
    'W640': (80, 640, 1280, 1, 'same'),
}


def geom_cfg(name):
    in_ch, dim, inter, layers, padding = GEOMS[name]
    return dict(VOCOS_24K_CONFIG if padding == 'center' else VOCOS_22K_CONFIG, input_channels=in_ch, dim=dim, intermediate_dim=inter,
                num_layers=layers, padding=padding)


@functools.lru_cache(maxsize=None)
def weights(name):
    """Synthetic state dict of a geometry (numpy float32), built once."""
    return synth.vocos_state_dict(geom_cfg(name))


def _cast(sd, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# backbone: reference, data, cases
# ---------------------------------------------------------------------------------------------------------------------------------

BACKBONE_MUTANTS = ('eps', 'tanh_gelu', 'dw_past', 'embed_past', 'no_gamma')


def backbone(W, x, n_layers, mut=None, lens=None):
    """The oracle's _vocos_backbone (models.py:77-89 over modules.py:43-60), x [B, C, T] -> [B, T, dim], with the CPU test's mutants:
      'eps'        LayerNorm eps 1e-5                'tanh_gelu'   the tanh approximation of GELU       'no_gamma'  layer scale left out
      'dw_past'    the depthwise convs read positions >= lens[b]     'embed_past'  the embed conv does
    lens=None: the same ops in the same order as the oracle's.  With lens: the padded batch, every conv along time reading positions
    at or past a row's length as zero (what the kernels do) unless the mutant says otherwise."""
    eps = 1e-5 if mut == 'eps' else 1e-6

    def seen(t, skip):
        if lens is None or mut == skip:
            return t
        return t * (torch.arange(t.shape[-1])[None, None, :] < torch.as_tensor(lens)[:, None, None])
    x = F.conv1d(seen(x, 'embed_past'), W['backbone.embed.weight'], W['backbone.embed.bias'], padding=3)
    d = x.shape[1]
    x = F.layer_norm(x.transpose(1, 2), (d,), W['backbone.norm.weight'], W['backbone.norm.bias'], eps=eps).transpose(1, 2)
    for i in range(n_layers):
        p = f'backbone.convnext.{i}.'
        res = x
        y = F.conv1d(seen(x, 'dw_past'), W[p + 'dwconv.weight'], W[p + 'dwconv.bias'], padding=3, groups=d).transpose(1, 2)
        y = F.layer_norm(y, (d,), W[p + 'norm.weight'], W[p + 'norm.bias'], eps=eps)
        y = F.linear(y, W[p + 'pwconv1.weight'], W[p + 'pwconv1.bias'])
        y = F.gelu(y, approximate='tanh') if mut == 'tanh_gelu' else F.gelu(y)
        y = F.linear(y, W[p + 'pwconv2.weight'], W[p + 'pwconv2.bias'])
        if mut != 'no_gamma':
            y = W[p + 'gamma'] * y
        x = res + y.transpose(1, 2)
    return F.layer_norm(x.transpose(1, 2), (d,), W['backbone.final_layer_norm.weight'], W['backbone.final_layer_norm.bias'], eps=eps)


def features_ref(geom, mel, lens, dtype=torch.float64, mut=None):
    """head.out(backbone(mel)) -> {'feats': [B, 1026, T]} (log-magnitude | phase), row b = the reference's call on mel[b, :, :lens[b]]
    alone (csrc/vocos.hip: every layer reads positions >= lens[b] as zero); zero at and past a row's length.
    mut=None: the oracle's own _vocos_backbone.  The two *_past mutants run the padded batch, the others the restatement row by row."""
    cfg, W = geom_cfg(geom), _cast(weights(geom), dtype)
    x = torch.as_tensor(mel).to(dtype)
    B, _, T = x.shape
    out = torch.zeros(B, N_FFT + 2, T, dtype=dtype)
    if mut in ('dw_past', 'embed_past'):
        f = backbone(W, x, cfg['num_layers'], mut, lens)
        o = F.linear(f, W['head.out.weight'], W['head.out.bias']).transpose(1, 2)
        for b, n in enumerate(int(v) for v in lens):
            out[b, :, :n] = o[b, :, :n]
        return {'feats': out}
    for b, n in enumerate(int(v) for v in lens):
        if n:
            xb = x[b:b + 1, :, :n]
            f = O._vocos_backbone(W, xb, cfg['num_layers']) if mut is None else backbone(W, xb, cfg['num_layers'], mut)
            out[b, :, :n] = F.linear(f, W['head.out.weight'], W['head.out.bias']).transpose(1, 2)[0]
    return {'feats': out}


def mel_data(in_ch, B, T, seed=5, quiet=False):
    """randn * 1.5 - 4 [B, in_ch, T] float32 (the scale of the whole-model tests), NOT zeroed past a row's length: an unmasked read
    shows.  quiet: the same mel times 0.05 -- the embed conv's output is then small against its bias and the LayerNorm's variance
    small enough for its eps to matter (the 'eps' mutant: ratio 4 to 7 on the loud mel, above 100 on the quiet one)."""
    g = torch.Generator().manual_seed(seed)
    mel = torch.randn(B, in_ch, T, generator=g) * 1.5 - 4.0
    return (mel * 0.05 if quiet else mel).contiguous()


def _b8_lens():
    # 32 rows: the routes of the conv engine depend on batch x t_max, not on the lengths, so most rows are short and the float64
    # reference stays cheap
    return (324, 323, 257, 129, 33, 1, 0) + tuple(8 + (5 * i) % 29 for i in range(25))


# name -> (geometry, B, T, lens, quiet)
BACKBONE_CASES = {
    'B1': ('L1', 1, 4, (4,), False),                                          # the depthwise halo (3) is wider than the row
    'B2': ('L1', 3, 36, (36, 33, 1), False),                                  # the conv engine's 32-frame tile edge; a one-frame row
    'B2q': ('L1', 3, 36, (36, 33, 1), True),
    'B3': ('L1', 2, 264, (264, 257), False),                                  # the edge of dwconv7_kernel's 256-thread block
    'B4': ('L1', 3, 36, (36, 0, 20), False),                                  # a row of length 0 between two others
    'B5': ('L8', 2, 40, (40, 37), False),                                     # the full eight layers
    'B5q': ('L8', 2, 40, (40, 37), True),
    'B6': ('24k', 2, 36, (36, 31), False),                                    # 100 -> 104 input channels
    'B7-128': ('W128', 2, 36, (36, 33), False),
    'B7-256': ('W256', 2, 36, (36, 33), False),
    'B7-384': ('W384', 2, 36, (36, 33), False),
    'B7-640': ('W640', 2, 36, (36, 33), False),
    # The routes of the benchmark-size call (32 x 496 frames; csrc/conv_route.hip: conv_route): the three
    # k = 1 convs on the GEMM route of the F(4,3) kernel (from 512 blocks of 64 rows x 256 frames and t_max >= 256: pwconv2 needs
    # 32 x 257), the embed conv on the direct kernel's 128 x 64 tile (from 768 such tiles: 32 x 321).  32 x 324 is the smallest batch
    # of 32 with all four; at 32 x 256 pwconv2 stays on the direct kernel (its 128 x 128 tile, as the embed conv) next to pwconv1 and
    # head.out on the GEMM route.  The cases above run the direct kernel's 64 x 64 and "tiny" 128 x 64 tiles.  TTSAMD_WINO=0 sends
    # every launch of both to the direct kernel.
    'B8-256': ('L1', 32, 256, tuple(min(v, 256) for v in _b8_lens()), False),
    'B8-324': ('L1', 32, 324, _b8_lens(), False),
}


def backbone_case(name):
    geom, B, T, lens, quiet = BACKBONE_CASES[name]
    return geom, mel_data(GEOMS[geom][0], B, T, quiet=quiet), lens


# ---------------------------------------------------------------------------------------------------------------------------------
# head: reference, data, cases
# ---------------------------------------------------------------------------------------------------------------------------------

HEAD_MUTANTS = ('no_clamp_max', 'no_clamp_min', 'drop_bin512', 'steady_env', 'trim_shift', 'center_as_same')


def f32(v):
    """A strength as the float32 the library receives, for both references."""
    return float(np.float32(v))


def head(xo, padding, denoise, bias_vec, dtype, mut=None):
    """The oracle's vocos_forward (pretrained.py:79-93, ISTFT "same": spectral_ops.py:47-75) or, for "center", melspec_ref.vocos24_ref
    (torch.istft(center=True)) behind head.out: xo [B, 1026, T] already in `dtype` -> wave [B, 256 T] / [B, 256 (T - 1)].  Mutants:
      'no_clamp_max'   the clamp at 100 dropped                 'no_clamp_min'    the clamp at 0 dropped (shows under denoise)
      'drop_bin512'    the Nyquist bin zeroed                   'steady_env'      division by the steady-state envelope 1.5
      'trim_shift'     the "same" trim one sample late          'center_as_same'  "center" trimmed by 384 instead of 512
    mut=None: the same ops in the same order as the oracle's."""
    mag, ph = xo.chunk(2, dim=1)
    mag = torch.exp(mag)
    lo, hi = (None if mut == 'no_clamp_min' else 0.), (None if mut == 'no_clamp_max' else 1e2)
    mag = mag - denoise * bias_vec.to(dtype)
    mag = torch.clamp(mag, min=lo, max=hi) if (lo is not None or hi is not None) else mag
    S = mag * (torch.cos(ph) + 1j * torch.sin(ph))
    if mut == 'drop_bin512':
        S = S.clone()
        S[:, 512] = 0
    win = torch.hann_window(N_FFT, dtype=dtype)
    if padding == 'center' and mut != 'center_as_same':
        assert mut not in ('steady_env', 'trim_shift')                        # mutants of the "same" overlap-add
        return torch.istft(S, N_FFT, HOP, N_FFT, win, center=True)
    pad = (N_FFT - HOP) // 2
    B, N, T = S.shape
    ifft = torch.fft.irfft(S, N_FFT, dim=1, norm='backward') * win[None, :, None]
    out_size = (T - 1) * HOP + N_FFT
    y = F.fold(ifft, output_size=(1, out_size), kernel_size=(1, N_FFT), stride=(1, HOP))[:, 0, 0]
    env = F.fold(win.square().expand(1, T, -1).transpose(1, 2), output_size=(1, out_size), kernel_size=(1, N_FFT),
                 stride=(1, HOP)).squeeze()
    if mut == 'steady_env':
        env = torch.full_like(env, 1.5)
    if mut == 'trim_shift':
        return (y / env)[:, pad + 1:][:, :HOP * T - 1]
    if mut == 'center_as_same':
        return (y / env)[:, pad:][:, :HOP * (T - 1)]
    return y[:, pad:-pad] / env[pad:-pad]


def head_samples(padding, n):
    """Samples of a row of n frames."""
    return HOP * n if padding == 'same' else HOP * max(n - 1, 0)


def head_ref(feats, lens, padding, denoise_rows=None, bias_vec=None, dtype=torch.float64, mut=None):
    """feats float32 [B, 1026, T], lens -> {'wave': [B, head_samples(T)]}: row b = `head` on feats[b, :, :lens[b]] alone with the
    strength denoise_rows[b]; zero past a row's end (and everywhere for a row without samples)."""
    feats = torch.as_tensor(feats)
    assert feats.dtype == torch.float32
    B, _, T = feats.shape
    bias = torch.zeros(1, N_BIN, 1) if bias_vec is None else torch.as_tensor(bias_vec).reshape(1, N_BIN, 1)
    out = torch.zeros(B, head_samples(padding, T), dtype=dtype)
    for b, n in enumerate(int(v) for v in lens):
        m = head_samples(padding, n)
        if m:
            dn = 0.0 if denoise_rows is None else f32(denoise_rows[b])
            w = head(feats[b:b + 1, :, :n].to(dtype), padding, dn, bias, dtype, mut)[0]
            out[b, :w.shape[0]] = w                                           # (a mutant may hand back a sample less)
    return {'wave': out}


LN100 = np.float32(math.log(100.0))


def head_feats(B, T, seed=9):
    """Crafted head.out output [B, 1026, T] float32.  Log-magnitudes O(1) (N(-0.3, 0.8)), the Nyquist bin 512 a little louder (+ 1), and
    in every frame: bins 40 / 41 / 42 at ln 100 and its float32 neighbours below / above (the clamp's edge), bin 60 at + 90 (exp
    overflows float32: the result must be the clamp's 100), bin 61 at - 110 (exp underflows to 0).  Phases uniform in +- pi; bins
    100 .. 131 at +- 1e3 and 132 .. 163 at +- 1e4 plus the same uniform part (argument reduction)."""
    g = torch.Generator().manual_seed(seed)
    lm = torch.randn(B, N_BIN, T, generator=g) * 0.8 - 0.3
    lm[:, 512] += 1.0
    ln100 = torch.tensor(LN100)
    lm[:, 40] = ln100
    lm[:, 41] = torch.nextafter(ln100, torch.tensor(0.0))
    lm[:, 42] = torch.nextafter(ln100, torch.tensor(10.0))
    lm[:, 60] = 90.0
    lm[:, 61] = -110.0
    ph = (torch.rand(B, N_BIN, T, generator=g) * 2 - 1) * math.pi
    sign = torch.where(torch.arange(32) % 2 == 0, 1.0, -1.0)[None, :, None]
    ph[:, 100:132] += 1e3 * sign
    ph[:, 132:164] += 1e4 * sign
    return torch.cat([lm, ph], dim=1).contiguous()


def head_bias(seed=13):
    """A bias vector [513] in [0.5, 1.5]: at strength 5 it takes 2.5 to 7.5 off magnitudes whose median is exp(-0.3), so that most bins
    clamp to 0 and the loud ones do not."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N_BIN, generator=g) + 0.5).contiguous()


# name -> (padding, B, T, lens)
HEAD_CASES = {
    'same-1': ('same', 1, 1, (1,)),
    'same-36': ('same', 4, 36, (36, 32, 2, 0)),                               # the 32-frame tile of vocos_spec_t_kernel; a row of length 0
    'center-1': ('center', 1, 1, (1,)),                                       # no sample at all
    'center-2': ('center', 1, 2, (2,)),
    'center-36': ('center', 3, 36, (36, 33, 2)),
}
# strengths per case: None = no denoise, a scalar, or one value per row
HEAD_DENOISE = {'none': None, '0.3': 0.3, 'rows': (0.3, 0.0, 5.0, 0.3)}


def head_case(name):
    padding, B, T, lens = HEAD_CASES[name]
    return padding, head_feats(B, T), lens


def head_rows(denoise, B):
    """The per-row strengths of a HEAD_DENOISE entry for a batch of B (None: no denoise)."""
    d = HEAD_DENOISE[denoise]
    if d is None:
        return None
    return tuple(d[:B]) if isinstance(d, tuple) else (d,) * B


def bias_vec_ref(geom, dtype=torch.float64):
    """O.vocos_bias_vec -> {'bias_vec': [1, 513]}."""
    return {'bias_vec': O.vocos_bias_vec(weights(geom), geom_cfg(geom), dtype)[:, :, 0]}


# ---------------------------------------------------------------------------------------------------------------------------------
# denoiser: reference, data, cases
# ---------------------------------------------------------------------------------------------------------------------------------

DENOISE_MUTANTS = ('zero_pad', 'reflect_off1', 'sym_hann', 'frames_minus1', 'no_clamp', 'bias_mirrored')


def denoise(wave, bias_spec, strength, dtype=torch.float32, mut=None):
    """The oracle's denoise (denoiser.py:66-72: torch.stft -> max(|X| - strength * bias, 0), phase kept -> torch.istft), wave [1, n] ->
    [1, 256 (n // 256)], with the CPU test's mutants:
      'zero_pad'       zeros in place of the reflect padding          'reflect_off1'   the reflection repeats the edge sample
      'sym_hann'       the symmetric Hann window (denominator 1023)   'frames_minus1'  n // 256 frames, the last one missing
      'no_clamp'       the clamp at 0 dropped                         'bias_mirrored'  bias[512 - k] in place of bias[k]
    mut=None: the same calls as the oracle's."""
    wave = wave.to(dtype)
    bias_spec = torch.as_tensor(bias_spec).to(dtype)
    if mut == 'bias_mirrored':
        bias_spec = bias_spec.flip(-2)
    win = torch.hann_window(N_FFT, periodic=mut != 'sym_hann', dtype=dtype)
    kw = dict(normalized=False, onesided=True, return_complex=True)
    if mut == 'reflect_off1':
        x = torch.cat([wave[:, :N_FFT // 2].flip(1), wave, wave[:, -(N_FFT // 2):].flip(1)], dim=1)      # symmetric: the edge sample twice
        spec = torch.stft(x, N_FFT, HOP, N_FFT, win, center=False, **kw)
    else:
        spec = torch.stft(wave, N_FFT, HOP, N_FFT, win, center=True, pad_mode='constant' if mut == 'zero_pad' else 'reflect', **kw)
    mag, ph = spec.abs(), spec.angle()
    mag = mag - bias_spec * strength
    if mut != 'no_clamp':
        mag = torch.clamp(mag, 0.0)
    S = mag * torch.exp(1j * ph)
    if mut == 'frames_minus1':
        short = torch.istft(S[..., :-1], N_FFT, HOP, N_FFT, win, center=True, normalized=False, onesided=True)
        return F.pad(short, (0, HOP))
    return torch.istft(S, N_FFT, HOP, N_FFT, win, center=True, normalized=False, onesided=True)


def denoise_valid(n):
    """Samples torch.istft hands back for n input samples."""
    return HOP * (n // HOP)


def denoise_ref(wave, ns, bias, strengths, dtype=torch.float64, mut=None):
    """wave float32 [B, n_max], ns, bias float32 [513], strengths (one per row) -> {'wave': [B, n_max]}: row b = the oracle's denoise on
    wave[b, :ns[b]] alone over its first 256 (ns[b] // 256) samples, zero behind them.  A row whose strength is not > 0 is not run (the
    library leaves it untouched, which the GPU test asserts in bits): it stays zero here and gets no valid position from
    `denoise_lens`."""
    wave = torch.as_tensor(wave)
    assert wave.dtype == torch.float32
    out = torch.zeros(wave.shape, dtype=dtype)
    b3 = torch.as_tensor(bias).reshape(1, N_BIN, 1)
    for b, n in enumerate(int(v) for v in ns):
        s = f32(strengths[b])
        if s > 0:
            w = wave[b:b + 1, :n]
            r = O.denoise(w, b3, s, dtype) if mut is None else denoise(w, b3, s, dtype, mut)
            out[b, :r.shape[1]] = r[0]
    return {'wave': out}


def denoise_lens(ns, strengths):
    return tuple(denoise_valid(int(n)) if f32(s) > 0 else 0 for n, s in zip(ns, strengths))


def voiced_batch(ns, seed=21, zeros=None):
    """melspec_ref.voiced signals [B, max(ns)] float32, zero behind each row's length.  zeros = (row, start, count): that stretch of
    that row is set to exact zeros (at least 1024 + 512 samples, so that whole frames have |X| = 0 in every bin)."""
    wave = torch.zeros(len(ns), max(ns))
    for b, n in enumerate(ns):
        wave[b, :n] = torch.from_numpy(melspec_ref.voiced(n, seed + b))
    if zeros is not None:
        b, start, count = zeros
        assert count >= N_FFT + N_FFT // 2 and start + count <= ns[b]
        wave[b, start:start + count] = 0.0
    return wave.contiguous()


def denoise_bias(seed=17):
    """A positive random bias [513], U(0.05, 3): between nothing and most of a bin of the voiced signals at strength 1."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N_BIN, generator=g) * 2.95 + 0.05).contiguous()


# name -> (ns, zeros)
DENOISE_CASES = {
    'n513': ((513,), None),                                                   # one sample above the reflect padding's minimum
    'n768': ((768,), None),
    'n1000': ((1000,), None),
    'n4113': ((4113,), (0, 1200, 1700)),                                      # frames 7 .. 9 lie wholly inside the zeros
    'ragged': ((4113, 513, 2048, 1279), (0, 1200, 1700)),
}
DENOISE_STRENGTHS = (0.005, 1.0)
DENOISE_ROWS = (1.0, 0.0, 0.005, 1.0)                                         # the ragged batch, per row: row 1 untouched


def denoise_case(name):
    ns, zeros = DENOISE_CASES[name]
    return voiced_batch(ns, zeros=zeros), ns


def clamping_strength(wave, ns, bias):
    """A strength above max |X| / min bias over the batch (float64 STFT), times 2: every bin of every frame clamps to 0."""
    win = torch.hann_window(N_FFT, dtype=torch.float64)
    top = max(float(torch.stft(wave[b:b + 1, :n].double(), N_FFT, HOP, N_FFT, win, center=True, pad_mode='reflect',
                               return_complex=True).abs().max()) for b, n in enumerate(ns))
    return 2.0 * top / float(torch.as_tensor(bias).min())


BIAS_SPEC_N = 22528                                                           # the 88-frame call (denoiser.py:50-64)
BIAS_SPEC_NS = (BIAS_SPEC_N, 513)                                             # ... and the smallest wave the call accepts


def bias_spec_ref(audio, dtype=torch.float64):
    """|STFT| of frame 0 (O.denoiser_bias_spec behind the vocoder call) -> {'bias_spec': [1, 513]}."""
    x = torch.as_tensor(audio).reshape(1, -1).to(dtype)
    win = torch.hann_window(N_FFT, dtype=dtype)
    spec = torch.stft(x, N_FFT, HOP, N_FFT, win, center=True, pad_mode='reflect', normalized=False, onesided=True,
                      return_complex=True).abs()
    return {'bias_spec': spec[:, :, 0]}


# Bounds of the GPU test, as multiples of the reference's own float32 rounding error on the same data: ceil(2 x the worst ratio measured
# on the MI355X per family); the per-case table and how they were derived: profiles/r26/NOTES.md
R_BACKBONE_F32 = 6       # fp32, default conv routes (worst 2.51); also bias_vec (2.08) and the whole forward at T0 = 5 (1.29)
R_BACKBONE_DIRECT = 6    # fp32, TTSAMD_WINO=0: every conv on the direct MFMA kernel (worst 2.51)
R_BACKBONE_X3 = 36       # split bf16, set_precision('bf16x3') (worst 17.57)
R_HEAD = 3               # the head has no conv: one family (worst 1.12)
R_DENOISE = 3            # denoise_fft_kernel + overlap-add (worst 1.23)
# bias_frame0_kernel: one radix-4 FFT of frame 0, the transform of denoise_fft_kernel (1.30 on the 22 528-sample wave and 1.30 on 513
# samples, whose frame 0 holds the same 513 samples; profiles/r40/NOTES.md)
R_BIAS_SPEC = 3

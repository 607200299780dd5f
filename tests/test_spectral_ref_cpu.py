"""The checker of tests/spectral_ref.py has teeth (CPU only): every restatement is the oracle's own function bit for bit when no switch
is set, the reference's float32 run passes at R = 2, and float64 restatements with one thing wrong -- the mistakes a depthwise conv,
LayerNorm, GELU, spectrum, inverse-FFT, overlap-add or denoiser kernel can make and a whole-wave tolerance of 1e-4 cannot see -- come
out above the committed R of every run family that uses their case.  Ratios here (profiles/r26/NOTES.md has the table): LayerNorm eps
1e-5 moves head.out's output by 4 to 9 times the reference's own float32 rounding on the usual mel and by 230 to 320 times on the same mel
times 0.05, which is why the quiet cases exist; the tanh GELU by 130 to 300 times; the symmetric Hann window of the denoiser by 36 to 80
times at strength 0.005."""
import functools

import pytest
import torch
import torch.nn.functional as F

import melspec_ref
import spectral_ref as S
import tts_oracle as O
from fft_block_ref import _max_err

R_BACKBONE = max(S.R_BACKBONE_F32, S.R_BACKBONE_DIRECT, S.R_BACKBONE_X3)      # a mutant must fail under every family's bound


def ratios(got, ref64, ref32, lens, tag):
    """name -> max |got - ref64| / max |ref32 - ref64| over the valid positions; the reference's own rounding must not be 0 there."""
    out = {}
    for name, r64 in ref64.items():
        e, e_ref = _max_err(got[name], r64, lens), _max_err(ref32[name], r64, lens)
        assert e_ref > 0.0, f'{tag} {name}: the float32 reference equals the float64 one, no ratio can be formed'
        out[name] = e / e_ref
        print(f'{tag} {name} e {e:.3e} e_ref {e_ref:.3e} ratio {out[name]:.1f}')
    return out


# ---- the restatements are the oracle -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('geom', ['L8', '24k'])
def test_backbone_and_head_restatements_are_the_oracle(geom):
    """`backbone` = O._vocos_backbone and `head` behind it = O.vocos_forward ("same") / melspec_ref.vocos24_ref ("center"), bit for
    bit, in both precisions, with and without denoise."""
    cfg, w = S.geom_cfg(geom), S.weights(geom)
    mel = S.mel_data(cfg['input_channels'], 2, 12)
    for dtype in (torch.float32, torch.float64):
        W = S._cast(w, dtype)
        f = O._vocos_backbone(W, mel.to(dtype), cfg['num_layers'])
        assert torch.equal(S.backbone(W, mel.to(dtype), cfg['num_layers']), f)
        xo = F.linear(f, W['head.out.weight'], W['head.out.bias']).transpose(1, 2)
        bias = O.vocos_bias_vec(w, cfg, dtype)
        for dn in (0.0, S.f32(0.3)):
            whole = O.vocos_forward(w, mel, cfg, dn, bias, dtype) if geom == 'L8' else melspec_ref.vocos24_ref(w, mel, cfg, dn, bias, dtype)
            assert torch.equal(S.head(xo, cfg['padding'], dn, bias, dtype), whole)


def test_masked_backbone_is_the_rows_alone():
    """The padded batch with every conv reading zeros past a row's length (what the *_past mutants switch off) is the row alone: the
    same sums of the same products, so float64 agrees to its own rounding."""
    geom, mel, lens = S.backbone_case('B2')
    W = S._cast(S.weights(geom), torch.float64)
    r64 = S.features_ref(geom, mel, lens)['feats']
    f = S.backbone(W, mel.double(), 1, None, lens)
    o = F.linear(f, W['head.out.weight'], W['head.out.bias']).transpose(1, 2)
    for b, n in enumerate(lens):
        assert float((o[b, :, :n] - r64[b, :, :n]).abs().max()) < 1e-12


def test_denoise_restatement_is_the_oracle():
    wave, ns = S.denoise_case('n4113')
    bias = S.denoise_bias().reshape(1, S.N_BIN, 1)
    for dtype in (torch.float32, torch.float64):
        for s in (S.f32(0.005), 1.0):
            assert torch.equal(S.denoise(wave, bias, s, dtype), O.denoise(wave, bias, s, dtype))


def test_oracle_denoise_default_is_float32():
    """The dtype parameter changes nothing for the callers that do not pass it."""
    wave, _ = S.denoise_case('n768')
    out = O.denoise(wave.double(), S.denoise_bias().reshape(1, S.N_BIN, 1), 0.3)
    assert out.dtype == torch.float32 and torch.equal(out, O.denoise(wave, S.denoise_bias().reshape(1, S.N_BIN, 1), 0.3, torch.float32))


# ---- backbone ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bb(name):
    geom, mel, lens = S.backbone_case(name)
    return geom, mel, lens, S.features_ref(geom, mel, lens), S.features_ref(geom, mel, lens, torch.float32)


@pytest.mark.parametrize('name', list(S.BACKBONE_CASES))
def test_backbone_case_is_sound(name):
    """Every case: a non-zero float32 rounding to measure against, the float32 run inside R = 2, mel non-zero past every row's length."""
    geom, mel, lens, r64, r32 = _bb(name)
    assert ratios(r32, r64, r32, lens, f'backbone {name} fp32')['feats'] == 1.0
    S.check(r32, r64, r32, lens, 2, f'backbone {name} fp32 restatement')
    assert mel.shape[2] % 4 == 0
    for b, n in enumerate(lens):
        assert n == mel.shape[2] or bool((mel[b, :, n:] != 0).all())


# the case that rejects each mutant, under the widest backbone bound (split bf16 included)
BACKBONE_REJECTS = {'eps': ('B2q', 'B5q'), 'tanh_gelu': ('B2', 'B5'), 'dw_past': ('B2', 'B4'), 'embed_past': ('B2', 'B4'),
                    'no_gamma': ('B2', 'B5')}


@pytest.mark.parametrize('mut', S.BACKBONE_MUTANTS)
def test_backbone_mutant_is_rejected(mut):
    for name in BACKBONE_REJECTS[mut]:
        geom, mel, lens, r64, r32 = _bb(name)
        got = S.features_ref(geom, mel, lens, mut=mut)
        assert ratios(got, r64, r32, lens, f'backbone {name} mutant {mut}')['feats'] > R_BACKBONE
        with pytest.raises(AssertionError):
            S.check(got, r64, r32, lens, R_BACKBONE, f'backbone {name} mutant {mut}')


def test_eps_mutant_needs_the_quiet_mel():
    """LayerNorm eps 1e-5 on the usual mel stays under 10 times the float32 rounding, which a bound of that size cannot see: the quiet
    mel is the case that sees it under every family."""
    geom, mel, lens, r64, r32 = _bb('B2')
    loud = ratios(S.features_ref(geom, mel, lens, mut='eps'), r64, r32, lens, 'backbone B2 mutant eps')['feats']
    geom, mel, lens, r64, r32 = _bb('B2q')
    quiet = ratios(S.features_ref(geom, mel, lens, mut='eps'), r64, r32, lens, 'backbone B2q mutant eps')['feats']
    assert loud < 10 and quiet > R_BACKBONE and quiet > 10 * loud


# ---- head ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hd(name, denoise):
    padding, feats, lens = S.head_case(name)
    rows, bias = S.head_rows(denoise, len(lens)), S.head_bias()
    slens = tuple(S.head_samples(padding, n) for n in lens)
    return (padding, feats, lens, rows, bias, slens, S.head_ref(feats, lens, padding, rows, bias),
            S.head_ref(feats, lens, padding, rows, bias, torch.float32))


@pytest.mark.parametrize('denoise', list(S.HEAD_DENOISE))
@pytest.mark.parametrize('name', list(S.HEAD_CASES))
def test_head_case_is_sound(name, denoise):
    padding, feats, lens, rows, bias, slens, r64, r32 = _hd(name, denoise)
    if not any(slens):
        assert name == 'center-1' and r64['wave'].numel() == 0                # one centred frame: no sample
        return
    ratios(r32, r64, r32, slens, f'head {name} denoise {denoise} fp32')
    S.check(r32, r64, r32, slens, 2, f'head {name} denoise {denoise} fp32 restatement')
    for b, m in enumerate(slens):
        assert float(r64['wave'][b, m:].abs().max() if m < r64['wave'].shape[1] else 0.0) == 0.0
    # the corners are in the data: the clamp's edge from both sides, overflow, underflow, large phases, a loud Nyquist bin
    lm, ph = feats[:, :S.N_BIN].double(), feats[:, S.N_BIN:].double()
    assert bool((lm[:, 41].exp() < 100).all()) and bool((lm[:, 42].exp() > 100).all())
    assert bool(torch.isinf(feats[:, 60].exp()).all()) and bool((feats[:, 61].exp() == 0).all())
    assert float(ph[:, 100:132].abs().min()) > 990 and float(ph[:, 132:164].abs().min()) > 9990
    assert float(lm[:, 512].exp().min()) > 0.05


def test_head_denoise_clamps_most_bins():
    """Strength 5 with head_bias clamps most bins of its row to 0 and leaves the loud ones."""
    padding, feats, lens, rows, bias, *_ = _hd('same-36', 'rows')
    mag = feats[2, :S.N_BIN, :lens[2]].double().exp() - S.f32(rows[2]) * bias.double()[:, None]
    frac = float((mag <= 0).double().mean())
    assert 0.8 < frac < 1.0


# mutant -> (case, denoise) that rejects it
HEAD_REJECTS = {'no_clamp_max': ('same-36', 'none'), 'no_clamp_min': ('same-36', 'rows'), 'drop_bin512': ('same-36', 'none'),
                'steady_env': ('same-36', 'none'), 'trim_shift': ('same-36', 'none'), 'center_as_same': ('center-36', 'none')}


@pytest.mark.parametrize('mut', S.HEAD_MUTANTS)
def test_head_mutant_is_rejected(mut):
    padding, feats, lens, rows, bias, slens, r64, r32 = _hd(*HEAD_REJECTS[mut])
    got = S.head_ref(feats, lens, padding, rows, bias, mut=mut)
    assert ratios(got, r64, r32, slens, f'head mutant {mut}')['wave'] > S.R_HEAD
    with pytest.raises(AssertionError):
        S.check(got, r64, r32, slens, S.R_HEAD, f'head mutant {mut}')


def test_head_mutants_on_the_small_shapes():
    """T = 1 ("same") and T = 2 ("center") reject what they can see as well; the clamp at 0 is inert without denoise (exp >= 0), which
    is why its case runs with the per-row strengths."""
    padding, feats, lens, rows, bias, slens, r64, r32 = _hd('same-1', 'none')
    for mut in ('no_clamp_max', 'drop_bin512', 'steady_env', 'trim_shift'):
        assert ratios(S.head_ref(feats, lens, padding, rows, bias, mut=mut), r64, r32, slens, f'head same-1 mutant {mut}')['wave'] > S.R_HEAD
    assert torch.equal(S.head_ref(feats, lens, padding, rows, bias, mut='no_clamp_min')['wave'], r64['wave'])
    padding, feats, lens, rows, bias, slens, r64, r32 = _hd('center-2', 'none')
    for mut in ('no_clamp_max', 'drop_bin512', 'center_as_same'):
        assert ratios(S.head_ref(feats, lens, padding, rows, bias, mut=mut), r64, r32, slens, f'head center-2 mutant {mut}')['wave'] > S.R_HEAD


@pytest.mark.parametrize('geom', ['L8', '24k'])
def test_bias_vec_reference(geom):
    r64, r32 = S.bias_vec_ref(geom), S.bias_vec_ref(geom, torch.float32)
    ratios(r32, r64, r32, (S.N_BIN,), f'bias_vec {geom} fp32')
    assert float(r64['bias_vec'].min()) > 0 and float(r64['bias_vec'].max()) < 100     # the clip at 100 is the head cases' business


# ---- denoiser ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dn(name, strength):
    wave, ns = S.denoise_case(name)
    bias = S.denoise_bias()
    st = (strength,) * len(ns) if not isinstance(strength, tuple) else strength
    return wave, ns, bias, st, S.denoise_lens(ns, st), S.denoise_ref(wave, ns, bias, st), S.denoise_ref(wave, ns, bias, st, torch.float32)


@pytest.mark.parametrize('strength', S.DENOISE_STRENGTHS)
@pytest.mark.parametrize('name', list(S.DENOISE_CASES))
def test_denoise_case_is_sound(name, strength):
    wave, ns, bias, st, lens, r64, r32 = _dn(name, strength)
    ratios(r32, r64, r32, lens, f'denoise {name} strength {strength} fp32')
    S.check(r32, r64, r32, lens, 2, f'denoise {name} strength {strength} fp32 restatement')
    assert float((r64['wave'][0, :lens[0]] - wave[0, :lens[0]]).abs().max()) > 1e-4 * strength      # the setting changes the signal


def test_denoise_zero_stretch_has_silent_frames():
    """Frames 7 .. 9 of the 4113-sample row see zeros only: |X| = 0 in every bin (the kernel's mag == 0 branch)."""
    wave, ns = S.denoise_case('n4113')
    spec = torch.stft(wave.double(), 1024, 256, 1024, torch.hann_window(1024, dtype=torch.float64), center=True, pad_mode='reflect',
                      return_complex=True).abs()
    assert float(spec[0, :, 7:10].max()) == 0.0 and float(spec[0, :, 6].max()) > 0.0 and float(spec[0, :, 10].max()) > 0.0


@pytest.mark.parametrize('name', list(S.DENOISE_CASES))
def test_denoise_clamping_strength_gives_exact_zeros(name):
    wave, ns = S.denoise_case(name)
    bias = S.denoise_bias()
    s = S.clamping_strength(wave, ns, bias)
    for dtype in (torch.float64, torch.float32):
        assert float(S.denoise_ref(wave, ns, bias, (s,) * len(ns), dtype)['wave'].abs().max()) == 0.0


@pytest.mark.parametrize('mut', S.DENOISE_MUTANTS)
def test_denoise_mutant_is_rejected(mut):
    """Every mutant at both strengths, on the single row just above the padding's minimum and on the ragged batch."""
    for name in ('n513', 'ragged'):
        for strength in S.DENOISE_STRENGTHS:
            wave, ns, bias, st, lens, r64, r32 = _dn(name, strength)
            got = S.denoise_ref(wave, ns, bias, st, mut=mut)
            assert ratios(got, r64, r32, lens, f'denoise {name} strength {strength} mutant {mut}')['wave'] > S.R_DENOISE
            with pytest.raises(AssertionError):
                S.check(got, r64, r32, lens, S.R_DENOISE, f'denoise {name} mutant {mut}')


def test_denoise_rows_reference_skips_the_zero_row():
    wave, ns, bias, st, lens, r64, r32 = _dn('ragged', S.DENOISE_ROWS)
    assert lens[1] == 0 and float(r64['wave'][1].abs().max()) == 0.0
    ratios(r32, r64, r32, lens, 'denoise ragged rows fp32')


@pytest.mark.parametrize('n', S.BIAS_SPEC_NS)
def test_bias_spec_reference(n):
    audio = melspec_ref.voiced(n, 31)
    r64, r32 = S.bias_spec_ref(audio), S.bias_spec_ref(audio, torch.float32)
    ratios(r32, r64, r32, (S.N_BIN,), f'bias_spec fp32 n = {n}')
    assert r64['bias_spec'].shape == (1, S.N_BIN) and float(r64['bias_spec'].min()) > 0

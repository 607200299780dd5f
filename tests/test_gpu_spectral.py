"""The spectral back end against float64 through the C ABI (pytest -m gpu): Vocos' backbone through ttsamd_vocos_features
(dwconv7_kernel, LayerNorm at eps 1e-6, the GELU and layer-scale epilogues of the conv engine, vocos_pad_channels_kernel), its ISTFT head
through ttsamd_vocos_head on crafted inputs (vocos_spec_t_kernel, vocos_istft_kernel, overlap_add_kernel frame-major in both trims,
vocos_bias_kernel) and the denoiser (denoise_fft_kernel, overlap_add_kernel, bias_frame0_kernel).

Reference, data, cases and checker: tests/spectral_ref.py -- every run is compared with the float64 reference (never with another run),
over the valid positions, and must stay within R times the error of the same reference in float32 on the same data; every output must be
finite, padding included.  tests/test_spectral_ref_cpu.py shows what that bound rejects.  R per family: spectral_ref.R_*, derived in
profiles/r26/NOTES.md.  ttsamd_vocos_forward_windows is pinned to ttsamd_vocos_forward_rows bit for bit (tests/test_gpu_vocos_stream.py)
and head(features(x)) to forward(x) here, so the one-shot path held to float64 holds the stream too.

The denoiser's tail: torch.istft returns 256 (n // 256) samples; the library works in place and its overlap-add writes exactly those, so
the remaining n % 256 samples of a row (and everything behind its length) keep the INPUT's bits -- which is what
Denoiser.forward_batch hands back today, asserted below."""
import functools

import pytest
import torch

import melspec_ref
import spectral_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


_ENGINES = {}


def _engine(geom):
    """One Vocos engine per geometry for the whole module."""
    from ttsamd.engine import VocosEngine
    if geom not in _ENGINES:
        _ENGINES[geom] = VocosEngine(S.weights(geom), S.geom_cfg(geom))
    return _ENGINES[geom]


def _denoiser():
    from ttsamd.engine import DenoiserEngine
    if 'denoiser' not in _ENGINES:
        _ENGINES['denoiser'] = DenoiserEngine()
    return _ENGINES['denoiser']


def _lens(lens, dev):
    return torch.tensor(lens, dtype=torch.int64, device=dev)


# ---- backbone ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bb_refs(name):
    geom, mel, lens = S.backbone_case(name)
    return geom, mel, lens, S.features_ref(geom, mel, lens), S.features_ref(geom, mel, lens, torch.float32)


def _run_backbone(dev, ttsopt, name, bound, tag, wino=None):
    geom, mel, lens, r64, r32 = _bb_refs(name)
    if wino is not None:
        ttsopt.set('TTSAMD_WINO', wino)
    feats = _engine(geom).features(mel.to(dev), _lens(lens, dev))
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        assert float(feats[b, :, n:].abs().max() if n < feats.shape[2] else 0.0) == 0.0, 'frames past a row\'s length are written as zero'
    return S.check({'feats': feats}, r64, r32, lens, bound, f'{tag} backbone {name}')


@pytest.mark.parametrize('name', list(S.BACKBONE_CASES))
def test_backbone(dev, ttsopt, name):
    """B1 - B8 in fp32 on the default routes (B8: the k = 1 GEMM route of the benchmark-size call).  B4's row of length 0 comes back finite (zero) and leaves its neighbours what the
    reference says they are."""
    _run_backbone(dev, ttsopt, name, S.R_BACKBONE_F32, 'fp32')


@pytest.mark.parametrize('name', list(S.BACKBONE_CASES))
def test_backbone_direct_convs(dev, ttsopt, name):
    """The same with TTSAMD_WINO=0: every conv on the direct MFMA kernel.  The launches differ from the default family's in B8 only,
    whose k = 1 convs leave the GEMM route of the F(4,3) kernel (profiles/r26/NOTES.md: the route log)."""
    _run_backbone(dev, ttsopt, name, S.R_BACKBONE_DIRECT, 'fp32 WINO=0', wino='0')


@pytest.mark.parametrize('name', list(S.BACKBONE_CASES))
def test_backbone_split_bf16(dev, ttsopt, name):
    from ttsamd.engine import set_precision
    set_precision('bf16x3')
    try:
        _run_backbone(dev, ttsopt, name, S.R_BACKBONE_X3, 'bf16x3')
    finally:
        set_precision('f32')


def test_forward_pads_odd_lengths(dev):
    """T0 = 5 through VocosEngine.forward, which pads the frame axis to 8: the wave of the five frames against the float64 oracle's
    whole MelVocos.forward, under the backbone's bound (the head adds a thousandth of the backbone's rounding)."""
    import tts_oracle as O
    geom = 'L1'
    mel = S.mel_data(80, 2, 8)[:, :, :5].contiguous()
    lens = (5, 3)
    w, cfg = S.weights(geom), S.geom_cfg(geom)
    refs = []
    for dtype in (torch.float64, torch.float32):
        r = torch.zeros(2, 256 * 5, dtype=dtype)
        for b, n in enumerate(lens):
            r[b, :256 * n] = O.vocos_forward(w, mel[b:b + 1, :, :n], cfg, dtype=dtype)[0]
        refs.append({'wave': r})
    wave = _engine(geom).forward(mel.to(dev), _lens(lens, dev))
    assert wave.shape == (2, 1280) and float(wave[1, 768:].abs().max()) == 0.0
    S.check({'wave': wave}, refs[0], refs[1], (1280, 768), S.R_BACKBONE_F32, 'fp32 forward T0 = 5')


@pytest.mark.parametrize('denoise', ['none', '0.3', 'rows'])
@pytest.mark.parametrize('geom', ['L8', '24k'])
def test_head_of_features_is_forward(dev, geom, denoise):
    """head(features(mel)) == forward(mel) in bits, "same" and "center", without denoise, with a scalar and with per-row strengths."""
    eng = _engine(geom)
    lens = (40, 37, 9)
    mel = S.mel_data(S.GEOMS[geom][0], 3, 40).to(dev)
    dn = {'none': 0.0, '0.3': 0.3, 'rows': [0.3, 0.0, 5.0]}[denoise]
    whole = eng.forward(mel, _lens(lens, dev), denoise=dn)
    parts = eng.head(eng.features(mel, _lens(lens, dev)), _lens(lens, dev), denoise=dn)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(whole).all()) and float(whole.abs().max()) > 0.01
    assert torch.equal(parts, whole)


@pytest.mark.parametrize('dim,inter', [(128, 1152), (256, 1280), (384, 1536), (640, 1280)])
def test_widths_build_and_head_fits(dev, dim, inter):
    """Every width of B7 is accepted by ttsamd_vocos_create (dim and inter multiples of 128) and its hidden buffer holds the spectrum
    (inter >= 1026), so the whole forward runs: finite, non-zero."""
    geom = f'W{dim}'
    assert S.GEOMS[geom][1:3] == (dim, inter)
    wave = _engine(geom).forward(S.mel_data(80, 1, 8).to(dev))
    assert bool(torch.isfinite(wave).all()) and float(wave.abs().max()) > 1e-3


def test_narrow_hidden_buffer_is_refused(dev):
    """inter = 1024 < 1026: the spectrum does not fit the hidden buffer; the head and the whole forward are refused with an error, no
    launch."""
    from ttsamd import lib
    from ttsamd.engine import VocosEngine
    cfg = dict(S.geom_cfg('L1'), dim=128, intermediate_dim=1024)
    from ttsamd import synth
    eng = VocosEngine(synth.vocos_state_dict(cfg), cfg)
    with pytest.raises(lib.TtsAmdError, match='does not fit'):
        eng.forward(S.mel_data(80, 1, 8).to(dev))
    with pytest.raises(lib.TtsAmdError, match='does not fit'):
        eng.head(S.head_feats(1, 4).to(dev))


# ---- head ----------------------------------------------------------------------------------------------------------------------------

HEAD_GEOM = {'same': 'L1', 'center': '24k'}                                   # the head has no weights: any engine of the padding mode


@functools.lru_cache(maxsize=None)
def _head_refs(name, denoise):
    padding, feats, lens = S.head_case(name)
    rows, bias = S.head_rows(denoise, len(lens)), S.head_bias()
    return (padding, feats, lens, rows, bias, S.head_ref(feats, lens, padding, rows, bias),
            S.head_ref(feats, lens, padding, rows, bias, torch.float32))


def _run_head(dev, name, denoise):
    padding, feats, lens, rows, bias, r64, r32 = _head_refs(name, denoise)
    eng = _engine(HEAD_GEOM[padding])
    dn = 0.0 if rows is None else (rows[0] if denoise != 'rows' else list(rows))
    wave = eng.head(feats.to(dev), _lens(lens, dev), denoise=dn, bias_vec=bias)
    torch.cuda.synchronize()
    slens = tuple(S.head_samples(padding, n) for n in lens)
    assert tuple(wave.shape) == tuple(r64['wave'].shape)
    for b, m in enumerate(slens):
        assert float(wave[b, m:].abs().max() if m < wave.shape[1] else 0.0) == 0.0, 'samples past a row\'s end are exactly 0'
    if any(slens):
        S.check({'wave': wave}, r64, r32, slens, S.R_HEAD, f'head {name} denoise {denoise}')
    return wave


@pytest.mark.parametrize('denoise', list(S.HEAD_DENOISE))
@pytest.mark.parametrize('name', list(S.HEAD_CASES))
def test_head(dev, name, denoise):
    """Crafted log-magnitudes and phases (the clamp's edge, exp overflow and underflow, phases up to 1e4, a loud Nyquist bin) through
    ttsamd_vocos_head; "center" with one frame has no sample."""
    wave = _run_head(dev, name, denoise)
    if name == 'center-1':
        assert wave.numel() == 0


@pytest.mark.parametrize('name', ['same-36', 'center-36'])
def test_head_row_at_zero_has_the_bits_of_no_denoise(dev, name):
    """Row 1 of the per-row call (strength 0) == row 1 of the call without denoise; rows 0 and 3 == the scalar call at 0.3."""
    rows, none, scalar = _run_head(dev, name, 'rows'), _run_head(dev, name, 'none'), _run_head(dev, name, '0.3')
    assert torch.equal(rows[1], none[1])
    assert torch.equal(rows[0], scalar[0]) and not torch.equal(rows[0], none[0])
    if rows.shape[0] > 3:
        assert torch.equal(rows[3], scalar[3])


@pytest.mark.parametrize('geom', ['L8', '24k'])
def test_bias_vec(dev, geom):
    """ttsamd_vocos_bias_vec (the backbone on a zero mel of 88 frames, vocos_bias_kernel) against float64 make_denoising_vector."""
    got = _engine(geom).bias_vec().reshape(1, S.N_BIN)
    S.check({'bias_vec': got}, S.bias_vec_ref(geom), S.bias_vec_ref(geom, torch.float32), (S.N_BIN,), S.R_BACKBONE_F32, f'bias_vec {geom}')


# ---- denoiser ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dn_refs(name, strengths):
    wave, ns = S.denoise_case(name)
    bias = S.denoise_bias()
    return wave, ns, bias, S.denoise_ref(wave, ns, bias, strengths), S.denoise_ref(wave, ns, bias, strengths, torch.float32)


def _check_tail(out, wave, ns, strengths):
    """Behind the 256 (n // 256) samples torch.istft returns -- and in the whole of a row whose strength is not > 0 -- the input's bits."""
    for b, (n, s) in enumerate(zip(ns, strengths)):
        m = S.denoise_valid(n) if S.f32(s) > 0 else 0
        assert torch.equal(out[b, m:], wave[b, m:]), f'row {b}: samples from {m} on are not the input\'s'


def _run_denoise(dev, name, strengths, bias=None, refs=None, tag=''):
    per_row = isinstance(strengths, tuple)
    wave, ns = S.denoise_case(name)
    st = strengths if per_row else (strengths,) * len(ns)
    if refs is None:
        wave, ns, bias, r64, r32 = _dn_refs(name, st)
    else:
        r64, r32 = refs
    out = _denoiser().denoise(wave.to(dev).clone().contiguous(), _lens(ns, dev), bias.to(dev), list(st) if per_row else strengths).cpu()
    _check_tail(out, wave, ns, st)
    S.check({'wave': out}, r64, r32, S.denoise_lens(ns, st), S.R_DENOISE, f'denoise {name} strength {strengths}{tag}')
    return out


@pytest.mark.parametrize('strength', S.DENOISE_STRENGTHS)
@pytest.mark.parametrize('name', list(S.DENOISE_CASES))
def test_denoise(dev, name, strength):
    """n = 513 (one sample above the reflect padding's minimum), 768, 1000, 4113 (with frames of exact zeros) and the ragged batch, at
    the default strength 0.005 and at 1.0, with a positive random bias."""
    _run_denoise(dev, name, strength)


def test_denoise_rows(dev):
    """Per-row strengths (1.0, 0, 0.005, 1.0) on the ragged batch: the row at 0 untouched bit for bit, the others against float64."""
    _run_denoise(dev, 'ragged', S.DENOISE_ROWS)


@pytest.mark.parametrize('name', ['n513', 'n4113', 'ragged'])
def test_denoise_clamping_strength_gives_exact_zeros(dev, name):
    """A strength above max |X| / min bias: every bin clamps, the output is exactly 0 over the samples the inverse transform returns."""
    wave, ns = S.denoise_case(name)
    bias = S.denoise_bias()
    s = S.clamping_strength(wave, ns, bias)
    out = _denoiser().denoise(wave.to(dev).clone().contiguous(), _lens(ns, dev), bias.to(dev), s).cpu()
    assert bool(torch.isfinite(out).all())
    for b, n in enumerate(ns):
        assert float(out[b, :S.denoise_valid(n)].abs().max()) == 0.0
    _check_tail(out, wave, ns, (s,) * len(ns))


@functools.lru_cache(maxsize=None)
def _bias_spec_audio(n=S.BIAS_SPEC_N):
    return torch.from_numpy(melspec_ref.voiced(n, 31))


@pytest.mark.parametrize('n', S.BIAS_SPEC_NS)
def test_bias_spec(dev, n):
    """ttsamd_denoiser_bias_spec (bias_frame0_kernel: frame 0 of the centred framing, windowed, one 1024-point FFT in LDS, |X| of bins
    0 .. 512) against float64 |STFT| of frame 0, on a 22 528-sample wave (the 88-frame call) and on 513 samples, the smallest wave the
    call accepts: frame 0 then reflects on the left and ends on the row's last sample."""
    audio = _bias_spec_audio(n)
    got = _denoiser().bias_spec(audio.to(dev)).reshape(1, S.N_BIN)
    S.check({'bias_spec': got}, S.bias_spec_ref(audio), S.bias_spec_ref(audio, torch.float32), (S.N_BIN,), S.R_BIAS_SPEC,
            f'bias_spec n = {n}')


@pytest.mark.parametrize('strength', S.DENOISE_STRENGTHS)
def test_denoise_with_the_engines_own_bias(dev, strength):
    """The ragged batch with the bias the engine computed itself (scaled to the signals' level): the references take that very vector."""
    bias = (_denoiser().bias_spec(_bias_spec_audio().to(dev)).reshape(-1).cpu() * 0.05).contiguous()
    wave, ns = S.denoise_case('ragged')
    st = (strength,) * len(ns)
    refs = (S.denoise_ref(wave, ns, bias, st), S.denoise_ref(wave, ns, bias, st, torch.float32))
    _run_denoise(dev, 'ragged', strength, bias=bias, refs=refs, tag=' own bias')


def test_forward_batch_keeps_the_tail(dev):
    """Denoiser.forward_batch today: the n % 256 samples behind the last whole hop come back as they went in."""
    from vocoder.hifigan.denoiser import Denoiser
    wave, ns = S.denoise_case('ragged')
    bias = S.denoise_bias()

    class _NoVocoder:                                                         # the bias is given, no vocoder call behind it
        pass
    dn = Denoiser(_NoVocoder()).to(dev)
    dn._bias[str(dev)] = bias.reshape(1, S.N_BIN, 1).to(dev)
    out = dn.forward_batch(wave.to(dev).clone(), _lens(ns, dev), 1.0, nsamples_min=min(ns)).cpu()
    _check_tail(out, wave, ns, (1.0,) * len(ns))
    assert not torch.equal(out[0, :4096], wave[0, :4096])

"""GPU (pytest -m gpu): the fused wave -> (log-)mel kernel (csrc/melspec.hip) through the C ABI against the float64 restatement of the
reference's analysis (melspec_ref.mel_ref), MelVocos('24k') against its fp32 restatement and the reference's golden, reconstruct,
copy-synthesis and the error paths.

Tolerances.  Linear mel: not a fixed number -- the yardstick is the reference's own arithmetic, torch.stft in fp32 on the CPU, whose
max-abs error against float64 relative to the batch's largest mel value is measured in the same test; the HIP result's error, measured
the same way, may be at most 4x that (a radix-4 Stockham FFT with an fp32 twiddle table against pocketfft, and another summation order in
the filterbank; a mis-rounded twiddle or a dropped bin is orders of magnitude larger).  Log-mel: MEL_TOL = 1e-3 max-abs.  The inputs are
voiced-like so that min(mel_f64) >= 1e-4, 10x the log clip: the clamp never decides a comparison (asserted: a condition on the inputs).
Every figure is printed before it is asserted (run with -s to keep them)."""
import numpy as np
import pytest
import torch

from conftest import MEL_TOL, WAVE_TOL
import melspec_ref as R

pytestmark = pytest.mark.gpu


def maxabs(a, b):
    a, b = (np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


def batch_of(waves):
    n_max = max(len(w) for w in waves)
    x = np.zeros((len(waves), n_max), np.float32)
    for b, w in enumerate(waves):
        x[b, :len(w)] = w
        x[b, len(w):] = 7.0               # poison past the row's end: the kernel must not read it
    return x, np.array([len(w) for w in waves], np.int64)


def check_case(dev, waves, fb, framing, mag_mode, log, label):
    """Runs the ragged batch, every row alone and the batch again; compares with float64 per row.  Returns the figures."""
    from ttsamd.engine import MelSpecEngine
    eng = MelSpecEngine(fb, framing, 'eps' if mag_mode else 'abs', 1e-5 if log else None, device=dev)
    x, ns = batch_of(waves)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(ns).to(dev)
    mel, frames = eng.forward(xd, nd)
    mel2, _ = eng.forward(xd, nd)
    mel, frames = mel.cpu(), frames.cpu().numpy()
    assert torch.equal(mel, mel2.cpu()), 'two runs differ'
    add = 1 if framing == 'center' else 0
    assert mel.shape == (len(waves), fb.shape[0], x.shape[1] // 256 + add)
    assert np.array_equal(frames, ns // 256 + add)
    err_gpu = err_f32 = top = 0.0
    lo = np.inf
    for b, w in enumerate(waves):
        T = len(w) // 256 + add
        lin64 = R.mel_ref(w, fb, framing, mag_mode)[0]
        lo, top = min(lo, float(lin64.min())), max(top, float(lin64.max()))
        ref64 = torch.log(torch.clamp(lin64, min=1e-5)) if log else lin64
        ref32 = R.mel_ref(w, fb, framing, mag_mode, 1e-5 if log else None, dtype=torch.float32)[0]
        assert ref64.shape == (fb.shape[0], T)
        err_gpu = max(err_gpu, maxabs(mel[b, :, :T], ref64))
        err_f32 = max(err_f32, maxabs(ref32, ref64))
        assert float(mel[b, :, T:].abs().max()) == 0.0 if T < mel.shape[2] else True, 'frames past the row are not zero'
        alone, fa = eng.forward(torch.from_numpy(np.ascontiguousarray(w))[None].to(dev))
        assert int(fa[0]) == T and torch.equal(alone[0].cpu(), mel[b, :, :T]), f'row {b} differs from the call on it alone'
    if log:
        print(f'melspec {label}: log-mel max-abs err HIP {err_gpu:.3e}, fp32 CPU reference {err_f32:.3e} (tol {MEL_TOL}); min linear mel {lo:.2e}')
    else:
        print(f'melspec {label}: linear mel max-abs err / max mel: HIP {err_gpu / top:.3e}, fp32 CPU reference {err_f32 / top:.3e} '
              f'(bound 4x = {4 * err_f32 / top:.3e}); min linear mel {lo:.2e}')
    assert lo >= 1e-4, 'input condition: a mel value near the log clip'
    if log:
        assert err_gpu < MEL_TOL
    else:
        assert err_gpu <= 4.0 * err_f32
    return err_gpu, err_f32, top


def ragged_waves(framing):
    """Lengths that are no multiples of 256, one sample above the framing's minimum, and an utterance ending one sample before / on /
    after a frame boundary."""
    m = R.MIN_SAMPLES[framing]
    lens = [m + 1, 5 * 256 - 1, 5 * 256, 5 * 256 + 1, 3333, 9001, 14 * 256 + 129]
    return [R.voiced(n, 200 + i) for i, n in enumerate(lens)]


@pytest.mark.parametrize('log', [False, True], ids=['linear', 'log'])
@pytest.mark.parametrize('mag_mode', [0, 1], ids=['abs', 'eps'])
@pytest.mark.parametrize('framing,fbname', [('same', 'audio'), ('same', 'v24k'), ('center', 'audio'), ('center', 'v24k')])
def test_melspec_ragged_against_float64(dev, framing, fbname, mag_mode, log):
    check_case(dev, ragged_waves(framing), R.fbank(fbname), framing, mag_mode, log,
               f'{framing} {fbname} mag{mag_mode} {"log" if log else "lin"}')


@pytest.mark.parametrize('B', [1, 32])
def test_melspec_at_the_bench_lengths(dev, B):
    """B = 1 and B = 32 at the bench's utterance lengths (64 tokens of synth.synth_durations frames, 256 samples per frame)."""
    from ttsamd import synth
    lens = synth.synth_durations(32, 64).sum(axis=1).astype(np.int64)[:B] * 256
    waves = [R.voiced(int(n) + 17 * b, 300 + b) for b, n in enumerate(lens)]
    check_case(dev, waves, R.fbank('audio'), 'same', 1, False, f'bench lengths B={B} same/audio linear')
    check_case(dev, waves, R.fbank('v24k'), 'center', 0, True, f'bench lengths B={B} center/v24k log')


def test_melspec_dense_user_matrix(dev):
    """A dense random non-negative mel_basis (no zero structure) is summed in full."""
    rng = np.random.default_rng(5)
    fb = (rng.random((37, 513)) * 0.02).astype(np.float32)
    check_case(dev, [R.voiced(n, 400 + i) for i, n in enumerate((4000, 2049, 777))], fb, 'same', 1, False, 'dense 37 x 513 matrix')
    fb128 = (rng.random((128, 513)) * 0.02).astype(np.float32)
    check_case(dev, [R.voiced(6000, 410)], fb128, 'center', 0, False, 'dense 128 x 513 matrix')


def test_mel_spectrogram_module_and_replaced_basis(dev, golden):
    """utils.audio.MelSpectrogram against the reference's golden; a replaced mel_basis is the matrix the engine uses."""
    from utils.audio import MelSpectrogram
    g = golden('melspec')
    ms = MelSpectrogram().to(dev)
    for i in (0, 1):
        w = torch.from_numpy(g[f'wave_{i}']).to(dev)
        out = ms(w[None])
        ref = g[f'mel_audio_{i}']
        e = maxabs(out[0], ref) / float(ref.max())
        print(f'MelSpectrogram vs reference golden {i}: max-abs err / max mel {e:.3e}')
        assert out.shape == (1, 80, len(w) // 256) and e < 1e-6          # two fp32 computations of one value: a few eps each
        assert torch.equal(ms(w), out[0])                                # [n] in, [n_mels, T] out
    w = torch.from_numpy(g['wave_0']).to(dev)[None]
    before = ms(w)
    ms.mel_basis = ms.mel_basis * 2.0                                    # replaced buffer
    assert maxabs(ms(w), 2.0 * before.cpu()) <= 1e-6 * float(before.max())
    ms.mel_basis.mul_(0.5)                                               # written in place
    assert torch.equal(ms(w), before)


def test_mel_basis_made_under_inference_mode(dev, golden):
    """A buffer that is an inference tensor has no version counter (Tensor._version raises): the module still runs, same bits."""
    from utils.audio import MelSpectrogram
    w = torch.from_numpy(golden('melspec')['wave_0']).to(dev)[None]
    want = MelSpectrogram().to(dev)(w)
    with torch.inference_mode():
        ms = MelSpectrogram().to(dev)
    assert ms.mel_basis.is_inference()
    assert torch.equal(ms(w), want) and torch.equal(ms(w), want)


def test_feature_extractors_against_the_reference_golden(dev, golden):
    from vocoder.vocos.feature_extractors import MelSpectrogramFeatures
    from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG
    g = golden('melspec')
    for name, cfg in (('22k', VOCOS_22K_CONFIG), ('24k', VOCOS_24K_CONFIG)):
        fe = MelSpectrogramFeatures(**cfg['feature_extractor']).to(dev)
        for i in (0, 1):
            out = fe(torch.from_numpy(g[f'wave_{i}']).to(dev)[None])[0]
            e = maxabs(out, g[f'feat_{name}_{i}'])
            print(f'MelSpectrogramFeatures {name} vs reference golden {i}: log-mel max-abs err {e:.3e}')
            assert e < MEL_TOL


def _vocos24(dev):
    from ttsamd import synth
    from ttsamd.config import VOCOS_24K_CONFIG
    from vocoder.vocos import MelVocos
    w = synth.vocos_state_dict(VOCOS_24K_CONFIG)
    voc = MelVocos('24k')
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return voc.to(dev), w


def test_vocos_24k_golden_restatement_and_ragged(dev, golden):
    """MelVocos('24k') within the bounds test_vocos_golden_and_ragged uses for '22k': waves WAVE_TOL, bias_vec 1e-4."""
    import tts_oracle as O
    from ttsamd.config import VOCOS_24K_CONFIG as cfg
    g = golden('vocos_24k')
    voc, w = _vocos24(dev)
    assert maxabs(voc.bias_vec, g['bias_vec']) < 1e-4
    bias = O.vocos_bias_vec(w, cfg)
    for T in (2, 5, 24):
        mel = torch.from_numpy(g[f'mel_T{T}']).to(dev)
        out, out_dn = voc(mel), voc(mel, denoise=0.3)
        assert out.shape == (2, 256 * (T - 1))
        e = (maxabs(out, g[f'wave_T{T}']), maxabs(out_dn, g[f'wave_dn_T{T}']),
             maxabs(out, R.vocos24_ref(w, g[f'mel_T{T}'], cfg, bias_vec=bias)),
             maxabs(out_dn, R.vocos24_ref(w, g[f'mel_T{T}'], cfg, denoise=0.3, bias_vec=bias)))
        print(f"MelVocos('24k') T={T}: wave max-abs err vs golden {e[0]:.2e} / denoise {e[1]:.2e}, vs fp32 restatement {e[2]:.2e} / {e[3]:.2e}")
        assert max(e) < WAVE_TOL
    with pytest.raises(ValueError):
        voc(torch.zeros(1, 100, 1, device=dev))
    # ragged batch == per-utterance exact-length runs of the restatement; each row 256 (lens[b] - 1) samples long and zero beyond
    rng = np.random.default_rng(19)
    lens = [29, 7, 16, 2]
    mel = (rng.standard_normal((4, 100, 29)) * 1.5 - 4.0).astype(np.float32)
    wave = voc(torch.from_numpy(mel).to(dev), lens=torch.tensor(lens).to(dev)).cpu()
    assert wave.shape == (4, 256 * 28)
    for b, n in enumerate(lens):
        ref = R.vocos24_ref(w, mel[b:b + 1, :, :n], cfg, bias_vec=bias)[0]
        assert ref.shape == (256 * (n - 1),)
        assert maxabs(wave[b, :256 * (n - 1)], ref) < WAVE_TOL
        assert n == 29 or float(wave[b, 256 * (n - 1):].abs().max()) == 0.0
        if n >= 2:                      # ... and the GPU call on the utterance alone (its own T, padded to a multiple of 4 on its own)
            alone = voc(torch.from_numpy(mel[b:b + 1, :, :n]).to(dev)).cpu()
            assert alone.shape == (1, 256 * (n - 1)) and maxabs(wave[b, :256 * (n - 1)], alone[0]) < WAVE_TOL


@pytest.mark.parametrize('name', ['22k', '24k'])
def test_reconstruct_is_forward_of_the_features(dev, golden, name):
    from ttsamd import synth
    from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG
    from vocoder.vocos import MelVocos
    cfg = {'22k': VOCOS_22K_CONFIG, '24k': VOCOS_24K_CONFIG}[name]
    voc = MelVocos(name)
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.vocos_state_dict(cfg).items()})
    voc = voc.to(dev)
    x = torch.from_numpy(np.stack([R.voiced(6000, 500), R.voiced(6000, 501)])).to(dev)
    for dn in (0.0, 0.3):
        assert torch.equal(voc.reconstruct(x, denoise=dn), voc(voc.feature_extractor(x), denoise=dn))
    # ragged: the device-side frame counts of the analysis are the vocoder's lens
    lens = torch.tensor([6000, 3100])
    rec = voc.reconstruct(x, lens=lens.to(dev))
    alone = voc.reconstruct(x[1:2, :3100])
    n1 = alone.shape[1]
    assert maxabs(rec[1, :n1], alone[0]) < WAVE_TOL and float(rec[1, n1:].abs().max()) == 0.0
    if name == '24k':
        g = golden('vocos_24k')
        out = voc.reconstruct(torch.from_numpy(g['recon_in']).to(dev))
        e = maxabs(out, g['recon_out'])
        print(f"MelVocos('24k').reconstruct vs reference golden: max-abs err {e:.2e}")
        assert e < WAVE_TOL


def test_copy_synthesis_smoke(dev):
    """MelSpectrogram() of a HiFi-GAN V1 wave has the frame count of the mel that produced it, and is finite (synthetic weights: no
    numeric claim)."""
    from ttsamd import synth
    from ttsamd.engine import HifiGanEngine
    from utils.audio import MelSpectrogram
    rng = np.random.default_rng(3)
    mel = torch.from_numpy((rng.standard_normal((2, 80, 37)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    wave = HifiGanEngine(synth.hifigan_state_dict(), device=dev).forward(mel)
    back = MelSpectrogram().to(dev)(wave)
    assert back.shape == mel.shape and bool(torch.isfinite(back).all())


def test_error_paths(dev):
    from ttsamd import lib
    from ttsamd.engine import MelSpecEngine
    from ttsamd.lib import TtsAmdError
    from utils.audio import MelSpectrogram
    from vocoder.vocos.feature_extractors import MelSpectrogramFeatures
    fb = R.fbank('audio')
    with pytest.raises(TtsAmdError, match='n_fft'):
        MelSpecEngine(np.zeros((80, 257), np.float32), n_fft=512, device=dev)
    with pytest.raises(TtsAmdError, match='hop'):
        MelSpecEngine(fb, hop_length=128, device=dev)
    with pytest.raises(TtsAmdError, match='n_mels'):
        MelSpecEngine(np.zeros((129, 513), np.float32), device=dev)
    for kw in (dict(n_fft=512), dict(n_mels=129), dict(center=True)):
        with pytest.raises(TtsAmdError):
            MelSpectrogram(**kw)
    ms = MelSpectrogram().to(dev)
    with pytest.raises(ValueError, match='more than 384 samples'):
        ms(torch.zeros(1, 384, device=dev))
    with pytest.raises(ValueError, match='more than 512 samples'):
        MelSpectrogramFeatures().to(dev)(torch.zeros(1, 512, device=dev))
    with pytest.raises(TtsAmdError, match='no CPU fallback'):
        MelSpectrogram()(torch.zeros(1, 4000))                           # a module left on the CPU
    h = lib.load()
    assert h.ttsamd_vocos_set_padding(None, 2) != 0

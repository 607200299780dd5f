"""GPU: HiFi-GAN V3 (ResBlock2) on the fp32 MFMA path (csrc/resblock2.hip).  Kernel-level ttsamd_resblock2 against float64,
the generator against the real reference's golden and the float64 restatement (test_hifigan_v3_cpu.py), ragged batches,
routes and schedules, error paths, and the drop-in surface with a V3 json."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, WAVE_TOL
from test_hifigan_v3_cpu import generator_f64, resblock2_f64

pytestmark = pytest.mark.gpu

KERNEL_TOL = 2e-5                        # max-abs of one ResBlock2 against float64 (as test_gpu_fused.py)
SENTINEL = 7.25


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def v3():
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_V3_CONFIG
    return dict(HIFIGAN_V3_CONFIG), synth.hifigan_state_dict(HIFIGAN_V3_CONFIG, seed=0)


@pytest.fixture(scope='module')
def v3_engine(dev, v3):
    from ttsamd.engine import HifiGanEngine
    h, sd = v3
    return HifiGanEngine(sd, h, device=dev)


# every V3 (C, k, (d1, d2)) + the largest k / dilation the kernels take
GEOS = [(c, k, d) for c in (128, 64, 32) for k, d in ((3, (1, 2)), (5, (2, 6)), (7, (3, 12)))] + [(32, 11, (1, 16)), (64, 3, (16, 1))]
# 0, 3, one ending inside the halo of the second tile, one not a multiple of the tile, >= 3 tiles (tiles: 128 / 256 columns)
LENS = [0, 3, 261, 477, 785]
LMAX = 800


@pytest.mark.parametrize('C,k,dil', GEOS)
def test_resblock2_kernel_matches_f64(dev, C, k, dil):
    from ttsamd.engine import resblock2
    from ttsamd.lib import TtsAmdError
    g = torch.Generator().manual_seed(C * 100 + k * 10 + dil[1])
    B = len(LENS)
    x = torch.randn(B, C, LMAX, generator=g, dtype=torch.float64)
    s = 0.9 / np.sqrt(C * k)
    w1, w2 = (torch.randn(C, C, k, generator=g, dtype=torch.float64) * s for _ in range(2))
    b1, b2 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.05 for _ in range(2))
    y0 = torch.randn(B, C, LMAX, generator=g, dtype=torch.float64)
    for b, n in enumerate(LENS):
        y0[b, :, n:] = SENTINEL
    ref = [resblock2_f64(x[b:b + 1, :, :n], w1, b1, w2, b2, *dil)[0] if n else None for b, n in enumerate(LENS)]
    lens = torch.tensor(LENS, dtype=torch.int64, device=dev)
    xd, w1d, w2d, b1d, b2d = (t.float().to(dev) for t in (x, w1, w2, b1, b2))
    for variant in (1, 2):
        if variant == 2 and C == 128:
            with pytest.raises(TtsAmdError, match='variant 2'):
                resblock2(xd, w1d, b1d, w2d, b2d, *dil, lens=lens, variant=2)
            continue
        for mode, div in ((0, 1.0), (1, 1.0), (2, 3.0)):
            outs = []
            for _ in range(2):
                y = y0.float().to(dev)
                resblock2(xd, w1d, b1d, w2d, b2d, *dil, lens=lens, y=y, mode=mode, div=div, variant=variant)
                outs.append(y)
            torch.cuda.synchronize()
            assert torch.equal(outs[0], outs[1]), f'variant {variant} mode {mode}: not run-to-run deterministic'
            y = outs[0].double().cpu()
            for b, n in enumerate(LENS):
                assert torch.all(y[b, :, n:] == SENTINEL), f'variant {variant} mode {mode}: written past len {n}'
                if not n:
                    continue
                want = ref[b] if mode == 0 else (y0[b, :, :n] + ref[b]) / (div if mode == 2 else 1.0)
                err = float((y[b, :, :n] - want).abs().max())
                assert err < KERNEL_TOL, (variant, mode, n, err)


def test_resblock2_kernel_refuses_what_it_does_not_cover(dev):
    from ttsamd.engine import resblock2
    from ttsamd.lib import TtsAmdError
    x = torch.zeros(1, 32, 64, device=dev)
    w = torch.zeros(32, 32, 3, device=dev)
    b = torch.zeros(32, device=dev)
    with pytest.raises(TtsAmdError, match='variant 1'):
        resblock2(x, w, b, w, b, 1, 17, variant=1)               # dilation above 16
    with pytest.raises(TtsAmdError, match='variant'):
        resblock2(x, w, b, w, b, 1, 2, variant=3)
    w9 = torch.zeros(32, 32, 9, device=dev)
    with pytest.raises(TtsAmdError):
        resblock2(x, w9, b, w9, b, 1, 2, variant=2)              # k = 9 is not built


@pytest.mark.parametrize('T', [1, 7, 40])
def test_v3_generator_matches_reference_golden(dev, golden, v3_engine, T):
    g = golden('hifigan_v3')
    mel = torch.from_numpy(g[f'mel_T{T}']).to(dev)[None]
    wave = v3_engine.forward(mel)[0].cpu().numpy()
    want = g[f'wave_T{T}'].reshape(-1)
    assert wave.shape == want.shape
    err = float(np.abs(wave - want).max())
    assert err < WAVE_TOL, err


def test_v3_ragged_batch_rows_equal_unbatched(dev, v3_engine):
    lens = [23, 9, 16, 1]
    T = max(lens)
    rng = np.random.default_rng(3)
    mel = torch.from_numpy((rng.standard_normal((len(lens), 80, T)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    wave = v3_engine.forward(mel, torch.tensor(lens, device=dev)).cpu()
    for b, n in enumerate(lens):
        one = v3_engine.forward(mel[b:b + 1, :, :n].contiguous())[0].cpu()
        assert float((wave[b, :256 * n] - one).abs().max()) <= 1e-5, b
        assert torch.all(wave[b, 256 * n:] == 0), b


def test_v3_full_size_against_f64(dev, v3, v3_engine):
    """The bench's synthetic batch-32 lengths (64 tokens, durations 2..12) with seeded mels; a fixed subset of 8 rows (incl. the
    longest and the shortest) against the float64 restatement."""
    from ttsamd import synth
    h, sd = v3
    dur = np.asarray(synth.synth_durations(32, 64))
    lens = dur.reshape(32, -1).sum(axis=1).astype(np.int64)
    T = int(lens.max())
    rng = np.random.default_rng(5)
    mel = (rng.standard_normal((32, 80, T)) * 1.5 - 4.0).astype(np.float32)
    wave = v3_engine.forward(torch.from_numpy(mel).to(dev), torch.from_numpy(lens).to(dev)).cpu().numpy()
    rows = sorted({int(lens.argmax()), int(lens.argmin()), 0, 5, 11, 17, 23, 31})
    assert len(rows) >= 8 or len(set(rows)) == len(rows)
    worst = 0.0
    for b in rows:
        n = int(lens[b])
        want = generator_f64(sd, h, mel[b, :, :n])
        worst = max(worst, float(np.abs(wave[b, :256 * n] - want).max()))
        assert np.all(wave[b, 256 * n:] == 0)
    print(f'V3 full size: max-abs {worst:.3g} over rows {rows} (T = {T})')
    assert worst < WAVE_TOL, worst


def test_v3_routes_and_schedules(dev, v3_engine, ttsopt):
    lens = torch.tensor([40, 17, 33, 5], device=dev)
    rng = np.random.default_rng(9)
    mel = torch.from_numpy((rng.standard_normal((4, 80, 40)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    ttsopt.set('TTSAMD_RESBLOCK2_PAIR', '3f')                     # every C = 32 / 64 ResBlock2 as one resblock2_pair launch
    fused = v3_engine.forward(mel, lens).clone()
    ttsopt.set('TTSAMD_RESBLOCK2_PAIR', 0)
    unfused = v3_engine.forward(mel, lens).clone()
    ttsopt.set('TTSAMD_RESBLOCK2_PAIR', None)
    assert float((fused - unfused).abs().max()) <= 1e-5
    for mask in ('3f', None):                                     # both routes in both schedules
        ttsopt.set('TTSAMD_RESBLOCK2_PAIR', mask)
        outs = {}
        for streams in (0, 1):
            ttsopt.set('TTSAMD_HIFIGAN_STREAMS', streams)
            outs[streams] = [v3_engine.forward(mel, lens).clone() for _ in range(20)]
        ttsopt.set('TTSAMD_HIFIGAN_STREAMS', None)
        ref = outs[0][0]
        for s in (0, 1):
            for o in outs[s]:
                assert torch.equal(o, ref), f'mask {mask} streams={s}: not bit-identical'


def test_v3_errors(dev, v3):
    from ttsamd import engine
    from ttsamd.engine import HifiGanEngine
    from ttsamd.lib import TtsAmdError
    h, sd = v3
    eng = HifiGanEngine(sd, h, device=dev)
    mel = torch.zeros(1, 80, 4, device=dev) - 4.0
    try:
        for prec in ('bf16', 'bf16x3'):
            engine.set_precision(prec)
            with pytest.raises(TtsAmdError, match='f32'):
                eng.forward(mel)
    finally:
        engine.set_precision('f32')
    assert torch.isfinite(eng.forward(mel)).all()
    with pytest.raises(TtsAmdError, match='resblock'):
        HifiGanEngine(sd, dict(h, resblock='3'), device=dev)
    bad = dict(sd)
    key = 'resblocks.4.convs.1.parametrizations.weight.original1'
    bad[key] = np.zeros((64, 64, 3), np.float32)
    with pytest.raises(TtsAmdError, match='resblocks.4.convs.1'):
        HifiGanEngine(bad, h, device=dev)
    with pytest.raises(TtsAmdError, match='two dilations'):
        HifiGanEngine(sd, dict(h, resblock_dilation_sizes=[[1], [2], [3]]), device=dev)


def test_v3_dropin_fastpitch2wave_and_inference(dev, v3, synth_weights, tmp_path):
    import text
    import tts_oracle as O
    import inference
    from scipy.io import wavfile
    from ttsamd.config import NET_CONFIG
    from models.fastpitch import FastPitch2Wave
    h, sd = v3
    fpd = {k: torch.from_numpy(v.copy()) for k, v in synth_weights['fastpitch'].items()}
    torch.save({'model': fpd, 'config': dict(NET_CONFIG), 'symbols': list(text.symbols)}, tmp_path / 'fp.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in sd.items()}}, tmp_path / 'v3.pth')
    with open(tmp_path / 'v3.json', 'w') as f:
        json.dump(h, f)
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        lines = json.load(f)[:3]
    g = dict(np.load(os.path.join(GOLDEN, 'infer_text_ids.npz'), allow_pickle=False))
    model = FastPitch2Wave(str(tmp_path / 'fp.pth'), vocoder_sd=str(tmp_path / 'v3.pth'),
                           vocoder_config=str(tmp_path / 'v3.json')).to(dev)
    waves = model.tts(lines, batch_size=1, denoise=0)
    assert len(waves) == len(lines)
    fw = {k: v.to(dev) for k, v in O.to_torch(synth_weights['fastpitch']).items()}
    for i, w in enumerate(waves):
        ids = np.asarray(g['flat'][g['offsets'][i]:g['offsets'][i + 1]], np.int64)[None]
        with torch.backends.cudnn.flags(enabled=False), torch.inference_mode(), torch.device(dev):
            mel_ref, lens_ref, *_ = O.fastpitch_infer(fw, NET_CONFIG, ids)
        n = int(lens_ref[0])
        want = generator_f64(sd, h, mel_ref[0, :, :n].cpu().numpy())
        assert w.shape[-1] == want.shape[0], i
        err = float(np.abs(w.reshape(-1).numpy() - want).max())
        assert err < WAVE_TOL, (i, err)
    den = model.tts(lines, batch_size=1, denoise=0.005)
    assert [d.shape for d in den] == [w.shape for w in waves] and all(torch.isfinite(d).all() for d in den)
    lst = tmp_path / 'lines.txt'
    lst.write_text('\n'.join(lines) + '\n', encoding='utf-8')
    out = tmp_path / 'out'
    inference.main(['--list', str(lst), '--model', 'fastpitch', '--checkpoint', str(tmp_path / 'fp.pth'), '--vocoder_sd',
                    str(tmp_path / 'v3.pth'), '--vocoder_config', str(tmp_path / 'v3.json'), '--out_dir', str(out), '--batch_size', '2'])
    for i in range(len(lines)):
        sr, data = wavfile.read(out / 'wavs' / f'static{i}.wav')
        assert sr == 22050 and data.size > 0 and data.size % 256 == 0

"""CPU: the host side of streaming synthesis (ttsamd/stream.py) and the facts it rests on, checked on the oracles.

  * plan_chunks: cores partition the utterance, windows stay inside it, every halo is min(halo, distance to the edge);
  * the halo derivation (the Python mirror of ttsamd_hifigan_halo_frames): 13 / 13 for V1, and on the oracle generators (V1: tts_oracle,
    V3: the float64 restatement of test_hifigan_v3_cpu; narrow channels, the configs' own kernels, dilations and rates) NaN in every
    frame outside a window leaves its core clean while NaN in the outermost frame of the window reaches it: the halo is enough and tight;
  * the denoiser: windows with 3 frames of halo reproduce the whole-wave result on their cores;
  * PCM16: the restatement ttsamd_stream_emit is tested against equals save_wav's bytes.
The GPU tests are in test_gpu_stream.py."""
import os

import numpy as np
import pytest
import torch

from test_hifigan_v3_cpu import generator_f64

TS = [1, 2, 3, 12, 13, 14, 31, 32, 33, 95, 96, 97, 300]
FIRST_CHUNK = [(1, 1), (4, 8), (32, 64)]
HALOS = [(13, 13), (16, 16)]


@pytest.mark.parametrize('halo', HALOS)
@pytest.mark.parametrize('first,chunk', FIRST_CHUNK)
def test_plan_chunks_invariants(first, chunk, halo):
    from ttsamd.stream import max_core_frames, plan_chunks
    hl, hr = halo
    for T in TS:
        plan = plan_chunks(T, first, chunk, hl, hr)
        pos = 0
        for i, (cs, cn, ws, wn) in enumerate(plan):
            assert cs == pos and cn >= 1, (T, plan)                               # the cores partition [0, T) in order
            pos += cn
            assert 0 <= ws <= cs and cs + cn <= ws + wn <= T, (T, plan)           # the window holds its core and lies inside [0, T)
            assert cs - ws == min(hl, cs) and (ws + wn) - (cs + cn) == min(hr, T - cs - cn), (T, plan)
            assert cn >= chunk // 2 or len(plan) == 1, (T, plan)
            assert cn <= max_core_frames(first, chunk)
            if i == 0:
                assert cn == min(first, T) or len(plan) == 1
            elif i + 1 < len(plan):
                assert cn == chunk
        assert pos == T
        assert plan[0][2] == 0 and plan[-1][2] + plan[-1][3] == T                 # the edge windows start / end exactly at the edges
    # the remainder rule: 4 + 8 + 3 -> the 3 is folded (3 < 8 // 2), 4 + 8 + 4 is not
    assert [c[:2] for c in plan_chunks(15, 4, 8, 13, 13)] == [(0, 4), (4, 11)]
    assert [c[:2] for c in plan_chunks(16, 4, 8, 13, 13)] == [(0, 4), (4, 8), (12, 4)]
    for bad in ((0, 4, 8, 13, 13), (5, 0, 8, 13, 13), (5, 4, 0, 13, 13), (5, 4, 8, -1, 13)):
        with pytest.raises(ValueError):
            plan_chunks(*bad)


def test_halo_mirror_on_the_shipped_configs():
    from ttsamd.config import HIFIGAN_CONFIG, HIFIGAN_V3_CONFIG
    from ttsamd.stream import DENOISER_HALO, hifigan_halo_frames
    assert hifigan_halo_frames(HIFIGAN_CONFIG) == (13, 13)
    assert hifigan_halo_frames(HIFIGAN_V3_CONFIG) == (11, 11)
    assert DENOISER_HALO == 3


def _narrow(config, c0):
    """the config's own kernels, dilations and rates on few channels: the receptive field is the same, the oracle runs in milliseconds"""
    from ttsamd import synth
    h = dict(config, upsample_initial_channel=c0)
    return h, synth.hifigan_state_dict(h, seed=3, weight_norm=False)


def _oracle_v1(h, sd):
    import tts_oracle as O
    W = O.to_torch(sd)
    return lambda mel: O.hifigan_forward(W, torch.from_numpy(mel), h)[0].numpy()


def _oracle_v3(h, sd):
    return lambda mel: generator_f64(sd, h, mel)


@pytest.mark.parametrize('version', ['v1', 'v3'])
def test_halo_is_enough_and_tight_on_the_oracle_generators(version):
    from ttsamd.config import HIFIGAN_CONFIG, HIFIGAN_V3_CONFIG
    from ttsamd.stream import hifigan_halo_frames, plan_chunks
    h, sd = _narrow(HIFIGAN_CONFIG, 32) if version == 'v1' else _narrow(HIFIGAN_V3_CONFIG, 16)
    forward = (_oracle_v1 if version == 'v1' else _oracle_v3)(h, sd)
    hl, hr = hifigan_halo_frames(h)
    assert (hl, hr) == hifigan_halo_frames(HIFIGAN_CONFIG if version == 'v1' else HIFIGAN_V3_CONFIG)
    T = 48
    mel = (np.random.default_rng(5).standard_normal((80, T)) * 1.5 - 4.0).astype(np.float32)
    whole = forward(mel)
    assert whole.shape == (256 * T,) and np.isfinite(whole).all()
    # a middle window with both halos inside the utterance, found by the planner: first 4, chunks of 2 -> the core [20, 22)
    cs, cn, ws, wn = next(c for c in plan_chunks(T, 4, 2, hl, hr) if c[0] == 20)
    assert (ws, wn) == (cs - hl, cn + hl + hr) and ws > 0 and ws + wn < T
    core = slice(256 * cs, 256 * (cs + cn))
    poisoned = mel.copy()
    poisoned[:, :ws] = np.nan
    poisoned[:, ws + wn:] = np.nan
    out = forward(poisoned)
    assert np.isfinite(out[core]).all()                             # enough: nothing outside the window reaches the core
    assert np.array_equal(out[core], whole[core])
    for frame, sample in ((ws, core.start), (ws + wn - 1, core.stop - 1)):
        poisoned = mel.copy()
        poisoned[:, frame] = np.nan
        out = forward(poisoned)
        assert np.isnan(out[sample]), (version, frame)              # tight: the outermost frame of the window is needed
    # the window alone, cut at the halo, reproduces the core (zero padding at the cut is harmless by the same argument)
    # (a call of another length may sum in another order: a few fp32 ulps of a signal inside [-1, 1])
    alone = forward(np.ascontiguousarray(mel[:, ws:ws + wn]))
    assert np.abs(alone[256 * (cs - ws):256 * (cs - ws + cn)] - whole[core]).max() <= 1e-6


def test_denoiser_windows_with_three_frames_of_halo_reproduce_the_core():
    import tts_oracle as O
    from ttsamd.stream import DENOISER_HALO, plan_chunks
    g = torch.Generator().manual_seed(21)
    T = 40
    wave = torch.randn(1, 256 * T, generator=g) * 0.1
    bias = torch.rand(1, 513, 1, generator=g) * 0.5
    whole = O.denoise(wave, bias, 0.3)
    assert whole.shape == wave.shape and float((whole - wave).abs().max()) > 1e-3
    plan = plan_chunks(T, 4, 8, DENOISER_HALO, DENOISER_HALO)
    assert len(plan) >= 4
    for cs, cn, ws, wn in (plan[0], plan[2], plan[-1]):             # a window at the start, one in the middle, one at the end
        out = O.denoise(wave[:, 256 * ws:256 * (ws + wn)], bias, 0.3)
        got = out[0, 256 * (cs - ws):256 * (cs - ws + cn)]
        assert torch.equal(got, whole[0, 256 * cs:256 * (cs + cn)]), (cs, cn, float((got - whole[0, 256 * cs:256 * (cs + cn)]).abs().max()))
    # one frame less is not enough (middle window): the halo is tight
    cs, cn, ws, wn = plan[2]
    out = O.denoise(wave[:, 256 * (ws + 1):256 * (ws + wn - 1)], bias, 0.3)
    assert not torch.equal(out[0, 256 * (cs - ws - 1):256 * (cs - ws - 1 + cn)], whole[0, 256 * cs:256 * (cs + cn)])


def test_pcm16_restatement_equals_save_wav(tmp_path):
    from ttsamd.stream import pcm16
    from utils.audio import save_wav
    ties = [(k + 0.5) / 32767.0 for k in (0, 1, 2, 3, 100, 101, 32765, 32766)]
    x = np.array([0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5, 100.0, -100.0, 1e-9, -1e-9, float('nan'), 32767.5 / 32767.0, -32768.5 / 32767.0]
                 + ties + [-t for t in ties], dtype=np.float32)
    x = np.concatenate([x, np.random.default_rng(2).uniform(-1.2, 1.2, 4096).astype(np.float32)])
    got = pcm16(x)
    assert got.dtype == np.dtype('<i2') and got[11] == 0 and got[1] == 32767 and got[2] == -32767 and got[7] == 32767 and got[8] == -32768
    prod = x[14:14 + len(ties)] * np.float32(32767.0)
    exact = prod == np.floor(prod) + 0.5                           # the fp32 products that land ON a tie go to the even neighbour
    assert exact.any() and (got[14:14 + len(ties)][exact] % 2 == 0).all()
    path = os.path.join(tmp_path, 'x.wav')
    with np.errstate(invalid='ignore'):
        save_wav(path, x)
    with open(path, 'rb') as f:
        raw = f.read()
    assert raw[44:] == got.tobytes()

"""CPU: Vocos in the chunked vocoder (ttsamd/stream.py), the host side and the fact it rests on.

  * the receptive field, on the float64 oracles ('22k': tts_oracle.vocos_forward, '24k': melspec_ref.vocos24_ref) with the synthetic
    weights at full width: a window with `vocos_halo_frames(config)` frames around its core gives on the core the whole-utterance wave
    with difference EXACTLY 0.0 (the same float64 sums of the same terms), one frame less on either side does not.  With these weights
    an off-by-one is 2e-10 ... 1e-9, far below what an fp32 GPU test could see: this test is what pins the halo;
  * `vocos_halo_frames` on the shipped configs and on a 2-layer one;
  * `plan_chunks_center`: the cores partition the 256 (T - 1) samples of a "center" utterance in order, none is empty, the windows
    hold every frame the cores' samples depend on;
  * the two new symbols are in the header and in the binding.
The GPU tests are in test_gpu_vocos_stream.py."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

T_UTT, CORE, DENOISE = 90, (35, 43), 0.3


def _mel(n_mels, T, seed):
    return (np.random.default_rng(seed).standard_normal((n_mels, T)) * 1.5 - 4.0).astype(np.float32)


@pytest.fixture(scope='module', params=['22k', '24k'])
def oracle(request):
    """(config, forward(mel [n_mels, T] float32) -> float64 wave of 256 T ('22k') or 256 (T - 1) ('24k') samples at DENOISE,
    the whole-utterance wave of the T_UTT-frame mel, that mel)"""
    import melspec_ref as R
    import tts_oracle as O
    from ttsamd import synth
    from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG
    cfg = {'22k': VOCOS_22K_CONFIG, '24k': VOCOS_24K_CONFIG}[request.param]
    w = synth.vocos_state_dict(cfg)
    bias = O.vocos_bias_vec(w, cfg, torch.float64)
    fwd = O.vocos_forward if request.param == '22k' else R.vocos24_ref

    def forward(mel):
        return fwd(w, mel[None], cfg, denoise=DENOISE, bias_vec=bias, dtype=torch.float64)[0].numpy()
    mel = _mel(cfg['input_channels'], T_UTT, 7)
    whole = forward(mel)
    assert whole.dtype == np.float64 and whole.shape == (256 * (T_UTT - (cfg['padding'] == 'center')),)
    return cfg, forward, whole, mel


def _core_diff(oracle, core, left, right):
    """max-abs over the samples of the frames `core` between the whole-utterance wave and the wave of the window with `left` / `right`
    frames around the frames the core occupies, clipped at the utterance"""
    cfg, forward, whole, mel = oracle
    c0, c1 = core
    ws, we = max(c0 - left, 0), min(c1 + right, T_UTT)
    win = forward(mel[:, ws:we])
    return float(np.abs(win[256 * (c0 - ws):256 * (c1 - ws)] - whole[256 * c0:256 * c1]).max())


def test_halo_is_exact_and_tight_in_float64(oracle):
    from ttsamd.stream import vocos_halo_frames
    left, right = vocos_halo_frames(oracle[0])
    exact = _core_diff(oracle, CORE, left, right)
    short_l, short_r = _core_diff(oracle, CORE, left - 1, right), _core_diff(oracle, CORE, left, right - 1)
    print(f"{oracle[0]['padding']}: halo ({left}, {right}): core difference {exact:.1e}; one frame less left {short_l:.1e}, right {short_r:.1e}")
    assert exact == 0.0
    assert short_l > 0.0 and short_r > 0.0


def test_windows_at_the_utterance_edges_are_exact(oracle):
    """a window that starts at the utterance's first frame, one that ends at its last sample, and every window of a plan"""
    from ttsamd.stream import plan_chunks, plan_chunks_center, vocos_halo_frames
    cfg, forward, whole, mel = oracle
    left, right = vocos_halo_frames(cfg)
    n_frames = whole.size // 256
    assert _core_diff(oracle, (0, 8), left, right) == 0.0
    assert _core_diff(oracle, (3, 30), left, right) == 0.0                        # left halo clipped to 3 frames
    assert _core_diff(oracle, (n_frames - 8, n_frames), left, right) == 0.0
    assert _core_diff(oracle, (n_frames - 40, n_frames - 5), left, right) == 0.0  # right halo clipped
    plan = (plan_chunks_center if cfg['padding'] == 'center' else plan_chunks)(T_UTT, 8, 16, left, right)
    parts = []
    for cs, cn, ws, wn in plan:
        parts.append(forward(mel[:, ws:ws + wn])[256 * (cs - ws):256 * (cs + cn - ws)])
    assert np.array_equal(np.concatenate(parts), whole)


def test_halo_frames_of_the_configs():
    from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG
    from ttsamd.stream import vocos_halo_frames
    assert vocos_halo_frames(VOCOS_22K_CONFIG) == (29, 29)
    assert vocos_halo_frames(VOCOS_24K_CONFIG) == (28, 29)
    assert vocos_halo_frames(dict(VOCOS_22K_CONFIG, num_layers=2)) == (11, 11)
    assert vocos_halo_frames(dict(VOCOS_24K_CONFIG, num_layers=2)) == (10, 11)
    with pytest.raises(ValueError):
        vocos_halo_frames(dict(VOCOS_22K_CONFIG, padding='valid'))


@pytest.mark.parametrize('first,chunk', [(1, 1), (4, 8), (8, 16), (32, 64), (5, 1)])
def test_plan_chunks_center_invariants(first, chunk):
    from ttsamd.stream import max_core_frames, plan_chunks, plan_chunks_center
    hl, hr = 28, 29
    for T in (2, 3, 9, 33, 64, 65, 200):
        plan = plan_chunks_center(T, first, chunk, hl, hr)
        pos = 0
        for cs, cn, ws, wn in plan:
            assert cs == pos and cn >= 1, (T, plan)                               # in order, none empty
            pos += cn
            # the samples of the frames [cs, cs + cn) read the mel frames [cs - hl, cs + cn + hr) of [0, T): the window is exactly those
            assert ws == max(cs - hl, 0) and ws + wn == min(cs + cn + hr, T), (T, plan)
            assert wn >= cn + 1 and cn <= max_core_frames(first, chunk)
        assert pos == T - 1                                                       # hop * (T - 1) samples: [0, 256 (T - 1)) is partitioned
        assert [c[:2] for c in plan] == [c[:2] for c in plan_chunks(T - 1, first, chunk, hl, hr)]
        assert plan[0][2] == 0 and plan[-1][2] + plan[-1][3] == T
    for bad in (1, 0):
        with pytest.raises(ValueError):
            plan_chunks_center(bad, first, chunk, hl, hr)


def test_new_symbols_are_declared_and_bound():
    from ttsamd import lib
    with open(os.path.join(REPO, 'include', 'ttsamd.h')) as f:
        declared = set(re.findall(r'\b(ttsamd_[a-z0-9_]+)\s*\(', f.read()))
    for name in ('ttsamd_vocos_halo_frames', 'ttsamd_vocos_forward_windows'):
        assert name in declared and name in lib.SYMBOLS, name


def test_melvocos_states_the_rate_of_its_wave():
    from vocoder.vocos import MelVocos
    assert MelVocos('22k').sampling_rate == 22050 and MelVocos('24k').sampling_rate == 24000
    assert MelVocos('22k').config['feature_extractor']['sample_rate'] == 24000    # the reference's quirk stays where it is

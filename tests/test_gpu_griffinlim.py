"""csrc/griffinlim.hip on the GPU against its numpy restatement (tests/griffinlim_ref.py, pinned by tests/test_griffinlim_cpu.py).

Inputs: wavescore_ref.speech_like at 22 050 Hz plus white noise at 20 dB (griffinlim_ref.test_signal); `mag` is the magnitude of the
restatement's own STFT, rounded to float32 (kernel and restatement get the same values); every buffer handed to the kernel is NaN
behind a row's frames.

Tolerances are the reference's own rounding noise, never the kernel's: the wave bound of a case is 8 x max |ref_float32 - ref_float64|
of that same case (the restatement run in float32 on numpy's pocketfft), with a floor of 1e-6 x the wave's peak; the complex
`mag * angles` is compared per frame, relative to the frame's largest magnitude, under the same rule (floor 1e-6).  The factor 8 covers
a radix-4 Stockham transform with twiddles rounded from double against pocketfft; a structural error moves these numbers by 1e-2 or
more (the mutants of the CPU test: > 100 x the float32 noise).  Raw angles are not compared: on this signal a third of the bins lie
below 1e-3 of their frame's maximum and their phase is noise in any precision.  `inconsistency`: 1e-4 relative at 1 and 2 iterations.

Values the bounds took on the first green run (MI355X; per case over the frame counts below; profiles/r39/NOTES.md has the table with
the kernel's errors beside them):
    iterations, momentum      wave bound (center | same)             mag * angles bound (center | same)
    0                         8.6e-8 .. 6.2e-7 | 3.1e-8 .. 7.6e-7    1e-6 (the floor; the kernel's error is 0: the angles are the given ones)
    1, 0 and 0.99             3.1e-7 .. 7.8e-6 | 7.4e-8 .. 1.9e-6    4.0e-6 .. 9.2e-5 | 1.9e-6 .. 1.3e-4
    2, 0                      1.0e-6 .. 1.4e-5 | 9.3e-8 .. 2.6e-6    7.3e-6 .. 2.4e-4 | 2.2e-6 .. 1.8e-4
    2, 0.99                   4.6e-7 .. 7.9e-5 | 1.0e-7 .. 3.2e-6    8.3e-6 .. 1.8e-3 | 2.5e-6 .. 1.8e-4
    32, 0.99 (33, 120 frames) 4.2e-4 .. 5.3e-4 | 1.8e-4 .. 1.9e-3    6.6e-2 .. 2.7e-1 | 6.7e-3 .. 2.3e-2
The kernel's largest share of a bound on that run: 0.26 (waves), 0.74 (mag * angles; 2 iterations at momentum 0.99).  Wave peaks 0.02 ..
0.74."""
import json
import os

import numpy as np
import pytest
import torch

import griffinlim_ref as G
import melspec_ref as MR
from conftest import GOLDEN
from test_gpu_tacotron2 import LINES as TACO_LINES, taco_ckpt                                   # noqa: F401

pytestmark = pytest.mark.gpu

FPB = 2                                                             # frames per block of gl_iter_kernel (GL_FPB): one pair
# the minimum (2 / 4; minimum - 1 is refused); F, F + 1 and 2 F + 1 = 2, 3, 5 (F - 1 = 1 is below both minima; 3 and 5 are also the odd
# counts whose last frame has no partner); 15 .. 17 and 33: even / odd counts over several blocks; one row of 120 frames
FRAMES = {'same': (2, 3, 5, 15, 16, 17, 33, 120), 'center': (4, 5, 15, 16, 17, 33, 120)}
assert FPB == 2 and all(T in FRAMES['same'] for T in (FPB, FPB + 1, 2 * FPB + 1))
CASES = [(f, T) for f in ('same', 'center') for T in FRAMES[f]]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def eng(dev):
    from ttsamd.engine import GriffinLimEngine
    return GriffinLimEngine(device=dev)


_inputs = {}


def inputs(framing, T, seed=0):
    """(mag [T, 513] float32, initial angles [T, 513] complex64) of a case, made once"""
    key = (framing, T, seed)
    if key not in _inputs:
        x = G.test_signal(G.samples(T, framing), seed=seed)
        _inputs[key] = (np.abs(G.stft(x, framing)).astype(np.float32), G.hash_phase(T, seed=100 + T + seed).astype(np.complex64))
    return _inputs[key]


_refs = {}


def refs(framing, T, n_iter, momentum, seed=0):
    """(float64 result, float32 result) of the restatement from the case's given phases, made once and left unchanged"""
    key = (framing, T, n_iter, momentum, seed)
    if key not in _refs:
        mag, ang = inputs(framing, T, seed)
        _refs[key] = (G.griffinlim(mag, n_iter, momentum, framing, init=2, phase=ang),
                      G.griffinlim(mag, n_iter, momentum, framing, init=2, phase=ang, dtype=np.float32))
    return _refs[key]


def run(eng, rows, framing, n_iter, momentum, init='phase', seed=0, t_max=None, frames_on_device=False):
    """rows: list of (mag [T, 513], angles [T, 513] or None).  Buffers are NaN behind each row's frames.  -> (wave [B, n(t_max)],
    phase [B, t_max, 513], inconsistency [B]) as numpy"""
    Ts = [m.shape[0] for m, _ in rows]
    t_max = max(Ts) + 1 if t_max is None else t_max
    mag = np.full((len(rows), 513, t_max), np.nan, dtype=np.float32)
    ph = np.full((len(rows), t_max, 513), np.nan + 1j * np.nan, dtype=np.complex64)
    for b, (m, a) in enumerate(rows):
        mag[b, :, :Ts[b]] = m.T
        if a is not None:
            ph[b, :Ts[b]] = a
    frames = torch.tensor(Ts, dtype=torch.int32).to(eng.device) if frames_on_device else Ts
    wave, phase, inc = eng.forward(torch.from_numpy(mag).to(eng.device), frames, n_iter=n_iter, momentum=momentum, framing=framing, init=init,
                                   seed=seed, phase=torch.from_numpy(ph).to(eng.device) if init == 'phase' else None, return_phase=True,
                                   return_inconsistency=True)
    torch.cuda.synchronize()
    return wave.cpu().numpy(), phase.cpu().numpy(), inc.cpu().numpy()


def spec_err(mag, a, b):
    """max over frames of max_k |mag (a - b)| / max_k mag"""
    return float((np.abs(mag * (a.astype(np.complex128) - b.astype(np.complex128))).max(axis=1) / mag.max(axis=1)).max())


def check(eng, framing, T, n_iter, momentum, tag):
    mag, ang = inputs(framing, T)
    r64, r32 = refs(framing, T, n_iter, momentum)
    wave, phase, inc = run(eng, [(mag, ang)], framing, n_iter, momentum)
    n = G.samples(T, framing)
    assert wave.shape == (1, G.samples(T + 1, framing)) and not wave[0, n:].any()
    peak = float(np.abs(r64['wave']).max())
    bound_w = max(8.0 * float(np.abs(r32['wave'].astype(np.float64) - r64['wave']).max()), 1e-6 * peak)
    err_w = float(np.abs(wave[0, :n].astype(np.float64) - r64['wave']).max())
    bound_s = max(8.0 * spec_err(mag.astype(np.float64), r32['angles'], r64['angles']), 1e-6)
    err_s = spec_err(mag.astype(np.float64), phase[0, :T], r64['angles'])
    print(f'{tag} {framing} T={T} n_iter={n_iter} momentum={momentum}: wave err {err_w:.2e} (bound {bound_w:.2e}, peak {peak:.2f}), '
          f'mag*angles err {err_s:.2e} (bound {bound_s:.2e}), inconsistency {inc[0]:.6f} (ref {r64["inconsistency"]:.6f})')
    assert np.isfinite(wave).all()
    assert err_w <= bound_w and err_s <= bound_s
    assert np.isnan(phase[0, T:]).all()                             # nothing is written behind the row's frames
    if n_iter == 0:
        assert np.isnan(inc[0])
    elif n_iter <= 2:
        assert abs(inc[0] - r64['inconsistency']) <= 1e-4 * r64['inconsistency']


@pytest.mark.parametrize('framing,T', CASES)
def test_one_and_two_iterations_from_given_phases(eng, framing, T):
    for n_iter in (1, 2):
        for momentum in (0.0, 0.99):
            check(eng, framing, T, n_iter, momentum, 'tight')


@pytest.mark.parametrize('framing,T', CASES)
def test_zero_iterations_is_the_istft(eng, framing, T):
    check(eng, framing, T, 0, 0.99, 'istft')


@pytest.mark.parametrize('framing', ['same', 'center'])
@pytest.mark.parametrize('T', [33, 120])
def test_thirty_two_iterations_with_momentum(eng, framing, T):
    check(eng, framing, T, 32, 0.99, 'long')


@pytest.mark.parametrize('framing', ['same', 'center'])
def test_below_the_minimum_is_refused_by_name(eng, framing):
    from ttsamd.lib import TtsAmdError
    need = G.MIN_FRAMES[framing]
    mag = torch.ones(1, 513, need - 1, device=eng.device)
    with pytest.raises(TtsAmdError, match=f'at least {need}'):
        eng.forward(mag, None, n_iter=1, framing=framing, init='zeros')
    with pytest.raises(TtsAmdError, match=f'at least {need}'):       # a row of a longer matrix, counts on the host
        eng.forward(torch.ones(2, 513, 8, device=eng.device), [8, need - 1], n_iter=1, framing=framing, init='zeros')
    # the library's own refusal (t_max below the minimum), past the Python checks
    import ctypes as C
    from ttsamd import lib as L
    lib = L.load()
    fr = torch.tensor([need - 1], dtype=torch.int32, device=eng.device)
    wave = torch.empty(1, 2048, device=eng.device)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=eng.device)
    rc = lib.ttsamd_griffinlim(C.c_void_p(mag.data_ptr()), C.c_void_p(fr.data_ptr()), 1, need - 1, int(framing == 'center'), 1, 0.99, 0, None, 0,
                               None, C.c_void_p(wave.data_ptr()), 2048, None, C.c_void_p(ws.data_ptr()), 1 << 20, None)
    assert rc != 0 and f'at least {need}' in lib.ttsamd_last_error().decode()
    # counts on the device cannot be refused: such a row is an empty row
    w, _, inc = run(eng, [(inputs(framing, 8)[0], None), (inputs(framing, 8)[0][:need - 1], None)], framing, 1, 0.0, init='zeros',
                    frames_on_device=True)
    assert not w[1].any() and np.isnan(inc[1]) and np.isfinite(w[0]).all() and w[0].any()


@pytest.mark.parametrize('framing', ['same', 'center'])
def test_silence_stays_silent(eng, framing):
    """a stretch of exact zeros: rebuilt is exactly 0 there and a / (|a| + 1e-16) must be 0, not 0 / 0"""
    T = 32
    x = G.test_signal(G.samples(T, framing), seed=2)
    x[256 * 8:256 * 24] = 0.0
    mag = np.abs(G.stft(x, framing)).astype(np.float32)
    ang = G.hash_phase(T, seed=11).astype(np.complex64)
    r64 = G.griffinlim(mag, 2, 0.99, framing, init=2, phase=ang)
    r32 = G.griffinlim(mag, 2, 0.99, framing, init=2, phase=ang, dtype=np.float32)
    wave, _, inc = run(eng, [(mag, ang)], framing, 2, 0.99)
    n = G.samples(T, framing)
    bound = max(8.0 * float(np.abs(r32['wave'].astype(np.float64) - r64['wave']).max()), 1e-6 * float(np.abs(r64['wave']).max()))
    assert np.isfinite(wave).all() and float(np.abs(wave[0, :n] - r64['wave']).max()) <= bound
    assert abs(inc[0] - r64['inconsistency']) <= 1e-4 * r64['inconsistency']


def test_hash_init(eng):
    T = 33
    mag, _ = inputs('same', T)
    w0, p0, _ = run(eng, [(mag, None)], 'same', 0, 0.99, init='hash', seed=0x1234567890ABCDEF)
    ref = G.hash_phase(T, seed=0x1234567890ABCDEF)
    assert float(np.abs(p0[0, :T] - ref).max()) <= 1e-6
    w1, p1, _ = run(eng, [(mag, None)], 'same', 0, 0.99, init='hash', seed=0x1234567890ABCDEE)
    w2, p2, _ = run(eng, [(mag, None)], 'same', 0, 0.99, init='hash', seed=0x0234567890ABCDEF)   # the high word counts too
    assert float(np.abs(p1[0, :T] - p0[0, :T]).max()) > 0.5 and float(np.abs(p2[0, :T] - p0[0, :T]).max()) > 0.5
    assert not np.array_equal(w1, w0) and not np.array_equal(w2, w0)
    w3, p3, _ = run(eng, [(mag, None)], 'same', 0, 0.99, init='hash', seed=0x1234567890ABCDEF)
    assert np.array_equal(w3.view(np.int32), w0.view(np.int32)) and np.array_equal(p3[0, :T].view(np.int32), p0[0, :T].view(np.int32))
    # the wave of the hash init is the restatement's
    r64 = G.griffinlim(mag, 0, 0.99, 'same', init=1, seed=0x1234567890ABCDEF)['wave']
    r32 = G.griffinlim(mag, 0, 0.99, 'same', init=1, seed=0x1234567890ABCDEF, dtype=np.float32)['wave']
    bound = max(8.0 * float(np.abs(r32.astype(np.float64) - r64).max()), 1e-6 * float(np.abs(r64).max()))
    assert float(np.abs(w0[0, :256 * T] - r64).max()) <= bound
    # per-row seeds: a row's audio depends on neither its batch nor its position
    wb, _, _ = run(eng, [(mag, None), (mag, None)], 'same', 3, 0.99, init='hash', seed=[7, 0x1234567890ABCDEF])
    wa, _, _ = run(eng, [(mag, None)], 'same', 3, 0.99, init='hash', seed=0x1234567890ABCDEF)
    assert np.array_equal(wb[1].view(np.int32), wa[0].view(np.int32)) and not np.array_equal(wb[0], wb[1])


@pytest.mark.parametrize('framing', ['same', 'center'])
@pytest.mark.parametrize('momentum', [0.0, 0.99])
def test_ragged_batch_rows_equal_rows_alone(eng, framing, momentum):
    Ts = (33, G.MIN_FRAMES[framing], 16, 5, 40)
    rows = [inputs(framing, T, seed=b) for b, T in enumerate(Ts)]
    t_max = 48
    wave, phase, inc = run(eng, rows, framing, 3, momentum, t_max=t_max)
    wave2, phase2, inc2 = run(eng, rows, framing, 3, momentum, t_max=t_max)
    assert np.array_equal(wave.view(np.int32), wave2.view(np.int32)) and np.array_equal(inc.view(np.int64), inc2.view(np.int64))
    assert np.array_equal(phase.view(np.int32), phase2.view(np.int32))
    for b, T in enumerate(Ts):
        n = G.samples(T, framing)
        w1, p1, i1 = run(eng, [rows[b]], framing, 3, momentum, t_max=T)
        assert np.array_equal(wave[b, :n].view(np.int32), w1[0].view(np.int32)), (b, T)
        assert np.array_equal(phase[b, :T].view(np.int32), p1[0].view(np.int32)) and inc[b] == i1[0]
        assert not wave[b, n:].any() and np.isfinite(wave[b]).all() and np.isfinite(inc[b])


@pytest.mark.parametrize('framing', ['same', 'center'])
def test_resume_through_phase(eng, framing):
    T = 17
    mag, ang = inputs(framing, T)
    w2, p2, _ = run(eng, [(mag, ang)], framing, 2, 0.0)
    _, p1, _ = run(eng, [(mag, ang)], framing, 1, 0.0)
    w11, p11, _ = run(eng, [(mag, p1[0, :T])], framing, 1, 0.0)
    assert np.array_equal(w11.view(np.int32), w2.view(np.int32)) and np.array_equal(p11[0, :T].view(np.int32), p2[0, :T].view(np.int32))


# ---- mel inversion ----
@pytest.mark.parametrize('name', ['audio', 'v24k'])
def test_mel_to_linear(eng, name):
    fb = MR.fbank(name)                                             # 80 and 100 bands
    n_mels = fb.shape[0]
    Ts = (70, 1, 64, 33)
    t_max = 72
    rng = np.random.default_rng(5)
    mel = np.full((len(Ts), n_mels, t_max), np.nan, dtype=np.float32)
    for b, T in enumerate(Ts):
        x = G.test_signal(256 * max(T, 2), seed=b)
        lin = fb.astype(np.float64) @ np.abs(G.stft(x, 'same')).T[:, :T]
        mel[b, :, :T] = np.log(np.maximum(lin, 1e-5)) + 0.05 * rng.standard_normal((n_mels, T))
    mel[0, :, 3] = -30.0                                            # a frame the floor decides
    out = eng.mel_to_linear(torch.from_numpy(mel).to(eng.device), list(Ts), log=True, fbank=fb).cpu().numpy()
    P = G.pinv_filterbank(fb)
    for b, T in enumerate(Ts):
        ref, scale = G.mel_to_linear(mel[b, :, :T], P)
        # 80-100 fp32 products and sums: about 100 x 2^-24; + the fp32 rounding of the floor itself (1e-10 x 2^-24 < 1e-17)
        assert np.all(np.abs(out[b, :, :T] - ref) <= 1e-5 * scale + 1e-17), (name, b)
        assert out[b, :, :T].min() >= np.float32(1e-10) and not out[b, :, T:].any()
        alone = eng.mel_to_linear(torch.from_numpy(np.ascontiguousarray(mel[b:b + 1, :, :T])).to(eng.device), None, log=True, fbank=fb).cpu().numpy()
        assert np.array_equal(alone[0].view(np.int32), out[b, :, :T].view(np.int32))
    assert np.all(out[0, :, 3] == np.float32(1e-10))
    lin_in = np.exp(mel[:1, :, :Ts[0]].astype(np.float64)).astype(np.float32)
    got = eng.mel_to_linear(torch.from_numpy(lin_in).to(eng.device), None, log=False, fbank=fb).cpu().numpy()
    ref, scale = G.mel_to_linear(lin_in[0], P, log=False)
    assert np.all(np.abs(got[0] - ref) <= 1e-5 * scale + 1e-17)


# ---- wrappers ----
def test_griffinlim_module_is_the_engine(eng):
    from utils.audio import GriffinLim, griffinlim
    T = 19
    for framing in ('center', 'same'):
        mag = torch.from_numpy(np.stack([inputs(framing, T, s)[0].T for s in (0, 1)])).to(eng.device)
        want = eng.forward(mag, None, n_iter=4, momentum=0.99, framing=framing, init='hash', seed=5)
        got = GriffinLim(n_iter=4, power=1.0, framing=framing, seed=5).to(eng.device)(mag)
        assert got.shape == (2, G.samples(T, framing)) and torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(griffinlim(mag[0], n_iter=4, power=1, framing=framing, seed=5), want[0])       # [..., 513, T] -> [..., n]
        zero = GriffinLim(n_iter=4, power=1.0, framing=framing, rand_init=False)(mag)
        assert torch.equal(zero, eng.forward(mag, None, n_iter=4, momentum=0.99, framing=framing, init='zeros'))
        # power = 2 on the squared input: the root gives the magnitudes back to an ulp or two (1.2e-7), which two iterations amplify
        # no more than they amplify the fp32 noise (a factor below 10 in the cases above): 1e-5 of the peak leaves a decade
        sq = GriffinLim(n_iter=2, power=2.0, framing=framing, seed=5)(mag * mag)
        lin = GriffinLim(n_iter=2, power=1.0, framing=framing, seed=5)(mag)
        assert float((sq - lin).abs().max()) <= 1e-5 * float(lin.abs().max())
        # ragged: lens in samples
        lens = [G.samples(T, framing), G.samples(T - 4, framing)]
        rag = GriffinLim(n_iter=2, power=1.0, framing=framing, seed=5)(mag, lens=lens)
        assert not bool(rag[1, lens[1]:].any())
        assert torch.equal(rag[1, :lens[1]], griffinlim(mag[1, :, :T - 4].contiguous(), n_iter=2, power=1, framing=framing, seed=5))


def test_refused_arguments_are_named(eng):
    from ttsamd.lib import TtsAmdError
    from utils.audio import GriffinLim, griffinlim
    mag = torch.ones(513, 8, device=eng.device)
    for kw, name in ((dict(n_fft=512), 'n_fft'), (dict(hop_length=128), 'hop_length'), (dict(win_length=512), 'win_length')):
        with pytest.raises(TtsAmdError, match=name):
            GriffinLim(**kw)
        with pytest.raises(TtsAmdError, match=name):
            griffinlim(mag, **kw)
    with pytest.raises(TtsAmdError, match='window'):
        griffinlim(mag, window=torch.hamming_window(1024))
    with pytest.raises(TtsAmdError, match='window'):
        griffinlim(mag, window=torch.hann_window(1024, periodic=False))
    with pytest.raises(TtsAmdError, match='length'):
        GriffinLim(length=1000)(mag)
    with pytest.raises(TtsAmdError, match='power'):
        griffinlim(mag, power=0.0)
    with pytest.raises(TtsAmdError, match='framing'):
        griffinlim(mag, framing='valid')
    with pytest.raises(TtsAmdError, match='momentum'):
        eng.forward(mag[None], None, momentum=1.0)
    with pytest.raises(TtsAmdError, match='513'):
        griffinlim(torch.ones(257, 8, device=eng.device))
    assert GriffinLim(length=256 * 7, n_iter=1, power=1.0)(mag).shape == (256 * 7,)      # the framing's own n is accepted
    assert griffinlim(mag, window=torch.hann_window(1024), n_iter=1, power=1).shape == (256 * 7,)


def test_vocoder_copy_synthesis(dev):
    from utils.objective import copy_synthesis
    from vocoder import load_griffinlim
    from vocoder.griffinlim import GriffinLimVocoder
    wave = torch.from_numpy(G.test_signal(256 * 60, seed=3)).to(dev)
    s8, out8 = copy_synthesis(GriffinLimVocoder(n_iter=8).to(dev), wave, mr_stft=True)
    s0, out0 = copy_synthesis(load_griffinlim(n_iter=0).to(dev), wave, mr_stft=True)
    assert out8.shape == out0.shape == (256 * 60,)
    for k, v in s8.items():
        assert np.isfinite(np.asarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else v, dtype=np.float64)).all(), k
    print('spectral convergence: n_iter 8', float(s8['spectral_convergence']), 'n_iter 0', float(s0['spectral_convergence']))
    assert float(s8['spectral_convergence']) < float(s0['spectral_convergence'])
    voc = GriffinLimVocoder(n_iter=2).to(dev)
    mel = torch.randn(2, 80, 12, device=dev) - 4.0
    assert voc(mel).shape == (2, 1, 256 * 12) and voc(mel[0]).shape == (1, 256 * 12)        # Generator.forward's shapes
    assert torch.equal(voc(mel[0])[0], voc(mel)[0, 0])
    with pytest.raises(ValueError):
        voc.stream(mel[0])


def test_fastpitch2wave_without_a_vocoder_checkpoint(tmp_path, synth_weights, dev):
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    from vocoder.griffinlim import GriffinLimVocoder
    from vocoder.hifigan.models import Generator
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['fastpitch'].items()}, 'config': dict(NET_CONFIG),
                'symbols': list(text.symbols)}, tmp_path / 'fp.pth')
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        every = json.load(f)
    lines = [every[68], every[14]]
    model = FastPitch2Wave(str(tmp_path / 'fp.pth'), vocoder='griffin_lim').to(dev)          # no vocoder checkpoint exists anywhere
    assert isinstance(model.vocoder, GriffinLimVocoder)
    waves = model.tts(lines, batch_size=2)
    assert len(waves) == 2
    for w, line in zip(waves, lines):
        one, mel = model.tts(line, return_mel=True)                                          # denoise 0.005 by default: taken as 0
        assert one.device.type == 'cpu' and one.numel() == 256 * mel.shape[-1] and bool(torch.isfinite(one).all()) and bool(one.any())
        assert torch.equal(one, model.vocoder(mel)[0].cpu())
        assert w.numel() > 0 and w.numel() % 256 == 0 and bool(torch.isfinite(w).all()) and bool(w.any())
    pk = model.tts(lines[0], normalize='peak')
    assert abs(float(pk.abs().max()) - 0.99) < 1e-6
    assert len(model.tts_requests([{'text': lines[0]}, {'text': lines[1], 'denoise': 0.1}])) == 2
    with pytest.raises(ValueError, match='griffin_lim'):
        next(iter(model.tts_stream(lines[0])))
    with pytest.raises(ValueError, match='vocoder'):
        FastPitch2Wave(str(tmp_path / 'fp.pth'), vocoder='wavenet')
    # without the keyword: the HiFi-GAN checkpoint, as before
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, tmp_path / 'hg.pth')
    with open(tmp_path / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    plain = FastPitch2Wave(str(tmp_path / 'fp.pth'), vocoder_sd=str(tmp_path / 'hg.pth'), vocoder_config=str(tmp_path / 'config.json')).to(dev)
    assert isinstance(plain.vocoder, Generator)
    hw, hmel = plain.tts(lines[0], denoise=0, return_mel=True)
    assert torch.equal(hw, plain.vocoder(hmel)[0].cpu())


def test_tacotron2wave_without_a_vocoder_checkpoint(taco_ckpt, dev):
    import text
    from models.tacotron2 import Tacotron2Wave
    from vocoder.griffinlim import GriffinLimVocoder
    taco = Tacotron2Wave(taco_ckpt[0], n_symbol=len(text.symbols), vocoder='griffin_lim').to(dev)      # the vocoder files are not passed
    assert isinstance(taco.vocoder, GriffinLimVocoder)
    taco.model.decoder_max_step = 40
    taco.model.dropout_seed = -1                                   # prenet dropout off: two calls give the same mel
    one, mel = taco.tts_single(TACO_LINES[1], denoise=0.005, return_mel=True)
    assert one.numel() == 256 * mel.shape[-1] and bool(torch.isfinite(one).all()) and bool(one.any())
    assert torch.equal(one, taco.vocoder(mel)[0].cpu())
    waves = taco.tts(TACO_LINES[1:3], batch_size=2, normalize='peak')
    assert len(waves) == 2 and all(w.numel() % 256 == 0 and abs(float(w.abs().max()) - 0.99) < 1e-6 for w in waves)
    with pytest.raises(ValueError, match='griffin_lim'):
        next(iter(taco.tts_stream(TACO_LINES[1])))

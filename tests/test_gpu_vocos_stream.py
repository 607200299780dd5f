"""Vocos in the chunked vocoder on the GPU (pytest -m gpu): ttsamd_vocos_halo_frames, ttsamd_vocos_forward_windows (csrc/vocos.hip), the
Vocos side of ttsamd/stream.py and MelVocos.stream, for '22k' ("same" framing) and '24k' ("center": 256 (T - 1) samples).

The yardstick of the streams is the CPU oracle's WHOLE-utterance wave (tts_oracle.vocos_forward / melspec_ref.vocos24_ref, fp32) at the
project's WAVE_TOL, the bound the one-shot MelVocos is held to: the oracle's own window-against-whole difference at these halos is
exactly zero in float64 (test_vocos_stream_cpu.py), so chunking adds nothing to it.  The halo itself is pinned there; here the
plumbing is: seams, utterance edges, ragged windows, per-row denoise, delivery.  The window entry is checked on bits against
ttsamd_vocos_forward_rows.  512-channel Vocos, at most 7 utterances of at most 130 frames, first 8 then chunks of 16: T = 130 has
interior windows with the full halo on both sides, the others cover every clipped-halo case.  The oracle waves are computed once."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import WAVE_TOL

pytestmark = pytest.mark.gpu

EINVAL = -1
TS = [2, 3, 30, 59, 60, 75, 130]
STRENGTHS = [0.0, 0.0, 0.3, 0.0, 0.3, 0.3, 0.0]
FIRST, CHUNK = 8, 16
NAMES = ['22k', '24k']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i32(vals):
    return (C.c_int32 * len(vals))(*vals)


def _mel(n_mels, T, seed):
    return (np.random.default_rng(seed).standard_normal((n_mels, T)) * 1.5 - 4.0).astype(np.float32)


def _config(name):
    from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG
    return {'22k': VOCOS_22K_CONFIG, '24k': VOCOS_24K_CONFIG}[name]


@pytest.fixture(scope='module')
def vocs(dev):
    """{name: MelVocos with the synthetic weights, on the GPU}"""
    from ttsamd import synth
    from vocoder.vocos import MelVocos
    out = {}
    for name in NAMES:
        voc = MelVocos(name)
        voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.vocos_state_dict(_config(name)).items()})
        out[name] = voc.to(dev)
    return out


@pytest.fixture(scope='module')
def oracle():
    """{name: {T: (mel [n_mels, T] float32, the oracle's whole-utterance wave at the utterance's strength of STRENGTHS)}}"""
    import melspec_ref as R
    import tts_oracle as O
    from ttsamd import synth
    out = {}
    for name in NAMES:
        cfg = _config(name)
        w = synth.vocos_state_dict(cfg)
        bias = O.vocos_bias_vec(w, cfg)
        fwd = O.vocos_forward if name == '22k' else R.vocos24_ref
        out[name] = {}
        for T, s in zip(TS, STRENGTHS):
            mel = _mel(cfg['input_channels'], T, 200 + T)
            out[name][T] = (mel, fwd(w, mel[None], cfg, denoise=s, bias_vec=bias)[0])
    return out


def _samples(name, T):
    return 256 * (T - 1) if name == '24k' else 256 * T


def _plan(name, T, extra=0):
    from ttsamd.stream import plan_chunks, plan_chunks_center, vocos_halo_frames
    left, right = vocos_halo_frames(_config(name))
    return (plan_chunks_center if name == '24k' else plan_chunks)(T, FIRST, CHUNK, left + extra, right + extra)


def _sv(voc, **kw):
    from ttsamd.stream import StreamingVocoder
    return StreamingVocoder(voc, **dict(dict(max_streams=8, max_frames=130, chunk_frames=CHUNK, first_chunk_frames=FIRST), **kw))


def _run(sv, mels, strengths=None, late=(), poison=False):
    """Open `mels` (the indices in `late` two steps after the others), step until every utterance has closed ->
    {index: [chunks, copied to the host step by step]}, with the per-utterance protocol (`last` once, in order) checked on the way."""
    if poison:
        sv._pool.fill_(float('nan'))                                               # unused slots and the frames past every T
    strengths = strengths or [0.0] * len(mels)
    sid_of, got, done = {}, {i: [] for i in range(len(mels))}, set()
    for i, m in enumerate(mels):
        if i not in late:
            sid_of[sv.open(torch.from_numpy(m).to(sv.device), strengths[i])] = i
    steps = 0
    while sv.open_streams or (late and steps < 2):
        if steps == 2:
            for i in late:
                sid_of[sv.open(torch.from_numpy(mels[i]).to(sv.device), strengths[i])] = i
        res = sv.step()
        steps += 1
        assert len(res) == len(set(s for s, _, _ in res))
        for sid, chunk, last in res:
            i = sid_of[sid]
            assert i not in done and chunk.device.type == 'cuda' and chunk.dim() == 1
            got[i].append(chunk.cpu())
            if last:
                done.add(i)
        assert steps < 100
    assert done == set(range(len(mels))) and sv.step() == [] and sv.free_slots == sv.max_streams
    return got


# ---- the library entries -----------------------------------------------------------------------------------------------------------------

def test_halo_frames_of_the_handles_equal_the_host_derivation(vocs):
    from ttsamd.stream import vocos_halo_frames
    for name, want in (('22k', (29, 29)), ('24k', (28, 29))):
        eng = vocs[name].engine()
        left, right = C.c_int32(-1), C.c_int32(-1)
        assert eng.lib.ttsamd_vocos_halo_frames(eng.handle, C.byref(left), C.byref(right)) == 0
        assert (left.value, right.value) == vocos_halo_frames(_config(name)) == want
        assert _sv(vocs[name]).halo == want
    assert eng.lib.ttsamd_vocos_halo_frames(None, C.byref(left), C.byref(right)) == EINVAL


@pytest.mark.parametrize('name', NAMES)
def test_forward_windows_has_the_bits_of_forward_rows_and_writes_nothing_else(dev, vocs, name):
    """a ragged batch of 4 windows, rows at denoise 0 and 0.3, the wave pre-filled with NaN: two sets of needed ranges (interior, whole
    window, window ends, one frame), each against ttsamd_vocos_forward_rows on the same batch"""
    eng = vocs[name].engine()
    lib, n_mels = eng.lib, eng.n_mels
    lens_h, w_max = [70, 41, 9, 2], 72
    W = len(lens_h)
    mel = torch.from_numpy(np.stack([_mel(n_mels, w_max, 300 + w) for w in range(W)])).to(dev)
    lens = torch.tensor(lens_h, dtype=torch.int64, device=dev)
    rows = torch.tensor([0.0, 0.3, 0.3, 0.0], dtype=torch.float32, device=dev)
    bias = eng.bias_vec().reshape(-1)
    nb = lib.ttsamd_vocos_workspace_bytes(eng.handle, W, w_max)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    ref = torch.zeros(W, 256 * w_max, device=dev)
    assert lib.ttsamd_vocos_forward_rows(eng.handle, _ptr(mel), _ptr(lens), W, w_max, _ptr(rows), _ptr(bias), _ptr(ref), _ptr(ws), nb,
                                         _stream()) == 0, lib.ttsamd_last_error()
    wave = torch.empty_like(ref)

    def call(start, length, w=W, wm=w_max, dn=rows, bv=bias, need=True):
        return lib.ttsamd_vocos_forward_windows(eng.handle, _ptr(mel), _ptr(lens), w, wm, _i32(start) if need else None, _i32(length), _ptr(dn),
                                                _ptr(bv), _ptr(wave), _ptr(ws), nb, _stream())
    for start, length in (([29, 0, 5, 0], [12, 41, 4, 2]), ([58, 33, 0, 1], [12, 8, 1, 1]), ([0, 40, 8, 0], [1, 1, 1, 1])):
        wave.fill_(float('nan'))
        assert call(start, length) == 0, lib.ttsamd_last_error()
        want = torch.full_like(ref, float('nan'))
        for w in range(W):
            a, b = 256 * start[w], min(256 * (start[w] + length[w]), _samples(name, lens_h[w]))
            want[w, a:b] = ref[w, a:b]
        assert not bool(torch.isnan(ref[0, :_samples(name, 70)]).any())
        assert torch.equal(wave.view(torch.int32), want.view(torch.int32)), (name, start, length)
    # descriptors out of range are refused before a launch: the wave stays as it is
    wave.fill_(float('nan'))
    ok_s, ok_l = [29, 0, 5, 0], [12, 41, 4, 2]
    for s, n in (([-1, 0, 5, 0], ok_l), (ok_s, [12, 0, 4, 2]), (ok_s, [12, 41, 4, -2]), ([61, 0, 5, 0], ok_l), ([72, 0, 5, 0], [1, 41, 4, 2])):
        assert call(s, n) == EINVAL, (s, n)
        assert b'vocos_forward_windows' in lib.ttsamd_last_error()
    assert call(ok_s, ok_l, w=0) == EINVAL and call(ok_s * 17, ok_l * 17, w=65) == EINVAL and call(ok_s, ok_l, wm=0) == EINVAL
    assert call(ok_s, ok_l, need=False) == EINVAL and call(ok_s, ok_l, bv=None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(wave).all())
    assert call(ok_s, ok_l, dn=None, bv=None) == 0                                # NULL denoise_rows: every row at 0, no bias needed
    torch.cuda.synchronize()
    assert torch.equal(wave[0, 256 * 29:256 * 41], ref[0, 256 * 29:256 * 41])     # (row 0 is at strength 0 in `rows` too)


# ---- the scheduler -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def plain_run(vocs, oracle):
    return {name: _run(_sv(vocs[name]), [oracle[name][T][0] for T in TS], strengths=STRENGTHS) for name in NAMES}


def _check_against_the_oracle(name, got, oracle, ts, what, one_shot=None):
    errs, dev_errs = [], []
    for i, T in enumerate(ts):
        wave = torch.cat(got[i])
        assert wave.shape == (_samples(name, T),) and wave.dtype == torch.float32, (name, T)
        assert [c.numel() for c in got[i]] == [256 * c[1] for c in _plan(name, T)], (name, T)      # chunk counts and lengths as planned
        errs.append(float((wave - oracle[name][T][1]).abs().max()))
        if one_shot is not None:
            dev_errs.append(float((wave - one_shot[i]).abs().max()))
    print(f"{what} '{name}', T = {ts}: max-abs against the oracle {['%.2e' % e for e in errs]} (tol {WAVE_TOL})"
          + (f"; against one-shot MelVocos.forward on the device {['%.2e' % e for e in dev_errs]}" if dev_errs else ''))
    assert max(errs) < WAVE_TOL


@pytest.mark.parametrize('name', NAMES)
def test_streams_opened_together_match_the_whole_utterance_oracle(vocs, oracle, plain_run, name):
    """seven utterances of 2 .. 130 frames in one pool, three of them at denoise 0.3: windows that are the whole utterance (2, 3, 30),
    that lose a part of a halo at one or both edges (59, 60, 75) and interior windows with both halos whole (130); '24k': 256 (T - 1)
    samples, no empty chunk"""
    voc = vocs[name]
    one_shot = [voc(torch.from_numpy(oracle[name][T][0]).to(voc.device)[None], denoise=s)[0].cpu() for T, s in zip(TS, STRENGTHS)]
    _check_against_the_oracle(name, plain_run[name], oracle, TS, 'streamed', one_shot)
    assert all(len(plain_run[name][i]) >= 1 and all(c.numel() > 0 for c in plain_run[name][i]) for i in range(len(TS)))
    assert len(plain_run[name][TS.index(130)]) == len(_plan(name, 130)) == 9


@pytest.mark.parametrize('name', NAMES)
def test_a_late_join_into_a_poisoned_pool(vocs, oracle, name):
    """every pool frame NaN before the mels go in (unused slots, the frames past each T), and the 60- and 2-frame utterances joining
    two steps late, into a batch whose other rows are in the middle of theirs"""
    got = _run(_sv(vocs[name]), [oracle[name][T][0] for T in TS], strengths=STRENGTHS, late=(0, 4), poison=True)
    _check_against_the_oracle(name, got, oracle, TS, 'late join, poisoned pool:')


def test_pcm16_chunks_equal_the_float_chunks_converted_on_the_host(vocs, oracle, plain_run):
    from ttsamd.stream import pcm16
    got = _run(_sv(vocs['22k'], encoding='pcm16'), [oracle['22k'][T][0] for T in TS], strengths=STRENGTHS)
    for i in range(len(TS)):
        assert len(got[i]) == len(plain_run['22k'][i])
        for a, b in zip(got[i], plain_run['22k'][i]):
            assert a.dtype == torch.int16 and np.array_equal(a.numpy(), pcm16(b.numpy())), TS[i]


@pytest.mark.parametrize('name,rate,encoding', [('22k', 8000, 'mulaw'), ('24k', 16000, None)])
def test_streams_at_another_rate_are_the_resampled_float_stream_on_bits(vocs, oracle, plain_run, name, rate, encoding):
    """the chunks at another rate (and encoded), put together, against utils.audio.resample (+ encode) of the float stream's samples in
    one piece: the resampler's halo around every core is in the windows and in the needed range of the vocoder call"""
    from ttsamd.stream import chunk_outputs
    from utils.audio import encode, resample
    voc = vocs[name]
    sv = _sv(voc, sample_rate=rate, encoding=encoding)
    assert sv.sample_rate == rate and voc.sampling_rate == {'22k': 22050, '24k': 24000}[name]
    got = _run(sv, [oracle[name][T][0] for T in TS], strengths=STRENGTHS)
    o, n = sv._rs[:2]
    for i, T in enumerate(TS):
        whole = torch.cat(plain_run[name][i]).to(voc.device)
        want = resample(whole[None], voc.sampling_rate, rate)[0]
        if encoding:
            want = encode(want, encoding)
        out = torch.cat(got[i])
        assert [c.numel() for c in got[i]] == [k1 - k0 for k0, k1 in (chunk_outputs(256 * c[0], 256 * (c[0] + c[1]), o, n) for c in _plan(name, T))]
        assert out.dtype == want.dtype and out.numel() == want.numel() == -(-n * _samples(name, T) // o), (name, T)
        if out.dtype == torch.float32:
            assert torch.equal(out.view(torch.int32), want.cpu().view(torch.int32)), (name, T)
        else:
            assert torch.equal(out, want.cpu()), (name, T)


# ---- the drop-in surface and the refusals ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_melvocos_stream_equals_a_one_slot_streaming_vocoder(vocs, oracle, name):
    from ttsamd.stream import StreamingVocoder
    voc = vocs[name]
    mel = torch.from_numpy(oracle[name][75][0]).to(voc.device)
    chunks = [c.cpu() for c in voc.stream(mel, chunk_frames=CHUNK, first_chunk_frames=FIRST, denoise=0.3)]
    direct = _run(StreamingVocoder(voc, max_streams=1, max_frames=75, chunk_frames=CHUNK, first_chunk_frames=FIRST), [oracle[name][75][0]],
                  strengths=[0.3])[0]
    assert len(chunks) == len(direct) == len(_plan(name, 75)) and all(torch.equal(a, b) for a, b in zip(chunks, direct))
    assert float((torch.cat(chunks) - oracle[name][75][1]).abs().max()) < WAVE_TOL                 # (75 is at 0.3 in STRENGTHS)
    assert [c.numel() for c in voc.stream(mel)] == [256 * 32, _samples(name, 75) - 256 * 32]       # the defaults: first 32, then 64


def test_errors(vocs):
    from ttsamd.stream import StreamingVocoder
    dev = vocs['22k'].device
    with pytest.raises(ValueError, match='denoiser'):
        StreamingVocoder(vocs['22k'], denoiser=object(), max_streams=1, max_frames=8)
    sv = _sv(vocs['24k'], max_streams=2, max_frames=40)
    with pytest.raises(ValueError, match='2 frames'):
        sv.open(torch.zeros(100, 1, device=dev))
    with pytest.raises(ValueError, match='max_frames'):
        sv.open(torch.zeros(100, 41, device=dev))
    for bad in (float('nan'), float('inf'), -0.1):
        with pytest.raises(ValueError):
            sv.open(torch.zeros(100, 4, device=dev), denoise=bad)
    with pytest.raises(ValueError):
        sv.open(torch.zeros(80, 4, device=dev))
    assert sv.free_slots == 2                                                         # a refused open takes no slot
    sv.open(torch.zeros(100, 40, device=dev), denoise=5.0)                            # any strength, any length from 2 frames on
    sv.open(torch.zeros(100, 2, device=dev), denoise=0.3)
    with pytest.raises(ValueError, match='slots'):
        sv.open(torch.zeros(100, 4, device=dev))
    sv22 = _sv(vocs['22k'], max_streams=1, max_frames=8)
    sid = sv22.open(torch.zeros(80, 1, device=dev), denoise=0.3)                      # '22k': one frame is an utterance of 256 samples
    (got_sid, chunk, last), = sv22.step()
    assert got_sid == sid and chunk.numel() == 256 and last

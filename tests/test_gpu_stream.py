"""Streaming synthesis on the GPU (pytest -m gpu): csrc/stream.hip, ttsamd/stream.py, Generator.stream and FastPitch2Wave.tts_stream.

The yardstick is the CPU oracle's WHOLE-utterance wave (tts_oracle.hifigan_forward; V3: the float64 restatement of
test_hifigan_v3_cpu) at the project's WAVE_TOL, the bound the one-shot path is held to: the oracle's own window-against-whole
difference at these halos is zero (test_stream_cpu.py), so chunking adds nothing to it.  The copies (gather, emit) are checked bit
for bit against numpy.  The oracle waves are computed once per module."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, WAVE_TOL
from test_hifigan_v3_cpu import generator_f64

pytestmark = pytest.mark.gpu

EINVAL = -1
TS = [1, 2, 3, 13, 14, 40, 70]
STRENGTHS = [0.0, 0.0, 0.01, 0.0, 0.01, 0.01, 0.0]          # per utterance of TS: the bias denoiser on some rows, not on others


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


def _mel(T, seed):
    return (np.random.default_rng(seed).standard_normal((80, T)) * 1.5 - 4.0).astype(np.float32)


@pytest.fixture(scope='module')
def v1(dev, synth_weights):
    from ttsamd.config import HIFIGAN_CONFIG
    from vocoder.hifigan.denoiser import Denoiser
    from vocoder.hifigan.models import Generator
    gen = Generator(dict(HIFIGAN_CONFIG), state_dict={k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}).to(dev)
    return gen, Denoiser(gen)


@pytest.fixture(scope='module')
def oracle_v1(synth_weights):
    """{T: (mel [80, T] float32, the oracle's whole-utterance wave [256 T], the oracle's denoised wave at strength 0.01 or None)}"""
    import tts_oracle as O
    from ttsamd.config import HIFIGAN_CONFIG
    W = O.fold_weight_norm(synth_weights['hifigan'])
    bias = O.denoiser_bias_spec(W, HIFIGAN_CONFIG)
    out = {}
    for T in TS:
        mel = _mel(T, 100 + T)
        wave = O.hifigan_forward(W, torch.from_numpy(mel), HIFIGAN_CONFIG)[0]
        out[T] = (mel, wave, O.denoise(wave[None], bias, 0.01)[0] if 256 * T > 512 else None)
    out['bias'] = bias
    return out


def _run(sv, mels, strengths=None, late=(), poison=False):
    """Open `mels` (a list; the indices in `late` two steps after the others), step until every utterance has closed.
    -> {index: [chunks, copied to the host step by step]}, with the per-utterance protocol checked on the way."""
    if poison:
        sv._pool.fill_(float('nan'))
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
        assert len(res) == len(set(s for s, _, _ in res))                       # one chunk per open utterance and step
        for sid, chunk, last in res:
            i = sid_of[sid]
            assert i not in done and chunk.device.type == 'cuda' and chunk.dim() == 1
            got[i].append(chunk.cpu())
            if last:
                done.add(i)
        assert steps < 200
    assert done == set(range(len(mels))) and sv.step() == [] and sv.free_slots == sv.max_streams
    return got


# ---- the two copies, bit for bit ---------------------------------------------------------------------------------------------------------

def test_gather_windows_out_of_a_poisoned_pool(dev):
    from ttsamd import lib as L
    lib = L.load()
    S, M, t_cap, w_max = 3, 80, 64, 12
    rng = np.random.default_rng(1)
    clean = rng.standard_normal((S, M, t_cap)).astype(np.float32)
    # starts 0, 1 and 63; lengths 1, 7 and w_max; slot 1 and slot 0 twice (overlapping windows on slot 1); a window ending at t_cap
    wins = [(0, 0, 1), (1, 1, 7), (2, 63, 1), (1, 3, 12), (0, 52, 12), (2, 0, 12)]
    pool = np.full_like(clean, np.nan)
    for s, a, n in wins:
        pool[s, :, a:a + n] = clean[s, :, a:a + n]
    assert np.isnan(pool).any()
    W = len(wins)
    batch = torch.full((W, M, w_max), 7.0, device=dev)
    lens = torch.full((W,), -1, dtype=torch.int64, device=dev)
    args = lambda wl, w=W, wm=w_max: (_ptr(pool_d), S, M, t_cap, _i32([x[0] for x in wl]), _i32([x[1] for x in wl]), _i32([x[2] for x in wl]),
                                      w, wm, _ptr(batch), _ptr(lens), _stream())
    pool_d = torch.from_numpy(pool).to(dev)
    assert lib.ttsamd_stream_gather(*args(wins)) == 0
    got = batch.cpu().numpy()
    for w, (s, a, n) in enumerate(wins):
        assert np.array_equal(got[w, :, :n], clean[s, :, a:a + n]), w
        assert not got[w, :, n:].any(), w
    assert lens.cpu().tolist() == [n for _, _, n in wins]
    # descriptors out of range are refused before a launch: the outputs stay as they are
    before = batch.clone()
    for bad in ([(3, 0, 1)], [(-1, 0, 1)], [(0, -1, 1)], [(0, 0, 0)], [(0, 0, w_max + 1)], [(0, 60, 5)], [(0, 64, 1)], [(0, 0, 1), (1, 53, 12)]):
        assert lib.ttsamd_stream_gather(*args(bad, w=len(bad))) == EINVAL, bad
        assert b'stream_gather' in lib.ttsamd_last_error()
    assert lib.ttsamd_stream_gather(*args(wins[:1] * 65, w=65)) == EINVAL
    assert lib.ttsamd_stream_gather(*args(wins, w=0)) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(batch, before)


@pytest.mark.parametrize('fmt', [0, 1])
def test_emit_cores_as_float32_and_pcm16(dev, fmt):
    from ttsamd import lib as L
    from ttsamd.stream import pcm16
    lib = L.load()
    W, w_max, hop, c_max = 4, 5, 256, 768
    rng = np.random.default_rng(2)
    wave = rng.uniform(-1.3, 1.3, (W, hop * w_max)).astype(np.float32)
    wave[1, 256:256 + 12] = [1.0, -1.0, 0.5 / 32767, -0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -2.5 / 32767, 5.0, -5.0, np.nan, 32766.5 / 32767, 0.0]
    off, n = [0, 256, 512, 1024], [256, 768, 0, 256]
    out = torch.full((W, c_max), 77, dtype=torch.int16 if fmt else torch.float32, device=dev)
    wave_d = torch.from_numpy(wave).to(dev)
    call = lambda o=off, m=n, cm=c_max, f=fmt, h=hop: lib.ttsamd_stream_emit(_ptr(wave_d), W, w_max, h, _i32(o), _i32(m), cm, f, _ptr(out), _stream())
    assert call() == 0
    got = out.cpu().numpy()
    for w in range(W):
        ref = np.zeros(c_max, np.float32)
        ref[:n[w]] = wave[w, off[w]:off[w] + n[w]]
        if fmt:
            assert np.array_equal(got[w], pcm16(ref)), w
        else:
            assert np.array_equal(got[w].view(np.uint32), ref.view(np.uint32)), w          # bits: the NaN too
    # offsets and lengths are multiples of the hop and fit the window wave and the chunk row; two formats
    before = out.clone()
    assert call(o=[0, 255, 512, 1024]) == EINVAL and call(m=[256, 760, 0, 256]) == EINVAL and call(o=[-256, 256, 512, 1024]) == EINVAL
    assert call(o=[0, 256, 512, 1280]) == EINVAL                                          # 1280 + 256 > hop * w_max
    assert call(o=[0, 256, 1024, 1024], m=[256, 768, 512, 256]) == EINVAL                 # 1024 + 512 > hop * w_max
    assert call(m=[256, 1024, 0, 256]) == EINVAL                                          # longer than the chunk row
    assert call(f=2) == EINVAL and call(cm=772) == EINVAL and call(h=100) == EINVAL
    assert b'stream_emit' in lib.ttsamd_last_error()
    torch.cuda.synchronize()
    bits = torch.int16 if fmt else torch.int32                                            # bits: the float32 rows hold a NaN
    assert torch.equal(out.view(bits), before.view(bits))


def test_halo_frames_of_the_handles_equal_the_host_derivation(dev, v1, v3):
    from ttsamd.config import HIFIGAN_CONFIG, HIFIGAN_V3_CONFIG
    from ttsamd.stream import StreamingVocoder, hifigan_halo_frames
    lib = v1[0].engine().lib
    for gen, cfg, want in ((v1[0], HIFIGAN_CONFIG, (13, 13)), (v3, HIFIGAN_V3_CONFIG, (11, 11))):
        left, right = C.c_int32(-1), C.c_int32(-1)
        assert lib.ttsamd_hifigan_halo_frames(gen.engine().handle, C.byref(left), C.byref(right)) == 0
        assert (left.value, right.value) == hifigan_halo_frames(cfg) == want
        assert StreamingVocoder(gen, max_streams=1, max_frames=8).halo == want
    assert lib.ttsamd_denoiser_halo_frames() == 3
    assert lib.ttsamd_hifigan_halo_frames(None, C.byref(left), C.byref(right)) == EINVAL


# ---- the scheduler on V1 -----------------------------------------------------------------------------------------------------------------

def _sv(v1, **kw):
    from ttsamd.stream import StreamingVocoder
    return StreamingVocoder(v1[0], v1[1], **dict(dict(max_streams=8, max_frames=96, chunk_frames=8, first_chunk_frames=4), **kw))


@pytest.fixture(scope='module')
def plain_run(v1, oracle_v1):
    return _run(_sv(v1), [oracle_v1[T][0] for T in TS])


def test_streams_opened_together_match_the_whole_utterance_oracle(oracle_v1, plain_run):
    """first 4, chunks of 8, utterances of 1 .. 70 frames in one pool: windows that are the whole utterance (1, 2, 3), that touch both
    edges (13, 14), and runs of middle windows (40, 70); up to seven rows per vocoder call, fewer as the short ones end."""
    from ttsamd.stream import plan_chunks
    errs = []
    for i, T in enumerate(TS):
        wave = torch.cat(plain_run[i])
        assert wave.shape == (256 * T,) and wave.dtype == torch.float32
        assert [c.numel() // 256 for c in plain_run[i]] == [c[1] for c in plan_chunks(T, 4, 8, 13, 13)]
        errs.append(float((wave - oracle_v1[T][1]).abs().max()))
    print(f'streamed V1, T = {TS}: max-abs against the oracle {["%.2e" % e for e in errs]} (tol {WAVE_TOL})')
    assert max(errs) < WAVE_TOL


def test_unused_pool_frames_do_not_matter(v1, oracle_v1, plain_run):
    """The same run on a pool whose every frame was NaN before the mels went in: the same launches on the same shapes, so the chunks are
    bit-identical -- nothing outside an utterance's own frames is read."""
    got = _run(_sv(v1), [oracle_v1[T][0] for T in TS], poison=True)
    for i in range(len(TS)):
        assert len(got[i]) == len(plain_run[i])
        for a, b in zip(got[i], plain_run[i]):
            assert torch.equal(a, b), (TS[i])


def test_denoise_on_some_rows(v1, oracle_v1):
    """Rows with the bias denoiser (their windows carry 3 more frames of halo per side) next to rows without it, the 1- and 2-frame
    utterances the denoiser could not take among them: one ttsamd_denoise_rows per step, which leaves the rows at strength 0 alone."""
    got = _run(_sv(v1), [oracle_v1[T][0] for T in TS], strengths=STRENGTHS)
    errs = []
    for i, (T, s) in enumerate(zip(TS, STRENGTHS)):
        wave = torch.cat(got[i])
        assert wave.shape == (256 * T,)
        ref = oracle_v1[T][2] if s > 0 else oracle_v1[T][1]
        errs.append(float((wave - ref).abs().max()))
    moved = [float((oracle_v1[T][2] - oracle_v1[T][1]).abs().max()) for T, s in zip(TS, STRENGTHS) if s > 0]
    print(f'streamed V1 with denoise {STRENGTHS}: max-abs against the oracle {["%.2e" % e for e in errs]} (tol {WAVE_TOL}); '
          f'the denoiser moves the oracle waves by {["%.2e" % m for m in moved]}')
    assert max(errs) < WAVE_TOL


def test_a_stream_that_joins_two_steps_later(v1, oracle_v1):
    """... into a batch whose other rows are in the middle of their utterances; with a strong denoiser setting (0.3: consecutive frames
    become inconsistent, so every overlap-add term at a window edge matters) on the short and on the late row."""
    import tts_oracle as O
    got = _run(_sv(v1), [oracle_v1[70][0], oracle_v1[14][0], oracle_v1[40][0]], strengths=[0.0, 0.3, 0.3], late=(2,))
    refs = [oracle_v1[70][1]] + [O.denoise(oracle_v1[T][1][None], oracle_v1['bias'], 0.3)[0] for T in (14, 40)]
    print(f'late join: denoise 0.3 moves the oracle waves by {["%.2e" % float((refs[i] - oracle_v1[T][1]).abs().max()) for i, T in ((1, 14), (2, 40))]}')
    errs = [float((torch.cat(got[i]) - refs[i]).abs().max()) for i in range(3)]
    print(f'late join: max-abs against the oracle {["%.2e" % e for e in errs]} (tol {WAVE_TOL})')
    assert [torch.cat(got[i]).numel() for i in range(3)] == [256 * 70, 256 * 14, 256 * 40] and max(errs) < WAVE_TOL


def test_pcm16_chunks_equal_the_float_chunks_converted_on_the_host(v1, oracle_v1, plain_run):
    from ttsamd.stream import pcm16
    got = _run(_sv(v1, pcm16=True), [oracle_v1[T][0] for T in TS])
    for i in range(len(TS)):
        a = torch.cat(got[i])
        assert a.dtype == torch.int16 and np.array_equal(a.numpy(), pcm16(torch.cat(plain_run[i]).numpy())), TS[i]


def test_generator_stream(v1, oracle_v1):
    gen = v1[0]
    mel = torch.from_numpy(oracle_v1[70][0]).to(gen.device)
    chunks = [c.cpu() for c in gen.stream(mel)]                                       # the defaults: first 32, then 64 -> 32 + 38
    assert [c.numel() for c in chunks] == [256 * 32, 256 * 38]
    assert float((torch.cat(chunks) - oracle_v1[70][1]).abs().max()) < WAVE_TOL
    den = torch.cat([c.cpu() for c in gen.stream(mel, chunk_frames=16, first_chunk_frames=8, denoiser=v1[1], denoise=0.01)])
    assert float((den - oracle_v1[70][2]).abs().max()) < WAVE_TOL


def test_errors(v1, oracle_v1):
    sv = _sv(v1, max_streams=2, max_frames=40)
    dev = sv.device
    with pytest.raises(ValueError, match='max_frames'):
        sv.open(torch.zeros(80, 41, device=dev))
    with pytest.raises(ValueError, match='512 samples'):
        sv.open(torch.zeros(80, 2, device=dev), denoise=0.01)
    with pytest.raises(ValueError):
        sv.open(torch.zeros(80, 0, device=dev))
    with pytest.raises(ValueError):
        sv.open(torch.zeros(79, 4, device=dev))
    with pytest.raises(ValueError):
        sv.open(torch.zeros(80, 4, device=dev), denoise=float('nan'))
    assert sv.free_slots == 2                                                         # a refused open takes no slot
    a = sv.open(torch.zeros(80, 40, device=dev))
    sv.open(torch.zeros(80, 2, device=dev))
    with pytest.raises(ValueError, match='slots'):
        sv.open(torch.zeros(80, 4, device=dev))
    sv.close(a)
    assert sv.free_slots == 1
    with pytest.raises(KeyError):
        sv.close(a)
    from ttsamd.stream import StreamingVocoder
    with pytest.raises(ValueError, match='denoiser'):
        StreamingVocoder(v1[0], max_streams=1, max_frames=8).open(torch.zeros(80, 4, device=dev), denoise=0.01)


# ---- V3 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def v3(dev):
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_V3_CONFIG
    from vocoder.hifigan.models import Generator
    sd = synth.hifigan_state_dict(HIFIGAN_V3_CONFIG, seed=0)
    gen = Generator(dict(HIFIGAN_V3_CONFIG), state_dict={k: torch.from_numpy(v.copy()) for k, v in sd.items()}).to(dev)
    gen._test_sd = sd
    return gen


def test_v3_generator_streams(v3):
    from ttsamd.config import HIFIGAN_V3_CONFIG
    from ttsamd.stream import StreamingVocoder
    mel = _mel(40, 9)
    ref = torch.from_numpy(generator_f64(v3._test_sd, HIFIGAN_V3_CONFIG, mel))
    got = _run(StreamingVocoder(v3, max_streams=2, max_frames=40, chunk_frames=8, first_chunk_frames=4), [mel])
    wave = torch.cat(got[0])
    err = float((wave.double() - ref).abs().max())
    print(f'streamed V3, T = 40: max-abs against the float64 restatement {err:.2e} (tol {WAVE_TOL})')
    assert wave.shape == (256 * 40,) and len(got[0]) == 6 and err < WAVE_TOL


# ---- the drop-in surface -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def model4(tmp_path_factory, synth_weights, dev):
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    cfg4 = dict(NET_CONFIG, n_speakers=4)
    d = tmp_path_factory.mktemp('ckpt_stream')
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['fastpitch_spk4'].items()}, 'config': cfg4,
                'symbols': list(text.symbols)}, d / 'fp4.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    return FastPitch2Wave(str(d / 'fp4.pth'), vocoder_sd=str(d / 'hg.pth'), vocoder_config=str(d / 'config.json')).to(dev)


@pytest.fixture(scope='module')
def lines5():
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        lines = json.load(f)
    return [lines[i] for i in (68, 14, 92, 63, 35)]                                   # five of the shortest committed lines, unsorted


@pytest.mark.parametrize('denoise', [0.0, 0.005])
def test_tts_stream_of_one_line_equals_tts_single(model4, lines5, denoise):
    ref = model4.tts_single(lines5[0], denoise=denoise, speaker_id=1)
    chunks = list(model4.tts_stream(lines5[0], chunk_frames=16, first_chunk_frames=8, denoise=denoise, speaker_id=1))
    assert len(chunks) > 3 and all(c.device.type == 'cpu' and c.dtype == torch.float32 for c in chunks)
    assert chunks[0].numel() == 256 * 8 and chunks[1].numel() == 256 * 16
    wave = torch.cat(chunks)
    assert wave.shape == ref.shape and ref.numel() % 256 == 0
    err = float((wave - ref).abs().max())
    print(f'tts_stream(str, denoise={denoise}): {len(chunks)} chunks, max-abs against tts_single {err:.2e} (tol {WAVE_TOL})')
    assert err < WAVE_TOL


def test_tts_stream_of_a_list_is_continuous_batching(model4, lines5):
    """Five lines with their own speed and denoise strength through two slots: a line's chunks arrive in order with `last` once, at most
    two lines are open at any time, a new line joins when one ends, and every line's audio is tts_single's with its options."""
    from ttsamd.stream import pcm16
    speed, denoise = [0.8, 1.0, 1.25, 1.0, 2.0], [0.005, 0.0, 0.1, 0.0, 0.02]
    kw = dict(chunk_frames=16, first_chunk_frames=8, max_streams=2, speed=speed, denoise=denoise, speaker_id=2)
    got, finished, open_now, most_open, first_seen = {i: [] for i in range(5)}, [], set(), 0, []
    for i, chunk, last in model4.tts_stream(lines5, **kw):
        assert i not in finished and chunk.device.type == 'cpu'
        if i not in open_now:
            first_seen.append(i)
        open_now.add(i)
        most_open = max(most_open, len(open_now))
        got[i].append(chunk)
        if last:
            finished.append(i)
            open_now.discard(i)
    assert sorted(finished) == [0, 1, 2, 3, 4] and first_seen == [0, 1, 2, 3, 4] and most_open == 2 and not open_now
    errs = []
    for i, line in enumerate(lines5):
        ref = model4.tts_single(line, speed=speed[i], denoise=denoise[i], speaker_id=2)
        wave = torch.cat(got[i])
        assert wave.shape == ref.shape, (i, wave.shape, ref.shape)
        errs.append(float((wave - ref).abs().max()))
    print(f'tts_stream(list of 5, two slots): max-abs against tts_single per line {["%.2e" % e for e in errs]} (tol {WAVE_TOL})')
    assert max(errs) < WAVE_TOL
    # pcm16: the same steps on the same shapes, converted on the device
    pcm = {i: [] for i in range(5)}
    for i, chunk, _ in model4.tts_stream(lines5, pcm16=True, **kw):
        assert chunk.dtype == torch.int16
        pcm[i].append(chunk)
    for i in range(5):
        assert np.array_equal(torch.cat(pcm[i]).numpy(), pcm16(torch.cat(got[i]).numpy())), i

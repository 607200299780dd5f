"""GPU: Tacotron2 as a stream -- the resumable decoder (ttsamd_tacotron2_stream_*), the postnet over windows, a vocoder stream that
grows (StreamingVocoder.open_growing / append / finish) and Tacotron2Wave.tts_stream -- against the one-shot calls of the same engine
(bit for bit where the launches are the same) and the oracles the one-shot tests use, at their tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import WAVE_TOL
from recurrent_ref import _gate_for_stops
from test_gpu_stream import _mel, oracle_v1, v1  # noqa: F401  (fixtures)
from test_gpu_tacotron2 import ALIGN_TOL, LINES, MEL_TOL, _tokens, _weights, dev, maxabs, taco_ckpt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EINVAL = -1
STOPS = [12, 27, 5, 21]


@functools.lru_cache(None)
def _stop_case():
    """B = 4, L = 19, max_step = 40, a gate layer fitted (at dropout seed 4) so that the rows stop at 12 / 27 / 5 / 21"""
    cfg, sd = _weights(gate_bias=-20.0)
    tok, lens = _tokens(4, 19, 9)
    sids = torch.tensor([0, 3, 7, 39])
    return cfg, _gate_for_stops(cfg, sd, tok, sids, lens, STOPS, max_step=40, seed=4), tok, lens, sids


@functools.lru_cache(None)
def _stop_oracle(seed):
    import taco_oracle as T
    cfg, sd, tok, lens, sids = _stop_case()
    return T.tacotron2_infer(sd, cfg, tok, sids, lens, max_step=40, seed=seed)


@pytest.fixture(scope='module')
def stop_eng(dev):
    from ttsamd.engine import Tacotron2Engine
    cfg, sd, *_ = _stop_case()
    return Tacotron2Engine(sd, cfg, device=dev)


def _drive(sess, schedule):
    """advance by the schedule's entries, then by its last one, until the session has ended -> steps_done after each advance"""
    trace, k = [], 0
    while not sess.ended:
        done, _ = sess.advance(schedule[min(k, len(schedule) - 1)])
        trace.append(done)
        k += 1
        assert k < 100
    return trace


# ---- 1. the decoder, bit for bit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('schedule', [(8,), (16, 8, 8)])
@pytest.mark.parametrize('mode', ['0', '1', '2'])
@pytest.mark.parametrize('seed', [4, -1])
def test_session_frames_are_infers_bit_for_bit(stop_eng, ttsopt, seed, mode, schedule):
    """Rows stop at 12 / 27 / 5 / 21 of 40: a session driven in advances of 8 (and 16, 8, 8) under TTSAMD_TACO_PERSISTENT = 0 / 1 / 2 leaves
    the raw frames, alignments and lengths of infer() under the same option, bit for bit; at the seed the gate was fitted for it ends at
    27 after the advance that reaches 32 -- the fourth of 8 -- and refuses a further one.  Alignments and lengths against the oracle."""
    cfg, sd, tok, lens, sids = _stop_case()
    ttsopt.set('TTSAMD_TACO_PERSISTENT', mode)
    mel, mel_lens, al, raw = stop_eng.infer(tok, sids, lens, max_step=40, dropout_seed=seed, return_raw=True)
    sess = stop_eng.stream(tok, sids, lens, max_step=40, dropout_seed=seed, max_chunk_steps=16)
    assert sess.steps_done == 0 and not sess.ended
    trace = _drive(sess, schedule)
    assert sess.steps_done == raw.shape[2] and trace[:-1] == np.cumsum([schedule[min(k, len(schedule) - 1)] for k in range(len(trace) - 1)]).tolist()
    assert torch.equal(sess.mel_raw, raw) and torch.equal(sess.alignments, al) and torch.equal(sess.mel_lens, mel_lens)
    with pytest.raises(ValueError):
        sess.advance(8)
    _, lens_ref, al_ref = _stop_oracle(seed)
    assert mel_lens.cpu().tolist() == np.asarray(lens_ref).tolist() and maxabs(sess.alignments, al_ref) < ALIGN_TOL
    if seed == 4:
        assert mel_lens.cpu().tolist() == STOPS and sess.steps_done == 27
        assert sess.n_advances == (4 if schedule == (8,) else 3)
        # the rows' report at the end: every row ended at its own length, everything final
        assert [r[1] for r in sess.rows] == [1] * 4 and [r[3] for r in sess.rows] == STOPS and [r[0] for r in sess.rows] == STOPS
    sess.close()


@pytest.mark.parametrize('mode', ['0', '2'])
def test_session_without_early_stopping_runs_to_max_step(dev, ttsopt, mode):
    """decoder_early_stopping=False, max_step = 24: every gate has fired by step 11, the session still ends at 24, after three advances"""
    from ttsamd.engine import Tacotron2Engine
    cfg, sd = _weights(gate_bias=-20.0)
    tok, lens = _tokens(3, 15, 21)
    sids = torch.tensor([1, 5, 9])
    stops = [6, 11, 4]
    sd = _gate_for_stops(cfg, sd, tok, sids, lens, stops, max_step=24, seed=3)
    eng = Tacotron2Engine(sd, dict(cfg, decoder_early_stopping=False), device=dev)
    ttsopt.set('TTSAMD_TACO_PERSISTENT', mode)
    mel, mel_lens, al, raw = eng.infer(tok, sids, lens, max_step=24, dropout_seed=3, return_raw=True)
    sess = eng.stream(tok, sids, lens, max_step=24, dropout_seed=3, max_chunk_steps=8)
    assert _drive(sess, (8,)) == [8, 16, 24] and raw.shape[2] == 24
    assert sess.mel_lens.cpu().tolist() == stops == mel_lens.cpu().tolist()
    assert torch.equal(sess.mel_raw, raw) and torch.equal(sess.alignments, al)
    # rows end at their own lengths although the batch runs on; a row is reported ended once its count stands still
    assert [r[3] for r in sess.rows] == stops and [r[1] for r in sess.rows] == [1, 1, 1]


@pytest.mark.parametrize('B,L,max_step', [(9, 12, 16), (1, 1, 12)])
def test_session_on_the_graph_path_only_batch_and_on_one_token(dev, B, L, max_step):
    """B = 9 does not fit the persistent decoder (graph path by the fits rule); B = 1, L = 1 is its smallest geometry, with a max_step
    that is no multiple of 8 (the last advance is clipped)"""
    from ttsamd.engine import Tacotron2Engine
    cfg, sd = _weights(gate_bias=-20.0)
    eng = Tacotron2Engine(sd, cfg, device=dev)
    tok, lens = _tokens(B, L, 3)
    sids = torch.arange(B) % cfg['num_speakers']
    mel, mel_lens, al, raw = eng.infer(tok, sids, lens, max_step=max_step, dropout_seed=2, return_raw=True)
    sess = eng.stream(tok, sids, lens, max_step=max_step, dropout_seed=2, max_chunk_steps=8)
    trace = _drive(sess, (8,))
    assert trace[-1] == max_step == raw.shape[2] and len(trace) == -(-max_step // 8)
    assert torch.equal(sess.mel_raw, raw) and torch.equal(sess.alignments, al) and torch.equal(sess.mel_lens, mel_lens)


def test_session_argument_errors(stop_eng):
    from ttsamd.lib import TtsAmdError
    cfg, sd, tok, lens, sids = _stop_case()
    with pytest.raises(ValueError):
        stop_eng.stream(tok, sids, lens, max_step=40, max_chunk_steps=12)
    sess = stop_eng.stream(tok, sids, lens, max_step=40, dropout_seed=4, max_chunk_steps=16)
    for n in (0, 4, 12, 24):                                     # not a positive multiple of 8, or more than max_chunk_steps
        with pytest.raises(TtsAmdError):
            sess.advance(n)
    assert sess.steps_done == 0 and sess.advance(8) == (8, False)


# ---- 2. the postnet over windows ----------------------------------------------------------------------------------------------------

def test_postnet_windows_as_the_frames_become_final(stop_eng):
    """mel_post put together from windows at the moments the frames become final (t + 10 < steps_done, everything at the end) is
    within MEL_TOL of the oracle on every row.  Against the one-shot engine: k = 5 convs always take the direct kernel, whose sum for
    an output column does not depend on the tile it sits in, and a zero-padded tap adds an exact zero -- so the windows are the one-shot
    postnet's bits (measured on the MI355X: max-abs 0; profiles/r36/NOTES.md), and that is asserted."""
    cfg, sd, tok, lens, sids = _stop_case()
    mel_ref, _, _ = _stop_oracle(4)
    mel_one, *_ = stop_eng.infer(tok, sids, lens, max_step=40, dropout_seed=4)
    sess = stop_eng.stream(tok, sids, lens, max_step=40, dropout_seed=4, max_chunk_steps=8)
    assert sess.halo == 10
    t0, windows = 0, []
    while not sess.ended:
        sess.advance(8)
        if sess.steps_done == 16:                                # frames [0, 10) are not final at 16 steps: 10 + 10 > 16
            ws = torch.empty(stop_eng.lib.ttsamd_tacotron2_postnet_window_bytes(stop_eng.handle, 4, 10), dtype=torch.uint8, device=sess._mel_raw.device)
            rc = stop_eng.lib.ttsamd_tacotron2_postnet_window(stop_eng.handle, C.c_void_p(sess._mel_raw.data_ptr()), C.c_void_p(sess._mel_post.data_ptr()),
                                                              4, 40, 16, 0, 10, 0, C.c_void_p(ws.data_ptr()), ws.numel(),
                                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == EINVAL
        t1 = sess.final_frames
        if t1 > t0:
            sess.postnet(t0, t1)
            windows.append((t0, t1))
            t0 = t1
    assert windows == [(0, 6), (6, 14), (14, 27)]
    got = sess.mel_post
    assert got.shape == tuple(mel_ref.shape)
    for b in range(4):
        assert maxabs(got[b], mel_ref[b]) < MEL_TOL, b
    diff = maxabs(got, mel_one)
    print(f'postnet windows {windows} against the one-shot postnet of the same engine: max-abs {diff:.3e}; against the oracle '
          f'{maxabs(got, mel_ref):.3e} (one-shot: {maxabs(mel_one, mel_ref):.3e})')
    assert torch.equal(got, mel_one)


# ---- 3. workspace ---------------------------------------------------------------------------------------------------------------------

def test_stream_workspace_is_sized_by_the_chunk(stop_eng):
    lib, h = stop_eng.lib, stop_eng.handle
    nb = lib.ttsamd_tacotron2_stream_bytes(h, 8, 256, 3000, 64)
    assert 0 < nb < lib.ttsamd_tacotron2_workspace_bytes(h, 8, 256, 3000)
    assert nb == lib.ttsamd_tacotron2_stream_bytes(h, 8, 256, 300, 64) == lib.ttsamd_tacotron2_stream_bytes(h, 8, 256, 30000, 64)
    assert lib.ttsamd_tacotron2_stream_bytes(h, 8, 256, 3000, 128) > nb
    assert lib.ttsamd_tacotron2_postnet_window_bytes(h, 8, 64) == 256 * -(-(8 * 512 * 84 * 4) // 256) * 2 + 256 * -(-(8 * 80 * 84 * 4) // 256)


# ---- 4. a vocoder stream that grows -----------------------------------------------------------------------------------------------------

def _sv(v1, **kw):
    from ttsamd.stream import StreamingVocoder
    return StreamingVocoder(v1[0], v1[1], **dict(dict(max_streams=4, max_frames=96, chunk_frames=8, first_chunk_frames=4), **kw))


def _opened(sv, mel, **kw):
    sv.open(mel, **kw)
    out = []
    while sv.open_streams:
        out += [(c.cpu(), last) for _, c, last in sv.step()]
    return out


def _grown(sv, mel, block=8, **kw):
    sid = sv.open_growing(**kw)
    out, T = [], mel.shape[1]
    assert sv.step() == [] and sv.open_streams == [sid]          # nothing ready: the stream stays open
    for t in range(0, T, block):
        sv.append(sid, mel[:, t:t + block])
        out += [(c.cpu(), last) for _, c, last in sv.step()]
    sv.finish(sid)
    while sv.open_streams:
        res = sv.step()
        assert res
        out += [(c.cpu(), last) for _, c, last in res]
    return out


@pytest.mark.parametrize('kw,okw', [({}, {}), ({}, {'denoise': 0.01}), ({'limiter': True}, {'gain_db': 6.0}),
                                    ({'sample_rate': 8000, 'encoding': 'mulaw'}, {})])
def test_growing_stream_equals_opened_stream(v1, dev, kw, okw):
    """one stream at a time, T = 1 / 14 / 40 / 70, first 4, chunks of 8, fed in blocks of 8: the chunks of open_growing + append + finish
    are those of open(mel), chunk by chunk and bit for bit -- plain, denoised, limited with 6 dB of gain, and as 8 kHz mu-law"""
    sv = _sv(v1, **kw)
    for T in (1, 14, 40, 70):
        if okw.get('denoise') and 256 * T <= 512:
            continue
        mel = torch.from_numpy(_mel(T, 100 + T)).to(dev)
        want, got = _opened(sv, mel, **okw), _grown(sv, mel, **okw)
        assert len(got) == len(want) and [l for _, l in got] == [False] * (len(got) - 1) + [True], T
        for (a, _), (b, _) in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b), T
    assert sv.free_slots == sv.max_streams


def test_three_growing_streams_at_different_paces(v1, dev, oracle_v1):
    """T = 14 / 40 / 70 open together and fed 8, 3 and 16 frames per turn: every wave within WAVE_TOL of the whole-utterance oracle"""
    sv = _sv(v1)
    Ts, pace = (14, 40, 70), (8, 3, 16)
    mels = [torch.from_numpy(oracle_v1[T][0]).to(dev) for T in Ts]
    sids = [sv.open_growing() for _ in Ts]
    fed, got, done = [0, 0, 0], {s: [] for s in sids}, set()
    for _ in range(100):
        for k, sid in enumerate(sids):
            if fed[k] < Ts[k]:
                sv.append(sid, mels[k][:, fed[k]:fed[k] + pace[k]])
                fed[k] = min(fed[k] + pace[k], Ts[k])
                if fed[k] == Ts[k]:
                    sv.finish(sid)
        for sid, chunk, last in sv.step():
            assert sid not in done
            got[sid].append(chunk.cpu())
            if last:
                done.add(sid)
        if len(done) == 3:
            break
    assert len(done) == 3 and sv.step() == [] and sv.free_slots == sv.max_streams
    errs = [float((torch.cat(got[sid]) - oracle_v1[T][1]).abs().max()) for sid, T in zip(sids, Ts)]
    print(f'three growing V1 streams, T = {Ts}: max-abs against the oracle {["%.2e" % e for e in errs]} (tol {WAVE_TOL})')
    assert max(errs) < WAVE_TOL


def test_growing_stream_errors(v1, dev):
    sv = _sv(v1)
    sid = sv.open_growing(denoise=0.01)
    sv.append(sid, torch.from_numpy(_mel(2, 1)).to(dev))
    with pytest.raises(ValueError, match='512 samples'):       # as open() on a mel of two frames
        sv.finish(sid)
    sv.close(sid)
    sid = sv.open_growing()
    with pytest.raises(ValueError):
        sv.finish(sid)                                          # no frames
    with pytest.raises(ValueError):
        sv.append(sid, torch.zeros(80, 97, device=dev))         # more than max_frames
    with pytest.raises(ValueError):
        sv.append(sid, torch.zeros(79, 4, device=dev))
    sv.close(sid)
    fixed = sv.open(torch.from_numpy(_mel(3, 1)).to(dev))
    with pytest.raises(ValueError):
        sv.append(fixed, torch.zeros(80, 4, device=dev))
    sv.close(fixed)
    with pytest.raises(ValueError):
        sv.open_growing(gain_db=3.0)                            # no limiter


def test_growing_stream_is_refused_on_the_centred_framing(dev):
    """MelVocos('24k'): T frames are 256 (T - 1) samples and the last core reads one frame past its end -- out of scope for growing streams"""
    from ttsamd import synth
    from ttsamd.config import VOCOS_24K_CONFIG
    from ttsamd.stream import StreamingVocoder
    from vocoder.vocos import MelVocos
    voc = MelVocos('24k')
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.vocos_state_dict(VOCOS_24K_CONFIG).items()})
    sv = StreamingVocoder(voc.to(dev), max_streams=2, max_frames=32, chunk_frames=8, first_chunk_frames=4)
    with pytest.raises(ValueError, match='centred'):
        sv.open_growing()
    assert sv.free_slots == 2


# ---- 5. Tacotron2Wave.tts_stream --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def wave_model(dev, taco_ckpt):
    """the synthetic checkpoint of test_dropin_tacotron2wave_tts (gate_bias -0.5, seed 4), decoder_max_step = 48, a fixed dropout seed"""
    import text
    from models.tacotron2 import Tacotron2Wave
    model = Tacotron2Wave(taco_ckpt[0], taco_ckpt[1], taco_ckpt[2], n_symbol=len(text.symbols)).to(dev)
    model.model.decoder_max_step = 48
    model.model.dropout_seed = 5
    return model


STREAM_KW = dict(chunk_frames=8, first_chunk_frames=4)


@pytest.mark.parametrize('postprocess', [True, False])
def test_tts_stream_of_one_line_equals_tts_single(wave_model, postprocess):
    """LINES[1] ends in r: with postprocess_mel the separator goes in and the mel is cut; the streamed chunks have tts_single's samples
    within WAVE_TOL, and the mel that entered the vocoder has truncate_mel's frame count (cut + the three repeated frames)"""
    line = LINES[1]
    want, mel = wave_model.tts_single(line, denoise=0.005, postprocess_mel=postprocess, return_mel=True)
    chunks = list(wave_model.tts_stream(line, denoise=0.005, postprocess_mel=postprocess, **STREAM_KW))
    got = torch.cat(chunks)
    assert all(c.device.type == 'cpu' and c.dtype == torch.float32 for c in chunks)
    assert got.numel() == want.numel() == 256 * mel.shape[1]
    sess = wave_model.stream_sessions[0]
    print(f'tts_stream({line!r}, postprocess_mel={postprocess}): {len(chunks)} chunks, {mel.shape[1]} frames of {sess.steps_done} decoded, '
          f'rows {sess.rows}; max-abs against tts_single {maxabs(got, want):.2e} (tol {WAVE_TOL})')
    assert maxabs(got, want) < WAVE_TOL
    if postprocess:
        assert mel.shape[1] == sess.rows[0][2] + 3 and sess.rows[0][2] < sess.steps_done


def test_tts_stream_of_a_list_in_batches_of_two(wave_model):
    """five lines in batches of two (the synthetic gate never fires: every batch decodes all 48 steps, so early stopping need not be
    switched off): line i's chunks arrive in order, `last` once, the wave is tts(list, batch_size=2)[i] within WAVE_TOL, and audio of
    some line leaves while its batch is still being decoded (steps_done and ended of the line's session, recorded at each yield);
    PCM16 chunks are the float chunks converted on the host"""
    from ttsamd.stream import pcm16
    want = wave_model.tts(LINES, batch_size=2, denoise=0.005)
    got, lasts, early = {i: [] for i in range(len(LINES))}, [], []
    for i, chunk, last in wave_model.tts_stream(LINES, batch_size=2, denoise=0.005, **STREAM_KW):
        assert i not in lasts
        got[i].append(chunk)
        sess = wave_model.stream_sessions[i]
        early.append((i, sess.steps_done, sess.ended))
        if last:
            lasts.append(i)
    assert sorted(lasts) == list(range(len(LINES)))
    errs = []
    for i in range(len(LINES)):
        wave = torch.cat(got[i])
        assert wave.shape == want[i].shape, i
        errs.append(maxabs(wave, want[i]))
    print(f'tts_stream(list, batch_size=2): max-abs per line {["%.2e" % e for e in errs]} (tol {WAVE_TOL}); chunks that left before '
          f'their batch had ended (line, steps_done): {[(i, s) for i, s, e in early if not e]}')
    assert max(errs) < WAVE_TOL
    assert any(not ended for _, _, ended in early)
    ints = {i: [] for i in range(len(LINES))}
    for i, chunk, last in wave_model.tts_stream(LINES, batch_size=2, denoise=0.005, pcm16=True, **STREAM_KW):
        ints[i].append(chunk)
    for i in range(len(LINES)):
        assert torch.cat(ints[i]).dtype == torch.int16
        assert np.array_equal(torch.cat(ints[i]).numpy(), pcm16(torch.cat(got[i]).numpy())), i


def test_tts_stream_refusals(wave_model):
    with pytest.raises(ValueError, match='speed'):
        wave_model.tts_stream(LINES[0], speed=1.2)
    with pytest.raises(ValueError, match='meter'):
        wave_model.tts_stream(LINES[0], meter=True)
    with pytest.raises(ValueError, match='gain_db'):
        wave_model.tts_stream(LINES[0], gain_db=3.0)
    assert len(list(wave_model.tts_stream(LINES[0], speed=1, denoise=0, **STREAM_KW))) >= 1


def test_tts_stream_of_a_two_frame_line_with_denoise_raises_as_the_one_shot_path(wave_model):
    """decoder_max_step = 2: the line is two frames (512 samples) long, which the denoiser refuses in tts_single and at the stream's finish"""
    m = wave_model.model
    m.decoder_max_step = 2
    try:
        with pytest.raises(ValueError, match='512 samples') as one:
            wave_model.tts_single(LINES[0], denoise=0.005, postprocess_mel=False)
        with pytest.raises(ValueError, match='512 samples'):
            list(wave_model.tts_stream(LINES[0], denoise=0.005, postprocess_mel=False, **STREAM_KW))
        assert 'Denoiser' in str(one.value)
        assert torch.cat(list(wave_model.tts_stream(LINES[0], denoise=0, postprocess_mel=False, **STREAM_KW))).numel() == 512
    finally:
        m.decoder_max_step = 48

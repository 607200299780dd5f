"""Stream delivery formats on the GPU (pytest -m gpu): ttsamd_stream_emit_resampled and ttsamd_wave_encode (csrc/stream.hip), the output
rate and the encodings of StreamingVocoder, Generator.stream and FastPitch2Wave.tts_stream.

The kernel is held to the whole-row resampler ON BITS (ttsamd_resample_forward's general kernel runs the same fp32 fma chain), the
encoders to tests/golden/g711.npz on every int16 value, the streams to the CPU oracle's whole-utterance wave resampled in float64 with
the same fp32 taps, at a tolerance derived from the project's wave bound and the rounding of a J-term fp32 chain."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, WAVE_TOL
from test_gpu_stream import _i32, _mel, _ptr, _run, _stream, dev, lines5, model4, v1  # noqa: F401  (fixtures of the stream tests)

pytestmark = pytest.mark.gpu

EINVAL = -1
HOP = 256
SOURCE = 22050
VOC_HALO = 13                                   # the V1 generator's receptive field in frames (test_gpu_stream.py pins it)


@pytest.fixture(scope='module')
def lib():
    from ttsamd import lib as L
    return L.load()


@pytest.fixture(scope='module')
def g711_golden():
    return dict(np.load(os.path.join(GOLDEN, 'g711.npz'), allow_pickle=False))


def _engine(rate, device):
    """the cached ResampleEngine 22 050 Hz -> rate of utils.audio (None: rate unchanged, the NULL handle)"""
    from utils.audio import _resampler
    return None if rate is None else _resampler(SOURCE, rate, 6, 0.99, 'sinc_interp_hann', device)


def _geometry(rate):
    from ttsamd.resample import geometry
    return (1, 1, 0) if rate is None else geometry(SOURCE, rate)


def _windows(x, plan, fill=np.nan):
    """the windows of `plan` (frames) cut out of the row x into [W][HOP * w_max], everything else `fill` -> (buffer, w_max, the five
    descriptor lists in samples)"""
    w_max = (max(c[3] for c in plan) + 3) & ~3
    buf = np.full((len(plan), HOP * w_max), fill, dtype=np.float32)
    for w, (cs, cn, ws, wn) in enumerate(plan):
        buf[w, :HOP * wn] = x[HOP * ws:HOP * (ws + wn)]
    desc = ([HOP * c[2] for c in plan], [HOP * c[3] for c in plan], [x.size] * len(plan), [HOP * c[0] for c in plan],
            [HOP * (c[0] + c[1]) for c in plan])
    return buf, w_max, desc


def _emit(lib, handle, buf_d, w_max, desc, c_max, fmt, out, nout=None, W=None, hop=HOP):
    W = len(desc[0]) if W is None else W
    return lib.ttsamd_stream_emit_resampled(handle, _ptr(buf_d), W, w_max, hop, *[_i32(d) for d in desc], c_max, fmt, _ptr(out), nout,
                                            _stream())


# ---- the kernel against the whole-row resampler, on bits -----------------------------------------------------------------------------------

@pytest.mark.parametrize('rate', [8000, 16000, 11025, 44100, 48000, None])
def test_emit_resampled_equals_the_whole_row_resampler_on_bits(lib, dev, rate):
    """One random row of 256 T samples, cut into windows by plan_chunks with the vocoder's 13 frames of halo plus the resampler's; every
    sample outside a window's valid part is NaN, so a read outside the contract shows in the output.  T = 1 is the window that touches
    both utterance edges.  (first, chunk) = (1, 1): cores of 256 samples, at 8 kHz shorter than one input frame o = 441, so a block's
    first and last frames are both partial and a chunk has 92 or 93 outputs (256 * 160 / 441 = 92.9), never none."""
    from ttsamd.resample import out_len
    from ttsamd.stream import chunk_outputs, plan_chunks, resample_halo_frames
    o, n, width = _geometry(rate)
    eng = _engine(rate, dev)
    halo = VOC_HALO + (resample_halo_frames(o, n, width, HOP) if rate else 0)
    for T in (1, 2, 5, 23):
        x = np.random.default_rng(10 * T + (rate or 0) % 7).uniform(-1.0, 1.0, HOP * T).astype(np.float32)
        if eng is None:
            ref = x
        else:
            ref_d, ref_n = eng.forward(torch.from_numpy(x).to(dev)[None], route='general')
            assert int(ref_n[0]) == out_len(x.size, o, n)
            ref = ref_d[0, :int(ref_n[0])].cpu().numpy()
        for first, chunk in ((1, 1), (1, 2), (2, 5)):
            plan = plan_chunks(T, first, chunk, halo, halo)
            buf, w_max, desc = _windows(x, plan)
            assert np.isnan(buf).any() or T == 1
            want = [k1 - k0 for k0, k1 in (chunk_outputs(s0, s1, o, n) for s0, s1 in zip(desc[3], desc[4]))]
            if rate == 8000 and (first, chunk) == (1, 1):
                assert set(want) <= {92, 93}
            W, c_max = len(plan), max(want) + 5
            out = torch.full((W * c_max + 64,), -7.25, dtype=torch.float32, device=dev)
            nout = (C.c_int32 * W)(*([-1] * W))
            assert _emit(lib, eng.handle if eng else None, torch.from_numpy(buf).to(dev), w_max, desc, c_max, 0, out, nout) == 0, \
                lib.ttsamd_last_error()
            got = out.cpu().numpy()
            assert list(nout) == want and sum(want) == ref.size
            rows = got[:W * c_max].reshape(W, c_max)
            whole = np.concatenate([rows[w, :want[w]] for w in range(W)])
            assert np.array_equal(whole.view(np.int32), ref.view(np.int32)), (rate, T, first, chunk)
            assert all(not rows[w, want[w]:].view(np.int32).any() for w in range(W))          # zero behind nout, +0.0 on bits
            assert np.array_equal(got[W * c_max:].view(np.int32), np.full(64, -7.25, np.float32).view(np.int32))      # the guard


# ---- the formats ---------------------------------------------------------------------------------------------------------------------------

SPECIAL = np.array([np.nan, np.inf, -np.inf, 2.0, -2.0], dtype=np.float32)
SPECIAL_PCM = np.array([0, 32767, -32768, 32767, -32768], dtype=np.int16)


def _all_int16_as_float():
    """k / 32767 in fp32 for every int16 k: the fp32 product with 32767 rounds back to k (checked here)"""
    k = np.arange(-32768, 32768, dtype=np.int64)
    x = (k / 32767).astype(np.float32)
    assert np.array_equal(np.rint(x * np.float32(32767.0)), k)
    return k.astype(np.int16), x


def _expected(fmt, pcm, g711_golden):
    if fmt == 1:
        return pcm
    return g711_golden['lin2ulaw' if fmt == 2 else 'lin2alaw'][pcm.astype(np.int32) + 32768]


@pytest.mark.parametrize('fmt', [1, 2, 3])
def test_emit_formats_on_every_int16_value(lib, dev, g711_golden, fmt):
    """the 65 536 inputs as four windows of 64 frames with the NULL handle, and a fifth utterance of five samples: NaN, +-inf, +-2"""
    pcm, x = _all_int16_as_float()
    plan = [(64 * i, 64, 64 * i, 64) for i in range(4)]
    buf, w_max, desc = _windows(x, plan)
    buf = np.concatenate([buf, np.full((1, buf.shape[1]), np.nan, np.float32)])
    buf[4, :5] = SPECIAL
    for d, v in zip(desc, (0, 5, 5, 0, 5)):
        d.append(v)
    c_max = 64 * HOP
    dtype = torch.int16 if fmt == 1 else torch.uint8
    out = torch.full((5 * c_max + 64,), 77, dtype=dtype, device=dev)
    nout = (C.c_int32 * 5)()
    assert _emit(lib, None, torch.from_numpy(buf).to(dev), w_max, desc, c_max, fmt, out, nout) == 0, lib.ttsamd_last_error()
    got = out.cpu().numpy()
    assert list(nout) == [c_max] * 4 + [5]
    assert np.array_equal(got[:4 * c_max], _expected(fmt, pcm, g711_golden))
    assert np.array_equal(got[4 * c_max:4 * c_max + 5], _expected(fmt, SPECIAL_PCM, g711_golden))
    if fmt > 1:
        assert got[4 * c_max] == (0xff if fmt == 2 else 0xd5)                              # NaN -> PCM 0 -> the encodings' zero
    assert not got[4 * c_max + 5:5 * c_max].any() and (got[5 * c_max:] == 77).all()


@pytest.mark.parametrize('fmt', [1, 2, 3])
def test_wave_encode_ragged_rows(lib, dev, g711_golden, fmt):
    """the same inputs as ragged rows, into rows of an odd stride (so that rows start at every alignment): zero behind each length up to
    min(wave_stride, out_stride), the rest of the row and the guard untouched"""
    pcm, x = _all_int16_as_float()
    lens = [0, 1, 7, 8, 9, 65536]
    B, ws, os_ = len(lens), 65536, 65539
    wave = torch.from_numpy(np.tile(x, (B, 1))).to(dev)
    dtype = torch.int16 if fmt == 1 else torch.uint8
    out = torch.full((B * os_ + 64,), 77, dtype=dtype, device=dev)
    ns = torch.tensor(lens, dtype=torch.int64, device=dev)
    assert lib.ttsamd_wave_encode(_ptr(wave), ws, _ptr(ns), B, fmt, _ptr(out), os_, _stream()) == 0, lib.ttsamd_last_error()
    got = out.cpu().numpy()
    want = _expected(fmt, pcm, g711_golden)
    for b, n in enumerate(lens):
        row = got[b * os_:(b + 1) * os_]
        assert np.array_equal(row[:n], want[:n]) and not row[n:ws].any() and (row[ws:] == 77).all(), (b, n)
    assert (got[B * os_:] == 77).all()
    # NULL lengths: the full stride; the special values; format 0 and 4 are refused
    sp = torch.from_numpy(SPECIAL).to(dev)
    out5 = torch.full((8,), 77, dtype=dtype, device=dev)
    assert lib.ttsamd_wave_encode(_ptr(sp), 5, None, 1, fmt, _ptr(out5), 5, _stream()) == 0
    assert np.array_equal(out5.cpu().numpy()[:5], _expected(fmt, SPECIAL_PCM, g711_golden)) and (out5[5:] == 77).all()
    before = out5.clone()
    assert lib.ttsamd_wave_encode(_ptr(sp), 5, None, 1, 0, _ptr(out5), 5, _stream()) == EINVAL
    assert lib.ttsamd_wave_encode(_ptr(sp), 5, None, 1, 4, _ptr(out5), 5, _stream()) == EINVAL
    assert lib.ttsamd_wave_encode(_ptr(sp), 5, None, 0, fmt, _ptr(out5), 5, _stream()) == EINVAL
    assert b'wave_encode' in lib.ttsamd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out5, before)


def test_audio_encode_and_decode(dev, g711_golden):
    from ttsamd import g711
    from utils.audio import decode, encode
    pcm, x = _all_int16_as_float()
    wave = torch.from_numpy(x[:60000].reshape(3, 20000)).to(dev)
    lens = [20000, 1, 0]
    for enc, fmt in (('pcm16', 1), ('mulaw', 2), ('alaw', 3)):
        want = _expected(fmt, pcm[:60000], g711_golden).reshape(3, 20000)
        got = encode(wave, enc)
        assert got.device == wave.device and got.shape == wave.shape and np.array_equal(got.cpu().numpy(), want)
        rag = encode(wave, enc, lens=lens).cpu().numpy()
        for b, n in enumerate(lens):
            assert np.array_equal(rag[b, :n], want[b, :n]) and not rag[b, n:].any()
        assert np.array_equal(encode(wave[0], enc).cpu().numpy(), want[0])
        host = pcm[:20000] if fmt == 1 else g711.DECODERS[enc](want[0])
        assert np.array_equal(decode(got[0].cpu(), enc), host.astype(np.float32) / 32768.0)
    with pytest.raises(ValueError):
        encode(wave, 'float32')


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_emit_resampled_refusals_leave_the_output_untouched(lib, dev):
    """TTSAMD_EINVAL before any launch.  One middle window of a 40-frame utterance at 8 kHz: core frames [20, 21), the tight window
    is the read interval itself; one sample less on either side is refused."""
    from ttsamd.stream import chunk_outputs
    o, n, width = _geometry(8000)
    eng = _engine(8000, dev)
    L, s0, s1 = HOP * 40, HOP * 20, HOP * 21
    k0, k1 = chunk_outputs(s0, s1, o, n)
    lo, hi = (k0 // n) * o - width, ((k1 - 1) // n) * o - width + 2 * width + o
    assert 0 < lo < s0 and s1 < hi < L
    w_max, c_max = 8, 96
    buf = torch.zeros(65, HOP * w_max, device=dev)
    out = torch.full((65 * c_max,), 3.5, device=dev)
    nout = (C.c_int32 * 65)(*([-1] * 65))

    def call(desc, W=1, fmt=0, cm=c_max, handle=eng.handle, hop=HOP):
        return _emit(lib, handle, buf, w_max, [list(d) * W for d in desc], cm, fmt, out, nout, W=W, hop=hop)

    ok = ([lo], [hi - lo], [L], [s0], [s1])
    assert call(ok) == 0 and nout[0] == k1 - k0
    out.fill_(3.5)
    nout[0] = -1
    assert call(([lo + 1], [hi - lo - 1], [L], [s0], [s1])) == EINVAL                        # one sample short on the left
    assert b'stream_emit_resampled' in lib.ttsamd_last_error()
    assert call(([lo], [hi - lo - 1], [L], [s0], [s1])) == EINVAL                            # ... on the right
    assert call(ok, cm=k1 - k0 - 1) == EINVAL                                                # nout > c_max
    assert call(ok, W=0) == EINVAL and call(ok, W=65) == EINVAL
    assert call(ok, fmt=4) == EINVAL and call(ok, fmt=-1) == EINVAL
    assert call(([lo], [hi - lo], [s1 - 1], [s0], [s1])) == EINVAL                           # core_end > utt_len
    assert call(([lo], [HOP * w_max + 1], [L], [s0], [s1])) == EINVAL                        # win_len > hop * w_max
    assert call(([s0 + 1], [hi - s0 - 1], [L], [s0], [s1])) == EINVAL                        # the window starts behind its core
    assert call(([lo], [hi - lo], [L], [s1], [s1])) == EINVAL                                # empty core
    torch.cuda.synchronize()
    assert bool((out == 3.5).all()) and nout[0] == -1                                        # a refusal writes neither out nor nout
    assert call(ok, W=64) == 0 and list(nout) == [k1 - k0] * 64 + [-1]                       # 64 windows are taken


# ---- end to end on the synthetic-weights V1 generator ---------------------------------------------------------------------------------------

TS = [70, 1, 14]
STRENGTHS = [0.01, 0.0, 0.01]                   # the one-frame utterance is too short for the denoiser


@pytest.fixture(scope='module')
def oracle(synth_weights):
    """{T: (mel [80, T] float32, the oracle's whole-utterance wave in float64 [256 T], denoised at STRENGTHS where that is > 0)}"""
    import tts_oracle as O
    from ttsamd.config import HIFIGAN_CONFIG
    W = O.fold_weight_norm(synth_weights['hifigan'])
    bias = O.denoiser_bias_spec(W, HIFIGAN_CONFIG)
    out = {}
    for T, s in zip(TS, STRENGTHS):
        mel = _mel(T, 100 + T)
        wave = O.hifigan_forward(W, torch.from_numpy(mel), HIFIGAN_CONFIG, dtype=torch.float64)[0]
        if s > 0:
            wave = O.denoise(wave[None], bias, s)[0]
        out[T] = (mel, wave.double().numpy())
    return out


def _resample_f64(x, rate):
    """the polyphase sum in float64 with the fp32 taps of the device table -> (out [ceil(n L / o)], G = max_p sum_j |taps[p][j]|, J)"""
    from ttsamd.resample import out_len, resample_taps
    taps, width, o, n = resample_taps(SOURCE, rate)
    J, L = taps.shape[1], x.size
    frames = -(-out_len(L, o, n) // n)
    xz = np.zeros(width + (frames - 1) * o + J + 1, dtype=np.float64)
    xz[width:width + L] = x
    idx = np.arange(frames)[:, None] * o + np.arange(J)[None, :]
    out = (xz[idx] @ taps.astype(np.float64).T).reshape(-1)[:out_len(L, o, n)]
    return out, float(np.abs(taps.astype(np.float64)).sum(axis=1).max()), J


def _tol(G, J, peak):
    """the project's wave bound carried through the filter, plus the rounding bound of a J-term fp32 fma chain"""
    return WAVE_TOL * G + J * 2.0 ** -24 * G * peak


def _sv(v1, **kw):
    from ttsamd.stream import StreamingVocoder
    return StreamingVocoder(v1[0], v1[1], **dict(dict(max_streams=8, max_frames=96, chunk_frames=8, first_chunk_frames=4), **kw))


@pytest.mark.parametrize('rate', [8000, 48000])
def test_streams_at_another_rate_match_the_resampled_oracle(v1, oracle, rate):
    """70, 1 and 14 frames in one pool, first 4 then chunks of 8, the 14-frame stream joining two steps late, the bias denoiser on two
    of the three rows (their windows carry vocoder + denoiser + resampler halos)."""
    from ttsamd.resample import out_len
    sv = _sv(v1, sample_rate=rate)
    o, n, width = _geometry(rate)
    assert sv.sample_rate == rate and sv.encoding == 'float32'
    got = _run(sv, [oracle[T][0] for T in TS], strengths=STRENGTHS, late=(2,))
    for i, T in enumerate(TS):
        wave = torch.cat(got[i])
        ref, G, J = _resample_f64(oracle[T][1], rate)
        assert wave.dtype == torch.float32 and wave.numel() == out_len(HOP * T, o, n) == ref.size
        err, tol = float(np.abs(wave.double().numpy() - ref).max()), _tol(G, J, float(np.abs(oracle[T][1]).max()))
        print(f'streamed at {rate} Hz, T = {T}, denoise {STRENGTHS[i]}: {len(got[i])} chunks, max-abs against the float64 oracle {err:.2e} '
              f'(tol {tol:.2e}: G = {G:.3f}, J = {J})')
        assert err < tol


@pytest.fixture(scope='module')
def float_run_16k(v1, oracle):
    return _run(_sv(v1, sample_rate=16000), [oracle[T][0] for T in TS], strengths=STRENGTHS)


@pytest.mark.parametrize('encoding', ['pcm16', 'mulaw', 'alaw'])
def test_encoded_chunks_equal_the_float_chunks_converted_on_the_host(v1, oracle, float_run_16k, encoding):
    from ttsamd import g711
    from ttsamd.stream import pcm16
    sv = _sv(v1, sample_rate=16000, encoding=encoding)
    assert sv.encoding == encoding and sv.sample_rate == 16000
    got = _run(sv, [oracle[T][0] for T in TS], strengths=STRENGTHS)
    for i in range(len(TS)):
        assert len(got[i]) == len(float_run_16k[i])
        for a, b in zip(got[i], float_run_16k[i]):
            want = pcm16(b.numpy())
            if encoding != 'pcm16':
                want = g711.ENCODERS[encoding](want)
            assert a.dtype == (torch.int16 if encoding == 'pcm16' else torch.uint8) and np.array_equal(a.numpy(), want), (TS[i], encoding)


def test_pcm16_flag_and_encoding_agree(v1):
    assert _sv(v1, pcm16=True).encoding == 'pcm16' and _sv(v1, pcm16=True, encoding='pcm16').pcm16
    assert _sv(v1).sample_rate == SOURCE and _sv(v1).encoding == 'float32'
    with pytest.raises(ValueError):
        _sv(v1, pcm16=True, encoding='alaw')


def test_generator_stream_at_16k_equals_the_streaming_vocoder(v1, oracle):
    from ttsamd.stream import StreamingVocoder
    gen = v1[0]
    mel = torch.from_numpy(oracle[70][0]).to(gen.device)
    chunks = [c.cpu() for c in gen.stream(mel, sample_rate=16000)]
    sv = StreamingVocoder(gen, max_streams=1, max_frames=70, sample_rate=16000)
    direct = _run(sv, [oracle[70][0]])[0]
    assert len(chunks) == len(direct) == 2 and all(torch.equal(a, b) for a, b in zip(chunks, direct))
    assert sum(c.numel() for c in chunks) == -(-320 * HOP * 70 // 441)


def test_the_path_without_a_resampler_is_unchanged(v1, oracle):
    """sample_rate = the vocoder's own with float32 is ttsamd_stream_emit, as before: the bits of StreamingVocoder()"""
    a = _run(_sv(v1), [oracle[T][0] for T in TS], strengths=STRENGTHS)
    sv = _sv(v1, sample_rate=SOURCE, encoding='float32')
    assert not sv._resampled
    b = _run(sv, [oracle[T][0] for T in TS], strengths=STRENGTHS)
    for i in range(len(TS)):
        assert len(a[i]) == len(b[i]) and all(torch.equal(p, q) for p, q in zip(a[i], b[i]))


# ---- the drop-in surface ---------------------------------------------------------------------------------------------------------------------

def test_tts_stream_of_one_line_as_8k_mulaw(model4, lines5):
    from ttsamd.resample import out_len
    ref = model4.tts_single(lines5[0], denoise=0.0, speaker_id=1)
    chunks = list(model4.tts_stream(lines5[0], chunk_frames=16, first_chunk_frames=8, denoise=0.0, speaker_id=1, sample_rate=8000,
                                    encoding='mulaw'))
    assert len(chunks) > 3 and all(c.device.type == 'cpu' and c.dtype == torch.uint8 for c in chunks)
    assert ref.numel() % HOP == 0 and sum(c.numel() for c in chunks) == out_len(ref.numel(), 441, 160)


def test_tts_stream_of_a_list_at_8k(model4, lines5):
    """five lines with their own speed and denoise strength through two slots, leaving at 8 kHz: every line's total, and its samples
    against utils.audio.resample of tts_single's wave in float32"""
    from ttsamd.resample import out_len, resample_taps
    from utils.audio import resample
    speed, denoise = [0.8, 1.0, 1.25, 1.0, 2.0], [0.005, 0.0, 0.1, 0.0, 0.02]
    kw = dict(chunk_frames=16, first_chunk_frames=8, max_streams=2, speed=speed, denoise=denoise, speaker_id=2)
    got, finished = {i: [] for i in range(5)}, []
    for i, chunk, last in model4.tts_stream(lines5, sample_rate=8000, **kw):
        assert i not in finished and chunk.device.type == 'cpu' and chunk.dtype == torch.float32
        got[i].append(chunk)
        if last:
            finished.append(i)
    assert sorted(finished) == [0, 1, 2, 3, 4]
    taps = resample_taps(SOURCE, 8000)[0].astype(np.float64)
    G, J = float(np.abs(taps).sum(axis=1).max()), taps.shape[1]
    errs = []
    for i, line in enumerate(lines5):
        single = model4.tts_single(line, speed=speed[i], denoise=denoise[i], speaker_id=2)
        ref = resample(single.reshape(1, -1).to(model4.device), SOURCE, 8000)[0].cpu()
        wave = torch.cat(got[i])
        assert wave.numel() == out_len(single.numel(), 441, 160) == ref.numel(), i
        errs.append((float((wave - ref).abs().max()), _tol(G, J, float(single.abs().max()))))
    print(f'tts_stream(list of 5, two slots, 8 kHz): max-abs against resample(tts_single) per line {["%.2e (tol %.2e)" % e for e in errs]}')
    assert all(e < t for e, t in errs)

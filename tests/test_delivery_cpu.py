"""CPU: the host side of the stream delivery formats (output sample rate, PCM16, G.711 mu-law / A-law) and the facts it rests on.

  * ttsamd/g711.py against tests/golden/g711.npz (tools/gen_golden_g711.py: the standard library's audioop on every value), both ways;
  * the reach of the resampler around a core, brute force, against the bound width + o - 1 that sizes the extra halo;
  * the chunk counts of a plan add up to the whole utterance's output length, consecutive ranges abutting;
  * G.711 WAVE files: header fields and the round trip through load_wav;
  * the argument errors of StreamingVocoder, which are raised before anything touches the GPU.
The GPU tests are in test_gpu_delivery.py."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN

RATES = [8000, 11025, 16000, 24000, 44100, 48000]
SOURCE = 22050
HOP = 256


@pytest.fixture(scope='module')
def g711_golden():
    return dict(np.load(os.path.join(GOLDEN, 'g711.npz'), allow_pickle=False))


def test_g711_module_equals_the_golden_on_every_value(g711_golden):
    from ttsamd import g711
    pcm = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    codes = np.arange(256, dtype=np.uint8)
    assert g711_golden['lin2ulaw'].shape == (65536,) and g711_golden['ulaw2lin'].shape == (256,)
    assert np.array_equal(g711.lin2ulaw(pcm), g711_golden['lin2ulaw'])
    assert np.array_equal(g711.lin2alaw(pcm), g711_golden['lin2alaw'])
    assert np.array_equal(g711.ulaw2lin(codes), g711_golden['ulaw2lin'])
    assert np.array_equal(g711.alaw2lin(codes), g711_golden['alaw2lin'])
    assert g711.lin2ulaw(pcm).dtype == np.uint8 and g711.alaw2lin(codes).dtype == np.int16


def test_g711_encode_of_decode_is_the_byte():
    from ttsamd import g711
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(g711.lin2alaw(g711.alaw2lin(codes)), codes)
    back = g711.lin2ulaw(g711.ulaw2lin(codes))
    assert np.nonzero(back != codes)[0].tolist() == [0x7f]            # mu-law has two zeros: 0x7f ("negative zero") decodes to 0 ...
    assert int(g711.ulaw2lin(codes)[0x7f]) == 0 and int(back[0x7f]) == 0xff          # ... which encodes as 0xff


def _geometry(rate):
    from ttsamd.resample import geometry
    return geometry(SOURCE, rate)


def test_resample_halo_frames_table():
    from ttsamd.stream import resample_halo_frames, resample_reach
    want_reach = {8000: 457, 16000: 449, 48000: 153, 44100: 7}
    want_frames = {8000: 2, 16000: 2, 32000: 2, 11025: 1, 24000: 1, 44100: 1, 48000: 1}
    for rate, frames in want_frames.items():
        o, n, width = _geometry(rate)
        assert resample_halo_frames(o, n, width, HOP) == frames, rate
        assert resample_reach(o, width) == width + o - 1
        if rate in want_reach:
            assert resample_reach(o, width) == want_reach[rate]


def test_geometry_is_the_table_builders():
    from ttsamd.resample import resample_taps
    for rate in RATES:
        taps, width, o, n = resample_taps(SOURCE, rate)
        assert _geometry(rate) == (o, n, width) and taps.shape == (n, 2 * width + o)


@pytest.mark.parametrize('rate', RATES)
def test_reach_of_the_resampler_stays_within_the_bound(rate):
    """every hop-aligned core of 1 and 2 frames in a 40-frame utterance: the samples its outputs read, [f0 o - width, f1 o - width + J),
    lie within width + o - 1 of the core"""
    from ttsamd.stream import chunk_outputs, resample_reach
    o, n, width = _geometry(rate)
    J, bound, T = 2 * width + o, resample_reach(*_geometry(rate)[::2]), 40
    most = [0, 0]
    for frames in (1, 2):
        for f in range(T - frames + 1):
            s0, s1 = HOP * f, HOP * (f + frames)
            k0, k1 = chunk_outputs(s0, s1, o, n)
            assert k1 > k0                                            # a whole frame of input always holds an output at these rates
            lo, hi = (k0 // n) * o - width, ((k1 - 1) // n) * o - width + J
            left, right = s0 - lo, hi - s1
            assert left <= bound and right <= bound, (rate, f, frames, left, right, bound)
            most = [max(most[0], left), max(most[1], right)]
    print(f'{SOURCE} -> {rate} Hz: reach left / right {most[0]} / {most[1]}, bound {bound}')
    assert most[0] >= 0 and most[1] >= 0


@pytest.mark.parametrize('rate', RATES)
def test_chunk_counts_of_a_plan_add_up(rate):
    from ttsamd.resample import out_len
    from ttsamd.stream import chunk_outputs, plan_chunks, resample_halo_frames
    o, n, width = _geometry(rate)
    halo = 13 + resample_halo_frames(o, n, width, HOP)
    for T in (1, 2, 5, 23, 40):
        end, total = 0, 0
        for cs, cn, ws, wn in plan_chunks(T, 1, 1, halo, halo):
            k0, k1 = chunk_outputs(HOP * cs, HOP * (cs + cn), o, n)
            assert k0 == end                                          # consecutive ranges abut: nothing twice, nothing dropped
            end, total = k1, total + (k1 - k0)
        assert total == end == out_len(HOP * T, o, n), (rate, T)


@pytest.mark.parametrize('encoding,code', [('ULAW', 7), ('ALAW', 6)])
def test_g711_wav_round_trip(tmp_path, encoding, code):
    from ttsamd import g711
    from ttsamd.stream import pcm16
    from utils.audio import decode, load_wav, save_wav
    name = {'ULAW': 'mulaw', 'ALAW': 'alaw'}[encoding]
    rng = np.random.default_rng(3)
    wave = np.concatenate([rng.uniform(-1.2, 1.2, 8001), [0.0, 1.0, -1.0]]).astype(np.float32)      # an odd byte count: the pad byte
    path = str(tmp_path / f'{name}.wav')
    save_wav(path, wave, 8000, encoding=encoding, bits_per_sample=8)
    raw = open(path, 'rb').read()
    assert raw[:4] == b'RIFF' and raw[8:16] == b'WAVEfmt ' and struct.unpack('<I', raw[4:8])[0] == len(raw) - 8 and len(raw) % 2 == 0
    size, fmt, channels, rate, byte_rate, block, bits, extra = struct.unpack('<IHHIIHHH', raw[16:38])
    assert (size, fmt, channels, rate, byte_rate, block, bits, extra) == (18, code, 1, 8000, 8000, 1, 8, 0)
    assert raw[38:42] == b'fact' and struct.unpack('<II', raw[42:50]) == (4, wave.size)
    assert raw[50:54] == b'data' and struct.unpack('<I', raw[54:58])[0] == wave.size
    data = g711.ENCODERS[name](pcm16(wave))
    assert raw[58:58 + wave.size] == data.tobytes()
    got, got_rate = load_wav(path)
    assert got_rate == 8000 and got.dtype == np.float32
    assert np.array_equal(got, g711.DECODERS[name](data).astype(np.float32) / 32768.0) and np.array_equal(got, decode(data, name))
    assert float(np.abs(got - np.clip(wave, -1, 1)).max()) < 0.04    # 8-bit companding: the largest step is 1024 / 32768 (A-law)
    # data that is already encoded is written as it is
    save_wav(path, data, 8000, encoding=encoding, bits_per_sample=8)
    assert open(path, 'rb').read() == raw
    with pytest.raises(ValueError):
        save_wav(path, wave, 8000, encoding=encoding, bits_per_sample=16)
    assert np.array_equal(decode(np.int16([-32768, 0, 16384]), 'pcm16'), np.float32([-1.0, 0.0, 0.5]))
    with pytest.raises(ValueError):
        decode(data, 'opus')


def test_argument_errors_come_before_the_gpu():
    """the delivery arguments are checked on the host, first: the vocoder is never touched"""
    from ttsamd.stream import StreamingVocoder, delivery
    with pytest.raises(ValueError, match='pcm16'):
        StreamingVocoder(object(), pcm16=True, encoding='mulaw')
    with pytest.raises(ValueError, match='encoding'):
        StreamingVocoder(object(), encoding='opus')
    with pytest.raises(ValueError, match=r'o = 22050 / n = 8003 outside \[1, 4096\]'):       # 8 003 Hz shares no factor with 22 050
        StreamingVocoder(object(), sample_rate=8003)
    assert delivery(22050, 8001)[2] == (350, 127, 17)                                          # 8 001 = 63 * 127 reduces and is built
    with pytest.raises(ValueError):
        StreamingVocoder(object(), sample_rate=8000.5)
    assert delivery(22050) == ('float32', 22050, None) and delivery(22050, 22050, 'pcm16', True) == ('pcm16', 22050, None)
    assert delivery(22050, None, None, True) == ('pcm16', 22050, None) and delivery(22050, 8000, 'mulaw') == ('mulaw', 8000, (441, 160, 17))
    assert delivery(22050, 48000) == ('float32', 48000, (147, 320, 7))

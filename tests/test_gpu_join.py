"""GPU: the paragraph join (csrc/join.hip, ttsamd/join.py, utils.audio.join_waves) against its numpy restatement (tests/join_ref.py, pinned
by tests/test_join_cpu.py), bit for bit; and `tts_long` of both models and `inference.py --long` on the synthetic checkpoints.

`tts_long` against `tts(segment)`: the joined wave holds, between the fades, a copy of the segment's own samples, and a row computed as
if alone equals its batch-of-one call within the project's fp32 bound (conftest.WAVE_TOL), so that bound is the tolerance.
normalize='lufs': the joined wave read back by utils.audio.loudness sits at -23 LUFS within 1e-4, the bound tests/test_gpu_loudness.py
and tests/test_gpu_limiter.py hold a levelled row to."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import join_ref as J
from conftest import GOLDEN, WAVE_TOL

pytestmark = pytest.mark.gpu

LENGTHS = [257, 0, 4097, 5, 1023, 256, 1, 2049, 255]            # [0, 1, 5, 255, 256, 257, 1023, 2049, 4097] shuffled
SENTINEL = 12345.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _batch(lengths=tuple(LENGTHS), seed=0, pad=3):
    """rows of noise, the stride a little wider than the longest row; what lies behind a row's length is noise too (it must not be read)"""
    rng = np.random.default_rng(seed)
    wave = rng.standard_normal((len(lengths), max(lengths) + pad)).astype(np.float32)
    return wave, np.array(lengths, dtype=np.int64)


def _bounds(lengths):
    """odd starts, an all-silent row (0, 0), rows whose bounds touch sample 0 and the last sample"""
    out = []
    for b, n in enumerate(lengths):
        if n == 0 or b == 3:
            out.append((0, 0))
        elif b % 3 == 0:
            out.append((0, n))                                      # touches both ends: keep is clamped at both
        elif b % 3 == 1:
            out.append((min(3, n - 1), n))                          # touches the last sample
        else:
            out.append((0, max(n - 5, 1)) if b % 2 else (min(7, n - 1), max(n - 3, min(7, n - 1))))
    return np.array(out, dtype=np.int64)


def _gaps(B, F):
    """0, 1, 500, -1, -64, -F and one below -F, in turn"""
    pool = [0, -1, 500, -64, 1, -F, -(F + 1000), 0, -3]
    return [pool[b % len(pool)] for b in range(B)]


def _run(dev, wave, ns, bounds, gaps, fade, keep, lead, out_stride, offset=0, tail=16):
    """ttsamd_wave_join through the C ABI into a buffer filled with a sentinel; -> (out [out_stride], segs [B, 4], total, the buffer)"""
    from ttsamd import lib
    h = lib.load()
    B = wave.shape[0]
    w = torch.from_numpy(wave).to(dev)
    n = torch.from_numpy(np.asarray(ns, dtype=np.int64)).to(dev)
    bd = torch.from_numpy(bounds).to(dev) if bounds is not None else None
    g = torch.tensor(list(gaps), dtype=torch.int64).to(dev)
    f = torch.from_numpy(np.asarray(fade, dtype=np.float32)).to(dev) if fade is not None and len(fade) else None
    buf = torch.full((offset + out_stride + tail,), SENTINEL, dtype=torch.float32, device=dev)
    segs = torch.full((B, 4), -7, dtype=torch.int64, device=dev)
    total = torch.full((1,), -7, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)                # noqa: E731
    out_ptr = C.c_void_p(buf.data_ptr() + 4 * offset)
    rc = h.ttsamd_wave_join(p(w), wave.shape[1], p(n), p(bd), p(g), B, p(f), 0 if f is None else f.numel(), keep, lead, out_ptr, out_stride,
                            p(segs), p(total), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib.check(rc, 'wave_join')
    torch.cuda.synchronize()
    buf = buf.cpu().numpy()
    return buf[offset:offset + out_stride], segs.cpu().numpy(), int(total[0]), buf


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


@pytest.mark.parametrize('F', [0, 1, 64, 110, 4096])
@pytest.mark.parametrize('with_bounds', [False, True])
def test_join_kernel_is_the_reference_bit_for_bit(dev, F, with_bounds):
    """the nine lengths in one batch; keep in {0, 7}, lead in {0, 1, 3} and the output buffer at every alignment (vector stores with a
    scalar head and tail); with F = 4096 every row is shorter than 2 F"""
    wave, ns = _batch()
    bounds = _bounds(LENGTHS) if with_bounds else None
    fade = J.fade_table(F)
    gaps = _gaps(len(LENGTHS), F)
    for keep, lead, offset in ((0, 0, 0), (7, 1, 1), (7, 3, 2), (0, 1, 3), (0, 3, 0)):
        _, _, want_total = J.join(wave, ns, bounds, gaps, fade, keep, lead, 0)
        stride = want_total + 37                                     # zeros from `total` to out_stride, then the sentinel
        want, want_segs, _ = J.join(wave, ns, bounds, gaps, fade, keep, lead, stride)
        got, segs, total, buf = _run(dev, wave, ns, bounds, gaps, fade, keep, lead, stride, offset)
        assert total == want_total and np.array_equal(segs, want_segs), (keep, lead, offset)
        assert _same(got, want), (keep, lead, offset, int(np.flatnonzero(got != want)[0]))
        assert not got[total:].any()
        assert (buf[:offset] == SENTINEL).all() and (buf[offset + stride:] == SENTINEL).all()
        again, segs2, total2, _ = _run(dev, wave, ns, bounds, gaps, fade, keep, lead, stride, offset)
        assert _same(again, got) and np.array_equal(segs2, segs) and total2 == total        # run twice: the same bits
    if with_bounds:
        assert (want_segs[3, 2:] == 0).all() and want_segs[3, 0] == want_segs[3, 1]           # the all-silent row: no samples, its gap counts


@pytest.mark.parametrize('B', [1, 33, 300])
def test_join_kernel_batch_sizes(dev, B):
    """B = 1, B = 33, and 300 rows: more than one row per thread of the scan block"""
    rng = np.random.default_rng(B)
    lengths = tuple(int(v) for v in rng.integers(0, 40, B)) if B > 1 else (77,)
    wave, ns = _batch(lengths, seed=B)
    F = 8
    gaps = [int(v) for v in rng.integers(-12, 6, B)]
    _, _, want_total = J.join(wave, ns, None, gaps, J.fade_table(F), 2, 3, 0)
    want, want_segs, _ = J.join(wave, ns, None, gaps, J.fade_table(F), 2, 3, want_total + 5)
    got, segs, total, buf = _run(dev, wave, ns, None, gaps, J.fade_table(F), 2, 3, want_total + 5)
    assert total == want_total and np.array_equal(segs, want_segs) and _same(got, want)
    assert (buf[want_total + 5:] == SENTINEL).all()


def test_join_kernel_truncates_and_reports_the_whole_length(dev):
    wave, ns = _batch()
    F = 64
    fade, gaps = J.fade_table(F), _gaps(len(LENGTHS), F)
    full, full_segs, full_total = J.join(wave, ns, None, gaps, fade, 0, 1, 9000)
    for stride in (0, 1, 5, 4098, 4099):
        got, segs, total, buf = _run(dev, wave, ns, None, gaps, fade, 0, 1, stride, offset=1)
        assert total == full_total > stride and np.array_equal(segs, full_segs)
        assert _same(got, full[:stride])
        assert (buf[:1] == SENTINEL).all() and (buf[1 + stride:] == SENTINEL).all()           # nothing past out_stride


def test_join_kernel_refusals(dev):
    from ttsamd import lib
    from ttsamd.lib import TtsAmdError
    h = lib.load()
    w = torch.zeros(2, 8, device=dev)
    n = torch.tensor([8, 8], device=dev)
    g = torch.zeros(4097, dtype=torch.int64, device=dev)
    f = torch.ones(4097, device=dev)
    out = torch.full((64,), SENTINEL, device=dev)
    segs = torch.full((4097, 4), -7, dtype=torch.int64, device=dev)
    total = torch.full((1,), -7, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)                # noqa: E731

    def call(wave=w, ns=n, gap=g, B=2, fade=f, F=4, keep=0, lead=0, o=out, stride=64, sg=segs, tot=total):
        return h.ttsamd_wave_join(p(wave), 8, p(ns), None, p(gap), B, p(fade), F, keep, lead, p(o), stride, p(sg), p(tot), None)
    assert call() == 0
    torch.cuda.synchronize()
    assert int(total[0]) == 16
    out.fill_(SENTINEL)
    total.fill_(-7)
    segs.fill_(-7)
    bad = [dict(B=0), dict(B=4097), dict(F=4097), dict(F=-1), dict(wave=None), dict(ns=None), dict(gap=None), dict(o=None), dict(sg=None),
           dict(tot=None), dict(fade=None), dict(keep=-1), dict(lead=-1), dict(stride=-1)]
    for kw in bad:
        rc = call(**kw)
        assert rc != 0, kw
        with pytest.raises(TtsAmdError):
            lib.check(rc, 'wave_join')
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and int(total[0]) == -7 and bool((segs == -7).all())  # nothing launched
    assert call(fade=None, F=0) == 0                                                          # no table with no fades is fine


def test_join_rows_and_join_waves(dev):
    from ttsamd.join import fade_table, join_rows
    from utils.audio import join_waves
    lengths = [300, 1, 1025, 64]
    wave, ns = _batch(tuple(lengths), seed=3, pad=0)
    rows = [torch.from_numpy(wave[b, :n].copy()) for b, n in enumerate(lengths)]
    # join_rows: the engine call, the output cut to `total`
    out, segs = join_rows(torch.from_numpy(wave).to(dev), torch.from_numpy(ns).to(dev), [10, -20, 0, 30], keep=0, lead=2, fade=fade_table(16))
    want, want_segs, total = J.join(wave, ns, None, [10, -20, 0, 30], J.fade_table(16), 0, 2, 2000)
    assert out.shape == (1, total) and out.device.type == 'cuda' and segs.dtype == torch.int64 and segs.device.type == 'cpu'
    assert _same(out[0].cpu().numpy(), want[:total]) and np.array_equal(segs.numpy(), want_segs)
    # join_waves on a list of host tensors of different lengths, no trim: 5 ms = 110 samples of fade, pauses in samples of 22 050 Hz
    got, segs = join_waves(rows, pause_ms=[100.0, -5.0, 0.0, 20.0], trim_db=None)
    gaps = [2205, -110, 0, 441]
    want, want_segs, total = J.join(wave, ns, None, gaps, J.fade_table(110), 221, 0, 6000)
    assert got.shape == (total,) and got.device.type == 'cuda'
    assert _same(got.cpu().numpy(), want[:total]) and np.array_equal(segs.numpy(), want_segs)
    # one pause: between the waves, none behind the last; a [B, n] tensor + lens is the same call
    got1, segs1 = join_waves(rows, pause_ms=100.0, trim_db=None)
    got2, segs2 = join_waves(torch.from_numpy(wave).to(dev), lens=torch.from_numpy(ns), pause_ms=[100.0, 100.0, 100.0, 0.0], trim_db=None)
    assert torch.equal(got1, got2) and torch.equal(segs1, segs2) and got1.numel() == sum(lengths) + 3 * 2205
    with pytest.raises(ValueError):
        join_waves(rows, pause_ms=[1.0, 2.0], trim_db=None)
    with pytest.raises(ValueError):
        join_waves([], trim_db=None)


def test_join_waves_trims_to_the_speech_bounds(dev):
    """zeros + noise burst + zeros: src_* are utils.audio.trim's bounds (frame 1024, hop 256) widened by keep_ms"""
    from utils.audio import join_waves, trim
    rng = np.random.default_rng(9)
    rows = []
    for lead, burst, tail in ((3000, 5000, 2500), (0, 4000, 6000), (1500, 2600, 0), (2048, 3072, 1024)):
        x = np.zeros(lead + burst + tail, dtype=np.float32)
        x[lead:lead + burst] = 0.3 * rng.standard_normal(burst)
        rows.append(torch.from_numpy(x))
    out, segs = join_waves(rows, pause_ms=50.0, trim_db=40.0, keep_ms=10.0, fade_ms=5.0)
    keep = 221
    pos = 0
    for b, r in enumerate(rows):
        _, (s, e) = trim(r.to(dev), top_db=40.0, frame_length=1024, hop_length=256)
        assert 0 <= s < e <= r.numel() and e - s < r.numel()
        want = (max(0, s - keep), min(r.numel(), e + keep))
        assert tuple(segs[b, 2:].tolist()) == want, (b, segs[b].tolist(), (s, e))
        assert segs[b, 0] == pos and segs[b, 1] - segs[b, 0] == want[1] - want[0]
        pos = int(segs[b, 1]) + (1103 if b < 3 else 0)                                        # 50 ms = 1102.5 -> 1103 samples
    assert out.numel() == pos
    # the interior of a row is a copy of its source
    s0, e0 = (int(v) for v in segs[0, 2:])
    assert torch.equal(out[110:e0 - s0 - 110].cpu(), rows[0][s0 + 110:e0 - 110])


# ---- through the models ----
@pytest.fixture(scope='module')
def model(tmp_path_factory, synth_weights, dev):
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    d = tmp_path_factory.mktemp('ckpt_join')
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['fastpitch'].items()}, 'config': dict(NET_CONFIG),
                'symbols': list(text.symbols)}, d / 'fp.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    return FastPitch2Wave(str(d / 'fp.pth'), vocoder_sd=str(d / 'hg.pth'), vocoder_config=str(d / 'config.json')).to(dev), d


@pytest.fixture(scope='module')
def paragraph():
    """six of the shortest committed infer_text lines joined with '. ', the Arabic comma, a newline and the Arabic question mark: five
    sentences, three of them closed by a mark"""
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        every = json.load(f)
    a, b, c, d, e, f6 = (every[i] for i in (9, 14, 92, 63, 35, 68))
    return f'{a}. {b}، {c}\n{d}. {e}؟ {f6}'


KINDS = ['sentence', 'paragraph', 'sentence', 'sentence', 'end']
F_FADE = 110          # 5 ms at 22 050 Hz
PAUSE = {'paragraph': 15435, 'sentence': 7718, 'clause': 5513, 'comma': 3308, 'end': 0}


@pytest.fixture(scope='module')
def long_result(model, paragraph):
    return model[0].tts_long(paragraph, denoise=0, return_segments=True)


def _check_table(out, rows, pieces):
    assert [(r['text'], r['boundary']) for r in rows] == pieces
    pos = 0
    for r in rows:
        assert r['end'] - r['start'] == r['src_end'] - r['src_start'] > 0 and r['src_start'] >= 0
        if r['boundary'] != 'forced':
            assert r['start'] == pos, (r, pos)
            pos = r['end'] + PAUSE[r['boundary']]
            assert not bool(out[r['end']:pos].any())                                           # the pause: exactly zero
        else:
            pos = None
    return pos


def test_tts_long_segments_pauses_and_samples(model, paragraph, long_result):
    from text import split_text, spoken_text
    m, _ = model
    out, rows = long_result
    pieces = split_text(paragraph)
    assert [k for _, k in pieces] == KINDS
    assert out.dim() == 1 and out.device.type == 'cpu' and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert _check_table(out, rows, pieces) == out.numel() == rows[-1]['end']
    assert rows[0]['start'] == 0
    for r in rows:
        # what the model says for a segment is the segment without the marks that close it (text.spoken_text): a free-standing '.' is a
        # token outside the symbol table, on which `tts` raises KeyError as the reference does
        line = spoken_text(r['text'])
        if r['text'].endswith('.'):
            assert line == r['text'][:-1]
            with pytest.raises(KeyError):
                m.tts(r['text'], denoise=0)
        own = m.tts(line, denoise=0)
        assert r['src_end'] <= own.numel()
        a = out[r['start'] + F_FADE:r['end'] - F_FADE]
        b = own[r['src_start'] + F_FADE:r['src_end'] - F_FADE]
        err = float((a - b).abs().max())
        print(f'{r["boundary"]:9s} {r["end"] - r["start"]:6d} samples of {own.numel():6d} (from {r["src_start"]}): against tts(segment) {err:.2e} '
              f'(tol {WAVE_TOL:.0e})')
        assert a.numel() > 0 and err < WAVE_TOL
    # a list of strings: paragraphs
    out2, rows2 = m.tts_long(paragraph.split('\n'), denoise=0, return_segments=True)
    assert rows2 == rows and torch.equal(out2, out)
    assert torch.equal(m.tts_long(paragraph, denoise=0), out)
    for empty in ('', ' \n ', []):
        with pytest.raises(ValueError):
            m.tts_long(empty)


def test_tts_long_does_not_depend_on_the_grouping(model, paragraph, long_result):
    m, _ = model
    out32, rows32 = long_result
    out2, rows2 = m.tts_long(paragraph, denoise=0, batch_size=2, return_segments=True)
    assert rows2 == rows32 and out2.shape == out32.shape
    err = float((out2 - out32).abs().max())
    print(f'batch_size 2 against 32: {err:.2e} (tol {WAVE_TOL:.0e})')
    assert err < WAVE_TOL


def test_tts_long_levels_the_joined_wave_as_one_row(model, paragraph, long_result):
    from utils.audio import loudness
    m, _ = model
    out, rows = m.tts_long(paragraph, denoise=0, normalize='lufs', return_segments=True)
    plain, plain_rows = long_result
    assert rows == plain_rows and out.shape == plain.shape
    lufs = float(loudness(out.to(m.device))[0])
    print(f"normalize='lufs': the joined wave reads {lufs:.5f} LUFS")
    assert abs(lufs + 23.0) < 1e-4
    gain = out[rows[0]['start'] + 200] / plain[rows[0]['start'] + 200]
    k = rows[-1]['start'] + 200
    assert abs(float(out[k] / plain[k] / gain) - 1.0) < 1e-5                                    # one gain for the paragraph
    for r in rows[:-1]:
        assert not bool(out[r['end']:r['end'] + PAUSE[r['boundary']]].any())
    with pytest.raises(ValueError):
        m.tts_long(paragraph, normalize=['lufs'] * 5)
    with pytest.raises(ValueError):
        m.tts_long(paragraph, pauses={'phrase': 100})


def test_tts_long_forced_seam_is_overlap_added(model, paragraph):
    from text import split_text
    m, _ = model
    line = paragraph.split('. ')[0]
    pieces = split_text(line, max_chars=len(line) // 2 + 4)
    assert [k for _, k in pieces] == ['forced', 'end']
    out, rows = m.tts_long(line, denoise=0, max_chars=len(line) // 2 + 4, return_segments=True)
    assert [(r['text'], r['boundary']) for r in rows] == pieces and bool(torch.isfinite(out).all())
    assert rows[1]['start'] == rows[0]['end'] - F_FADE and out.numel() == rows[1]['end']       # overlap of the fade's length
    seam = out[rows[1]['start'] - 64:rows[0]['end'] + 64]
    zero = (seam == 0).to(torch.int8)
    assert int((zero[1:] * zero[:-1]).sum()) == 0                                               # no run of zeros across the seam
    # pauses override: a forced boundary with a pause of its own
    out_p, rows_p = m.tts_long(line, denoise=0, max_chars=len(line) // 2 + 4, pauses={'forced': 20.0}, return_segments=True)
    assert rows_p[1]['start'] == rows_p[0]['end'] + 441 and not bool(out_p[rows_p[0]['end']:rows_p[1]['start']].any())


def test_tacotron2_tts_long(dev, synth_weights, tmp_path):
    import text
    from models.tacotron2 import Tacotron2Wave
    from text import split_text
    from ttsamd.config import HIFIGAN_CONFIG, TACOTRON2_CONFIG
    from ttsamd.synth import tacotron2_state_dict
    sd = tacotron2_state_dict(dict(TACOTRON2_CONFIG, num_speakers=40), seed=4, gate_bias=-0.5)
    torch.save({'model': {k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd.items()}, 'symbols': list(text.symbols)}, tmp_path / 'taco.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, tmp_path / 'hg.pth')
    with open(tmp_path / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    m = Tacotron2Wave(str(tmp_path / 'taco.pth'), str(tmp_path / 'hg.pth'), str(tmp_path / 'config.json'), n_symbol=len(text.symbols)).to(dev)
    m.model.decoder_max_step = 40
    m.model.dropout_seed = 5
    para = 'اَلسَّلامُ عَلَيكُم يَا صَدِيقِي. كِتَاب'
    out, rows = m.tts_long(para, denoise=0, return_segments=True)
    pieces = split_text(para)
    assert [k for _, k in pieces] == ['sentence', 'end']
    assert out.dim() == 1 and out.device.type == 'cpu' and bool(torch.isfinite(out).all())
    assert _check_table(out, rows, pieces) == out.numel()
    assert torch.equal(m.tts_long(para, denoise=0), out)
    with pytest.raises(ValueError):
        m.tts_long('  ')


def test_inference_cli_long(model, tmp_path):
    """inference.py --long: one wav per list line, every line a paragraph"""
    import inference
    from scipy.io import wavfile
    _, d = model
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        every = json.load(f)
    lst = tmp_path / 'lines.txt'
    lst.write_text(f'{every[9]}. {every[14]}\n{every[63]}\n{every[35]}، {every[68]}? {every[92]}\n', encoding='utf-8')
    inference.main(['--list', str(lst), '--model', 'fastpitch', '--checkpoint', str(d / 'fp.pth'), '--vocoder_sd', str(d / 'hg.pth'),
                    '--vocoder_config', str(d / 'config.json'), '--out_dir', str(tmp_path / 'out'), '--long'])
    sizes = []
    for i in range(3):
        sr, data = wavfile.read(tmp_path / 'out' / 'wavs' / f'static{i}.wav')
        assert sr == 22050 and data.dtype == np.int16 and data.size > 0
        sizes.append(data.size)
    assert not (tmp_path / 'out' / 'wavs' / 'static3.wav').exists()
    assert len((tmp_path / 'out' / 'index.tsv').read_text(encoding='utf-8').splitlines()) == 3
    first = lst.read_text(encoding='utf-8').splitlines()[0]
    assert sizes[0] == model[0].tts_long(first, denoise=0, speed=1.0).numel()                  # the file is tts_long of its line

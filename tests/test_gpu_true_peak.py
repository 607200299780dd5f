"""True peak on the GPU (pytest -m gpu): ttsamd_true_peak and ttsamd_wave_limit_true_peak against the numpy restatement
tests/true_peak_ref.py BIT FOR BIT (float64 chains over fp32 values: a product is exact, so fma and multiply-then-add agree), and the
`true_peak=` switch of the levelling calls, the limiter, the tts wrappers and the stream.

Sizes: a ragged batch of 7 rows in a stride of 8 200 with lengths 0, 1, 13 (the detector's reach), 2 047, 2 048, 2 049 (the tile of
both kernels and of the limiter's second launch, +- 1) and 8 195 (four tiles and a tail that is no multiple of four samples)."""
import ctypes as C

import numpy as np
import pytest
import torch

import limiter_ref as LR
import true_peak_ref as T
from test_gpu_limiter import SV_KW, _gains_for, _mel, _stream_run, dev, lines, model, v1      # noqa: F401  (helpers and fixtures)
from test_gpu_tacotron2 import LINES as TACO_LINES, taco_ckpt                                   # noqa: F401

pytestmark = pytest.mark.gpu

EINVAL = -1
Q = LR.Q
STRIDE = 8200
LENS = [0, 1, 13, 2047, 2048, 2049, 8195]
SINE = 4                                # the row that is a sine at fs / 4 with 45 degrees of phase: every peak lies between two samples
CEIL = np.float32(0.99)


def _rows():
    rng = np.random.default_rng(2024)
    xs = [rng.uniform(-0.9, 0.9, n).astype(np.float32) for n in LENS]
    xs[SINE] = (0.9 * np.sin(2 * np.pi * np.arange(LENS[SINE]) / 4 + np.pi / 4)).astype(np.float32)
    return xs


@pytest.fixture(scope='module')
def rows():
    return _rows()


@pytest.fixture(scope='module')
def eng(dev):
    from ttsamd.engine import leveller
    return leveller(22050, dev)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poisoned(xs, dev, stride=STRIDE):
    buf = np.full((len(xs), stride), np.nan, dtype=np.float32)
    for b, x in enumerate(xs):
        buf[b, :len(x)] = x
    return torch.from_numpy(buf).to(dev), torch.tensor([len(x) for x in xs], dtype=torch.int64, device=dev)


@pytest.fixture(scope='module')
def ref_tp(rows):
    return np.array([T.true_peak(x) for x in rows], dtype=np.float32)


def test_true_peak_is_the_restatement_bit_for_bit(eng, dev, rows, ref_tp):
    from utils import audio
    wave, lens = _poisoned(rows, dev)
    got = eng.true_peak(wave, lens).cpu().numpy()
    print('true peak per row:', got.tolist(), 'sample peaks:', [float(np.abs(x).max()) if len(x) else 0.0 for x in rows])
    assert got.dtype == np.float32 and np.array_equal(LR.bits(got), LR.bits(ref_tp))
    assert ref_tp[0] == 0.0 and ref_tp[SINE] > 1.3 * np.abs(rows[SINE]).max() and all(ref_tp[b] >= np.abs(x).max() for b, x in enumerate(rows) if len(x))
    for b, x in enumerate(rows):                                         # rows as if alone
        one = eng.true_peak(torch.from_numpy(x).to(dev)[None].contiguous() if len(x) else torch.zeros(1, 0, device=dev)).cpu().numpy()
        assert np.array_equal(LR.bits(one), LR.bits(ref_tp[b:b + 1])), b
    # a stride that is no multiple of four samples (rows off the 16-byte grid), and the public helpers
    odd, olens = _poisoned(rows[3:6], dev, stride=2051)
    assert np.array_equal(LR.bits(eng.true_peak(odd, olens).cpu().numpy()), LR.bits(ref_tp[3:6]))
    assert np.array_equal(LR.bits(audio.true_peak(wave, lens).cpu().numpy()), LR.bits(ref_tp))
    db = audio.true_peak_db(wave, lens).cpu().numpy()
    assert db.dtype == np.float64 and db[0] == -np.inf and np.allclose(db[1:], 20 * np.log10(ref_tp[1:].astype(np.float64)), rtol=0, atol=1e-12)
    assert float(audio.true_peak(torch.zeros(3, 500, device=dev)).abs().max()) == 0.0


def _limit(eng, xs, A, Rh, gains_db, true_peak=True, c=CEIL):
    wave, lens = _poisoned(xs, eng.device)
    B = len(xs)
    mode = torch.full((B,), 3, dtype=torch.int32, device=eng.device)
    target = torch.tensor(list(gains_db), dtype=torch.float32).to(eng.device)
    out, gain, red = eng.limit_samples(wave, lens, mode, target, float(c), 1e6, A, Rh, **(dict(true_peak=True) if true_peak else {}))
    out = out.cpu().numpy()
    assert np.isnan(np.concatenate([out[b, len(x):] for b, x in enumerate(xs)])).all()          # nothing behind a row was written
    return [out[b, :len(x)] for b, x in enumerate(xs)], gain.cpu().numpy(), red.cpu().numpy()


# measured with the float64 restatement alone on the rows above (A = 33, R = 331, the gain below): max TP(y) / c - 1 = 0.00089 (the
# row of 8 195; 0.00076 and 0.00028 on the other noise rows, 0 on the sine; the sample-peak detector leaves 0.56 .. 0.73 there).  The
# assertion below allows twice that.  With A = 0 the gain steps from sample to sample and the same rows overshoot by up to 0.27.
OVERSHOOT = 0.00089


@pytest.mark.parametrize('A,Rh', [(33, 331), (0, 0)])
def test_limiter_with_the_true_peak_detector_is_the_restatement_bit_for_bit(eng, rows, A, Rh):
    db = 20 * np.log10(0.99 / 0.81)            # |u| > c on a tenth of the uniform +-0.9 noise samples
    ys, gain, red = _limit(eng, rows, A, Rh, [db] * len(rows))
    g64 = LR.row_gain(3, db, 1e6)
    worst = 0.0
    for b, x in enumerate(rows):
        assert gain[b] == np.float32(g64) or abs(float(gain[b]) / g64 - 1) < 1.2e-7
        r = T.curves(x, gain[b], CEIL, A, Rh)
        assert np.array_equal(LR.bits(ys[b]), LR.bits(r['y'])), (b, len(x), np.flatnonzero(LR.bits(ys[b]) != LR.bits(r['y']))[:8])
        assert int(red[b]) == (int(r['s'].min()) if len(x) else Q), b
        if len(x):
            assert np.abs(ys[b]).max() <= CEIL
            share = float((np.abs(r['u']) > CEIL).mean())
            worst = max(worst, T.true_peak64(ys[b]) / float(CEIL) - 1.0)
            if len(x) > 2000 and b != SINE:
                assert 0.07 < share < 0.13 and int(red[b]) < Q, (b, share)
    print(f'A {A}, R {Rh}: largest true-peak overshoot of the limited rows {worst:.4f} of the ceiling')
    if A == 33:
        assert worst <= 2 * OVERSHOOT
    # rows alone have the batch's bits
    for b in (2, 5):
        y1, g1, r1 = _limit(eng, [rows[b]], A, Rh, [db])
        assert g1[0] == gain[b] and r1[0] == red[b] and np.array_equal(LR.bits(y1[0]), LR.bits(ys[b]))
    # the sample-peak detector is another curve on these rows: the switch does something
    y0, _, red0 = _limit(eng, rows, A, Rh, [db] * len(rows), true_peak=False)
    assert int(red0[SINE]) == Q and int(red[SINE]) < Q                   # the sine's samples stay under the ceiling, its true peak does not
    assert not np.array_equal(LR.bits(y0[6]), LR.bits(ys[6]))
    assert np.array_equal(LR.bits(y0[6]), LR.bits(LR.limit(rows[6], gain[6], CEIL, A, Rh)[0]))


def test_limiter_far_below_the_ceiling_is_the_plain_product(eng, rows):
    ys, gain, red = _limit(eng, rows, 33, 331, [-20.0] * len(rows))
    for b, x in enumerate(rows):
        assert int(red[b]) == Q and np.array_equal(LR.bits(ys[b]), LR.bits(x * gain[b])), b


def test_levelling_to_a_true_peak_ceiling(eng, dev, rows):
    from utils import audio
    xs = rows[3:]
    wave, lens = _poisoned(xs, dev)
    bound = T.level_bound(CEIL)
    out = audio.normalize_loudness(wave, target_lufs=6.0, lens=lens, true_peak=True)          # a target the cap stops short of
    old = audio.normalize_loudness(wave, target_lufs=6.0, lens=lens)
    for b, x in enumerate(xs):
        y, y_old = out[b, :len(x)].cpu().numpy(), old[b, :len(x)].cpu().numpy()
        tp, tp_old = T.true_peak64(y), T.true_peak64(y_old)
        print(f'row of {len(x)}: true peak {tp:.9f} (bound {bound:.9f}), sample peak {np.abs(y).max():.6f}; without true_peak {tp_old:.6f} / '
              f'{np.abs(y_old).max():.6f}')
        assert 0.98 < tp <= bound and np.abs(y_old).max() <= CEIL < tp_old
        assert torch.equal(out[b, len(x):].isnan(), torch.ones_like(out[b, len(x):], dtype=torch.bool))
    sine = out[SINE - 3, :LENS[SINE]].cpu().numpy()
    # its sample peak: 3 dB under the ceiling (3.01 dB for the endless sine; the row starts and ends abruptly, and the interpolator
    # overshoots by 1.2 % at those edges: TP 0.9109 for an amplitude of 0.9, another 0.10 dB)
    assert abs(20 * np.log10(np.abs(sine).max() / float(CEIL)) + 3.115) < 0.01
    assert T.true_peak64(old[SINE - 3, :LENS[SINE]].cpu().numpy()) > 1.25                      # what true_peak=False leaves behind
    got_tp = audio.true_peak(out, lens).cpu().numpy()
    assert (got_tp <= np.float32(bound)).all() or (got_tp.astype(np.float64) <= bound * (1 + 2.0 ** -23)).all()
    # peak mode on every row of the batch, the short ones included
    wave, lens = _poisoned(rows, dev)
    pk = audio.peak_normalize(wave, lens=lens, true_peak=True)
    for b, x in enumerate(rows):
        if len(x):
            tp = T.true_peak64(pk[b, :len(x)].cpu().numpy())
            assert 0.99 * (1 - 1e-6) < tp <= bound, (b, tp)
    lim = audio.normalize_loudness(wave[3:], target_lufs=6.0, lens=lens[3:], limiter=True, true_peak=True)
    want, _, _ = eng.limit(wave[3:].clone(), lens[3:], 2, 6.0, true_peak=True)
    assert torch.equal(lim.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(lim.view(torch.int32), audio.normalize_loudness(wave[3:], target_lufs=6.0, lens=lens[3:], limiter=True).view(torch.int32))


def test_stream_chunks_are_the_whole_wave_limited(v1):
    from ttsamd.stream import StreamingVocoder
    from utils import audio
    mels = [_mel(80, 40, 140), _mel(80, 14, 114)]
    kw = dict(SV_KW, chunk_frames=8)
    sv = StreamingVocoder(v1[0], v1[1], limiter=dict(max_gain_db=120.0), true_peak=True, **kw)
    assert (sv._lim_lb, sv._lim_la) == (33 + 331 + 13, 66 + 13)
    sv.bypass = True
    plain, _, _ = _stream_run(sv, mels, [0.0, 0.01], [0.0, 0.0])
    plain = [torch.cat(plain[i]) for i in range(2)]
    gains = _gains_for(plain)
    sv.bypass = False
    got, _, red_min = _stream_run(sv, mels, [0.0, 0.01], gains)
    assert red_min < Q
    for i, u in enumerate(plain):
        want, red_db = audio.limit(u.to(sv.device), gain_db=gains[i], true_peak=True)
        y = torch.cat(got[i])
        assert float(red_db[0]) < 0.0 and y.shape == u.shape and len(got[i]) > 1
        assert torch.equal(y.view(torch.int32), want.cpu().view(torch.int32)), (i, int((y != want.cpu()).sum()))
        other, _ = audio.limit(u.to(sv.device), gain_db=gains[i])
        assert not torch.equal(other.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError):
        StreamingVocoder(v1[0], v1[1], true_peak=True, **kw)


def test_true_peak_false_is_the_call_without_it(eng, dev, rows, v1):
    from ttsamd.engine import level_waves
    from ttsamd.stream import StreamingVocoder
    from utils import audio
    wave, lens = _poisoned(rows, dev)

    def same(a, b):
        a, b = (a[0] if isinstance(a, tuple) else a), (b[0] if isinstance(b, tuple) else b)
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(audio.peak_normalize(wave, lens=lens, true_peak=False), audio.peak_normalize(wave, lens=lens))
    assert same(audio.normalize_loudness(wave, lens=lens, target_lufs=6.0, true_peak=False), audio.normalize_loudness(wave, lens=lens, target_lufs=6.0))
    assert same(audio.normalize_loudness(wave, lens=lens, target_lufs=6.0, limiter=True, true_peak=False),
                audio.normalize_loudness(wave, lens=lens, target_lufs=6.0, limiter=True))
    assert same(audio.limit(wave, gain_db=3.0, lens=lens, true_peak=False), audio.limit(wave, gain_db=3.0, lens=lens))
    assert same(eng.level(wave.clone(), lens, 2, 6.0, true_peak=False), eng.level(wave.clone(), lens, 2, 6.0))
    assert same(eng.limit(wave.clone(), lens, 3, 3.0, true_peak=False), eng.limit(wave.clone(), lens, 3, 3.0))
    opts = ['peak', None, -3.0, 'lufs', -3.0, 'peak', -3.0]
    assert same(level_waves(wave.clone(), lens, opts, limiter=True, true_peak=False), level_waves(wave.clone(), lens, opts, limiter=True))
    a, b = StreamingVocoder(v1[0], v1[1], limiter=True, true_peak=False, **SV_KW), StreamingVocoder(v1[0], v1[1], limiter=True, **SV_KW)
    assert (a._lim_lb, a._lim_la, a._lim_halo, a._w_cap, a._lim_tp) == (b._lim_lb, b._lim_la, b._lim_halo, b._w_cap, False)
    with pytest.raises(ValueError):
        level_waves(wave.clone(), lens, None, true_peak=True)


def test_tts_takes_true_peak(model, lines, eng):
    two = lines[:2]
    plain = model.tts(two, batch_size=2)
    assert all(torch.equal(a, b) for a, b in zip(model.tts(two, batch_size=2, normalize=-3.0, limiter=True, true_peak=False),
                                                 model.tts(two, batch_size=2, normalize=-3.0, limiter=True)))
    for kw in (dict(normalize=-3.0, limiter=True), dict(normalize='peak'), dict(normalize=[-3.0, None])):
        for bs in (1, 2):
            waves = model.tts(two, batch_size=bs, true_peak=True, **kw)
            base = plain if bs == 2 else model.tts(two, batch_size=1)
            for i, (w, p) in enumerate(zip(waves, base)):
                row = p.to(model.device)[None].contiguous()
                opt = kw['normalize'][i] if isinstance(kw['normalize'], list) else kw['normalize']
                if opt is None:
                    want = row
                elif kw.get('limiter'):
                    want = eng.limit(row, None, 2, opt, true_peak=True)[0]
                else:
                    want = eng.level(row, None, 1 if opt == 'peak' else 2, 0.99 if opt == 'peak' else opt, true_peak=True)[0]
                assert torch.equal(w.view(torch.int32), want[0].cpu().view(torch.int32)), (kw, bs, i)
    one = model.tts(two[0], normalize='peak', true_peak=True)
    assert float(eng.true_peak(one.to(model.device)[None])[0]) <= np.float32(T.level_bound(CEIL)) and float(one.abs().max()) < 0.99
    for call in (lambda: model.tts(two, true_peak=True), lambda: model.tts(two[0], true_peak=True),
                 lambda: model.tts_requests([dict(text=two[0])], true_peak=True), lambda: list(model.tts_stream(two[0], true_peak=True)),
                 lambda: model.tts(two, normalize=[None, None], true_peak=True)):
        with pytest.raises(ValueError):
            call()
    sv_kw = dict(chunk_frames=16, first_chunk_frames=8, denoise=0.0, limiter=dict(max_gain_db=120.0), true_peak=True)
    list(model.tts_stream(two[0], **sv_kw))                              # makes the model's streamer for these settings
    assert model._stream_voc._lim_tp
    model._stream_voc.bypass = True
    u = torch.cat(list(model.tts_stream(two[0], **sv_kw)))
    model._stream_voc.bypass = False
    g = _gains_for([u])[0]
    y = torch.cat(list(model.tts_stream(two[0], gain_db=g, **sv_kw)))
    from utils import audio
    assert torch.equal(y.view(torch.int32), audio.limit(u.to(model.device), gain_db=g, true_peak=True)[0].cpu().view(torch.int32))


def test_tacotron2_takes_true_peak(taco_ckpt, dev, eng):
    import text
    from models.tacotron2 import Tacotron2Wave
    taco = Tacotron2Wave(taco_ckpt[0], taco_ckpt[1], taco_ckpt[2], n_symbol=len(text.symbols)).to(dev)
    taco.model.decoder_max_step = 40
    taco.model.dropout_seed = -1                               # prenet dropout off: two calls give the same wave
    two = TACO_LINES[1:3]
    plain = taco.tts(two, batch_size=2, denoise=0)
    for kw in (dict(normalize='peak'), dict(normalize=-3.0, limiter=True)):
        waves = taco.tts(two, batch_size=2, denoise=0, true_peak=True, **kw)
        for w, p in zip(waves, plain):
            row = p.to(dev)[None].contiguous()
            want = eng.limit(row, None, 2, -3.0, true_peak=True)[0] if 'limiter' in kw else eng.level(row, None, 1, 0.99, true_peak=True)[0]
            assert torch.equal(w.view(torch.int32), want[0].cpu().view(torch.int32)), kw
        assert all(torch.equal(a, b) for a, b in zip(taco.tts(two, batch_size=2, denoise=0, true_peak=False, **kw), taco.tts(two, batch_size=2, denoise=0, **kw)))
    one = taco.tts(two[0], denoise=0, normalize='peak', true_peak=True)
    assert float(eng.true_peak(one.to(dev)[None])[0]) <= np.float32(T.level_bound(CEIL))
    for call in (lambda: taco.tts(two, true_peak=True), lambda: taco.tts(two[0], true_peak=True), lambda: taco.tts_batch(two, true_peak=True)):
        with pytest.raises(ValueError):
            call()


def test_refusals(eng, dev, rows):
    from ttsamd import lib
    h = lib.load()
    wave, lens = _poisoned(rows, dev)
    before = wave.clone()
    B = len(rows)
    out = torch.full((B,), 7.0, dtype=torch.float32, device=dev)

    def tp(wave_=wave, lens_=lens, B_=B, out_=out, stride=STRIDE):
        return h.ttsamd_true_peak(_ptr(wave_), stride, _ptr(lens_), B_, _ptr(out_), _stream())
    for kw in (dict(wave_=None), dict(lens_=None), dict(out_=None), dict(B_=0), dict(B_=-1), dict(B_=65536), dict(stride=-1), dict(stride=1 << 40)):
        assert tp(**kw) == EINVAL, kw
        assert b'true_peak' in h.ttsamd_last_error()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0] * B                               # nothing was launched, the result not even zeroed
    mode = torch.full((B,), 3, dtype=torch.int32, device=dev)
    target = torch.full((B,), 6.0, dtype=torch.float32, device=dev)
    gain = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    red = torch.full((B,), 7, dtype=torch.int32, device=dev)
    nb = h.ttsamd_wave_limit_workspace_bytes(B, STRIDE)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def lim(wave_=wave, lens_=lens, B_=B, mode_=mode, target_=target, c=0.99, mg=31.6, A=33, Rh=331, gain_=gain, red_=red, ws_=ws, nb_=nb):
        return h.ttsamd_wave_limit_true_peak(_ptr(wave_), STRIDE, _ptr(lens_), B_, _ptr(mode_), _ptr(target_), c, mg, A, Rh, None, _ptr(gain_),
                                             _ptr(red_), _ptr(ws_), nb_, _stream())
    for kw in (dict(wave_=None), dict(lens_=None), dict(mode_=None), dict(target_=None), dict(gain_=None), dict(red_=None), dict(ws_=None),
               dict(B_=0), dict(B_=65536), dict(c=0.0), dict(c=1.5), dict(c=float('nan')), dict(mg=0.0), dict(mg=float('inf')), dict(A=-1),
               dict(A=332), dict(A=1025, Rh=1025), dict(Rh=4097), dict(nb_=nb - 1)):
        assert lim(**kw) == EINVAL, kw
        assert b'wave_limit' in h.ttsamd_last_error()
    torch.cuda.synchronize()
    assert gain.cpu().tolist() == [7.0] * B and red.cpu().tolist() == [7] * B and torch.equal(wave.view(torch.int32), before.view(torch.int32))
    assert lim(A=1024, Rh=4096) == 0 and float(wave[6, :8195].abs().max()) <= 0.99

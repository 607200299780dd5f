"""Mixed requests in one batch (pytest -m gpu): per-row speaker, pace, pitch_mul / pitch_add and denoise strength through
ttsamd_fastpitch_encode_rows / _decode_rows, ttsamd_denoise_rows, ttsamd_vocos_forward_rows and the wrappers above them.

The yardstick is the scalar entry: the row arrays reach the kernels the scalars reach, in the same expressions, so row b of a mixed call
has the BITS of the scalar call on the same batch with row b's values.  Against the oracle and the one-by-one calls the tolerances are
the ones the existing tests use for the same comparisons (conftest.MEL_TOL / WAVE_TOL; tests/test_gpu_alone.py: 2e-5 / 5e-4).

Fixture: five rows of 7, 1, 12, 4 and 9 tokens (unsorted on purpose) on the four-speaker synthetic FastPitch; dur_tgt holds small
integers chosen so that dur / pace + 0.5 lands ON an integer for some (2 / 0.8 + 0.5 = 3, 3 / 2 + 0.5 = 2, 5 / 1.25 + 0.5 = 4.5 ...)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, MEL_TOL, WAVE_TOL

pytestmark = pytest.mark.gpu

LENS = [7, 1, 12, 4, 9]
SPEAKERS = [2, 0, 3, 1, 2]
PACES = [0.8, 1.0, 1.25, 1.0, 2.0]
PITCH_MUL = [1.0, 0.5, 1.5, 0.9, 1.2]
PITCH_ADD = [0.0, 0.3, -0.2, 0.1, -0.5]
PRECISIONS = [('f32', 2e-5), ('bf16x3', 5e-4)]          # ... and the one-by-one tolerances of tests/test_gpu_alone.py


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cfg4():
    from ttsamd.config import NET_CONFIG
    return dict(NET_CONFIG, n_speakers=4)


@pytest.fixture(scope='module')
def batch():
    """ids int64 [5, 12] zero-padded at the end, dur_tgt float32 [5, 12] (zero on the padding)"""
    from ttsamd import synth
    ids = synth.synth_ids(5, 12, seed=77)
    ids[ids == 0] = 1
    dur = np.array([[2, 3, 5, 1, 0, 4, 2, 0, 0, 0, 0, 0],
                    [3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                    [5, 1, 2, 3, 4, 5, 6, 1, 2, 7, 3, 5],
                    [1, 2, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0],
                    [3, 1, 5, 2, 7, 3, 1, 4, 3, 0, 0, 0]], np.float32)
    for b, n in enumerate(LENS):
        ids[b, n:] = 0
        assert not dur[b, n:].any()
    return ids, dur


@pytest.fixture
def precision():
    from ttsamd import engine as E

    def use(name):
        E.set_precision(name)
    yield use
    E.set_precision('f32')


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _fp_call(eng, ids, dur_tgt=None, speaker=0, pace=1.0, mul=1.0, add=0.0, rows=None, flags=None, decode=False):
    """One FastPitch call straight through the C ABI.  flags None: the scalar entries (ttsamd_fastpitch_encode / _decode); otherwise
    the _rows entries with `flags` and the device arrays of `rows` (a dict with any of speaker, pace, mul, add).  -> dict of outputs."""
    from ttsamd import lib as L
    lib, dev = eng.lib, eng.device
    ids = torch.as_tensor(ids).to(dev).contiguous()
    B, Lt = ids.shape
    d = eng.d_model
    dur_tgt = None if dur_tgt is None else torch.as_tensor(dur_tgt).to(dev).float().contiguous()
    o = dict(enc_cond=torch.empty(B, d, Lt, device=dev), dur_pred=torch.empty(B, Lt, device=dev), pitch_pred=torch.empty(B, 1, Lt, device=dev),
             energy_pred=torch.empty(B, Lt, device=dev) if eng.config['energy_conditioning'] else None,
             reps=torch.empty(B, Lt, dtype=torch.int64, device=dev), dec_lens=torch.empty(B, dtype=torch.int64, device=dev))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = lib.ttsamd_fastpitch_encode_workspace_bytes(eng.handle, B, Lt)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    args = (eng.handle, _ptr(ids), B, Lt, int(speaker), float(pace), _ptr(dur_tgt), None, None, float(mul), float(add), 75.0,
            _ptr(o['enc_cond']), _ptr(o['dur_pred']), _ptr(o['pitch_pred']), _ptr(o['energy_pred']), _ptr(o['reps']), _ptr(o['dec_lens']),
            _ptr(ws), nb)
    if flags is None:
        L.check(lib.ttsamd_fastpitch_encode(*args, stream), 'encode')
    else:
        rows = rows or {}
        r = {k: None if rows.get(k) is None else torch.tensor(rows[k], dtype=torch.int32 if k == 'speaker' else torch.float32).to(dev)
             for k in ('speaker', 'pace', 'mul', 'add')}
        L.check(lib.ttsamd_fastpitch_encode_rows(*args, _ptr(r['speaker']), _ptr(r['pace']), _ptr(r['mul']), _ptr(r['add']), int(flags),
                                                 stream), 'encode_rows')
    if decode:
        t0 = int(o['dec_lens'].max())
        T = (t0 + 3) & ~3 if B >= 2 else t0
        x = torch.empty(B, d, T, device=dev)
        mel = torch.empty(B, eng.n_mel, T, device=dev)
        L.check(lib.ttsamd_length_regulate(_ptr(o['enc_cond']), _ptr(o['reps']), B, Lt, d, T, _ptr(x), None, stream), 'regulate')
        nb = lib.ttsamd_fastpitch_decode_workspace_bytes(eng.handle, B, T)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        args = (eng.handle, _ptr(x), _ptr(o['dec_lens']), B, T, _ptr(mel), _ptr(ws), nb)
        if flags is None:
            L.check(lib.ttsamd_fastpitch_decode(*args, stream), 'decode')
        else:
            L.check(lib.ttsamd_fastpitch_decode_rows(*args, int(flags), stream), 'decode_rows')
        o['mel'] = mel[:, :, :t0]
    torch.cuda.synchronize()
    return o


def _set_mode(eng, mode):
    assert eng.lib.ttsamd_fastpitch_set_batch_mode(eng.handle, mode) == 0
    eng._alone = bool(mode)


ENC_OUT = ('enc_cond', 'dur_pred', 'pitch_pred', 'energy_pred', 'reps', 'dec_lens')


@pytest.mark.parametrize('B,with_dur', [(1, False), (3, False), (5, False), (5, True)])
@pytest.mark.parametrize('prec', ['f32', 'bf16x3'])
def test_encode_rows_row_b_has_the_bits_of_the_scalar_call(dev, cfg4, synth_weights, batch, precision, prec, B, with_dur):
    """encode_rows with mixed speakers, paces, pitch_mul and pitch_add: every output's row b equals, bit for bit, row b of
    ttsamd_fastpitch_encode on the same ids with row b's values as scalars -- under both values of the flag (the scalar call then runs
    with the handle switched to that mode).  B = 1 and 3 sit on the two sides of the small-batch fp32 switch of the split-bf16 mode."""
    from ttsamd.engine import FastPitchEngine
    precision(prec)
    ids, dur = batch[0][:B], (batch[1][:B] if with_dur else None)
    eng = FastPitchEngine(synth_weights['fastpitch_spk4'], cfg4, device=dev)
    rows = dict(speaker=SPEAKERS[:B], pace=PACES[:B], mul=PITCH_MUL[:B], add=PITCH_ADD[:B])
    try:
        for flag in (0, 1):
            _set_mode(eng, 1 - flag)                    # the rows entry must not look at the handle: set it to the OTHER mode
            got = _fp_call(eng, ids, dur, rows=rows, flags=flag)
            _set_mode(eng, flag)
            for b in range(B):
                ref = _fp_call(eng, ids, dur, speaker=SPEAKERS[b], pace=PACES[b], mul=PITCH_MUL[b], add=PITCH_ADD[b])
                for k in ENC_OUT:
                    if got[k] is not None:
                        assert torch.equal(got[k][b], ref[k][b]), (prec, B, flag, b, k)
            assert bool(torch.isfinite(got['enc_cond']).all())
        if B > 1:                                       # the controls did something: rows with different speakers / pitch differ from a uniform call
            uni = _fp_call(eng, ids, dur, speaker=SPEAKERS[0], pace=PACES[0], mul=PITCH_MUL[0], add=PITCH_ADD[0])
            assert not torch.equal(got['enc_cond'][1], uni['enc_cond'][1]) and not torch.equal(got['pitch_pred'][1], uni['pitch_pred'][1])
    finally:
        _set_mode(eng, 0)


@pytest.mark.parametrize('prec', ['f32', 'bf16x3'])
def test_uniform_arrays_equal_the_scalar_entries_through_the_decoder(dev, cfg4, synth_weights, golden, precision, prec):
    """Arrays [2, 2, 2] / [1, 1, 1] / [0, 0, 0] on the fastpitch_b3_spk2 golden: the mel of the _rows entries equals the scalar entries'
    bit for bit and reproduces the reference golden within the tolerance of test_fastpitch_multispeaker_golden."""
    from ttsamd.engine import FastPitchEngine
    precision(prec)
    g = golden('fastpitch_b3_spk2')
    eng = FastPitchEngine(synth_weights['fastpitch_spk4'], cfg4, device=dev)
    mel_s, lens_s, dur_s, pitch_s, _ = eng.infer(g['ids'], dur_tgt=g['dur_tgt'], speaker=2)
    mel_r, lens_r, dur_r, pitch_r, _ = eng.infer(g['ids'], dur_tgt=g['dur_tgt'], speaker=[2, 2, 2], pace=[1.0] * 3, pitch_mul=[1.0] * 3,
                                                 pitch_add=np.zeros(3, np.float32))
    assert torch.equal(lens_r, lens_s) and torch.equal(dur_r, dur_s) and torch.equal(pitch_r, pitch_s) and torch.equal(mel_r, mel_s)
    assert np.array_equal(lens_r.cpu().numpy(), g['dec_lens'])
    err = float((mel_r.cpu() - torch.from_numpy(g['mel'])).abs().max())
    print(f'{prec}: uniform arrays vs the reference golden, mel max-abs {err:.2e} (tol {MEL_TOL})')
    assert err < MEL_TOL
    # one array is enough to take the _rows route; the others stay scalars
    mel_1, *_ = eng.infer(g['ids'], dur_tgt=g['dur_tgt'], speaker=torch.tensor([2, 2, 2]))
    assert torch.equal(mel_1, mel_s)


@pytest.mark.parametrize('B', [3, 5])
@pytest.mark.parametrize('prec', ['f32', 'bf16x3'])
def test_padded_mode_mel_row_b_has_the_bits_of_the_scalar_call(dev, cfg4, synth_weights, batch, precision, prec, B):
    """With dur_tgt given and one pace, dec_lens does not depend on the controls, so the decoder sees the same padded batch in every call:
    mel row b of the call with mixed speakers and pitch values equals, bit for bit, row b of the scalar call with row b's values."""
    from ttsamd.engine import FastPitchEngine
    precision(prec)
    ids, dur = batch[0][:B], batch[1][:B]
    eng = FastPitchEngine(synth_weights['fastpitch_spk4'], cfg4, device=dev)
    got = _fp_call(eng, ids, dur, rows=dict(speaker=SPEAKERS[:B], mul=PITCH_MUL[:B], add=PITCH_ADD[:B]), flags=0, decode=True)
    want_lens = torch.from_numpy(dur.sum(1)).long()
    assert torch.equal(got['dec_lens'].cpu(), want_lens)
    for b in range(B):
        ref = _fp_call(eng, ids, dur, speaker=SPEAKERS[b], mul=PITCH_MUL[b], add=PITCH_ADD[b], decode=True)
        assert torch.equal(ref['dec_lens'].cpu(), want_lens)
        t = int(want_lens[b])
        assert torch.equal(got['mel'][b, :, :t], ref['mel'][b, :, :t]), (prec, B, b)
    assert not torch.equal(got['mel'][0, :, :int(want_lens[0])], ref['mel'][0, :, :int(want_lens[0])])      # ref: the LAST row's controls


@pytest.fixture(scope='module')
def oracle_rows(cfg4, synth_weights, batch):
    """tts_oracle.fastpitch_infer on each row alone with its own options: [(mel [80, t], t)], computed once for both precisions"""
    import tts_oracle as O
    W = O.to_torch(synth_weights['fastpitch_spk4'])
    ids, dur = batch
    out = []
    for b, n in enumerate(LENS):
        trf = (lambda m, a: (lambda p, *_: m * p + a))(PITCH_MUL[b], PITCH_ADD[b])
        mel, lens, *_ = O.fastpitch_infer(W, cfg4, ids[b:b + 1, :n], pace=PACES[b], dur_tgt=torch.from_numpy(dur[b:b + 1, :n]),
                                          pitch_transform=trf, speaker=SPEAKERS[b])
        out.append((mel[0], int(lens[0])))
    return out


@pytest.mark.parametrize('prec,tol', PRECISIONS)
def test_rows_alone_against_the_oracle_and_the_one_by_one_calls(dev, cfg4, synth_weights, batch, oracle_rows, precision, prec, tol):
    """Mixed paces, speakers and pitch values with flag bit 0 (FastPitchEngine.infer(alone=True) with per-row controls): each row against
    the oracle on that row alone with its own options (dec_lens exact, mel within MEL_TOL) and against the engine's own batch-of-one
    call (the tolerances of tests/test_gpu_alone.py)."""
    from ttsamd.engine import FastPitchEngine
    precision(prec)
    ids, dur = batch
    eng = FastPitchEngine(synth_weights['fastpitch_spk4'], cfg4, device=dev)
    mel, lens, _, pitch, _ = eng.infer(ids, dur_tgt=dur, pace=PACES, speaker=SPEAKERS, pitch_mul=PITCH_MUL, pitch_add=PITCH_ADD, alone=True)
    assert eng._alone is False                          # the flag went down with the call; the handle was not switched
    worst_o = worst_1 = 0.0
    for b, n in enumerate(LENS):
        ref, t = oracle_rows[b]
        assert int(lens[b]) == t, (b, int(lens[b]), t)
        worst_o = max(worst_o, float((mel[b, :, :t].cpu() - ref[:, :t]).abs().max()))
        mel_1, lens_1, _, pitch_1, _ = eng.infer(ids[b:b + 1, :n], dur_tgt=dur[b:b + 1, :n], pace=PACES[b], speaker=SPEAKERS[b],
                                                 pitch_mul=PITCH_MUL[b], pitch_add=PITCH_ADD[b])
        assert int(lens_1[0]) == t
        assert float((pitch[b, 0, :n] - pitch_1[0, 0, :n]).abs().max()) < tol
        worst_1 = max(worst_1, float((mel[b, :, :t] - mel_1[0, :, :t]).abs().max()))
    print(f'{prec}: rows alone, mixed controls: vs the oracle mel max-abs {worst_o:.2e} (tol {MEL_TOL}), vs one-by-one {worst_1:.2e} (tol {tol})')
    assert worst_o < MEL_TOL and worst_1 < tol


@pytest.mark.parametrize('prec,tol', PRECISIONS)
def test_batch_mode_1_with_pitch_add_through_the_scalar_entries(dev, cfg4, synth_weights, batch, precision, prec, tol):
    """The handle switch with a scalar pitch_add != 0 (FastPitchEngine.infer(alone=True), all controls scalars: ttsamd_fastpitch_encode /
    _decode under set_batch_mode 1): every row equals its batch-of-one call, as the mode's contract says.  The transformed pitch is 0 past
    a row's end in this mode; the padded-batch mode holds pitch_add there, as the reference's padded batch does, and so differs."""
    from ttsamd.engine import FastPitchEngine
    precision(prec)
    ids, dur = batch
    eng = FastPitchEngine(synth_weights['fastpitch_spk4'], cfg4, device=dev)
    kw = dict(speaker=1, pace=1.25, pitch_mul=0.9, pitch_add=0.4)
    mel, lens, _, pitch, _ = eng.infer(ids, dur_tgt=dur, alone=True, **kw)
    assert eng._alone is True                           # all scalars: the handle's switch, as before
    mel_p, lens_p, _, pitch_p, _ = eng.infer(ids, dur_tgt=dur, alone=False, **kw)
    worst = worst_p = 0.0
    for b, n in enumerate(LENS):
        mel_1, lens_1, _, pitch_1, _ = eng.infer(ids[b:b + 1, :n], dur_tgt=dur[b:b + 1, :n], **kw)
        t = int(lens_1[0])
        assert int(lens[b]) == t == int(lens_p[b])
        assert float((pitch[b, 0, :n] - pitch_1[0, 0, :n]).abs().max()) < tol
        assert not bool(pitch[b, 0, n:].any()) and bool((pitch_p[b, 0, n:] == 0.4).all())
        worst = max(worst, float((mel[b, :, :t] - mel_1[0, :, :t]).abs().max()))
        worst_p = max(worst_p, float((mel_p[b, :, :t] - mel_1[0, :, :t]).abs().max()))
    print(f'{prec}: batch mode 1, scalar pitch_add 0.4: vs one-by-one mel max-abs {worst:.2e} (tol {tol}); padded-batch mode {worst_p:.2e}')
    assert worst < tol


@pytest.mark.parametrize('prec', ['f32', 'bf16x3'])
def test_the_flag_is_per_call(dev, cfg4, synth_weights, batch, precision, prec):
    """On one handle, never touching set_batch_mode in between, calls with flags 1, 0, 1 each equal, bit for bit, the scalar entries under
    the handle switch in that mode -- and the handle's mode is what it was: the scalar entries still answer in it."""
    from ttsamd.engine import FastPitchEngine
    precision(prec)
    ids, dur = batch
    eng = FastPitchEngine(synth_weights['fastpitch_spk4'], cfg4, device=dev)
    uni = dict(speaker=[2] * 5, pace=[1.25] * 5, mul=[0.9] * 5, add=[0.1] * 5)
    sc = dict(speaker=2, pace=1.25, mul=0.9, add=0.1)
    ref = {}
    try:
        for mode in (1, 0):
            _set_mode(eng, mode)
            ref[mode] = _fp_call(eng, ids, dur, decode=True, **sc)
        assert not torch.equal(ref[0]['mel'], ref[1]['mel'])             # the two modes differ on this ragged batch
        for handle_mode in (0, 1):
            _set_mode(eng, handle_mode)
            for flag in (1, 0, 1):
                got = _fp_call(eng, ids, dur, rows=uni, flags=flag, decode=True)
                for k in ENC_OUT + ('mel',):
                    if got[k] is not None:
                        assert torch.equal(got[k], ref[flag][k]), (prec, handle_mode, flag, k)
            after = _fp_call(eng, ids, dur, decode=True, **sc)           # the handle's mode is unchanged
            assert torch.equal(after['mel'], ref[handle_mode]['mel'])
    finally:
        _set_mode(eng, 0)


def test_denoise_rows(dev):
    """A ragged batch with strengths [0.005, 0, 0.1, 0, 0.02]: a non-zero row has the bits of ttsamd_denoise with that scalar on the
    same batch, a zero row keeps its input bit for bit (the scalar entry at 0 would run it through STFT -> ISTFT, which is no identity)."""
    from ttsamd.engine import DenoiserEngine
    g = torch.Generator().manual_seed(11)
    ns = [4000, 1537, 5120, 700, 2600]
    strengths = [0.005, 0.0, 0.1, 0.0, 0.02]
    wave = (torch.randn(5, max(ns), generator=g) * 0.1).to(dev)
    bias = (torch.rand(1, 513, 1, generator=g) * 0.5).to(dev)
    n_dev = torch.tensor(ns).to(dev)
    eng = DenoiserEngine(device=dev)
    out = eng.denoise(wave.clone(), n_dev, bias, strengths)
    for b, s in enumerate(strengths):
        if s > 0:
            ref = eng.denoise(wave.clone(), n_dev, bias, s)
            assert torch.equal(out[b], ref[b]), b
            assert not torch.equal(out[b], wave[b])
        else:
            assert torch.equal(out[b], wave[b]), b
    zero = eng.denoise(wave.clone(), n_dev, bias, 0.0)
    assert not torch.equal(zero[1], wave[1])            # ... which is why a zero row is skipped rather than run at strength 0
    assert torch.equal(eng.denoise(wave.clone(), n_dev, bias, torch.zeros(5)), wave)


def test_denoiser_forward_batch_per_row(dev, model4):
    """The wrapper: Denoiser.forward_batch with a list has the engine's bits, and a row without denoising does not count for the length
    check (the reflect padding needs more than 512 samples) while a denoised one still does."""
    g = torch.Generator().manual_seed(12)
    strengths = [0.005, 0.0, 0.1, 0.0, 0.02]
    wave = (torch.randn(5, 5120, generator=g) * 0.1).to(dev)
    n_dev = torch.tensor([4000, 1537, 5120, 700, 2600]).to(dev)
    dn = model4.denoiser
    out = dn.forward_batch(wave.clone(), n_dev, strengths)
    for b, s in enumerate(strengths):
        assert torch.equal(out[b], dn.forward_batch(wave.clone(), n_dev, s)[b] if s > 0 else wave[b]), b
    short = torch.tensor([4000, 300, 5120, 700, 2600]).to(dev)
    assert torch.equal(dn.forward_batch(wave.clone(), short, strengths)[1], wave[1])
    with pytest.raises(ValueError):
        dn.forward_batch(wave.clone(), short, [0.005, 0.1, 0.1, 0.0, 0.02])
    assert torch.equal(dn.forward_batch(wave.clone(), n_dev, [0.0] * 5), wave)


def test_vocos_forward_rows(dev):
    """The same for Vocos: row b of a call with strengths [0.3, 0, 0.1, 0, 0.02] has the bits of ttsamd_vocos_forward on the same batch
    with that scalar (0: no subtraction at all)."""
    from ttsamd import synth
    from ttsamd.engine import VocosEngine
    rng = np.random.default_rng(17)
    lens = torch.tensor([29, 7, 16, 1, 22]).to(dev)
    strengths = [0.3, 0.0, 0.1, 0.0, 0.02]
    mel = torch.from_numpy((rng.standard_normal((5, 80, 29)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    voc = VocosEngine(synth.vocos_state_dict(), device=dev)
    out = voc.forward(mel, lens, strengths)
    refs = {s: voc.forward(mel, lens, s) for s in set(strengths)}
    for b, s in enumerate(strengths):
        assert torch.equal(out[b], refs[s][b]), b
    assert not torch.equal(refs[0.3][0], refs[0.0][0])
    from vocoder.vocos import MelVocos
    mv = MelVocos('22k')
    mv.load_state_dict({k: torch.from_numpy(v) for k, v in synth.vocos_state_dict().items()})
    assert torch.equal(mv.to(dev)(mel, denoise=strengths, lens=lens), out)


# ---- the wrappers ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def model4(tmp_path_factory, synth_weights, cfg4, dev):
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd.config import HIFIGAN_CONFIG
    d = tmp_path_factory.mktemp('ckpt4')
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['fastpitch_spk4'].items()}, 'config': dict(cfg4),
                'symbols': list(text.symbols)}, d / 'fp4.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    return FastPitch2Wave(str(d / 'fp4.pth'), vocoder_sd=str(d / 'hg.pth'), vocoder_config=str(d / 'config.json')).to(dev)


@pytest.fixture(scope='module')
def requests5():
    """five of the shortest committed infer_text lines (35 - 42 tokens), unsorted, each with its own options"""
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        lines = json.load(f)
    dn = [0.005, 0.0, 0.1, 0.0, 0.02]
    return [dict(text=lines[i], speed=PACES[k], speaker_id=SPEAKERS[k], pitch_mul=PITCH_MUL[k], pitch_add=PITCH_ADD[k], denoise=dn[k])
            for k, i in enumerate([68, 14, 92, 63, 35])]


@pytest.fixture(scope='module')
def singles(model4, requests5):
    return [model4.tts_single(r['text'], **{k: v for k, v in r.items() if k != 'text'}) for r in requests5]


def _lists(reqs):
    return {k: [r[k] for r in reqs] for k in ('speed', 'speaker_id', 'pitch_mul', 'pitch_add', 'denoise')}


@pytest.mark.parametrize('batch_size', [1, 2, 5])
def test_tts_with_per_line_lists(model4, requests5, singles, batch_size):
    """tts(lines, speed=[..], speaker_id=[..], pitch_mul=[..], pitch_add=[..], denoise=[..]): wave i has tts_single's length for request
    i and lies within WAVE_TOL of tts_single with request i's options -- through the pipelined list path (batch_size 1: the length-sorted
    alone groups; 2: chunks and the collate sort) and the single tts_batch call (5)."""
    waves = model4.tts([r['text'] for r in requests5], batch_size=batch_size, **_lists(requests5))
    assert len(waves) == 5
    errs = []
    for w, ref in zip(waves, singles):
        assert w.device.type == 'cpu' and w.shape == ref.shape, (w.shape, ref.shape)
        errs.append(float((w - ref).abs().max()))
    print(f'batch_size {batch_size}: wave max-abs against tts_single per request {["%.2e" % e for e in errs]} (tol {WAVE_TOL})')
    assert max(errs) < WAVE_TOL
    assert model4.tts_single(requests5[4]['text']).shape != singles[4].shape        # the options matter: speed 2 halves the frames


def test_lists_follow_their_lines_through_several_length_sorted_groups(model4, requests5, singles, monkeypatch):
    """batch_size = 1 with the pipeline's group size cut to 2: the five lines are sorted by length and go through FastPitch and the vocoder
    as three groups (2 + 2 + 1); every list takes the same sort, is cut into the same groups and the waves come back through order[] --
    wave i still answers request i, also for a permuted list."""
    monkeypatch.setattr(type(model4), '_ALONE_GROUP', 2)
    calls = []
    real = model4.model.ttmel_lines_alone
    monkeypatch.setattr(model4.model, 'ttmel_lines_alone', lambda lines, *a, **k: calls.append(len(lines)) or real(lines, *a, **k))
    for perm in ([0, 1, 2, 3, 4], [3, 0, 4, 2, 1]):
        calls.clear()
        reqs = [requests5[i] for i in perm]
        waves = model4.tts([r['text'] for r in reqs], batch_size=1, **_lists(reqs))
        assert calls == [2, 2], calls                   # two ragged calls of two lines; the fifth line goes alone through ttmel_single
        for k, i in enumerate(perm):
            assert waves[k].shape == singles[i].shape, (perm, k)
            assert float((waves[k] - singles[i]).abs().max()) < WAVE_TOL, (perm, k)


def test_tts_requests_and_a_permutation(model4, requests5, singles):
    """tts_requests on the same data: the waves of test_tts_with_per_line_lists, and a permuted request list returns the permuted waves."""
    waves = model4.tts_requests(requests5, batch_size=5)
    for w, ref in zip(waves, singles):
        assert w.shape == ref.shape and float((w - ref).abs().max()) < WAVE_TOL
    perm = [3, 0, 4, 2, 1]
    for bs in (1, 2, 5):
        a = model4.tts_requests(requests5, batch_size=bs)
        p = model4.tts_requests([requests5[i] for i in perm], batch_size=bs)
        for k, i in enumerate(perm):
            assert p[k].shape == a[i].shape == singles[i].shape
            assert float((p[k] - singles[i]).abs().max()) < WAVE_TOL
    # a request that leaves an option out gets tts()'s default
    w = model4.tts_requests([dict(text=requests5[0]['text'])])[0]
    assert torch.equal(w, model4.tts([requests5[0]['text']])[0])
    assert model4.tts_requests([]) == []
    # ttmel: the mels follow their lines too
    kw = {k: v for k, v in _lists(requests5).items() if k != 'denoise'}
    mels = model4.model.ttmel([r['text'] for r in requests5], batch_size=2, **kw)
    assert [256 * m.shape[1] for m in mels] == [s.shape[0] for s in singles]


def test_refusals(dev, cfg4, synth_weights, batch, model4, requests5):
    from ttsamd import lib as L
    from ttsamd.dp import tts_sharded
    from ttsamd.engine import FastPitchEngine
    from models.fastpitch.networks import pitch_trf
    ids, dur = batch
    eng = FastPitchEngine(synth_weights['fastpitch_spk4'], cfg4, device=dev)
    for kw, exc in ((dict(speaker=[0, 1, 2]), ValueError), (dict(pace=[1.0] * 6), ValueError), (dict(speaker=[0, 1, 2, 3, 4]), IndexError),
                    (dict(speaker=[0, -1, 2, 3, 1]), IndexError), (dict(pace=[1, 1, 0, 1, 1]), ValueError), (dict(pace=[1, -0.5, 1, 1, 1]), ValueError),
                    (dict(pace=[1, 1, float('nan'), 1, 1]), ValueError), (dict(pitch_mul=[1, 1, 1, float('nan'), 1]), ValueError),
                    (dict(pitch_add=[float('inf'), 0, 0, 0, 0]), ValueError)):
        with pytest.raises(exc):
            eng.infer(ids, dur_tgt=dur, **kw)
    # an unknown flag bit
    with pytest.raises(L.TtsAmdError, match='flag'):
        _fp_call(eng, ids, dur, rows=dict(speaker=SPEAKERS), flags=2)
    with pytest.raises(L.TtsAmdError, match='flag'):
        _fp_call(eng, ids, dur, flags=4)
    # the C entries trust device values, memory-safely: a speaker out of range is clamped into the table, a pace that is not > 0 is 1
    bad = _fp_call(eng, ids, dur, rows=dict(speaker=[9, -3, 3, 1, 2], pace=[0.0, -1.0, 1.25, 1.0, 2.0]), flags=0)
    ok = _fp_call(eng, ids, dur, rows=dict(speaker=[3, 0, 3, 1, 2], pace=[1.0, 1.0, 1.25, 1.0, 2.0]), flags=0)
    assert all(torch.equal(bad[k], ok[k]) for k in ('enc_cond', 'reps', 'dec_lens'))
    # wrappers
    texts, lists = [r['text'] for r in requests5], _lists(requests5)
    with pytest.raises(ValueError):
        model4.tts(texts, speed=[1.0, 1.0])
    with pytest.raises(IndexError):
        model4.tts(texts, speaker_id=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError):
        model4.tts(texts, denoise=[0.0, float('nan'), 0, 0, 0])
    with pytest.raises(ValueError):
        model4.tts_requests([dict(text=texts[0], tempo=2)])
    with pytest.raises(ValueError):
        model4.model.ttmel_batch(texts, pitch_mul=lists['pitch_mul'], pitch_transform=lambda p, *a: p)
    with pytest.raises(ValueError):
        model4.model.infer(ids, pitch_add=lists['pitch_add'], pitch_transform=pitch_trf(1.0, 0.5))
    with pytest.raises(ValueError):
        tts_sharded(model4, texts, speed=lists['speed'], dp=object())

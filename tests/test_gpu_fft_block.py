"""FastPitch's own kernels against float64 through the C ABI (pytest -m gpu): attention_kernel<1|2|4>, attention_tile_kernel +
attention_merge_kernel, layernorm_cf_reg_kernel<48|32|64|0>, layernorm_cf_kernel, embed_kernel, pred_fc_kernel, scalar_emb_add_kernel,
add_pos_kernel, lens_plus1_kernel, durations_to_reps_kernel (csrc/elementwise.hip) and, in split bf16, launch_layernorm_cf_x3 and the packed
attention output.

A ONE-layer model through ttsamd_fastpitch_decode is almost a kernel-level test: pos-add -> qkv -> attention -> o_net + residual ->
LayerNorm -> conv-FF -> LayerNorm -> proj, with no further LayerNorm between a kernel's mistake and the assertion; ttsamd_fastpitch_encode
hands back every intermediate result the reference names.  Reference, data, cases and checker: tests/fft_block_ref.py -- every run is
compared with the float64 reference (never with another run), over the valid positions, and must stay within R times the error of the
same reference in float32 on the same data; every output must be finite, padding included.  tests/test_fft_block_ref_cpu.py shows what
that bound rejects.  R per family (fp32 / fp32 with TTSAMD_WINO=0 / split bf16): fft_block_ref.R_*, derived in profiles/r25/NOTES.md."""
import functools

import pytest
import torch

import fft_block_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


_ENGINES = {}


def _engine(cfg):
    """One engine per configuration for the whole module."""
    from ttsamd.engine import FastPitchEngine
    key = R.cfg_key(cfg)
    if key not in _ENGINES:
        _ENGINES[key] = FastPitchEngine(R.weights(cfg), cfg)
    return _ENGINES[key]


# attention schedules (csrc/elementwise.hip: launch_attention): the default choice, each one-kernel tile forced, the tile + merge pair forced
SCHEDULES = {
    'default': {},
    'ra1': {'TTSAMD_ATT_RA': '1', 'TTSAMD_ATT_SPLIT': '0'},
    'ra2': {'TTSAMD_ATT_RA': '2', 'TTSAMD_ATT_SPLIT': '0'},
    'ra4': {'TTSAMD_ATT_RA': '4', 'TTSAMD_ATT_SPLIT': '0'},
    'split': {'TTSAMD_ATT_RA': '1', 'TTSAMD_ATT_SPLIT': '1'},
}


@functools.lru_cache(maxsize=None)
def _dec_refs(name, alone):
    """Data and both references of a decoder case, computed once for all its runs."""
    cfg, x, lens = R.dec_case(name)
    return cfg, x, lens, R.decoder_ref(cfg, x, lens, torch.float64, alone), R.decoder_ref(cfg, x, lens, torch.float32, alone)


def _run_decoder(dev, ttsopt, name, bound, tag, sched='default', wino=None, alone=False):
    cfg, x, lens, r64, r32 = _dec_refs(name, alone)
    for k, v in SCHEDULES[sched].items():
        ttsopt.set(k, v)
    if wino is not None:
        ttsopt.set('TTSAMD_WINO', wino)
    fp = _engine(cfg)
    try:
        mel = fp.decode(x.to(dev).contiguous(), torch.tensor(lens, dtype=torch.int64), alone=alone)     # a fresh copy: decode clobbers x
        torch.cuda.synchronize()
    finally:
        fp.set_batch_mode(False)
    return R.check({'mel': mel}, r64, r32, lens, bound, f'{tag} decoder {name} schedule {sched}')


@pytest.mark.parametrize('sched', sorted(SCHEDULES))
@pytest.mark.parametrize('name', ['A1', 'A2', 'A3'])
def test_decoder_attention_schedules(dev, ttsopt, name, sched):
    """A1 - A3 on the default schedule and under every forced one, each against float64.  A3's zero-length row must come back finite
    (the checker looks at every position) and leave the other rows what the reference says they are."""
    _run_decoder(dev, ttsopt, name, R.R_F32, 'fp32', sched=sched)


@pytest.mark.parametrize('name', [k for k in R.DEC_CASES if k not in ('A1', 'A2', 'A3')])
def test_decoder_shapes_and_widths(dev, ttsopt, name):
    """The smallest shapes, the four LayerNorm variants by width, and the six-layer decoder on the same checker."""
    _run_decoder(dev, ttsopt, name, R.R_F32, 'fp32')


@pytest.mark.parametrize('name', ['A2', 'A3'])
def test_decoder_rows_alone(dev, ttsopt, name):
    """Batch mode 1 against row b alone at its exact length."""
    _run_decoder(dev, ttsopt, name, R.R_F32, 'fp32 alone', alone=True)


@pytest.mark.parametrize('name', list(R.DEC_CASES))
def test_decoder_direct_convs(dev, ttsopt, name):
    """Every case once more with TTSAMD_WINO=0: the conv engine's share apart from attention and LayerNorm."""
    _run_decoder(dev, ttsopt, name, R.R_F32_DIRECT, 'fp32 WINO=0', wino='0')


# ---- encoder ---------------------------------------------------------------------------------------------------------------------

PACES = (1.0, 0.9, 1.1)


@functools.lru_cache(maxsize=None)
def _enc_refs(cfg_key, shape, speaker, targets, pitch_mul, pitch_add, alone):
    cfg = dict(cfg_key)
    ids, counts = R.enc_case(shape)
    pitch_tgt, energy_tgt = R.enc_targets(ids) if targets else (None, None)
    if not cfg['energy_conditioning']:
        energy_tgt = None
    kw = dict(speaker=speaker, pitch_tgt=pitch_tgt, energy_tgt=energy_tgt, pitch_mul=pitch_mul, pitch_add=pitch_add, alone=alone)
    return ids, counts, pitch_tgt, energy_tgt, R.encoder_ref(cfg, ids, torch.float64, **kw), R.encoder_ref(cfg, ids, torch.float32, **kw)


def _run_encoder(dev, ttsopt, cfg, shape, bound, tag, speaker=0, targets=False, pitch_mul=1.0, pitch_add=0.0, alone=False, pace=1.0,
                 wino=None):
    ids, counts, pitch_tgt, energy_tgt, r64, r32 = _enc_refs(R.cfg_key(cfg), shape, speaker, targets, pitch_mul, pitch_add, alone)
    if wino is not None:
        ttsopt.set('TTSAMD_WINO', wino)
    dur_tgt = R.durations_with_ties(ids)                # given, so nothing discrete rides on a rounding of dur_pred
    fp = _engine(cfg)
    try:
        enc, dur_pred, pitch_pred, energy_pred, reps, dec_lens = fp.encode(ids, pace=pace, dur_tgt=dur_tgt, pitch_tgt=pitch_tgt,
                                                                           energy_tgt=energy_tgt, pitch_mul=pitch_mul, pitch_add=pitch_add,
                                                                           speaker=speaker, alone=alone)
        torch.cuda.synchronize()
    finally:
        fp.set_batch_mode(False)
    got = {'enc_cond': enc, 'dur_pred': dur_pred, 'pitch_pred': pitch_pred}
    if cfg['energy_conditioning']:
        got['energy_pred'] = energy_pred
    else:
        assert energy_pred is None and 'energy_pred' not in r64
    want_reps, want_lens = R.reps_exact(dur_tgt, pace)
    assert torch.equal(reps.cpu(), want_reps), 'reps differ from (dur_tgt.float() / pace + 0.5).long()'
    assert torch.equal(dec_lens.cpu(), want_lens)
    return R.check(got, r64, r32, counts, bound, f'{tag} encoder {shape}')


@pytest.mark.parametrize('shape', sorted(R.ENC_COUNTS))
@pytest.mark.parametrize('energy', [True, False])
@pytest.mark.parametrize('n_speakers', [1, 4])
def test_encoder(dev, ttsopt, n_speakers, energy, shape):
    """One encoder layer, the predictors at their two layers: enc_cond, dur_pred, pitch_pred, energy_pred; reps / dec_lens exactly."""
    _run_encoder(dev, ttsopt, R._enc_cfg(n_speakers, energy), shape, R.R_F32, f'fp32 speakers {n_speakers} energy {int(energy)}',
                 speaker=2 if n_speakers > 1 else 0)


@pytest.mark.parametrize('pace', PACES[1:])
def test_encoder_pace(dev, ttsopt, pace):
    """Durations on the rounding step (k + 0.5 and its float32 neighbours) at a pace that is no power of two."""
    _run_encoder(dev, ttsopt, R._enc_cfg(), 'ragged', R.R_F32, f'fp32 pace {pace}', pace=pace)


def test_encoder_from_targets(dev, ttsopt):
    """pitch_tgt / energy_tgt given: the embedding convs read the targets."""
    _run_encoder(dev, ttsopt, R._enc_cfg(), 'ragged', R.R_F32, 'fp32 targets', targets=True)


def test_encoder_pitch_transform(dev, ttsopt):
    """pitch_mul 1.3, pitch_add -0.2: in the padded batch the positions past a row's end hold pitch_add, which the row's last token reads."""
    _run_encoder(dev, ttsopt, R._enc_cfg(), 'ragged', R.R_F32, 'fp32 pitch 1.3 x - 0.2', pitch_mul=1.3, pitch_add=-0.2)


def test_encoder_rows_alone(dev, ttsopt):
    _run_encoder(dev, ttsopt, R._enc_cfg(), 'ragged', R.R_F32, 'fp32 alone', alone=True)
    _run_encoder(dev, ttsopt, R._enc_cfg(), 'ragged', R.R_F32, 'fp32 alone pitch 1.3 x - 0.2', alone=True, pitch_mul=1.3, pitch_add=-0.2)


@pytest.mark.parametrize('pred_filter', [192, 640])
def test_encoder_predictor_widths(dev, ttsopt, pred_filter):
    """Predictor LayerNorm at 192 channels (the run-time-bound kernel) and at 640 (the two-pass kernel)."""
    _run_encoder(dev, ttsopt, R._enc_cfg(pred_filter=pred_filter), 'ragged', R.R_F32, f'fp32 predictor filter {pred_filter}')


@pytest.mark.parametrize('shape', sorted(R.ENC_COUNTS))
def test_encoder_direct_convs(dev, ttsopt, shape):
    _run_encoder(dev, ttsopt, R._enc_cfg(), shape, R.R_F32_DIRECT, 'fp32 WINO=0', wino='0')


# ---- split bf16 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ['A2', 'A3', 'encoder'])
def test_split_bf16(dev, ttsopt, case):
    """set_precision('bf16x3') at B >= 3 (smaller batches run fp32 by design): launch_layernorm_cf_x3 and the packed attention output."""
    from ttsamd.engine import set_precision
    set_precision('bf16x3')
    try:
        if case == 'encoder':
            _run_encoder(dev, ttsopt, R._enc_cfg(), 'ragged', R.R_X3, 'bf16x3')
        else:
            _run_decoder(dev, ttsopt, case, R.R_X3, 'bf16x3')
    finally:
        set_precision('f32')

"""The checker of tests/fft_block_ref.py has teeth (CPU only): it passes the reference's own float32 restatement at R = 2 and rejects,
at the widest bound the GPU test uses, float64 restatements with one thing wrong -- the mistakes an attention, LayerNorm or predictor-head
kernel can make and a whole-model tolerance of 1e-3 cannot see (LayerNorm eps 1e-6 moves the mel by 1.2e-5).

Also the record that the inputs of tests/test_gpu_fft_block.py meet its conditions: layer-0 attention scores with a standard deviation
in [1, 4] over unmasked keys and a mean largest probability below 0.5, for every configuration and shape."""
import functools

import pytest
import torch

import fft_block_ref as R
import tts_oracle as O

R_MAX = max(R.R_F32, R.R_F32_DIRECT)            # a mutant must fail under every fp32 bound
# The mutants' decoder case: W256 (one layer, d_model 256, conv-FF 512, B = 2, T = 100, lens 100 / 37).  LayerNorm eps 1e-6 moves the
# mel by 1.2e-5 to 1.4e-5 at every width; at d_model 384 with the 1536-wide conv-FF the reference's own float32 error is 3.5e-6 (ratio
# 3.2 to 3.5: inside a bound of 4), with the narrow conv-FF it is 2.1e-6 (ratio 6.6), so the narrow one is the case that can see it.
# No zero-length row: its NaN in the float64 reference's padding would be rejected for the wrong reason.
DEC = 'W256'


@functools.lru_cache(maxsize=None)
def _dec():
    cfg, x, lens = R.dec_case(DEC)
    return cfg, x, lens, R.decoder_ref(cfg, x, lens), R.decoder_ref(cfg, x, lens, torch.float32)


@functools.lru_cache(maxsize=None)
def _enc():
    ids, counts = R.enc_case('ragged')
    cfg = R._enc_cfg()
    return cfg, ids, counts, R.encoder_ref(cfg, ids), R.encoder_ref(cfg, ids, torch.float32)


def test_restatement_is_the_oracle():
    """fft_block without a mutant = the oracle's _fft, bit for bit, in both precisions."""
    cfg, x, lens, _, _ = _dec()
    for dtype in (torch.float64, torch.float32):
        W = R._cast(R.weights(cfg), dtype)
        mask = (torch.arange(x.shape[2])[None, :] < torch.tensor(lens)[:, None]).unsqueeze(2)
        inp = x.to(dtype).transpose(1, 2) + R.pos_table(x.shape[2], W['decoder.pos_emb.inv_freq'], dtype) * mask
        assert torch.equal(R.fft_block(W, 'decoder', 1, inp, mask, 64), O._fft(W, 'decoder', 1, inp, mask, 64, 1))


def test_pos_table_float32_is_the_oracle():
    """In float32 the table is the oracle's _pos_emb (the argument rounded to float32 by the matmul); in float64 the argument stays
    the float32 one: it differs from a float64 product by up to T 2^-24."""
    inv = torch.from_numpy(R.weights(R._dec_cfg())['decoder.pos_emb.inv_freq'])
    assert torch.equal(R.pos_table(450, inv, torch.float32), O._pos_emb(torch.arange(450).float(), inv))
    t64 = R.pos_table(450, inv, torch.float64)
    assert float((t64 - R.pos_table(450, inv, torch.float32)).abs().max()) < 2e-7
    assert float((t64 - O._pos_emb(torch.arange(450).double(), inv.double())).abs().max()) > 1e-5


def test_fp32_restatement_passes():
    """The reference's own float32 run as the "kernel", at R = 2: the padded batch through fft_block, the rows alone, the encoder."""
    cfg, x, lens, r64, r32 = _dec()
    W = R._cast(R.weights(cfg), torch.float32)
    mask = (torch.arange(x.shape[2])[None, :] < torch.tensor(lens)[:, None]).unsqueeze(2)
    inp = x.transpose(1, 2) + R.pos_table(x.shape[2], W['decoder.pos_emb.inv_freq'], torch.float32) * mask
    out = R.fft_block(W, 'decoder', 1, inp, mask, 64)
    mel = torch.nn.functional.linear(out, W['proj.weight'], W['proj.bias']).permute(0, 2, 1)
    R.check({'mel': mel}, r64, r32, lens, 2, 'decoder fp32 restatement')
    a32 = R.decoder_ref(cfg, x, lens, torch.float32, alone=True)
    R.check(a32, R.decoder_ref(cfg, x, lens, alone=True), a32, lens, 2, 'decoder fp32 restatement, rows alone')
    ecfg, ids, counts, e64, e32 = _enc()
    R.check(R.encoder_ref(ecfg, ids, torch.float32), e64, e32, counts, 2, 'encoder fp32 restatement')


def test_alone_is_another_result():
    """The padded batch and the rows alone differ at a row's last frame (the un-masked hidden frame): a library that
    ran the wrong one of its two modes is rejected."""
    cfg, x, lens, r64, r32 = _dec()
    with pytest.raises(AssertionError):
        R.check(R.decoder_ref(cfg, x, lens, alone=True), r64, r32, lens, R_MAX, 'rows alone against the padded batch')


@pytest.mark.parametrize('mut', R.FFT_MUTANTS)
def test_decoder_mutant_is_rejected(mut):
    """A key left out at index 64 / at len - 1, LayerNorm eps 1e-6, LayerNorm without the mask multiply (the conv-FF then reads a
    non-zero frame `len`), softmax over all S keys: float64 arithmetic, one thing wrong."""
    cfg, x, lens, r64, r32 = _dec()
    with pytest.raises(AssertionError):
        R.check(R.decoder_ref(cfg, x, lens, mut=mut), r64, r32, lens, R_MAX, f'decoder mutant {mut}')


@pytest.mark.parametrize('mut', R.FFT_MUTANTS)
def test_encoder_mutant_is_rejected(mut):
    cfg, ids, counts, e64, e32 = _enc()
    with pytest.raises(AssertionError):
        R.check(R.encoder_ref(cfg, ids, mut=mut), e64, e32, counts, R_MAX, f'encoder mutant {mut}')


def test_pred_fc_without_mask_is_rejected():
    """The predictor head not zeroed past `len`: the predictions themselves are unchanged at valid positions; the k = 3 pitch embedding
    reads position `len` at the row's last token, so enc_cond (and the energy prediction behind it) moves."""
    cfg, ids, counts, e64, e32 = _enc()
    with pytest.raises(AssertionError):
        R.check(R.encoder_ref(cfg, ids, mut='fc_nomask'), e64, e32, counts, R_MAX, 'encoder mutant fc_nomask')


def test_pos_emb_past_len():
    """The positional embedding added past `len`, the one mutant no output can show: a position past a row's end is read as a key
    (masked: probability exactly 0) and as a query / residual whose row both LayerNorms multiply by 0 before any conv reads it.  The
    valid outputs are the same bits in float64, so the checker -- valid positions only -- cannot reject it, whatever the layer count
    or the attention weights.  Recorded here so that nobody counts on that coverage; what the checker does hold at those positions
    is that they are finite."""
    cfg, x, lens, r64, _ = _dec()
    m = R.decoder_ref(cfg, x, lens, mut='pos_past')['mel']
    assert all(torch.equal(m[b, :, :n], r64['mel'][b, :, :n]) for b, n in enumerate(lens))
    cfg, ids, counts, e64, _ = _enc()
    me = R.encoder_ref(cfg, ids, mut='pos_past')
    assert all(torch.equal(me[k][b, ..., :n], e64[k][b, ..., :n]) for k in e64 for b, n in enumerate(counts))


@pytest.mark.parametrize('name', R.DEC_STATS_CASES)
def test_decoder_inputs_meet_the_conditions(name):
    cfg, x, lens = R.dec_case(name)
    R.assert_conditions(f'decoder {name} (d_model {cfg["symbols_embedding_dim"]})', R.decoder_stats(cfg, x, lens))


@pytest.mark.parametrize('shape', sorted(R.ENC_COUNTS))
@pytest.mark.parametrize('n_speakers', [1, 4])
def test_encoder_inputs_meet_the_conditions(shape, n_speakers):
    ids, counts = R.enc_case(shape)
    R.assert_conditions(f'encoder {shape}, {n_speakers} speaker(s)', R.encoder_stats(R._enc_cfg(n_speakers), ids, speaker=2 if n_speakers > 1 else 0))


def test_durations_sit_on_the_rounding_step():
    """dur_tgt holds k + 0.5 and both float32 neighbours, so reps = (d / pace + 0.5).long() differs between them at pace 1."""
    ids, _ = R.enc_case('ragged')
    dur = R.durations_with_ties(ids)
    frac = dur[0] - dur[0].floor()
    assert bool((frac == 0.5).any()) and bool(((frac > 0.4999) & (frac < 0.5)).any()) and bool(((frac > 0.5) & (frac < 0.5001)).any())
    assert not bool(dur[1, 64:].any()) and not bool(dur[3, 1:].any())
    reps, lens = R.reps_exact(dur, 1.0)
    assert bool((reps[0][frac == 0.5] == dur[0][frac == 0.5] + 0.5).all())
    assert len({tuple(R.reps_exact(dur, p)[1].tolist()) for p in (1.0, 0.9, 1.1)}) == 3

"""Reference, data and checker for FastPitch's own kernels (csrc/elementwise.hip: attention, LayerNorm, embedding, predictor head, scalar
embeddings, positional add) through the two phases of the C ABI.  Plain module: tests/test_fft_block_ref_cpu.py shows that the checker
rejects wrong arithmetic, tests/test_gpu_fft_block.py holds the library to it.

Reference = the oracle's own pieces (oracle/tts_oracle.py: _fft, _predictor, F.embedding, F.conv1d) run at a `dtype`: float64 is the
reference, float32 "the reference's own rounding".  The bound of every check is a multiple R of that rounding error, measured on the
same data -- never an absolute number.

What is restated here rather than taken from the oracle:
  - the positional table: the argument t * inv_freq is rounded to float32 (torch.matmul of float32 tensors in the reference,
    `(float)t * fr` in build_pos_table, csrc/fastpitch.hip), sin / cos are then taken in the run's dtype.  A float64 argument differs
    by up to T 2^-24 (2.7e-5 at T = 450), more than everything else measured here;
  - `fft_block`: the oracle's _fft with switches for the mutants of the CPU test; without a switch it is the oracle's _fft bit for bit
    (the CPU test asserts it), and the references below call the oracle's.

Layout: every tensor handed to `check` has time last ([B, C, T] or [B, T]); `lens[b]` positions of row b are valid."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import tts_oracle as O
from ttsamd import synth
from ttsamd.config import NET_CONFIG


# ---------------------------------------------------------------------------------------------------------------------------------
# configurations and weights
# ---------------------------------------------------------------------------------------------------------------------------------

def make_cfg(d_model=384, dec_layers=1, dec_filter=None, enc_layers=1, enc_filter=None, pred_filter=256, n_speakers=1, energy=True):
    """NET_CONFIG at another width / depth.  Filters default to the product's 4 d."""
    return dict(NET_CONFIG, symbols_embedding_dim=d_model, in_fft_output_size=d_model, out_fft_output_size=d_model,
                in_fft_n_layers=enc_layers, out_fft_n_layers=dec_layers,
                in_fft_conv1d_filter_size=4 * d_model if enc_filter is None else enc_filter,
                out_fft_conv1d_filter_size=4 * d_model if dec_filter is None else dec_filter,
                dur_predictor_filter_size=pred_filter, pitch_predictor_filter_size=pred_filter,
                energy_predictor_filter_size=pred_filter, n_speakers=n_speakers, energy_conditioning=energy)


def cfg_key(cfg):
    return tuple(sorted(cfg.items()))


@functools.lru_cache(maxsize=None)
def _weights(key):
    return synth.fastpitch_state_dict(dict(key))


def weights(cfg):
    """Synthetic state dict of a configuration (numpy float32), built once."""
    return _weights(cfg_key(cfg))


def _cast(sd, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------

def decoder_input(d_model, B, T, lens, seed=3):
    """x ~ N(0, 1) [B, d_model, T] float32, zero past each row's length (what the length regulator hands the decoder)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, d_model, T, generator=g)
    return (x * (torch.arange(T)[None, None, :] < torch.as_tensor(lens)[:, None, None])).contiguous()


def encoder_ids(B, L, counts):
    """synth_ids with the tokens past each row's count set to the padding index 0."""
    ids = torch.from_numpy(synth.synth_ids(B, L))
    return (ids * (torch.arange(L)[None, :] < torch.as_tensor(counts)[:, None])).contiguous()


def durations_with_ties(ids, seed=7):
    """dur_tgt [B, L] float32 in [1.5, 12.5]: k + 0.5 (where (d / pace + 0.5).long() sits on its step at pace 1), its two float32
    neighbours, and whole numbers; 0 at padding."""
    g = torch.Generator().manual_seed(seed)
    B, L = ids.shape
    k = torch.randint(1, 12, (B, L), generator=g).float()
    half = k + 0.5
    kind = torch.arange(B * L).reshape(B, L) % 4
    dur = torch.where(kind == 0, k, half)
    dur = torch.where(kind == 2, torch.nextafter(half, torch.zeros(())), dur)
    dur = torch.where(kind == 3, torch.nextafter(half, torch.full((), 100.0)), dur)
    return (dur * (ids != 0)).contiguous()


def reps_exact(dur_tgt, pace):
    """model.py:72-76 in torch float32: reps int64 [B, L], dec_lens int64 [B]."""
    reps = (dur_tgt.float() / pace + 0.5).long()
    return reps, reps.sum(dim=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------------------

def pos_table(n, inv_freq, dtype):
    """transformer.py:41-44 for positions 0 .. n - 1 -> [1, n, d_model]: float32 argument, sin | cos in `dtype`."""
    arg = torch.arange(n, dtype=torch.float32)[:, None] * inv_freq.to(torch.float32)[None, :]
    arg = arg.to(dtype)
    return torch.cat([arg.sin(), arg.cos()], dim=1)[None]


def fft_block(W, prefix, n_layers, inp, mask, d_head, mut=None):
    """The oracle's _fft (transformer.py:207-225 behind the embedding, one head) with the CPU test's mutants:
      'drop64'      key 64 left out of every softmax          'droplast'   key len - 1 left out
      'eps'         LayerNorm eps 1e-6                        'ln_nomask'  no mask multiply behind the LayerNorms
      'softmax_all' softmax over all S keys, padding included
    mut=None: the same ops in the same order as the oracle's."""
    out = inp
    scale = 1 / (d_head ** 0.5)
    eps = 1e-6 if mut == 'eps' else 1e-5
    keep = mask.squeeze(2)                                                     # [B, S] valid keys
    if mut == 'drop64':
        keep = keep.clone()
        keep[:, 64:65] = False
    elif mut == 'droplast':
        last = keep.sum(dim=1) - 1
        keep = keep & (torch.arange(keep.shape[1])[None, :] != last[:, None])
    elif mut == 'softmax_all':
        keep = torch.ones_like(keep)
    for i in range(n_layers):
        p = f'{prefix}.layers.{i}.'
        B, S, _ = out.shape
        qkv = F.linear(out, W[p + 'dec_attn.qkv_net.weight'], W[p + 'dec_attn.qkv_net.bias'])
        q, k, v = torch.chunk(qkv, 3, dim=2)
        score = torch.bmm(q, k.transpose(1, 2)) * scale
        am = (~keep).unsqueeze(1).repeat(1, S, 1)
        score = score.masked_fill(am, -float('inf'))
        prob = F.softmax(score, dim=2)
        vec = torch.bmm(prob, v)
        att = F.linear(vec, W[p + 'dec_attn.o_net.weight'])
        d_model = out.shape[2]
        out1 = F.layer_norm(out + att, (d_model,), W[p + 'dec_attn.layer_norm.weight'], W[p + 'dec_attn.layer_norm.bias'], eps)
        if mut != 'ln_nomask':
            out1 = out1 * mask
        w0, w2 = W[p + 'pos_ff.CoreNet.0.weight'], W[p + 'pos_ff.CoreNet.2.weight']
        h = F.relu(F.conv1d(out1.transpose(1, 2), w0, W[p + 'pos_ff.CoreNet.0.bias'], padding=w0.shape[2] // 2))
        h2 = F.conv1d(h, w2, W[p + 'pos_ff.CoreNet.2.bias'], padding=w2.shape[2] // 2).transpose(1, 2)
        out2 = F.layer_norm(out1 + h2, (d_model,), W[p + 'pos_ff.layer_norm.weight'], W[p + 'pos_ff.layer_norm.bias'], eps)
        out = out2 if mut == 'ln_nomask' else out2 * mask
    return out


FFT_MUTANTS = ('drop64', 'droplast', 'eps', 'ln_nomask', 'softmax_all')


def _fft(W, prefix, n_layers, inp, mask, d_head, mut):
    if mut in FFT_MUTANTS:
        return fft_block(W, prefix, n_layers, inp, mask, d_head, mut)
    return O._fft(W, prefix, n_layers, inp, mask, d_head, 1)


def _decoder_padded(W, cfg, x, lens, dtype, mut):
    B, d, T = x.shape
    mask = (torch.arange(T)[None, :] < lens[:, None]).unsqueeze(2)
    pos = pos_table(T, W['decoder.pos_emb.inv_freq'], dtype)
    pos = pos if mut == 'pos_past' else pos * mask
    out = _fft(W, 'decoder', cfg['out_fft_n_layers'], x.to(dtype).transpose(1, 2) + pos, mask, cfg['out_fft_d_head'], mut)
    return F.linear(out, W['proj.weight'], W['proj.bias']).permute(0, 2, 1)


def decoder_ref(cfg, x, lens, dtype=torch.float64, alone=False, mut=None):
    """Phase B (model.py:405-408) on x [B, d_model, T] float32, lens [B] -> {'mel': [B, 80, T]}.
    alone=False: the reference's padded batch with masks -- the conv-FF's hidden activation is NOT masked, so frame len - 1 of a row
    reads hid[len].  The batch is as wide as its longest row, which for one row is the caller's T (include/ttsamd.h:
    ttsamd_fastpitch_decode); columns past that are padding and come back zero here.
    alone=True: row b on its own at its exact length.  Rows of length 0 have no valid position and stay zero."""
    lens = torch.as_tensor(lens, dtype=torch.int64)
    W = _cast(weights(cfg), dtype)
    B, d, T = x.shape
    mel = torch.zeros(B, cfg['n_mel_channels'], T, dtype=dtype)
    if alone:
        for b in range(B):
            n = int(lens[b])
            if n:
                mel[b, :, :n] = _decoder_padded(W, cfg, x[b:b + 1, :, :n], lens[b:b + 1], dtype, mut)[0]
    else:
        width = T if B == 1 else int(lens.max())
        mel[:, :, :width] = _decoder_padded(W, cfg, x[:, :, :width], lens, dtype, mut)
    return {'mel': mel}


def _predictor(W, prefix, n_layers, enc_out, mask, mut):
    if mut != 'fc_nomask':
        return O._predictor(W, prefix, n_layers, enc_out, mask)
    return O._predictor(W, prefix, n_layers, enc_out * mask, torch.ones_like(mask))      # the input masked, the head's output not


def _encoder_padded(W, cfg, ids, speaker, pitch_tgt, energy_tgt, pitch_mul, pitch_add, max_duration, dtype, mut):
    B, L = ids.shape
    spk = W['speaker_emb.weight'][torch.ones(B).long() * speaker].unsqueeze(1) * cfg['speaker_emb_weight'] if cfg['n_speakers'] > 1 else 0
    inp = F.embedding(ids, W['encoder.word_emb.weight'], padding_idx=cfg['padding_idx'])
    mask = (ids != cfg['padding_idx']).unsqueeze(2)
    pos = pos_table(L, W['encoder.pos_emb.inv_freq'], dtype)
    pos = pos if mut == 'pos_past' else pos * mask
    enc = _fft(W, 'encoder', cfg['in_fft_n_layers'], inp + pos + spk, mask, cfg['in_fft_d_head'], mut)
    log_dur = _predictor(W, 'duration_predictor', cfg['dur_predictor_n_layers'], enc, mask, mut).squeeze(-1)
    out = {'dur_pred': torch.clamp(torch.exp(log_dur) - 1, 0, max_duration)}
    pitch = _predictor(W, 'pitch_predictor', cfg['pitch_predictor_n_layers'], enc, mask, mut).permute(0, 2, 1)
    if (pitch_mul, pitch_add) != (1.0, 0.0):
        pitch = pitch_mul * pitch + pitch_add                   # pitch_trf (networks.py:38-42) on the masked prediction
    out['pitch_pred'] = pitch
    kp = W['pitch_emb.weight'].shape[2]
    src = pitch if pitch_tgt is None else pitch_tgt.to(dtype)
    enc = enc + F.conv1d(src, W['pitch_emb.weight'], W['pitch_emb.bias'], padding=int((kp - 1) / 2)).transpose(1, 2)
    if cfg['energy_conditioning']:
        ke = W['energy_emb.weight'].shape[2]
        # the library's predictor runs whenever the caller hands it a buffer, targets or not
        energy = _predictor(W, 'energy_predictor', cfg['energy_predictor_n_layers'], enc, mask, mut).squeeze(-1)
        out['energy_pred'] = energy
        e_src = energy.unsqueeze(1) if energy_tgt is None else energy_tgt.to(dtype)
        enc = enc + F.conv1d(e_src, W['energy_emb.weight'], W['energy_emb.bias'], padding=int((ke - 1) / 2)).transpose(1, 2)
    out['enc_cond'] = enc.transpose(1, 2)
    return out


def encoder_ref(cfg, ids, dtype=torch.float64, alone=False, mut=None, speaker=0, pitch_tgt=None, energy_tgt=None, pitch_mul=1.0,
                pitch_add=0.0, max_duration=75):
    """Phase A up to the conditioned encoder output (model.py:355-399) -> {'enc_cond': [B, d_model, L], 'dur_pred': [B, L],
    'pitch_pred': [B, 1, L], 'energy_pred': [B, L]} (no 'energy_pred' without energy conditioning).  alone as in decoder_ref."""
    ids = torch.as_tensor(ids).long()
    W = _cast(weights(cfg), dtype)
    B, L = ids.shape
    args = (speaker, pitch_tgt, energy_tgt, pitch_mul, pitch_add, max_duration, dtype, mut)
    if not alone:
        return _encoder_padded(W, cfg, ids, *args)
    counts = (ids != cfg['padding_idx']).sum(dim=1).tolist()
    rows = []
    for b, n in enumerate(counts):
        sl = (lambda t: None if t is None else t[b:b + 1, ..., :n])
        rows.append(_encoder_padded(W, cfg, ids[b:b + 1, :n], speaker, sl(pitch_tgt), sl(energy_tgt), pitch_mul, pitch_add, max_duration,
                                    dtype, mut) if n else None)
    out = {}
    for name, t in next(r for r in rows if r is not None).items():
        full = torch.zeros((B,) + tuple(t.shape[1:-1]) + (L,), dtype=dtype)
        for b, r in enumerate(rows):
            if r is not None:
                full[b, ..., :counts[b]] = r[name][0]
        out[name] = full
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# input conditions
# ---------------------------------------------------------------------------------------------------------------------------------

def attention_stats(cfg, prefix, inp, lens):
    """(std of the layer-0 scores over unmasked keys, mean over valid queries of the largest probability), float64.
    inp [B, S, d_model] float64: the stack's input (embedding + positions)."""
    W = _cast(weights(cfg), torch.float64)
    p = f'{prefix}.layers.0.'
    qkv = F.linear(inp, W[p + 'dec_attn.qkv_net.weight'], W[p + 'dec_attn.qkv_net.bias'])
    q, k, _ = torch.chunk(qkv, 3, dim=2)
    d_head = q.shape[2]
    scores, pmax = [], []
    for b, n in enumerate(int(v) for v in lens):
        if n:
            s = q[b, :n] @ k[b, :n].T / math.sqrt(d_head)
            scores.append(s.reshape(-1))
            pmax.append(F.softmax(s, dim=1).max(dim=1).values)
    return float(torch.cat(scores).std()), float(torch.cat(pmax).mean())


def decoder_stats(cfg, x, lens):
    lens = torch.as_tensor(lens, dtype=torch.int64)
    T = x.shape[2]
    mask = (torch.arange(T)[None, :] < lens[:, None]).unsqueeze(2)
    inv = torch.from_numpy(weights(cfg)['decoder.pos_emb.inv_freq'])
    return attention_stats(cfg, 'decoder', x.double().transpose(1, 2) + pos_table(T, inv, torch.float64) * mask, lens)


def encoder_stats(cfg, ids, speaker=0):
    ids = torch.as_tensor(ids).long()
    W = _cast(weights(cfg), torch.float64)
    mask = (ids != cfg['padding_idx']).unsqueeze(2)
    inp = F.embedding(ids, W['encoder.word_emb.weight']) + pos_table(ids.shape[1], W['encoder.pos_emb.inv_freq'], torch.float64) * mask
    if cfg['n_speakers'] > 1:
        inp = inp + W['speaker_emb.weight'][speaker] * cfg['speaker_emb_weight']
    return attention_stats(cfg, 'encoder', inp, mask.sum(dim=(1, 2)))


def assert_conditions(tag, stats):
    """A case whose attention is flat cannot see a wrong softmax: score std in [1, 4], mean largest probability below 0.5."""
    std, pmax = stats
    print(f'{tag}: layer-0 score std {std:.2f}, mean max probability {pmax:.3f}')
    assert 1.0 <= std <= 4.0, f'{tag}: score std {std:.3f} outside [1, 4]'
    assert pmax < 0.5, f'{tag}: mean max probability {pmax:.3f}'


# ---------------------------------------------------------------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------------------------------------------------------------

def _max_err(a, ref, lens):
    worst = 0.0
    for b, n in enumerate(int(v) for v in lens):
        if n:
            e = float((a[b, ..., :n].double() - ref[b, ..., :n].double()).abs().max())
            worst = max(worst, e if e == e else float('inf'))           # a NaN among the valid positions: no bound holds
    return worst


def check(got, ref64, ref32, lens, R, tag=''):
    """Per output tensor (dicts name -> tensor, time last), over the valid positions t < lens[b] only:
    e_gpu = max |got - ref64| <= R * e_ref, e_ref = max |ref32 - ref64|; and no NaN / Inf anywhere in `got`, padding included.
    Prints `tag name e_gpu e_ref ratio` per tensor; returns the worst ratio."""
    worst = 0.0
    failures = []
    for name, r64 in ref64.items():
        g = got[name].detach().cpu()
        assert tuple(g.shape) == tuple(r64.shape), f'{tag} {name}: shape {tuple(g.shape)}, expected {tuple(r64.shape)}'
        e_gpu, e_ref = _max_err(g, r64, lens), _max_err(ref32[name], r64, lens)
        ratio = e_gpu / e_ref if e_ref else (0.0 if e_gpu == 0.0 else float('inf'))
        finite = bool(torch.isfinite(g).all())
        print(f'{tag} {name} e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} ratio {ratio:.2f}' + ('' if finite else ' NOT FINITE'))
        worst = max(worst, ratio)
        if not finite:
            failures.append(f'{name}: NaN or Inf in the output')
        if not e_gpu <= R * e_ref:
            failures.append(f'{name}: max-abs {e_gpu:.3e} > {R} x {e_ref:.3e} (the reference\'s own float32 rounding)')
    assert not failures, f'{tag}: ' + '; '.join(failures)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# cases (shared by the CPU test, which records that their inputs meet the conditions above, and the GPU test)
# ---------------------------------------------------------------------------------------------------------------------------------

def _dec_cfg(d_model=384, layers=1, dec_filter=None):
    # the encoder half of the handle is not run by a decoder case: one narrow layer keeps its creation cheap
    return make_cfg(d_model=d_model, dec_layers=layers, dec_filter=dec_filter, enc_layers=1, enc_filter=d_model)


# name -> (cfg, B, T, lens)
DEC_CASES = {
    'A1': (_dec_cfg(), 1, 200, (200,)),                              # batch-1 default: tile + merge kernels
    'A2': (_dec_cfg(), 4, 131, (131, 65, 64, 1)),                    # odd T; one key in the second tile; a full tile; a single key
    'A3': (_dec_cfg(), 5, 200, (200, 129, 128, 17, 0)),              # query blocks wholly / partly past a row's end; a zero-length row
    'A4-1': (_dec_cfg(), 1, 1, (1,)),
    'A4-16': (_dec_cfg(), 2, 16, (16, 15)),
    'A4-17': (_dec_cfg(), 1, 17, (17,)),
    'W256': (_dec_cfg(256, dec_filter=512), 2, 100, (100, 37)),      # layernorm_cf_reg_kernel<32>
    'W512': (_dec_cfg(512, dec_filter=1024), 2, 100, (100, 37)),     # <64>
    'W320': (_dec_cfg(320, dec_filter=640), 2, 100, (100, 37)),      # <0>: run-time bound
    'W576': (_dec_cfg(576, dec_filter=1152), 2, 100, (100, 37)),     # layernorm_cf_kernel: two passes
    'A5': (_dec_cfg(layers=6), 3, 200, (200, 129, 65)),              # the product's depth
    # rows of 256 frames and 192 blocks per launch: the first size at which the conv-FF pair leaves the direct kernel for the Winograd
    # F(4,3) route (csrc/conv_route.hip: conv_route), so that the TTSAMD_WINO=0 run of this case differs from its default run
    'A6': (_dec_cfg(), 8, 256, (256, 255, 200, 131, 129, 64, 17, 1)),
}
# the smallest shapes hold fewer than 64 keys: the largest probability is at least 1 / len whatever the weights are, so the conditions
# on the attention are asserted on the cases below, which share their configuration
DEC_STATS_CASES = tuple(k for k in DEC_CASES if not k.startswith('A4'))


def dec_case(name):
    cfg, B, T, lens = DEC_CASES[name]
    return cfg, decoder_input(cfg['symbols_embedding_dim'], B, T, lens), lens


def _enc_cfg(n_speakers=1, energy=True, pred_filter=256):
    return make_cfg(enc_layers=1, dec_layers=1, dec_filter=384, n_speakers=n_speakers, energy=energy, pred_filter=pred_filter)


ENC_L = 70                                                           # two embed_kernel column blocks, two key tiles
ENC_COUNTS = {'one': (70,), 'ragged': (70, 64, 17, 1)}


def enc_case(shape):
    counts = ENC_COUNTS[shape]
    return encoder_ids(len(counts), ENC_L, counts), counts


def enc_targets(ids, seed=11):
    """pitch_tgt [B, 1, L], energy_tgt [B, 1, L]: N(0, 1), zero at padding (as the reference's collate pads them)."""
    g = torch.Generator().manual_seed(seed)
    m = (ids != 0)[:, None, :]
    return torch.randn(ids.shape[0], 1, ids.shape[1], generator=g) * m, torch.randn(ids.shape[0], 1, ids.shape[1], generator=g) * m


# Bounds of the GPU test, as multiples of the reference's own float32 rounding error on the same data: ceil(2 x the worst ratio measured
# on the MI355X per family); the per-case table and how they were derived: profiles/r25/NOTES.md
R_F32 = 4                # fp32, default conv routes
R_F32_DIRECT = 4         # fp32, TTSAMD_WINO=0 (every conv on the direct MFMA kernel)
R_X3 = 65                # split bf16 (set_precision('bf16x3')), batches of 3 and more

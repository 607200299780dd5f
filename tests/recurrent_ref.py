"""References, cases, mutants and bounds for the two recurrent model families: Tacotron2 (csrc/tacotron2.hip: the encoder, the graph-path
decoder kernels, the persistent decoder, the postnet) and the diacritizer taggers (csrc/tagger.hip).  Plain module:
tests/test_recurrent_ref_cpu.py shows that the checker rejects wrong arithmetic, tests/test_gpu_recurrent.py holds the library to it.

Reference = the oracles themselves (oracle/taco_oracle.py: tacotron2_infer, oracle/diac_oracle.py: shakkelha_forward / shakkala_forward)
run at a `dtype`: float64 is the reference, float32 "the reference's own rounding".  The checker is fft_block_ref.check: over the valid
positions e_gpu = max |got - ref64| <= R * e_ref with e_ref = max |ref32 - ref64| on the same data, every output finite, padding
included; where e_ref is exactly 0 (a one-token row: its attention is 1.0) the library has to be exact as well.  No run is ever compared
with another run.

What is restated here rather than taken from the oracles:
  - `taco_forward` / `tagger_forward`: the oracles' forward passes with switches (`mut=`) for the mutants of the CPU test.  Without a
    switch they are the oracles bit for bit in float64 (the CPU test asserts it), and the references below call the oracles';
  - mel_raw: tacotron2_infer returns the postnet's output only; the frame before the postnet is its own linear projection applied to
    the `hc` it traces, the same op on the same operand;
  - the padded tagger geometry (2H no multiple of 32) has three layers fewer than shakkelha_forward spells out, so its reference is
    `tagger_forward` on the oracle's own _bilstm."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import diac_oracle as DO
import taco_oracle as TO
from fft_block_ref import _max_err, check
from ttsamd import synth
from ttsamd.config import SHAKKALA_CONFIG, SHAKKELHA_CONFIG, TACOTRON2_CONFIG


# ---------------------------------------------------------------------------------------------------------------------------------
# Tacotron2: weights, tokens, cases
# ---------------------------------------------------------------------------------------------------------------------------------

def taco_cfg(num_speakers):
    return dict(TACOTRON2_CONFIG, num_speakers=num_speakers)


@functools.lru_cache(maxsize=None)
def taco_weights(num_speakers):
    """seed 1, gate bias -20: no stop decision rides on a rounding."""
    return synth.tacotron2_state_dict(taco_cfg(num_speakers), seed=1, gate_bias=-20.0)


def _gate_for_stops(cfg, sd, tok, sids, lens, stops, max_step, seed):
    """Synthetic gates barely move in time, so fit (ridge, dual form) a gate layer whose logit is -2 before
    utterance b's chosen stop step and +2 from it on.  The trajectory before a stop does not depend on the
    gate, so a traced never-stopping run provides the layer's inputs; with the prenet dropout on they differ
    enough from step to step that the fit needs only O(1) weights (margin 2 vs ~1e-3 of fp32 noise)."""
    import taco_oracle as T
    tr = {}
    T.tacotron2_infer(sd, cfg, tok, sids, lens, max_step=max_step, seed=seed, trace=tr)
    hc = torch.stack(tr['hc']).double()                                   # [T, B, D+M]
    rows, tgt = [], []
    for b, stop in enumerate(stops):
        for t in range(max_step):
            rows.append(hc[t, b])
            tgt.append(2.0 if t >= stop - 1 else -2.0)
    H, y = torch.stack(rows), torch.tensor(tgt, dtype=torch.float64)
    w = H.T @ torch.linalg.solve(H @ H.T + 1e-6 * torch.eye(len(y), dtype=torch.float64), y)
    assert float(((H @ w) * y).min()) > 1.0 and float(w.abs().sum()) < 5e3
    out = dict(sd)
    out['decoder.gate_layer.weight'] = w[None].float().numpy().copy()
    out['decoder.gate_layer.bias'] = np.zeros(1, np.float32)
    return out


# name -> lens (token count per row, in the order given: not sorted), steps, dropout seed (-1: off), speakers (40: M = 640, 1: M = 512),
# stops (a fitted gate layer: rows end at these steps) and the routing options the case is run under besides the decoder route
TACO_CASES = {
    'T1': dict(lens=(1,), steps=3, seed=2),                           # one token: every location-conv tap but the centre is outside
    'T2': dict(lens=(16, 15), steps=4, seed=-1),                      # L <= 15 = half the location window: every window crosses both edges
    'T3': dict(lens=(65, 64, 1), steps=4, seed=5),                    # 2nd taco_embed_kernel block, partial taco_energy_kernel block, a one-token row
    'T4': dict(lens=(70, 131, 129, 128), steps=4, seed=-1),           # taco_context_kernel's 2nd pass, lens not descending, reverse BiLSTM from n - 1
    'T5': dict(lens=(33, 20, 33, 1, 7, 16, 31, 32, 9), steps=4, seed=5, speakers=1),   # B = 9: the graph path's second batch-column group
    'T6': dict(lens=(256, 255, 200, 131, 129, 64, 17, 1), steps=4, seed=3),            # the persistent decoder's residency corner
    'T7': dict(lens=(300, 257), steps=3, seed=-1),                    # L > 256: graph path only, third context pass
    'TP': dict(lens=(12,) * 8, steps=256, seed=-1),                   # postnet and mel_raw at 256 frames x 8 rows
    'T6S': dict(lens=(256, 255, 200, 131, 129, 64, 17, 1), steps=20, seed=3, opts={'TTSAMD_TACO_SEG': '8'}),   # T6 in segments of 8 steps
    'STOP': dict(lens=(19, 17, 12, 9), steps=16, seed=4, stops=(5, 11, 3, 8)),         # rows stop at different steps; max_step = 16
}


def taco_fits_persistent(name):
    """The persistent decoder's residency plan (csrc/tacotron2.hip: tacotron2_infer): B <= 8 and L <= 256."""
    lens = TACO_CASES[name]['lens']
    return len(lens) <= 8 and max(lens) <= 256


def taco_routes(name):
    """Values of TTSAMD_TACO_PERSISTENT a case is run under: the graph path, both persistent decoders; or the graph path and unset (the
    default route has to fall back to the graph path by itself).  The segmented case is about the persistent decoders only."""
    if name == 'T6S':
        return ('1', '2')
    return ('0', '1', '2') if taco_fits_persistent(name) else ('0', None)


@functools.lru_cache(maxsize=None)
def taco_case(name):
    """(cfg, sd, tokens int64 [B, L], speaker ids or None, lens int64 [B], steps, seed, stops or None) of a case, built once."""
    c = TACO_CASES[name]
    lens = torch.tensor(c['lens'], dtype=torch.int64)
    B, L = len(c['lens']), max(c['lens'])
    speakers = c.get('speakers', 40)
    cfg, sd = taco_cfg(speakers), taco_weights(speakers)
    g = torch.Generator().manual_seed(1000 + sorted(TACO_CASES).index(name))
    tok = torch.randint(1, 40, (B, L), generator=g)
    tok = (tok * (torch.arange(L)[None] < lens[:, None])).contiguous()
    sids = torch.arange(B) % speakers if speakers > 1 else None
    stops = c.get('stops')
    if stops is not None:
        sd = _gate_for_stops(cfg, sd, tok, sids, lens, list(stops), max_step=c['steps'], seed=c['seed'])
    return cfg, sd, tok, sids, lens, c['steps'], c['seed'], stops


# ---------------------------------------------------------------------------------------------------------------------------------
# Tacotron2: the oracle's forward pass with the mutants' switches
# ---------------------------------------------------------------------------------------------------------------------------------

# mutant -> the cases it can show in (a function of the case's entry in TACO_CASES)
TACO_MUTANTS = {
    'ctx128': lambda c: max(c['lens']) > 128,            # the context sums tokens < 128 only
    'tap_last': lambda c: max(c['lens']) >= 16,          # the location conv's last tap (token t + 15) is dropped
    'edge0': lambda c: max(c['lens']) >= 2,              # token 0 of aw / aw_cum is read as 0 (a one-token row's attention is 1.0 whatever its energy)
    'no_cum': lambda c: max(c['lens']) >= 2 and c['steps'] >= 3,      # aw_cum = aw: differs from the sum once two steps have been summed
    'rev_pad': lambda c: min(c['lens']) < max(c['lens']),             # the reverse encoder direction starts at L - 1
    'b8_dup': lambda c: len(c['lens']) >= 9,             # rows >= 8 of the mel frame copy row 7
    # the mel frame is multiplied by 1 + 3e-6 each step: 13 to 45 times float32's own error over 3 to 20 steps.  Not over TP's 256: there
    # the decoder multiplies float32's own error by 70 to 700 (e_ref 2e-5 on one CPU, 2e-4 on another), the mutant's footprint with it, and
    # their ratio is 9 on the first and 2.3 on the second: a trajectory float32 itself has lost cannot show a 3e-6 mutation
    'mel_3e-6': lambda c: c['steps'] <= 20,
    'bn_eps': lambda c: True,                            # 1e-3 instead of 1e-5 in the encoder fold
}


def taco_mutant_cases(mut):
    return [name for name, c in TACO_CASES.items() if TACO_MUTANTS[mut](c)]


def _bn_fold(W, name, eps):
    s = W[name + '.weight'] / torch.sqrt(W[name + '.running_var'] + eps)
    return s, W[name + '.bias'] - W[name + '.running_mean'] * s


def taco_forward(w, cfg, tokens, speaker_ids=None, lengths=None, max_step=None, seed=-1, dtype=torch.float32, mut=None):
    """taco_oracle.tacotron2_infer, op for op, with the switches of TACO_MUTANTS -> ({'mel_raw', 'mel_post': [B, 80, T], 'alignments':
    [B, T, L]}, mel_lens int32 [B])."""
    assert mut is None or mut in TACO_MUTANTS, mut
    W = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items()}
    tokens = torch.as_tensor(np.asarray(tokens)).long()
    B, L = tokens.shape
    lengths = torch.full((B,), L, dtype=torch.long) if lengths is None else torch.as_tensor(np.asarray(lengths)).long()
    speaker_ids = torch.zeros(B, dtype=torch.long) if speaker_ids is None else torch.as_tensor(np.asarray(speaker_ids)).long()
    max_step = cfg['decoder_max_step'] if max_step is None else max_step
    # ---- encoder
    x = F.embedding(tokens, W['embedding.weight']).transpose(1, 2)
    for i in range(cfg['encoder_n_convolution']):
        p = f'encoder.convolutions.{i}.'
        x = F.conv1d(x, W[p + '0.weight'], W[p + '0.bias'], padding=(cfg['encoder_kernel_size'] - 1) // 2)
        s, t = _bn_fold(W, p + '1', 1e-3 if mut == 'bn_eps' else 1e-5)
        x = F.relu(x * s[None, :, None] + t[None, :, None])
    x = x.transpose(1, 2)
    Hh = cfg['encoder_embedding_dim'] // 2
    enc = torch.zeros(B, L, 2 * Hh, dtype=dtype)
    for b in range(B):
        n = int(lengths[b])
        h = c = torch.zeros(1, Hh, dtype=dtype)
        for t in range(n):
            h, c = TO._lstm_cell(x[b:b + 1, t], h, c, W, 'encoder.lstm', '_l0')
            enc[b, t, :Hh] = h[0]
        h = c = torch.zeros(1, Hh, dtype=dtype)
        for t in range((L if mut == 'rev_pad' else n) - 1, -1, -1):
            h, c = TO._lstm_cell(x[b:b + 1, t], h, c, W, 'encoder.lstm', '_l0_reverse')
            if t < n:
                enc[b, t, Hh:] = h[0]
    if cfg['num_speakers'] > 1:
        spk = W['speaker_embedding.weight'][speaker_ids].unsqueeze(1).repeat(1, L, 1)
        memory = torch.cat((enc, spk), dim=2)
    else:
        memory = enc
    # ---- decoder
    A, D = cfg['attention_rnn_dim'], cfg['decoder_rnn_dim']
    Mdim = memory.shape[2]
    mask = torch.arange(L)[None, :] >= lengths[:, None]
    pm = F.linear(memory, W['decoder.attention_layer.memory_layer.weight'])
    att_h = torch.zeros(B, A, dtype=dtype); att_c = torch.zeros(B, A, dtype=dtype)
    dec_h = torch.zeros(B, D, dtype=dtype); dec_c = torch.zeros(B, D, dtype=dtype)
    aw = torch.zeros(B, L, dtype=dtype); aw_cum = torch.zeros(B, L, dtype=dtype)
    ctx = torch.zeros(B, Mdim, dtype=dtype)
    dec_in = torch.zeros(B, cfg['n_mels'], dtype=dtype)
    mel_lens = torch.zeros(B, dtype=torch.int32)
    finished = torch.zeros(B, dtype=torch.bool)
    mels, aligns = [], []
    ks = cfg['attention_location_kernel_size']
    loc_w = W['decoder.attention_layer.location_layer.location_conv.weight']
    if mut == 'tap_last':
        loc_w = loc_w.clone()
        loc_w[:, :, -1] = 0
    for step in range(max_step):
        p = dec_in
        for li in range(2):
            p = F.relu(F.linear(p, W[f'decoder.prenet.layers.{li}.weight']))
            if seed >= 0:
                p = p * TO.keep_mask(seed, li, step, B, p.shape[1]).to(dtype)
        att_h, att_c = TO._lstm_cell(torch.cat((p, ctx), -1), att_h, att_c, W, 'decoder.attention_rnn')
        cat = torch.cat((aw.unsqueeze(1), aw_cum.unsqueeze(1)), dim=1)
        if mut == 'edge0':
            cat = cat.clone()
            cat[:, :, 0] = 0
        pq = F.linear(att_h.unsqueeze(1), W['decoder.attention_layer.query_layer.weight'])
        loc = F.conv1d(cat, loc_w, padding=(ks - 1) // 2)
        pl = F.linear(loc.transpose(1, 2), W['decoder.attention_layer.location_layer.location_dense.weight'])
        e = F.linear(torch.tanh(pq + pl + pm), W['decoder.attention_layer.v.weight']).squeeze(2)
        e = e.masked_fill(mask, -float('inf'))
        aw = F.softmax(e, dim=1)
        if mut == 'ctx128':
            ctx = torch.bmm(aw[:, :128].unsqueeze(1), memory[:, :128]).squeeze(1)
        else:
            ctx = torch.bmm(aw.unsqueeze(1), memory).squeeze(1)
        aw_cum = aw if mut == 'no_cum' else aw_cum + aw
        dec_h, dec_c = TO._lstm_cell(torch.cat((att_h, ctx), -1), dec_h, dec_c, W, 'decoder.decoder_rnn')
        hc = torch.cat((dec_h, ctx), dim=1)
        mel = F.linear(hc, W['decoder.linear_projection.weight'], W['decoder.linear_projection.bias'])
        gate = F.linear(hc, W['decoder.gate_layer.weight'], W['decoder.gate_layer.bias'])
        if mut == 'b8_dup':
            mel = mel.clone()
            mel[8:] = mel[7]
        elif mut == 'mel_3e-6':
            mel = mel * (1 + 3e-6)
        mels.append(mel); aligns.append(aw)
        mel_lens[~finished] += 1
        finished |= torch.sigmoid(gate.squeeze(1)) > cfg['gate_threshold']
        if cfg.get('decoder_early_stopping', True) and bool(torch.all(finished)):
            break
        dec_in = mel
    mel = torch.stack(mels, dim=2)
    align = torch.stack(aligns, dim=1)
    # ---- postnet
    y = mel
    n = cfg['postnet_n_convolution']
    for i in range(n):
        p = f'postnet.convolutions.{i}.'
        y = F.conv1d(y, W[p + '0.weight'], W[p + '0.bias'], padding=(cfg['postnet_kernel_size'] - 1) // 2)
        s, t = _bn_fold(W, p + '1', 1e-5)
        y = y * s[None, :, None] + t[None, :, None]
        if i < n - 1:
            y = torch.tanh(y)
    return {'mel_raw': mel, 'mel_post': mel + y, 'alignments': align}, mel_lens


def taco_oracle_run(cfg, sd, tok, sids, lens, steps, seed, dtype):
    """The oracle at `dtype` -> the same pair as taco_forward; mel_raw from the traced gate-layer input."""
    tr = {}
    post, mel_lens, align = TO.tacotron2_infer(sd, cfg, tok, sids, lens, max_step=steps, seed=seed, dtype=dtype, trace=tr)
    Wp, bp = (torch.as_tensor(np.asarray(sd['decoder.linear_projection.' + k])).to(dtype) for k in ('weight', 'bias'))
    raw = torch.stack([F.linear(hc, Wp, bp) for hc in tr['hc']], dim=2)
    return {'mel_raw': raw, 'mel_post': post, 'alignments': align}, mel_lens


@functools.lru_cache(maxsize=None)
def taco_refs(name):
    """(ref64, ref32, mel_lens) of a case: both references, computed once for every run of the case."""
    cfg, sd, tok, sids, lens, steps, seed, stops = taco_case(name)
    r64, l64 = taco_oracle_run(cfg, sd, tok, sids, lens, steps, seed, torch.float64)
    r32, l32 = taco_oracle_run(cfg, sd, tok, sids, lens, steps, seed, torch.float32)
    want = list(stops) if stops is not None else [steps] * len(lens)
    assert l64.tolist() == l32.tolist() == want, (name, l64.tolist(), l32.tolist())
    return r64, r32, l64


def taco_mutant(name, mut, dtype=torch.float32):
    cfg, sd, tok, sids, lens, steps, seed, _ = taco_case(name)
    return taco_forward(sd, cfg, tok, sids, lens, max_step=steps, seed=seed, dtype=dtype, mut=mut)


def check_taco(got, name, R, tag):
    """mel_raw / mel_post [B][80][T] over the frames before each row's stop (every frame where no gate fires), alignments [B][T][L]
    over each row's tokens and, in the stop-token case, row by row over the frames before its stop.  Returns the worst ratio."""
    r64, r32, mel_lens = taco_refs(name)
    lens = TACO_CASES[name]['lens']
    frames = mel_lens.tolist()
    mels = ('mel_raw', 'mel_post')
    worst = check({k: got[k] for k in mels}, {k: r64[k] for k in mels}, {k: r32[k] for k in mels}, frames, R, f'{tag} {name}')
    if TACO_CASES[name].get('stops') is None:
        al = {'alignments': got['alignments']}, {'alignments': r64['alignments']}, {'alignments': r32['alignments']}
        return max(worst, check(*al, lens, R, f'{tag} {name}'))
    assert tuple(got['alignments'].shape) == tuple(r64['alignments'].shape)
    for b, n in enumerate(frames):
        row = [{f'alignments[{b}]': t['alignments'][b:b + 1, :n]} for t in (got, r64, r32)]
        worst = max(worst, check(*row, lens[b:b + 1], R, f'{tag} {name}'))
    assert bool(torch.isfinite(got['alignments']).all())
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# taggers
# ---------------------------------------------------------------------------------------------------------------------------------

# 2H = 200 and 104: Cy = align_up(2H, 32) != 2H, the zero-padded channel rows of tagger_forward
PADDED_CONFIG = dict(SHAKKELHA_CONFIG, lstm_hidden=[100, 52], dense_dim=[64, 19])
TAGGER_CONFIGS = {'shakkelha': SHAKKELHA_CONFIG, 'shakkala': SHAKKALA_CONFIG, 'padded': PADDED_CONFIG}
# (B, T): the smallest shape; a second tagger_embed_kernel block; a second tagger_softmax_kernel block; the 1x1 convs at a block count
# where the conv router may leave the direct kernel
TAGGER_CASES = {
    'shakkelha': ((1, 1), (2, 65), (3, 257), (9, 300)),
    'shakkala': ((1, 1), (2, 65), (3, 257), (9, 300)),
    'padded': ((2, 65), (1, 1)),
}
TAGGER_MUTANTS = {
    'hard_knee': lambda cfg, B, T: bool(cfg['hard_sigmoid']),         # the hard sigmoid is clamped to [0, 0.999]
    't64_dup': lambda cfg, B, T: T > 64,                              # the embedding of position t >= 64 is read from t - 64
    'bn_eps': lambda cfg, B, T: bool(cfg['bn_after_lstm0']),          # 1e-5 instead of 1e-3
}


def tagger_mutant_cases(mut):
    return [(kind, B, T) for kind, shapes in TAGGER_CASES.items() for B, T in shapes if TAGGER_MUTANTS[mut](TAGGER_CONFIGS[kind], B, T)]


@functools.lru_cache(maxsize=None)
def tagger_weights(kind):
    if kind == 'shakkelha':
        return synth.shakkelha_state_dict()
    if kind == 'shakkala':
        return synth.shakkala_state_dict()
    # the padded geometry: made as synth.shakkelha_state_dict makes its own
    c, sd, seed = TAGGER_CONFIGS[kind], {}, 0
    sd['emb0.weight'] = synth._normal(seed, kind + '.emb', (c['n_vocab'], c['emb_dim']), 1.0)
    n_in = c['emb_dim']
    for i, h in enumerate(c['lstm_hidden']):
        synth._lstm(sd, seed, f'lstm{i}', n_in, h, ('_l0', '_l0_reverse'), gain=synth.TAGGER_LSTM_GAIN)
        n_in = 2 * h
    for i, d in enumerate(c['dense_dim']):
        synth._dense(sd, seed, f'dense{i}', n_in, d, 1.4 if i < len(c['dense_dim']) - 1 else synth.TAGGER_OUT_GAIN)
        n_in = d
    return sd


def tagger_ids(kind, B, T):
    g = torch.Generator().manual_seed(T)
    return torch.randint(1, TAGGER_CONFIGS[kind]['n_vocab'], (B, T), generator=g)


def _cast(sd, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) if np.asarray(v).dtype.kind == 'f' else torch.from_numpy(np.asarray(v))
            for k, v in sd.items()}


def _bilstm(x, W, name, hard, knee):
    """diac_oracle._bilstm; knee < 1: its hard sigmoid clamped to [0, knee]."""
    if knee == 1.0:
        return DO._bilstm(x, W, name, hard)
    assert hard
    gate = (lambda v: torch.clamp(0.2 * v + 0.5, 0.0, knee))
    outs = []
    for sfx, rev in (('_l0', False), ('_l0_reverse', True)):
        w_ih, w_hh = W[f'{name}.weight_ih{sfx}'], W[f'{name}.weight_hh{sfx}']
        b = W[f'{name}.bias_ih{sfx}'] + W[f'{name}.bias_hh{sfx}']
        h = c = torch.zeros(x.shape[0], w_hh.shape[1], dtype=x.dtype)
        xp = F.linear(x, w_ih, b)
        ys = [None] * x.shape[1]
        for t in (range(x.shape[1] - 1, -1, -1) if rev else range(x.shape[1])):
            i, f, g, o = (xp[:, t] + F.linear(h, w_hh)).chunk(4, 1)
            c = gate(f) * c + gate(i) * torch.tanh(g)
            h = gate(o) * torch.tanh(c)
            ys[t] = h
        outs.append(torch.stack(ys, 1))
    return torch.cat(outs, 2)


def tagger_forward(cfg, W, ids, mut=None):
    """shakkelha_forward / shakkala_forward for any tagger geometry (W: tensors of the run's dtype), with the switches of TAGGER_MUTANTS."""
    assert mut is None or mut in TAGGER_MUTANTS, mut
    hard = bool(cfg['hard_sigmoid'])
    knee = 0.999 if mut == 'hard_knee' else 1.0
    x = F.embedding(torch.as_tensor(np.asarray(ids)).long(), W['emb_input.weight' if 'emb_input.weight' in W else 'emb0.weight'])
    if mut == 't64_dup':
        x = torch.cat((x[:, :64], x[:, :x.shape[1] - 64]), dim=1)
    for l in range(len(cfg['lstm_hidden'])):
        x = _bilstm(x, W, f'lstm{l}', hard, knee)
        if l == 0 and cfg['bn_after_lstm0']:
            s = W['bn0.weight'] / torch.sqrt(W['bn0.running_var'] + (1e-5 if mut == 'bn_eps' else 1e-3))
            x = (x - W['bn0.running_mean']) * s + W['bn0.bias']
    n = len(cfg['dense_dim'])
    for i in range(n):
        x = F.linear(x, W[f'dense{i}.weight'], W[f'dense{i}.bias'])
        if i < n - 1:
            x = F.relu(x)
    return F.softmax(x, dim=-1)


def tagger_run(kind, B, T, dtype, mut=None, oracle=True):
    """probs [B, T, n_classes] at `dtype`: the oracle's function where it has one for the geometry (and no mutant is asked for)."""
    W = _cast(tagger_weights(kind), dtype)
    ids = tagger_ids(kind, B, T)
    if oracle and mut is None and kind == 'shakkelha':
        return DO.shakkelha_forward(W, ids)
    if oracle and mut is None and kind == 'shakkala':
        return DO.shakkala_forward(W, ids)
    return tagger_forward(TAGGER_CONFIGS[kind], W, ids, mut)


@functools.lru_cache(maxsize=None)
def tagger_refs(kind, B, T):
    return tagger_run(kind, B, T, torch.float64), tagger_run(kind, B, T, torch.float32)


def check_tagger(probs, kind, B, T, R, tag):
    """The bound on the probabilities (classes on the last axis, all of them valid), and no arg-max other than float64's wherever
    float64's top-two margin exceeds R * e_ref."""
    r64, r32 = tagger_refs(kind, B, T)
    n_cls = r64.shape[2]
    worst = check({'probs': probs}, {'probs': r64}, {'probs': r32}, [n_cls] * B, R, f'{tag} {kind} ({B}, {T})')
    e_ref = float((r32.double() - r64).abs().max())
    top = r64.topk(2, dim=-1).values
    sure = (top[..., 0] - top[..., 1]) > R * e_ref
    differ = (probs.detach().cpu().argmax(-1) != r64.argmax(-1)) & sure
    assert not bool(differ.any()), f'{tag} {kind} ({B}, {T}): {int(differ.sum())} arg-max differ from float64 at a margin above {R} x {e_ref:.3e}'
    return worst


# Bounds of the GPU test, as multiples of the reference's own float32 rounding error on the same data: ceil(2 x the worst ratio measured
# on the MI355X per family); the per-case table and how they follow from it: profiles/r32/NOTES.md
R_TACO_F32 = 10          # fp32, default conv routes: worst 4.60 (T6S, persistent 2, mel_post)
R_TACO_DIRECT = 6        # fp32, TTSAMD_WINO=0 (TP): worst 2.56 (graph path, mel_raw) over four runs of a 256-step draw, 0.34 in the last
R_TACO_X3 = 37           # split bf16 (set_precision('bf16x3')): worst 18.47 (T4, persistent 2, mel_post)
R_TAGGER = 5             # taggers (always fp32), both conv routes: worst 2.50 (shakkelha (3, 257))

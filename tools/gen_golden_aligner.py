"""Generate tests/golden/aligner.npz with the REAL reference's FastPitch (its ConvAttention, mas_width1 and average_pitch).
Run manually where the reference tree is readable (oracle/_refstub.py: TTS_REFERENCE):  python tools/gen_golden_aligner.py

What runs is the reference's own text on the CPU: fp.attention(...) as FastPitch.forward calls it (model.py:299-308), mas_width1 per row as
binarize_attention does (model.py:246-255; the method itself cannot run on the CPU: attn.get_device() is -1 there; the numba decorator is the
identity, oracle/_refstub.py), average_pitch (model.py:318).  Weights: ttsamd.synth.fastpitch_state_dict + fastpitch_aligner_state_dict.

Inputs.  With weights of order 1 the factor -0.0005 makes the attention nearly uniform and the path a matter of rounding, so GAIN scales the
last conv of both encoders, and the mel starts piecewise constant per token (a random band vector per token, held for a planned duration),
is moved until its queries sit at the planned tokens' keys (fit_mel) and gets noise: a recording that belongs to its text, so MAS has a real
path to find (it recovers the planned durations up to a frame here and there).  The reference alone must then be unambiguous, which the file records and
tests/test_aligner_cpu.py asserts: its fp32 path equals the float64 path, and the smallest |log_p[i-1, j-1] - log_p[i-1, j]| met on the
backtrack is at least 8 x the largest |log_p fp32 - log_p float64| over the table.  Per compared key the file also holds the reference's own
noise floor: max |fp32 reference - float64 restatement (tests/aligner_ref.py)|."""
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN, SEED = 8.0, 0
IN_LENS, MEL_LENS = (18, 13, 9), (48, 37, 22)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


R = _load('aligner_ref', os.path.join(REPO, 'tests', 'aligner_ref.py'))
# our own synth generator, loaded by path (package names must not shadow the reference's)
_pkg = types.ModuleType('ttsamd')
_pkg.__path__ = [os.path.join(REPO, 'tts-arabic-pytorch_amd', 'ttsamd')]
sys.modules['ttsamd'] = _pkg
config = _load('ttsamd.config', os.path.join(_pkg.__path__[0], 'config.py'))
synth = _load('ttsamd.synth', os.path.join(_pkg.__path__[0], 'synth.py'))
_refstub = _load('_refstub', os.path.join(REPO, 'oracle', '_refstub.py'))


def make_inputs(rng, cfg):
    """-> ids, planned segments (token of each frame, -1 past the row's end), a piecewise-constant mel to start from, pitch, prior"""
    B, L, T = len(IN_LENS), max(IN_LENS), max(MEL_LENS)
    ids = np.zeros((B, L), np.int64)
    seg = np.full((B, T), -1, np.int64)
    mel = np.zeros((B, cfg['n_mel_channels'], T), np.float32)
    pitch = np.zeros((B, 1, T), np.float32)
    for b, (n, t) in enumerate(zip(IN_LENS, MEL_LENS)):
        ids[b, :n] = rng.integers(1, cfg['n_symbols'], n)
        cuts = np.sort(rng.choice(np.arange(1, t), n - 1, replace=False))
        seg[b, :t] = np.repeat(np.arange(n), np.diff(np.concatenate([[0], cuts, [t]])))
        mel[b, :, :t] = (rng.standard_normal((cfg['n_mel_channels'], n)) * 2.0 - 5.0)[:, seg[b, :t]]
        voiced = rng.random(T) > 0.3
        pitch[b, 0] = np.where(voiced, rng.standard_normal(T) * 0.8, 0.0)
    prior = rng.random((B, T, L)).astype(np.float32) ** 2
    return ids, seg, mel, pitch, prior


def fit_mel(fp, ids, seg, mel, rng, steps=400):
    """Moves the piecewise-constant mel towards one whose queries sit at the keys of the planned tokens (Adam on the reference's own query
    encoder), then adds noise: a recording that does belong to its text, so the search has a real path to find.  Frames past a row's end keep
    noise only (the reference reads them too)."""
    import torch
    with torch.enable_grad():
        keys = fp.attention.key_proj(fp.encoder.word_emb(torch.from_numpy(ids)).permute(0, 2, 1)).detach()      # [B, C, L]
        live = torch.from_numpy(seg >= 0)
        target = torch.gather(keys, 2, torch.from_numpy(np.maximum(seg, 0))[:, None, :].expand(-1, keys.shape[1], -1))
        x = torch.from_numpy(mel.copy()).requires_grad_(True)
        opt = torch.optim.Adam([x], lr=0.05)
        for _ in range(steps):
            opt.zero_grad()
            loss = (((fp.attention.query_proj(x) - target) ** 2).sum(1) * live).sum()
            loss.backward()
            opt.step()
    out = x.detach().numpy() * (seg >= 0)[:, None, :]
    return (out + rng.standard_normal(out.shape) * 0.05).astype(np.float32)


def main():
    cfg = dict(config.NET_CONFIG)
    rng = np.random.default_rng(SEED)
    ids, seg, mel, pitch, prior = make_inputs(rng, cfg)
    in_lens, mel_lens = np.array(IN_LENS, np.int64), np.array(MEL_LENS, np.int64)
    sd = synth.fastpitch_state_dict(cfg, 0)
    sd.update(synth.fastpitch_aligner_state_dict(cfg, 0, GAIN))

    _refstub.install()
    import torch
    from models.fastpitch.fastpitch.model import FastPitch, average_pitch, mask_from_lens
    from models.fastpitch.fastpitch.alignment import mas_width1
    torch.set_grad_enabled(False)
    fp = FastPitch(**cfg)
    missing, unexpected = fp.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith('attention.attn_proj.') for k in missing), (missing, unexpected)
    fp.eval()
    want = {k: tuple(v.shape) for k, v in fp.state_dict().items()
            if k.startswith('attention.key_proj.') or k.startswith('attention.query_proj.')}

    mel = fit_mel(fp, ids, seg, mel, rng)
    t_ids, t_in, t_mel, t_ml = torch.from_numpy(ids), torch.from_numpy(in_lens), torch.from_numpy(mel), torch.from_numpy(mel_lens)
    text_emb = fp.encoder.word_emb(t_ids)
    attn_mask = mask_from_lens(t_in, max_len=ids.shape[1])[..., None] == 0
    out = {'ids': ids, 'in_lens': in_lens, 'mel': mel, 'mel_lens': mel_lens, 'pitch': pitch, 'prior': prior,
           'gain': np.float64(GAIN), 'aligner_keys': np.array(sorted(want)), 'aligner_shapes': np.array([str(want[k]) for k in sorted(want)])}
    for tag, pr in (('', None), ('_prior', prior)):
        soft, logprob = fp.attention(t_mel, text_emb.permute(0, 2, 1), t_ml, attn_mask, key_lens=t_in,
                                     attn_prior=None if pr is None else torch.from_numpy(pr))
        soft64, logprob64 = R.attention(sd, ids, mel, in_lens, pr, np.float64)
        log_attn = torch.log(soft.data).to(dtype=torch.float32).numpy()                       # model.py:248-249
        hard = np.zeros(log_attn.shape, np.float32)
        log64 = np.log(soft64)
        margin, table_err, same = np.inf, 0.0, True
        for b in range(ids.shape[0]):
            t, n = int(mel_lens[b]), int(in_lens[b])
            hard[b, 0, :t, :n] = mas_width1(log_attn[b, 0, :t, :n])
            p32, p64 = R.mas_forward(log_attn[b, 0, :t, :n]), R.mas_forward(log64[b, 0, :t, :n])
            path64, _ = R.mas_backtrack(p64)
            same = same and np.array_equal(path64, hard[b, 0, :t, :n])
            _, m = R.mas_backtrack(p32)
            margin = min(margin, float(np.nanmin(m)))
            fin = np.isfinite(p32) & np.isfinite(p64)
            assert np.array_equal(np.isfinite(p32), np.isfinite(p64))
            table_err = max(table_err, float(np.abs(p32[fin].astype(np.float64) - p64[fin]).max()))
        dur = hard.sum(2)[:, 0, :]
        assert np.array_equal(dur.sum(1), mel_lens.astype(np.float32))                        # model.py:315
        out['attn_soft' + tag] = soft.numpy()
        out['attn_logprob' + tag] = logprob.numpy()
        out['attn_hard' + tag] = hard.astype(np.uint8)
        out['dur' + tag] = dur
        out['floor_attn_soft' + tag] = np.float64(np.abs(soft.numpy() - soft64).max())
        out['floor_attn_logprob' + tag] = np.float64(np.abs(logprob.numpy() - logprob64).max())
        out['path_fp32_equals_fp64' + tag] = np.bool_(same)
        out['min_backtrack_margin' + tag] = np.float64(margin)
        out['max_table_err' + tag] = np.float64(table_err)
        if pr is None:
            out['log_attn'] = log_attn
            pt = average_pitch(torch.from_numpy(pitch), torch.from_numpy(dur)).numpy()
            out['pitch_tgt'] = pt
            out['floor_pitch_tgt'] = np.float64(np.abs(pt - R.average_pitch(pitch, dur)).max())
        print(f'aligner{tag}: fp32 path == float64 path: {same}; smallest margin on the backtrack {margin:.3e}, largest |log_p fp32 - f64| '
              f'{table_err:.3e} (ratio {margin / table_err:.1f}, needs >= 8); floors soft {float(out["floor_attn_soft" + tag]):.3e} '
              f'logprob {float(out["floor_attn_logprob" + tag]):.3e}; soft row max: median {np.median(soft.numpy().max(-1)):.3f}')
        assert same and margin >= 8 * table_err
    planned = [np.bincount(seg[b][seg[b] >= 0], minlength=ids.shape[1]).tolist() for b in range(ids.shape[0])]
    print(f'pitch_tgt floor {float(out["floor_pitch_tgt"]):.3e}\nplanned {planned}\ndur     {out["dur"].astype(int).tolist()}')
    path = os.path.join(REPO, 'tests', 'golden', 'aligner.npz')
    np.savez_compressed(path, **out)
    print(f'aligner: {os.path.getsize(path) / 1024:.1f} kB')


if __name__ == '__main__':
    main()

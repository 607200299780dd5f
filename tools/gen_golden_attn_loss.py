"""Generate tests/golden/attn_loss.npz: the alignment prior and the two alignment losses as the REAL reference computes them.
Run manually where the reference tree is readable (oracle/_refstub.py: TTS_REFERENCE):  python tools/gen_golden_attn_loss.py

What runs: the reference's attn_loss_function.py, loaded by path (AttentionCTCLoss, AttentionBinarizationLoss; torch on the CPU), and
scipy.stats.betabinom / scipy.ndimage.zoom called exactly as the reference's data_function.py:59-78 calls them (that module imports librosa
at its top, so its two functions' arithmetic is invoked through scipy directly).

Contents: exact priors and interpolated priors at small sizes (float64); a random attn_logprob (standard normal x 3, seed 0) [4, 1, 48, 18]
with two sets of out_lens, the second of which leaves row 0 fewer frames than tokens; on both, AttentionCTCLoss in float64 and float32 and
the per-row float64 F.ctc_loss(reduction='none'); AttentionBinarizationLoss on aligner.npz's attn_hard / attn_soft in both precisions.
And one check the GPU test leans on: with aligner.npz's inputs and weights, tests/aligner_ref.py (float64) and the interpolated prior, the
forward-sum cost per token of rows 1 and 2 rises when their texts are swapped; the margin is recorded."""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ((18, 48), (13, 37), (9, 22), (1, 1), (1, 7), (65, 70))                     # (P, M)
INTERP = ((48, 18), (37, 13), (22, 9), (149, 29), (150, 30), (249, 49), (250, 50), (49, 9), (51, 11), (2, 1), (1, 3), (1, 1))   # (w, h)
IN_LENS, OUT_LENS, OUT_LENS_INFEASIBLE = (18, 13, 9, 1), (48, 37, 22, 5), (10, 37, 22, 5)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def ref_exact(P, M, scaling=1.0):
    """data_function.py:68-78"""
    from scipy.stats import betabinom
    x = np.arange(0, P)
    rows = []
    for i in range(1, M + 1):
        a, b = scaling * i, scaling * (M + 1 - i)
        rows.append(betabinom(P, a, b).pmf(x))
    return np.array(rows)


def ref_interpolated(w, h, round_mel_len_to=100, round_text_len_to=20):
    """data_function.py:56-65"""
    from scipy import ndimage
    rnd = lambda val, to: max(1, int(np.round((val + 1) / to))) * to   # noqa: E731
    bw, bh = rnd(w, round_mel_len_to), rnd(h, round_text_len_to)
    ret = ndimage.zoom(ref_exact(bw, bh).T, zoom=(w / bw, h / bh), order=1)
    assert ret.shape == (w, h), ret.shape
    return ret


def main():
    import torch
    import torch.nn as nn
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    import _refstub
    R = _load('attn_loss_ref', os.path.join(REPO, 'tests', 'attn_loss_ref.py'))
    A = _load('aligner_ref', os.path.join(REPO, 'tests', 'aligner_ref.py'))
    ref = _load('ref_attn_loss_function', os.path.join(_refstub.REF, 'models', 'fastpitch', 'fastpitch', 'attn_loss_function.py'))
    torch.set_grad_enabled(False)
    out = {}
    worst = 0.0
    for P, M in EXACT:
        out[f'exact_{P}_{M}'] = v = ref_exact(P, M)
        worst = max(worst, float(np.abs(R.exact_prior(P, M) - v).max()))
    for w, h in INTERP:
        out[f'interp_{w}_{h}'] = v = ref_interpolated(w, h)
        worst = max(worst, float(np.abs(R.interpolated_prior(w, h) - v).max()))
    print(f'priors: restatement against scipy, largest |difference| {worst:.2e}')

    rng = np.random.default_rng(0)
    logprob = (rng.standard_normal((4, 1, 48, 18)) * 3.0).astype(np.float32)
    out['attn_logprob'], out['in_lens'] = logprob, np.array(IN_LENS, np.int64)
    t_in = torch.tensor(IN_LENS)
    for tag, lens in (('', OUT_LENS), ('_infeasible', OUT_LENS_INFEASIBLE)):
        out['out_lens' + tag] = np.array(lens, np.int64)
        t_out = torch.tensor(lens)
        loss = ref.AttentionCTCLoss()
        out['ctc64' + tag] = np.float64(loss(torch.from_numpy(logprob).double(), t_in, t_out).item())
        out['ctc32' + tag] = np.float32(loss(torch.from_numpy(logprob).clone(), t_in, t_out).item())
        loss.CTCLoss = nn.CTCLoss(reduction='none')
        out['ctc_rows64' + tag] = rows = loss(torch.from_numpy(logprob).double(), t_in, t_out).numpy()
        mine = R.batch_forward_sum(logprob, IN_LENS, lens)
        print(f'forward-sum{tag}: rows {rows.tolist()}; restatement relative {max(abs(a - b) / b for a, b in zip(mine, rows) if np.isfinite(b)):.2e}; '
              f'scalar float64 {float(out["ctc64" + tag]):.12f} float32 {float(out["ctc32" + tag]):.8f}')

    g = np.load(os.path.join(REPO, 'tests', 'golden', 'aligner.npz'))
    for tag in ('', '_prior'):
        hard, soft = torch.from_numpy(g['attn_hard' + tag].astype(np.float32)), torch.from_numpy(g['attn_soft' + tag])
        out['bin64' + tag] = np.float64(ref.AttentionBinarizationLoss()(hard.double(), soft.double()).item())
        out['bin32' + tag] = np.float32(ref.AttentionBinarizationLoss()(hard, soft).item())
        print(f'binarization{tag}: float64 {float(out["bin64" + tag]):.15f} float32 {float(out["bin32" + tag]):.8f}')

    # swapped texts: rows 1 and 2 exchange their ids; the cost per token of both must rise (float64 restatement of the aligner, synthetic
    # weights as the generator of aligner.npz made them, the interpolated prior of each pairing's own lengths)
    import types
    pkg = types.ModuleType('ttsamd')
    pkg.__path__ = [os.path.join(REPO, 'tts-arabic-pytorch_amd', 'ttsamd')]
    sys.modules['ttsamd'] = pkg
    config = _load('ttsamd.config', os.path.join(pkg.__path__[0], 'config.py'))
    synth = _load('ttsamd.synth', os.path.join(pkg.__path__[0], 'synth.py'))
    cfg = dict(config.NET_CONFIG)
    sd = synth.fastpitch_state_dict(cfg, 0)
    sd.update(synth.fastpitch_aligner_state_dict(cfg, 0, float(g['gain'])))
    ids, in_lens, mel, mel_lens = g['ids'], g['in_lens'], g['mel'], g['mel_lens']

    def per_token(ids, in_lens):
        T, L = mel.shape[2], ids.shape[1]
        prior = np.zeros((len(ids), T, L), np.float32)
        for b in range(len(ids)):
            prior[b, :mel_lens[b], :in_lens[b]] = ref_interpolated(int(mel_lens[b]), int(in_lens[b]))
        _, lp = A.attention(sd, ids, mel, in_lens, prior, np.float64)
        return R.batch_forward_sum(lp.astype(np.float32), in_lens, mel_lens) / in_lens

    perm = np.array([0, 2, 1])
    matched, swapped = per_token(ids, in_lens), per_token(ids[perm], in_lens[perm])
    out['swap_perm'], out['swap_matched'], out['swap_swapped'] = perm, matched, swapped
    out['swap_margin'] = np.float64((swapped - matched)[1:].min())
    print(f'swapped texts: cost per token matched {matched.tolist()} swapped {swapped.tolist()}; margin {float(out["swap_margin"]):.3f}')
    assert float(out['swap_margin']) > 0.5
    path = os.path.join(REPO, 'tests', 'golden', 'attn_loss.npz')
    np.savez_compressed(path, **out)
    print(f'attn_loss: {os.path.getsize(path) / 1024:.1f} kB')


if __name__ == '__main__':
    main()

"""Generate tests/golden/hifigan_v3.npz with the REAL reference's HiFi-GAN V3 generator (ResBlock2).  Run manually where the
reference tree is readable (oracle/_refstub.py: TTS_REFERENCE):  python tools/gen_golden_hifigan_v3.py

Follows oracle/gen_golden.py's build_ref_hifigan recipe with HIFIGAN_V3_CONFIG written to a temporary json: the reference's
load_hifigan builds Generator(resblock "2") from synth.hifigan_state_dict(HIFIGAN_V3_CONFIG, seed=0).  The fixture holds the mels,
the reference's waves for T = 1 / 7 / 40 and the sha256 digest of the synthetic weights; no weights (the tests regenerate them).
"""
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'oracle'))
import gen_golden as gg  # noqa: E402  (loads our synth / config by path and installs the reference, as for the other goldens)

import torch  # noqa: E402


def main():
    cfg = gg.config.HIFIGAN_V3_CONFIG
    sd = gg.synth.hifigan_state_dict(cfg, 0)
    with tempfile.TemporaryDirectory() as td:
        cfg_path, sd_path = os.path.join(td, 'config.json'), os.path.join(td, 'g.pth')
        with open(cfg_path, 'w') as f:
            json.dump(cfg, f)
        torch.save({'generator': gg.t(sd)}, sd_path)
        with torch.enable_grad():        # remove_parametrizations leaves plain tensors under no_grad
            g = gg.load_hifigan(sd_path, cfg_path)
    assert type(g.resblocks[0]).__name__ == 'ResBlock2'
    rng = np.random.default_rng(17)
    out = {'digest': np.array(gg.sd_digest(sd))}
    with torch.no_grad():
        for T in (1, 7, 40):
            mel = torch.from_numpy((rng.standard_normal((80, T)) * 1.5 - 4.0).astype(np.float32))
            wave = g(mel)                                     # 2-D in, as networks.py:312,341
            out[f'mel_T{T}'] = mel.numpy()
            out[f'wave_T{T}'] = wave.numpy()
            print(T, tuple(wave.shape), 'abs max', float(wave.abs().max()))
    path = os.path.join(REPO, 'tests', 'golden', 'hifigan_v3.npz')
    np.savez_compressed(path, **out)
    print(f'hifigan_v3: {os.path.getsize(path) / 1024:.1f} kB')


if __name__ == '__main__':
    main()

"""Writes tests/golden/hifigan_state_dict_manifest.json and tests/golden/vocoder_synth.npz from the REFERENCE HiFi-GAN generator.

Runs only in the build container, where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.
The weights are not stored: they are ``synthetic_state_dict(manifest shapes, 1234)`` (the weight-normed keys as the reference's
``HiFiGANGenerator`` names them), loaded with ``load_state_dict(strict=True)``, folded by the reference's ``remove_weight_norm``.
The fixture holds the mels and the reference's fp32 waveforms; the fp64 forward of the same weights is only printed (the fp32
spread the parity bars are set against).

    python tests/golden/make_golden_vocoder.py
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = '/root/reference/src/daft_exprt/vocoder/hifigan.py'

from ubisoft_laforge_daft_exprt_amd.synth import synthetic_state_dict  # noqa: E402

SEED = 1234
LENGTHS = (1, 13, 40)
torch.set_num_threads(8)


def _load_reference():
    spec = importlib.util.spec_from_file_location('ref_hifigan', REF)     # the module imports only torch / numpy / stdlib
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = _load_reference()
    gen = ref.HiFiGANGenerator(ref.DEFAULT_CONFIG)
    shapes = {k: list(v.shape) for k, v in gen.state_dict().items()}
    with open(os.path.join(HERE, 'hifigan_state_dict_manifest.json'), 'w') as f:
        json.dump({'config': ref.DEFAULT_CONFIG, 'seed': SEED, 'keys': shapes}, f, indent=1)
    gen.load_state_dict(synthetic_state_dict({k: tuple(v) for k, v in shapes.items()}, SEED), strict=True)
    gen.remove_weight_norm()
    gen.eval()
    g = torch.Generator().manual_seed(SEED)
    rec = {'lengths': np.array(LENGTHS, dtype=np.int64)}
    for i, n in enumerate(LENGTHS):
        mel = (torch.randn(1, 80, n, generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0)     # log-mel-like range
        with torch.no_grad():
            wav = gen(mel).squeeze(0).squeeze(0)
            wav64 = gen.double()(mel.double()).squeeze(0).squeeze(0)
            gen.float()
        rec[f'mel{i}'] = mel[0].numpy()
        rec[f'wav{i}'] = wav.numpy()
        print(f'len {n}: std {wav.std().item():.3f} max {wav.abs().max().item():.3f} '
              f'f32 vs f64 max {(wav.double() - wav64).abs().max().item():.2e}')
    np.savez_compressed(os.path.join(HERE, 'vocoder_synth.npz'), **rec)


if __name__ == '__main__':
    main()

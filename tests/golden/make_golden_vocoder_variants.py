"""Writes tests/golden/hifigan_variants_manifest.json and tests/golden/vocoder_variants.npz from the REFERENCE HiFi-GAN generator built
with the V2 and V3 configurations (the published config_v2.json / config_v3.json in the key names of the reference's config dicts).

Runs only in the build container, where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.
As in make_golden_vocoder.py the weights are not stored: they are ``synthetic_state_dict(manifest shapes, 1234)``, loaded with
``load_state_dict(strict=True)`` and folded by the reference's ``remove_weight_norm``.  Per configuration and length the fixture holds the
mel, the reference's fp32 waveform, the max and mean of |fp32 - fp64| of the reference against itself (what the f32 parity bars are set
against) and the SNR in dB of the reference run wholly in bfloat16 (weights, activations, sums) against its fp64 run (what the bf16
bar is set against).

    python tests/golden/make_golden_vocoder_variants.py
"""
import copy
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
CONFIGS = {
    'v2': {'sampling_rate': 22050, 'upsample_rates': [8, 8, 2, 2], 'upsample_kernel_sizes': [16, 16, 4, 4], 'upsample_initial_channel': 128,
           'resblock': '1', 'resblock_kernel_sizes': [3, 7, 11], 'resblock_dilation_sizes': [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
           'model_in_dim': 80},
    'v3': {'sampling_rate': 22050, 'upsample_rates': [8, 8, 4], 'upsample_kernel_sizes': [16, 16, 8], 'upsample_initial_channel': 256,
           'resblock': '2', 'resblock_kernel_sizes': [3, 5, 7], 'resblock_dilation_sizes': [[1, 2], [2, 6], [3, 12]], 'model_in_dim': 80},
}
torch.set_num_threads(8)


def _load_reference():
    spec = importlib.util.spec_from_file_location('ref_hifigan', REF)     # the module imports only torch / numpy / stdlib
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _snr_db(x, ref):
    return float(10.0 * torch.log10(ref.pow(2).sum() / (x.double() - ref).pow(2).sum()))


def main():
    ref = _load_reference()
    manifest = {}
    rec = {'lengths': np.array(LENGTHS, dtype=np.int64)}
    for name, config in CONFIGS.items():
        gen = ref.HiFiGANGenerator(config)
        shapes = {k: list(v.shape) for k, v in gen.state_dict().items()}
        manifest[name] = {'config': config, 'seed': SEED, 'keys': shapes}
        gen.load_state_dict(synthetic_state_dict({k: tuple(v) for k, v in shapes.items()}, SEED), strict=True)
        gen.remove_weight_norm()
        gen.eval()
        g = torch.Generator().manual_seed(SEED)
        for i, n in enumerate(LENGTHS):
            mel = (torch.randn(1, 80, n, generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0)     # log-mel-like range, make_golden_vocoder.py's recipe
            with torch.no_grad():
                wav = gen(mel).squeeze(0).squeeze(0)
                wav64 = copy.deepcopy(gen).double()(mel.double()).squeeze(0).squeeze(0)
                wav16 = copy.deepcopy(gen).bfloat16()(mel.bfloat16()).squeeze(0).squeeze(0)
            diff = (wav.double() - wav64).abs()
            rec[f'{name}_mel{i}'] = mel[0].numpy()
            rec[f'{name}_wav{i}'] = wav.numpy()
            rec[f'{name}_f32_vs_f64_max{i}'] = np.float64(diff.max().item())
            rec[f'{name}_f32_vs_f64_mean{i}'] = np.float64(diff.mean().item())
            rec[f'{name}_bf16_snr_db{i}'] = np.float64(_snr_db(wav16, wav64))
            print(f'{name} len {n}: std {wav.std().item():.3f} max {wav.abs().max().item():.3f} f32 vs f64 max {diff.max().item():.2e} '
                  f'mean {diff.mean().item():.2e}; all-bfloat16 vs f64 {_snr_db(wav16, wav64):.1f} dB')
    with open(os.path.join(HERE, 'hifigan_variants_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1)
    np.savez_compressed(os.path.join(HERE, 'vocoder_variants.npz'), **rec)


if __name__ == '__main__':
    main()

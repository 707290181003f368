"""Fixture loading for the vocoder tests (data only; nothing here touches the reference tree)."""
import json
import os

import numpy as np

from ubisoft_laforge_daft_exprt_amd.synth import synthetic_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
VARIANTS = ('v2', 'v3')


def manifest(name='v1'):
    """Keys, shapes, seed and configuration of the reference generator's state dict: V1's in its own file, V2's and V3's in one."""
    with open(os.path.join(GOLDEN, 'hifigan_state_dict_manifest.json' if name == 'v1' else 'hifigan_variants_manifest.json')) as f:
        man = json.load(f)
    return man if name == 'v1' else man[name]


def state_dict(name='v1', seed=None):
    """The reference generator's weight-normed state dict of configuration ``name`` under synthetic_state_dict(manifest shapes, seed)."""
    man = manifest(name)
    return synthetic_state_dict({k: tuple(v) for k, v in man['keys'].items()}, man['seed'] if seed is None else seed)


def golden():
    z = np.load(os.path.join(GOLDEN, 'vocoder_synth.npz'))
    lengths = [int(v) for v in z['lengths']]
    return lengths, [z[f'mel{i}'] for i in range(len(lengths))], [z[f'wav{i}'] for i in range(len(lengths))]


def variant_golden(name):
    """-> lengths, mels, reference fp32 waveforms, and per length (max, mean) of the reference's |fp32 - fp64| and its all-bfloat16 SNR."""
    z = np.load(os.path.join(GOLDEN, 'vocoder_variants.npz'))
    lengths = [int(v) for v in z['lengths']]
    n = range(len(lengths))
    return dict(lengths=lengths, mels=[z[f'{name}_mel{i}'] for i in n], wavs=[z[f'{name}_wav{i}'] for i in n],
                f32_max=[float(z[f'{name}_f32_vs_f64_max{i}']) for i in n], f32_mean=[float(z[f'{name}_f32_vs_f64_mean{i}']) for i in n],
                bf16_snr_db=[float(z[f'{name}_bf16_snr_db{i}']) for i in n])

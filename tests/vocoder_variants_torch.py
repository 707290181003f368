"""Plain-torch restatement of the HiFi-GAN generator forward for any of the V1, V2, V3 configurations (ResBlock1 or ResBlock2), and the
fixture loading of the V2 / V3 tests.  For the tests only: the product package never imports it.  ``weights``: {layer: (folded weight,
bias)} as ``vocoder.fold_state_dict`` (or ``vocoder.pad_folded_weights``) returns it -- channel counts are read off the weights, so a
padded set runs as it is."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from ubisoft_laforge_daft_exprt_amd.synth import synthetic_state_dict

SLOPE = 0.1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAMES = ('v2', 'v3')


def to(weights, device, dtype=torch.float32):
    return {k: (w.to(device, dtype), b.to(device, dtype)) for k, (w, b) in weights.items()}


def resblock1(x, weights, name, k, dilations):
    for p, d in enumerate(dilations):
        w1, b1 = weights[f'{name}.convs1.{p}']
        w2, b2 = weights[f'{name}.convs2.{p}']
        t = F.conv1d(F.leaky_relu(x, SLOPE), w1, b1, padding=d * (k - 1) // 2, dilation=d)
        t = F.conv1d(F.leaky_relu(t, SLOPE), w2, b2, padding=(k - 1) // 2)
        x = t + x
    return x


def resblock2(x, weights, name, k, dilations):
    for p, d in enumerate(dilations):
        w, b = weights[f'{name}.convs.{p}']
        x = F.conv1d(F.leaky_relu(x, SLOPE), w, b, padding=d * (k - 1) // 2, dilation=d) + x
    return x


def generator(mel, weights, config):
    """mel (B, 80, T) -> waveform (B, 256 T) (tanh output, as the reference generator's forward then squeeze(1))."""
    block = resblock2 if str(config['resblock']) == '2' else resblock1
    ks, ds = config['resblock_kernel_sizes'], config['resblock_dilation_sizes']
    w, b = weights['conv_pre']
    x = F.conv1d(mel, w, b, padding=3)
    for i, (u, k) in enumerate(zip(config['upsample_rates'], config['upsample_kernel_sizes'])):
        w, b = weights[f'ups.{i}']
        x = F.conv_transpose1d(F.leaky_relu(x, SLOPE), w, b, stride=u, padding=(k - u) // 2)
        xs = None
        for j, kk in enumerate(ks):
            r = block(x, weights, f'resblocks.{i * len(ks) + j}', kk, ds[j])
            xs = r if xs is None else xs + r
        x = xs / len(ks)
    w, b = weights['conv_post']
    x = F.conv1d(F.leaky_relu(x, SLOPE), w, b, padding=3)
    return torch.tanh(x).squeeze(1)


# ---- fixtures (data only; nothing here touches the reference tree) ----------------------------------------------------------------
def manifest(name):
    with open(os.path.join(GOLDEN, 'hifigan_variants_manifest.json')) as f:
        return json.load(f)[name]


def state_dict(name):
    """The reference generator's weight-normed state dict of configuration ``name`` under synthetic_state_dict(manifest shapes, seed)."""
    man = manifest(name)
    return synthetic_state_dict({k: tuple(v) for k, v in man['keys'].items()}, man['seed'])


def golden(name):
    """-> lengths, mels, reference fp32 waveforms, and per length (max, mean) of the reference's |fp32 - fp64| and its all-bfloat16 SNR."""
    z = np.load(os.path.join(GOLDEN, 'vocoder_variants.npz'))
    lengths = [int(v) for v in z['lengths']]
    n = range(len(lengths))
    return dict(lengths=lengths, mels=[z[f'{name}_mel{i}'] for i in n], wavs=[z[f'{name}_wav{i}'] for i in n],
                f32_max=[float(z[f'{name}_f32_vs_f64_max{i}']) for i in n], f32_mean=[float(z[f'{name}_f32_vs_f64_mean{i}']) for i in n],
                bf16_snr_db=[float(z[f'{name}_bf16_snr_db{i}']) for i in n])

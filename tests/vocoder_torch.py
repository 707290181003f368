"""Plain-torch restatement of the HiFi-GAN generator forward (F.conv1d / F.conv_transpose1d) for any of the V1, V2, V3 configurations
(ResBlock1 or ResBlock2), for the tests and tools/bench_vocoder.py only: the product package never imports it.  ``weights``: {layer:
(folded weight, bias)} as ``vocoder.fold_state_dict`` (or ``vocoder.pad_folded_weights``) returns it -- channel counts are read off the
weights, so a padded set runs as it is."""
import torch
import torch.nn.functional as F

from ubisoft_laforge_daft_exprt_amd.vocoder import v1_config

SLOPE = 0.1


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


def generator(mel, weights, config=None):
    """mel (B, 80, T) -> waveform (B, 256 T) (tanh output, as the reference generator's forward then squeeze(1)); ``config``: None is V1."""
    config = v1_config() if config is None else config
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

"""Plain-torch restatement of the HiFi-GAN V1 generator forward (F.conv1d / F.conv_transpose1d), for the tests and
tools/bench_vocoder.py only: the product package never imports it.  ``weights``: {layer: (folded weight, bias)} as
``ubisoft_laforge_daft_exprt_amd.vocoder.fold_state_dict`` returns it."""
import torch
import torch.nn.functional as F

SLOPE = 0.1
UPS = ((8, 16), (8, 16), (2, 4), (2, 4))
KERNELS = (3, 7, 11)
DILATIONS = (1, 3, 5)


def to(weights, device, dtype=torch.float32):
    return {k: (w.to(device, dtype), b.to(device, dtype)) for k, (w, b) in weights.items()}


def resblock(x, weights, name, k):
    for p, d in enumerate(DILATIONS):
        w1, b1 = weights[f'{name}.convs1.{p}']
        w2, b2 = weights[f'{name}.convs2.{p}']
        t = F.conv1d(F.leaky_relu(x, SLOPE), w1, b1, padding=d * (k - 1) // 2, dilation=d)
        t = F.conv1d(F.leaky_relu(t, SLOPE), w2, b2, padding=(k - 1) // 2)
        x = t + x
    return x


def generator(mel, weights):
    """mel (B, 80, T) -> waveform (B, 256 T) (tanh output, as the reference generator's forward then squeeze(1))."""
    w, b = weights['conv_pre']
    x = F.conv1d(mel, w, b, padding=3)
    for i, (u, k) in enumerate(UPS):
        w, b = weights[f'ups.{i}']
        x = F.conv_transpose1d(F.leaky_relu(x, SLOPE), w, b, stride=u, padding=(k - u) // 2)
        xs = None
        for j, kk in enumerate(KERNELS):
            r = resblock(x, weights, f'resblocks.{i * len(KERNELS) + j}', kk)
            xs = r if xs is None else xs + r
        x = xs / len(KERNELS)
    w, b = weights['conv_post']
    x = F.conv1d(F.leaky_relu(x, SLOPE), w, b, padding=3)
    return torch.tanh(x).squeeze(1)

"""The mel front end restated in torch (any float dtype, differentiable) and the loading of the backward fixture, for the mel gradient
tests.  Nothing here reads the reference tree.

The fixture is tests/golden/mel_backward.npz (upstream gradients, loss targets, spreads, shares, loss values) plus one file per
variant and quantity for the per-sample arrays, mel_backward_{grad,loss}_{hifi,full}.npz: a single file would pass the 1 MiB limit on
committed files (12 bytes per sample, variant and quantity over 59 551 samples)."""
import os

import numpy as np
import torch

from tests.mel_helpers import FMAX, GOLDEN

CLIP = 1e-5
MARGIN = 1e-2                  # cells whose fp64 linear mel lies within this relative distance of the clip carry no upstream gradient
SCALE = 45.0
BIG = ('grad', 'loss')


def mel_torch(wav, fb, clip=CLIP):
    """wav (S,) and fb (n_mels, 513) tensors of one float dtype -> (log-mel (n_mels, T), linear mel before the clamp): reflect pad 384,
    torch.stft 1024 / 256 under the periodic Hann window, sqrt(re^2 + im^2 + 1e-9), fb @ mag, log(clamp(., clip))."""
    x = torch.nn.functional.pad(wav[None, None], (384, 384), mode='reflect')[0, 0]
    spec = torch.stft(x, 1024, hop_length=256, win_length=1024, window=torch.hann_window(1024, dtype=wav.dtype, device=wav.device),
                      center=False, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    lin = fb @ mag
    return torch.log(torch.clamp(lin, min=clip)), lin


def lin_fp64(wav, fb):
    with torch.no_grad():
        return mel_torch(torch.from_numpy(np.asarray(wav, dtype=np.float64)), torch.from_numpy(fb.astype(np.float64)))[1].numpy()


def near_clip(lin64, clip=CLIP, margin=MARGIN):
    """Cells where an fp32 and an fp64 clamp may disagree."""
    return np.abs(lin64 - clip) <= margin * clip


def grad_fp64(wav, fb, g):
    """d(sum g . mel) / d(wav) by autograd through the double restatement -> float64 (S,)."""
    x = torch.from_numpy(np.asarray(wav, dtype=np.float64)).requires_grad_(True)
    mel, _ = mel_torch(x, torch.from_numpy(fb.astype(np.float64)))
    (mel * torch.from_numpy(np.asarray(g, dtype=np.float64))).sum().backward()
    return x.grad.numpy()


def mel_fp64(wav, fb):
    with torch.no_grad():
        return mel_torch(torch.from_numpy(np.asarray(wav, dtype=np.float64)), torch.from_numpy(fb.astype(np.float64)))[0].numpy()


def loss_fp64(wav, fb, target):
    """The reference's F.l1_loss(target, mel(wav)) * 45 in double -> (value, gradient (S,))."""
    x = torch.from_numpy(np.asarray(wav, dtype=np.float64)).requires_grad_(True)
    mel, _ = mel_torch(x, torch.from_numpy(fb.astype(np.float64)))
    loss = torch.nn.functional.l1_loss(torch.from_numpy(np.asarray(target, dtype=np.float64)), mel) * SCALE
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def golden():
    """-> {name: {'wav', 'hifi' / 'full': {'g', 'share', 'd64', 'd32_ref', 'spread', 'target', 'loss_ref', 'loss64', 'dloss64',
    'dloss32_ref', 'loss_spread'}}}; wav from mel_frontend.npz."""
    from tests import mel_helpers as mh
    z = np.load(os.path.join(GOLDEN, 'mel_backward.npz'))
    big = {(k, v): np.load(os.path.join(GOLDEN, f'mel_backward_{k}_{v}.npz')) for k in BIG for v in FMAX}
    wavs = mh.golden()
    out = {}
    for name in [str(n) for n in z['names']]:
        d = {'wav': wavs[name]['wav']}
        for v in FMAX:
            e = {k: z[f'{name}/{v}/{k}'] for k in ('g', 'share', 'spread', 'target', 'loss_ref', 'loss64', 'loss_spread')}
            e.update({k: big['grad', v][f'{name}/{k}'] for k in ('d64', 'd32_ref')})
            e.update({k: big['loss', v][f'{name}/{k}'] for k in ('dloss64', 'dloss32_ref')})
            d[v] = e
        out[name] = d
    return out

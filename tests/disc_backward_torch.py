"""The linearised yardstick of the discriminators' backward.

|r - g| and leaky-ReLU are not smooth: an fp32 and a float64 forward disagree on a few signs near ties, and that, not rounding,
dominates any fp32-against-float64 comparison of gradients.  So the hard bar is set on a gradient LINEARISED at given feature maps
R_i, G_i: from the folded weights and the maps this module builds a surrogate that is linear in the waveform,

    sum_i c_i <sign(G_i - R_i), h_i> + c_gen <G_S - 1, h_S>,      h_i = conv_i(h_{i-1}) * where(G_i > 0, 1, 0.1)   (bias-free),

whose x-gradient is exactly the chain the kernels run, with every decision taken from the maps.  Any dtype; ``operand='bf16'`` rounds
the weights of the layers that run on the matrix pipes to bf16 and ``round_grad`` also rounds the gradient arriving at those layers'
outputs (what dx_disc_conv_dgrad stages), for the bf16 emulation.  Linearised at float64 maps it equals float64 autograd of
tests/disc_torch.py to 1e-9 relative.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import disc_helpers, disc_torch
from ubisoft_laforge_daft_exprt_amd import discriminators as disc

WEIGHT_ORDER = disc.GEN_LOSS_NAMES          # loss_gen_f, loss_fm_f, loss_gen_s, loss_fm_s


_NPZ = None


def fixture():
    """tests/golden/discriminators_backward.npz: the reference's own float64 and float32 autograd gradients (data only)."""
    global _NPZ
    if _NPZ is None:
        z = np.load(os.path.join(disc_helpers.GOLDEN, 'discriminators_backward.npz'))
        _NPZ = {k: z[k] for k in z.files}
    return _NPZ


def fixture_folded():
    """-> (mpd, msd) folded weights exactly as the fixture's run had them.  Weight norm folds to the same bits everywhere, but the
    spectral norm's sigma is an fp32 dot product whose last bit depends on the machine's summation order, and it divides every weight of
    its layer (a relative 6e-8 there moves the float64 gradient by 1e-10): the eight layers are re-divided by the recorded sigmas."""
    states = disc_helpers.state_dicts()
    mpd = {k: (w.reshape(w.shape[0], w.shape[1], w.shape[2]), b) for k, (w, b) in disc.fold_state_dict(states['mpd']).items()}
    msd = dict(disc.fold_state_dict(states['msd']))
    for key, sigma in fixture().items():
        if key.startswith('sigma/'):
            name = key[len('sigma/'):]
            msd[name] = (states['msd'][name + '.weight_orig'] / torch.tensor(float(sigma), dtype=torch.float32), msd[name][1])
    return mpd, msd


class _RoundGrad(torch.autograd.Function):
    """Identity forward; the gradient is rounded to bf16 on the way back."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _mask(g, dtype):
    one, slope = torch.ones((), dtype=dtype), torch.full((), disc.LRELU_SLOPE, dtype=torch.float64).to(dtype)
    return torch.where(g > 0, one, slope)       # the constants carry the working dtype (a Python scalar would make 0.1 a float32)


def _sub(x, weights, layers, maps_r, maps_g, two_d, w_gen, w_fm, dtype, operand, round_grad):
    """x: the folded (B, 1, H, p) or plain (B, 1, N) input in ``dtype`` -> the surrogate of one sub-discriminator (0-d)."""
    total = torch.zeros((), dtype=dtype)
    h = x
    n = len(layers)
    for i in range(n + 1):
        if i < n:
            _, _, _, s, g, pad = layers[i]
            w = weights[f'convs.{i}'][0].to(dtype)
        else:
            s, g, pad = 1, 1, 1
            w = weights['conv_post'][0].to(dtype)
        mfma = 0 < i < n
        if mfma and operand == 'bf16':
            w = w.to(torch.bfloat16).to(dtype)
        if two_d:
            z = F.conv2d(h, w[..., None], None, stride=(s, 1), padding=(pad, 0))
        else:
            z = F.conv1d(h, w, None, stride=s, padding=pad, groups=g)
        if mfma and round_grad:
            z = _RoundGrad.apply(z)
        r, gm = maps_r[i].to(dtype), maps_g[i].to(dtype)
        assert z.shape == gm.shape, (i, z.shape, gm.shape)
        h = z * _mask(gm, dtype) if i < n else z
        c = 2.0 / gm.numel()
        total = total + w_fm * c * (torch.sign(gm - r) * h).sum()
        if i == n:
            total = total + w_gen * c * ((gm - 1) * h).sum()
    return total


def surrogate(y_hat, folded_mpd, folded_msd, mpd_maps, msd_maps, weights, dtype=torch.float64, operand='f32', round_grad=False):
    """mpd_maps / msd_maps: (fmap_rs, fmap_gs) in the reference's shapes (the scores as the last map of each list), any float dtype.
    weights: four numbers in WEIGHT_ORDER."""
    wgf, wff, wgs, wfs = [float(w) for w in weights]
    x = y_hat.to(dtype)
    b, c, t = x.shape
    total = torch.zeros((), dtype=dtype)
    for i, p in enumerate(disc.PERIODS):
        xp = F.pad(x, (0, p - t % p), 'reflect') if t % p else x
        total = total + _sub(xp.view(b, c, -1, p), disc_torch.split(folded_mpd, i), disc.MPD_LAYERS, mpd_maps[0][i], mpd_maps[1][i], True,
                             wgf, wff, dtype, operand, round_grad)
    for i in range(3):
        if i:
            x = F.avg_pool1d(x, 4, 2, padding=2)
        total = total + _sub(x, disc_torch.split(folded_msd, i), disc.MSD_LAYERS, msd_maps[0][i], msd_maps[1][i], False,
                             wgs, wfs, dtype, operand, round_grad)
    return total


def linearised_grad(y_hat, folded_mpd, folded_msd, mpd_maps, msd_maps, weights, dtype=torch.float64, operand='f32', round_grad=False):
    """-> d surrogate / d y_hat, (B, 1, T) in ``dtype``."""
    x = y_hat.detach().to(dtype).requires_grad_(True)
    surrogate(x, folded_mpd, folded_msd, mpd_maps, msd_maps, weights, dtype, operand, round_grad).backward()
    return x.grad.detach()


def autograd_grad(y, y_hat, folded_mpd, folded_msd, weights, dtype=torch.float64):
    """True autograd of the restatement: d sum_i weights[i] loss_i / d y_hat -> ((B, 1, T) in ``dtype``, (mpd outputs, msd outputs))."""
    x = y_hat.detach().to(dtype).requires_grad_(True)
    mo = disc_torch.mpd(y.to(dtype), x, folded_mpd, dtype)
    so = disc_torch.msd(y.to(dtype), x, folded_msd, dtype)
    six = disc_torch.six_losses(mo, so)
    sum(float(w) * six[name] for w, name in zip(weights, WEIGHT_ORDER)).backward()
    return x.grad.detach(), (mo, so)

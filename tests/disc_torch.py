"""Plain-torch restatement of the HiFi-GAN discriminators' forward and losses from FOLDED weights: the full-tensor yardstick of the
GPU tests (F.conv2d / F.conv1d with groups, fp32 or fp64).  ``operand='bf16'`` rounds the folded weights and the input of every
layer that runs on the matrix pipes (all but the Cin = 1 first layer and the Cout = 1 last layer) to bf16, as the kernels' bf16
mode does; sums stay in ``dtype``."""
import torch
import torch.nn.functional as F

from ubisoft_laforge_daft_exprt_amd import discriminators as disc

SLOPE = disc.LRELU_SLOPE


def _r(t, operand):
    return t.to(torch.bfloat16).to(t.dtype) if operand == 'bf16' else t


def sub_p(x, weights, period, dtype=torch.float32, operand='f32'):
    """x (B, 1, T), weights {layer: (w (Cout, Cin, 5), bias)} -> (scores (B, n), [6 feature maps (B, C, H, p)])."""
    x = x.to(dtype)
    b, c, t = x.shape
    if t % period:
        x = F.pad(x, (0, period - t % period), 'reflect')
    x = x.view(b, c, -1, period)
    fmap = []
    for i, (_, _, _, s, _, pad) in enumerate(disc.MPD_LAYERS):
        w, bias = weights[f'convs.{i}']
        w, bias = w.to(dtype)[..., None], bias.to(dtype)
        if i:
            w, x = _r(w, operand), _r(x, operand)
        x = F.leaky_relu(F.conv2d(x, w, bias, stride=(s, 1), padding=(pad, 0)), SLOPE)
        fmap.append(x)
    w, bias = weights['conv_post']
    x = F.conv2d(x, w.to(dtype)[..., None], bias.to(dtype), padding=(1, 0))
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def sub_s(x, weights, dtype=torch.float32, operand='f32'):
    """x (B, 1, T) -> (scores (B, n), [8 feature maps (B, C, N)])."""
    x = x.to(dtype)
    fmap = []
    for i, (_, _, _, s, g, pad) in enumerate(disc.MSD_LAYERS):
        w, bias = weights[f'convs.{i}']
        w, bias = w.to(dtype), bias.to(dtype)
        if i:
            w, x = _r(w, operand), _r(x, operand)
        x = F.leaky_relu(F.conv1d(x, w, bias, stride=s, padding=pad, groups=g), SLOPE)
        fmap.append(x)
    w, bias = weights['conv_post']
    x = F.conv1d(x, w.to(dtype), bias.to(dtype), padding=1)
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def split(folded, i):
    """{'discriminators.i.convs.j': ...} -> {'convs.j': ...} of sub-discriminator i."""
    pre = f'discriminators.{i}.'
    return {k[len(pre):]: v for k, v in folded.items() if k.startswith(pre)}


def mpd(y, y_hat, folded, dtype=torch.float32, operand='f32'):
    out = [[], [], [], []]
    for i, p in enumerate(disc.PERIODS):
        w = split(folded, i)
        for x, k in ((y, 0), (y_hat, 1)):
            score, fmap = sub_p(x, w, p, dtype, operand)
            out[k].append(score)
            out[2 + k].append(fmap)
    return tuple(out)


def msd(y, y_hat, folded, dtype=torch.float32, operand='f32'):
    out = [[], [], [], []]
    y, y_hat = y.to(dtype), y_hat.to(dtype)
    for i in range(3):
        if i:
            y, y_hat = F.avg_pool1d(y, 4, 2, padding=2), F.avg_pool1d(y_hat, 4, 2, padding=2)
        w = split(folded, i)
        for x, k in ((y, 0), (y_hat, 1)):
            score, fmap = sub_s(x, w, dtype, operand)
            out[k].append(score)
            out[2 + k].append(fmap)
    return tuple(out)


def discriminator_loss(drs, dgs):
    loss, r_losses, g_losses = 0, [], []
    for dr, dg in zip(drs, dgs):
        r_loss, g_loss = torch.mean((1 - dr) ** 2), torch.mean(dg ** 2)
        loss = loss + (r_loss + g_loss)
        r_losses.append(r_loss)
        g_losses.append(g_loss)
    return loss, r_losses, g_losses


def generator_loss(dgs):
    loss, gen = 0, []
    for dg in dgs:
        term = torch.mean((1 - dg) ** 2)
        gen.append(term)
        loss = loss + term
    return loss, gen


def feature_loss(fmap_r, fmap_g):
    loss = 0
    for dr, dg in zip(fmap_r, fmap_g):
        for rl, gl in zip(dr, dg):
            loss = loss + torch.mean(torch.abs(rl - gl))
    return loss * 2


def six_losses(mpd_out, msd_out):
    """-> {name: 0-d tensor} in the names of HiFiGanDiscriminators.losses."""
    out = {}
    for tag, (drs, dgs, fr, fg) in (('f', mpd_out), ('s', msd_out)):
        out[f'loss_disc_{tag}'] = discriminator_loss(drs, dgs)[0]
        out[f'loss_gen_{tag}'] = generator_loss(dgs)[0]
        out[f'loss_fm_{tag}'] = feature_loss(fr, fg)
    return out

"""Fixture loading for the discriminator tests (data only; nothing here touches the reference tree)."""
import json
import os

import numpy as np
import torch

from ubisoft_laforge_daft_exprt_amd.synth import synthetic_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LENGTHS = (12, 257, 2048)
BATCH = 2
N_SAMPLES = 256


def manifest():
    with open(os.path.join(GOLDEN, 'discriminators_manifest.json')) as f:
        return json.load(f)


_NPZ = None


def fixture():
    global _NPZ
    if _NPZ is None:
        z = np.load(os.path.join(GOLDEN, 'discriminators.npz'))
        _NPZ = {k: z[k] for k in z.files}
    return _NPZ


def synthetic_states(man, overlay=None):
    """{'mpd': sd, 'msd': sd}: synthetic_state_dict over the manifest's shapes (the two discriminators seeded under their own names),
    the spectral-normed layers' ``weight_u`` / ``weight_v`` replaced by ``overlay`` (npz-style {'sn/<key>': array})."""
    out = {}
    for d in ('mpd', 'msd'):
        sd = synthetic_state_dict({f'{d}.{k}': tuple(v) for k, v in man[d].items()}, man['seed'])
        out[d] = {k[len(d) + 1:]: v for k, v in sd.items()}
    if overlay is not None:
        for k in out['msd']:
            if 'sn/' + k in overlay:
                out['msd'][k] = torch.from_numpy(np.asarray(overlay['sn/' + k])).clone()
    return out


def state_dicts():
    """The fixture's weights: synthetic, with the power-iterated spectral-norm vectors the fixture stores."""
    return synthetic_states(manifest(), fixture())


def sample_index(numel):
    """The fixed flat indices at which the fixture samples a feature map of ``numel`` elements."""
    return np.unique(np.linspace(0, numel - 1, min(N_SAMPLES, numel)).round().astype(np.int64))


def inputs(T):
    z = fixture()
    return torch.from_numpy(z[f'{T}/y']), torch.from_numpy(z[f'{T}/y_hat'])


def make_inputs(T, seed, batch=BATCH):
    """y: a band-limited tone mix plus noise, |y| <= 1; y_hat: y plus a perturbation.  (B, 1, T) fp32."""
    g = torch.Generator().manual_seed(seed * 100003 + T)
    t = torch.arange(T, dtype=torch.float64)[None] / 22050.0
    f = 80.0 + 3000.0 * torch.rand(batch, 6, generator=g, dtype=torch.float64)
    a = torch.rand(batch, 6, generator=g, dtype=torch.float64) / 6
    ph = 6.283185307179586 * torch.rand(batch, 6, generator=g, dtype=torch.float64)
    y = (a[:, :, None] * torch.sin(6.283185307179586 * f[:, :, None] * t[None] + ph[:, :, None])).sum(1)
    y = (y + 0.02 * torch.randn(batch, T, generator=g, dtype=torch.float64)).clamp(-1, 1)
    y_hat = (0.9 * y + 0.05 * torch.randn(batch, T, generator=g, dtype=torch.float64)).clamp(-1, 1)
    return y.float()[:, None].contiguous(), y_hat.float()[:, None].contiguous()


def fmap_keys(T):
    """[(discriminator, sub index, map index)] of the 54 feature maps, in the reference's order."""
    return [(d, i, j) for d, n_sub, n_map in (('mpd', 5, 6), ('msd', 3, 8)) for i in range(n_sub) for j in range(n_map)]

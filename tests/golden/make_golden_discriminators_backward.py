"""Writes tests/golden/discriminators_backward.npz from the REFERENCE HiFi-GAN discriminators, with autograd.

Runs only in the build container, where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.
Same weights as make_golden_discriminators.py (``synthetic_state_dict`` over the manifest's shapes, the spectral-norm vectors of
discriminators.npz overlaid), both norms removed, and the same inputs (read back from discriminators.npz).  Per length T in
(12, 257, 2048), batch 2, the reference modules and loss functions run in float64 and in float32 and autograd gives

    d (loss_gen_s + loss_gen_f + loss_fm_s + loss_fm_f) / d y_hat          (finetune_hifigan.py:229-242 without the mel term)

(the eight spectral-norm sigmas of this run are stored as ``sigma/<layer>``) stored as ``<T>/grad64`` (float64) and ``<T>/grad32`` (float32), with the four loss values in float64 (``<T>/losses64``, in the order
loss_gen_f, loss_fm_f, loss_gen_s, loss_fm_s).  Fixed zip timestamps: a rerun reproduces the file bit for bit.

    python tests/golden/make_golden_discriminators_backward.py
"""
import copy
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from tests import disc_helpers as dh  # noqa: E402
import make_golden_discriminators as fwd  # noqa: E402

torch.set_num_threads(8)


def main():
    ref = fwd._load_reference()
    models = {'mpd': ref.MultiPeriodDiscriminator(), 'msd': ref.MultiScaleDiscriminator()}
    states = dh.state_dicts()
    for d, m in models.items():
        m.load_state_dict(states[d], strict=True)
        m.eval()
        fwd._remove_norms(m)
    rec = {}
    # The spectral norm's sigma = u . (W v) is an fp32 sum whose last bit depends on the machine's summation order, and every weight of
    # the layer is divided by it: the eight sigmas used here are recorded, so that the float64 yardstick can be rebuilt bit for bit.
    removed = models['msd'].state_dict()
    for k in sorted(states['msd']):
        if k.startswith('discriminators.0.') and k.endswith('.weight_orig'):
            name = k[:-len('.weight_orig')]
            w, u, v = (states['msd'][f'{name}.{s}'] for s in ('weight_orig', 'weight_u', 'weight_v'))
            sigma = torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v))
            assert torch.equal(w / sigma, removed[name + '.weight']), name
            rec['sigma/' + name] = sigma.numpy().copy()
    models64 = {d: copy.deepcopy(m).double().eval() for d, m in models.items()}
    for T in dh.LENGTHS:
        y, y_hat = dh.inputs(T)
        for tag, mods, dtype in (('64', models64, torch.float64), ('32', models, torch.float32)):
            x = y_hat.to(dtype).requires_grad_(True)
            yy = y.to(dtype)
            _, dg_f, fr_f, fg_f = mods['mpd'](yy, x)
            _, dg_s, fr_s, fg_s = mods['msd'](yy, x)
            four = [ref.generator_loss(dg_f)[0], ref.feature_loss(fr_f, fg_f), ref.generator_loss(dg_s)[0], ref.feature_loss(fr_s, fg_s)]
            (four[2] + four[0] + four[3] + four[1]).backward()
            rec[f'{T}/grad{tag}'] = x.grad.numpy().copy()
            if tag == '64':
                rec[f'{T}/losses64'] = np.array([float(v.detach()) for v in four], dtype=np.float64)
        g64, g32 = rec[f'{T}/grad64'], rec[f'{T}/grad32'].astype(np.float64)
        print(f'T {T}: max|g64| {np.abs(g64).max():.4f}, f32 vs f64: max|d| {np.abs(g32 - g64).max():.3e}, '
              f'relative L2 {np.linalg.norm(g32 - g64) / np.linalg.norm(g64):.3e}')
    fwd._write_npz(os.path.join(HERE, 'discriminators_backward.npz'), rec)
    print('wrote', os.path.getsize(os.path.join(HERE, 'discriminators_backward.npz')), 'bytes')


if __name__ == '__main__':
    main()
